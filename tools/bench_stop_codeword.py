"""Per-codeword stop of the fused flooding decoders against fixed iterations and the batch stop (DESIGN.md
"Per-codeword stop on the fused flooding decoders"), one GPU, one process, inputs of the all-zero codeword resident
in HBM, HIP events around ``decode`` on the decoder's stream.

  python tools/bench_stop_codeword.py [--reps 3] [--warmup 1] [--scale 1.0] [--out profiles/stop_codeword.json]

Codes (i_max 50): the (3,6)-regular N = 8000 code with the IB decoder (DE tables designed at 1.3 dB), 65,536
codewords; WLAN 802.11n N = 1944 with fp32 min-sum, fp32 BP and corrected min-sum (0.8125, 0.15), 262,144 codewords.
Two Eb/N0 a code, around its waterfall. Arms, alternating repetition by repetition: "fixed" (early_stop=False),
"batch" (early_stop=True) and "codeword" (early_stop="codeword"). Per arm: best and spread of the repetitions in ms
and cw/s; for the per-codeword arm the mean and histogram of iters and the mean over the kernel's groups of the
group's last stop (what a workgroup actually runs). The arms' outputs are compared on the device: a column whose
iters is i_max - 1 equals the fixed arm's, and a column whose iters is the batch arm's count equals the batch arm's.
--scale shrinks the batches (smoke runs). One JSON line per run on stdout; --out writes them as one document."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from informationbottleneckdecodingldpc_amd import codes, engine, graph, tables  # noqa: E402
from informationbottleneckdecodingldpc_amd.channel import UniformQuantizer, sigma2_from_ebn0  # noqa: E402

IMAX = 50


def awgn_llr(n, B, ebn0_dB, seed, dev, R):
    s2 = sigma2_from_ebn0(ebn0_dB, R)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    y = 1.0 + (s2 ** 0.5) * torch.randn((n, B), generator=g, device=dev, dtype=torch.float32)
    return (y * (2.0 / s2)).contiguous()


def run_case(name, dec, x, group, reps, warmup, dev, extra):
    B = x.shape[1]
    out = {k: torch.empty_like(x) if x.dtype == torch.float32 else torch.empty(x.shape, dtype=torch.uint8, device=dev)
           for k in ("fixed", "batch", "codeword")}
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    its = torch.zeros(B, dtype=torch.int32, device=dev)
    arms = {"fixed": lambda: dec.decode(x, out=out["fixed"], early_stop=False),
            "batch": lambda: dec.decode(x, out=out["batch"], early_stop=True, iters=one),
            "codeword": lambda: dec.decode(x, out=out["codeword"], early_stop="codeword", iters=its)}
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    s = torch.cuda.current_stream(dev)
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    L = int(one.item())
    full = its == IMAX - 1
    same_fixed = bool((out["codeword"][:, full] == out["fixed"][:, full]).all().item())
    at_l = its == L
    same_batch = bool((out["codeword"][:, at_l] == out["batch"][:, at_l]).all().item())
    ng = B // group
    last = its[:ng * group].view(ng, group).max(dim=1).values.float().mean().item()
    rec = dict(case=name, batch=B, imax=IMAX, group=group, batch_stop=L, iters_mean=float(its.float().mean().item()),
               iters_hist=torch.bincount(its, minlength=IMAX).tolist(), group_last_stop_mean=last,
               columns_at_imax=int(full.sum().item()), equals_fixed_where_full=same_fixed,
               equals_batch_where_same_stop=same_batch, **extra)
    rec["arms"] = {k: dict(ms=v, best_ms=min(v), spread_ms=max(v) - min(v), cw_per_s=B / (min(v) * 1e-3))
                   for k, v in ms.items()}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--scale", type=float, default=1.0)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    runs = []
    # IB, the (3,6)-regular N = 8000 code
    g = graph.build_graph(codes.regular_code(8000, 3, 6, seed=0))
    G = engine.Graph(g, dev)
    B = max(64, int(65536 * a.scale)) // 8 * 8
    qd = UniformQuantizer(sigma2_from_ebn0(1.3, g.R_c), 16)
    rho, lam = tables.edge_degree_distributions(g)
    tb = tables.de_tables(qd.p_t_given_x0, qd.output_LLRs, rho, lam, IMAX)
    dec = engine.IBDecoder(G, tb, True, B, path="fused")
    for ebn0 in (1.4, 1.8):
        gen = torch.Generator(device=dev)
        gen.manual_seed(3)
        x = UniformQuantizer(sigma2_from_ebn0(ebn0, g.R_c), 16).sample_all_zero_device(g.n_v, B, dev, gen)
        runs.append(run_case("ib_reg36_8000", dec, x, dec.fused_ncw(B), a.reps, a.warmup, dev, dict(ebn0_dB=ebn0)))
    del dec, x
    # float, WLAN N = 1944
    g = graph.build_graph(codes.wlan_80211n(81))
    G = engine.Graph(g, dev)
    B = max(64, int(262144 * a.scale)) // 4 * 4
    for name, kind, kw in (("minsum_fp32_wlan1944", 0, {}), ("bp_fp32_wlan1944", 1, {}),
                           ("corrected_fp32_wlan1944", 0, dict(alpha=0.8125, beta=0.15))):
        dec = engine.FloatDecoder(G, kind, IMAX, B, precision=torch.float32, path="fused", **kw)
        for ebn0 in (2.0, 2.5):
            x = awgn_llr(g.n_v, B, ebn0, 5, dev, g.R_c)
            runs.append(run_case(name, dec, x, 4, a.reps, a.warmup, dev, dict(ebn0_dB=ebn0, **kw)))
        del dec, x
    if a.out:
        doc = dict(tool="tools/bench_stop_codeword.py", device=torch.cuda.get_device_name(0), reps=a.reps,
                   warmup=a.warmup, scale=a.scale, runs=runs)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
