"""Layered min-sum on the per-layer HBM path against the flooding fp32 min-sum per-pass decoder, DVB-S2-structured
N = 64800 rate 1/2 (codes.dvbs2_structured, the 90 residue layers of codes.dvbs2_layers), one GPU, one process,
AWGN LLRs of the all-zero codeword resident in HBM, HIP events around decode only (DESIGN.md "Layered min-sum:
the per-layer path").

  python tools/bench_layered_dvbs2.py [--batch B] [--reps R] [--warmup W] [--points dB dB]
                                      [--out profiles/layered_dvbs2.json]

  (a)  layered per-layer, alpha = 0.8125, beta = 0, 25 iterations, no stop; with the algorithmic bytes per
       iteration, sum over checks of (8 d + 24) B, and the achieved TB/s against 8 TB/s
  (a1) the same with 1 iteration: the fixed part (staging in and out)
  (b)  flooding fp32 min-sum (engine.FloatDecoder, path="passes"), 50 iterations, no stop: the yardstick
  (c)  layered per-layer, i_max = 30, per-codeword stop, at two Eb/N0 points: mean iterations, frames in error;
       once per syndrome form (--forms; IBL_LAY_SYNDROME=packed|gather)
One JSON line per run on stdout; --out also writes them as one JSON document."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from informationbottleneckdecodingldpc_amd import codes, engine  # noqa: E402

HBM_TBS = 8.0


def awgn_llr(n, B, ebn0_dB, seed, dev, R=0.5):
    s2 = 1.0 / (2.0 * R * 10 ** (ebn0_dB / 10))
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    y = 1.0 + (s2 ** 0.5) * torch.randn((n, B), generator=g, device=dev, dtype=torch.float32)
    return (y * (2.0 / s2)).contiguous()


def timed(fn, reps, warmup, dev):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.current_stream(dev)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8192)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--alpha", type=float, default=0.8125)
    p.add_argument("--beta", type=float, default=0.0)
    p.add_argument("--points", type=float, nargs=2, default=(1.2, 1.5))
    p.add_argument("--forms", nargs="+", default=("packed", "gather"), choices=("packed", "gather"))
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    B = a.batch
    H = codes.dvbs2_structured(seed=3)
    layers = codes.dvbs2_layers(H)
    G = engine.Graph(H, dev)
    n_c, N = H.shape
    deg = np.diff(H.indptr).astype(np.int64)
    E = int(deg.sum())
    # per codeword and iteration: d rows of P read and written, three state words read and written
    bytes_iter = int((8 * deg + 24).sum())
    # per codeword and syndrome. gather: every edge's P value read once. packed: every P value read once, one
    # bit written, and one 64-bit word read per edge and 64 codewords
    bytes_syndrome = {"gather": 4 * E, "packed": 4 * N + N // 8 + E // 8}
    out = torch.empty((N, B), dtype=torch.float32, device=dev)
    iters = torch.zeros(B, dtype=torch.int32, device=dev)
    rows = []

    def report(name, ms, **kw):
        best = min(ms)
        r = {"run": name, "code": "dvbs2_structured_64800_r12", "N": N, "batch": B, "ms": [round(m, 3) for m in ms],
             "value": round(B / (best * 1e-3), 1), "unit": "codewords/s (best of reps)", **kw}
        rows.append(r)
        print(json.dumps(r), flush=True)
        return best

    llr = awgn_llr(N, B, a.points[0], 1, dev)
    lay1 = engine.LayeredDecoder(G, layers, 1, B, alpha=a.alpha, beta=a.beta, path="passes")
    fixed = report("a1_layered_passes_imax1_fixed",
                   timed(lambda: lay1.decode(llr, out=out, early_stop=False, iters=iters), a.reps, a.warmup, dev),
                   imax=1, early_stop=False, ebn0_db=a.points[0], launches=len(layers) + 2)
    del lay1
    lay25 = engine.LayeredDecoder(G, layers, 25, B, alpha=a.alpha, beta=a.beta, path="auto")
    assert lay25.path_in_use == "passes"
    ms = timed(lambda: lay25.decode(llr, out=out, early_stop=False, iters=iters), a.reps, a.warmup, dev)
    best = min(ms)
    # the 24 iterations beyond the imax = 1 run carry 24 iterations' bytes
    per_iter_ms = (best - fixed) / 24.0
    report("a_layered_passes_imax25_fixed", ms, imax=25, early_stop=False, ebn0_db=a.points[0], alpha=a.alpha,
           beta=a.beta, n_layers=len(layers), launches=25 * len(layers) + 2, tile=64, syndrome="none (no stop)",
           bytes_per_codeword_iteration=bytes_iter, bytes_per_iteration=bytes_iter * B,
           ms_per_iteration=round(per_iter_ms, 4),
           achieved_TBps=round(bytes_iter * B / (per_iter_ms * 1e-3) / 1e12, 3),
           fraction_of_8TBps=round(bytes_iter * B / (per_iter_ms * 1e-3) / 1e12 / HBM_TBS, 3),
           frame_errors=int((out < 0).any(dim=0).sum().item()))
    del lay25
    fl = engine.FloatDecoder(G, 0, 50, B, precision=torch.float32, path="passes")
    report("b_flooding_passes_imax50_fixed", timed(lambda: fl.decode(llr, out=out, early_stop=False), a.reps, a.warmup, dev),
           imax=50, early_stop=False, ebn0_db=a.points[0], fused=fl.fused,
           frame_errors=int((out < 0).any(dim=0).sum().item()))
    del fl
    # the syndrome's two forms (the library's default first; IBL_LAY_SYNDROME is read when a decoder is created)
    for form in a.forms:
        os.environ["IBL_LAY_SYNDROME"] = form
        lay30 = engine.LayeredDecoder(G, layers, 30, B, alpha=a.alpha, beta=a.beta, path="passes")
        per_syn = bytes_syndrome[form]
        for ebn0 in a.points:
            x = awgn_llr(N, B, ebn0, 2, dev)
            ms = timed(lambda: lay30.decode(x, out=out, early_stop=True, iters=iters), a.reps, a.warmup, dev)
            report(f"c_layered_passes_imax30_early_{ebn0}dB_{form}", ms, imax=30, early_stop=True, ebn0_db=ebn0,
                   alpha=a.alpha, beta=a.beta, syndrome=form, bytes_per_codeword_syndrome=per_syn,
                   launches=30 * len(layers) + (3 if form == "packed" else 2) * 29 + 2,
                   mean_iters=round(float(iters.float().mean().item()), 3),
                   iters_hist=torch.bincount(iters, minlength=31).tolist(),
                   frame_errors=int((out < 0).any(dim=0).sum().item()))
        del lay30
    os.environ.pop("IBL_LAY_SYNDROME", None)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/bench_layered_dvbs2.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
                       "warmup": a.warmup, "hbm_peak_TBps": HBM_TBS, "runs": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
