"""Fixed-point layered min-sum (engine.LayeredFixedDecoder) against the fp32 layered decoder on the same per-layer
HBM path, DVB-S2-structured N = 64800 rate 1/2 (codes.dvbs2_structured, the 90 residue layers of
codes.dvbs2_layers), one GPU, one process, AWGN LLRs of the all-zero codeword resident in HBM, HIP events around
decode only (DESIGN.md "Layered min-sum: fixed point"). Every ratio is taken against the fp32 decoder timed in the
same process, the two alternating repetition by repetition.

  python tools/bench_layered_fixed.py [--batch B] [--reps R] [--warmup W] [--points dB dB] [--ber-blocks K]
                                      [--out profiles/layered_fixed_dvbs2.json]

  (a)  fp32 per-layer, alpha = 0.8125, 25 iterations, no stop
  (b)  fixed point, alpha16 = 13, q_max 31, scale 2.0, 25 iterations, no stop, float32 input and int8 input;
       both with a 1-iteration run subtracted for the time of an iteration, the algorithmic bytes of an iteration
       (fp32: sum over checks of 8 d + 24; fixed: 2 d + 8) and the achieved TB/s against 8 TB/s
  (c)  both with the per-codeword stop, i_max = 30, at two Eb/N0 points
  (d)  ber.run_ber of the drop-in class, fp32 and fixed=True, at the two points on the same channel stream
One JSON line per run on stdout; --out also writes them as one JSON document."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import informationbottleneckdecodingldpc_amd as pkg  # noqa: E402
from informationbottleneckdecodingldpc_amd import codes, engine  # noqa: E402
from informationbottleneckdecodingldpc_amd.ber import BERConfig, run_ber  # noqa: E402

HBM_TBS = 8.0
ALPHA, ALPHA16, Q_MAX, SCALE = 0.8125, 13, 31, 2.0


def awgn_llr(n, B, ebn0_dB, seed, dev, R=0.5):
    s2 = 1.0 / (2.0 * R * 10 ** (ebn0_dB / 10))
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    y = 1.0 + (s2 ** 0.5) * torch.randn((n, B), generator=g, device=dev, dtype=torch.float32)
    return (y * (2.0 / s2)).contiguous()


def quantise(llr):
    return torch.clamp(torch.round(llr * SCALE), -127, 127).to(torch.int8)


def timed_alternating(fns, reps, warmup, dev):
    """fns: name -> callable. Every repetition runs each once, in turn. -> name -> [ms]."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    s = torch.cuda.current_stream(dev)
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return ms


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8192)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--points", type=float, nargs=2, default=(1.2, 1.5))
    p.add_argument("--ber-blocks", type=int, default=4096)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    B = a.batch
    H = codes.dvbs2_structured(seed=3)
    layers = codes.dvbs2_layers(H)
    G = engine.Graph(H, dev)
    n_c, N = H.shape
    deg = np.diff(H.indptr).astype(np.int64)
    # per codeword and iteration: d entries of P read and written, the check's state read and written
    bytes_iter = {"fp32": int((8 * deg + 24).sum()), "fixed": int((2 * deg + 8).sum())}
    ldb = {"fp32": -(-B // 64) * 64, "fixed": -(-B // 256) * 256}
    owned = {"fp32": ((4 * N + 12 * n_c) * ldb["fp32"] + 8 * N * -(-B // 64)) / B,
             "fixed": ((N + 4 * n_c) * ldb["fixed"] + 8 * N * -(-B // 64)) / B}
    rows = []

    def report(name, ms, **kw):
        best = min(ms)
        r = {"run": name, "code": "dvbs2_structured_64800_r12", "N": N, "batch": B, "ms": [round(m, 3) for m in ms],
             "value": round(B / (best * 1e-3), 1), "unit": "codewords/s (best of reps)", **kw}
        rows.append(r)
        print(json.dumps(r), flush=True)
        return r

    def make(kind, imax):
        if kind == "fp32":
            return engine.LayeredDecoder(G, layers, imax, B, alpha=ALPHA, beta=0.0, path="passes")
        return engine.LayeredFixedDecoder(G, layers, imax, B, alpha16=ALPHA16, beta_q=0, q_max=Q_MAX, scale=SCALE,
                                          path="passes")

    out32 = torch.empty((N, B), dtype=torch.float32, device=dev)
    out8 = torch.empty((N, B), dtype=torch.int8, device=dev)
    iters = torch.zeros(B, dtype=torch.int32, device=dev)
    llr = awgn_llr(N, B, a.points[0], 1, dev)
    llr8 = quantise(llr)

    def runs(imax, early, x32, x8):
        d32, dfx = make("fp32", imax), make("fixed", imax)
        fns = {"fp32": lambda: d32.decode(x32, out=out32, early_stop=early, iters=iters),
               "fixed_f32": lambda: dfx.decode(x32, out=out32, early_stop=early, iters=iters),
               "fixed_i8": lambda: dfx.decode(x8, out=out8, early_stop=early, iters=iters)}
        ms = timed_alternating(fns, a.reps, a.warmup, dev)
        stats = {}
        for k, fn in fns.items():   # once more, untimed, for what the decode left behind
            fn()
            o = out8 if k == "fixed_i8" else out32
            stats[k] = dict(mean_iters=round(float(iters.float().mean().item()), 3),
                            frame_errors=int((o < 0).any(dim=0).sum().item()))
        return ms, stats

    # (a), (b): 25 fixed iterations, and 1 iteration for the fixed part (staging in and out)
    ms1, _ = runs(1, False, llr, llr8)
    ms25, st25 = runs(25, False, llr, llr8)
    base = None
    for k in ("fp32", "fixed_f32", "fixed_i8"):
        kind = "fp32" if k == "fp32" else "fixed"
        per_iter_ms = (min(ms25[k]) - min(ms1[k])) / 24.0
        tbps = bytes_iter[kind] * B / (per_iter_ms * 1e-3) / 1e12
        r = report(("a_" if k == "fp32" else "b_") + k + "_imax25_no_stop", ms25[k], imax=25, early_stop=False,
                   ebn0_db=a.points[0], ms_imax1=[round(m, 3) for m in ms1[k]], ms_per_iteration=round(per_iter_ms, 4),
                   bytes_per_codeword_iteration=bytes_iter[kind], achieved_TBps=round(tbps, 3),
                   fraction_of_8TBps=round(tbps / HBM_TBS, 3), device_bytes_per_codeword=round(owned[kind], 1),
                   launches=25 * len(layers) + 2, **st25[k])
        if k == "fp32":
            base = r
        else:
            r["ratio_to_fp32"] = round(r["value"] / base["value"], 3)
            r["ratio_to_fp32_per_iteration"] = round(base["ms_per_iteration"] / r["ms_per_iteration"], 3)
            print(json.dumps({"run": r["run"], "ratio_to_fp32": r["ratio_to_fp32"],
                              "ratio_to_fp32_per_iteration": r["ratio_to_fp32_per_iteration"]}), flush=True)
    # (c): with the stop
    for ebn0 in a.points:
        x = awgn_llr(N, B, ebn0, 2, dev)
        ms, st = runs(30, True, x, quantise(x))
        for k in ("fp32", "fixed_f32", "fixed_i8"):
            r = report(f"c_{k}_imax30_early_{ebn0}dB", ms[k], imax=30, early_stop=True, ebn0_db=ebn0,
                       launches=30 * len(layers) + 3 * 29 + 2, **st[k])
            if k == "fp32":
                base = r
            else:
                r["ratio_to_fp32"] = round(r["value"] / base["value"], 3)
    # (d): BER of the drop-in class on one channel stream (recorded, not gated)
    ber = []
    for fixed in (False, True):
        dec = pkg.Min_Sum_Layered_Decoder_class_irregular(H, 30, 16, 1024, layers=layers, alpha=ALPHA, path="passes",
                                                          fixed=fixed, scale=SCALE, q_max=Q_MAX)
        for ebn0 in a.points:
            cfg = BERConfig(EbN0_dB_start=ebn0, EbN0_dB_max_value=ebn0, min_errors=10 ** 9, msg_at_time=1024,
                            max_blocks=a.ber_blocks, seed=11, llr_dtype=torch.float32)
            r = run_ber(dec, cfg)
            row = {"run": "d_ber_" + ("fixed" if fixed else "fp32"), "ebn0_db": ebn0, "imax": 30,
                   "blocks": int(r.blocks[0]), "bit_errors": float(r.errors[0]),
                   "ber": float(r.errors[0]) / (int(r.blocks[0]) * dec.data_len)}
            ber.append(row)
            print(json.dumps(row), flush=True)
        del dec
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/bench_layered_fixed.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
                       "warmup": a.warmup, "hbm_peak_TBps": HBM_TBS,
                       "parameters": {"alpha": ALPHA, "alpha16": ALPHA16, "beta_q": 0, "q_max": Q_MAX, "scale": SCALE},
                       "runs": rows, "ber": ber}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
