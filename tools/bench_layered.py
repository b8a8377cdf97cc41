"""Layered min-sum throughput on one GPU against the flooding fp32 min-sum decoder (DESIGN.md "Layered min-sum"):
WLAN 802.11n N = 1944 (Z = 81), AWGN LLRs of the all-zero codeword resident in HBM, every run in this one
process, timed with HIP events on the decoder's stream.

  python tools/bench_layered.py [--batch B] [--reps R] [--warmup W] [--out profiles/layered_wlan.json]

  (a) layered, i_max = 5, no early stop
  (b) flooding fp32 min-sum (engine.FloatDecoder, its fused on-chip path), i_max = 10, no early stop — the
      yardstick: twice the iterations, the same passes over the edges
  (c) layered, i_max = 10, per-codeword early stop, at 2.0 and 2.5 dB, with the mean iteration count
One JSON line per run on stdout; --out also writes them as one JSON document."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from informationbottleneckdecodingldpc_amd import codes, engine  # noqa: E402


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
    p.add_argument("--batch", type=int, default=262144)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--alpha", type=float, default=1.0)
    p.add_argument("--beta", type=float, default=0.0)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    B = a.batch
    H = codes.wlan_80211n(81)
    layers = codes.qc_layers(H, 81)
    G = engine.Graph(H, dev)
    N = H.shape[1]
    out = torch.empty((N, B), dtype=torch.float32, device=dev)
    iters = torch.zeros(B, dtype=torch.int32, device=dev)
    rows = []

    def report(name, ms, **kw):
        best = min(ms)
        r = {"run": name, "code": "wlan1944", "N": N, "batch": B, "ms": [round(m, 3) for m in ms],
             "value": round(B / (best * 1e-3), 1), "unit": "codewords/s (best of reps)", **kw}
        rows.append(r)
        print(json.dumps(r), flush=True)

    llr15 = awgn_llr(N, B, 1.5, 1, dev)
    lay5 = engine.LayeredDecoder(G, layers, 5, B, alpha=a.alpha, beta=a.beta)
    cw, ngroups, grid = lay5.geometry(B)
    report("a_layered_imax5_fixed", timed(lambda: lay5.decode(llr15, out=out, early_stop=False, iters=iters),
                                          a.reps, a.warmup, dev),
           imax=5, early_stop=False, ebn0_db=1.5, alpha=a.alpha, beta=a.beta, cw_per_group=cw, ngroups=ngroups,
           grid=grid, frame_errors=int((out < 0).any(dim=0).sum().item()))
    del lay5
    # the fixed part of a layered decode (two transposes, the codeword's load, state reset and store): i_max = 1
    lay1 = engine.LayeredDecoder(G, layers, 1, B, alpha=a.alpha, beta=a.beta)
    report("a1_layered_imax1_fixed", timed(lambda: lay1.decode(llr15, out=out, early_stop=False, iters=iters),
                                           a.reps, a.warmup, dev), imax=1, early_stop=False, ebn0_db=1.5)
    del lay1
    fl = engine.FloatDecoder(G, 0, 10, B, precision=torch.float32)
    report("b_flooding_imax10_fixed", timed(lambda: fl.decode(llr15, out=out, early_stop=False), a.reps, a.warmup, dev),
           imax=10, early_stop=False, ebn0_db=1.5, fused=fl.fused,
           frame_errors=int((out < 0).any(dim=0).sum().item()))
    del fl
    lay10 = engine.LayeredDecoder(G, layers, 10, B, alpha=a.alpha, beta=a.beta)
    for ebn0 in (2.0, 2.5):
        llr = awgn_llr(N, B, ebn0, 2, dev)
        ms = timed(lambda: lay10.decode(llr, out=out, early_stop=True, iters=iters), a.reps, a.warmup, dev)
        report(f"c_layered_imax10_early_{ebn0}dB", ms, imax=10, early_stop=True, ebn0_db=ebn0, alpha=a.alpha,
               beta=a.beta, mean_iters=round(float(iters.float().mean().item()), 3),
               iters_hist=torch.bincount(iters, minlength=11).tolist(),
               frame_errors=int((out < 0).any(dim=0).sum().item()))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/bench_layered.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
                       "warmup": a.warmup, "runs": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
