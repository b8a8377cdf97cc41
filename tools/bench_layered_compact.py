"""Compaction of the running codewords on the layered decoder's per-layer HBM path, off against on:
DVB-S2-structured N = 64800 rate 1/2 (codes.dvbs2_structured, the 90 residue layers of codes.dvbs2_layers), one GPU,
one process, AWGN LLRs of the all-zero codeword resident in HBM, HIP events around decode only (DESIGN.md "Layered
min-sum: compaction"). The code, batch and inputs are those of tools/bench_layered_dvbs2.py.

  python tools/bench_layered_compact.py [--batch B] [--reps R] [--warmup W] [--points dB dB]
                                        [--every 1 2 4] [--pct 12 25 50] [--out profiles/layered_compact_dvbs2.json]

  (y)  25 iterations, no stop, no compaction: the yardstick the stop has to beat
  (c)  i_max = 30, per-codeword stop, at each Eb/N0 point and for each (every, min_free_pct): one handle, compaction
       switched off and on repetition by repetition, so that both see the same machine; out and iters of the two
       are compared (equal, or the run says so); compactions and final extent from compaction_stats()
  (e)  the cost of the empty waves of freed tiles: one codeword that never converges among B - 1 that finish at
       once, iterations 17..30 in grids of ceil(B / 64) tiles against the same in grids of one tile
One JSON line per run on stdout; --out also writes them as one JSON document."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from informationbottleneckdecodingldpc_amd import codes, engine  # noqa: E402
from tools.bench_layered_dvbs2 import awgn_llr  # noqa: E402


def event_ms(fn, dev):
    s = torch.cuda.current_stream(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8192)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--alpha", type=float, default=0.8125)
    p.add_argument("--beta", type=float, default=0.0)
    p.add_argument("--imax", type=int, default=30)
    p.add_argument("--points", type=float, nargs="+", default=(1.2, 1.5))
    p.add_argument("--every", type=int, nargs="+", default=(1, 2, 4))
    p.add_argument("--pct", type=int, nargs="+", default=(12, 25, 50))
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    B = a.batch
    H = codes.dvbs2_structured(seed=3)
    layers = codes.dvbs2_layers(H)
    G = engine.Graph(H, dev)
    N = H.shape[1]
    out = torch.empty((N, B), dtype=torch.float32, device=dev)
    out_on = torch.empty((N, B), dtype=torch.float32, device=dev)
    iters = torch.zeros(B, dtype=torch.int32, device=dev)
    iters_on = torch.zeros(B, dtype=torch.int32, device=dev)
    rows = []

    def report(name, **kw):
        r = {"run": name, "code": "dvbs2_structured_64800_r12", "N": N, "batch": B, **kw}
        rows.append(r)
        print(json.dumps(r), flush=True)

    llr = awgn_llr(N, B, a.points[0], 1, dev)
    lay25 = engine.LayeredDecoder(G, layers, 25, B, alpha=a.alpha, beta=a.beta, path="passes")
    fn = lambda: lay25.decode(llr, out=out, early_stop=False, iters=iters)  # noqa: E731
    for _ in range(a.warmup):
        fn()
    ms = [event_ms(fn, dev) for _ in range(a.reps)]
    report("y_layered_passes_imax25_fixed", imax=25, early_stop=False, ebn0_db=a.points[0],
           ms=[round(m, 3) for m in ms], best_ms=round(min(ms), 3))
    del lay25

    dec = engine.LayeredDecoder(G, layers, a.imax, B, alpha=a.alpha, beta=a.beta, path="passes")
    for ebn0 in a.points:
        x = awgn_llr(N, B, ebn0, 2, dev)
        for every in a.every:
            for pct in a.pct:
                off, on = [], []
                for rep in range(a.warmup + a.reps):
                    dec.compaction = None
                    m0 = event_ms(lambda: dec.decode(x, out=out, early_stop=True, iters=iters), dev)
                    dec.compaction = (every, pct)
                    m1 = event_ms(lambda: dec.decode(x, out=out_on, early_stop=True, iters=iters_on), dev)
                    if rep >= a.warmup:
                        off.append(m0)
                        on.append(m1)
                n, extent = dec.compaction_stats()
                it = iters.cpu().numpy()
                attempts = sum(1 for k in range(1, a.imax) if k % every == 0)
                report(f"c_imax{a.imax}_early_{ebn0}dB_every{every}_pct{pct}", imax=a.imax, early_stop=True,
                       ebn0_db=ebn0, every=every, min_free_pct=pct, off_ms=[round(m, 3) for m in off],
                       on_ms=[round(m, 3) for m in on], off_best_ms=round(min(off), 3), on_best_ms=round(min(on), 3),
                       on_over_off=round(min(on) / min(off), 4), compactions=n, final_extent=extent,
                       attempts=attempts, launches_added=3 * attempts, mean_iters=round(float(it.mean()), 3),
                       unconverged=int((it == a.imax).sum()),
                       same_out=bool(torch.equal(out, out_on)), same_iters=bool(torch.equal(iters, iters_on)),
                       frame_errors=int((out_on < 0).any(dim=0).sum().item()))
    # (e) what the empty waves of freed tiles cost: one codeword that never converges (AWGN at -2 dB) among B - 1
    # noiseless ones is alone from iteration 2 on. Iterations 17..30 (the difference of an i_max 30 and an i_max 16
    # decode) then run one live tile in grids of ceil(B / 64) tiles; the same 64 leading columns decoded as a batch
    # of 64 run it in grids of one tile. The difference, per launch, is the cost of the waves that leave at once.
    xe = torch.full((N, B), 4.0, dtype=torch.float32, device=dev)
    xe[:, :1] = awgn_llr(N, 1, -2.0, 3, dev)
    xs = xe[:, :64].contiguous()
    outs = torch.empty((N, 64), dtype=torch.float32, device=dev)
    dec16 = engine.LayeredDecoder(G, layers, 16, B, alpha=a.alpha, beta=a.beta, path="passes", compact=(1, 1))
    dec.compaction = (1, 1)
    best_ms = {}
    for name, d, x_, o_ in (("wide30", dec, xe, out), ("wide16", dec16, xe, out), ("one30", dec, xs, outs),
                            ("one16", dec16, xs, outs)):
        f = lambda: d.decode(x_, out=o_, early_stop=True, iters=iters)  # noqa: E731
        for _ in range(a.warmup):
            f()
        best_ms[name] = min(event_ms(f, dev) for _ in range(a.reps))
        best_ms[name + "_stats"] = d.compaction_stats()
    launches = 14 * (len(layers) + 6)   # per iteration: the layers, pack, syndrome, finalise and one attempt of three
    wide, one = best_ms["wide30"] - best_ms["wide16"], best_ms["one30"] - best_ms["one16"]
    report("e_empty_waves", ebn0_db=None, tiles=(B + 63) // 64,
           **{k: (round(v, 3) if isinstance(v, float) else list(v)) for k, v in best_ms.items()},
           ms_14_iterations_wide_grid=round(wide, 3), ms_14_iterations_one_tile_grid=round(one, 3), launches=launches,
           us_per_launch_wide_grid=round(1e3 * wide / launches, 2),
           us_per_launch_one_tile_grid=round(1e3 * one / launches, 2),
           us_per_launch_empty_waves=round(1e3 * (wide - one) / launches, 2))
    del dec16
    best = {}
    for r in rows:
        if "every" in r:
            k = (r["every"], r["min_free_pct"])
            best[k] = best.get(k, 0.0) + r["on_best_ms"]
    if best:
        k = min(best, key=best.get)
        report("best_pair_by_summed_on_best_ms", every=k[0], min_free_pct=k[1], summed_ms=round(best[k], 3))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/bench_layered_compact.py", "device": torch.cuda.get_device_name(0),
                       "reps": a.reps, "warmup": a.warmup, "runs": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
