"""Layered min-sum at the high DVB-S2 rates — check degrees 30 (rate 9/10) and 18 (rate 4/5), the wide kernels —
against the rate-1/2 code of tools/bench_layered_dvbs2.py (check degree 7, the narrow kernels) decoded in the same
process: DVB-S2-structured N = 64800 (codes.dvbs2_structured, the residue layers of codes.dvbs2_layers), per-layer
HBM path, one GPU, AWGN LLRs of the all-zero codeword resident in HBM, HIP events around decode only (DESIGN.md
"Layered min-sum: wide checks").

  python tools/bench_layered_wide.py [--batch B] [--reps R] [--warmup W] [--out profiles/layered_wide_dvbs2.json]

For each code, fp32 (alpha = 0.8125) and fixed point (alpha16 = 13, q_max 31, scale 2.0, int8 input): 25
iterations without the stop, and a 1-iteration run subtracted for the time of an iteration. Recorded: codewords/s,
edges/s (E x 24 iterations' worth over the 24 iterations' time), the algorithmic bytes of an iteration (fp32: sum
over checks of 8 d + 24, wide 8 d + 32; fixed: 2 d + 8, wide 2 d + 16) and the achieved TB/s, and each wide run's
edges/s against the rate-1/2 run of the same arithmetic. The codes' repetitions alternate, so that a drift of the
device falls on all alike. One JSON line per run on stdout; --out also writes them as one JSON document."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from informationbottleneckdecodingldpc_amd import codes, engine  # noqa: E402

HBM_TBS = 8.0
ALPHA, ALPHA16, Q_MAX, SCALE = 0.8125, 13, 31, 2.0
N = 64800
# name -> (dvbs2_structured keywords, the degree most checks have, q, Eb/N0 of the input)
CODES = {
    "r12": (dict(seed=3), 7, 90, 1.2),
    "r45": (dict(seed=5, n=N, k=51840, groups_hi=18, deg_hi=11, deg_lo=3), 18, 36, 3.0),
    "r910": (dict(seed=5, n=N, k=58320, groups_hi=18, deg_hi=4, deg_lo=3), 30, 18, 4.0),
}


def awgn_llr(n, B, ebn0_dB, seed, dev, R):
    s2 = 1.0 / (2.0 * R * 10 ** (ebn0_dB / 10))
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    y = 1.0 + (s2 ** 0.5) * torch.randn((n, B), generator=g, device=dev, dtype=torch.float32)
    return (y * (2.0 / s2)).contiguous()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8192)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    B = a.batch
    out32 = torch.empty((N, B), dtype=torch.float32, device=dev)
    out8 = torch.empty((N, B), dtype=torch.int8, device=dev)
    s = torch.cuda.current_stream(dev)
    info, fns = {}, {}
    for name, (kw, d_main, q, ebn0) in CODES.items():
        H = codes.dvbs2_structured(**kw)
        layers = codes.dvbs2_layers(H)
        deg = np.diff(H.indptr).astype(np.int64)
        assert int(np.bincount(deg).argmax()) == d_main == int(deg.max()) and len(layers) == q, (name, np.bincount(deg))
        wide = bool(deg.max() > 16)
        G = engine.Graph(H, dev)
        x = awgn_llr(N, B, ebn0, 1, dev, R=1.0 - H.shape[0] / N)
        x8 = torch.clamp(torch.round(x * SCALE), -127, 127).to(torch.int8)
        info[name] = dict(code=f"dvbs2_structured_64800_{name}", n_c=int(H.shape[0]), check_degree=d_main, q=q,
                          edges=int(deg.sum()), wide=wide, ebn0_db=ebn0,
                          bytes={"fp32": int((8 * deg + (32 if wide else 24)).sum()),
                                 "fixed": int((2 * deg + (16 if wide else 8)).sum())})
        for imax in (1, 25):
            d32 = engine.LayeredDecoder(G, layers, imax, B, alpha=ALPHA, beta=0.0, path="passes")
            dfx = engine.LayeredFixedDecoder(G, layers, imax, B, alpha16=ALPHA16, beta_q=0, q_max=Q_MAX, scale=SCALE,
                                             path="passes")
            assert d32.wide == dfx.wide == wide and d32.path_in_use == "passes"
            fns[(name, "fp32", imax)] = lambda d=d32, x=x: d.decode(x, out=out32, early_stop=False)
            fns[(name, "fixed", imax)] = lambda d=dfx, x=x8: d.decode(x, out=out8, early_stop=False)
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    rows = {}
    for name in CODES:
        for kind in ("fp32", "fixed"):
            m1, m25 = ms[(name, kind, 1)], ms[(name, kind, 25)]
            per_iter = [(b - a1) / 24.0 for a1, b in zip(m1, m25)]      # ms, repetition by repetition
            best = min(per_iter)
            i = info[name]
            eps = [i["edges"] * B / (t * 1e-3) for t in per_iter]
            tbps = i["bytes"][kind] * B / (best * 1e-3) / 1e12
            rows[(name, kind)] = r = {
                "run": f"{name}_{kind}_imax25_no_stop", **{k: v for k, v in i.items() if k != "bytes"},
                "arithmetic": kind, "batch": B, "imax": 25, "early_stop": False, "launches": 25 * i["q"] + 2,
                "ms": [round(m, 3) for m in m25], "ms_imax1": [round(m, 3) for m in m1],
                "ms_per_iteration": [round(t, 4) for t in per_iter],
                "value": round(B / (min(m25) * 1e-3), 1), "unit": "codewords/s (best of reps)",
                "edges_per_s": round(max(eps), 1), "edges_per_s_reps": [round(e, 1) for e in eps],
                "edges_per_s_spread": round((max(eps) - min(eps)) / max(eps), 4),
                "bytes_per_codeword_iteration": i["bytes"][kind], "achieved_TBps": round(tbps, 3),
                "fraction_of_8TBps": round(tbps / HBM_TBS, 3)}
    for (name, kind), r in rows.items():
        r["edges_per_s_vs_r12"] = round(r["edges_per_s"] / rows[("r12", kind)]["edges_per_s"], 3)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/bench_layered_wide.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
                       "warmup": a.warmup, "hbm_peak_TBps": HBM_TBS,
                       "parameters": {"alpha": ALPHA, "alpha16": ALPHA16, "beta_q": 0, "q_max": Q_MAX, "scale": SCALE},
                       "runs": list(rows.values())}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
