"""Flooding float decoders at the high DVB-S2 rates — check degrees 30 (rate 9/10) and 18 (rate 4/5), the wide check
kernels — against the rate-1/2 code (check degree 7, the narrow kernels) in the same process, and beside them the
wide layered fp32 decoder on the same inputs: the three DVB-S2-structured N = 64800 codes of
tools/bench_layered_wide.py, per-pass path, one GPU, AWGN LLRs of the all-zero codeword resident in HBM, HIP events
around decode only (DESIGN.md "Flooding float decoders: wide checks").

  python tools/bench_float_wide.py [--batch B] [--reps R] [--warmup W] [--out profiles/float_wide_dvbs2.json]

Arms per code, alternating within each repetition: fp32 min-sum, corrected min-sum (0.8125, 0) and BP at 50 iterations
without the stop, and the layered fp32 decoder (alpha 0.8125) at 25. Recorded per arm: codewords/s, edges/s (E x the
check passes run, imax - 1 for the flooding arms), the algorithmic bytes of a flooding iteration — a check pass reads
and writes E messages, a variable pass reads E messages and N channel values and writes E messages: (4 E + N) x 4 B,
the unfolded traffic — and the achieved TB/s against 8 TB/s, and each arm's edges/s against the rate-1/2 run of the
same arithmetic. One code's decoders are alive at a time (a flooding decoder owns four E x B inboxes). Then
wide_mixed (tests/_layered_wide.py) on the fused kernel against the per-pass path at B = 65,536, and B = 2 on the rate
9/10 code (the reference driver's batch, the small-batch kernels). One JSON line per run on stdout; --out also writes
them as one JSON document."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from informationbottleneckdecodingldpc_amd import _lib, codes, engine  # noqa: E402
from bench_layered_wide import ALPHA, CODES, HBM_TBS, N, awgn_llr  # noqa: E402

IMAX, LAY_IMAX = 50, 25
ARMS = {"minsum": dict(kind=0), "corrected": dict(kind=0, alpha=ALPHA, beta=0.0), "bp": dict(kind=1)}


def timed(fn, s):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def pass_times(dec, fn):
    """(check ms, check launches, variable ms, variable launches) of one decode (ibl_float_timing)."""
    L = _lib.load()
    _lib.check(L.ibl_float_timing(dec._h, 1), "ibl_float_timing")
    fn()
    torch.cuda.synchronize()
    cm, vm, cn, vn = ctypes.c_double(), ctypes.c_double(), ctypes.c_int32(), ctypes.c_int32()
    _lib.check(L.ibl_float_timing_read(dec._h, ctypes.byref(cm), ctypes.byref(cn), ctypes.byref(vm), ctypes.byref(vn)),
               "ibl_float_timing_read")
    _lib.check(L.ibl_float_timing(dec._h, 0), "ibl_float_timing")
    return cm.value, cn.value, vm.value, vn.value


def measure(fns, reps, warmup, s):
    """ms per repetition of every entry of fns, the entries alternating within a repetition."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(timed(fn, s))
    return ms


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8192)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev)
    B = a.batch
    rows = []
    out = torch.empty((N, B), dtype=torch.float32, device=dev)
    for name, (kw, d_main, q, ebn0) in CODES.items():
        H = codes.dvbs2_structured(**kw)
        layers = codes.dvbs2_layers(H)
        deg = np.diff(H.indptr).astype(np.int64)
        E, wide = int(deg.sum()), bool(deg.max() > 16)
        G = engine.Graph(H, dev)
        x = awgn_llr(N, B, ebn0, 1, dev, R=1.0 - H.shape[0] / N)
        decs = {arm: engine.FloatDecoder(G, kw2["kind"], IMAX, B, path="passes", alpha=kw2.get("alpha", 1.0),
                                         beta=kw2.get("beta", 0.0)) for arm, kw2 in ARMS.items()}
        lay = engine.LayeredDecoder(G, layers, LAY_IMAX, B, alpha=ALPHA, beta=0.0, path="passes")
        assert all(d.wide == wide and not d.fused for d in decs.values()) and lay.wide == wide
        fns = {arm: (lambda d=d: d.decode(x, out=out, early_stop=False)) for arm, d in decs.items()}
        fns["layered"] = lambda: lay.decode(x, out=out, early_stop=False)
        ms = measure(fns, a.reps, a.warmup, s)
        nbytes = (4 * E + N) * 4
        for arm, m in ms.items():
            passes = (LAY_IMAX if arm == "layered" else IMAX - 1)
            best = min(m) * 1e-3
            r = {"run": f"{name}_{arm}", "code": f"dvbs2_structured_64800_{name}", "check_degree": d_main, "edges": E,
                 "wide": wide, "ebn0_db": ebn0, "arm": arm, "batch": B, "imax": LAY_IMAX if arm == "layered" else IMAX,
                 "early_stop": False, "path": "passes", "ms": [round(t, 3) for t in m],
                 "value": round(B / best, 1), "unit": "codewords/s (best of reps)",
                 "edges_per_s": round(E * passes * B / best, 1)}
            if arm != "layered":
                tbps = nbytes * passes * B / best / 1e12
                r.update(folded=decs[arm].folded, bytes_per_codeword_iteration=nbytes, achieved_TBps=round(tbps, 3),
                         fraction_of_8TBps=round(tbps / HBM_TBS, 3))
                # one more decode with HIP events around every pass: the check pass alone (it reads and writes E
                # messages, 8 E bytes a codeword, besides what the fold adds)
                cn_ms, cn_n, vn_ms, vn_n = pass_times(decs[arm], fns[arm])
                cn_tbps = 8 * E * B / (cn_ms / cn_n * 1e-3) / 1e12
                r.update(check_pass_ms=round(cn_ms / cn_n, 4), variable_pass_ms=round(vn_ms / max(vn_n, 1), 4),
                         check_pass_TBps=round(cn_tbps, 3), check_pass_fraction_of_8TBps=round(cn_tbps / HBM_TBS, 3))
            rows.append(r)
        if name == "r910":   # the reference driver's batch on the small-batch kernels
            x2 = x[:, :2].contiguous()
            small = {arm: engine.FloatDecoder(G, ARMS[arm]["kind"], IMAX, 2, path="passes") for arm in ("minsum", "bp")}
            assert all(d.small_batch >= 2 and d.wide for d in small.values())
            ms2 = measure({arm: (lambda d=d: d.decode(x2, early_stop=False)) for arm, d in small.items()},
                          a.reps, a.warmup, s)
            for arm, m in ms2.items():
                rows.append({"run": f"r910_{arm}_B2", "code": "dvbs2_structured_64800_r910", "arm": arm, "batch": 2,
                             "imax": IMAX, "early_stop": False, "path": "small batch", "ms": [round(t, 3) for t in m],
                             "value": round(2 / (min(m) * 1e-3), 1), "unit": "codewords/s (best of reps)",
                             "us_per_iteration": round(min(m) * 1e3 / (IMAX - 1), 2)})
            del small
        del decs, lay, fns, G, x
        torch.cuda.empty_cache()
    by = {r["run"]: r for r in rows}
    for r in rows:
        if r["run"].split("_")[0] in CODES and "edges_per_s" in r:
            r["edges_per_s_vs_r12"] = round(r["edges_per_s"] / by["r12_" + r["arm"]]["edges_per_s"], 3)
    del out
    # wide_mixed: the fused kernel against the per-pass path
    from tests._layered_wide import code_rate, wide_mixed
    H = wide_mixed()[0]
    Bf = 65536
    G = engine.Graph(H, dev)
    x = awgn_llr(H.shape[1], Bf, 3.0, 1, dev, R=code_rate(H))
    decs = {path: engine.FloatDecoder(G, 0, IMAX, Bf, path=path) for path in ("fused", "passes")}
    assert decs["fused"].fused and not decs["passes"].fused and decs["fused"].wide
    ms = measure({path: (lambda d=d: d.decode(x, early_stop=False)) for path, d in decs.items()}, a.reps, a.warmup, s)
    for path, m in ms.items():
        rows.append({"run": f"wide_mixed_minsum_{path}", "code": "wide_mixed_124x400", "edges": int(H.nnz), "arm": "minsum",
                     "batch": Bf, "imax": IMAX, "early_stop": False, "path": path, "ms": [round(t, 3) for t in m],
                     "value": round(Bf / (min(m) * 1e-3), 1), "unit": "codewords/s (best of reps)",
                     "edges_per_s": round(int(H.nnz) * (IMAX - 1) * Bf / (min(m) * 1e-3), 1)})
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/bench_float_wide.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
                       "warmup": a.warmup, "hbm_peak_TBps": HBM_TBS, "runs": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
