"""Layered BP with half-precision state against layered BP with fp32 state, one GPU, one process, AWGN LLRs of the
all-zero codeword resident in HBM, HIP events around whole decodes, 1 warm-up and at least 3 repetitions (DESIGN.md
"Layered BP: half-precision state").

  python tools/bench_layered_bp_half.py [--batch B] [--wlan-batch B] [--reps R] [--warmup W] [--points dB dB]
                                        [--ber-blocks N] [--out profiles/layered_bp_half.json]

DVB-S2-structured N = 64800 rate 1/2 (codes.dvbs2_structured(seed=3), the 90 layers of codes.dvbs2_layers), --batch
codewords, per-layer path, for each state (fp32, half):
  (a1) 1 iteration, no stop: the fixed part (staging in and out) and the first iteration
  (a)  25 iterations, no stop; with the algorithmic bytes of a later iteration per codeword, 16 E (fp32) or 8 E
       (half: P and R of every edge read and written, 2 bytes each), and the achieved TB/s against 8 TB/s
  (c)  i_max = 30, per-codeword stop, at two Eb/N0 points: mean iterations, frames in error
WLAN N = 1944 rate 1/2, --wlan-batch codewords, fused on-chip kernels, no stop:
  (w)  layered BP 25 iterations, fp32 state and half state, and (wf) flooding fp32 BP 50 iterations
One ber.run_ber point at 1.0 dB, seed 5, on the DVB-S2 code, one channel stream of --ber-blocks blocks:
  (r)  the layered BP class at 25 iterations with each state
One JSON line per run on stdout; --out also writes them as one JSON document.

  python tools/bench_layered_bp_half.py --measure-tolerance
needs no GPU: it re-measures the tolerance figures of tests/_layered_half_ref.py MEASURED["full_size"] (the numpy
emulation against 8 one-ulp draws on the N = 64800 input; minutes) and prints them."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from informationbottleneckdecodingldpc_amd import codes, engine  # noqa: E402

HBM_TBS = 8.0
STATES = (("fp32", torch.float32, 16), ("half", torch.float16, 8))   # name, state_dtype, bytes per edge and iteration


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


def measure_tolerance():
    from tests import _layered_half_ref as hr
    H, layers, llr = hr.full_size_input()
    a, r, differ, flips = hr.measure(H, layers, llr, hr.FULL_IMAX)
    print(json.dumps({"input": "full_size", "largest_abs": a, "largest_rel_above_1": r, "stops_differing": differ,
                      "hard_flips": flips, "recorded": list(hr.MEASURED["full_size"])}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8192)
    p.add_argument("--wlan-batch", type=int, default=262144)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--points", type=float, nargs=2, default=(1.2, 1.5))
    p.add_argument("--ber-blocks", type=int, default=4096)
    p.add_argument("--out", default=None)
    p.add_argument("--measure-tolerance", action="store_true")
    a = p.parse_args()
    if a.measure_tolerance:
        return measure_tolerance()
    if a.reps < 3:
        p.error("--reps must be at least 3")
    dev = torch.device("cuda", 0)
    rows = []

    def report(name, code, N, B, ms, **kw):
        best = min(ms)
        r = {"run": name, "code": code, "N": N, "batch": B, "ms": [round(m, 3) for m in ms],
             "value": round(B / (best * 1e-3), 1), "unit": "codewords/s (best of reps)", **kw}
        rows.append(r)
        print(json.dumps(r), flush=True)
        return r

    def frame_errors(out):
        return int((out < 0).any(dim=0).sum().item())

    def note_ratio(r, base, key):
        r[key] = round(r["value"] / base["value"], 3)
        print(json.dumps({"run": r["run"], key: r[key]}), flush=True)

    # ---- DVB-S2, per-layer path ----
    B = a.batch
    H = codes.dvbs2_structured(seed=3)
    layers = codes.dvbs2_layers(H)
    G = engine.Graph(H, dev)
    N = H.shape[1]
    E = int(H.nnz)
    code = "dvbs2_structured_64800_r12"
    out = torch.empty((N, B), dtype=torch.float32, device=dev)
    iters = torch.zeros(B, dtype=torch.int32, device=dev)
    llr = awgn_llr(N, B, a.points[0], 1, dev)
    xs = [awgn_llr(N, B, ebn0, 2, dev) for ebn0 in a.points]
    base = {}
    for state, dt, per_edge in STATES:
        free0 = torch.cuda.mem_get_info(dev)[0]
        d1 = engine.LayeredBPDecoder(G, layers, 1, B, path="passes", state_dtype=dt)
        handle_bytes = free0 - torch.cuda.mem_get_info(dev)[0]
        r1 = report(f"a1_layered_bp_{state}_passes_imax1_fixed", code, N, B,
                    timed(lambda: d1.decode(llr, out=out, early_stop=False, iters=iters), a.reps, a.warmup, dev),
                    state=state, imax=1, early_stop=False, ebn0_db=a.points[0], launches=len(layers) + 2,
                    handle_device_bytes=int(handle_bytes), handle_bytes_per_codeword=round(handle_bytes / B, 1))
        del d1
        d25 = engine.LayeredBPDecoder(G, layers, 25, B, path="auto", state_dtype=dt)
        assert d25.path_in_use == "passes" and d25.half == (state == "half")
        ms = timed(lambda: d25.decode(llr, out=out, early_stop=False, iters=iters), a.reps, a.warmup, dev)
        per_iter_ms = (min(ms) - min(r1["ms"])) / 24.0
        tbps = per_edge * E * B / (per_iter_ms * 1e-3) / 1e12
        r25 = report(f"a_layered_bp_{state}_passes_imax25_fixed", code, N, B, ms, state=state, imax=25,
                     early_stop=False, ebn0_db=a.points[0], n_layers=len(layers), launches=25 * len(layers) + 2, E=E,
                     bytes_per_codeword_iteration=per_edge * E, bytes_per_iteration=per_edge * E * B,
                     ms_per_iteration=round(per_iter_ms, 4), achieved_TBps=round(tbps, 3),
                     fraction_of_8TBps=round(tbps / HBM_TBS, 3), frame_errors=frame_errors(out))
        del d25
        d30 = engine.LayeredBPDecoder(G, layers, 30, B, path="passes", state_dtype=dt)
        r30 = []
        for ebn0, x in zip(a.points, xs):
            ms = timed(lambda: d30.decode(x, out=out, early_stop=True, iters=iters), a.reps, a.warmup, dev)
            r30.append(report(f"c_layered_bp_{state}_passes_imax30_early_{ebn0}dB", code, N, B, ms, state=state,
                              imax=30, early_stop=True, ebn0_db=ebn0, launches=30 * len(layers) + 3 * 29 + 2,
                              mean_iters=round(float(iters.float().mean().item()), 3),
                              iters_hist=torch.bincount(iters, minlength=31).tolist(), frame_errors=frame_errors(out)))
        del d30
        if state == "fp32":
            base = {"a": r25, "c": r30}
        else:
            note_ratio(r25, base["a"], "ratio_to_fp32_state")
            for r, b in zip(r30, base["c"]):
                note_ratio(r, b, "ratio_to_fp32_state")
    del out, iters, llr, xs

    # ---- one BER point, one channel stream ----
    from informationbottleneckdecodingldpc_amd import BeliefPropagation_Layered_Decoder_class_irregular as LayeredBP
    from informationbottleneckdecodingldpc_amd.ber import BERConfig, run_ber
    nb = a.ber_blocks
    mb = min(nb, 4096)
    cfg = BERConfig(EbN0_dB_start=1.0, EbN0_dB_max_value=1.0, min_errors=10 ** 12, msg_at_time=mb, max_blocks=nb, seed=5,
                    llr_dtype=torch.float32)
    for state, dt, _ in STATES:
        dec = LayeredBP(H, 25, 16, mb, layers=layers, path="passes", state_dtype=dt)
        res = run_ber(dec, cfg)
        r = {"run": f"r_ber_layered_bp_{state}_imax25", "code": code, "N": N, "state": state, "ebn0_db": 1.0, "seed": 5,
             "blocks": int(res.blocks[0]), "bit_errors": float(res.errors[0]), "ber": float(res.BER_vector[0]),
             "seconds": round(res.seconds[0], 3),
             "note": "seconds: decoding and channel generation of the point; the same Philox channel stream in both"}
        rows.append(r)
        print(json.dumps(r), flush=True)
        del dec
    del G
    torch.cuda.empty_cache()

    # ---- WLAN, fused kernels ----
    from informationbottleneckdecodingldpc_amd.codes import qc_layers, wlan_80211n
    Bw = a.wlan_batch
    Hw = wlan_80211n(81)
    lw = qc_layers(Hw, 81)
    Gw = engine.Graph(Hw, dev)
    Nw = Hw.shape[1]
    xw = awgn_llr(Nw, Bw, 1.5, 3, dev)
    ow = torch.empty((Nw, Bw), dtype=torch.float32, device=dev)
    iw = torch.zeros(Bw, dtype=torch.int32, device=dev)
    flw = engine.FloatDecoder(Gw, 1, 50, Bw, precision=torch.float32, path="fused")
    fw = report("wf_flooding_bp_fused_imax50_fixed", "wlan_1944_r12", Nw, Bw,
                timed(lambda: flw.decode(xw, out=ow, early_stop=False), a.reps, a.warmup, dev),
                imax=50, early_stop=False, ebn0_db=1.5, fused=flw.fused, frame_errors=frame_errors(ow))
    del flw
    w32 = None
    for state, dt, _ in STATES:
        bpw = engine.LayeredBPDecoder(Gw, lw, 25, Bw, path="fused", state_dtype=dt)
        cw, ngroups, grid = bpw.geometry(Bw)
        r = report(f"w_layered_bp_{state}_fused_imax25_fixed", "wlan_1944_r12", Nw, Bw,
                   timed(lambda: bpw.decode(xw, out=ow, early_stop=False, iters=iw), a.reps, a.warmup, dev),
                   state=state, imax=25, early_stop=False, ebn0_db=1.5, geometry=[cw, ngroups, grid],
                   waves_per_workgroup=cw, frame_errors=frame_errors(ow))
        note_ratio(r, fw, "ratio_to_flooding_bp_imax50")
        if w32 is None:
            w32 = r
        else:
            note_ratio(r, w32, "ratio_to_fp32_state")
        del bpw

    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/bench_layered_bp_half.py", "command": "python " + " ".join(sys.argv),
                       "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
                       "hbm_peak_TBps": HBM_TBS, "runs": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
