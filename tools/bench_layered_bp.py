"""Layered BP against flooding fp32 BP and layered fp32 min-sum, one GPU, one process, AWGN LLRs of the all-zero
codeword resident in HBM, HIP events around whole decodes, warm-up and at least 3 repetitions (DESIGN.md "Layered
BP").

  python tools/bench_layered_bp.py [--batch B] [--wlan-batch B] [--reps R] [--warmup W] [--points dB dB]
                                   [--ber-blocks N] [--out profiles/layered_bp_dvbs2.json]

DVB-S2-structured N = 64800 rate 1/2 (codes.dvbs2_structured(seed=3), the 90 layers of codes.dvbs2_layers), --batch
codewords:
  (a1) layered BP, per-layer path, 1 iteration, no stop: the fixed part (staging in and out) and the first
       iteration, which moves 12 E bytes per codeword
  (a)  layered BP, per-layer path, 25 iterations, no stop; with the algorithmic bytes of a later iteration, 16 E per
       codeword (P and R of every edge read and written), and the achieved TB/s against 8 TB/s
  (b)  flooding fp32 BP (engine.FloatDecoder, kind 1, path="passes"), 50 iterations, no stop: the yardstick; every
       layered BP row carries its ratio to this one
  (m)  layered fp32 min-sum (alpha 0.8125), per-layer path, 25 iterations, no stop
  (c)  layered BP, i_max = 30, per-codeword stop, at two Eb/N0 points: mean iterations, frames in error
WLAN N = 1944 rate 1/2, --wlan-batch codewords, fused on-chip kernels:
  (w)  layered BP 25 iterations against (wf) flooding fp32 BP 50 iterations, no stop
One ber.run_ber point at 1.0 dB on the DVB-S2 code, one channel stream of --ber-blocks blocks:
  (r)  the layered BP class at 25 iterations against (rf) the flooding BP class at 50
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
    p.add_argument("--wlan-batch", type=int, default=262144)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--points", type=float, nargs=2, default=(1.2, 1.5))
    p.add_argument("--ber-blocks", type=int, default=4096)
    p.add_argument("--out", default=None)
    a = p.parse_args()
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

    # ---- DVB-S2 ----
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

    fl = engine.FloatDecoder(G, 1, 50, B, precision=torch.float32, path="passes")
    flood = report("b_flooding_bp_passes_imax50_fixed", code, N, B,
                   timed(lambda: fl.decode(llr, out=out, early_stop=False), a.reps, a.warmup, dev),
                   imax=50, early_stop=False, ebn0_db=a.points[0], fused=fl.fused, frame_errors=frame_errors(out))
    del fl

    def ratio(r):
        return round(r["value"] / flood["value"], 3)

    bp1 = engine.LayeredBPDecoder(G, layers, 1, B, path="passes")
    r1 = report("a1_layered_bp_passes_imax1_fixed", code, N, B,
                timed(lambda: bp1.decode(llr, out=out, early_stop=False, iters=iters), a.reps, a.warmup, dev),
                imax=1, early_stop=False, ebn0_db=a.points[0], launches=len(layers) + 2,
                bytes_per_codeword_first_iteration=12 * E)
    del bp1
    bp25 = engine.LayeredBPDecoder(G, layers, 25, B, path="auto")
    assert bp25.path_in_use == "passes"
    ms = timed(lambda: bp25.decode(llr, out=out, early_stop=False, iters=iters), a.reps, a.warmup, dev)
    per_iter_ms = (min(ms) - min(r1["ms"])) / 24.0
    r25 = report("a_layered_bp_passes_imax25_fixed", code, N, B, ms, imax=25, early_stop=False, ebn0_db=a.points[0],
                 n_layers=len(layers), launches=25 * len(layers) + 2, E=E, bytes_per_codeword_iteration=16 * E,
                 bytes_per_iteration=16 * E * B, ms_per_iteration=round(per_iter_ms, 4),
                 achieved_TBps=round(16 * E * B / (per_iter_ms * 1e-3) / 1e12, 3),
                 fraction_of_8TBps=round(16 * E * B / (per_iter_ms * 1e-3) / 1e12 / HBM_TBS, 3),
                 boxplus_per_codeword_iteration=int((3 * (np.diff(H.indptr) - 2)).sum()),
                 frame_errors=frame_errors(out))
    r25["ratio_to_flooding_bp_imax50"] = ratio(r25)
    print(json.dumps({"run": r25["run"], "ratio_to_flooding_bp_imax50": r25["ratio_to_flooding_bp_imax50"]}), flush=True)
    del bp25

    ms25 = engine.LayeredDecoder(G, layers, 25, B, alpha=0.8125, beta=0.0, path="passes")
    report("m_layered_minsum_passes_imax25_fixed", code, N, B,
           timed(lambda: ms25.decode(llr, out=out, early_stop=False, iters=iters), a.reps, a.warmup, dev),
           imax=25, early_stop=False, ebn0_db=a.points[0], alpha=0.8125, beta=0.0, frame_errors=frame_errors(out))
    del ms25

    bp30 = engine.LayeredBPDecoder(G, layers, 30, B, path="passes")
    for ebn0 in a.points:
        x = awgn_llr(N, B, ebn0, 2, dev)
        ms = timed(lambda: bp30.decode(x, out=out, early_stop=True, iters=iters), a.reps, a.warmup, dev)
        r = report(f"c_layered_bp_passes_imax30_early_{ebn0}dB", code, N, B, ms, imax=30, early_stop=True,
                   ebn0_db=ebn0, launches=30 * len(layers) + 3 * 29 + 2,
                   mean_iters=round(float(iters.float().mean().item()), 3),
                   iters_hist=torch.bincount(iters, minlength=31).tolist(), frame_errors=frame_errors(out))
        r["ratio_to_flooding_bp_imax50"] = ratio(r)
        del x
    del bp30, out, iters, llr

    # ---- one BER point, one channel stream ----
    from informationbottleneckdecodingldpc_amd import BeliefPropagation_Layered_Decoder_class_irregular as LayeredBP
    from informationbottleneckdecodingldpc_amd.ber import BERConfig, run_ber
    from informationbottleneckdecodingldpc_amd.bp_decoder_irreg import BeliefPropagationDecoderClassIrregular
    nb = a.ber_blocks
    mb = min(nb, 4096)
    cfg = BERConfig(EbN0_dB_start=1.0, EbN0_dB_max_value=1.0, min_errors=10 ** 12, msg_at_time=mb, max_blocks=nb, seed=5,
                    llr_dtype=torch.float32)
    for name, dec in (("r_ber_layered_bp_imax25", LayeredBP(H, 25, 16, mb, layers=layers, path="passes")),
                      ("rf_ber_flooding_bp_imax50", BeliefPropagationDecoderClassIrregular(H, 50, 16, mb))):
        res = run_ber(dec, cfg)
        r = {"run": name, "code": code, "N": N, "ebn0_db": 1.0, "seed": 5, "blocks": int(res.blocks[0]),
             "bit_errors": float(res.errors[0]), "ber": float(res.BER_vector[0]), "seconds": round(res.seconds[0], 3),
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
    bpw = engine.LayeredBPDecoder(Gw, lw, 25, Bw, path="fused")
    r = report("w_layered_bp_fused_imax25_fixed", "wlan_1944_r12", Nw, Bw,
               timed(lambda: bpw.decode(xw, out=ow, early_stop=False, iters=iw), a.reps, a.warmup, dev),
               imax=25, early_stop=False, ebn0_db=1.5, geometry=list(bpw.geometry(Bw)), frame_errors=frame_errors(ow))
    r["ratio_to_flooding_bp_imax50"] = round(r["value"] / fw["value"], 3)
    print(json.dumps({"run": r["run"], "ratio_to_flooding_bp_imax50": r["ratio_to_flooding_bp_imax50"]}), flush=True)
    del bpw

    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/bench_layered_bp.py", "command": "python " + " ".join(sys.argv),
                       "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
                       "hbm_peak_TBps": HBM_TBS, "runs": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
