"""Corrected (normalised / offset) flooding min-sum against plain min-sum on the same float decoder
(engine.FloatDecoder, alpha = 0.8125, beta = 0; DESIGN.md "Corrected min-sum"): one GPU, one process, channel LLRs
resident in HBM, HIP events around decode only, the two decoders alternating repetition by repetition, warm-ups
first, best of --reps with the spread reported.

  python tools/bench_minsum_corrected.py [--reps R] [--warmup W] [--out profiles/minsum_corrected.json]
                                         [--ber-out profiles/minsum_corrected_ber.json] [--skip-large]

  wlan1944_fused     WLAN N = 1944 fp32, fused kernel, B = 262144, i_max 50 (bench.py's C3), fixed iterations
  dvbs2_passes       DVB-S2-structured N = 64800 rate 1/2 fp32, per-pass kernels with the degree-2 fold, B = 8192,
                     i_max 50, fixed iterations
  *_small_B2 / _B32  the same two codes on the small-batch kernels (path="passes")
  --ber-out          ber.run_ber of the drop-in classes on one channel stream: plain min-sum, corrected min-sum and
                     BP, fp32, DVB-S2-structured rate 1/2, B = 8192, 4 batches a point, 1.0 .. 1.6 dB, i_max 50
One JSON line per run on stdout; --out / --ber-out also write them as JSON documents."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from informationbottleneckdecodingldpc_amd import codes, engine  # noqa: E402

ALPHA, BETA = 0.8125, 0.0


def awgn_llr(n, B, ebn0_dB, seed, dev, R=0.5):
    s2 = 1.0 / (2.0 * R * 10 ** (ebn0_dB / 10))
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    y = 1.0 + (s2 ** 0.5) * torch.randn((n, B), generator=g, device=dev, dtype=torch.float32)
    return (y * (2.0 / s2)).contiguous()


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


def compare(name, H, B, imax, path, ebn0, reps, warmup, dev, rows):
    G = engine.Graph(H, dev)
    N = H.shape[1]
    llr = awgn_llr(N, B, ebn0, 1, dev)
    out = torch.empty((N, B), dtype=torch.float32, device=dev)
    decs = {"plain": engine.FloatDecoder(G, 0, imax, B, path=path),
            "corrected": engine.FloatDecoder(G, 0, imax, B, path=path, alpha=ALPHA, beta=BETA)}
    fns = {k: (lambda d=d: d.decode(llr, out=out, early_stop=False)) for k, d in decs.items()}
    ms = timed_alternating(fns, reps, warmup, dev)
    d = decs["corrected"]
    kernels = "fused" if d.fused else ("small-batch" if B <= d.small_batch else "per-pass")
    res = {}
    for k in ("plain", "corrected"):
        best, worst = min(ms[k]), max(ms[k])
        fns[k]()
        torch.cuda.synchronize()
        res[k] = {"run": f"{name}_{k}", "N": N, "batch": B, "imax": imax, "kernels": kernels,
                  "folded": decs[k].folded if kernels == "per-pass" else 0, "ebn0_db": ebn0,
                  "ms": [round(m, 4) for m in ms[k]], "spread_pct": round(100.0 * (worst - best) / best, 2),
                  "value": round(B / (best * 1e-3), 1), "unit": "codewords/s (best of reps)",
                  "frame_errors": int((out < 0).any(dim=0).sum().item())}
    res["corrected"]["ratio_to_plain"] = round(res["corrected"]["value"] / res["plain"]["value"], 4)
    for k in ("plain", "corrected"):
        rows.append(res[k])
        print(json.dumps(res[k]), flush=True)


def ber_curves(H, dev, points, batch, batches, imax):
    from informationbottleneckdecodingldpc_amd.ber import BERConfig, run_ber
    from informationbottleneckdecodingldpc_amd.bp_decoder_irreg import BeliefPropagationDecoderClassIrregular
    from informationbottleneckdecodingldpc_amd.min_sum_decoder_irreg import Min_Sum_Decoder_class_irregular
    curves = {}
    for name, make in (("minsum", lambda: Min_Sum_Decoder_class_irregular(H, imax, 16, batch)),
                       ("minsum_corrected", lambda: Min_Sum_Decoder_class_irregular(H, imax, 16, batch, alpha=ALPHA,
                                                                                    beta=BETA)),
                       ("bp", lambda: BeliefPropagationDecoderClassIrregular(H, imax, 16, batch))):
        dec = make()
        c = {"ber": [], "errors": [], "blocks": [], "seconds": []}
        for ebn0 in points:
            cfg = BERConfig(EbN0_dB_start=ebn0, EbN0_dB_max_value=ebn0, min_errors=10 ** 12, msg_at_time=batch,
                            max_blocks=batches * batch, seed=7, llr_dtype=torch.float32)
            r = run_ber(dec, cfg)
            c["errors"].append(float(r.errors[0]))
            c["blocks"].append(int(r.blocks[0]))
            c["ber"].append(float(r.errors[0]) / (int(r.blocks[0]) * dec.data_len))
            c["seconds"].append(round(float(r.seconds[0]), 3))
            print(json.dumps({"run": "ber_" + name, "ebn0_db": ebn0, "ber": c["ber"][-1], "errors": c["errors"][-1],
                              "blocks": c["blocks"][-1]}), flush=True)
        curves[name] = c
        del dec
    return curves


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=None)
    p.add_argument("--ber-out", default=None)
    p.add_argument("--skip-large", action="store_true", help="small-batch rows only")
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    wlan, dvb = codes.wlan_80211n(81), codes.dvbs2_structured(seed=3)
    rows = []
    if not a.skip_large:
        compare("wlan1944_fused", wlan, 262144, 50, "fused", 2.0, a.reps, a.warmup, dev, rows)
        compare("dvbs2_passes", dvb, 8192, 50, "passes", 1.2, a.reps, a.warmup, dev, rows)
    for B in (2, 32):
        compare(f"wlan1944_small_B{B}", wlan, B, 50, "passes", 2.0, a.reps, a.warmup, dev, rows)
        compare(f"dvbs2_small_B{B}", dvb, B, 50, "passes", 1.2, a.reps, a.warmup, dev, rows)
    head = {"tool": "tools/bench_minsum_corrected.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
            "warmup": a.warmup, "parameters": {"alpha": ALPHA, "beta": BETA, "precision": "fp32"}}
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({**head, "runs": rows}, fh, indent=1)
            fh.write("\n")
    if a.ber_out:
        points = [1.0, 1.2, 1.4, 1.6]
        curves = ber_curves(dvb, dev, points, 8192, 4, 50)
        with open(a.ber_out, "w") as fh:
            json.dump({"tool": head["tool"], "device": head["device"], "parameters": head["parameters"],
                       "metric": "DVB-S2 BER on one channel stream (run_ber, device channel, Philox seed 7)",
                       "code": "DVB-S2-structured N=64800 R=1/2 (codes.dvbs2_structured(seed=3))",
                       "channel": "BPSK/AWGN, 16-cluster uniform quantiser (AD_max_abs 3), all-zero codeword",
                       "batch": 8192, "blocks_per_point": 4 * 8192, "imax": 50, "ebn0_db": points, "curves": curves},
                      fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
