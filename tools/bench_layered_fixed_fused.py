"""The fixed-point fused layered kernel (engine.LayeredFixedDecoder path="onchip") beside the fp32 fused decoder and
the fixed-point per-layer decoder: one GPU, one process, AWGN LLRs of the all-zero codeword resident in HBM, HIP events
around decode only (DESIGN.md "Layered min-sum: fixed point, fused"). The arms of a setting alternate repetition by
repetition; 2 warm-ups, best of 5, the spread recorded. Not part of bench.py; there is no pass bar.

  python tools/bench_layered_fixed_fused.py [--batch B] [--reps R] [--warmup W] [--caps K ...] [--quick]
                                            [--out profiles/layered_fixed_fused.json]

  (a)  WLAN N = 1944 (Z = 81, its 12 block rows as layers), B = 262,144, alpha 0.8125 / alpha16 13, q_max 31,
       scale 2.0. Arms: fp32 fused; fixed point per layer; on chip with float32 I/O; on chip with int8 I/O; on chip
       with the workgroup capped at 16, 8, 2 and 1 codewords instead of 4 (--caps; IBL_LAYFIX_FUSED_CW at create).
       5 fixed iterations and 1 (the fixed part and the time of an iteration), and the stop at i_max 10 at 2.0 and
       2.5 dB.
  (b)  the same decoders at B = 8 and B = 64, i_max 10 with the stop: the launch-count case (20 decodes a window).
  (c)  the DVB-S2-structured N = 16200 code the fp32 fused kernel cannot hold, B = 8192: on chip against per layer.
Every on-chip arm's output and iteration counts are compared with the per-layer decoder's (recorded as `equal`).
One JSON line per arm on stdout; --out also writes them as one JSON document."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from informationbottleneckdecodingldpc_amd import codes, engine  # noqa: E402

ALPHA, ALPHA16, Q_MAX, SCALE = 0.8125, 13, 31, 2.0
CW_ENV = "IBL_LAYFIX_FUSED_CW"


def awgn_llr(n, B, ebn0_dB, seed, dev, R):
    s2 = 1.0 / (2.0 * R * 10 ** (ebn0_dB / 10))
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    y = 1.0 + (s2 ** 0.5) * torch.randn((n, B), generator=g, device=dev, dtype=torch.float32)
    return (y * (2.0 / s2)).contiguous()


def quantise(llr):
    return torch.clamp(torch.round(llr * SCALE), -127, 127).to(torch.int8)


def timed_alternating(fns, reps, warmup, inner, dev):
    """fns: name -> callable. Every repetition runs each arm once (`inner` decodes in one window), in turn.
    -> name -> [ms per decode]."""
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
            for _ in range(inner):
                fn()
            e1.record(s)
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / inner)
    return ms


class Bench:
    def __init__(self, a, dev):
        self.a, self.dev, self.rows = a, dev, []

    def make(self, G, layers, arm, imax, B):
        if arm == "fp32_fused":
            return engine.LayeredDecoder(G, layers, imax, B, alpha=ALPHA, beta=0.0, path="fused")
        kw = dict(alpha16=ALPHA16, beta_q=0, q_max=Q_MAX, scale=SCALE)
        if arm == "fixed_per_layer":
            return engine.LayeredFixedDecoder(G, layers, imax, B, path="passes", **kw)
        cap = arm[len("onchip_cw"):] if arm.startswith("onchip_cw") else None   # read by the library at create
        old = os.environ.pop(CW_ENV, None)
        try:
            if cap:
                os.environ[CW_ENV] = cap
            return engine.LayeredFixedDecoder(G, layers, imax, B, path="onchip", **kw)
        finally:
            os.environ.pop(CW_ENV, None)
            if old is not None:
                os.environ[CW_ENV] = old

    def setting(self, section, code, G, layers, arms, imax, early, ebn0, x32, inner=1):
        """One setting: every arm of `arms` (name -> (decoder kind, int8 I/O)) on the input x32."""
        N, B = x32.shape
        x8 = quantise(x32)
        out32 = torch.empty((N, B), dtype=torch.float32, device=self.dev)
        out8 = torch.empty((N, B), dtype=torch.int8, device=self.dev)
        iters = torch.zeros(B, dtype=torch.int32, device=self.dev)
        decs = {name: self.make(G, layers, kind, imax, B) for name, (kind, _) in arms.items()}

        def call(name):
            i8 = arms[name][1]
            return lambda: decs[name].decode(x8 if i8 else x32, out=out8 if i8 else out32, early_stop=early,
                                             iters=iters)

        fns = {name: call(name) for name in arms}
        ms = timed_alternating(fns, self.a.reps, self.a.warmup, inner, self.dev)
        # once more, untimed: what each arm left behind, and the on-chip arms against the per-layer decoder
        left = {}
        for name, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            o = out8 if arms[name][1] else out32
            # int8 output in LLR units (SCALE is a power of two: the division is exact, as the decoder's own)
            keep = name == "fixed_per_layer" or arms[name][0].startswith("onchip")
            left[name] = ((o.float() / SCALE if arms[name][1] else o.clone()) if keep else None,
                          iters.clone(), int((o < 0).any(dim=0).sum().item()))
        n_layers = len(layers)
        for name, (kind, i8) in arms.items():
            best, med = min(ms[name]), statistics.median(ms[name])
            r = {"section": section, "code": code, "N": N, "batch": B, "imax": imax, "early_stop": early,
                 "ebn0_db": ebn0, "arm": name, "io": "int8" if i8 else "float32", "decodes_per_window": inner,
                 "ms": [round(m, 4) for m in ms[name]], "best_ms": round(best, 4), "median_ms": round(med, 4),
                 "spread_pct": round(100.0 * (max(ms[name]) - best) / best, 2),
                 "codewords_per_s": round(B / (best * 1e-3), 1),
                 "mean_iters": round(float(left[name][1].float().mean().item()), 3), "frame_errors": left[name][2],
                 "path_in_use": decs[name].path_in_use, "geometry": list(decs[name].geometry(B))}
            if kind == "fixed_per_layer":
                r["launches"] = 1 + n_layers * imax + (3 * (imax - 1) if early else 0) + 1
            else:
                r["launches"] = 3
            if kind.startswith("onchip") and "fixed_per_layer" in left:
                ref = left["fixed_per_layer"]
                r["equal"] = bool(torch.equal(left[name][1], ref[1]) and torch.equal(left[name][0], ref[0]))
            self.rows.append(r)
            print(json.dumps(r), flush=True)
        return {name: min(v) for name, v in ms.items()}

    def split(self, section, code, best1, best5):
        """The fixed part (staging) and the time of an iteration from the 1- and 5-iteration runs."""
        for name in best5:
            per_it = (best5[name] - best1[name]) / 4.0
            r = {"section": section, "code": code, "arm": name, "derived": "imax 5 and imax 1, no stop",
                 "ms_per_iteration": round(per_it, 4), "fixed_part_ms": round(best1[name] - per_it, 4)}
            self.rows.append(r)
            print(json.dumps(r), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=262144)
    p.add_argument("--batch16200", type=int, default=8192)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--caps", type=int, nargs="*", default=[16, 8, 2, 1],
                   help="codewords per workgroup of the further on-chip arms (the library's default is 4)")
    p.add_argument("--quick", action="store_true", help="sections (a) at 5 iterations and (b) only")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    bench = Bench(a, dev)

    H = codes.wlan_80211n(81)
    layers = codes.qc_layers(H, 81)
    G = engine.Graph(H, dev)
    N = H.shape[1]
    wlan = "wlan_80211n_1944_r12"
    arms = {"fp32_fused": ("fp32_fused", False), "fixed_per_layer": ("fixed_per_layer", False),
            "onchip_f32": ("onchip", False), "onchip_i8": ("onchip", True)}
    for k in a.caps:
        arms[f"onchip_cw{k}_i8"] = (f"onchip_cw{k}", True)
    x = awgn_llr(N, a.batch, 2.0, 1, dev, 0.5)
    best5 = bench.setting("a", wlan, G, layers, arms, 5, False, 2.0, x)
    if a.quick:
        del x
        for B in (8, 64):
            bench.setting("b", wlan, G, layers, arms, 10, True, 2.0, awgn_llr(N, B, 2.0, 3, dev, 0.5), inner=20)
    else:
        best1 = bench.setting("a", wlan, G, layers, arms, 1, False, 2.0, x)
        bench.split("a", wlan, best1, best5)
        for ebn0 in (2.0, 2.5):
            bench.setting("a", wlan, G, layers, arms, 10, True, ebn0, awgn_llr(N, a.batch, ebn0, 2, dev, 0.5))
        del x
        for B in (8, 64):
            bench.setting("b", wlan, G, layers, arms, 10, True, 2.0, awgn_llr(N, B, 2.0, 3, dev, 0.5), inner=20)

        H2 = codes.dvbs2_structured(seed=9, n=16200, k=7200, groups_hi=5, deg_hi=11, deg_lo=3)
        l2 = codes.dvbs2_layers(H2)
        G2 = engine.Graph(H2, dev)
        name2 = "dvbs2_structured_16200_k7200"
        arms2 = {"fixed_per_layer": ("fixed_per_layer", False), "onchip_f32": ("onchip", False),
                 "fixed_per_layer_i8": ("fixed_per_layer", True), "onchip_i8": ("onchip", True)}
        R2 = 7200 / 16200
        x2 = awgn_llr(16200, a.batch16200, 3.0, 4, dev, R2)
        b5 = bench.setting("c", name2, G2, l2, arms2, 5, False, 3.0, x2)
        b1 = bench.setting("c", name2, G2, l2, arms2, 1, False, 3.0, x2)
        bench.split("c", name2, b1, b5)
        bench.setting("c", name2, G2, l2, arms2, 10, True, 3.0, x2)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/bench_layered_fixed_fused.py", "device": torch.cuda.get_device_name(0),
                       "reps": a.reps, "warmup": a.warmup,
                       "parameters": {"alpha": ALPHA, "alpha16": ALPHA16, "beta_q": 0, "q_max": Q_MAX, "scale": SCALE},
                       "runs": bench.rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
