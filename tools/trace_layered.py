"""Task trace of the layered min-sum kernel (DESIGN.md "Layered min-sum"): where a layer step spends its time.

Needs the diagnostic variant: `python tools/variants.py laytrace`, then

  python tools/trace_layered.py [--batch B] [--out profiles/layered_task_trace.txt]

Decodes WLAN N = 1944 (12 layers of 81 checks: a 64-lane and a 17-lane task each) with every CU busy; wave 0 of
workgroup 0 records, for the second iteration of its first codeword, the clock (s_memtime) at each task's
start, when the task's variable indices have arrived from memory, and at its end (its LDS writes done). The
clock reads wait for all of the wave's outstanding memory operations, so the wave traced runs a little slower
than its neighbours; the other wave of its SIMD runs untraced beside it."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANT = os.path.join(ROOT, "informationbottleneckdecodingldpc_amd", "variants", "libibldpc_laytrace.so")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8 * 256 * 4)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if not os.path.exists(VARIANT):
        sys.exit(f"{VARIANT} not found: build it with `python tools/variants.py laytrace`")
    os.environ["IBLDPC_LIB"] = VARIANT
    raw = os.path.join(os.path.dirname(a.out) if a.out else ".", "layered_task_trace.bin")
    os.environ["IBL_TRACE_LAYERED"] = raw
    import torch

    from informationbottleneckdecodingldpc_amd import codes, engine
    H = codes.wlan_80211n(81)
    layers = codes.qc_layers(H, 81)
    dev = torch.device("cuda", 0)
    dec = engine.LayeredDecoder(engine.Graph(H, dev), layers, 3, a.batch)
    s2 = 1.0 / (2.0 * 0.5 * 10 ** 0.15)
    llr = ((1.0 + s2 ** 0.5 * torch.randn((H.shape[1], a.batch), device=dev)) * (2.0 / s2)).contiguous()
    dec.decode(llr, early_stop=False)
    torch.cuda.synchronize()
    tr = np.fromfile(raw, dtype=np.uint64).reshape(-1, 3).astype(np.int64)
    os.remove(raw)
    deg = np.diff(H.indptr)
    lines = [f"layered min-sum task trace: WLAN N=1944, B={a.batch}, cw_per_group/ngroups/grid={dec.geometry(a.batch)}",
             "workgroup 0, wave 0, first codeword, iteration 2; clocks (s_memtime)",
             "task layer lanes degree   idx_wait   body   total   gap_to_next"]
    t = 0
    for l, layer in enumerate(layers):
        d = int(deg[layer[0]])
        for cnt in ([64, len(layer) - 64] if len(layer) > 64 else [len(layer)]):
            gap = int(tr[t + 1, 0] - tr[t, 2]) if t + 1 < len(tr) else 0
            lines.append(f"{t:4d} {l:5d} {cnt:5d} {d:6d} {tr[t, 1] - tr[t, 0]:10d} {tr[t, 2] - tr[t, 1]:6d} "
                         f"{tr[t, 2] - tr[t, 0]:7d} {gap:8d}")
            t += 1
    full = [i for i in range(len(tr)) if i % 2 == 0]
    part = [i for i in range(len(tr)) if i % 2 == 1]
    tot = tr[:, 2] - tr[:, 0]
    lines.append(f"iteration: {int(tr[-1, 2] - tr[0, 0])} clocks; 64-lane tasks mean {tot[full].mean():.0f}, "
                 f"17-lane tasks mean {tot[part].mean():.0f}; idx wait mean {(tr[:, 1] - tr[:, 0]).mean():.0f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
