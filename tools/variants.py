"""Build kernel variants of libibldpc.so side by side (in-tree, so they travel to the GPU box) for A/B
timing: `python tools/variants.py` then `IBLDPC_LIB=<path> python bench.py ...`."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from informationbottleneckdecodingldpc_amd import _build  # noqa: E402

VARIANTS = {
    "w1": ["IBL_W=1"],
    # one dword per lane everywhere (rows padded to 512 codewords): the Infinity-Cache sub-batch experiment
    "w1l1": ["IBL_W=1", "IBL_LIGHT_W=1"],
    "w2": ["IBL_W=2"],
    "w4": ["IBL_W=4", "IBL_LB8=512"],
    "w2b": ["IBL_W=2", "IBL_LB8=512"],
    "wpe5": ["IBL_WPE8=5"],
    "wpe6": ["IBL_WPE8=6"],
    # spill experiment (DESIGN.md "Private segment"): MAXD=16 kernels at 1024-thread launch bounds
    # (128 VGPRs) spill their item buffers to scratch; run with IBL_ALLOW_SCRATCH=1
    "spill16": ["IBL_LB16=1024"],
    # variable pass co-scheduling: waves with (threadIdx.x >> 8) < IBL_MIX take the light (degree <= 4,
    # HBM-bound) items first, the others the heavy (LDS-bound) ones
    "mix1": ["IBL_MIX16=4"],
    # no light-first waves in the variable pass (round 5 adopted 4 of 16, round 6 6 of 16, the variable composite 4 again)
    "mix0": ["IBL_MIX16=0"],
    "mixw5": ["IBL_MIX16=5"],
    "mixw10": ["IBL_MIX16=10"],
    "mix2": ["IBL_MIX16=8"],
    "mix3": ["IBL_MIX16=12"],
    "mixw2": ["IBL_MIX16=2"],
    "mixw3": ["IBL_MIX16=3"],
    "mixw6": ["IBL_MIX16=6"],
    # three light variable items in flight per wave instead of two; round-2 light rows (W=2, depth 3)
    "ld3": ["IBL_LIGHT_DEPTH=3"],
    "lw2": ["IBL_LIGHT_W=2", "IBL_LIGHT_DEPTH=3"],
    # variable pass light items with 1-KiB row segments per wave (4 dwords per lane), 3 / 2 in flight
    "lw4": ["IBL_LIGHT_W=4"],
    "lw4d2": ["IBL_LIGHT_W=4", "IBL_LIGHT_DEPTH=2"],
    # plain (cached) variable-pass row accesses instead of the default nontemporal ones
    "nt0": ["IBL_NT=0"],
    # check schedule of 2 codewords x 4 chains (half the column-term registers of 4 x 2)
    "s2n": ['IBL_SCHED_FILE="ib_sched_s2n.inc"'],
    "w1l4": ["IBL_W=1", 'IBL_SCHED_FILE="ib_sched_w1l4.inc"'],
    "w2l4": ['IBL_SCHED_FILE="ib_sched_w2l4.inc"'],
    "cl3": ['IBL_SCHED_FILE="ib_sched_cl3.inc"'],
    "v4l2": ['IBL_SCHED_FILE="ib_sched_v4l2.inc"'],
    "v2l3": ['IBL_SCHED_FILE="ib_sched_v2l3.inc"'],
    # the variable pass's composite bodies with 4 codewords x 4 chains / 4 x 2 (the default is 2 x 4); both put
    # ib_vn_fast<8> at 128 VGPRs with 7 spilled (24 B private segment), which ibl_ib_create refuses
    "vk44": ['IBL_SCHED_FILE="ib_sched_vk44.inc"'],
    "vk42": ['IBL_SCHED_FILE="ib_sched_vk42.inc"'],
    # fused IB kernel phase trace (IBL_TRACE_FUSED=<file>)
    "ftrace": ["IBL_FUSED_TRACE=1", "IBL_DIAG=1"],
    # layered min-sum kernel task trace (IBL_TRACE_LAYERED=<file>; tools/trace_layered.py)
    "laytrace": ["IBL_LAY_TRACE=1", "IBL_DIAG=1"],
    # timing-only host hooks (IBL_VN_PART, IBL_TRACE_WAVES, IBL_DEBUG_SYNC): not in the product build
    "diag": ["IBL_DIAG=1"],
    # float per-pass rows as plain loads / stores (the default is nontemporal since round 5)
    "flplain": ["IBL_FL_NT=0"],
    # check-pass rows nontemporal (the default since round 5) / with the default cache policy
    "ntcn": ["IBL_NT_CN=1"],
    "ntcn0": ["IBL_NT_CN=0"],
    # float kernels built with NaNs not honoured but the IEEE mode bit on
    "ieeeon": [],
}
# per-source flag overrides (replace _build.SRC_FLAGS)
SRC_FLAGS = {"ieeeon": {"float_kernels.hip": ["-fno-honor-nans"]}}
# gen_sched.py arguments of the variants that need their own schedule file
# (S_cn L_cn S_vn L_vn [S_vk L_vk]; both generated files, ib_sched_<n>.inc and ib_sched_<n>_unrolled.inc)
SCHED_ARGS = {"s2n": "2 4 2 4", "w1l4": "4 4 2 4", "w2l4": "4 4 2 4", "cl3": "4 3 2 4", "v4l2": "4 2 4 2", "v2l3": "4 2 2 3",
              "vk44": "4 2 2 4 4 4", "vk42": "4 2 2 4 4 2"}

if __name__ == "__main__":
    names = sys.argv[1:] or list(VARIANTS)
    outdir = os.path.join(_build.PKG, "variants")
    os.makedirs(outdir, exist_ok=True)
    for n in names:
        defines = list(VARIANTS[n])
        if n in SCHED_ARGS:
            gen = [sys.executable, os.path.join(os.path.dirname(__file__), "gen_sched.py")]
            args = SCHED_ARGS[n].split()
            with open(os.path.join(_build.CSRC, f"ib_sched_{n}.inc"), "w") as f:
                subprocess.run([*gen, *args], stdout=f, check=True)
            # the unrolled bodies follow the variant's S / L (their own file)
            with open(os.path.join(_build.CSRC, f"ib_sched_{n}_unrolled.inc"), "w") as f:
                subprocess.run([*gen, "--unrolled", *args], stdout=f, check=True)
            defines.append(f'IBL_UNROLLED_FILE="ib_sched_{n}_unrolled.inc"')
        lib = os.path.join(outdir, f"libibldpc_{n}.so")
        _build.build(defines=defines, lib=lib, tag=n, src_flags=SRC_FLAGS.get(n), force="--force" in os.environ.get("VARIANT_FLAGS", ""))
        print(lib)
