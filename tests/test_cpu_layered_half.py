"""CPU: the layered BP decoder with half-precision state (include/ibldpc.h "Layered BP, half-precision state") — the
numpy emulation (tests/_layered_half_ref.py) against an independent scalar restatement, the measured tolerance of the
GPU comparison, stop iterations and decisions under transcendentals moved by 1 ulp, the half state against the fp32
state, the host plan under AddressSanitizer / UndefinedBehaviorSanitizer as a stand-alone program
(tests/asan/layered_half_plan_check.cpp; nothing loaded into Python is sanitized), the C ABI's host-only refusals and
the private segments of the new kernels in the built code object."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

from informationbottleneckdecodingldpc_amd import codes
from tests import _layered_bp_ref as br
from tests import _layered_census as lc
from tests import _layered_half_ref as hr
from tests.test_cpu_layered_bp import run_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------
# 1. an independent scalar restatement: per codeword, per check, plain loops, leave-one-out by the specification's
#    forward-backward order written out on scalars
# ---------------------------------------------------------------------------------------------------------------
def _h(x):
    return np.float16(min(max(np.float32(x), np.float32(-65504.0)), np.float32(65504.0)))


def _bp(a, b, L):
    return np.float32(br.boxplus(np.float32(a), np.float32(b), L, np.float32))


def layered_half_scalar(H, layers, llr, imax, llr_max=150.0):
    A = sp.csr_matrix(H)
    A.sort_indices()
    rows = [[int(v) for v in A.indices[A.indptr[c]:A.indptr[c + 1]]] for c in range(A.shape[0])]
    L = np.float32(llr_max)
    n, B = llr.shape
    out = np.empty((n, B), np.float32)
    for b in range(B):
        P = [_h(np.float32(x) + np.float32(0)) for x in llr[:, b]]
        R = [[np.float16(0)] * len(r) for r in rows]
        for _ in range(imax):
            for layer in layers:
                for c in layer:
                    vs, Rc = rows[int(c)], R[int(c)]
                    D = len(vs)
                    q = [np.float32(np.float32(P[v]) - np.float32(Rc[k])) for k, v in enumerate(vs)]
                    new = [None] * D
                    if D == 2:
                        new[0] = min(max(q[1], -L), L)
                        new[1] = min(max(q[0], -L), L)
                    else:
                        S = [None] * D
                        S[D - 1] = q[D - 1]
                        for j in range(D - 2, 0, -1):
                            S[j] = _bp(q[j], S[j + 1], L)
                        new[0] = S[1]
                        F = q[0]
                        for w in range(1, D - 1):
                            new[w] = _bp(F, S[w + 1], L)
                            F = _bp(q[w], F, L)
                        new[D - 1] = F
                    for k, v in enumerate(vs):
                        Rc[k] = _h(new[k])
                        P[v] = _h(np.float32(q[k] + np.float32(Rc[k])))
        out[:, b] = [np.float32(x) for x in P]
    return out


def test_emulation_equals_the_scalar_restatement():
    """Bit for bit: on the code whose checks all have degree 2 (every family of hr.degree2_input, 3 iterations), where
    no box-plus is evaluated and every operation is exact or one correctly rounded operation, and on mixed() (degrees
    2..16) for two iterations, where both call numpy's transcendentals on the same scalars."""
    H, layers = hr.degree2_code()
    assert 380 <= H.shape[1] <= 420 and set(np.diff(H.indptr).tolist()) == {2}
    llr = hr.degree2_input(9)
    _, _, P_at = hr.layered_half_decode(H, layers, llr, 3, record=True)
    ref = P_at[-1]
    sc = layered_half_scalar(H, layers, llr, 3)
    assert np.array_equal(ref.view(np.uint32), sc.view(np.uint32))
    first = P_at[0]
    assert (np.signbit(first) & (first == 0)).any()        # -0 arises and is kept
    sub = (np.abs(first) > 0) & (np.abs(first) < 2.0 ** -14)
    assert sub.any()                                       # subnormal halves arise and are kept
    assert np.abs(ref).max() == 65504.0                    # the stage-in clamp bites
    H, layers = lc.mixed()
    llr = lc.awgn_llr(H.shape[1], 3, 3.0, seed=7, R=1.0 - H.shape[0] / H.shape[1])
    ref = hr.layered_half_decode(H, layers, llr, 2, early_stop=False)[0]
    sc = layered_half_scalar(H, layers, llr, 2)
    assert np.array_equal(ref.view(np.uint32), sc.view(np.uint32))


def test_minus_zero_decides_zero_and_a_sign_bit_would_not():
    """The pitfall the kernels spell out: on the degree-2 inputs the emulation holds -0 values; a decision read from
    the sign bit differs from the decision by value there, and the stop iterations of a decoder that did so differ."""
    H, layers = hr.degree2_code()
    llr = hr.degree2_input(130)
    out, it, P_at = hr.layered_half_decode(H, layers, llr, 4, record=True)
    minus_zero = np.signbit(P_at) & (P_at == 0)
    assert minus_zero.any()
    A = sp.csr_matrix(H)
    by_sign = [((A @ np.signbit(P).astype(np.int32)) % 2 == 0).all(axis=0) for P in P_at]
    by_value = [((A @ (P < 0).astype(np.int32)) % 2 == 0).all(axis=0) for P in P_at]
    print("stops", np.bincount(it, minlength=5).tolist(), "columns where the two decisions' syndromes differ",
          int(np.any(np.array(by_sign) != np.array(by_value), axis=0).sum()))
    assert np.any(np.array(by_sign) != np.array(by_value))
    assert len(set(it.tolist())) >= 2


# ---------------------------------------------------------------------------------------------------------------
# 2. and 3. the tolerance, stop iterations and decisions under one-ulp transcendentals
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hr.NAMED)
def test_tolerance_constants_and_stops_under_one_ulp(name):
    """hr.measure: the emulation against hr.DRAWS = 8 draws of br.one_ulp on the named input, over the values after
    every one of its 8 iterations. The largest absolute and (above 1) relative differences are the recorded ones — the
    draws are seeded, so they are reproduced, not approached — no stop iteration of the 130 differs in any draw and no
    hard decision of a frozen output flips. The full-size input's figures (N = 64800, 2 iterations) are recorded in
    hr.MEASURED the same way and are re-measured by tools/bench_layered_bp_half.py --measure-tolerance, not here: its
    nine decodes take about two minutes."""
    H, layers, llr = hr.named_input(name)
    assert llr.shape[1] == 130 and hr.DRAWS >= 8
    a, r, differ, flips = hr.measure(H, layers, llr, hr.IMAX)
    print(f"{name}: largest |x - y| {a!r}, largest relative above 1 {r!r}, stops differing {differ}, flips {flips}")
    assert (a, r) == hr.MEASURED[name]
    assert differ == 0 and flips == 0
    assert hr.ABS16 == 4 * max(v[0] for v in hr.MEASURED.values())
    assert hr.REL16 == 4 * max(v[1] for v in hr.MEASURED.values())
    assert hr.BAND16 == 10 * hr.ABS16 and br.excuse_cap(130) == 3


# ---------------------------------------------------------------------------------------------------------------
# 4. half state against fp32 state
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hr.NAMED)
def test_half_state_stops_where_the_fp32_state_does(name):
    H, layers, llr = hr.named_input(name)
    _, it, _ = hr.named_reference(name)
    o32, i32 = br.layered_bp_decode(H, layers, llr, hr.IMAX, dtype=np.float32)
    print(f"{name}: stops {np.bincount(it, minlength=hr.IMAX + 1).tolist()}")
    assert np.array_equal(it, i32)
    assert len(set(it.tolist())) >= 4


# ---------------------------------------------------------------------------------------------------------------
# 5. host plan under the sanitizers
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def half_plan_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("asan") / "layered_half_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "informationbottleneckdecodingldpc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "asan", "layered_half_plan_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("name,max_batch", [("wlan27", 64), ("wlan27", 129), ("wlan81", 65), ("dvbs2_small", 130),
                                            ("mixed", 9), ("mixed", 128)])
def test_half_plan_under_sanitizers(half_plan_check, tmp_path, name, max_batch):
    if name == "dvbs2_small":
        H, layers = br.small_dvbs2()
    elif name == "mixed":
        H, layers = lc.mixed()
    else:
        H, layers = lc.wlan(int(name[4:]))
    A = codes.canonical_csr(H)
    n_c, n_v = A.shape
    E = int(A.nnz)
    out = run_plan(half_plan_check, A, layers, max_batch, tmp_path)
    assert out["valid"] == 0 and out["unsupported"] == -1 and out["n_e"] == E
    cw_bytes = -(-(2 * n_v + 2 * E) // 4) * 4
    assert out["cw_bytes"] == cw_bytes
    assert out["cw_per_group"] == min(8, (160 * 1024) // cw_bytes)
    ldb = -(-max_batch // 128) * 128
    t64 = -(-max_batch // 64)
    assert out["ldb"] == ldb and out["mask_words"] == ldb // 64
    assert out["pad_words_all_ones"] == ldb // 64 - t64
    assert out["bytes_P"] == 2 * n_v * ldb and out["bytes_R"] == 2 * E * ldb and out["bytes_mask"] == 8 * (ldb // 64)
    assert out["bytes_total"] == (2 * n_v + 2 * E) * ldb + 16 * (ldb // 64) + 4 + 8 * n_v * t64
    if name == "wlan81":
        assert (n_v, E, cw_bytes, out["cw_per_group"]) == (1944, 6966, 17820, 8)     # the fp32 state holds 4
    if name == "dvbs2_small":
        assert (cw_bytes, out["cw_per_group"]) == (39600, 4)                          # the fp32 state holds 2
    assert out["pad_words_all_ones"] == {64: 1, 129: 1, 65: 0, 130: 1, 9: 1, 128: 0}[max_batch]


def test_half_plan_names_the_first_wide_check(half_plan_check, tmp_path):
    H, layers = lc.mixed()
    A = sp.lil_matrix(codes.canonical_csr(H))
    c = int(np.argmax(np.diff(codes.canonical_csr(H).indptr) == 16))
    A[c, [v for v in range(A.shape[1]) if A[c, v] == 0][0]] = 1
    H17 = codes.canonical_csr(sp.csr_matrix(A))
    out = run_plan(half_plan_check, H17, codes.greedy_layers(H17), 4, tmp_path)
    assert out["valid"] == 0 and out["unsupported"] == c


# ---------------------------------------------------------------------------------------------------------------
# 6. the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------
def _lib_loaded():
    from informationbottleneckdecodingldpc_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    return _lib, _lib.load()


def test_new_symbols_prototypes_and_host_only_refusals():
    _lib, L = _lib_loaded()
    assert {"ibl_layered_create_bp_half", "ibl_layered_is_half"} <= set(_lib.EXPORTS)
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    at = L.ibl_layered_create_bp_half.argtypes
    assert len(at) == 9 and list(at[:2]) == [vp, i32] and list(at[4:8]) == [i32, f32, i32, i32]
    with open(os.path.join(ROOT, "include", "ibldpc.h")) as fh:
        header = fh.read()
    flat = " ".join(header.split())
    assert ("int ibl_layered_create_bp_half(const ibl_graph* g, int32_t n_layers, const int32_t* layer_ptr, "
            "const int32_t* layer_checks, int32_t imax, float llr_max, int32_t max_batch, int32_t path, "
            "ibl_layered** out);") in flat
    assert "int ibl_layered_is_half(const ibl_layered* h, int32_t* half);" in header
    assert "Layered BP, half-precision state" in header
    for must in ("round-to-nearest-even", "65504", "BY VALUE", "binary16 input and output are not built",
                 "2 N + 2 E", "|llr| + 16 * llr_max <= 65504", "ROUNDED message"):
        assert must in flat, must
    # the existing entry point is documented as it was
    assert "int ibl_layered_create_bp(const ibl_graph* g" in header
    # refusals that need no device, in ibl_layered_create_bp's order: out, graph (then imax / max_batch, llr_max and
    # path, which are reached only with a graph: tests/test_gpu_layered_half.py)
    half = i32(7)
    assert L.ibl_layered_is_half(None, ctypes.byref(half)) == _lib.IBL_EINVAL
    assert L.ibl_last_error() == b"NULL argument" and half.value == 7
    ptr = np.zeros(2, np.int32)
    assert L.ibl_layered_create_bp_half(None, 1, ptr, ptr, 5, 150.0, 4, _lib.IBL_PATH_AUTO, None) == _lib.IBL_EINVAL
    assert L.ibl_last_error() == b"out is NULL"
    h = vp(1)
    assert L.ibl_layered_create_bp_half(None, 1, ptr, ptr, 0, -1.0, 0, 77, ctypes.byref(h)) == _lib.IBL_EINVAL
    assert L.ibl_last_error() == b"graph is NULL" and not h.value
    h32 = vp(1)
    assert L.ibl_layered_create_bp(None, 1, ptr, ptr, 0, -1.0, _lib.IBL_F32, 0, 77, ctypes.byref(h32)) == _lib.IBL_EINVAL
    assert L.ibl_last_error() == b"graph is NULL"


def test_python_layer_refuses_other_state_dtypes():
    import torch
    from informationbottleneckdecodingldpc_amd import BeliefPropagation_Layered_Decoder_class_irregular as Cls
    from informationbottleneckdecodingldpc_amd import ber, engine
    H, _ = lc.wlan(27)
    d = Cls(H, 10, 16, 4, Z=27, path="auto", state_dtype=torch.float16)
    assert d.state_dtype is torch.float16 and ber.decoder_kind(d) == "bp"
    assert Cls(H, 10, 16, 4, Z=27).state_dtype is torch.float32
    for bad in (torch.bfloat16, torch.float64, "float16", None):
        with pytest.raises(ValueError, match="state_dtype"):
            Cls(H, 10, 16, 4, Z=27, state_dtype=bad)
        with pytest.raises(ValueError, match="state_dtype"):
            engine.LayeredBPDecoder(None, [], 5, 4, state_dtype=bad)
    with pytest.raises(ValueError, match="alpha"):
        Cls(H, 10, 16, 4, Z=27, state_dtype=torch.float16, alpha=0.75)


# ---------------------------------------------------------------------------------------------------------------
# 7. the new kernels run without scratch and keep out of the fp32 kernels' names
# ---------------------------------------------------------------------------------------------------------------
def test_half_kernels_have_no_private_segment():
    _lib, _ = _lib_loaded()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kstats import code_objects
    half, fp32 = {}, set()
    for co in code_objects(_lib.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name],
                                 capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s+- \.", txt):
            m = re.search(r"\.name:\s+(\S+)", blk)
            p = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            if m and p and "layhp_" in m.group(1):
                half[m.group(1)] = int(p.group(1))
            if m and p and "laybp_" in m.group(1):
                fp32.add(m.group(1))
    names = sorted(re.search(r"layhp_[a-z_]+?(?=E)", k).group(0) for k in half)
    print(names)
    assert names == ["layhp_fused", "layhp_layer", "layhp_layer_first", "layhp_pack", "layhp_stage_in",
                     "layhp_stage_out"], half
    assert {k: v for k, v in half.items() if v} == {}
    assert len(fp32) == 4, fp32
