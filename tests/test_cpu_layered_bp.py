"""CPU: the layered BP decoder's specification and host side (include/ibldpc.h "Layered BP") — the numpy
restatement against an independent scalar one, its float32 form against its float64 form, the instability of the
min-sum clamp rule that the specification avoids, the named inputs of the GPU tests, the new C ABI names, the
drop-in class's refusals, the host plan under AddressSanitizer / UndefinedBehaviorSanitizer as a stand-alone program
(tests/asan/layered_bp_plan_check.cpp; nothing loaded into Python is sanitized), and the private segments of the
new kernels in the built code object."""
import ctypes
import json
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


small_dvbs2 = br.small_dvbs2


# ---------------------------------------------------------------------------------------------------------------
# an independent scalar restatement: per codeword, per check, leave-one-out folds of the other inputs in fp64
# ---------------------------------------------------------------------------------------------------------------
def _boxplus_scalar(a, b, L):
    import math
    aa, ab = abs(a), abs(b)
    mag = min(aa, ab) + math.log1p(math.exp(-(aa + ab))) - math.log1p(math.exp(-abs(aa - ab)))
    mag = min(max(mag, 0.0), L)
    return -mag if (a < 0) != (b < 0) else mag


def layered_bp_scalar(H, layers, llr, imax, llr_max):
    A = sp.csr_matrix(H)
    A.sort_indices()
    rows = [[int(v) for v in A.indices[A.indptr[c]:A.indptr[c + 1]]] for c in range(A.shape[0])]
    L = float(np.float32(llr_max))
    n, B = llr.shape
    out = np.empty((n, B))
    for b in range(B):
        P = [float(x) for x in llr[:, b]]
        R = [[0.0] * len(r) for r in rows]
        for _ in range(imax):
            for layer in layers:
                for c in layer:
                    vs, Rc = rows[int(c)], R[int(c)]
                    q = [P[v] - Rc[k] for k, v in enumerate(vs)]
                    for k, v in enumerate(vs):
                        others = [q[j] for j in range(len(vs)) if j != k]
                        t = others[0]
                        for x in others[1:]:
                            t = _boxplus_scalar(x, t, L)
                        t = min(max(t, -L), L)
                        Rc[k] = t
                        P[v] = q[k] + t
        out[:, b] = P
    return out


def test_restatement_equals_the_scalar_one():
    """The vectorised forward-backward restatement against plain loops with leave-one-out folds (another order of
    an associative operation: equal up to fp64 rounding), on every degree 2..16."""
    H, layers = lc.mixed()
    llr = lc.awgn_llr(H.shape[1], 4, 2.0, seed=3, R=1.0 - H.shape[0] / H.shape[1])
    ref, _ = br.layered_bp_decode(H, layers, llr, 3, early_stop=False, dtype=np.float64)
    sc = layered_bp_scalar(H, layers, llr, 3, 150.0)
    assert np.abs(ref - sc).max() <= 1e-9


# ---------------------------------------------------------------------------------------------------------------
# the named inputs of the GPU tests: shared with tests/test_gpu_layered_bp.py
# ---------------------------------------------------------------------------------------------------------------
dvb_input, wlan_input, dvb_reference, wlan_reference = br.dvb_input, br.wlan_input, br.dvb_reference, br.wlan_reference


@pytest.mark.parametrize("which,imax", [("dvb", 10), ("wlan81", 20), ("wlan27_2.5dB", 20)])
def test_float32_form_is_within_h5_of_the_float64_form(which, imax):
    """On the two stop-test inputs and on the input of the instability finding (llr_max 150, where all 64 codewords
    converge). A codeword that does NOT converge amplifies rounding differences from iteration to iteration: on WLAN
    Z = 27 at 1.5 dB, awgn_llr(648, 32, 1.5, seed=7), the codewords 5, 20 and 26 leave H5 from iterations 13, 14 and
    15 on (relative differences up to 0.3), every converged one stays inside."""
    if which == "dvb":
        H, layers, llr = dvb_input()
    elif which == "wlan27_2.5dB":
        H, layers = lc.wlan(27)
        llr = lc.awgn_llr(648, 64, 2.5, seed=7)
    else:
        H, layers, llr = wlan_input(int(which[4:]))
    r64, _ = br.layered_bp_decode(H, layers, llr, imax, early_stop=False, dtype=np.float64)
    r32, _ = br.layered_bp_decode(H, layers, llr, imax, early_stop=False, dtype=np.float32)
    assert r32.dtype == np.float32
    bad = br.h5_violations(r32, r64)
    assert not bad.any(), (int(bad.sum()), float(np.abs(r32 - r64).max()))


def test_clamping_q_is_unstable_and_the_specified_rule_is_not():
    """WLAN Z = 27 at 2.5 dB, llr_max 30, 12 iterations: the specified rule (Q not clamped) leaves all 64 codewords
    with a zero syndrome; the layered min-sum rule, Q = clamp(P - R), does not (it left none)."""
    H, layers = lc.wlan(27)
    A = sp.csr_matrix(H)
    llr = lc.awgn_llr(648, 64, 2.5, seed=7)

    def clean(P):
        return int((((A @ (P < 0).astype(np.int32)) % 2) == 0).all(axis=0).sum())

    good, _ = br.layered_bp_decode(H, layers, llr, 12, llr_max=30.0, early_stop=False)
    bad, _ = br.layered_bp_decode(H, layers, llr, 12, llr_max=30.0, early_stop=False, clamp_q=True)
    assert clean(good) == 64
    assert clean(bad) < 64
    print("clamped-Q variant: zero syndromes", clean(bad), "of 64")


def test_named_inputs_meet_their_conditions():
    _, it_d, exc_d = dvb_reference(10, True)
    H, layers, llr = dvb_input()
    A = sp.csr_matrix(H)
    out_d = dvb_reference(10, True)[0]
    unconverged = int((((A @ (out_d < 0).astype(np.int32)) % 2) != 0).any(axis=0).sum())
    print("dvb: stops", sorted(set(it_d.tolist())), "unconverged", unconverged, "excusable", int(exc_d.sum()))
    assert len(set(it_d.tolist())) >= 4 and unconverged >= 1
    assert int(exc_d.sum()) <= br.excuse_cap(130)
    _, it_w, exc_w = wlan_reference(81, 20, True)
    print("wlan81: stops", sorted(set(it_w.tolist())), "excusable", int(exc_w.sum()))
    assert int(exc_w.sum()) <= br.excuse_cap(32)
    _, _, exc_w27 = wlan_reference(27, 20, True)
    assert int(exc_w27.sum()) <= br.excuse_cap(32)


# ---------------------------------------------------------------------------------------------------------------
# the library's new names
# ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_and_prototypes():
    from informationbottleneckdecodingldpc_amd import _build, _lib
    assert {"ibl_layered_create_bp", "ibl_layered_is_bp"} <= set(_lib.EXPORTS)
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    L = _lib.load()
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    assert list(L.ibl_layered_create_bp.argtypes[:2]) == [vp, i32]
    assert list(L.ibl_layered_create_bp.argtypes[4:9]) == [i32, f32, i32, i32, i32]
    assert len(L.ibl_layered_create_bp.argtypes) == 10
    assert L.ibl_layered_is_bp.argtypes[0] is vp
    with open(os.path.join(ROOT, "include", "ibldpc.h")) as fh:
        header = fh.read()
    proto = ("int ibl_layered_create_bp(const ibl_graph* g, int32_t n_layers, const int32_t* layer_ptr, "
             "const int32_t* layer_checks, int32_t imax, float llr_max, int32_t precision, int32_t max_batch, "
             "int32_t path, ibl_layered** out);")
    assert proto in " ".join(header.split())
    assert "int ibl_layered_is_bp(const ibl_layered* h, int32_t* bp);" in header
    assert "Layered BP:" in header and "layered BP are not built" not in header
    # host-only refusals: NULL arguments need no device
    bp = i32(7)
    assert L.ibl_layered_is_bp(None, ctypes.byref(bp)) == _lib.IBL_EINVAL
    h = vp()
    ptr = np.zeros(2, np.int32)
    assert L.ibl_layered_create_bp(None, 1, ptr, ptr, 5, 150.0, _lib.IBL_F32, 4, _lib.IBL_PATH_AUTO,
                                   ctypes.byref(h)) == _lib.IBL_EINVAL
    assert b"graph is NULL" in L.ibl_last_error()


def test_dropin_class_refusals():
    from informationbottleneckdecodingldpc_amd import BeliefPropagation_Layered_Decoder_class_irregular as Cls
    from informationbottleneckdecodingldpc_amd import ber
    from informationbottleneckdecodingldpc_amd.min_sum_layered_decoder_irreg import \
        Min_Sum_Layered_Decoder_class_irregular
    H, layers = lc.wlan(27)
    d = Cls(H, 10, 16, 4, Z=27, path="auto")
    assert isinstance(d, Min_Sum_Layered_Decoder_class_irregular)
    assert d.data_len == 324 and len(d.layers) == 12 and d.llr_max == 150.0 and d.last_iterations is None
    assert ber.decoder_kind(d) == "bp"
    assert hasattr(d, "decode_OpenCL_belief_propagation") and not hasattr(d, "decode_OpenCL_min_sum")
    assert d._DECODER_NAME == "layered BP"
    with pytest.raises(AttributeError):
        d.decode_OpenCL_min_sum(np.zeros((648, 1), np.float32))
    for kw in (dict(alpha=0.75), dict(beta=0.5), dict(fixed=True), dict(compact=True), dict(compact=(2, 25))):
        with pytest.raises(ValueError, match=next(iter(kw))):
            Cls(H, 10, 16, 4, Z=27, **kw)
    with pytest.raises(ValueError, match="path"):
        Cls(H, 10, 16, 4, Z=27, path="onchip")
    with pytest.raises(ValueError, match="not both"):
        Cls(H, 10, 16, 4, Z=27, layers=layers)


# ---------------------------------------------------------------------------------------------------------------
# host plan under the sanitizers
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bp_plan_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("asan") / "layered_bp_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "informationbottleneckdecodingldpc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "asan", "layered_bp_plan_check.cpp"), "-o", exe], check=True)
    return exe


def run_plan(exe, H, layers, max_batch, tmp_path):
    A = codes.canonical_csr(H)
    f = tmp_path / "g.bin"
    with open(f, "wb") as fh:
        np.array([A.shape[1], A.shape[0]], np.int32).tofile(fh)
        A.indptr.astype(np.int32).tofile(fh)
        A.indices.astype(np.int32).tofile(fh)
        np.array([len(layers)], np.int32).tofile(fh)
        np.concatenate([[0], np.cumsum([len(l) for l in layers])]).astype(np.int32).tofile(fh)
        np.concatenate([np.asarray(l, np.int32) for l in layers]).astype(np.int32).tofile(fh)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(f), str(max_batch)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout)
    assert out["failures"] == 0
    return out


@pytest.mark.parametrize("name,max_batch", [("dvbs2_small", 130), ("wlan27", 64), ("wlan81", 65), ("mixed", 9)])
def test_bp_plan_under_sanitizers(bp_plan_check, tmp_path, name, max_batch):
    if name == "dvbs2_small":
        H, layers = small_dvbs2()
    elif name == "mixed":
        H, layers = lc.mixed()
    else:
        H, layers = lc.wlan(int(name[4:]))
    A = codes.canonical_csr(H)
    n_c, n_v = A.shape
    E = int(A.nnz)
    out = run_plan(bp_plan_check, A, layers, max_batch, tmp_path)
    tiles = -(-max_batch // 64)
    assert out["valid"] == 0 and out["unsupported"] == -1 and out["n_e"] == E
    assert out["cw_bytes"] == 4 * n_v + 4 * E
    assert out["cw_per_group"] == min(8, (160 * 1024) // (4 * n_v + 4 * E))
    assert out["bytes_P"] == 4 * n_v * 64 * tiles and out["bytes_R"] == 4 * E * 64 * tiles
    assert out["bytes_total"] == (4 * n_v + 4 * E) * 64 * tiles + 16 * tiles + 4 + 8 * n_v * tiles


def test_bp_plan_names_the_first_wide_check(bp_plan_check, tmp_path):
    """A check of degree 17 passes the layer validation (the min-sum decoder runs it) and is named as unsupported."""
    H, layers = lc.mixed()
    A = sp.lil_matrix(codes.canonical_csr(H))
    c = int(np.argmax(np.diff(codes.canonical_csr(H).indptr) == 16))
    free = [v for v in range(A.shape[1]) if A[c, v] == 0]
    A[c, free[0]] = 1
    H17 = codes.canonical_csr(sp.csr_matrix(A))
    out = run_plan(bp_plan_check, H17, codes.greedy_layers(H17), 4, tmp_path)
    assert out["valid"] == 0 and out["unsupported"] == c


# ---------------------------------------------------------------------------------------------------------------
# the new kernels run without scratch
# ---------------------------------------------------------------------------------------------------------------
def test_bp_kernels_have_no_private_segment():
    """private_segment_fixed_size of every laybp_* kernel in the built code object is 0, read as
    tests/test_cpu_host.py reads it; ibl_layered_create_bp checks the same at run time."""
    from informationbottleneckdecodingldpc_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kstats import code_objects
    seen = {}
    for co in code_objects(_lib.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name],
                                 capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s+- \.", txt):
            m = re.search(r"\.name:\s+(\S+)", blk)
            p = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            if m and p and "laybp_" in m.group(1):
                seen[m.group(1)] = int(p.group(1))
    assert len(seen) == 4, seen   # laybp_fused, laybp_layer, laybp_layer_first, laybp_stage_in
    assert {k: v for k, v in seen.items() if v} == {}
