"""Wide flooding float decoders (a check of degree 17..32) without a device: what tests/test_gpu_float_wide.py rests
on. The two codes' degree profiles; the oracle's stop iterations at the inputs the GPU tests decode; the numpy float32
restatement of the fp32 BP order (tests/_float_wide_ref.py) against the fp64 oracle under the project's fp32 BP
criterion, at exactly those inputs; the float path's host planning on degree-32 checks under AddressSanitizer and
UndefinedBehaviorSanitizer as a stand-alone program (tests/asan/float_wide_plan_check.cpp; nothing loaded into Python
is sanitized); the wide kernels' metadata and the new C ABI entry."""
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
from oracle import oracle
from tests import _float_wide_ref as R
from tests._layered_census import mixed
from tests._layered_wide import small30, wide_mixed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from informationbottleneckdecodingldpc_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    return _lib


def test_degree_profiles():
    """wide_mixed: four checks of every degree 2..32 (so every degree 17..32), E = 2108, and it fits the fused kernel;
    small30: checks {29: 1, 30: 1079}, 1079 degree-2 staircase variables, too large for the fused kernel. Variable
    degrees stay within 16 on both."""
    H = wide_mixed()[0]
    cd, vd = np.diff(H.indptr), np.bincount(H.indices, minlength=H.shape[1])
    assert H.shape == (124, 400) and H.nnz == 2108
    assert np.bincount(cd)[2:].tolist() == [4] * 31 and set(range(17, 33)) <= set(cd.tolist())
    assert 1 <= vd.min() and vd.max() <= 16
    assert (H.nnz + H.shape[1]) * 16 < 160 * 1024
    H = small30()[0]
    cd, vd = np.diff(H.indptr), np.bincount(H.indices, minlength=H.shape[1])
    assert H.shape == (1080, 11160) and H.nnz == 32399
    assert dict(zip(*np.unique(cd, return_counts=True))) == {29: 1, 30: 1079}
    assert dict(zip(*np.unique(vd, return_counts=True))) == {1: 1, 2: 1079, 3: 10080}
    assert (H.nnz + H.shape[1]) * 16 > 160 * 1024


def _stop(name, B, dB, imax, what):
    g, llr = R.wide_graph(name), R.wide_llr(name, B, dB)
    if what == "ms32":
        return oracle.float32_decode(g, imax, llr, early_stop=True, return_iters=True)[1]
    kind = oracle.MINSUM if what == "ms64" else oracle.BP
    return oracle.float_decode(g, kind, imax, llr.astype(np.float64), early_stop=True, return_iters=True)[1]


@pytest.mark.parametrize("what", ["ms64", "bp64", "ms32"])
@pytest.mark.parametrize("B,want", [(9, 5), (130, 6)])
def test_oracle_stop_small30(what, B, want):
    """small30 at 5.5 dB with imax 12: the batch stop comes at 5 (B = 9) and 6 (B = 130), inside [2, imax - 2], in
    every arithmetic the GPU tests compare."""
    assert _stop("small30", B, 5.5, 12, what) == want and 2 <= want <= 10


def test_oracle_stop_wide_mixed():
    """wide_mixed at 7.0 dB with imax 12: B = 9 stops at 2; B = 130 runs to imax - 1 = 11 as a batch, while its
    columns, each decoded alone, stop at more than one iteration (the per-codeword stop's premise). At 3.0 dB
    (wide_mixed) and 4.0 dB (small30) nothing stops within 8."""
    assert _stop("wide_mixed", 9, 7.0, 12, "ms32") == 2
    assert _stop("wide_mixed", 130, 7.0, 12, "ms32") == 11
    g, llr = R.wide_graph("wide_mixed"), R.wide_llr("wide_mixed", 37, 7.0)
    each = {oracle.float32_decode(g, 12, llr[:, c:c + 1], early_stop=True, return_iters=True)[1] for c in range(37)}
    assert len(each) >= 2
    assert _stop("wide_mixed", 130, 3.0, 8, "ms32") == 7 and _stop("wide_mixed", 3, 3.0, 8, "bp64") == 7
    assert _stop("small30", 9, 4.0, 8, "ms32") == 7 and _stop("small30", 9, 4.0, 8, "bp64") == 7


@pytest.mark.parametrize("name,B,dB,imax,early", [("wide_mixed", 3, 3.0, 6, False), ("wide_mixed", 9, 3.0, 6, False),
                                                  ("wide_mixed", 130, 3.0, 6, True), ("small30", 9, 4.0, 8, False),
                                                  ("small30", 9, 5.5, 12, True)])
def test_fp32_bp_restatement_within_criterion(name, B, dB, imax, early):
    """The forward-backward order in float32, at every degree of both codes, stays within 1e-5 relative + 1e-4 of the
    fp64 oracle at the inputs of the GPU tests' fp32 BP cases, with the oracle's stop iteration."""
    g, llr = R.wide_graph(name), R.wide_llr(name, B, dB)
    ref, ref_it = oracle.float_decode(g, oracle.BP, imax, llr.astype(np.float64), early_stop=early, return_iters=True)
    out, it = R.bp32_decode(g, imax, llr, early_stop=early)
    bad = R.h5(out.astype(np.float64), ref)
    print(f"{name} B={B} {dB} dB: max |x-y| = {np.abs(out - ref).max():.3e}, outside: {int(bad.sum())}")
    assert it == ref_it
    assert bad.sum() == 0


def test_restated_minsum_is_the_oracle():
    """tests/_minsum_corrected_ref.decode, the corrected cases' reference, at (1, 0) on wide_mixed equals the oracle
    bit for bit in both precisions: its closed form holds at degrees 17..32 as well."""
    from tests._minsum_corrected_ref import decode
    g, llr = R.wide_graph("wide_mixed"), R.wide_llr("wide_mixed", 9, 3.0)
    out, it = decode(g, 1.0, 0.0, 6, llr, np.float32)
    assert np.array_equal(out.view(np.uint32), oracle.float32_decode(g, 6, llr).view(np.uint32))
    out, it = decode(g, 1.0, 0.0, 6, llr.astype(np.float64), np.float64)
    assert np.array_equal(out.view(np.uint64), oracle.float_decode(g, oracle.MINSUM, 6, llr.astype(np.float64)).view(np.uint64))


# ------------------------------------------------------------------ host planning under sanitizers
@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("asan") / "float_wide_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "informationbottleneckdecodingldpc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "asan", "float_wide_plan_check.cpp"), "-o", exe], check=True)
    return exe


def degree32_staircase():
    """70 checks of degree 32 over 2200 variables whose last two inputs are a staircase of degree-2 variables: every
    fold position is 30 or 31, a full fused task of 64 wide checks and a ragged one of 6."""
    n_c, n_i = 70, 30 * 70
    rows = np.repeat(np.arange(n_c), 30)
    cols = np.arange(n_i)
    H = sp.lil_matrix((n_c, n_i + n_c), dtype=np.int64)
    H[rows, cols] = 1
    for c in range(n_c):
        H[c, n_i + c] = 1
        H[c, n_i + (c + 1) % n_c] = 1
    return codes.canonical_csr(H.tocsr())


@pytest.mark.parametrize("name", ["degree32", "wide_mixed", "small30", "mixed"])
def test_float_plan_under_sanitizers(plan_check, tmp_path, name):
    H = {"degree32": degree32_staircase, "wide_mixed": lambda: wide_mixed()[0], "small30": lambda: small30()[0],
         "mixed": lambda: mixed()[0]}[name]()
    A = codes.canonical_csr(H)
    f = tmp_path / "g.bin"
    with open(f, "wb") as fh:
        np.array([A.shape[1], A.shape[0]], np.int32).tofile(fh)
        A.indptr.astype(np.int32).tofile(fh)
        A.indices.astype(np.int32).tofile(fh)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([plan_check, str(f)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout)
    print(out)
    assert out["failures"] == 0 and out["E"] == A.nnz
    assert out["wide"] == (name != "mixed")
    if name == "degree32":
        assert out["dcm"] == 32 and out["folded"] == 70 and out["fold_positions_above_16"] == 140
        assert out["fits_fused"] == 1 and out["fused_wide_tasks"] == 2 and out["small_wide_tasks"] == 2
    if name == "wide_mixed":
        assert out["fits_fused"] == 1 and out["fused_wide_tasks"] == 16 and out["small_wide_tasks"] == 16
    if name == "small30":
        assert out["fits_fused"] == 0 and out["folded"] == 1079 and out["small_wide_tasks"] == 18
    if name == "mixed":
        assert out["small_wide_tasks"] == 0 and out["fused_wide_tasks"] == 0


# ------------------------------------------------------------------ the build and the C ABI
def test_wide_float_kernels_exist_without_private_segment(lib):
    """The 24 wide instantiations (check kinds 0, 1, 2 with the wide bit 8, x fp32, fp64: fl_cn, fl_cn_small, fl_fused
    with and without the per-codeword stop's bit 4) are in the code object and none has a private segment
    (float_create refuses one that has)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kstats import code_objects
    seen = {}
    for co in code_objects(lib.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name],
                                 capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s+- \.", txt):
            m = re.search(r"\.name:\s+(_ZN3ibl\d+fl_(?:cn|cn_small|fused)ILi\d+E[fd]Li32E\S*)", blk)
            p = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            if m and p:
                seen[m.group(1)] = int(p.group(1))
    want = {f"_ZN3ibl{len(k)}{k}ILi{kind}E{f}Li32E" for k in ("fl_cn", "fl_cn_small") for kind in (8, 9, 10) for f in "fd"}
    want |= {f"_ZN3ibl8fl_fusedILi{kind}E{f}Li32ELi16E" for kind in (8, 9, 10, 12, 13, 14) for f in "fd"}
    got = {re.match(r"(.*?Li32E(?:Li16E)?)", k).group(1) for k in seen}
    assert got == want and len(seen) == 24
    assert {k: v for k, v in seen.items() if v} == {}


def test_capi_is_wide_without_a_device(lib):
    assert "ibl_float_is_wide" in lib.EXPORTS
    L = lib.load()
    with open(os.path.join(ROOT, "include", "ibldpc.h")) as fh:
        header = fh.read()
    assert "int ibl_float_is_wide(const ibl_float* h, int32_t* wide);" in header
    w = ctypes.c_int32(7)
    assert L.ibl_float_is_wide(None, ctypes.byref(w)) == lib.IBL_EINVAL and w.value == 7
    assert "NULL" in L.ibl_last_error().decode()


def test_dropin_classes_report_wide():
    """The reference-named classes tell a wide code from a narrow one from the code alone."""
    from informationbottleneckdecodingldpc_amd.bp_decoder_irreg import BeliefPropagationDecoderClassIrregular
    from informationbottleneckdecodingldpc_amd.min_sum_decoder_irreg import Min_Sum_Decoder_class_irregular
    assert Min_Sum_Decoder_class_irregular(wide_mixed()[0], 6, 16, 2).wide is True
    assert BeliefPropagationDecoderClassIrregular(small30()[0], 6, 16, 2).wide is True
    assert Min_Sum_Decoder_class_irregular(codes.wlan_80211n(27), 6, 16, 2).wide is False
    with pytest.raises(AttributeError):
        Min_Sum_Decoder_class_irregular(codes.wlan_80211n(27), 6, 16, 2).wide = True
