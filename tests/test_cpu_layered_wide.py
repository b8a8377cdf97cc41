"""CPU: the layered min-sum decoder at check degrees 17..32 without a device — the validators' range, the census
that holds the inputs of tests/test_gpu_layered_wide.py to every (degree, first-argmin position) pair of the wide
bodies, the spread of the stop iterations its compaction and skipping cases rest on, the wide host plan
(csrc/layered_plan.h) under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program
(tests/asan/layered_wide_plan_check.cpp; nothing loaded into Python is sanitized), the code object's metadata and the
new C ABI entry."""
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
from tests import _layered_wide as lw
from tests._layered_census import FAMILIES, mixed, wlan
from tests._layered_fixed_ref import fixed_decode, quantise
from tests._layered_ref import layered_decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from informationbottleneckdecodingldpc_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    return _lib


def with_degree(d, n_v=40):
    """One check of degree d over n_v variables and a degree-2 check beside it, each a layer."""
    H = sp.lil_matrix((2, n_v), dtype=np.int64)
    H[0, :d] = 1
    H[1, n_v - 2:] = 1
    return codes.canonical_csr(H.tocsr()), [np.array([0]), np.array([1])]


def test_codes():
    H, layers = lw.wide_mixed()
    deg = np.diff(H.indptr)
    assert H.shape == (124, 400) and np.bincount(deg)[2:].tolist() == [4] * 31 and H.data.max() == 1
    assert np.bincount(H.indices, minlength=400).min() >= 1
    assert len(layers) > 8 and len({len(l) for l in layers}) > 3      # greedy layers of uneven size
    H, layers = lw.small30()
    deg = np.diff(H.indptr)
    assert H.shape == (1080, 11160) and {int(d): int((deg == d).sum()) for d in np.unique(deg)} == {29: 1, 30: 1079}
    assert len(layers) == 3 and all(len(l) == 360 for l in layers)
    assert 4 * 11160 + 16 * 1080 == 61920 and (160 * 1024) // 61920 == 2      # the fused kernel's fit: 2 per group


def test_validators_accept_degrees_up_to_32(lib):
    """codes.validate_layers and ibl_layers_validate accept both codes (dvbs2_layers validates on its way) and the
    two high-rate DVB-S2 shapes' degree; degree 33 and degree 1 are refused, naming the degree."""
    for H, layers in (lw.wide_mixed(), lw.small30()):
        codes.validate_layers(H, layers)
        lib.layers_validate(H.shape[1], H.shape[0], H.indptr, H.indices, layers)
    H, layers = with_degree(32)
    codes.validate_layers(H, layers)
    lib.layers_validate(40, 2, H.indptr, H.indices, layers)
    H, layers = with_degree(33)
    with pytest.raises(ValueError, match="degree 33") as e:
        codes.validate_layers(H, layers)
    assert "2..32" in str(e.value)
    with pytest.raises(lib.IBLError) as e:
        lib.layers_validate(40, 2, H.indptr, H.indices, layers)
    assert f"rc={lib.IBL_EUNSUPPORTED}" in str(e.value) and "degree 33" in str(e.value) and "2..32" in str(e.value)
    H1 = sp.csr_matrix(np.array([[1, 1, 0], [0, 0, 1]], dtype=np.int64))
    with pytest.raises(ValueError, match="degree 1"):
        codes.validate_layers(H1, [[0], [1]])
    with pytest.raises(lib.IBLError) as e:
        lib.layers_validate(3, 2, H1.indptr, H1.indices, [[0], [1]])
    assert f"rc={lib.IBL_EUNSUPPORTED}" in str(e.value) and "degree 1" in str(e.value)


def fp32_runs(B):
    """(what, llr, alpha, beta, llr_max, early) of every fp32 decode the GPU tests make on wide_mixed at batch B."""
    H, _ = lw.wide_mixed()
    for a, b in lw.WIDE_AB:
        for early in (True, False):
            yield "awgn", lw.wide_awgn(B), a, b, 150.0, early
    for fam in lw.WIDE_FAMILIES:
        gen, params = FAMILIES[fam]
        x = gen(H, B)
        for a, b, L in params:
            for early in (True, False):
                yield fam, x, a, b, L, early


@pytest.mark.parametrize("B", lw.CENSUS_BATCHES)
def test_census_fp32(B):
    """The reference alone, on the inputs the GPU decodes (6 iterations), visits every (degree, first-argmin
    position) pair of degrees 17..32 among the updates of running codewords — position 31 of degree 32 included —
    writes a negated R on edge 31, and at B = 130 the AWGN input alone does, with stops spread over the
    iterations."""
    H, layers = lw.wide_mixed()
    seen, neg31, awgn_alone = set(), 0, None

    def hook(it, cs, D, Q, pos, m1, m2, mag, Rn, done):
        nonlocal neg31
        d = Q.shape[1]
        if d < 17:
            return
        run = ~done
        got.update((d, int(p)) for p in np.unique(pos[:, run]))
        if d == 32:
            neg31 += int(np.signbit(Rn[:, 31, :][:, run]).sum())

    for what, x, a, b, L, early in fp32_runs(B):
        got = set()
        out, it = layered_decode(H, layers, x, lw.CENSUS_IMAX, a, b, L, early_stop=early, hook=hook)
        seen |= got
        if what == "awgn" and early and (a, b) == lw.WIDE_AB[1]:
            awgn_alone = got
            print("B", B, "awgn stops", np.bincount(it, minlength=lw.CENSUS_IMAX + 1).tolist(), "pairs", len(got))
            assert len(set(it.tolist())) >= (4 if B == 130 else 3)
    assert len(lw.WIDE_PAIRS) == 392 and seen >= lw.WIDE_PAIRS
    assert (32, 31) in seen and neg31 > 0
    if B == 130:
        assert awgn_alone >= lw.WIDE_PAIRS


def test_census_fixed():
    """The same for the integer reference on the fixed-point tests' input (B = 260 of AWGN, both parameter sets):
    every pair, and sign bit 31 of a degree-32 check set."""
    H, layers = lw.wide_mixed()
    x = lw.wide_awgn(260)
    for p in lw.FIXED_PARAMS:
        seen, bit31 = set(), 0

        def hook(it, cs, Pin, T, pos, m1, m2, mag_in, mag, Pu, done):
            nonlocal bit31
            d = T.shape[1]
            if d < 17:
                return
            run = ~done
            seen.update((d, int(q)) for q in np.unique(pos[:, run]))
            if d == 32:
                Rn = Pu - T
                bit31 += int((Rn[:, 31, :][:, run] < 0).sum())

        out, it = fixed_decode(H, layers, quantise(x, p[3]), lw.CENSUS_IMAX, *p[:3], hook=hook)
        print(p, "stops", np.bincount(it, minlength=lw.CENSUS_IMAX + 1).tolist(), "pairs", len(seen), "bit 31", bit31)
        assert seen >= lw.WIDE_PAIRS and bit31 > 0 and len(set(it.tolist())) >= 3


def test_small30_spreads_the_stops():
    """small30 at 4.0 dB, 130 codewords, 8 iterations: at least 4 distinct stop iterations in both arithmetics, and
    in fp32 at least one tile's worth of codewords (of three tiles) done after iteration 4, so that a compaction
    attempted after every iteration frees a tile."""
    hist = np.bincount(lw.small30_ref()[1], minlength=9).tolist()
    print("fp32 iters", hist)
    assert hist == [0, 0, 0, 0, 13, 30, 27, 17, 43]
    assert 130 - sum(hist[:6]) <= 128 and (np.asarray(hist) > 0).sum() >= 4
    for p in lw.FIXED_PARAMS:
        h = np.bincount(lw.small30_fixed_ref(p)[1], minlength=9)
        print("fixed", p, "iters", h.tolist())
        assert (h > 0).sum() >= 4


@pytest.fixture(scope="module")
def wide_plan_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("asan") / "layered_wide_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "informationbottleneckdecodingldpc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "asan", "layered_wide_plan_check.cpp"), "-o", exe], check=True)
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


@pytest.mark.parametrize("name,max_batch", [("wide_mixed", 130), ("wide_mixed", 260), ("small30", 5), ("small30", 257),
                                            ("degree32", 1), ("mixed", 257), ("wlan27", 64)])
def test_wide_plan_under_sanitizers(wide_plan_check, tmp_path, name, max_batch):
    """Wide codes get the wide sizes, narrow codes exactly the sizes the narrow formulas always gave."""
    H, layers = {"wide_mixed": lw.wide_mixed, "small30": lw.small30, "degree32": lambda: with_degree(32),
                 "mixed": mixed, "wlan27": lambda: wlan(27)}[name]()
    A = codes.canonical_csr(H)
    n_c, n_v = A.shape
    wide = name in ("wide_mixed", "small30", "degree32")
    out = run_plan(wide_plan_check, A, layers, max_batch, tmp_path)
    assert out["valid"] == 0 and out["wide"] == int(wide) and out["max_degree"] == int(np.diff(A.indptr).max())
    sw = 16 if wide else 12
    assert out["cw_bytes"] == 4 * n_v + sw * n_c
    assert out["cw_per_group"] == min(8, (160 * 1024) // (4 * n_v + sw * n_c))
    t64, t256 = -(-max_batch // 64), -(-max_batch // 256)
    assert out["pass_state"] == 4 * n_c * 64 * t64
    assert out["pass_total"] == (4 * n_v + sw * n_c) * 64 * t64 + 16 * t64 + 4 + 8 * n_v * t64
    assert out["compact_rows"] == n_v + (4 if wide else 3) * n_c
    assert out["fix_state"] == (8 if wide else 4) * n_c * 256 * t256
    assert out["fix_total"] == (n_v + (8 if wide else 4) * n_c) * 256 * t256 + 64 * t256 + 4 + 8 * n_v * t64
    if name == "small30":
        assert (out["cw_bytes"], out["cw_per_group"]) == (61920, 2)


def test_wide_plan_check_refuses_degree_33(wide_plan_check, tmp_path):
    H, layers = with_degree(33)
    out = run_plan(wide_plan_check, H, layers, 64, tmp_path)
    assert out["valid"] == -2 and "degree 33" in out["error"] and "2..32" in out["error"]


WIDE_KERNELS = ("lay_fused_wide", "lay_stage_in_wide", "lay_stage_in_c_wide", "lay_layer_wide", "lay_compact_rows_wide",
                "layfix_stage_in_wide", "layfix_layer_wide")


def test_layered_kernels_have_no_private_segment(lib):
    """Every kernel whose name starts with lay — the wide ones, which must be there, included — runs without
    scratch: private_segment_fixed_size 0 in the code object's metadata (the create functions check the same at
    run time and refuse a build that violates it)."""
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
            m = re.search(r"\.name:\s+(\S+)", blk)
            p = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            if m and p:
                plain = re.match(r"_ZN3ibl\d+(lay\w*?)E", m.group(1))
                if plain:
                    seen[plain.group(1)] = int(p.group(1))
    print(seen)
    assert set(WIDE_KERNELS) <= set(seen) and {"lay_fused", "lay_layer", "layfix_layer"} <= set(seen)
    assert len(seen) >= 26
    assert {k: v for k, v in seen.items() if v} == {}


def test_capi_is_wide_without_a_device(lib):
    assert "ibl_layered_is_wide" in lib.EXPORTS
    L = lib.load()
    with open(os.path.join(ROOT, "include", "ibldpc.h")) as fh:
        header = fh.read()
    assert "int ibl_layered_is_wide(const ibl_layered* h, int32_t* wide);" in header
    w = ctypes.c_int32(7)
    assert L.ibl_layered_is_wide(None, ctypes.byref(w)) == lib.IBL_EINVAL and w.value == 7
    assert "NULL" in L.ibl_last_error().decode()
    assert L.ibl_version() == 3
