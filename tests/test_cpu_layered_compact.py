"""CPU: the host side of the per-layer layered decoder's compaction of running codewords — the two C ABI names and
their device-free refusals, the drop-in class's refusals, the policy and the rank map of csrc/layered_plan.h under
AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program (tests/asan/layered_compact_plan_check.cpp;
nothing loaded into Python is sanitized), the Python restatement of the policy (tests/_layered_compact_ref.py)
against that program, and the conditions on the input of tests/test_gpu_layered_compact.py."""
import ctypes
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from informationbottleneckdecodingldpc_amd import codes
from tests import _layered_compact_ref as cr
from tests._layered_census import awgn_llr
from tests._layered_ref import layered_decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAB = (0.8125, 0.0)

# (B, (every, min_free_pct)) -> the compactions (iteration, extent, running) of the GPU test's input
EXPECTED = {
    (260, (1, 1)): [(3, 260, 253), (5, 253, 126), (7, 126, 48)],
    (260, (1, 50)): [(5, 260, 126), (7, 126, 48)],
    (260, (2, 1)): [(4, 260, 203), (6, 203, 72), (8, 72, 41)],
    (130, (1, 1)): [(3, 130, 127), (5, 127, 62)],
    (65, (1, 1)): [(3, 65, 64)],
}


@functools.lru_cache(maxsize=None)
def small260():
    """The GPU test's input and its reference decode: (H, layers, llr, out, iters)."""
    H = codes.dvbs2_structured(seed=5, n=5400, k=1800, groups_hi=2, deg_hi=7, deg_lo=2)
    layers = codes.dvbs2_layers(H)
    llr = awgn_llr(5400, 260, 2.0, seed=7)
    out, it = layered_decode(H, layers, llr, 10, *NAB)
    for a in (llr, out, it):
        a.setflags(write=False)
    return H, layers, llr, out, it


@pytest.fixture(scope="module")
def lib():
    from informationbottleneckdecodingldpc_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    return _lib


def test_exports_and_header(lib):
    names = {"ibl_layered_set_compaction", "ibl_layered_compaction_stats"}
    assert names <= set(lib.EXPORTS)
    L = lib.load()
    assert L.ibl_layered_set_compaction and L.ibl_layered_compaction_stats
    with open(os.path.join(ROOT, "include", "ibldpc.h")) as fh:
        header = fh.read()
    assert "int ibl_layered_set_compaction(ibl_layered* h, int32_t every, int32_t min_free_pct);" in header
    assert "int ibl_layered_compaction_stats(const ibl_layered* h, void* stream, int32_t* compactions," in header
    assert "tE - tR >= max(1, ceil(min_free_pct * tE / 100))" in header
    assert L.ibl_version() == 3


def test_refusals_without_a_device(lib):
    L = lib.load()
    for every, pct, word in [(1, 25, "NULL"), (-1, 25, "every"), (1, 0, "min_free_pct"), (1, 101, "min_free_pct"),
                             (0, 0, "NULL")]:
        assert L.ibl_layered_set_compaction(None, every, pct) == lib.IBL_EINVAL, (every, pct)
        assert word in L.ibl_last_error().decode(), (every, pct, L.ibl_last_error().decode())
    n, e = ctypes.c_int32(-5), ctypes.c_int32(-5)
    assert L.ibl_layered_compaction_stats(None, None, ctypes.byref(n), ctypes.byref(e)) == lib.IBL_EINVAL
    assert "NULL" in L.ibl_last_error().decode() and (n.value, e.value) == (-5, -5)


def test_dropin_refusals():
    import informationbottleneckdecodingldpc_amd as pkg
    H = codes.regular_code(96, 3, 6, seed=1)
    cls = pkg.Min_Sum_Layered_Decoder_class_irregular
    for kw in (dict(fixed=True, path="passes"), dict(fixed=True, path="auto"), dict(path="fused"), dict()):
        for compact in (True, (1, 1)):
            with pytest.raises(ValueError) as e:
                cls(H, 5, 16, 8, compact=compact, **kw)     # path defaults to "fused"
            assert "compact" in str(e.value)
    for compact in (None, False):
        assert cls(H, 5, 16, 8, compact=compact).compact is None
    d = cls(H, 5, 16, 8, path="passes", compact=(2, 25))
    assert d.compact == (2, 25) and cls(H, 5, 16, 8, path="auto", compact=True).compact is True


@pytest.fixture(scope="module")
def compact_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("asan") / "layered_compact_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "informationbottleneckdecodingldpc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "asan", "layered_compact_plan_check.cpp"), "-o", exe], check=True)
    return exe


def run_check(exe, args=()):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout)
    assert out["failures"] == 0
    return out


def replay(exe, tmp_path, iters, B, imax, every, pct):
    f = tmp_path / f"decode_{B}_{imax}_{every}_{pct}.bin"
    with open(f, "wb") as fh:
        np.array([B, imax, every, pct], np.int32).tofile(fh)
        np.asarray(iters[:B], np.int32).tofile(fh)
    return run_check(exe, [str(f)])


def test_policy_and_map_under_sanitizers(compact_check):
    out = run_check(compact_check)
    assert out["cases"] >= 2000 and out["events"] == []


def test_restatement_agrees_with_the_program(compact_check, tmp_path):
    """The same iteration counts through csrc/layered_plan.h (masks, the rank map, the in-place move) and through
    the Python restatement: the same compactions, the same final extent and the same columns in the same order."""
    rng = np.random.default_rng(3)
    cases = [(np.full(130, 1), 130, 4, 1, 1), (np.full(130, 4), 130, 4, 1, 1), (np.arange(1, 301) % 7 + 1, 300, 7, 1, 1),
             (np.r_[np.full(64, 1), np.full(66, 9)], 130, 9, 1, 1), (np.r_[np.full(129, 1), [6]], 130, 6, 1, 100),
             (np.r_[np.full(129, 1), [6]], 130, 6, 1, 50)]
    for B in (1, 63, 64, 65, 130, 260, 1000):
        for every, pct in ((1, 1), (1, 50), (2, 1), (4, 25), (3, 100)):
            cases.append((rng.integers(1, 13, size=B), B, 12, every, pct))
    some = 0
    for iters, B, imax, every, pct in cases:
        got = replay(compact_check, tmp_path, iters, B, imax, every, pct)
        events, extent, orig = cr.compactions(iters, B, imax, every, pct)
        assert [tuple(e) for e in got["events"]] == events, (B, imax, every, pct)
        assert got["extent"] == extent and got["orig"] == orig.tolist()
        some += len(events)
    assert some > 20


def test_restatement_without_stop():
    events, extent, orig = cr.compactions(np.full(130, 10), 130, 10, 1, 1, early_stop=False)
    assert events == [] and extent == 130 and np.array_equal(orig, np.arange(130))


def test_gpu_input_exercises_the_compactions(compact_check, tmp_path):
    """Conditions on the input of tests/test_gpu_layered_compact.py: its reference iteration histogram, and the
    compactions the policy makes of it — one, two and three in a decode, one of them from a padded tile."""
    H, layers, llr, out, it = small260()
    assert np.bincount(it, minlength=11).tolist() == [0, 0, 0, 7, 50, 77, 54, 24, 7, 8, 33]
    for (B, (every, pct)), want in EXPECTED.items():
        events, extent, orig = cr.compactions(it, B, 10, every, pct)
        assert events == want, (B, every, pct, events)
        assert extent == want[-1][2] and np.array_equal(orig, np.flatnonzero(it[:B] > want[-1][0]))
        got = replay(compact_check, tmp_path, it, B, 10, every, pct)
        assert [tuple(e) for e in got["events"]] == want and got["extent"] == extent
    assert sorted(len(v) for v in EXPECTED.values()) == [1, 2, 2, 3, 3]
    assert any(E % 64 for v in EXPECTED.values() for _, E, _ in v)
