"""CPU: the IB fast path's degree-2 variable fold plan (csrc/plan.h plan_ib_fold) under AddressSanitizer and
UndefinedBehaviorSanitizer — a stand-alone program, tests/asan/fold_plan_check.cpp; nothing loaded into Python is
sanitized."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from informationbottleneckdecodingldpc_amd import codes, graph
from tests._codes import mixed_code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_dvb():
    """The headline's degree profile at one ninth of the size: check degrees {6: 1, 7: 3599}, variable degrees
    {1: 1, 2: 3599, 3: 2160, 8: 1440}, E = 25,199."""
    return codes.dvbs2_structured(seed=3, n=7200, k=3600, groups_hi=4)


@pytest.fixture(scope="module")
def fold_plan_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("asan") / "fold_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "informationbottleneckdecodingldpc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "asan", "fold_plan_check.cpp"), "-o", exe], check=True)
    return exe


def run_plan(exe, H, tmp_path):
    A = codes.canonical_csr(H)
    f = tmp_path / "g.bin"
    with open(f, "wb") as fh:
        np.array([A.shape[1], A.shape[0]], np.int32).tofile(fh)
        A.indptr.astype(np.int32).tofile(fh)
        A.indices.astype(np.int32).tofile(fh)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(f)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout)
    g = graph.build_graph(H)
    assert (out["n_v"], out["n_c"], out["n_e"]) == (g.n_v, g.n_c, g.n_e) and out["failures"] == 0
    assert out["folded"] + out["rest"] == g.n_v and sum(out["classes"]) == g.n_c
    return out


def test_fold_plan_staircase(fold_plan_check, tmp_path):
    """Every staircase parity variable folds: 3599 of the small code's; the first check has one parity input
    (class 2: its last position only), the last holds a degree-2 variable next to the degree-1 one (class 1)."""
    H = small_dvb()
    cd, vd = np.diff(sp.csr_matrix(H).indptr), np.bincount(sp.csr_matrix(H).indices, minlength=H.shape[1])
    assert dict(zip(*np.unique(cd, return_counts=True))) == {6: 1, 7: 3599}
    assert dict(zip(*np.unique(vd, return_counts=True))) == {1: 1, 2: 3599, 3: 2160, 8: 1440}
    out = run_plan(fold_plan_check, H, tmp_path)
    assert out["folded"] == 3599
    assert out["classes"] == [0, 1, 1, 3598]


def test_fold_plan_nothing_qualifies(fold_plan_check, tmp_path):
    """Column order reversed: the parity columns come first in every check, no variable qualifies."""
    H = sp.csr_matrix(small_dvb())[:, ::-1]
    out = run_plan(fold_plan_check, H, tmp_path)
    assert out["folded"] == 0 and out["classes"][1:] == [0, 0, 0]


def test_fold_plan_random_mixed(fold_plan_check, tmp_path):
    """A random irregular graph (degree-2 variables at arbitrary positions, checks of degree 2): whatever
    folds, the invariants hold."""
    H = mixed_code(np.arange(2, 9), np.array([1, 2, 2, 2, 3, 4]), 900, seed=21)
    out = run_plan(fold_plan_check, H, tmp_path)
    assert 0 <= out["folded"] <= int((np.bincount(sp.csr_matrix(H).indices, minlength=H.shape[1]) == 2).sum())


def test_fold_plan_full_size_dvbs2(fold_plan_check, tmp_path, dvb_H):
    """The headline graph (N = 64800, R = 1/2): all 32,399 staircase variables fold."""
    out = run_plan(fold_plan_check, dvb_H, tmp_path)
    assert out["folded"] == 32399
