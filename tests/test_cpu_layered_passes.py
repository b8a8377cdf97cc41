"""CPU: the host side of the layered decoder's per-layer (HBM) path — codes.dvbs2_layers, the two new C ABI
names, and the per-layer host plan (csrc/layered_plan.h plan_layered_passes and the launch / scratch geometry)
under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program
(tests/asan/layered_pass_plan_check.cpp; nothing loaded into Python is sanitized)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from informationbottleneckdecodingldpc_amd import codes
from tests import _layered_census as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_dvbs2():
    return codes.dvbs2_structured(seed=5, n=5400, k=1800, groups_hi=2, deg_hi=7, deg_lo=2)


def test_dvbs2_layers_small_and_full_size():
    H = small_dvbs2()
    assert H.shape == (3600, 5400) and H.nnz == 14399
    deg = np.bincount(np.diff(H.indptr))
    assert {d: int(c) for d, c in enumerate(deg) if c} == {3: 1, 4: 3599}
    layers = codes.dvbs2_layers(H)
    assert len(layers) == 10 and all(len(l) == 360 for l in layers)
    assert [l[:3].tolist() for l in layers[:2]] == [[0, 10, 20], [1, 11, 21]]
    codes.validate_layers(H, layers)
    Hd = codes.dvbs2_structured(seed=3)
    full = codes.dvbs2_layers(Hd)
    assert len(full) == 90 and all(len(l) == 360 for l in full)
    assert sorted(int(c) for l in full for c in l) == list(range(32400))
    # an explicit q that divides n_c and still separates the staircase: 2 q classes of 180
    assert len(codes.dvbs2_layers(H, q=20)) == 20


def test_dvbs2_layers_refusals():
    H = small_dvbs2()
    with pytest.raises(ValueError) as e:
        codes.dvbs2_layers(H, q=7)               # 3600 is no multiple of 7
    assert "multiple" in str(e.value)
    with pytest.raises(ValueError):
        codes.dvbs2_layers(H[:3599])             # n_c / 360 is not whole: q = 9 does not divide 3599
    # two same-residue edges of one variable: variable 0 also joins a second check of the class of its first
    A = codes.canonical_csr(H).tolil()
    c0 = int(codes.canonical_csr(H).tocsc().indices[0])      # a check of variable 0
    c1 = next(c for c in range(c0 % 10, 3600, 10) if c != c0 and A[c, 0] == 0)
    A[c1, 0] = 1
    B = codes.canonical_csr(sp.csr_matrix(A))
    with pytest.raises(ValueError) as e:
        codes.dvbs2_layers(B)
    lo, hi = sorted((c0, c1))
    assert f"checks {lo} and {hi} of layer {c0 % 10} share variable 0" in str(e.value)


def test_exports_hold_the_new_names():
    from informationbottleneckdecodingldpc_amd import _build, _lib
    assert {"ibl_layered_create_path", "ibl_layered_path_in_use"} <= set(_lib.EXPORTS)
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    L = _lib.load()
    assert L.ibl_layered_create_path and L.ibl_layered_path_in_use
    with open(os.path.join(ROOT, "include", "ibldpc.h")) as fh:
        header = fh.read()
    assert "int ibl_layered_create_path(" in header and "int ibl_layered_path_in_use(" in header
    assert "not part of this interface yet" not in header


@pytest.fixture(scope="module")
def pass_plan_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("asan") / "layered_pass_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "informationbottleneckdecodingldpc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "asan", "layered_pass_plan_check.cpp"), "-o", exe], check=True)
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


@pytest.mark.parametrize("name,max_batch", [("dvbs2_small", 130), ("wlan27", 64), ("reg96", 65)])
def test_pass_plan_under_sanitizers(pass_plan_check, tmp_path, name, max_batch):
    if name == "dvbs2_small":
        H = small_dvbs2()
        layers = codes.dvbs2_layers(H)
    elif name == "wlan27":
        H, layers = lc.wlan(27)
    else:
        H = codes.regular_code(96, 3, 6, seed=1)
        layers = codes.greedy_layers(H)
    A = codes.canonical_csr(H)
    n_c, n_v = A.shape
    out = run_plan(pass_plan_check, A, layers, max_batch, tmp_path)
    tiles = -(-max_batch // 64)
    assert out["valid"] == 0 and out["n_layers"] == len(layers) and out["max_layer"] == max(len(l) for l in layers)
    assert out["ntiles"] == tiles and out["ldb"] == 64 * tiles
    # a wave item per (check of the layer, tile of 64 codewords), four items a workgroup
    assert out["layer_grids"] == [-(-len(l) * tiles // 4) for l in layers]
    assert out["syn_grid"] == -(-(-(-n_c // 16)) * tiles // 4)
    assert out["bytes_P"] == 4 * n_v * 64 * tiles and out["bytes_state"] == 4 * n_c * 64 * tiles
    assert out["bytes_bits"] == 8 * n_v * tiles
    assert out["bytes_total"] == (4 * n_v + 12 * n_c) * 64 * tiles + 16 * tiles + 4 + 8 * n_v * tiles
    assert out["launches_fixed"] == len(layers) and out["launches_early"] == len(layers) + 3


def test_pass_plan_refuses_bad_layers(pass_plan_check, tmp_path):
    H = codes.regular_code(96, 3, 6, seed=1)
    layers = [l.tolist() for l in codes.greedy_layers(H)]
    layers[-1].append(layers[0][0])
    out = run_plan(pass_plan_check, H, layers, 8, tmp_path)
    assert out["valid"] == -1 and "listed twice" in out["error"]
