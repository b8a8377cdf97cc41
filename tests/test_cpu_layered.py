"""CPU: the layered min-sum decoder's host side — layer constructions (codes.qc_layers / greedy_layers /
validate_layers), the C ABI's host-only ibl_layers_validate, the device plan (csrc/layered_plan.h) under
AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program, tests/asan/layered_plan_check.cpp; nothing
loaded into Python is sanitized), and the numpy reference the GPU tests compare against."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from informationbottleneckdecodingldpc_amd import codes
from tests._layered_ref import layered_decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from informationbottleneckdecodingldpc_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    return _lib


@pytest.fixture(scope="module")
def reg96():
    return codes.regular_code(96, 3, 6, seed=1)


def as_sets(layers):
    return [frozenset(int(c) for c in l) for l in layers]


@pytest.mark.parametrize("Z", [27, 81])
def test_qc_layers_are_the_block_rows(Z):
    H = codes.wlan_80211n(Z)
    layers = codes.qc_layers(H, Z)
    assert len(layers) == 12 and all(len(l) == Z for l in layers)
    assert [int(l[0]) for l in layers] == [i * Z for i in range(12)]
    codes.validate_layers(H, layers)
    # taking checks in row order, every check of a block row conflicts with none of its own row and with some
    # check of every earlier block row: the greedy partition is the block rows
    assert as_sets(codes.greedy_layers(H)) == as_sets(layers)
    with pytest.raises(ValueError):
        codes.qc_layers(H, Z + 1)


def test_greedy_layers_uneven(reg96):
    layers = codes.greedy_layers(reg96)
    codes.validate_layers(reg96, layers)
    assert [len(l) for l in layers] == [8, 8, 7, 7, 7, 6, 3, 2]
    assert sorted(int(c) for l in layers for c in l) == list(range(48))


def bad_layer_cases(H):
    """(name, H, layers, word expected in the message)."""
    A = codes.canonical_csr(H)
    good = [l.tolist() for l in codes.greedy_layers(A)]
    missing = [list(l) for l in good]
    gone = missing[-1].pop()
    dup = [list(l) for l in good]
    dup[-1].append(dup[0][0])
    # two checks of one layer sharing a variable: move a check of layer 1 that conflicts with layer 0 into layer 0
    share = [list(l) for l in good]
    vars0 = set(A.indices[np.concatenate([np.arange(A.indptr[c], A.indptr[c + 1]) for c in good[0]])].tolist())
    mover = next(c for c in good[1] if vars0 & set(A.indices[A.indptr[c]:A.indptr[c + 1]].tolist()))
    share[1].remove(mover)
    share[0].append(mover)
    # a degree-1 check: drop all but the first entry of the last row
    B = A.tolil()
    keep = A.indices[A.indptr[-2]]
    B[A.shape[0] - 1, :] = 0
    B[A.shape[0] - 1, keep] = 1
    B = codes.canonical_csr(B.tocsr())
    return [("missing", A, missing, f"check {gone} is in no layer"),
            ("duplicate", A, dup, f"check {dup[0][0]} is listed twice"),
            ("shared", A, share, f"and {mover} of layer 0 share variable"),
            ("degree1", B, [l.tolist() for l in codes.greedy_layers(B)], f"check {A.shape[0] - 1} has degree 1")]


def test_layers_validate_capi_agrees_with_python(lib, reg96):
    for H in (codes.wlan_80211n(27), codes.wlan_80211n(81), reg96):
        A = codes.canonical_csr(H)
        for layers in (codes.greedy_layers(A), [np.array([c]) for c in range(A.shape[0])]):
            codes.validate_layers(A, layers)
            lib.layers_validate(A.shape[1], A.shape[0], A.indptr, A.indices, layers)
    for name, A, layers, word in bad_layer_cases(reg96):
        with pytest.raises(ValueError) as ep:
            codes.validate_layers(A, layers)
        assert word in str(ep.value), (name, str(ep.value))
        with pytest.raises(lib.IBLError) as ec:
            lib.layers_validate(A.shape[1], A.shape[0], A.indptr, A.indices, layers)
        assert word in str(ec.value), (name, str(ec.value))
        nl, ptr, chk = lib.pack_layers(layers)
        rc = lib.load().ibl_layers_validate(A.shape[1], A.shape[0], A.indptr.astype(np.int32),
                                            A.indices.astype(np.int32), nl, ptr, chk)
        assert rc == (lib.IBL_EUNSUPPORTED if name == "degree1" else lib.IBL_EINVAL), name


@pytest.fixture(scope="module")
def layered_plan_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("asan") / "layered_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "informationbottleneckdecodingldpc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "asan", "layered_plan_check.cpp"), "-o", exe], check=True)
    return exe


def run_plan(exe, H, layers, tmp_path):
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
    r = subprocess.run([exe, str(f)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout)
    assert out["failures"] == 0
    return out


@pytest.mark.parametrize("name", ["wlan27", "wlan81", "reg96"])
def test_layered_plan_under_sanitizers(layered_plan_check, tmp_path, reg96, name):
    H = {"wlan27": lambda: codes.wlan_80211n(27), "wlan81": lambda: codes.wlan_80211n(81), "reg96": lambda: reg96}[name]()
    A = codes.canonical_csr(H)
    layers = codes.greedy_layers(A)
    out = run_plan(layered_plan_check, A, layers, tmp_path)
    deg = np.diff(A.indptr)
    # tasks: per layer and degree, ceil(count / 64)
    want = sum(-(-int((deg[l] == d).sum()) // 64) for l in layers for d in np.unique(deg[l]))
    assert out["valid"] == 0 and out["n_layers"] == len(layers) and out["n_tasks"] == want
    assert out["cw_bytes"] == 4 * A.shape[1] + 12 * A.shape[0]
    assert out["cw_per_group"] == min(8, 160 * 1024 // out["cw_bytes"])
    if name == "wlan81":
        assert out["cw_bytes"] == 19440 and out["cw_per_group"] == 8
    # the refused layer lists go through the same code under the sanitizers
    if name == "reg96":
        for case, B, bad, word in bad_layer_cases(A):
            o = run_plan(layered_plan_check, B, bad, tmp_path)
            assert o["valid"] == (-2 if case == "degree1" else -1) and word in o["error"], (case, o)


def test_reference_noiseless_and_fixed_iterations():
    H = codes.wlan_80211n(27)
    layers = codes.qc_layers(H, 27)
    llr = np.full((H.shape[1], 3), 4.0, np.float32)
    out, iters = layered_decode(H, layers, llr, 6)
    assert iters.tolist() == [1, 1, 1] and (out > 0).all()
    out2, iters2 = layered_decode(H, layers, llr, 6, early_stop=False)
    assert iters2.tolist() == [6, 6, 6] and (out2 > 0).all()
    # plain min-sum on a noiseless word only ever adds positive messages; the correction shrinks them
    out3, it3 = layered_decode(H, layers, llr, 1, alpha=0.75, beta=0.5)
    assert it3.tolist() == [1, 1, 1] and (out3 >= 4.0).all() and (out3 <= out).all() and (out3 < out).any()
