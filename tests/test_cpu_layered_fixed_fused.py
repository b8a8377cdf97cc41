"""CPU: the fixed-point fused layered kernel without a device — the new C ABI entry point's exports and refusals
(ibl_layered_create_fixed_fused), the Python layers' path names, and the host geometry (csrc/layered_plan.h
fixfused_*: the fit rule, the LDS slices, the staging buffer and its tiles) under AddressSanitizer and
UndefinedBehaviorSanitizer as a stand-alone program (tests/asan/layered_fixed_fused_plan_check.cpp; nothing loaded
into Python is sanitized) against a numpy restatement of the fit rule."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from informationbottleneckdecodingldpc_amd import codes
from tests import _layered_fixed_census as fc
from tests._layered_wide import small30, wide_mixed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS, CAP = 160 * 1024, 4


def fit(n_v, n_c, wide):
    """The header's fit rule: (ldn, cw_bytes, codewords before the cap, cw_per_group)."""
    ldn = -(-n_v // 4) * 4
    cw_bytes = ldn + (8 if wide else 4) * n_c
    return ldn, cw_bytes, LDS // cw_bytes, min(CAP, LDS // cw_bytes)


def code16200():
    """The code of the GPU tests that the fp32 fused kernel cannot hold."""
    H = codes.dvbs2_structured(seed=9, n=16200, k=7200, groups_hi=5, deg_hi=11, deg_lo=3)
    return H, codes.dvbs2_layers(H)


def test_capi_without_a_device():
    """The new name is exported and declared, every refusal that needs no graph is given without one, in the order
    of ibl_layered_create_fixed, and the older entry point answers as it did."""
    from informationbottleneckdecodingldpc_amd import _build, _lib
    assert "ibl_layered_create_fixed_fused" in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    L = _lib.load()
    with open(os.path.join(ROOT, "include", "ibldpc.h")) as fh:
        header = fh.read()
    assert "int ibl_layered_create_fixed_fused(" in header
    for text in ("cw_bytes = ldn + 4 n_c", "ldn + 8 n_c", "min(4, floor(160 KiB / cw_bytes))", "THREE launches"):
        assert text in header, text
    ptr, chk = np.zeros(2, np.int32), np.zeros(1, np.int32)

    def create(imax=5, a16=13, bq=0, qm=31, scale=2.0, mb=8, out=True):
        h = ctypes.c_void_p(1)
        rc = L.ibl_layered_create_fixed_fused(None, 1, ptr, chk, imax, a16, bq, qm, scale, mb,
                                              ctypes.byref(h) if out else None)
        assert not out or h.value is None
        return rc, L.ibl_last_error().decode()

    for kw in (dict(a16=-1), dict(a16=17), dict(bq=-1), dict(bq=64), dict(qm=0), dict(qm=64), dict(scale=0.0),
               dict(scale=-2.0), dict(scale=float("inf")), dict(scale=float("nan")), dict(imax=0), dict(mb=0),
               dict(out=False)):
        rc, msg = create(**kw)
        assert rc == _lib.IBL_EINVAL and "graph is NULL" not in msg, (kw, msg)
    for kw in (dict(), dict(a16=0, bq=63, qm=63), dict(a16=16, qm=1, scale=3.3)):   # in range: the graph is missing
        rc, msg = create(**kw)
        assert rc == _lib.IBL_EINVAL and "graph is NULL" in msg, (kw, msg)
    # ibl_layered_create_fixed is what it was
    h = ctypes.c_void_p(1)
    rc = L.ibl_layered_create_fixed(None, 1, ptr, chk, 5, 13, 0, 31, 2.0, 8, _lib.IBL_PATH_FUSED, ctypes.byref(h))
    assert rc == _lib.IBL_EUNSUPPORTED and "fixed-point fused kernel is not built" in L.ibl_last_error().decode()
    rc = L.ibl_layered_create_fixed(None, 1, ptr, chk, 5, 13, 0, 31, 2.0, 8, 3, ctypes.byref(h))
    assert rc == _lib.IBL_EINVAL


def test_path_names():
    """"onchip" belongs to the fixed-point decoder alone; the path is judged before anything touches a device."""
    from informationbottleneckdecodingldpc_amd import engine
    assert set(engine.LayeredDecoder._PATHS) == {"auto", "passes", "fused"}
    assert set(engine.LayeredFixedDecoder._PATHS) == {"auto", "passes", "fused", "onchip"}
    assert engine.LayeredFixedDecoder._PATHS is not engine.LayeredDecoder._PATHS
    with pytest.raises(ValueError):
        engine.LayeredDecoder(None, [], 5, 8, path="onchip")
    with pytest.raises(ValueError):
        engine.LayeredFixedDecoder(None, [], 5, 8, path="hbm")


def test_drop_in_class():
    import informationbottleneckdecodingldpc_amd as pkg
    cls = pkg.Min_Sum_Layered_Decoder_class_irregular
    H, layers = fc.wlan(27)
    ok = dict(layers=layers, alpha=0.8125, beta=0.5, path="onchip", fixed=True)
    d = cls(H, 8, 16, 16, **ok)
    assert d.path == "onchip" and d.fixed and (d.alpha16, d.beta_q, d.q_max, d.scale) == (13, 1, 31, 2.0)
    for kw in (dict(fixed=False), dict(compact=True), dict(compact=(2, 25)), dict(alpha=0.8), dict(beta=0.25),
               dict(path="on-chip")):
        with pytest.raises(ValueError):
            cls(H, 8, 16, 16, **{**ok, **kw})
    with pytest.raises(ValueError):
        cls(H, 8, 16, 16, layers=layers, path="onchip")              # fp32 has path="fused"
    with pytest.raises(ValueError):
        cls(H, 8, 16, 16, layers=layers, path="fused", fixed=True)   # as before
    assert cls(H, 8, 16, 16, **{**ok, "compact": False}).compact is None


@pytest.fixture(scope="module")
def fused_plan_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("asan") / "layered_fixed_fused_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "informationbottleneckdecodingldpc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "asan", "layered_fixed_fused_plan_check.cpp"), "-o", exe], check=True)
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


CODES = {
    # name: (code and layers, wide, codewords before the cap as the issue states them or None, max_batch)
    "wlan27": (lambda: fc.wlan(27), False, 84, 1),
    "wlan54": (lambda: fc.wlan(54), False, 42, 65),
    "wlan81": (lambda: fc.wlan(81), False, 28, 130),
    "mixed": (fc.mixed, False, None, 257),
    "dvbs2_small": (lambda: fc.small()[:2], False, None, 260),
    "wide_mixed": (wide_mixed, True, None, 64),
    "small30": (small30, True, None, 19),
    "n16200": (code16200, False, 3, 7),
    "n64800": (lambda: (lambda H: (H, codes.dvbs2_layers(H)))(codes.dvbs2_structured(seed=3)), False, 0, 70),
}


@pytest.mark.parametrize("name", list(CODES))
def test_fit_rule_and_plan_under_sanitizers(fused_plan_check, tmp_path, name):
    make, wide, uncapped, max_batch = CODES[name]
    H, layers = make()
    n_c, n_v = H.shape
    out = run_plan(fused_plan_check, H, layers, max_batch, tmp_path)
    ldn, cw_bytes, before_cap, cw = fit(n_v, n_c, wide)
    print(name, out)
    assert out["valid"] == 0 and out["wide"] == int(wide)
    assert (out["ldn"], out["cw_bytes"], out["uncapped"], out["cw_per_group"]) == (ldn, cw_bytes, before_cap, cw)
    if uncapped is not None:
        assert before_cap == uncapped
    assert out["buf_bytes"] == max_batch * ldn
    assert out["stage_tiles"] == -(-ldn // 64) * -(-max_batch // 64)
    if cw:
        assert out["lds_bytes"] == cw * cw_bytes <= LDS and out["ngroups"] == -(-max_batch // cw)
        assert out["n_tasks"] >= len([l for l in layers if len(l)])
    else:
        assert (out["lds_bytes"], out["ngroups"], out["n_tasks"]) == (0, 0, 0)
    if name == "dvbs2_small":
        assert cw_bytes == 19800 and before_cap == 8 and cw == 4
    if name == "small30":
        assert cw_bytes == 19800 and before_cap == 8 and cw == 4
    if name == "n16200":
        assert (n_c, n_v, len(layers), cw_bytes) == (9000, 16200, 25, 52200)
        assert sorted(set(np.diff(codes.canonical_csr(H).indptr).tolist())) == [5, 6]
        assert 4 * n_v + 12 * n_c == 172800 > LDS       # the fp32 fused kernel's codeword does not fit
    if name == "n64800":
        assert cw_bytes == 194400
