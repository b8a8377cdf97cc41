"""CPU: the fixed-point layered min-sum decoder without a device — the two restatements of its specification
against each other (tests/_layered_fixed_ref.py), the census that holds the GPU tests' inputs to the arithmetic's
edges (tests/_layered_fixed_census.py), the specification's error rate beside the fp32 decoder's, the C ABI's
refusals, and the host geometry (csrc/layered_plan.h fix_*) under AddressSanitizer and UndefinedBehaviorSanitizer
as a stand-alone program (tests/asan/layered_fixed_plan_check.cpp; nothing loaded into Python is sanitized)."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from informationbottleneckdecodingldpc_amd import codes
from tests import _layered_fixed_census as fc
from tests._layered_fixed_ref import dequantise, fixed_decode, fixed_decode_scalar, quantise
from tests._layered_ref import layered_decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("early", [True, False])
@pytest.mark.parametrize("code", ["mixed", "wlan27"])
def test_scalar_equals_vectorised(code, early):
    """The plain-Python restatement and the numpy one agree exactly on every family's first parameter sets (three
    codewords each)."""
    H, layers = fc.mixed() if code == "mixed" else fc.wlan(27)
    for name, (gen, params) in fc.FAMILIES.items():
        x = gen(H, fc.FAMILY_B)[:, 5:8]
        for p in params[:2]:
            P0 = quantise(x, p[3])
            a = fixed_decode(H, layers, P0, 4, *p[:3], early_stop=early)
            b = fixed_decode_scalar(H, layers, P0, 4, *p[:3], early_stop=early)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, p)
            assert a[0].dtype == np.int8 and a[1].dtype == np.int32


@pytest.fixture(scope="module")
def census():
    """family -> code -> parameters -> counts, with the early stop (the GPU tests' B and iterations)."""
    res = {}
    for name, (gen, params) in fc.FAMILIES.items():
        for code in ("mixed", "wlan27"):
            H, layers = fc.mixed() if code == "mixed" else fc.wlan(27)
            x = gen(H, fc.FAMILY_B)
            for p in params:
                res.setdefault(name, {}).setdefault(code, {})[p] = fc.fixed_census(
                    H, layers, quantise(x, p[3]), fc.FAMILY_IMAX, *p[:3])[2]
    return res


def test_edge_census(census):
    """Every edge of the arithmetic is reached by the inputs the GPU decodes, on both codes."""
    for code in ("mixed", "wlan27"):
        strong = census["strong"][code]
        c = strong[(13, 2, 31, 2.0)]
        print(code, "strong (13, 2, 31):", {k: v for k, v in c.items() if k != "degrees"})
        assert c["p_sat_hi"] > 0 and c["p_sat_lo"] > 0            # P saturating at +127 and at -127
        assert c["t_hi"] > 0 and c["t_lo"] > 0                    # T outside +-q_max on both sides
        assert c["beta_floor"] > 0                                # a magnitude floored to 0 by beta_q
        c1 = strong[(16, 0, 1, 2.0)]
        assert c1["t_hi"] > 0 and c1["t_lo"] > 0 and c1["m1_eq_m2"] > 0          # q_max = 1
        c63 = strong[(16, 0, 63, 3.3)]
        assert c63["t_hi"] > 0 and c63["t_lo"] > 0 and c63["p_sat_hi"] > 0 and c63["p_sat_lo"] > 0   # q_max = 63
        for fam in ("noisy", "quarters", "int8"):
            c = census[fam][code][fc.DEFAULT]
            print(code, fam, "default:", {k: v for k, v in c.items() if k != "degrees"})
            assert c["tie_first_not_last"] > 0 and c["m1_eq_m2"] > 0 and c["t_zero"] > 0
            assert c["half_up"] > 0                               # (13 mag + 8) >> 4 with 13 mag = 8 mod 16
        assert census["quarters"][code][(13, 3, 31, 2.0)]["beta_floor"] > 0
    assert census["noisy"]["mixed"][fc.DEFAULT]["degrees"] == set(range(2, 17))   # every check degree 2..16
    used = [p for _, params in fc.FAMILIES.values() for p in params]
    assert {p[0] for p in used} >= {0, 13, 16} and {p[2] for p in used} >= {1, 31, 63}
    assert any(p[3] == 3.3 for p in used)


def test_quantiser_edges():
    """Products exactly on a half rounded to even in both directions, the float clamp on both sides, an int8 input
    of -128, a scale that is no power of two, and the output division."""
    for code in ("mixed", "wlan27"):
        H, _ = fc.mixed() if code == "mixed" else fc.wlan(27)
        q = fc.FAMILIES["quarters"][0](H, fc.FAMILY_B)
        down, up = fc.half_products(q, 2.0)
        print(code, "ties rounded down / up to even:", down, up)
        assert down > 0 and up > 0
        s = fc.FAMILIES["strong"][0](H, fc.FAMILY_B)
        for scale in (2.0, 3.3):
            P = quantise(s, scale)
            assert P.max() == 127 and P.min() == -127
            assert (np.abs(s.astype(np.float32) * np.float32(scale)) > 127).any()
        i8 = fc.FAMILIES["int8"][0](H, fc.FAMILY_B)
        assert i8.dtype == np.int8 and (i8 == -128).any() and (i8 == 127).any()
        assert quantise(i8).min() == -127 and np.array_equal(quantise(i8)[i8 > -128], i8[i8 > -128])
    assert quantise(np.array([[0.25, 0.75, -0.25, -0.75, 1.25]], np.float32)).tolist() == [[0, 2, 0, -2, 2]]
    assert quantise(np.array([[np.inf, -np.inf, 63.4, 1e30]], np.float32)).tolist() == [[127, -127, 127, 127]]
    x = dequantise(np.arange(-127, 128, dtype=np.int8), 3.3)
    assert x.dtype == np.float32 and np.array_equal(x, (np.arange(-127, 128) / np.float64(np.float32(3.3))).astype(np.float32))


def test_specification_sanity():
    """The small DVB-S2-structured code at 2.0 dB, 300 codewords, 10 iterations, defaults (13, 0, 31, 2.0): frame
    errors at most 1.5 x the fp32 layered reference's at alpha = 0.8125 on the same input. The prototype the
    specification was drafted with gave 32 frame errors against 41 and the iteration histogram below."""
    H, layers, llr = fc.small(300)
    out, it = fc.small_ref(10, True, 300)
    fe = int((out[:1800] < 0).any(axis=0).sum())
    fe_all = int((out < 0).any(axis=0).sum())
    ref = layered_decode(H, layers, llr, 10, 0.8125, 0.0)[0]
    fe32 = int((ref < 0).any(axis=0).sum())
    hist = np.bincount(it, minlength=11).tolist()
    print("fixed frame errors", fe_all, "(information part", fe, ") fp32", fe32, "iters", hist)
    assert fe_all <= 1.5 * fe32
    assert (fe_all, fe32) == (32, 41)
    assert hist == [0, 0, 0, 11, 83, 77, 55, 25, 8, 6, 35]


def test_capi_without_a_device():
    """The new names are exported and declared, and every refusal that needs no graph is given without one."""
    from informationbottleneckdecodingldpc_amd import _build, _lib
    assert {"ibl_layered_create_fixed", "ibl_layered_is_fixed"} <= set(_lib.EXPORTS) and _lib.IBL_I8 == 5
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    L = _lib.load()
    with open(os.path.join(ROOT, "include", "ibldpc.h")) as fh:
        header = fh.read()
    assert "int ibl_layered_create_fixed(" in header and "IBL_I8 = 5" in header
    assert "Layered min-sum, fixed point" in header
    ptr, chk = np.zeros(2, np.int32), np.zeros(1, np.int32)

    def create(imax=5, a16=13, bq=0, qm=31, scale=2.0, mb=8, path=_lib.IBL_PATH_AUTO, out=True):
        h = ctypes.c_void_p(1)
        rc = L.ibl_layered_create_fixed(None, 1, ptr, chk, imax, a16, bq, qm, scale, mb, path,
                                        ctypes.byref(h) if out else None)
        assert not out or h.value is None
        return rc, L.ibl_last_error().decode()

    for kw in (dict(a16=-1), dict(a16=17), dict(bq=-1), dict(bq=64), dict(qm=0), dict(qm=64), dict(scale=0.0),
               dict(scale=-2.0), dict(scale=float("inf")), dict(scale=float("nan")), dict(imax=0), dict(mb=0),
               dict(path=3), dict(out=False)):
        rc, msg = create(**kw)
        assert rc == _lib.IBL_EINVAL, (kw, msg)
    rc, msg = create(path=_lib.IBL_PATH_FUSED)
    assert rc == _lib.IBL_EUNSUPPORTED and "fixed-point fused kernel is not built" in msg
    for path in (_lib.IBL_PATH_AUTO, _lib.IBL_PATH_PASSES):      # in range: the next thing missing is the graph
        rc, msg = create(path=path, a16=0, bq=63, qm=63)
        assert rc == _lib.IBL_EINVAL and "graph is NULL" in msg
    f = ctypes.c_int32()
    assert L.ibl_layered_is_fixed(None, ctypes.byref(f)) == _lib.IBL_EINVAL


def test_drop_in_class_refusals():
    import informationbottleneckdecodingldpc_amd as pkg
    cls = pkg.Min_Sum_Layered_Decoder_class_irregular
    H, layers = fc.wlan(27)
    ok = dict(layers=layers, alpha=0.8125, beta=0.5, path="auto", fixed=True)
    d = cls(H, 8, 16, 16, **ok)
    assert (d.alpha16, d.beta_q, d.q_max, d.scale) == (13, 1, 31, 2.0)
    d = cls(H, 8, 16, 16, **{**ok, "scale": 4.0, "beta": 0.25, "q_max": 15})
    assert (d.alpha16, d.beta_q, d.q_max, d.scale) == (13, 1, 15, 4.0)
    for kw in (dict(path="fused"), dict(alpha=0.8), dict(alpha=1.0625), dict(alpha=-0.0625), dict(beta=0.25),
               dict(beta=32.0), dict(beta=-0.5)):
        with pytest.raises(ValueError):
            cls(H, 8, 16, 16, **{**ok, **kw})
    assert cls(H, 8, 16, 16, layers=layers, alpha=0.8).fixed is False      # the defaults leave fp32 as it was


@pytest.fixture(scope="module")
def fixed_plan_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("asan") / "layered_fixed_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "informationbottleneckdecodingldpc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "asan", "layered_fixed_plan_check.cpp"), "-o", exe], check=True)
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


@pytest.mark.parametrize("name,max_batch", [("dvbs2_small", 260), ("dvbs2_small", 256), ("wlan27", 1), ("mixed", 257)])
def test_fixed_plan_under_sanitizers(fixed_plan_check, tmp_path, name, max_batch):
    if name == "dvbs2_small":
        H, layers, _ = fc.small()
    else:
        H, layers = fc.wlan(27) if name == "wlan27" else fc.mixed()
    A = codes.canonical_csr(H)
    n_c, n_v = A.shape
    out = run_plan(fixed_plan_check, A, layers, max_batch, tmp_path)
    t64, t256 = -(-max_batch // 64), -(-max_batch // 256)
    ldb = 256 * t256
    assert out["valid"] == 0 and out["n_layers"] == len(layers)
    assert (out["ntiles"], out["ntiles4"], out["ldb"], out["mask_words"]) == (t64, t256, ldb, 4 * t256)
    # a wave item per (check of the layer, tile of 256 codewords), four items a workgroup
    assert out["layer_grids"] == [-(-len(l) * t256 // 4) for l in layers]
    assert out["bytes_P"] == n_v * ldb and out["bytes_state"] == 4 * n_c * ldb and out["bytes_mask"] == 32 * t256
    assert out["bytes_bits"] == 8 * n_v * t64
    assert out["bytes_total"] == (n_v + 4 * n_c) * ldb + 64 * t256 + 4 + 8 * n_v * t64
