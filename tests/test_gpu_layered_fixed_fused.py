"""GPU: the fused on-chip kernel of the fixed-point layered min-sum decoder (ibl_layered_create_fixed_fused,
csrc/layered_kernels.hip layfix_fused / layfix_fused_wide and their staging kernels; engine.LayeredFixedDecoder
path="onchip") against the numpy integer restatement of the specification (tests/_layered_fixed_ref.py): outputs and
per-codeword iteration counts compared with np.array_equal, no tolerance. The inputs are those of
tests/_layered_fixed_census.py and tests/_layered_wide.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from informationbottleneckdecodingldpc_amd import _lib, codes
from tests import _layered_wide as lw
from tests._layered_fixed_census import (DEFAULT, FAMILIES, FAMILY_B, FAMILY_IMAX, awgn_llr, mixed, small, small_ref,
                                         wlan)
from tests._layered_fixed_ref import dequantise, fixed_decode, quantise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from informationbottleneckdecodingldpc_amd import engine as e
    return e


@pytest.fixture(scope="module")
def small_graph(engine):
    return engine.Graph(small()[0], "cuda:0")


def make(engine, graph, layers, imax, max_batch, params=DEFAULT, path="onchip"):
    a16, bq, qm, scale = params
    dec = engine.LayeredFixedDecoder(graph, layers, imax, max_batch, alpha16=a16, beta_q=bq, q_max=qm, scale=scale,
                                     path=path)
    if path == "onchip":
        c, ngroups, grid = dec.geometry(max_batch)
        assert dec.path_in_use == "fused" and c >= 1 and ngroups == -(-max_batch // c) and 1 <= grid <= ngroups
    return dec


def gpu_decode(dec, x, early, out_dtype=None):
    it = torch.full((x.shape[1],), -1, dtype=torch.int32, device=dec.device)
    out = dec.decode(torch.from_numpy(np.array(x, order="C")).to(dec.device), out_dtype=out_dtype, early_stop=early,
                     iters=it)
    return out.cpu().numpy(), it.cpu().numpy()


def check(dec, x, early, ref, what="", out_dtype=None):
    """ref: (out int8 integer units, iters). A float32 output is compared with the reference's division."""
    out, it = gpu_decode(dec, x, early, out_dtype)
    r_out, r_it = ref
    if out.dtype == np.float32:
        r_out = dequantise(r_out, dec.scale)
    print(f"{what} early={early} B={x.shape[1]} {x.dtype}->{out.dtype}: iters {np.bincount(r_it).tolist()}, iters "
          f"equal {np.array_equal(it, r_it)}, out mismatches {int((out != r_out).sum())}")
    assert out.dtype == r_out.dtype
    assert np.array_equal(it, r_it)
    assert np.array_equal(out, r_out)
    return out, it


@pytest.mark.parametrize("early", [True, False])
@pytest.mark.parametrize("imax", [1, 2, 10])
def test_small_batches(engine, small_graph, imax, early):
    """N = 5400, 10 layers, cw_bytes 19,800: one codeword, a group short of one wave, a whole group, a second group
    of one wave, and three groups with a ragged last one (B = 1, 3, 4, 5, 11), sliced from one reference."""
    H, layers, llr = small()
    probe = make(engine, small_graph, layers, imax, 64)
    c = probe.geometry(64)[0]
    assert c == 4                                   # floor(160 KiB / 19,800) = 8 fit; the cap is 4
    ref = small_ref(imax, early)
    dec = make(engine, small_graph, layers, imax, 2 * c + 3)
    for B in (1, c - 1, c, c + 1, 2 * c + 3):
        assert dec.geometry(B)[:2] == (c, -(-B // c)) and dec.geometry(B)[2] >= 1
        check(dec, llr[:, :B], early, (ref[0][:, :B], ref[1][:B]), f"imax={imax}")


def test_group_loop(engine):
    """WLAN N = 648: more groups than workgroups, so that a workgroup takes a second group, and a ragged last one."""
    H, layers = wlan(27)
    G = engine.Graph(H, "cuda:0")
    huge = 1 << 16
    dec = make(engine, G, layers, 5, huge)
    c, ngroups, grid = dec.geometry(huge)
    assert c == 4 and grid < ngroups              # the grid is the device's, not the batch's
    B = c * (grid + 1) + 3
    assert B <= huge
    g = dec.geometry(B)
    print("geometry", g, "B", B)
    assert g[0] == c and g[2] == grid and g[1] == grid + 2 > grid
    x = awgn_llr(648, B, 2.0, seed=21)
    ref = fixed_decode(H, layers, quantise(x), 5, *DEFAULT[:3])
    assert len(set(ref[1].tolist())) >= 3
    check(dec, x, True, ref, "group loop")


def test_waves_that_run_ahead(engine, small_graph):
    """Every second column noiseless: those waves finish after one iteration and start the next group's codeword
    while their neighbours are in mid-decode."""
    H, layers, awgn = small()
    c = 4
    B = 4 * c
    llr = np.array(awgn[:, :B])
    llr[:, 0::2] = np.float32(4.0)
    ref = fixed_decode(H, layers, quantise(llr), 10, *DEFAULT[:3])
    assert (ref[1][0::2] == 1).all() and ref[1][1::2].min() > 1
    dec = make(engine, small_graph, layers, 10, B)
    assert dec.geometry(B)[:2] == (c, 4)
    check(dec, llr, True, ref, "run ahead")


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("code", ["mixed", "wlan27"])
def test_edge_families(engine, code, family):
    """The per-layer test's matrix: the inputs of the CPU census on check degrees 2..16 and on WLAN Z = 27; B = 16,
    6 iterations, early stop on and off, input and output of the family's own dtype, every parameter set."""
    H, layers = mixed() if code == "mixed" else wlan(27)
    G = engine.Graph(H, "cuda:0")
    gen, params = FAMILIES[family]
    x = gen(H, FAMILY_B)
    for p in params:
        dec = make(engine, G, layers, FAMILY_IMAX, FAMILY_B, p)
        assert dec.wide is False
        for early in (True, False):
            ref = fixed_decode(H, layers, quantise(x, p[3]), FAMILY_IMAX, *p[:3], early_stop=early)
            check(dec, x, early, ref, f"{family} {code} {p}")


WIDE_B = 19


@pytest.mark.parametrize("params", lw.FIXED_PARAMS)
@pytest.mark.parametrize("code", ["wide_mixed", "small30"])
def test_wide(engine, code, params):
    """Check degrees 2..32 (greedy layers) and the degree-30 long-code shape (cw_bytes 19,800, 4 codewords a
    workgroup): B = 19 is four groups and a ragged fifth on small30."""
    if code == "small30":
        H, layers = lw.small30()
        imax, x = lw.SMALL30_IMAX, np.array(lw.small30_llr()[:, :WIDE_B])
    else:
        H, layers = lw.wide_mixed()
        imax, x = lw.CENSUS_IMAX, np.array(lw.wide_awgn(130)[:, :WIDE_B])
    dec = make(engine, engine.Graph(H, "cuda:0"), layers, imax, WIDE_B, params)
    assert dec.wide is True
    if code == "small30":
        assert dec.geometry(WIDE_B)[:2] == (4, 5)
    for early in (True, False):
        ref = fixed_decode(H, layers, quantise(x, params[3]), imax, *params[:3], early_stop=early)
        check(dec, x, early, ref, f"{code} {params}")


@pytest.mark.parametrize("scale", [2.0, 3.3])
def test_dtype_combinations(engine, small_graph, scale):
    """float32 / int8 in and out, all four, on one group and one wave more: the int8 input is the quantised float
    input with some of its -127 written as -128, the float32 output the int8 output divided by scale (3.3: neither
    the product nor the quotient is exact)."""
    H, layers, llr = small()
    B = 5
    p = (13, 0, 31, scale)
    dec = make(engine, small_graph, layers, 10, B, p)
    assert dec.geometry(B)[0] + 1 == B
    x = np.array(llr[:, :B])
    at = np.random.default_rng(3).choice(x.size, 12, replace=False)
    x.reshape(-1)[at] = np.float32(-100.0)          # beyond the quantiser's range at either scale: -127
    xq = quantise(x, scale)
    assert (xq.reshape(-1)[at] == -127).all()
    ref = fixed_decode(H, layers, xq, 10, *p[:3])
    assert len(set(ref[1].tolist())) >= 2
    x8 = np.array(xq)
    x8.reshape(-1)[at[::2]] = -128
    assert (x8 == -128).any() and np.array_equal(quantise(x8, scale), xq)
    for src in (x, x8):
        for dt in (torch.float32, torch.int8):
            check(dec, src, True, ref, f"scale={scale}", out_dtype=dt)
    with pytest.raises(ValueError):
        dec.decode(torch.zeros((5400, 2), dtype=torch.float64, device=dec.device))
    with pytest.raises(ValueError):
        dec.decode(torch.zeros((5400, 2), dtype=torch.float32, device=dec.device), out_dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def code16200():
    H = codes.dvbs2_structured(seed=9, n=16200, k=7200, groups_hi=5, deg_hi=11, deg_lo=3)
    return H, codes.dvbs2_layers(H)


def test_code_fp32_cannot_hold(engine):
    """9000 x 16200, 25 layers: 172,800 bytes a codeword in fp32 (refused by the fp32 fused kernel), 52,200 in fixed
    point, three codewords a workgroup. B = 7 at 3.0 dB with one noiseless column."""
    H, layers = code16200()
    assert H.shape == (9000, 16200) and len(layers) == 25
    G = engine.Graph(H, "cuda:0")
    with pytest.raises(_lib.IBLError) as e:
        engine.LayeredDecoder(G, layers, 6, 7, path="fused")
    assert f"rc={_lib.IBL_EUNSUPPORTED}" in str(e.value) and "172800" in str(e.value)
    dec = make(engine, G, layers, 6, 7)
    assert dec.geometry(7)[:2] == (3, 3)
    llr = awgn_llr(16200, 7, 3.0, seed=31, R=1 - 9000 / 16200)
    llr[:, 3] = np.float32(4.0)
    ref = fixed_decode(H, layers, quantise(llr), 6, *DEFAULT[:3])
    assert ref[1][3] == 1 and len(set(np.delete(ref[1], 3).tolist())) >= 2
    check(dec, llr, True, ref, "N = 16200")
    check(dec, llr, False, fixed_decode(H, layers, quantise(llr), 6, *DEFAULT[:3], early_stop=False), "N = 16200")


@pytest.fixture(scope="module")
def small_dec(engine, small_graph):
    return make(engine, small_graph, small()[1], 10, 65)


@pytest.mark.parametrize("dtype", [np.float32, np.int8])
def test_in_place_and_no_iters(small_dec, dtype):
    H, layers, llr = small()
    ref = small_ref(10, True)
    B = 19
    want = ref[0][:, :B] if dtype == np.int8 else dequantise(ref[0][:, :B])
    x = np.array(llr[:, :B]) if dtype == np.float32 else quantise(llr[:, :B])
    t = torch.from_numpy(x).to(small_dec.device)
    out = small_dec.decode(t.clone(), iters=None)
    assert np.array_equal(out.cpu().numpy(), want)
    it = torch.full((B,), -1, dtype=torch.int32, device=small_dec.device)
    same = small_dec.decode(t, out=t, iters=it)
    assert same is t
    assert np.array_equal(t.cpu().numpy(), want) and np.array_equal(it.cpu().numpy(), ref[1][:B])


def test_side_stream(small_dec):
    H, layers, llr = small()
    ref = small_ref(10, True)
    B = 19
    t = torch.from_numpy(np.array(llr[:, :B])).to(small_dec.device)
    it = torch.full((B,), -1, dtype=torch.int32, device=small_dec.device)
    torch.cuda.synchronize(small_dec.device)
    side = torch.cuda.Stream(device=small_dec.device)
    with torch.cuda.stream(side):
        out = small_dec.decode(t, out_dtype=torch.int8, iters=it)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref[0][:, :B]) and np.array_equal(it.cpu().numpy(), ref[1][:B])


def test_descending_reuse_and_batch_too_large(small_dec):
    """One decoder decodes B = 2c + 3, then c, then 1, columns from the far end of the batch: stale rows of the
    staging buffer and stale LDS of the wider decode do not leak."""
    H, layers, llr = small()
    ref = small_ref(10, True)
    c = small_dec.geometry(1)[0]
    for B in (2 * c + 3, c, 1):
        check(small_dec, llr[:, 260 - B:], True, (ref[0][:, 260 - B:], ref[1][260 - B:]), "reuse")
    t = torch.zeros((5400, 66), dtype=torch.float32, device=small_dec.device)
    with pytest.raises(_lib.IBLError) as e:
        small_dec.decode(t)
    assert f"rc={_lib.IBL_EINVAL}" in str(e.value)


def test_api(engine, small_dec, small_graph):
    L = _lib.load()
    f = ctypes.c_int32(-1)
    assert L.ibl_layered_is_fixed(small_dec._h, ctypes.byref(f)) == _lib.IBL_OK and f.value == 1
    assert small_dec.path_in_use == "fused" and small_dec.wide is False
    assert not hasattr(small_dec, "compaction")
    for every in (2, 0):
        assert L.ibl_layered_set_compaction(small_dec._h, every, 25) == _lib.IBL_EUNSUPPORTED
        assert L.ibl_last_error().decode() == "compaction is not built for the fixed-point decoder"
    n, ext = ctypes.c_int32(), ctypes.c_int32()
    assert L.ibl_layered_compaction_stats(small_dec._h, None, ctypes.byref(n), ctypes.byref(ext)) \
         == _lib.IBL_EUNSUPPORTED
    # the older entry point is what it was
    with pytest.raises(_lib.IBLError) as e:
        make(engine, small_graph, small()[1], 5, 8, path="fused")
    assert f"rc={_lib.IBL_EUNSUPPORTED}" in str(e.value) and "not built" in str(e.value)
    assert make(engine, small_graph, small()[1], 5, 8, path="auto").path_in_use == "passes"
    with pytest.raises(ValueError):
        engine.LayeredDecoder(small_graph, small()[1], 5, 8, path="onchip")
    for bad in [(17, 0, 31, 2.0), (13, 64, 31, 2.0), (13, 0, 0, 2.0), (13, 0, 31, 0.0), (13, 0, 31, float("nan"))]:
        with pytest.raises(_lib.IBLError) as e:
            make(engine, small_graph, small()[1], 5, 8, bad)
        assert f"rc={_lib.IBL_EINVAL}" in str(e.value), bad


def test_code_that_does_not_fit(engine):
    """DVB-S2-structured N = 64800 rate 1/2: 64800 + 4 x 32400 = 194,400 bytes a codeword."""
    H = codes.dvbs2_structured(seed=3)
    with pytest.raises(_lib.IBLError) as e:
        make(engine, engine.Graph(H, "cuda:0"), codes.dvbs2_layers(H), 3, 8)
    msg = str(e.value)
    assert f"rc={_lib.IBL_EUNSUPPORTED}" in msg and "194400" in msg and "163840" in msg and "160 KiB" in msg


def test_equals_the_per_layer_decoder(engine, small_graph):
    """small() at B = 65: out and iters of the per-layer fixed-point kernels on the same device."""
    H, layers, llr = small()
    x = llr[:, :65]
    for early in (True, False):
        a = gpu_decode(make(engine, small_graph, layers, 10, 65), x, early)
        b = gpu_decode(make(engine, small_graph, layers, 10, 65, path="passes"), x, early)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        ref = small_ref(10, early)
        assert np.array_equal(a[0], dequantise(ref[0][:, :65])) and np.array_equal(a[1], ref[1][:65])


def test_drop_in_class_and_ber_driver():
    """Min_Sum_Layered_Decoder_class_irregular(fixed=True, path="onchip") through ber.run_ber: the errors of the
    reference decoding the same Philox channel stream."""
    import informationbottleneckdecodingldpc_amd as pkg
    from informationbottleneckdecodingldpc_amd.awgn_quantizer import AWGN_Channel_Quantizer
    from informationbottleneckdecodingldpc_amd.ber import BERConfig, run_ber
    from informationbottleneckdecodingldpc_amd.engine import philox_blocks
    H, layers, _ = small()
    N = H.shape[1]
    cls = pkg.Min_Sum_Layered_Decoder_class_irregular
    for kw in (dict(fixed=False), dict(compact=True), dict(alpha=0.8)):
        with pytest.raises(ValueError):
            cls(H, 8, 16, 64, **{"layers": layers, "alpha": 0.8125, "path": "onchip", "fixed": True, **kw})
    dec = cls(H, 8, 16, 64, layers=layers, alpha=0.8125, beta=0.5, path="onchip", fixed=True)
    assert (dec.alpha16, dec.beta_q, dec.q_max, dec.scale) == (13, 1, 31, 2.0)
    B, nb = 64, 2
    cfg = BERConfig(EbN0_dB_start=1.5, EbN0_dB_max_value=1.5, min_errors=10 ** 9, msg_at_time=B, max_blocks=nb * B,
                    seed=5, llr_dtype=torch.float32)
    r = run_ber(dec, cfg)
    assert r.blocks == [nb * B] and dec._dec.path_in_use == "fused"
    q = AWGN_Channel_Quantizer(10 ** (-1.5 / 10) / (2 * dec.R_c), cfg.AD_max_abs, cfg.cardinality_T_channel,
                               cfg.cardinality_Y_channel, seed=5)
    q.init_OpenCL_quanti(N, B, return_buffer_only=True)
    want = 0
    for g in range(nb):
        q.offset = g * philox_blocks(N, B)
        ch = q.quantize_direct_OpenCL_LLR(N, B, dtype=torch.float32).cpu().numpy()
        want += int((fixed_decode(H, layers, quantise(ch), 8, 13, 1, 31)[0][:dec.data_len] < 0).sum())
    print("BER point: errors", r.errors[0], "reference", want)
    assert want > 0 and r.errors[0] == float(want)
