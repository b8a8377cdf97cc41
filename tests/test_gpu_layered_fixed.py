"""GPU: the fixed-point layered min-sum decoder (ibl_layered_create_fixed, csrc/layered_kernels.hip layfix_*)
against the numpy integer restatement of the specification (tests/_layered_fixed_ref.py): outputs and per-codeword
iteration counts compared with np.array_equal, no tolerance. The inputs are those of tests/_layered_fixed_census.py
(tests/test_cpu_layered_fixed.py holds them to the arithmetic's edges)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from informationbottleneckdecodingldpc_amd import _lib, codes
from tests._layered_fixed_census import (DEFAULT, FAMILIES, FAMILY_B, FAMILY_IMAX, awgn_llr, mixed, small, small_ref,
                                         wlan)
from tests._layered_fixed_ref import dequantise, fixed_decode, quantise

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 260)


@pytest.fixture(scope="module")
def engine():
    from informationbottleneckdecodingldpc_amd import engine as e
    return e


@pytest.fixture(scope="module")
def small_graph(engine):
    return engine.Graph(small()[0], "cuda:0")


def make(engine, graph, layers, imax, max_batch, params=DEFAULT, path="auto"):
    a16, bq, qm, scale = params
    return engine.LayeredFixedDecoder(graph, layers, imax, max_batch, alpha16=a16, beta_q=bq, q_max=qm, scale=scale,
                                      path=path)


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
def test_small_long_code(engine, small_graph, imax, early):
    """Batches with one lane partly filled, at a boundary of the 64-codeword masks, at a tile of 256 and with a
    second tile of 1 and of 4 codewords, sliced from one 260-column reference."""
    H, layers, llr = small()
    dec = make(engine, small_graph, layers, imax, 260)
    assert dec.path_in_use == "passes" and dec.geometry(260) == (0, 0, 0)
    ref = small_ref(imax, early)
    for B in BATCHES:
        check(dec, llr[:, :B], early, (ref[0][:, :B], ref[1][:B]), f"imax={imax}")


def test_small_input_spreads_the_stops():
    H, layers, llr = small()
    out, it = small_ref(10, True)
    hist = np.bincount(it, minlength=11)
    print("reference iters histogram:", {i: int(c) for i, c in enumerate(hist) if c})
    assert (hist > 0).sum() >= 4
    unconverged = ((sp.csr_matrix(H) @ (out < 0).astype(np.int64)) % 2 != 0).any(axis=0)
    assert (unconverged & (it == 10)).any()


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("code", ["mixed", "wlan27"])
def test_edge_families(engine, code, family):
    """The inputs of the CPU census on check degrees 2..16 (greedy layers of uneven size) and on WLAN Z = 27; B = 16,
    6 iterations, early stop on and off, input and output of the family's own dtype."""
    H, layers = mixed() if code == "mixed" else wlan(27)
    G = engine.Graph(H, "cuda:0")
    gen, params = FAMILIES[family]
    x = gen(H, FAMILY_B)
    for p in params:
        dec = make(engine, G, layers, FAMILY_IMAX, FAMILY_B, p, path="passes")
        for early in (True, False):
            ref = fixed_decode(H, layers, quantise(x, p[3]), FAMILY_IMAX, *p[:3], early_stop=early)
            check(dec, x, early, ref, f"{family} {code} {p}")


@pytest.mark.parametrize("scale", [2.0, 3.3])
def test_dtype_combinations(engine, small_graph, scale):
    """float32 / int8 in and out, all four: the int8 input is the quantised float input, the float32 output the
    int8 output divided by scale (3.3: neither the product nor the quotient is exact)."""
    H, layers, llr = small()
    B = 65
    p = (13, 0, 31, scale)
    dec = make(engine, small_graph, layers, 10, B, p)
    x = np.array(llr[:, :B])
    xq = quantise(x, scale)
    ref = fixed_decode(H, layers, xq, 10, *p[:3])
    for src in (x, xq):
        for dt in (torch.float32, torch.int8):
            check(dec, src, True, ref, f"scale={scale}", out_dtype=dt)
    with pytest.raises(ValueError):
        dec.decode(torch.zeros((5400, 2), dtype=torch.float64, device=dec.device))
    with pytest.raises(ValueError):
        dec.decode(torch.zeros((5400, 2), dtype=torch.float32, device=dec.device), out_dtype=torch.int32)


@pytest.mark.parametrize("quiet", [256, 64])
def test_skipping(engine, small_graph, quiet):
    """Columns 0..quiet-1 noiseless (+4.0) finish after iteration 1, the others run on: 256 leaves a whole first tile
    to be skipped beside a second tile of 4 codewords, 64 a finished mask word inside a running tile. A finished
    codeword written again, or a skipped lane that was needed, shows in out or iters."""
    H, layers, awgn = small()
    llr = np.array(awgn)
    llr[:, :quiet] = np.float32(4.0)
    ref = fixed_decode(H, layers, quantise(llr), 10, *DEFAULT[:3])
    assert (ref[1][:quiet] == 1).all() and ref[1][quiet:].min() > 1
    dec = make(engine, small_graph, layers, 10, 260)
    check(dec, llr, True, ref, f"skipping {quiet}")


@pytest.fixture(scope="module")
def small_dec(engine, small_graph):
    return make(engine, small_graph, small()[1], 10, 260)


@pytest.mark.parametrize("dtype", [np.float32, np.int8])
def test_in_place_and_no_iters(small_dec, dtype):
    H, layers, llr = small()
    ref = small_ref(10, True)
    want = ref[0][:, :65] if dtype == np.int8 else dequantise(ref[0][:, :65])
    x = np.array(llr[:, :65]) if dtype == np.float32 else quantise(llr[:, :65])
    t = torch.from_numpy(x).to(small_dec.device)
    out = small_dec.decode(t.clone(), iters=None)
    assert np.array_equal(out.cpu().numpy(), want)
    it = torch.full((65,), -1, dtype=torch.int32, device=small_dec.device)
    same = small_dec.decode(t, out=t, iters=it)
    assert same is t
    assert np.array_equal(t.cpu().numpy(), want) and np.array_equal(it.cpu().numpy(), ref[1][:65])


def test_side_stream(small_dec):
    H, layers, llr = small()
    ref = small_ref(10, True)
    t = torch.from_numpy(np.array(llr[:, :65])).to(small_dec.device)
    it = torch.full((65,), -1, dtype=torch.int32, device=small_dec.device)
    torch.cuda.synchronize(small_dec.device)
    side = torch.cuda.Stream(device=small_dec.device)
    with torch.cuda.stream(side):
        out = small_dec.decode(t, out_dtype=torch.int8, iters=it)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref[0][:, :65]) and np.array_equal(it.cpu().numpy(), ref[1][:65])


def test_descending_reuse_and_batch_too_large(small_dec):
    """One decoder decodes B = 260, then 64, then 1, columns from the far end of the batch: stale rows, masks and
    counters of the wider decode do not leak."""
    H, layers, llr = small()
    ref = small_ref(10, True)
    for B in (260, 64, 1):
        check(small_dec, llr[:, 260 - B:], True, (ref[0][:, 260 - B:], ref[1][260 - B:]), "reuse")
    t = torch.zeros((5400, 261), dtype=torch.float32, device=small_dec.device)
    with pytest.raises(_lib.IBLError) as e:
        small_dec.decode(t)
    assert f"rc={_lib.IBL_EINVAL}" in str(e.value)


def test_api(engine, small_graph):
    H, layers, _ = small()
    with pytest.raises(_lib.IBLError) as e:
        make(engine, small_graph, layers, 5, 8, path="fused")
    assert f"rc={_lib.IBL_EUNSUPPORTED}" in str(e.value) and "not built" in str(e.value)
    with pytest.raises(ValueError):
        make(engine, small_graph, layers, 5, 8, path="hbm")
    for bad in [(17, 0, 31, 2.0), (-1, 0, 31, 2.0), (13, 64, 31, 2.0), (13, 0, 0, 2.0), (13, 0, 64, 2.0),
                (13, 0, 31, 0.0), (13, 0, 31, float("inf")), (13, 0, 31, float("nan"))]:
        with pytest.raises(_lib.IBLError) as e:
            make(engine, small_graph, layers, 5, 8, bad)
        assert f"rc={_lib.IBL_EINVAL}" in str(e.value), bad
    # a code the fused kernel would fit still runs the per-layer kernels
    H27, l27 = wlan(27)
    dec = make(engine, engine.Graph(H27, "cuda:0"), l27, 5, 8, path="auto")
    assert dec.path_in_use == "passes"


@pytest.mark.parametrize("early", [True, False])
def test_full_size(engine, early):
    """DVB-S2-structured N = 64800 rate 1/2, its 90 residue layers: 69 columns of AWGN at 1.0 dB and one noiseless
    column; 3 iterations."""
    H = codes.dvbs2_structured(seed=3)
    layers = codes.dvbs2_layers(H)
    assert len(layers) == 90
    llr = awgn_llr(64800, 70, 1.0, seed=17)
    llr[:, 41] = np.float32(4.0)
    dec = make(engine, engine.Graph(H, "cuda:0"), layers, 3, 70)
    ref = fixed_decode(H, layers, quantise(llr), 3, *DEFAULT[:3], early_stop=early)
    assert ref[1][41] == (1 if early else 3)
    check(dec, llr, early, ref, "full size")


def test_drop_in_class_and_ber_driver():
    """Min_Sum_Layered_Decoder_class_irregular(fixed=True) through ber.run_ber: the errors of the reference decoding
    the same Philox channel stream."""
    import informationbottleneckdecodingldpc_amd as pkg
    from informationbottleneckdecodingldpc_amd.awgn_quantizer import AWGN_Channel_Quantizer
    from informationbottleneckdecodingldpc_amd.ber import BERConfig, run_ber
    from informationbottleneckdecodingldpc_amd.engine import philox_blocks
    H, layers, _ = small()
    N = H.shape[1]
    cls = pkg.Min_Sum_Layered_Decoder_class_irregular
    for kw in (dict(path="fused"), dict(alpha=0.8), dict(alpha=1.0625), dict(beta=0.25), dict(beta=32.0)):
        with pytest.raises(ValueError):
            cls(H, 8, 16, 64, **{"layers": layers, "alpha": 0.8125, "path": "passes", "fixed": True, **kw})
    dec = cls(H, 8, 16, 64, layers=layers, alpha=0.8125, beta=0.5, path="passes", fixed=True)
    assert (dec.alpha16, dec.beta_q, dec.q_max, dec.scale) == (13, 1, 31, 2.0)
    B, nb = 64, 2
    cfg = BERConfig(EbN0_dB_start=1.5, EbN0_dB_max_value=1.5, min_errors=10 ** 9, msg_at_time=B, max_blocks=nb * B,
                    seed=5, llr_dtype=torch.float32)
    r = run_ber(dec, cfg)
    assert r.blocks == [nb * B] and dec._dec.path_in_use == "passes"
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
