"""GPU: the layered normalised / offset min-sum decoder (ibl_layered_*, csrc/layered_kernels.hip) against the
numpy float32 restatement of its specification (tests/_layered_ref.py): outputs equal as values
(np.array_equal: -0.0 equals +0.0) and per-codeword iteration counts exactly. Continuous AWGN LLRs never tie,
cancel, saturate or go subnormal: the input families of tests/_layered_census.py do (tests/test_cpu_layered.py
holds them to it), and the reference itself is pinned there by an independent scalar restatement."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from informationbottleneckdecodingldpc_amd import _lib, codes
from tests._codes import mixed_code
from tests._layered_census import (AB, FAMILIES, FAMILY_B, FAMILY_IMAX, MIXED_BATCH_COLUMNS, awgn_llr, mixed,
                                   mixed_batch_llr, quantised_llr, wlan)
from tests._layered_ref import layered_decode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from informationbottleneckdecodingldpc_amd import engine as e
    return e


def gpu_decode(dec, llr, early):
    it = torch.full((llr.shape[1],), -1, dtype=torch.int32, device=dec.device)
    out = dec.decode(torch.from_numpy(np.ascontiguousarray(llr)).to(dec.device), early_stop=early, iters=it)
    return out.cpu().numpy(), it.cpu().numpy()


def check(dec, H, layers, llr, imax, a, b, early, ref=None, cols=None, llr_max=150.0):
    """Decode on the GPU, compare (the columns `cols` of) out and iters with the reference; -> the GPU's."""
    out, it = gpu_decode(dec, llr, early)
    if ref is None:
        sel = llr if cols is None else llr[:, cols]
        ref = layered_decode(H, layers, sel, imax, a, b, llr_max, early_stop=early)
    if cols is not None:
        out, it = out[:, cols], it[cols]
    r_out, r_it = ref
    print(f"imax={imax} alpha={a} beta={b} early={early} B={llr.shape[1]}: iters {np.bincount(r_it).tolist()}, "
          f"iters equal {np.array_equal(it, r_it)}, out mismatches {int((out != r_out).sum())}")
    assert np.array_equal(it, r_it)
    assert np.array_equal(out, r_out)
    return out, it


@pytest.mark.parametrize("ab", AB)
@pytest.mark.parametrize("Z", [27, 81])
def test_smallest_shapes(engine, Z, ab):
    """A layer narrower than a wave (Z = 27) and one spanning two waves (Z = 81); batches of 1, 5 and one more
    than a workgroup's codewords (ragged groups); 1, 2 and 10 iterations; early stop on and off."""
    H, layers = wlan(Z)
    a, b = ab
    G = engine.Graph(H, "cuda:0")
    for imax in (1, 2, 10):
        dec = engine.LayeredDecoder(G, layers, imax, 64, alpha=a, beta=b)
        cw = dec.geometry(1)[0]
        assert 1 <= cw <= 8 and dec.geometry(cw + 1)[1:] == (2, 2)
        llr = awgn_llr(H.shape[1], cw + 1, 1.5, seed=100 + Z)
        for early in (True, False):
            # codewords decode independently: one reference for the widest batch serves the narrower ones
            ref = layered_decode(H, layers, llr, imax, a, b, early_stop=early)
            for B in (1, 5, cw + 1):
                check(dec, H, layers, llr[:, :B], imax, a, b, early, ref=(ref[0][:, :B], ref[1][:B]))


def test_irregular_non_qc(engine):
    """Check degrees 2..16 (every degree body), greedy layers of uneven sizes, B = 9."""
    H = mixed_code(np.arange(2, 17), np.array([2, 3, 3, 4, 6]), 400, seed=5)
    deg = np.diff(sp.csr_matrix(H).indptr)
    assert set(deg.tolist()) == set(range(2, 17))
    layers = codes.greedy_layers(H)
    codes.validate_layers(H, layers)
    assert len(set(len(l) for l in layers)) > 2
    G = engine.Graph(H, "cuda:0")
    llr = awgn_llr(H.shape[1], 9, 3.0, seed=11)
    for (a, b), early in (((0.8125, 0.25), True), ((1.0, 0.0), False)):
        dec = engine.LayeredDecoder(G, layers, 6, 9, alpha=a, beta=b)
        check(dec, H, layers, llr, 6, a, b, early)


def test_group_loop(engine):
    """Every workgroup decodes a second and a third group and the batch ends in a ragged group of one codeword:
    64 columns spread over the batch, the last three included."""
    H, layers = wlan(27)
    G = engine.Graph(H, "cuda:0")
    probe = engine.LayeredDecoder(G, layers, 5, 8)
    cw = probe.geometry(1)[0]
    grid_full = probe.geometry(8)[2]
    # the full grid: blocks per CU x CUs, reached once ngroups exceeds it
    big = engine.LayeredDecoder(G, layers, 5, 20000)
    grid = big.geometry(20000)[2]
    B = cw * (2 * grid + 1) + 1
    assert grid_full >= 1
    if B > 20000:
        pytest.skip(f"B = {B} codewords (cw_per_group {cw}, grid {grid}) exceeds 20,000")
    assert big.geometry(B) == (cw, 2 * grid + 2, grid)
    llr = awgn_llr(H.shape[1], B, 2.0, seed=3)
    # 64 columns: 55 spread over the first and second rounds of groups, and the cw + 1 codewords of the third
    # round (workgroup 0's third group and the ragged last group of one codeword)
    third = 2 * cw * grid
    cols = np.unique(np.concatenate([np.linspace(0, third - 1, 64 - (B - third)).astype(np.int64),
                                     np.arange(third, B)]))
    assert cols.size == 64 and (cols >= cw * grid).sum() > 20 and (cols >= third).sum() == cw + 1
    check(big, H, layers, llr, 5, 1.0, 0.0, True, cols=cols)


def test_per_codeword_stop(engine):
    """N = 1944 at 2.0 dB: codewords of one batch stop after different numbers of iterations and one never
    converges; out and iters equal the reference for each."""
    H, layers = wlan(81)
    llr = awgn_llr(1944, 64, 2.0, seed=7)
    ref = layered_decode(H, layers, llr, 10, 1.0, 0.0)
    hist = np.bincount(ref[1], minlength=11)
    print("reference iters histogram:", {i: int(c) for i, c in enumerate(hist) if c})
    assert (hist > 0).sum() >= 4
    x = (ref[0] < 0).astype(np.int64)
    unconverged = ((sp.csr_matrix(H) @ x) % 2 != 0).any(axis=0)
    assert (unconverged & (ref[1] == 10)).any()
    dec = engine.LayeredDecoder(engine.Graph(H, "cuda:0"), layers, 10, 64)
    check(dec, H, layers, llr, 10, 1.0, 0.0, True, ref=ref)


def test_api_edges(engine):
    H, layers = wlan(27)
    G = engine.Graph(H, "cuda:0")
    with pytest.raises(_lib.IBLError) as e:
        engine.LayeredDecoder(G, layers, 5, 8, precision=torch.float64)
    assert f"rc={_lib.IBL_EUNSUPPORTED}" in str(e.value)
    Hd = codes.dvbs2_structured(seed=3, n=64800, k=32400)
    q = Hd.shape[0] // 360
    res = [np.arange(r, Hd.shape[0], q) for r in range(q)]   # the residue classes mod q are valid layers
    codes.validate_layers(Hd, res)
    with pytest.raises(_lib.IBLError) as e:
        engine.LayeredDecoder(engine.Graph(Hd, "cuda:0"), res, 5, 8)
    assert f"rc={_lib.IBL_EUNSUPPORTED}" in str(e.value) and "fit" in str(e.value)
    with pytest.raises(_lib.IBLError) as e:   # a check listed twice
        engine.LayeredDecoder(G, [list(l) for l in layers[:-1]] + [list(layers[-1]) + [0]], 5, 8)
    assert f"rc={_lib.IBL_EINVAL}" in str(e.value) and "check 0 is listed twice" in str(e.value)


def test_drop_in_class_and_ber_driver():
    import informationbottleneckdecodingldpc_amd as pkg
    from informationbottleneckdecodingldpc_amd.awgn_quantizer import AWGN_Channel_Quantizer
    from informationbottleneckdecodingldpc_amd.ber import BERConfig, decoder_kind, run_ber
    from informationbottleneckdecodingldpc_amd.engine import philox_blocks
    H, layers = wlan(27)
    N = H.shape[1]
    cls = pkg.Min_Sum_Layered_Decoder_class_irregular
    dec = cls(H, 8, 16, 16, Z=27, alpha=0.75)
    assert decoder_kind(dec) == "minsum" and len(dec.layers) == 12
    greedy = cls(H, 8, 16, 16)
    assert [sorted(l.tolist()) for l in greedy.layers] == [sorted(l.tolist()) for l in layers]
    llr = awgn_llr(N, 16, 2.0, seed=9)
    ref = layered_decode(H, layers, llr, 8, 0.75, 0.0)
    out = dec.decode_OpenCL_min_sum(llr)                       # numpy in, numpy out
    assert isinstance(out, np.ndarray) and np.array_equal(out, ref[0])
    assert np.array_equal(dec.last_iterations.cpu().numpy(), ref[1])
    buf = dec.decode_OpenCL_min_sum(torch.from_numpy(llr).cuda(), buffer_in=True, return_buffer=True)
    assert isinstance(buf, torch.Tensor) and np.array_equal(buf.cpu().numpy(), ref[0])
    assert dec.return_errors_all_zero(buf) == float((ref[0][:dec.data_len] < 0).sum())
    bad = llr.copy()
    bad[3, 2] = np.inf
    with pytest.raises(ValueError):
        dec.decode_OpenCL_min_sum(bad)
    # one Eb/N0 point of the BER driver: the same errors as the reference decoding the same channel stream
    B, nb = 64, 2
    cfg = BERConfig(EbN0_dB_start=1.0, EbN0_dB_max_value=1.0, min_errors=10 ** 9, msg_at_time=B, max_blocks=nb * B,
                    seed=5, llr_dtype=torch.float32)
    r = run_ber(dec, cfg)
    assert r.blocks == [nb * B]
    q = AWGN_Channel_Quantizer(10 ** (-1.0 / 10) / (2 * dec.R_c), cfg.AD_max_abs, cfg.cardinality_T_channel,
                               cfg.cardinality_Y_channel, seed=5)
    q.init_OpenCL_quanti(N, B, return_buffer_only=True)
    want = 0
    for g in range(nb):
        q.offset = g * philox_blocks(N, B)
        ch = q.quantize_direct_OpenCL_LLR(N, B, dtype=torch.float32).cpu().numpy()
        want += int((layered_decode(H, layers, ch, 8, 0.75, 0.0)[0][:dec.data_len] < 0).sum())
    print("BER point: errors", r.errors[0], "reference", want)
    assert want > 0 and r.errors[0] == float(want)


# ---------------------------------------------------------------------------------------------------------------
# arithmetic edges: ties, zeros of either sign, the clamp and llr_max, subnormals (tests/_layered_census.py)
# ---------------------------------------------------------------------------------------------------------------
def edge_code(name):
    return mixed() if name == "mixed" else wlan(27)


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("code", ["mixed", "wlan27"])
def test_edge_families(engine, code, family):
    """quantised: integers with +-0.0 entries (m1 == m2, Q == 0, R = -0 on Q == 0; the sign-bit arithmetic and
    the running two minima), all four (alpha, beta). saturating: the clamp at +-150, +-FLT_MAX. small_llr_max:
    llr_max = 7.5 through the constructor. subnormal: LLRs below 2^-126 and across it, beta = 0 and 2^-140
    (every operation keeps subnormals, as numpy does). B = 16, 6 iterations, early stop on and off."""
    H, layers = edge_code(code)
    G = engine.Graph(H, "cuda:0")
    gen, params = FAMILIES[family]
    llr = gen(H, FAMILY_B)
    for a, b, L in params:
        dec = engine.LayeredDecoder(G, layers, FAMILY_IMAX, FAMILY_B, alpha=a, beta=b, llr_max=L)
        for early in (True, False):
            check(dec, H, layers, llr, FAMILY_IMAX, a, b, early, llr_max=L)


@pytest.mark.parametrize("code", ["mixed", "wlan27"])
def test_mixed_batch(engine, code):
    """Neighbouring columns from different families, three more than a workgroup's codewords: the waves of one
    workgroup do unlike things and stop at unlike times. The all-zero columns (+0.0, -0.0) stop after one
    iteration with an all-zero output."""
    H, layers = edge_code(code)
    G = engine.Graph(H, "cuda:0")
    col = {k: i for i, k in enumerate(MIXED_BATCH_COLUMNS)}
    for a, b in AB:
        dec = engine.LayeredDecoder(G, layers, FAMILY_IMAX, 16, alpha=a, beta=b)
        B = dec.geometry(1)[0] + 3
        assert len(MIXED_BATCH_COLUMNS) <= B <= 16 and dec.geometry(B)[1] == 2
        llr = mixed_batch_llr(H.shape[1], B, seed=31)
        for early in (True, False):
            out, it = check(dec, H, layers, llr, FAMILY_IMAX, a, b, early)
            for z in (col["zeros"], col["negative_zeros"]):
                assert it[z] == (1 if early else FAMILY_IMAX) and (out[:, z] == 0).all()
            assert not early or len(set(it.tolist())) >= 2


# ---------------------------------------------------------------------------------------------------------------
# API and layout (Z = 27, quantised input)
# ---------------------------------------------------------------------------------------------------------------
QAB = (0.8125, 0.25)


@pytest.mark.parametrize("Z,widths", [(27, (63, 64, 65, 129)), (81, (65,))])
def test_transposition_tiles(engine, Z, widths):
    """lay_transpose through full and ragged 64 x 64 tiles in both directions: N = 648 is 10 tiles and 8 rows,
    N = 1944 30 tiles and 24 rows; B one less than, equal to, one more than a tile and two tiles and one column.
    1 and 3 iterations."""
    H, layers = wlan(Z)
    G = engine.Graph(H, "cuda:0")
    a, b = QAB
    llr = quantised_llr(H.shape[1], max(widths), seed=60 + Z)
    for imax in (1, 3):
        dec = engine.LayeredDecoder(G, layers, imax, max(widths), alpha=a, beta=b)
        for early in (True, False):
            ref = layered_decode(H, layers, llr, imax, a, b, early_stop=early)   # codewords decode independently
            for B in widths:
                check(dec, H, layers, llr[:, :B], imax, a, b, early, ref=(ref[0][:, :B], ref[1][:B]))


@pytest.fixture(scope="module")
def z27(engine):
    """One decoder of max_batch 129 on Z = 27 and a quantised batch with its reference (early stop, 6 iterations)."""
    H, layers = wlan(27)
    a, b = QAB
    dec = engine.LayeredDecoder(engine.Graph(H, "cuda:0"), layers, FAMILY_IMAX, 129, alpha=a, beta=b)
    llr = quantised_llr(H.shape[1], FAMILY_B, seed=70)
    return dec, H, layers, llr, layered_decode(H, layers, llr, FAMILY_IMAX, a, b)


def test_descending_reuse(z27):
    """One decoder decodes B = 129, then 5, then 1 (unlike inputs): stale rows of the staging buffer do not leak."""
    dec, H, layers, _, _ = z27
    for B, seed in ((129, 71), (5, 72), (1, 73)):
        check(dec, H, layers, quantised_llr(H.shape[1], B, seed=seed), FAMILY_IMAX, *QAB, True)


def test_in_place_and_no_iters(z27):
    dec, H, layers, llr, ref = z27
    t = torch.from_numpy(llr).to(dec.device)
    out = dec.decode(t.clone(), iters=None)                    # no iters tensor
    assert np.array_equal(out.cpu().numpy(), ref[0])
    it = torch.full((llr.shape[1],), -1, dtype=torch.int32, device=dec.device)
    same = dec.decode(t, out=t, iters=it)                      # in place
    assert same is t
    assert np.array_equal(t.cpu().numpy(), ref[0]) and np.array_equal(it.cpu().numpy(), ref[1])


def test_side_stream(z27):
    dec, H, layers, llr, ref = z27
    t = torch.from_numpy(llr).to(dec.device)
    it = torch.full((llr.shape[1],), -1, dtype=torch.int32, device=dec.device)
    torch.cuda.synchronize(dec.device)
    side = torch.cuda.Stream(device=dec.device)
    with torch.cuda.stream(side):
        out = dec.decode(t, iters=it)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref[0]) and np.array_equal(it.cpu().numpy(), ref[1])


def test_batch_too_large(z27):
    dec, H, _, _, _ = z27
    t = torch.zeros((H.shape[1], dec.max_batch + 1), dtype=torch.float32, device=dec.device)
    with pytest.raises(_lib.IBLError) as e:
        dec.decode(t)
    assert f"rc={_lib.IBL_EINVAL}" in str(e.value)
