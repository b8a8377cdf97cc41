"""GPU: the corrected (normalised / offset) flooding min-sum decoder against its numpy reference
(tests/_minsum_corrected_ref.py, pinned to the oracle by tests/test_cpu_minsum_corrected.py) on the per-pass, the
small-batch and the fused kernels, fp32 and fp64. Bars: APP LLRs equal by value (np.array_equal; the sign of a zero
is not specified, include/ibldpc.h "Corrected min-sum") and an equal stop iteration. The inputs' zeroing and tie
shares are asserted on the CPU side (test_gpu_inputs_reach_the_zeroing_and_the_ties)."""
import functools

import numpy as np
import pytest
import torch

from informationbottleneckdecodingldpc_amd import graph
from oracle import oracle
from tests import _minsum_corrected_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMAX = 6
PREC = {np.float32: torch.float32, np.float64: torch.float64}
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def eng():
    from informationbottleneckdecodingldpc_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _graph(name):
    return graph.build_graph({"mixed": R.mixed_H, "wlan": R.wlan_H, "dvb": R.dvb_H}[name]())


@functools.lru_cache(maxsize=None)
def _device_graph(name):
    from informationbottleneckdecodingldpc_amd import engine
    return engine.Graph(_graph(name), DEV)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _llr(name, B, ebn0=2.0):
    """The shared channel values of a code (read-only): halves on the mixed code, 16-level quantised LLRs elsewhere;
    above 2 dB (the early-stop cases) the degree-1 variables get the most reliable level, since a wrong one keeps
    its check unsatisfied for ever."""
    g = _graph(name)
    if name == "mixed":
        return _frozen(R.halves_llrs(g, B, 15))
    llr = R.quantised_llrs(g, B, ebn0, 3)
    if ebn0 > 2.0:
        llr[np.asarray(g.vn_deg) == 1] = np.abs(llr).max()
    return _frozen(llr)


@functools.lru_cache(maxsize=None)
def _ref(name, B, pair, dtype, early, ebn0=2.0, cols=None):
    """Reference decode (computed once, read-only) of _llr(name, B, ebn0), or of its columns `cols` (a tuple)."""
    llr = _llr(name, B, ebn0)
    if cols is not None:
        llr = llr[:, list(cols)]
    out, it = R.decode(_graph(name), pair[0], pair[1], IMAX, llr.astype(dtype), dtype, early_stop=early)
    return _frozen(out), it


def _decode(dec, llr, early, out_dtype=None):
    it = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    out = dec.decode(torch.from_numpy(np.ascontiguousarray(llr)).to(DEV), early_stop=early, iters=it,
                     out_dtype=out_dtype)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(it.item())


def _make(eng, name, pair, dtype, max_batch, path="auto"):
    return eng.FloatDecoder(_device_graph(name), 0, IMAX, max_batch, precision=PREC[dtype], path=path,
                            alpha=pair[0], beta=pair[1])


# ------------------------------------------------------------------ 1. every check body
@pytest.mark.parametrize("early", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pair", R.MIXED_PAIRS)
def test_every_check_body(eng, pair, dtype, early):
    """Check degrees 2..16 (MAXD = 16 kernels) on all three families: B = 260 per-pass (fp32: one 256-wide item and a
    ragged one; fp64: two 128-wide and a tail), B = 24 small-batch, B = 260 fused (the code fits in LDS)."""
    g = _graph("mixed")
    assert set(np.unique(g.cn_deg)) == set(range(2, 17))
    for path, B in (("passes", 260), ("passes", 24), ("fused", 260)):
        dec = _make(eng, "mixed", pair, dtype, B, path=path)
        assert dec.fused == (path == "fused")
        if path == "passes":
            assert (B <= dec.small_batch) == (B == 24)
        ref, ref_it = _ref("mixed", 260, pair, dtype, early, cols=None if B == 260 else tuple(range(24)))
        out, it = _decode(dec, _llr("mixed", 260)[:, :B].astype(dtype), early)
        assert it == ref_it, (path, B)
        assert out.dtype == dtype and np.array_equal(out, ref), (path, B)


# ------------------------------------------------------------------ 2. fused, past the first group
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pair", R.PAIRS)
def test_fused_past_the_first_group(eng, pair, dtype):
    """WLAN Z = 27 on the fused kernel with B = 2 x (codewords per group) x grid + 5: every workgroup runs a second
    group and the last group is ragged. Fixed iterations at 2 dB, every column compared: this run pins the arithmetic
    past the first group (its inputs are the censused ones of tests/test_cpu_minsum_corrected.py). Early stop at 12 dB,
    where the reference stops before imax - 1: nearly every LLR is the top level there, so that run pins the stop
    iteration and the second pass to it, not the zeroing or the rounding."""
    cwl = 4 if dtype is np.float32 else 2
    cap = 16384
    dec = _make(eng, "wlan", pair, dtype, cap, path="fused")
    assert dec.fused and dec.correction == pair
    _, grid = dec.fused_geometry(cap)
    B = 2 * cwl * grid + 5
    assert grid > 0 and B <= cap, (grid, B)
    ngroups, grid_b = dec.fused_geometry(B)
    assert grid_b == grid and ngroups == 2 * grid + -(-5 // cwl)
    ref, ref_it = _ref("wlan", B, pair, dtype, True, ebn0=12.0)
    assert 0 < ref_it < IMAX - 1
    out, it = _decode(dec, _llr("wlan", B, 12.0).astype(dtype), True)
    assert it == ref_it
    assert np.array_equal(out, ref)
    ref, ref_it = _ref("wlan", B, pair, dtype, False)
    out, it = _decode(dec, _llr("wlan", B).astype(dtype), False)
    assert it == ref_it == IMAX - 1
    assert out.shape == ref.shape == (_graph("wlan").n_v, B) and np.array_equal(out, ref)


# ------------------------------------------------------------------ 3. per-pass with the fold
@pytest.mark.parametrize("early", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pair", R.PAIRS)
def test_per_pass_with_the_fold(eng, pair, dtype, early):
    """The n = 7200 DVB-S2-structured code: B = 300 on the per-pass kernels with the degree-2 fold (fold_put receives
    the corrected output), then B = 5 on the small-batch kernels. Early stop at 10 dB (degree-1 variables at the top
    level), where the reference converges before imax - 1: those runs pin the stop iteration; the 2 dB runs, on the
    censused inputs, pin the arithmetic."""
    ebn0 = 10.0 if early else 2.0
    dec = _make(eng, "dvb", pair, dtype, 300)
    assert not dec.fused and dec.folded > 0 and 5 <= dec.small_batch < 300
    for B in (300, 5):
        ref, ref_it = _ref("dvb", 300, pair, dtype, early, ebn0=ebn0, cols=None if B == 300 else tuple(range(5)))
        if early:
            assert 0 < ref_it < IMAX - 1
        out, it = _decode(dec, _llr("dvb", 300, ebn0)[:, :B].astype(dtype), early)
        assert it == ref_it, B
        assert np.array_equal(out, ref), B


# ------------------------------------------------------------------ 4. reuse and coexistence
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pair", R.PAIRS)
def test_one_decoder_across_batch_sizes(eng, pair, dtype):
    """One corrected decoder decodes B = 300, 64 and 1, the smaller ones taken from the far end of the batch: from the
    per-pass kernels to the captured small-batch chains and back to a batch of one."""
    dec = _make(eng, "dvb", pair, dtype, 300)
    assert not dec.fused and 64 <= dec.small_batch < 300
    llr = _llr("dvb", 300).astype(dtype)
    ref, _ = _ref("dvb", 300, pair, dtype, False)
    for B in (300, 64, 1, 64, 300):
        out, it = _decode(dec, llr[:, 300 - B:], False)
        assert it == IMAX - 1
        assert np.array_equal(out, ref[:, 300 - B:]), B


def test_plain_and_corrected_decoders_coexist(eng):
    """A plain and a corrected decoder on one Graph, decoded alternately: the correction travels in each launch's
    arguments, so neither disturbs the other."""
    pair = R.PAIRS[0]
    g = _graph("dvb")
    llr = _llr("dvb", 300).astype(np.float32)
    plain = eng.FloatDecoder(_device_graph("dvb"), 0, IMAX, 300)
    other = _make(eng, "dvb", (0.75, 0.5), np.float32, 300)
    corr = _make(eng, "dvb", pair, np.float32, 300)
    want_plain = oracle.float32_decode(g, IMAX, llr, early_stop=False)
    want_corr, _ = _ref("dvb", 300, pair, np.float32, False)
    want_other, _ = _ref("dvb", 300, (0.75, 0.5), np.float32, False)
    assert plain.correction == (1.0, 0.0)
    for _ in range(2):
        for B in (300, 5):
            assert np.array_equal(_decode(plain, llr[:, :B], False)[0], want_plain[:, :B])
            assert np.array_equal(_decode(corr, llr[:, :B], False)[0], want_corr[:, :B])
            assert np.array_equal(_decode(other, llr[:, :B], False)[0], want_other[:, :B])


# ------------------------------------------------------------------ 5. dtype mix and special values
@pytest.mark.parametrize("path", ["fused", "passes"])
@pytest.mark.parametrize("pair", R.PAIRS)
def test_dtype_mix_and_infinite_channel_values(eng, pair, path):
    """An fp32 decoder fed float64 LLRs and asked for float64 outputs (staged by round-to-nearest-even, outputs
    widened exactly), on a batch with +-inf channel values on variables that share no check (a check with two
    infinite inputs would send an infinite message against an infinite channel value of the other sign)."""
    g = _graph("wlan")
    B = 70
    llr = np.array(_llr("wlan", B)) * (1.0 + 2.0 ** -30)      # not representable in fp32
    rows, used = [], set()
    for v in np.random.default_rng(2).permutation(g.n_v):
        checks = set(np.asarray(g.csc_rows)[g.csc_indptr[v]:g.csc_indptr[v + 1]].tolist())
        if not (checks & used):
            rows.append(int(v))
            used |= checks
        if len(rows) == 6:
            break
    assert len(rows) == 6
    for k, v in enumerate(rows):
        llr[v, (11 * k) % B] = np.inf if k % 2 == 0 else -np.inf
    assert (llr.astype(np.float32).astype(np.float64) != llr).any()
    dec = _make(eng, "wlan", pair, np.float32, B, path=path)
    dec.input_violations(raise_on_error=False)
    ref, ref_it = R.decode(g, pair[0], pair[1], IMAX, llr.astype(np.float32), np.float32)
    assert not np.isnan(ref).any() and np.isinf(ref).sum() == 6
    out, it = _decode(dec, llr, False, out_dtype=torch.float64)
    assert dec.input_violations() == 0
    assert out.dtype == np.float64 and it == ref_it
    assert np.array_equal(out, ref.astype(np.float64))


# ------------------------------------------------------------------ 6. API on the device
def test_engine_api(eng):
    G = _device_graph("wlan")
    llr = _llr("wlan", 70).astype(np.float32)
    assert eng.FloatDecoder(G, 0, IMAX, 70, alpha=0.8125, beta=0.15).correction == (0.8125, 0.15)
    assert eng.FloatDecoder(G, 0, IMAX, 70, beta=0.25).correction == (1.0, 0.25)
    a, b = eng.FloatDecoder(G, 0, IMAX, 70, alpha=0.5, beta=-0.0).correction
    assert (a, b) == (0.5, 0.0) and np.copysign(1.0, b) == 1.0      # -0.0 is taken and reported as +0
    with pytest.raises(ValueError):
        eng.FloatDecoder(G, 1, IMAX, 70, alpha=0.8)
    with pytest.raises(ValueError):
        eng.FloatDecoder(G, 1, IMAX, 70, beta=0.25)
    from informationbottleneckdecodingldpc_amd import _lib
    for kw in (dict(alpha=0.0), dict(alpha=1.0625), dict(beta=-0.25), dict(alpha=float("nan"))):
        with pytest.raises(_lib.IBLError):
            eng.FloatDecoder(G, 0, IMAX, 70, **kw)
    bp = eng.FloatDecoder(G, 1, IMAX, 70)
    with pytest.raises(_lib.IBLError):
        bp.correction
    for path in ("fused", "passes"):
        a = eng.FloatDecoder(G, 0, IMAX, 70, path=path)
        b = eng.FloatDecoder(G, 0, IMAX, 70, path=path, alpha=1.0, beta=0.0)
        assert b.correction == (1.0, 0.0)
        oa, ia = _decode(a, llr, True)
        ob, ib = _decode(b, llr, True)
        assert ia == ib and np.array_equal(oa.view(np.uint32), ob.view(np.uint32))
        assert np.array_equal(oa, oracle.float32_decode(_graph("wlan"), IMAX, llr, early_stop=True))


# ------------------------------------------------------------------ 7. drop-in class and BER driver
def test_drop_in_class_and_ber_driver():
    """Min_Sum_Decoder_class_irregular(alpha=, beta=) through ber.run_ber: the errors of the reference decoding the
    same Philox channel stream (early stop on, as the class decodes)."""
    from informationbottleneckdecodingldpc_amd.awgn_quantizer import AWGN_Channel_Quantizer
    from informationbottleneckdecodingldpc_amd.min_sum_decoder_irreg import Min_Sum_Decoder_class_irregular
    from informationbottleneckdecodingldpc_amd.ber import BERConfig, decoder_kind, run_ber
    from informationbottleneckdecodingldpc_amd.engine import philox_blocks
    H = R.wlan_H()
    g = _graph("wlan")
    N = H.shape[1]
    dec = Min_Sum_Decoder_class_irregular(H, IMAX, 16, 64, alpha=0.8125, beta=0.15)
    assert decoder_kind(dec) == "minsum" and dec.correction == (0.8125, 0.15)
    B, nb, ebn0 = 64, 2, 1.5
    cfg = BERConfig(EbN0_dB_start=ebn0, EbN0_dB_max_value=ebn0, min_errors=10 ** 9, msg_at_time=B, max_blocks=nb * B,
                    seed=5, llr_dtype=torch.float32)
    r = run_ber(dec, cfg)
    assert r.blocks == [nb * B] and dec._dec.correction == (0.8125, 0.15)
    q = AWGN_Channel_Quantizer(10 ** (-ebn0 / 10) / (2 * dec.R_c), cfg.AD_max_abs, cfg.cardinality_T_channel,
                               cfg.cardinality_Y_channel, seed=5)
    q.init_OpenCL_quanti(N, B, return_buffer_only=True)
    want = 0
    for k in range(nb):
        q.offset = k * philox_blocks(N, B)
        ch = q.quantize_direct_OpenCL_LLR(N, B, dtype=torch.float32).cpu().numpy()
        out, _ = R.decode(g, 0.8125, 0.15, IMAX, ch, np.float32, early_stop=True)
        want += int((out[:dec.data_len] < 0).sum())
    print("BER point: errors", r.errors[0], "reference", want)
    assert want > 0 and r.errors[0] == float(want)
