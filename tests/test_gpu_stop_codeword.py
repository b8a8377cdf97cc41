"""GPU: the per-codeword stop of the fused flooding decoders, float and IB (include/ibldpc.h "Per-codeword stop").

Reference of column c: the oracle decoding that column alone with early_stop=True (tests/_stop_codeword.py;
tests/test_cpu_stop_codeword.py pins that those stops spread inside the kernel's groups, that some column never
stops and that the batch rule would stop nowhere). Bars: np.array_equal on out and iters for IB (uint8 and int32 in
and out), min-sum and corrected min-sum in fp32 and fp64; fp64 BP within 1e-9 and equal iters; fp32 BP by
tests/test_gpu_codewords._float_compare against the fp64 oracle and equal iters. Independent cross-check for every
family, fp32 BP included: each column of a batch equals, bit for bit, the same handle decoding that column alone
with today's early_stop=True."""
import numpy as np
import pytest
import torch

from tests import _codewords as cw
from tests import _stop_codeword as sc
from tests.test_gpu_codewords import KINDS, PRECS, _family, _float_compare, device_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMAX = sc.IMAX
SENTINEL = -77


@pytest.fixture(scope="module")
def eng():
    from informationbottleneckdecodingldpc_amd import engine
    return engine


def _decoder(eng, kind, prec, cap, imax=IMAX, path="fused"):
    k, corr, _ = KINDS[kind]
    return eng.FloatDecoder(device_graph(eng, sc.NAME), k, imax, cap, precision=PRECS[prec][0], path=path, **corr)


def _each(dec, llr, tdt, extra=3, **kw):
    """Decode with the per-codeword stop -> (out, iters [B]); `extra` sentinel entries behind iters stay untouched."""
    B = llr.shape[1]
    it = torch.full((B + extra,), SENTINEL, dtype=torch.int32, device=DEV)
    out = dec.decode(torch.from_numpy(np.array(llr)).to(DEV).to(tdt), early_stop="codeword", iters=it, **kw)
    torch.cuda.synchronize()
    it = it.cpu().numpy()
    assert (it[B:] == SENTINEL).all(), "iters written beyond B"
    return out.cpu().numpy(), it[:B]


def _check(out, it, ref, kind, prec, what):
    r_out, r_it = ref
    print(f"{what} {kind} {prec}: iters {np.bincount(r_it).tolist()}, device equal {np.array_equal(it, r_it)}")
    assert np.array_equal(it, r_it), (what, it.tolist(), r_it.tolist())
    _float_compare(out, r_out, kind, prec, what)


@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_each_column_equals_the_oracle_alone(eng, kind, prec):
    """B = 24 and the ragged B = 23 (last group of 3 of 4, 1 of 2), decoder and channel dtype the same."""
    tdt, ndt = PRECS[prec]
    family = _family(kind, prec)
    dec = _decoder(eng, kind, prec, 24)
    for B in (24, 23):
        llr = sc.spread_input(B)[0]
        out, it = _each(dec, llr.astype(ndt), tdt)
        assert out.dtype == ndt
        _check(out, it, sc.spread_ref(family, B), kind, prec, f"B={B}")


@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_each_column_equals_the_same_handle_alone(eng, kind, prec):
    """The unchanged path as the reference: column c alone with early_stop=True on the same handle, bit for bit."""
    tdt, ndt = PRECS[prec]
    dec = _decoder(eng, kind, prec, 24)
    llr = torch.from_numpy(sc.spread_input(24)[0].astype(ndt)).to(DEV)
    out, it = _each(dec, llr.cpu().numpy(), tdt)
    one = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    for c in range(24):
        o = dec.decode(llr[:, c:c + 1].contiguous(), early_stop=True, iters=one)
        assert int(one.item()) == it[c], c
        assert np.array_equal(o.cpu().numpy()[:, 0], out[:, c]), c
    assert len(set(it.tolist())) >= 4


@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_past_the_first_group(eng, kind, prec):
    """test_float_fused_past_the_first_group's recipe, B = 2 x (codewords per group) x grid + 5: every workgroup
    takes a second group after an early exit from its first (every second tile of 64 holds early stoppers only), and
    the last group is ragged."""
    tdt, ndt = PRECS[prec]
    cwl = 4 if prec == "fp32" else 2
    cap = 16384
    dec = _decoder(eng, kind, prec, cap)
    _, grid = dec.fused_geometry(cap)
    B = 2 * cwl * grid + 5
    assert dec.fused and grid > 0 and B <= cap
    family = _family(kind, prec)
    llr = sc.spread_input(B)[0]
    ref = sc.spread_ref(family, B)
    groups = ref[1][:B // cwl * cwl].reshape(-1, cwl).max(axis=1)
    assert (groups[:grid] < IMAX - 1).any() and (groups[grid:] == IMAX - 1).any()
    out, it = _each(dec, llr.astype(ndt), tdt)
    _check(out, it, ref, kind, prec, f"B={B}")


@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_whole_batch_stops_at_once(eng, kind, prec):
    """12 dB (BP 7.3 dB): every column stops at its first possible pass (BP: within a few), so every group leaves
    early; decisions are the transmitted bits."""
    tdt, ndt = PRECS[prec]
    family = _family(kind, prec)
    B = 70
    dec = _decoder(eng, kind, prec, B)
    llr = sc.high_input(B, sc.high_db(family))
    out, it = _each(dec, llr.astype(ndt), tdt)
    _check(out, it, sc.high_ref(family, B), kind, prec, "high SNR")
    assert np.array_equal(out < 0, cw.codewords(sc.NAME, B) == 1)


@pytest.mark.parametrize("imax", [1, 2])
def test_imax_one_and_two(eng, imax):
    llr = sc.spread_input(23)[0]
    for kind, prec in (("minsum", "fp32"), ("bp", "fp64")):
        tdt, ndt = PRECS[prec]
        dec = _decoder(eng, kind, prec, 23, imax=imax)
        out, it = _each(dec, llr.astype(ndt), tdt)
        ref = sc.decode_columns(_family(kind, prec), llr, imax=imax)
        assert (ref[1] == imax - 1).all()
        _check(out, it, ref, kind, prec, f"imax={imax}")
        fixed = dec.decode(torch.from_numpy(llr.astype(ndt)).to(DEV), early_stop=False)
        assert np.array_equal(fixed.cpu().numpy(), out)


def test_dtype_mixes_no_iters_and_in_place(eng):
    """fp64 channel into the fp32 decoder with fp64 output and the reverse; iters=None; out is the input tensor."""
    B = 23
    llr = sc.spread_input(B)[0]
    for kind, prec, family in (("minsum", "fp32", "ms32"), ("corrected", "fp64", "corr64")):
        tdt, ndt = PRECS[prec]
        odt = torch.float64 if prec == "fp32" else torch.float32
        r_out, r_it = sc.spread_ref(family, B)
        dec = _decoder(eng, kind, prec, B)
        x = torch.from_numpy(np.array(llr)).to(DEV).to(odt)      # float32 values: exact in either dtype
        out = dec.decode(x, out_dtype=odt, early_stop="codeword")
        assert out.dtype == odt
        assert np.array_equal(out.cpu().numpy(), r_out.astype(out.cpu().numpy().dtype))
        y = torch.from_numpy(llr.astype(ndt)).to(DEV)
        it = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
        res = dec.decode(y, out=y, early_stop="codeword", iters=it)
        assert res.data_ptr() == y.data_ptr()
        assert np.array_equal(y.cpu().numpy(), r_out) and np.array_equal(it.cpu().numpy(), r_it)


def test_side_stream_and_batch_sizes_on_one_handle(eng):
    """A side stream; a larger batch, then a smaller one; the columns of a wider output buffer beyond B stay."""
    tdt, ndt = PRECS["fp32"]
    dec = _decoder(eng, "minsum", "fp32", 130)
    s = torch.cuda.Stream(device=DEV)
    for B in (130, 23):
        llr = sc.spread_input(B)[0]
        x = torch.from_numpy(np.array(llr)).to(DEV)
        it = torch.full((B + 2,), SENTINEL, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            out = dec.decode(x, early_stop="codeword", iters=it)
        s.synchronize()
        r_out, r_it = sc.spread_ref("ms32", B)
        assert np.array_equal(out.cpu().numpy(), r_out)
        assert np.array_equal(it.cpu().numpy()[:B], r_it) and (it.cpu().numpy()[B:] == SENTINEL).all()


def test_output_rows_end_at_the_batch(eng):
    """The [N][B] output is contiguous: with B = 23 the element after a row's last column is the next row's first.
    A sentinel-filled buffer one element longer than N x B keeps that element, and every element of the N x B is
    written (none keeps the sentinel)."""
    B = 23
    dec = _decoder(eng, "minsum", "fp32", B)
    llr = sc.spread_input(B)[0]
    n = llr.shape[0]
    buf = torch.full((n * B + 1,), float(SENTINEL), dtype=torch.float32, device=DEV)
    out = buf[:n * B].view(n, B)
    dec.decode(torch.from_numpy(np.array(llr)).to(DEV), out=out, early_stop="codeword")
    r_out, _ = sc.spread_ref("ms32", B)
    assert np.array_equal(out.cpu().numpy(), r_out)
    assert float(buf[-1].item()) == SENTINEL


def test_modes_in_turn_on_one_handle(eng):
    """early_stop=True, then "codeword", then False on one handle, each equal to its reference."""
    B = 24
    llr = sc.spread_input(B)[0]
    dec = _decoder(eng, "minsum", "fp32", B)
    x = torch.from_numpy(np.array(llr)).to(DEV)
    g = cw.code(sc.NAME)[1]
    from oracle import oracle
    one = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    for mode in (True, "codeword", False, "codeword", True):
        if mode == "codeword":
            out, it = _each(dec, llr, torch.float32)
            r_out, r_it = sc.spread_ref("ms32", B)
            assert np.array_equal(it, r_it)
        else:
            out = dec.decode(x, early_stop=mode, iters=one).cpu().numpy()
            r_out, r_it = oracle.float32_decode(g, IMAX, llr, early_stop=mode, return_iters=True)
            assert int(one.item()) == r_it == IMAX - 1
        assert np.array_equal(out, r_out), mode


def test_input_violations_are_counted(eng):
    dec = _decoder(eng, "minsum", "fp32", 23)
    llr = np.array(sc.spread_input(23)[0])
    llr[5, 7] = np.nan
    dec.input_violations(raise_on_error=False)
    dec.decode(torch.from_numpy(llr).to(DEV), early_stop="codeword")
    assert dec.input_violations(raise_on_error=False) == 1


def test_refusals(eng):
    from informationbottleneckdecodingldpc_amd import _lib
    B = 23
    llr = torch.from_numpy(np.array(sc.spread_input(B)[0])).to(DEV)
    n = llr.shape[0]
    # a handle on the per-pass path
    dec = _decoder(eng, "minsum", "fp32", B, path="passes")
    out = torch.full((n, B), float(SENTINEL), dtype=torch.float32, device=DEV)
    it = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.IBLError, match="rc=-4"):
        dec.decode(llr, out=out, early_stop="codeword", iters=it)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (it == SENTINEL).all()
    # a code that does not fit the fused kernel (the DVB-S2 test code)
    gd = device_graph(eng, "dvb")
    dvb = eng.FloatDecoder(gd, 0, IMAX, 8)
    assert not dvb.fused
    x = torch.zeros((cw.code("dvb")[1].n_v, 8), dtype=torch.float32, device=DEV)
    o = torch.full_like(x, float(SENTINEL))
    with pytest.raises(_lib.IBLError, match="rc=-4"):
        dvb.decode(x, out=o, early_stop="codeword")
    torch.cuda.synchronize()
    assert (o == SENTINEL).all()
    # a short iters
    fused = _decoder(eng, "minsum", "fp32", B)
    with pytest.raises(ValueError, match="at least B"):
        fused.decode(llr, early_stop="codeword", iters=torch.zeros(B - 1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="early_stop"):
        fused.decode(llr, early_stop="each")


@pytest.mark.parametrize("which", ["minsum", "corrected", "bp"])
def test_reference_named_classes(eng, which):
    """stop="codeword" on the two float classes: decode_OpenCL* output and last_iters equal the engine's, and
    return_errors_all_zero counts what the per-column oracle outputs hold."""
    from informationbottleneckdecodingldpc_amd import _lib
    from informationbottleneckdecodingldpc_amd.bp_decoder_irreg import BeliefPropagationDecoderClassIrregular
    from informationbottleneckdecodingldpc_amd.min_sum_decoder_irreg import Min_Sum_Decoder_class_irregular
    B = 24
    H = cw.code(sc.NAME)[0]
    llr = sc.spread_input(B)[0]
    prec = "fp64" if which == "bp" else "fp32"
    tdt, ndt = PRECS[prec]
    kw = dict(precision=tdt, stop="codeword")
    if which == "corrected":
        kw.update(alpha=cw.CORRECTED[0], beta=cw.CORRECTED[1])
    cls = BeliefPropagationDecoderClassIrregular if which == "bp" else Min_Sum_Decoder_class_irregular
    d = cls(H, IMAX, cw.T_CH, B, **kw)
    d.init_OpenCL_decoding(B, torch.device(DEV))
    run = d.decode_OpenCL_belief_propagation if which == "bp" else d.decode_OpenCL_min_sum
    buf = run(torch.from_numpy(llr.astype(ndt)).to(DEV), buffer_in=True, return_buffer=True)
    e_out, e_it = _each(_decoder(eng, which, prec, B), llr.astype(ndt), tdt)
    assert d.last_iters.dtype == torch.int32 and d.last_iters.numel() == B
    assert np.array_equal(d.last_iters.cpu().numpy(), e_it) and np.array_equal(buf.cpu().numpy(), e_out)
    host = run(llr.astype(ndt))
    assert isinstance(host, np.ndarray) and np.array_equal(host, e_out)
    r_out, r_it = sc.spread_ref(_family(which, prec), B)
    assert np.array_equal(e_it, r_it)
    assert d.return_errors_all_zero(buf) == float((r_out[:d.data_len] < 0).sum())
    # decode_on_host is unchanged: fixed iterations, and it leaves last_iters alone
    before = d.last_iters
    fixed = d.decode_on_host(llr[:, 1])
    ref = sc.decode_columns(_family(which, prec), llr[:, 1:2], early=False)[0][:, 0]
    _float_compare(fixed.astype(ndt), ref, which, prec, "decode_on_host")
    assert d.last_iters is before
    # a code that does not run fused is refused when the decoder is made
    dv = Min_Sum_Decoder_class_irregular(cw.code("dvb")[0], IMAX, cw.T_CH, 8, stop="codeword")
    with pytest.raises(_lib.IBLError, match="fused"):
        dv.init_OpenCL_decoding(8, torch.device(DEV))


# ---------------------------------------------------------------------------------------------------------------
# information-bottleneck decoder
# ---------------------------------------------------------------------------------------------------------------
_ib_graphs = {}


def _ib_decoder(eng, name, cap, imax=IMAX, **kw):
    _, g, match = sc.ib_code(name)
    if name not in _ib_graphs:
        _ib_graphs[name] = eng.Graph(g, DEV)
    tb = sc.ib_input(name, 24 if name == "wlan" else None, imax)[0]
    return eng.IBDecoder(_ib_graphs[name], tb, match, cap, **kw)


def _ib_each(dec, ch, dt, extra=3, **kw):
    B = ch.shape[1]
    it = torch.full((B + extra,), SENTINEL, dtype=torch.int32, device=DEV)
    out = dec.decode(torch.from_numpy(np.array(ch)).to(DEV).to(dt).contiguous(), out_dtype=dt, early_stop="codeword",
                     iters=it, **kw)
    torch.cuda.synchronize()
    it = it.cpu().numpy()
    assert out.dtype == dt and (it[B:] == SENTINEL).all()
    return out.cpu().numpy().astype(np.int32), it[:B]


@pytest.mark.parametrize("dbuf", ["1", "0"])
@pytest.mark.parametrize("ncw", ["8", "4"])
@pytest.mark.parametrize("name", list(sc.IB_CODES))
def test_ib_each_column_equals_the_oracle_alone(eng, name, ncw, dbuf, monkeypatch):
    """WLAN at B = 130 (ragged last group) and the two-quad (3, 9) code at B = 4100 (workgroups run several groups:
    the set parity crosses early group exits), with 8 and 4 codewords a workgroup and with two table sets and one."""
    monkeypatch.setenv("IBL_FUSED_NCW", ncw)
    monkeypatch.setenv("IBL_FUSED_DBUF", dbuf)
    _, ch, _ = sc.ib_input(name)
    B = ch.shape[1]
    dec = _ib_decoder(eng, name, B, path="fused")
    assert dec.fused and dec.fused_ncw(B) == int(ncw)
    r_out, r_it = sc.ib_ref(name)
    for dt in (torch.uint8, torch.int32):
        out, it = _ib_each(dec, ch, dt)
        print(f"{name} ncw={ncw} dbuf={dbuf} {dt}: iters {np.bincount(r_it).tolist()}, equal "
              f"{np.array_equal(it, r_it)}, out mismatches {int((out != r_out).sum())}")
        assert np.array_equal(it, r_it)
        assert np.array_equal(out, r_out)


@pytest.mark.parametrize("ncw", ["8", "4"])
def test_ib_each_column_equals_the_same_handle_alone(eng, ncw, monkeypatch):
    monkeypatch.setenv("IBL_FUSED_NCW", ncw)
    _, ch, _ = sc.ib_input("wlan", 24)
    dec = _ib_decoder(eng, "wlan", 24, path="fused")
    out, it = _ib_each(dec, ch, torch.int32)
    x = torch.from_numpy(np.array(ch)).to(DEV)
    one = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    for c in range(24):
        o = dec.decode(x[:, c:c + 1].contiguous(), early_stop=True, iters=one)
        assert int(one.item()) == it[c], c
        assert np.array_equal(o.cpu().numpy()[:, 0], out[:, c]), c
    assert np.array_equal(it, sc.ib_ref("wlan", 24)[1]) and len(set(it.tolist())) >= 4


@pytest.mark.parametrize("imax", [1, 2])
def test_ib_imax_one_and_two(eng, imax):
    _, ch, _ = sc.ib_input("wlan", 24, imax)
    dec = _ib_decoder(eng, "wlan", 24, imax=imax, path="fused")
    out, it = _ib_each(dec, ch, torch.uint8)
    r_out, r_it = sc.ib_ref("wlan", 24, imax)
    assert (r_it == imax - 1).all() and np.array_equal(it, r_it) and np.array_equal(out, r_out)
    fixed = dec.decode(torch.from_numpy(np.array(ch)).to(DEV), early_stop=False).cpu().numpy()
    assert np.array_equal(fixed, out)


def test_ib_edges_on_one_handle(eng):
    """iters=None; a side stream; a larger batch, then a smaller one; early_stop=True, "codeword", False in turn;
    nothing behind the N x B outputs is written."""
    from oracle import oracle
    _, g, match = sc.ib_code("wlan")
    dec = _ib_decoder(eng, "wlan", 130, path="fused")
    s = torch.cuda.Stream(device=DEV)
    for B in (130, 23):
        tb, ch, _ = sc.ib_input("wlan", B)
        r_out, r_it = sc.ib_ref("wlan", B)
        x = torch.from_numpy(np.array(ch)).to(DEV)
        n = x.shape[0]
        buf = torch.full((n * B + 1,), 99, dtype=torch.int32, device=DEV)
        out = buf[:n * B].view(n, B)
        it = torch.full((B + 2,), SENTINEL, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            dec.decode(x, out=out, early_stop="codeword", iters=it)
        s.synchronize()
        assert np.array_equal(out.cpu().numpy(), r_out) and int(buf[-1].item()) == 99
        assert np.array_equal(it.cpu().numpy()[:B], r_it) and (it.cpu().numpy()[B:] == SENTINEL).all()
        assert np.array_equal(dec.decode(x, early_stop="codeword").cpu().numpy(), r_out)
        one = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        for mode in (True, "codeword", False):
            if mode == "codeword":
                o, i = _ib_each(dec, ch, torch.int32)
                assert np.array_equal(i, r_it) and np.array_equal(o, r_out)
            else:
                o = dec.decode(x, early_stop=mode, iters=one).cpu().numpy()
                ro, ri = oracle.ib_decode(g, tb, ch, match=match, early_stop=mode, return_iters=True)
                assert int(one.item()) == ri and np.array_equal(o, ro)


def test_ib_refusals(eng):
    from informationbottleneckdecodingldpc_amd import _lib
    _, ch, _ = sc.ib_input("wlan", 24)
    x = torch.from_numpy(np.array(ch)).to(DEV)
    for kw in (dict(path="passes"), dict(force_generic=True)):
        dec = _ib_decoder(eng, "wlan", 24, **kw)
        assert not dec.fused
        out = torch.full(x.shape, 99, dtype=torch.int32, device=DEV)
        it = torch.full((24,), SENTINEL, dtype=torch.int32, device=DEV)
        with pytest.raises(_lib.IBLError, match="rc=-4"):
            dec.decode(x, out=out, early_stop="codeword", iters=it)
        torch.cuda.synchronize()
        assert (out == 99).all() and (it == SENTINEL).all()
    # the DVB-S2 test code: refused unless this device's LDS holds it on the fused kernel
    tb, ch_d, _, _ = cw.flood_input("dvb", 300, 6.0)
    dvb = eng.IBDecoder(device_graph(eng, "dvb"), tb, cw.ib_match("dvb"), 8)
    if not dvb.fused:
        xd = torch.from_numpy(np.array(ch_d[:, :8])).to(DEV).contiguous()
        od = torch.full(xd.shape, 99, dtype=torch.int32, device=DEV)
        with pytest.raises(_lib.IBLError, match="rc=-4"):
            dvb.decode(xd, out=od, early_stop="codeword")
        torch.cuda.synchronize()
        assert (od == 99).all()
    fused = _ib_decoder(eng, "wlan", 24, path="fused")
    with pytest.raises(ValueError, match="at least B"):
        fused.decode(x, early_stop="codeword", iters=torch.zeros(23, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="early_stop"):
        fused.decode(x, early_stop="each")


@pytest.mark.parametrize("which", ["irregular", "regular"])
def test_ib_reference_named_classes(eng, which):
    """stop="codeword" on the two IB classes: decode_OpenCL output and last_iters equal the engine's and the
    per-column oracle's, return_errors_all_zero counts the oracle outputs' decided ones."""
    from informationbottleneckdecodingldpc_amd.discrete_LDPC_decoder import Discrete_LDPC_Decoder_class
    from informationbottleneckdecodingldpc_amd.discrete_LDPC_decoder_irreg import Discrete_LDPC_Decoder_class_irregular
    name = "wlan" if which == "irregular" else "reg39"
    B = 24
    H, g, match = sc.ib_code(name)
    tb, ch, _ = sc.ib_input(name, B)
    if which == "irregular":
        d = Discrete_LDPC_Decoder_class_irregular(H, IMAX, 16, 16, tb.cn, tb.vn, tb.match_cn, tb.match_vn, B,
                                                  match="true" if match else "false", stop="codeword")
        r_out, r_it = sc.ib_ref(name, B)
        rows = d.data_len
    else:     # the regular class never matches
        d = Discrete_LDPC_Decoder_class(H, IMAX, 16, 16, tb.cn, tb.vn, B, stop="codeword")
        from oracle import oracle
        cols = [oracle.ib_decode(g, tb, np.ascontiguousarray(ch[:, c:c + 1]), match=False, early_stop=True,
                                 return_iters=True) for c in range(B)]
        r_out = np.concatenate([np.asarray(o).astype(np.int32) for o, _ in cols], axis=1)
        r_it = np.array([i for _, i in cols], dtype=np.int32)
        rows = g.n_v
    d.init_OpenCL_decoding(B, torch.device(DEV))
    buf = d.decode_OpenCL(torch.from_numpy(np.array(ch)).to(DEV), buffer_in=True, return_buffer=True)
    assert d.last_iters.dtype == torch.int32 and d.last_iters.numel() == B
    assert np.array_equal(d.last_iters.cpu().numpy(), r_it) and np.array_equal(buf.cpu().numpy(), r_out)
    assert len(set(r_it.tolist())) >= 3
    host = d.decode_OpenCL(np.array(ch))
    assert isinstance(host, np.ndarray) and np.array_equal(host, r_out)
    assert d.return_errors_all_zero(buf) == int((r_out[:rows] < 8).sum())
    before = d.last_iters
    d.decode_on_host(np.array(ch[:, 1]))
    assert d.last_iters is before


@pytest.mark.parametrize("kind", ["ib", "minsum"])
def test_run_ber_counts_the_per_column_oracle(kind):
    """One run_ber point (WLAN Z = 27, 256 frames in batches of 128) through a stop="codeword" class counts exactly
    the bit errors of a per-column oracle replay of the same Philox stream (tests/test_gpu_ber_parity.py replays the
    batch stop the same way); run_ber itself is unchanged and only calls the class methods."""
    from informationbottleneckdecodingldpc_amd import tables
    from informationbottleneckdecodingldpc_amd.ber import BERConfig, run_ber
    from informationbottleneckdecodingldpc_amd.discrete_LDPC_decoder_irreg import Discrete_LDPC_Decoder_class_irregular
    from informationbottleneckdecodingldpc_amd.min_sum_decoder_irreg import Min_Sum_Decoder_class_irregular
    from tests.test_gpu_ber_parity import _quanti, _replay
    H, g, _, _ = cw.code(sc.NAME)
    B = 128
    cfg = BERConfig(EbN0_dB_start=2.5, EbN0_dB_max_value=2.5, EbN0_dB_normal_stepwidth=1.0,
                    EbN0_dB_small_stepwidth=0.5, target_error_rate=1e-9, min_errors=10 ** 9, msg_at_time=B,
                    max_blocks=256, seed=13, llr_dtype=torch.float32)
    if kind == "ib":
        design = _quanti(cfg, 10 ** (-2.5 / 10) / (2 * g.R_c))
        tb = tables.llr_tables(design.output_LLRs, g.d_c_max, g.d_v_max, IMAX)
        dec = Discrete_LDPC_Decoder_class_irregular(H, IMAX, 16, 16, tb.cn, tb.vn, tb.match_cn, tb.match_vn, B,
                                                    match="true", stop="codeword")
        its = []

        def decode(cl, q):
            out, it = sc.ib_decode_columns("wlan", tb, np.ascontiguousarray(cl, dtype=np.int32))
            its.append(it)
            return out
        ones = lambda out, dl: float((out[:dl] < 8).sum())
    else:
        dec = Min_Sum_Decoder_class_irregular(H, IMAX, 16, B, stop="codeword")
        its = []

        def decode(cl, q):
            out, it = sc.decode_columns("ms32", q.output_LLRs.astype(np.float32)[cl])
            its.append(it)
            return out
        ones = lambda out, dl: float((out[:dl] < 0).sum())
    r = run_ber(dec, cfg)
    ebn0, ber, errs, blks = _replay(cfg, g.n_v, dec.data_len, float(dec.R_c), decode, ones)
    print(f"{kind}: errors gpu {[int(e) for e in r.errors]} oracle {[int(e) for e in errs]}, last batch's stops "
          f"{np.bincount(its[-1]).tolist()}")
    assert [int(e) for e in r.errors] == [int(e) for e in errs] and r.blocks == blks
    np.testing.assert_array_equal(r.BER_vector, ber)
    assert errs[0] > 0 and len(set(its[-1].tolist())) >= 3       # a spread of stops, and errors to count
    assert np.array_equal(dec.last_iters.cpu().numpy(), its[-1])
