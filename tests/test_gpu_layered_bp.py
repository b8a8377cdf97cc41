"""GPU: the layered BP decoder (ibl_layered_create_bp, csrc/layered_bp_kernels.hip) against the float64 restatement
of its specification (tests/_layered_bp_ref.py). Every comparison with the reference asks that `out` is within
SURVEY H5, that no hard decision differs outside H5's band around zero, and that `iters` is equal except on
excusable codewords (tests/_layered_bp_ref.py reference_with_excusable), of which at most 2 % of a batch, rounded up,
may be excused; where the reference recorded its values after every iteration, an excused codeword that stopped at
another iteration is compared with the reference's values at that iteration. The fused kernel and the per-layer kernels are held to IDENTICAL bits of each other."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from informationbottleneckdecodingldpc_amd import _lib, codes
from tests import _layered_bp_ref as br
from tests._layered_census import awgn_llr, mixed, wlan
from tests.test_gpu_float import _hard_flips

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from informationbottleneckdecodingldpc_amd import engine as e
    return e


def gpu_decode(dec, llr, early=True):
    it = torch.full((llr.shape[1],), -1, dtype=torch.int32, device=dec.device)
    out = dec.decode(torch.from_numpy(np.ascontiguousarray(llr)).to(dec.device), early_stop=early, iters=it)
    return out.cpu().numpy(), it.cpu().numpy()


def compare(got, ref, label):
    """got = (out, iters) of a decoder, ref = (out, iters, excusable[, P_at, ...]) of the reference for the same
    columns. With P_at (reference_with_excusable(record=True)) an excusable column whose iters differ is compared
    with the reference's values at the decoder's own stop iteration (br.reference_for_columns); every other column,
    and every column without P_at, with the reference's `out`. -> br.compare_columns' findings."""
    out, it = got
    r_it, exc = ref[1], ref[2]
    B = out.shape[1]
    res = br.compare_columns(out, it, ref)
    bad, flips, differ, want = res["bad"], res["flips"], res["differ"], res["want"]
    assert flips == _hard_flips(out.astype(np.float64), want)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(out - want) / np.maximum(np.abs(out), np.abs(want))
    print(f"{label}: B={B} H5 violations {int(bad.sum())} in columns {np.nonzero(bad.any(axis=0))[0].tolist()}, "
          f"max |diff| {float(np.abs(out - want).max()):.3g}, max rel {float(np.nanmax(rel)):.3g}, hard flips {flips}, "
          f"iters differ at {np.nonzero(differ)[0].tolist()} (excusable {np.nonzero(exc)[0].tolist()}), "
          f"reference iters {np.bincount(r_it).tolist()}")
    assert not bad.any()
    assert flips == 0
    assert not (differ & ~exc).any()
    assert int((differ & exc).sum()) <= br.excuse_cap(B)
    return res


def cut(ref, B=None, cols=None):
    """The reference of the first B columns, or of the columns `cols` (out, iters, excusable and, if there, P_at)."""
    sel = slice(0, B) if cols is None else cols
    out, it, exc = ref[:3]
    head = (out[:, sel], it[sel], exc[sel])
    return head + (ref[3][:, :, sel],) if len(ref) > 3 and ref[3] is not None else head


# ---------------------------------------------------------------------------------------------------------------
# the named input: small DVB-S2-structured code, 130 codewords at 1.0 dB
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("imax", [1, 2, 10])
def test_named_input_both_paths(engine, imax):
    """Stop on and off, B = 1, 63, 64, 65 and 130 (one tile, a tile boundary, two tiles, ragged groups), both paths
    against the reference and bit for bit against each other."""
    H, layers, llr = br.dvb_input()
    G = engine.Graph(H, "cuda:0")
    passes = engine.LayeredBPDecoder(G, layers, imax, 130, path="passes")
    fused = engine.LayeredBPDecoder(G, layers, imax, 130, path="fused")
    assert passes.path_in_use == "passes" and fused.path_in_use == "fused"
    assert passes.geometry(130) == (0, 0, 0)
    cw = fused.geometry(130)[0]
    assert cw == min(8, (160 * 1024) // (4 * 5400 + 4 * H.nnz)) and fused.geometry(130)[1] == -(-130 // cw)
    for early in (True, False):
        ref = br.dvb_reference(imax, early)
        for B in (1, 63, 64, 65, 130):
            p = gpu_decode(passes, llr[:, :B], early)
            f = gpu_decode(fused, llr[:, :B], early)
            compare(p, cut(ref, B), f"passes imax={imax} early={early}")
            compare(f, cut(ref, B), f"fused imax={imax} early={early}")
            assert np.array_equal(p[1], f[1])
            assert np.array_equal(p[0].view(np.uint32), f[0].view(np.uint32))


def test_freezing_and_independence(engine):
    """Eight columns of the 130-codeword batch — both tiles, the earliest and the latest stoppers, one codeword that
    never converges — decoded alone give the bits they have in the batch, on both paths."""
    H, layers, llr = br.dvb_input()
    r_out, r_it, _ = br.dvb_reference(10, True)
    clean = br.syndrome_clean(H, r_out)
    never = np.nonzero(~clean)[0]
    stopped = np.nonzero(clean)[0]
    earliest = stopped[np.argmin(r_it[stopped])]
    latest = stopped[np.argmax(r_it[stopped])]
    cols = [int(earliest), int(latest), int(never[0]), 0, 63, 64, 129]
    cols += [c for c in (31, 97, 100, 17) if c not in cols][:8 - len(set(cols))]
    cols = sorted(set(cols))
    assert len(cols) == 8 and min(cols) < 64 <= max(cols) and never.size >= 1
    G = engine.Graph(H, "cuda:0")
    for path in ("passes", "fused"):
        dec = engine.LayeredBPDecoder(G, layers, 10, 130, path=path)
        out, it = gpu_decode(dec, llr)
        assert it[int(never[0])] == 10 and len(set(it[cols].tolist())) >= 3
        for c in cols:
            o1, i1 = gpu_decode(dec, llr[:, c:c + 1])
            assert i1[0] == it[c], (path, c)
            assert np.array_equal(o1[:, 0].view(np.uint32), out[:, c].view(np.uint32)), (path, c)


# ---------------------------------------------------------------------------------------------------------------
# the fused kernel on WLAN codes: a layer narrower than a wave (Z = 27) and one spanning two (Z = 81)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", ["1", "5", "cw+1"])
@pytest.mark.parametrize("imax", [1, 2, 20])
@pytest.mark.parametrize("Z", [27, 81])
def test_wlan_fused(engine, Z, imax, batch):
    """The first B = 1, 5 and cw_per_group + 1 (a ragged last group) columns of awgn_llr(N, 32, 1.5, seed=7).
    Column 5 of the Z = 27 input does not converge in 20 iterations; such a codeword amplifies rounding differences
    (tests/test_cpu_layered_bp.py: the numpy float32 form leaves H5 on it from iteration 13 on). Measured on an
    MI355X, Z = 27, i_max 20, B = 9: no value outside H5, largest |difference| 3.3e-4 (on column 5), largest relative
    difference 5.3e-5."""
    H, layers, llr = br.wlan_input(Z)
    dec = engine.LayeredBPDecoder(engine.Graph(H, "cuda:0"), layers, imax, 32)
    cw = dec.geometry(1)[0]
    assert cw == min(8, (160 * 1024) // (4 * H.shape[1] + 4 * sp.csr_matrix(H).nnz))
    assert dec.geometry(cw + 1)[1:] == (2, 2)
    B = cw + 1 if batch == "cw+1" else int(batch)
    compare(gpu_decode(dec, llr[:, :B]), cut(br.wlan_reference(Z, imax, True), B), f"Z={Z} imax={imax}")


def test_wlan_fused_small_llr_max_stays_converged(engine):
    """llr_max = 30, 50 iterations, stop off: every codeword the reference converges has a zero syndrome on the GPU
    too (with the clamp on Q instead, none has: tests/test_cpu_layered_bp.py), and on those codewords the values are
    within H5 with no hard-decision flip — the one GPU comparison at an llr_max other than 150, where R sits at its
    clamp. A codeword the reference does not converge (1 of the 32 here) may leave H5 after 50 iterations: it
    amplifies rounding differences from iteration to iteration, so it is held to nothing but iters."""
    H, layers, llr = br.wlan_input(27)
    r_out, _ = br.layered_bp_decode(H, layers, llr, 50, llr_max=30.0, early_stop=False)
    r_clean = br.syndrome_clean(H, r_out)
    dec = engine.LayeredBPDecoder(engine.Graph(H, "cuda:0"), layers, 50, 32, llr_max=30.0)
    out, it = gpu_decode(dec, llr, early=False)
    g_clean = br.syndrome_clean(H, out)
    bad = br.h5_violations(out, r_out)[:, r_clean]
    flips = _hard_flips(out[:, r_clean].astype(np.float64), r_out[:, r_clean])
    at_clamp = int((np.abs(r_out[:, r_clean]) > 30.0).sum())
    print(f"reference converges {int(r_clean.sum())} of 32, the GPU {int(g_clean.sum())}; on the reference's converged "
          f"codewords: H5 violations {int(bad.sum())}, hard flips {flips}, "
          f"max |diff| {float(np.abs(out - r_out)[:, r_clean].max()):.3g}, values beyond llr_max {at_clamp}")
    assert r_clean.sum() >= 24 and (it == 50).all()
    assert at_clamp > 0          # P past llr_max: at least one message of such a variable sits at the clamp
    assert g_clean[r_clean].all()
    assert not bad.any()
    assert flips == 0


def test_group_loop(engine):
    """Every workgroup decodes a second and a third group and the batch ends in a ragged group of one codeword:
    64 columns spread over the batch, the last cw + 1 included."""
    H, layers = wlan(27)
    G = engine.Graph(H, "cuda:0")
    cw = engine.LayeredBPDecoder(G, layers, 5, 8).geometry(1)[0]
    # the full grid (blocks per CU x CUs) is reached once the groups exceed it; a handle costs 4 N bytes a codeword
    cap = 1 << 16
    big = engine.LayeredBPDecoder(G, layers, 5, cap)
    grid = big.geometry(cap)[2]
    B = cw * (2 * grid + 1) + 1
    assert grid < -(-cap // cw) and B <= cap, f"B = {B} (cw_per_group {cw}, grid {grid}): raise cap"
    assert big.geometry(B) == (cw, 2 * grid + 2, grid)
    llr = awgn_llr(H.shape[1], B, 2.0, seed=3)
    third = 2 * cw * grid
    cols = np.unique(np.concatenate([np.linspace(0, third - 1, 64 - (B - third)).astype(np.int64),
                                     np.arange(third, B)]))
    assert cols.size == 64 and (cols >= cw * grid).sum() > 20 and (cols >= third).sum() == cw + 1
    ref = br.reference_with_excusable(H, layers, llr[:, cols], 5)
    out, it = gpu_decode(big, llr)
    compare((out[:, cols], it[cols]), ref, "group loop")


# ---------------------------------------------------------------------------------------------------------------
# every degree body, erased variables, messages at the clamp
# ---------------------------------------------------------------------------------------------------------------
def mixed_llr():
    H, _ = mixed()
    n = H.shape[1]
    x = awgn_llr(n, 9, 3.0, seed=11, R=1.0 - H.shape[0] / n)
    x[::7] = 0.0                              # erased variables: the box-plus meets 0
    x[3::11] *= np.float32(40)                # R meets its clamp
    return x


def test_every_degree_body(engine):
    """mixed(): check degrees 2..16, greedy layers of uneven size; B = 9, 6 iterations, both paths."""
    H, layers = mixed()
    assert set(np.diff(sp.csr_matrix(H).indptr).tolist()) == set(range(2, 17))
    llr = mixed_llr()
    hit = []
    br.layered_bp_decode(H, layers, llr, 2, early_stop=False, hook=lambda it, P: hit.append(float(np.abs(P).max())))
    assert hit[-1] > 150.0 and (llr[::7] == 0).all()
    G = engine.Graph(H, "cuda:0")
    for early in (True, False):
        ref = br.reference_with_excusable(H, layers, llr, 6, early_stop=early)
        got = {}
        for path in ("passes", "fused"):
            dec = engine.LayeredBPDecoder(G, layers, 6, 9, path=path)
            got[path] = gpu_decode(dec, llr, early)
            compare(got[path], ref, f"mixed {path} early={early}")
        assert np.array_equal(got["passes"][1], got["fused"][1])
        assert np.array_equal(got["passes"][0].view(np.uint32), got["fused"][0].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------
# full size
# ---------------------------------------------------------------------------------------------------------------
def test_full_size_per_layer(engine):
    """The N = 64800 rate-1/2 structured code on the per-layer path: B = 65 (two tiles, one of a single codeword),
    3 iterations, stop on, every column against the reference."""
    H = codes.dvbs2_structured(seed=3)
    layers = codes.dvbs2_layers(H)
    assert H.shape == (32400, 64800)
    llr = awgn_llr(64800, 65, 1.0, seed=13)
    G = engine.Graph(H, "cuda:0")
    with pytest.raises(_lib.IBLError) as e:
        engine.LayeredBPDecoder(G, layers, 3, 65, path="fused")
    assert f"rc={_lib.IBL_EUNSUPPORTED}" in str(e.value) and "4 N + 4 E" in str(e.value)
    dec = engine.LayeredBPDecoder(G, layers, 3, 65, path="auto")
    assert dec.path_in_use == "passes"
    ref = br.reference_with_excusable(H, layers, llr, 3)
    compare(gpu_decode(dec, llr), ref, "N=64800")


# ---------------------------------------------------------------------------------------------------------------
# reuse, graph capture, refusals, the drop-in class
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["passes", "fused"])
def test_reuse_and_graph_capture(engine, path):
    """Two decodes on one handle with different B give the bits of fresh handles (the per-layer path leaves the
    first decode's R rows behind and must not read them); a decode captured into a graph and replayed equals the
    eager one."""
    H, layers, llr = br.dvb_input()
    G = engine.Graph(H, "cuda:0")
    dec = engine.LayeredBPDecoder(G, layers, 4, 130, path=path)
    a130 = gpu_decode(dec, llr)
    a5 = gpu_decode(dec, llr[:, 60:65])
    b130 = gpu_decode(dec, llr)
    f5 = gpu_decode(engine.LayeredBPDecoder(G, layers, 4, 130, path=path), llr[:, 60:65])
    for x, y in ((a130, b130), (a5, f5)):
        assert np.array_equal(x[1], y[1]) and np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32))
    dev = dec.device
    x = torch.from_numpy(np.ascontiguousarray(llr[:, :65])).to(dev)
    out = torch.zeros((5400, 65), dtype=torch.float32, device=dev)
    it = torch.zeros(65, dtype=torch.int32, device=dev)
    eager = gpu_decode(dec, llr[:, :65])
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dec.decode(x, out=out, iters=it)
    out.zero_()
    it.zero_()
    g.replay()
    torch.cuda.synchronize(dev)
    assert np.array_equal(it.cpu().numpy(), eager[1])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), eager[0].view(np.uint32))


def test_refusals(engine):
    H, layers = mixed()
    A = sp.lil_matrix(codes.canonical_csr(H))
    c = int(np.argmax(np.diff(codes.canonical_csr(H).indptr) == 16))
    A[c, [v for v in range(A.shape[1]) if A[c, v] == 0][0]] = 1
    H17 = codes.canonical_csr(sp.csr_matrix(A))
    with pytest.raises(_lib.IBLError) as e:
        engine.LayeredBPDecoder(engine.Graph(H17, "cuda:0"), codes.greedy_layers(H17), 5, 4, path="auto")
    assert f"rc={_lib.IBL_EUNSUPPORTED}" in str(e.value) and f"check {c} has degree 17" in str(e.value)
    Hw, lw = wlan(27)
    G = engine.Graph(Hw, "cuda:0")
    with pytest.raises(_lib.IBLError) as e:
        engine.LayeredBPDecoder(G, lw, 5, 4, precision=torch.float64)
    assert f"rc={_lib.IBL_EUNSUPPORTED}" in str(e.value) and "fp64 is not built" in str(e.value)
    L = _lib.load()
    import ctypes
    for path in ("passes", "fused"):
        dec = engine.LayeredBPDecoder(G, lw, 5, 4, path=path)
        assert L.ibl_layered_set_compaction(dec._h, 2, 25) == _lib.IBL_EUNSUPPORTED
        assert L.ibl_last_error() == b"compaction is not built for the BP decoder"
        for fn, want in ((L.ibl_layered_is_bp, 1), (L.ibl_layered_is_wide, 0), (L.ibl_layered_is_fixed, 0)):
            v = ctypes.c_int32(-1)
            assert fn(dec._h, ctypes.byref(v)) == _lib.IBL_OK and v.value == want
    ms = engine.LayeredDecoder(G, lw, 5, 4)
    v = ctypes.c_int32(-1)
    assert L.ibl_layered_is_bp(ms._h, ctypes.byref(v)) == _lib.IBL_OK and v.value == 0


def test_drop_in_class_and_ber_driver(engine):
    """The drop-in class on the small DVB code: numpy and device buffers, the finite-input check, and one 2-point
    sweep of ber.run_ber whose error counts equal those of decoding the same channel stream through
    engine.LayeredBPDecoder directly."""
    import informationbottleneckdecodingldpc_amd as pkg
    from informationbottleneckdecodingldpc_amd.awgn_quantizer import AWGN_Channel_Quantizer
    from informationbottleneckdecodingldpc_amd.ber import BERConfig, decoder_kind, run_ber
    from informationbottleneckdecodingldpc_amd.engine import count_below, philox_blocks
    H, layers, llr = br.dvb_input()
    N = H.shape[1]
    dec = pkg.BeliefPropagation_Layered_Decoder_class_irregular(H, 10, 16, 64, layers=layers, path="passes")
    assert decoder_kind(dec) == "bp"
    out = dec.decode_OpenCL_belief_propagation(llr[:, :16])
    assert isinstance(out, np.ndarray)
    compare((out, dec.last_iterations.cpu().numpy()), cut(br.dvb_reference(10, True), 16), "drop-in")
    buf = dec.decode_OpenCL_belief_propagation(torch.from_numpy(llr[:, :16]).cuda(), buffer_in=True, return_buffer=True)
    assert isinstance(buf, torch.Tensor) and np.array_equal(buf.cpu().numpy().view(np.uint32), out.view(np.uint32))
    assert dec.return_errors_all_zero(buf) == float((out[:dec.data_len] < 0).sum())
    bad = llr[:, :4].copy()
    bad[3, 2] = np.inf
    with pytest.raises(ValueError, match="layered BP precondition"):
        dec.decode_OpenCL_belief_propagation(bad)
    B, nb = 64, 2
    cfg = BERConfig(EbN0_dB_start=0.5, EbN0_dB_max_value=0.6, EbN0_dB_normal_stepwidth=0.1, min_errors=10 ** 9,
                    msg_at_time=B, max_blocks=nb * B, seed=5, llr_dtype=torch.float32)
    r = run_ber(dec, cfg)
    assert r.blocks == [nb * B] * 2 and len(r.EbN0_dB_vector) == 2
    direct = engine.LayeredBPDecoder(engine.Graph(H, "cuda:0"), layers, 10, B, path="passes")
    want = []
    for k, db in enumerate(r.EbN0_dB_vector):
        q = AWGN_Channel_Quantizer(10 ** (-db / 10) / (2 * dec.R_c), cfg.AD_max_abs, cfg.cardinality_T_channel,
                                   cfg.cardinality_Y_channel, seed=5)
        q.init_OpenCL_quanti(N, B, return_buffer_only=True)
        n = 0
        for g in range(nb):
            q.offset = (k * nb + g) * philox_blocks(N, B)
            ch = q.quantize_direct_OpenCL_LLR(N, B, dtype=torch.float32)
            n += int(count_below(direct.decode(ch), dec.data_len, 0.0).item())
        want.append(float(n))
    print("BER sweep: errors", list(r.errors), "direct", want)
    assert want[0] > 0 and list(r.errors) == want
