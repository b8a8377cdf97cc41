"""GPU: the layered BP decoder with half-precision state (ibl_layered_create_bp_half, csrc/layered_half_kernels.hip)
against the numpy emulation of its specification (tests/_layered_half_ref.py): bit for bit where no box-plus is
evaluated, by value within the measured tolerance (hr.REL16, hr.ABS16; tests/test_cpu_layered_half.py) elsewhere, the
fused kernel and the per-layer kernels bit for bit against each other. Every decode's output must consist of binary16
values."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from informationbottleneckdecodingldpc_amd import _lib, codes
from tests import _layered_bp_ref as br
from tests import _layered_half_ref as hr
from tests._layered_census import awgn_llr, mixed, wlan

pytestmark = pytest.mark.gpu
F16 = torch.float16


@pytest.fixture(scope="module")
def engine():
    from informationbottleneckdecodingldpc_amd import engine as e
    return e


def gpu_decode(dec, llr, early=True):
    it = torch.full((llr.shape[1],), -1, dtype=torch.int32, device=dec.device)
    out = dec.decode(torch.from_numpy(np.ascontiguousarray(llr)).to(dec.device), early_stop=early, iters=it)
    out = out.cpu().numpy()
    assert np.isfinite(out).all()
    assert np.array_equal(out.astype(np.float16).astype(np.float32).view(np.uint32), out.view(np.uint32)), \
        "an output value is not a binary16 value"
    return out, it.cpu().numpy()


def same_bits(x, y):
    return np.array_equal(x[1], y[1]) and np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32))


def both(engine, H, layers, imax, max_batch, **kw):
    G = engine.Graph(H, "cuda:0")
    p = engine.LayeredBPDecoder(G, layers, imax, max_batch, path="passes", state_dtype=F16, **kw)
    f = engine.LayeredBPDecoder(G, layers, imax, max_batch, path="fused", state_dtype=F16, **kw)
    assert p.half and f.half and p.path_in_use == "passes" and f.path_in_use == "fused"
    return p, f


def compare(got, ref, early, label):
    """got = (out, iters) of a decoder; ref = (out, iters, P_at) of hr.layered_half_decode(record=True) for the same
    columns. Without the stop the emulation's values are P_at[-1] and iters is imax everywhere. Every entry within the
    tolerance, hard decisions equal outside the band around zero, iters equal on all but at most br.excuse_cap(B)
    columns, each of which is judged against the emulation's values at the decoder's own stop iteration."""
    out, it = got
    r_out, r_it, P_at = ref
    B = out.shape[1]
    if early:
        want = hr.want_for(it, ref)
        differ = it != r_it
    else:
        want = P_at[-1].astype(np.float64)
        differ = it != P_at.shape[0]
    bad = hr.violations(out, want)
    flips = hr.hard_flips(out, want)
    d = np.abs(out - want)
    m = np.maximum(np.abs(out), np.abs(want))
    rel = float((d[m > 1] / m[m > 1]).max()) if (m > 1).any() else 0.0
    print(f"{label}: B={B} outside the tolerance {int(bad.sum())}, max |diff| {float(d.max()):.4g} (ABS16 {hr.ABS16}), "
          f"max rel above 1 {rel:.4g} (REL16 {hr.REL16:.4g}), entries differing {int((d > 0).sum())} of {d.size}, "
          f"hard flips {flips}, iters differ at {np.flatnonzero(differ).tolist()}, "
          f"emulation iters {np.bincount(r_it).tolist()}")
    assert not bad.any()
    assert flips == 0
    assert int(differ.sum()) <= (br.excuse_cap(B) if early else 0)


def cut(ref, B):
    return ref[0][:, :B], ref[1][:B], ref[2][:, :, :B]


# ---------------------------------------------------------------------------------------------------------------
# 1. bit for bit on the code whose checks all have degree 2
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [9, 130])
def test_degree2_code_bit_for_bit(engine, B):
    """No box-plus: every operation is exact or one correctly rounded operation, so output and iters equal the
    emulation's exactly, on both paths, stop on and off. The inputs (hr.degree2_input) hold AWGN values, zeros of
    either sign, +-1e5 (the stage-in clamp), -2^-26 and +-2^-20 (h gives -0 and subnormal halves), integers with ties
    and columns whose values are all >= 0 by value with -0 among them after h: those stop after iteration 1 by value
    and would not by sign bit. B = 130: the per-layer path's second tile holds 2 codewords, the fused path's last group
    is ragged."""
    H, layers = hr.degree2_code()
    llr = hr.degree2_input(B)
    imax = 4
    p, f = both(engine, H, layers, imax, B)
    if B == 130:
        cw = f.geometry(B)[0]
        assert cw == 8 and B % cw != 0
    ref_on = hr.layered_half_decode(H, layers, llr, imax, record=True)
    assert (np.signbit(ref_on[0]) & (ref_on[0] == 0)).any() and np.abs(ref_on[0]).max() == 65504.0
    assert len(set(ref_on[1].tolist())) >= 2
    for early in (True, False):
        want = (ref_on[0], ref_on[1]) if early else (ref_on[2][-1], np.full(B, imax, np.int32))
        for dec in (p, f):
            got = gpu_decode(dec, llr, early)
            assert np.array_equal(got[1], want[1]), (dec.path, early)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (dec.path, early)


# ---------------------------------------------------------------------------------------------------------------
# 2. the two paths against each other
# ---------------------------------------------------------------------------------------------------------------
def _path_inputs(name):
    if name == "mixed":
        return hr.named_input("mixed_3dB")
    if name == "dvb":
        return hr.named_input("dvb")
    H, layers = wlan(int(name[4:]))
    if name == "wlan27":
        return hr.named_input("wlan27_1.5dB")
    return H, layers, awgn_llr(H.shape[1], 130, 1.5, seed=7)


@pytest.mark.parametrize("name", ["mixed", "wlan27", "wlan81", "dvb"])
def test_fused_and_per_layer_give_the_same_bits(engine, name):
    """mixed() (degrees 2..16; B = 9 and 130), wlan(27), wlan(81) and small_dvbs2(), i_max 8, stop on and off."""
    H, layers, llr = _path_inputs(name)
    p, f = both(engine, H, layers, hr.IMAX, 130)
    E = sp.csr_matrix(H).nnz
    cw_bytes = -(-(2 * H.shape[1] + 2 * E) // 4) * 4
    assert f.geometry(130)[0] == min(8, (160 * 1024) // cw_bytes) and p.geometry(130) == (0, 0, 0)
    for B in ((9, 130) if name == "mixed" else (130,)):
        for early in (True, False):
            a, b = gpu_decode(p, llr[:, :B], early), gpu_decode(f, llr[:, :B], early)
            assert same_bits(a, b), (name, B, early)
            if early:
                assert len(set(a[1].tolist())) >= 2


# ---------------------------------------------------------------------------------------------------------------
# 3. against the emulation, by value
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hr.NAMED)
def test_named_inputs_against_the_emulation(engine, name):
    H, layers, llr = hr.named_input(name)
    ref = hr.named_reference(name)
    p, f = both(engine, H, layers, hr.IMAX, 130)
    for early in (True, False):
        for dec in (p, f):
            compare(gpu_decode(dec, llr, early), ref, early, f"{name} {dec.path} early={early}")


# ---------------------------------------------------------------------------------------------------------------
# 5. full size
# ---------------------------------------------------------------------------------------------------------------
def test_full_size_per_layer(engine):
    """N = 64800 rate 1/2, B = 130 (two tiles of 128, the second holding 2 codewords), 2 iterations, stop on."""
    H, layers, llr = hr.full_size_input()
    assert H.shape == (32400, 64800) and llr.shape[1] == 130
    G = engine.Graph(H, "cuda:0")
    with pytest.raises(_lib.IBLError) as e:
        engine.LayeredBPDecoder(G, layers, hr.FULL_IMAX, 130, path="fused", state_dtype=F16)
    assert f"rc={_lib.IBL_EUNSUPPORTED}" in str(e.value) and "2 N + 2 E" in str(e.value)
    dec = engine.LayeredBPDecoder(G, layers, hr.FULL_IMAX, 130, path="auto", state_dtype=F16)
    assert dec.path_in_use == "passes" and dec.half
    ref = hr.layered_half_decode(H, layers, llr, hr.FULL_IMAX, record=True)
    compare(gpu_decode(dec, llr), ref, True, "N=64800")


# ---------------------------------------------------------------------------------------------------------------
# 6. reuse, graph capture, aliasing
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["passes", "fused"])
def test_reuse_graph_capture_and_aliasing(engine, path):
    """B = 130, then 5, then 130 on one handle give the bits of fresh handles (the per-layer path leaves the first
    decode's R rows behind and must not read them); a decode captured into a graph and replayed equals the eager one;
    `out` may be `llr`."""
    H, layers, llr = hr.named_input("dvb")
    G = engine.Graph(H, "cuda:0")

    def fresh():
        return engine.LayeredBPDecoder(G, layers, 4, 130, path=path, state_dtype=F16)

    dec = fresh()
    a130 = gpu_decode(dec, llr)
    a5 = gpu_decode(dec, llr[:, 60:65])
    b130 = gpu_decode(dec, llr)
    assert same_bits(a5, gpu_decode(fresh(), llr[:, 60:65])) and same_bits(a130, b130)
    assert same_bits(a130, gpu_decode(fresh(), llr))
    assert np.array_equal(a5[0].view(np.uint32), a130[0][:, 60:65].view(np.uint32))
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
    assert same_bits((out.cpu().numpy(), it.cpu().numpy()), eager)
    y = x.clone()
    it.zero_()
    dec.decode(y, out=y, iters=it)
    torch.cuda.synchronize(dev)
    assert same_bits((y.cpu().numpy(), it.cpu().numpy()), eager)


# ---------------------------------------------------------------------------------------------------------------
# 7. refusals and flags
# ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_flags(engine):
    H, layers = mixed()
    A = sp.lil_matrix(codes.canonical_csr(H))
    c = int(np.argmax(np.diff(codes.canonical_csr(H).indptr) == 16))
    A[c, [v for v in range(A.shape[1]) if A[c, v] == 0][0]] = 1
    H17 = codes.canonical_csr(sp.csr_matrix(A))
    with pytest.raises(_lib.IBLError) as e:
        engine.LayeredBPDecoder(engine.Graph(H17, "cuda:0"), codes.greedy_layers(H17), 5, 4, path="auto",
                                state_dtype=F16)
    assert f"rc={_lib.IBL_EUNSUPPORTED}" in str(e.value) and f"check {c} has degree 17" in str(e.value)
    Hw, lw = wlan(27)
    G = engine.Graph(Hw, "cuda:0")
    L = _lib.load()
    # ibl_layered_create_bp's order and messages: imax / max_batch, llr_max, path, then the layers
    nl, ptr, chk = _lib.pack_layers(lw)
    h = ctypes.c_void_p()
    for args, msg in (((0, 150.0, 4, _lib.IBL_PATH_AUTO), b"imax and max_batch must be >= 1"),
                      ((5, 150.0, 0, _lib.IBL_PATH_AUTO), b"imax and max_batch must be >= 1"),
                      ((5, float("inf"), 4, 77), b"llr_max must be finite and > 0"),
                      ((5, 0.0, 4, 77), b"llr_max must be finite and > 0")):
        assert L.ibl_layered_create_bp_half(G.handle, nl, ptr, chk, *args, ctypes.byref(h)) == _lib.IBL_EINVAL
        assert L.ibl_last_error() == msg and not h.value
    assert L.ibl_layered_create_bp_half(G.handle, nl, ptr, chk, 5, 150.0, 4, 77, ctypes.byref(h)) == _lib.IBL_EINVAL
    path_msg = L.ibl_last_error()
    assert L.ibl_layered_create_bp(G.handle, nl, ptr, chk, 5, 150.0, _lib.IBL_F32, 4, 77, ctypes.byref(h)) == \
        _lib.IBL_EINVAL and L.ibl_last_error() == path_msg
    for path in ("passes", "fused"):
        dec = engine.LayeredBPDecoder(G, lw, 5, 4, path=path, state_dtype=F16)
        assert dec.half is True
        for every in (2, 0):
            assert L.ibl_layered_set_compaction(dec._h, every, 25) == _lib.IBL_EUNSUPPORTED
            assert L.ibl_last_error() == b"compaction is not built for the BP decoder"
        n, ext = ctypes.c_int32(), ctypes.c_int32()
        assert L.ibl_layered_compaction_stats(dec._h, None, ctypes.byref(n), ctypes.byref(ext)) == _lib.IBL_EUNSUPPORTED
        for fn, want in ((L.ibl_layered_is_half, 1), (L.ibl_layered_is_bp, 1), (L.ibl_layered_is_wide, 0),
                         (L.ibl_layered_is_fixed, 0)):
            v = ctypes.c_int32(-1)
            assert fn(dec._h, ctypes.byref(v)) == _lib.IBL_OK and v.value == want
        with pytest.raises(ValueError, match="float32"):
            dec.decode(torch.zeros((648, 2), dtype=torch.float16, device=dec.device))
    for other in (engine.LayeredBPDecoder(G, lw, 5, 4), engine.LayeredBPDecoder(G, lw, 5, 4, path="passes"),
                  engine.LayeredDecoder(G, lw, 5, 4), engine.LayeredFixedDecoder(G, lw, 5, 4)):
        v = ctypes.c_int32(-1)
        assert L.ibl_layered_is_half(other._h, ctypes.byref(v)) == _lib.IBL_OK and v.value == 0
    assert engine.LayeredBPDecoder(G, lw, 5, 4).half is False
    with pytest.raises(ValueError, match="state_dtype"):
        engine.LayeredBPDecoder(G, lw, 5, 4, state_dtype=torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------
# 8. the drop-in class and the BER driver
# ---------------------------------------------------------------------------------------------------------------
def test_drop_in_class_and_ber_driver(engine):
    import informationbottleneckdecodingldpc_amd as pkg
    from informationbottleneckdecodingldpc_amd.awgn_quantizer import AWGN_Channel_Quantizer
    from informationbottleneckdecodingldpc_amd.ber import BERConfig, decoder_kind, run_ber
    from informationbottleneckdecodingldpc_amd.engine import count_below, philox_blocks
    H, layers, llr = hr.named_input("dvb")
    N = H.shape[1]
    dec = pkg.BeliefPropagation_Layered_Decoder_class_irregular(H, 8, 16, 64, layers=layers, path="passes",
                                                                state_dtype=F16)
    assert decoder_kind(dec) == "bp"
    out = dec.decode_OpenCL_belief_propagation(llr[:, :16])
    assert dec._dec.half and dec._dec.path_in_use == "passes"
    direct = engine.LayeredBPDecoder(engine.Graph(H, "cuda:0"), layers, 8, 64, path="passes", state_dtype=F16)
    want = gpu_decode(direct, llr[:, :16])
    assert same_bits((out, dec.last_iterations.cpu().numpy()), want)
    fp32 = pkg.BeliefPropagation_Layered_Decoder_class_irregular(H, 8, 16, 64, layers=layers, path="passes")
    o32 = fp32.decode_OpenCL_belief_propagation(llr[:, :16])
    assert not fp32._dec.half and not np.array_equal(o32, out)
    B, nb = 64, 2
    cfg = BERConfig(EbN0_dB_start=0.5, EbN0_dB_max_value=0.5, EbN0_dB_normal_stepwidth=0.1, min_errors=10 ** 9,
                    msg_at_time=B, max_blocks=nb * B, seed=5, llr_dtype=torch.float32)
    r = run_ber(dec, cfg)
    assert r.blocks == [nb * B] and len(r.EbN0_dB_vector) == 1
    db = r.EbN0_dB_vector[0]
    q = AWGN_Channel_Quantizer(10 ** (-db / 10) / (2 * dec.R_c), cfg.AD_max_abs, cfg.cardinality_T_channel,
                               cfg.cardinality_Y_channel, seed=5)
    q.init_OpenCL_quanti(N, B, return_buffer_only=True)
    n = 0
    for g in range(nb):
        q.offset = g * philox_blocks(N, B)
        ch = q.quantize_direct_OpenCL_LLR(N, B, dtype=torch.float32)
        n += int(count_below(direct.decode(ch), dec.data_len, 0.0).item())
    print("BER point: errors", list(r.errors), "direct", n)
    assert n > 0 and list(r.errors) == [float(n)]
