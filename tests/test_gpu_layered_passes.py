"""GPU: the layered min-sum decoder's per-layer path over HBM (ibl_layered_create_path IBL_PATH_PASSES / AUTO,
csrc/layered_kernels.hip lay_layer ...) against the numpy float32 restatement of the specification
(tests/_layered_ref.py): outputs equal as values (np.array_equal), per-codeword iteration counts exactly, no
tolerance. The inputs are those of tests/_layered_census.py (tests/test_cpu_layered.py holds them to their
arithmetic edges); the long-code shape is a DVB-S2-structured N = 5400 code (10 residue layers of 360 checks) that
the fused kernel also fits, so the two paths are compared on the same tensors, and the full-size N = 64800 code."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from informationbottleneckdecodingldpc_amd import _lib, codes
from tests._layered_census import (AB, FAMILIES, FAMILY_B, FAMILY_IMAX, MIXED_BATCH_COLUMNS, awgn_llr, mixed,
                                   mixed_batch_llr, quantised_llr, wlan)
from tests._layered_ref import layered_decode

pytestmark = pytest.mark.gpu

NAB = (0.8125, 0.0)


@pytest.fixture(scope="module")
def engine():
    from informationbottleneckdecodingldpc_amd import engine as e
    return e


@functools.lru_cache(maxsize=None)
def small():
    """DVB-S2-structured 3600 x 5400 (check degrees {3: 1, 4: 3599}), its 10 residue layers, and 130 codewords of
    AWGN at 2.0 dB (all-zero codeword)."""
    H = codes.dvbs2_structured(seed=5, n=5400, k=1800, groups_hi=2, deg_hi=7, deg_lo=2)
    llr = awgn_llr(5400, 130, 2.0, seed=7)
    llr.setflags(write=False)
    return H, codes.dvbs2_layers(H), llr


@functools.lru_cache(maxsize=None)
def small_ref(a, b, imax, early):
    H, layers, llr = small()
    out, it = layered_decode(H, layers, llr, imax, a, b, early_stop=early)
    out.setflags(write=False)
    it.setflags(write=False)
    return out, it


@pytest.fixture(scope="module")
def small_graph(engine):
    return engine.Graph(small()[0], "cuda:0")


def gpu_decode(dec, llr, early):
    it = torch.full((llr.shape[1],), -1, dtype=torch.int32, device=dec.device)
    out = dec.decode(torch.from_numpy(np.array(llr, order="C")).to(dec.device), early_stop=early, iters=it)
    return out.cpu().numpy(), it.cpu().numpy()


def check(dec, llr, early, ref, what=""):
    out, it = gpu_decode(dec, llr, early)
    r_out, r_it = ref
    print(f"{what} early={early} B={llr.shape[1]}: iters {np.bincount(r_it).tolist()}, iters equal "
          f"{np.array_equal(it, r_it)}, out mismatches {int((out != r_out).sum())}")
    assert np.array_equal(it, r_it)
    assert np.array_equal(out, r_out)
    return out, it


@pytest.mark.parametrize("ab", AB)
def test_small_long_code(engine, small_graph, ab):
    """1, 2 and 10 iterations, early stop on and off, batches of 1, one less than / equal to / one more than a
    tile of 64 and two tiles and two columns; one reference for the widest batch, sliced. The fused kernel decodes
    the same tensors to the same values."""
    H, layers, llr = small()
    a, b = ab
    for imax in (1, 2, 10):
        dec = engine.LayeredDecoder(small_graph, layers, imax, 130, alpha=a, beta=b, path="passes")
        assert dec.path_in_use == "passes" and dec.geometry(130) == (0, 0, 0)
        fused = engine.LayeredDecoder(small_graph, layers, imax, 130, alpha=a, beta=b, path="fused")
        assert fused.path_in_use == "fused" and fused.geometry(130)[0] == 2
        for early in (True, False):
            ref = small_ref(a, b, imax, early)
            for B in (1, 63, 64, 65, 130):
                out, it = check(dec, llr[:, :B], early, (ref[0][:, :B], ref[1][:B]), f"imax={imax} ab={ab}")
                f_out, f_it = gpu_decode(fused, llr[:, :B], early)
                assert np.array_equal(f_out, out) and np.array_equal(f_it, it)


def test_small_input_spreads_the_stops():
    """Conditions on the input of the (0.8125, 0) / 10 iterations / early-stop case: codewords stop after at
    least 4 distinct iteration counts and some codeword is unconverged at 10."""
    H, layers, llr = small()
    out, it = small_ref(*NAB, 10, True)
    hist = np.bincount(it, minlength=11)
    print("reference iters histogram:", {i: int(c) for i, c in enumerate(hist) if c})
    assert (hist > 0).sum() >= 4
    unconverged = ((sp.csr_matrix(H) @ (out < 0).astype(np.int64)) % 2 != 0).any(axis=0)
    assert (unconverged & (it == 10)).any()


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("code", ["mixed", "wlan27"])
def test_edge_families(engine, code, family):
    """Ties, zeros of either sign, the clamp, llr_max = 7.5 and subnormals (tests/_layered_census.py) on check
    degrees 2..16 with greedy layers of uneven size (some smaller than a wave's worth of items) and on WLAN
    Z = 27; B = 16, 6 iterations, early stop on and off."""
    H, layers = mixed() if code == "mixed" else wlan(27)
    G = engine.Graph(H, "cuda:0")
    gen, params = FAMILIES[family]
    llr = gen(H, FAMILY_B)
    for a, b, L in params:
        dec = engine.LayeredDecoder(G, layers, FAMILY_IMAX, FAMILY_B, alpha=a, beta=b, llr_max=L, path="passes")
        for early in (True, False):
            ref = layered_decode(H, layers, llr, FAMILY_IMAX, a, b, L, early_stop=early)
            check(dec, llr, early, ref, f"{family} {code} a={a} b={b} L={L}")


def test_mixed_batch(engine):
    """Neighbouring columns from different families stop at unlike times inside one tile (67 columns: one full
    tile and three lanes of the next)."""
    H, layers = mixed()
    G = engine.Graph(H, "cuda:0")
    col = {k: i for i, k in enumerate(MIXED_BATCH_COLUMNS)}
    llr = mixed_batch_llr(H.shape[1], 67, seed=31)
    for a, b in AB:
        dec = engine.LayeredDecoder(G, layers, FAMILY_IMAX, 67, alpha=a, beta=b, path="passes")
        for early in (True, False):
            ref = layered_decode(H, layers, llr, FAMILY_IMAX, a, b, early_stop=early)
            out, it = check(dec, llr, early, ref, f"mixed batch a={a} b={b}")
            for z in (col["zeros"], col["negative_zeros"]):
                assert it[z] == (1 if early else FAMILY_IMAX) and (out[:, z] == 0).all()
            assert not early or len(set(it.tolist())) >= 2


def test_tile_skipping(engine, small_graph):
    """Columns 0..63 noiseless (+4.0): the whole first tile is finished after iteration 1 and skipped from then
    on; columns 64..129 AWGN at 2.0 dB go on. A finished lane written again, or a skipped tile that was needed,
    shows in out or iters."""
    H, layers, awgn = small()
    llr = np.array(awgn)
    llr[:, :64] = np.float32(4.0)
    ref = layered_decode(H, layers, llr, 10, *NAB)
    assert (ref[1][:64] == 1).all() and ref[1][64:].min() > 1
    dec = engine.LayeredDecoder(small_graph, layers, 10, 130, alpha=NAB[0], beta=NAB[1], path="passes")
    check(dec, llr, True, ref, "tile skipping")


@pytest.mark.parametrize("form", ["gather", "packed"])
def test_syndrome_forms(engine, small_graph, monkeypatch, form):
    """Both syndrome forms (IBL_LAY_SYNDROME at create; the other tests run the default): the small long code at
    65 and 130 codewords (a second tile of 1 and of 2 lanes), and every check degree 2..16 with a last run of
    checks and of variables shorter than 64, on the quantised family (zeros of either sign in the decisions)."""
    monkeypatch.setenv("IBL_LAY_SYNDROME", form)
    H, layers, llr = small()
    ref = small_ref(*NAB, 10, True)
    dec = engine.LayeredDecoder(small_graph, layers, 10, 130, alpha=NAB[0], beta=NAB[1], path="passes")
    for B in (65, 130):
        check(dec, llr[:, :B], True, (ref[0][:, :B], ref[1][:B]), form)
    Hm, lm = mixed()
    assert Hm.shape[0] % 64 and Hm.shape[1] % 64
    x = quantised_llr(Hm.shape[1], 67, seed=41)
    dm = engine.LayeredDecoder(engine.Graph(Hm, "cuda:0"), lm, FAMILY_IMAX, 67, path="passes")
    check(dm, x, True, layered_decode(Hm, lm, x, FAMILY_IMAX), form + " mixed")
    monkeypatch.setenv("IBL_LAY_SYNDROME", "neither")
    with pytest.raises(_lib.IBLError):
        engine.LayeredDecoder(small_graph, layers, 10, 130, path="passes")


@pytest.mark.parametrize("early", [True, False])
def test_full_size(engine, early):
    """DVB-S2-structured N = 64800 rate 1/2, its 90 residue layers, path="auto": 69 columns of AWGN at 1.0 dB and
    one noiseless column (two tiles, the second of 6 lanes); 3 iterations."""
    H = codes.dvbs2_structured(seed=3)
    layers = codes.dvbs2_layers(H)
    assert len(layers) == 90
    llr = awgn_llr(64800, 70, 1.0, seed=17)
    llr[:, 41] = np.float32(4.0)
    dec = engine.LayeredDecoder(engine.Graph(H, "cuda:0"), layers, 3, 70, alpha=NAB[0], beta=NAB[1], path="auto")
    assert dec.path_in_use == "passes" and dec.geometry(70) == (0, 0, 0)
    ref = layered_decode(H, layers, llr, 3, *NAB, early_stop=early)
    assert ref[1][41] == (1 if early else 3)
    check(dec, llr, early, ref, "full size")


def test_api(engine, small_graph):
    H27, l27 = wlan(27)
    G27 = engine.Graph(H27, "cuda:0")
    assert engine.LayeredDecoder(G27, l27, 5, 8, path="auto").path_in_use == "fused"
    assert engine.LayeredDecoder(G27, l27, 5, 8).path_in_use == "fused"
    with pytest.raises(ValueError):
        engine.LayeredDecoder(G27, l27, 5, 8, path="hbm")
    with pytest.raises(_lib.IBLError) as e:
        engine.LayeredDecoder(G27, l27, 5, 8, precision=torch.float64, path="passes")
    assert f"rc={_lib.IBL_EUNSUPPORTED}" in str(e.value)
    H81, l81 = wlan(81)
    dec = engine.LayeredDecoder(engine.Graph(H81, "cuda:0"), l81, 6, 16, alpha=0.75, path="passes")
    assert dec.path_in_use == "passes" and dec.geometry(16) == (0, 0, 0)
    llr = awgn_llr(1944, 16, 2.0, seed=7)
    check(dec, llr, True, layered_decode(H81, l81, llr, 6, 0.75, 0.0), "wlan81 passes")


@pytest.fixture(scope="module")
def small_dec(engine, small_graph):
    H, layers, llr = small()
    return engine.LayeredDecoder(small_graph, layers, 10, 130, alpha=NAB[0], beta=NAB[1], path="passes")


def test_in_place_and_no_iters(small_dec):
    H, layers, llr = small()
    ref = small_ref(*NAB, 10, True)
    t = torch.from_numpy(np.array(llr[:, :65])).to(small_dec.device)
    out = small_dec.decode(t.clone(), iters=None)
    assert np.array_equal(out.cpu().numpy(), ref[0][:, :65])
    it = torch.full((65,), -1, dtype=torch.int32, device=small_dec.device)
    same = small_dec.decode(t, out=t, iters=it)
    assert same is t
    assert np.array_equal(t.cpu().numpy(), ref[0][:, :65]) and np.array_equal(it.cpu().numpy(), ref[1][:65])


def test_side_stream(small_dec):
    H, layers, llr = small()
    ref = small_ref(*NAB, 10, True)
    t = torch.from_numpy(np.array(llr[:, :65])).to(small_dec.device)
    it = torch.full((65,), -1, dtype=torch.int32, device=small_dec.device)
    torch.cuda.synchronize(small_dec.device)
    side = torch.cuda.Stream(device=small_dec.device)
    with torch.cuda.stream(side):
        out = small_dec.decode(t, iters=it)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref[0][:, :65]) and np.array_equal(it.cpu().numpy(), ref[1][:65])


def test_descending_reuse_and_batch_too_large(small_dec):
    """One decoder decodes B = 130, then 64, then 1 (columns from the far end of the batch, so unlike inputs):
    stale rows, masks and counters of the wider decode do not leak."""
    H, layers, llr = small()
    ref = small_ref(*NAB, 10, True)
    for B in (130, 64, 1):
        check(small_dec, llr[:, 130 - B:], True, (ref[0][:, 130 - B:], ref[1][130 - B:]), "reuse")
    t = torch.zeros((5400, 131), dtype=torch.float32, device=small_dec.device)
    with pytest.raises(_lib.IBLError) as e:
        small_dec.decode(t)
    assert f"rc={_lib.IBL_EINVAL}" in str(e.value)


def test_driver_counts_equal_fused():
    """Min_Sum_Layered_Decoder_class_irregular(path=...) through ber.run_ber: the same seed gives the same Philox
    channel stream, so the per-layer and the fused decoder count the same errors."""
    import informationbottleneckdecodingldpc_amd as pkg
    from informationbottleneckdecodingldpc_amd.ber import BERConfig, run_ber
    H, layers, _ = small()
    cls = pkg.Min_Sum_Layered_Decoder_class_irregular
    with pytest.raises(ValueError):
        cls(H, 8, 16, 64, layers=layers, path="hbm")
    res = {}
    for path in ("passes", "fused"):
        dec = cls(H, 8, 16, 64, layers=layers, alpha=NAB[0], path=path)
        cfg = BERConfig(EbN0_dB_start=1.5, EbN0_dB_max_value=1.5, min_errors=10 ** 9, msg_at_time=64,
                        max_blocks=128, seed=5, llr_dtype=torch.float32)
        r = run_ber(dec, cfg)
        assert dec._dec.path_in_use == path
        res[path] = (list(r.errors), list(r.blocks))
    print("driver counters:", res)
    assert res["passes"][1] == [128] and res["passes"][0][0] > 0
    assert res["passes"] == res["fused"]
