"""GPU: compaction of the running codewords on the layered decoder's fp32 per-layer path
(ibl_layered_set_compaction; csrc/layered_kernels.hip lay_compact_plan / lay_compact_rows / lay_compact_commit).
Compaction changes no value, so every comparison is np.array_equal on out and iters against the numpy restatement
of the decoder (tests/_layered_ref.py), and against a decoder without compaction; compaction_stats() equals the
count and the final extent the restated policy gives (tests/_layered_compact_ref.py), so a compaction that silently
never happens fails. tests/test_cpu_layered_compact.py holds the main input to one, two and three compactions."""
import functools

import numpy as np
import pytest
import torch

from informationbottleneckdecodingldpc_amd import _lib, codes
from tests import _layered_compact_ref as cr
from tests._layered_census import AB, FAMILIES, FAMILY_IMAX, awgn_llr, mixed, wlan
from tests._layered_ref import layered_decode

pytestmark = pytest.mark.gpu

NAB = (0.8125, 0.0)
PAIRS = [(1, 1), (1, 50), (2, 1)]


@pytest.fixture(scope="module")
def engine():
    from informationbottleneckdecodingldpc_amd import engine as e
    return e


@functools.lru_cache(maxsize=None)
def small():
    """DVB-S2-structured 3600 x 5400, its 10 residue layers, and 260 codewords of AWGN at 2.0 dB."""
    H = codes.dvbs2_structured(seed=5, n=5400, k=1800, groups_hi=2, deg_hi=7, deg_lo=2)
    llr = awgn_llr(5400, 260, 2.0, seed=7)
    llr.setflags(write=False)
    return H, codes.dvbs2_layers(H), llr


@functools.lru_cache(maxsize=None)
def small_ref(a=NAB[0], b=NAB[1], imax=10, early=True, B=260):
    H, layers, llr = small()
    out, it = layered_decode(H, layers, llr[:, :B], imax, a, b, early_stop=early)
    out.setflags(write=False)
    it.setflags(write=False)
    return out, it


@pytest.fixture(scope="module")
def small_graph(engine):
    return engine.Graph(small()[0], "cuda:0")


def make(engine, graph, imax=10, max_batch=260, ab=NAB, compact=None, layers=None, **kw):
    return engine.LayeredDecoder(graph, small()[1] if layers is None else layers, imax, max_batch, alpha=ab[0],
                                 beta=ab[1], path="passes", compact=compact, **kw)


def gpu_decode(dec, llr, early=True):
    it = torch.full((llr.shape[1],), -1, dtype=torch.int32, device=dec.device)
    out = dec.decode(torch.from_numpy(np.array(llr, order="C")).to(dec.device), early_stop=early, iters=it)
    return out.cpu().numpy(), it.cpu().numpy()


def check(dec, plain, llr, ref, early=True, what=""):
    """`dec` (with compaction) and `plain` (without) decode llr to the reference's values and counts; the
    compactions made and the final extent are the restated policy's. Returns the compactions."""
    B = llr.shape[1]
    out, it = gpu_decode(dec, llr, early)
    stats = dec.compaction_stats()
    every, pct = dec.compaction
    events, extent, _ = cr.compactions(ref[1], B, dec.imax, every, pct, early_stop=early)
    print(f"{what} B={B} compact={dec.compaction} early={early}: iters {np.bincount(ref[1]).tolist()}, policy "
          f"{events} -> extent {extent}, device {stats}, iters equal {np.array_equal(it, ref[1])}, out mismatches "
          f"{int((out != ref[0]).sum())}")
    assert np.array_equal(it, ref[1])
    assert np.array_equal(out, ref[0])
    assert stats == (len(events), extent)
    if plain is not None:
        p_out, p_it = gpu_decode(plain, llr, early)
        assert np.array_equal(p_out, out) and np.array_equal(p_it, it)
        assert plain.compaction is None and plain.compaction_stats() == (0, B)
    return events


@pytest.mark.parametrize("pair", PAIRS)
def test_small_long_code(engine, small_graph, pair):
    """Slices of the 260 draw: one codeword, a full tile, a tile and one column, two tiles and two columns, four
    tiles and four columns; with the stop (up to three compactions, tests/test_cpu_layered_compact.py) and without
    (none)."""
    H, layers, llr = small()
    dec, plain = make(engine, small_graph, compact=pair), make(engine, small_graph)
    assert dec.compaction == pair and dec.path_in_use == "passes"
    ref, fixed = small_ref(), small_ref(early=False, B=130)
    most = 0
    for B in (1, 64, 65, 130, 260):
        most = max(most, len(check(dec, plain, llr[:, :B], (ref[0][:, :B], ref[1][:B]), what="small")))
    assert most == (2 if pair == (1, 50) else 3)
    for B in (65, 130):
        assert check(dec, plain, llr[:, :B], (fixed[0][:, :B], fixed[1][:B]), early=False, what="no stop") == []


def strong_batches():
    """B = 130 on the small code; the columns set to +4.0 are finished by the stop check of iteration 1."""
    H, layers, awgn = small()
    base = np.array(awgn[:, :130])
    cols = {"first_tile": np.arange(64), "every_second": np.arange(0, 130, 2), "all_but_last": np.arange(129),
            "all": np.arange(130), "none": np.arange(0)}
    for name, strong in cols.items():
        x = base.copy()
        x[:, strong] = np.float32(4.0)
        yield name, x, strong, (2 if name == "none" else 10)


@pytest.mark.parametrize("name", ["first_tile", "every_second", "all_but_last", "all", "none"])
def test_built_batches(engine, small_graph, name):
    H, layers, _ = small()
    x, strong, imax = next((x, s, i) for n, x, s, i in strong_batches() if n == name)
    ref = layered_decode(H, layers, x, imax, *NAB)
    assert (ref[1][strong] == 1).all() and (np.delete(ref[1], strong) > 1).all()
    dec, plain = make(engine, small_graph, imax=imax, max_batch=130, compact=(1, 1)), None
    if name == "first_tile":
        plain = make(engine, small_graph, imax=imax, max_batch=130)
    events = check(dec, plain, x, ref, what=name)
    if name in ("first_tile", "every_second", "all_but_last"):
        assert events[0] == (1, 130, 130 - len(strong))
    else:   # all finished: `running` is 0, every later launch leaves, out is complete; none: nothing to free
        assert events == []


def test_alpha_beta(engine, small_graph):
    H, layers, llr = small()
    for ab in AB:
        ref = small_ref(ab[0], ab[1], 10, True, 130)
        check(make(engine, small_graph, max_batch=130, ab=ab, compact=(1, 1)), None, llr[:, :130], ref, what=f"ab={ab}")


@pytest.mark.parametrize("code,family", [("mixed", "subnormal_boundary"), ("wlan27", "subnormal")])
def test_other_codes(engine, code, family):
    """Check degrees 2..16 with greedy layers of uneven size, and WLAN Z = 27 (codes the fused kernel would take),
    through path="passes" at B = 130, one edge family each."""
    H, layers = mixed() if code == "mixed" else wlan(27)
    G = engine.Graph(H, "cuda:0")
    gen, params = FAMILIES[family]
    llr = gen(H, 130)
    a, b, L = params[-1]
    ref = layered_decode(H, layers, llr, FAMILY_IMAX, a, b, L)
    dec = make(engine, G, imax=FAMILY_IMAX, max_batch=130, ab=(a, b), compact=(1, 1), layers=layers, llr_max=L)
    plain = make(engine, G, imax=FAMILY_IMAX, max_batch=130, ab=(a, b), layers=layers, llr_max=L)
    assert len(check(dec, plain, llr, ref, what=f"{code} {family}")) == (1 if code == "mixed" else 2)


def test_many_tiles(engine):
    """WLAN Z = 27 at B = 4230: 67 tiles, so the plan's scan takes a second trip (64 tiles a trip), the row move
    17 chunks of 256 columns and the commit 17 of its own; six compactions, the first from a padded tile."""
    H, layers = wlan(27)
    G = engine.Graph(H, "cuda:0")
    llr = awgn_llr(648, 4230, 2.5, seed=11)
    ref = layered_decode(H, layers, llr, 8, *NAB)
    dec = make(engine, G, imax=8, max_batch=4230, compact=(1, 1), layers=layers)
    events = check(dec, make(engine, G, imax=8, max_batch=4230, layers=layers), llr, ref, what="many tiles")
    assert len(events) == 6 and events[0] == (2, 4230, 4011)


def test_in_place_no_iters_side_stream(engine, small_graph):
    H, layers, llr = small()
    ref = small_ref()
    dec = make(engine, small_graph, compact=(1, 1))
    t = torch.from_numpy(np.array(llr[:, :130])).to(dec.device)
    out = dec.decode(t.clone(), iters=None)
    assert np.array_equal(out.cpu().numpy(), ref[0][:, :130]) and dec.compaction_stats() == (2, 62)
    it = torch.full((130,), -1, dtype=torch.int32, device=dec.device)
    same = dec.decode(t, out=t, iters=it)      # finished codewords are flushed into llr mid-decode: read at stage-in only
    assert same is t
    assert np.array_equal(t.cpu().numpy(), ref[0][:, :130]) and np.array_equal(it.cpu().numpy(), ref[1][:130])
    t = torch.from_numpy(np.array(llr)).to(dec.device)
    it = torch.full((260,), -1, dtype=torch.int32, device=dec.device)
    torch.cuda.synchronize(dec.device)
    side = torch.cuda.Stream(device=dec.device)
    with torch.cuda.stream(side):
        out = dec.decode(t, iters=it)
        in_stream = dec.compaction_stats()
    assert dec.compaction_stats(side) == in_stream == (3, 48)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref[0]) and np.array_equal(it.cpu().numpy(), ref[1])


def test_descending_reuse_and_switching_off(engine, small_graph):
    """One handle decodes B = 260, then 65, then 130 (columns from the far end, so unlike inputs): the maps, the
    extent and the count of the wider decode do not leak. Then every = 0 on the same handle: the launches of a
    decoder that never had compaction, the same values, no compactions; and on again."""
    H, layers, llr = small()
    ref = small_ref()
    dec = make(engine, small_graph, compact=(1, 1))
    for B in (260, 65, 130):
        check(dec, None, llr[:, 260 - B:], (ref[0][:, 260 - B:], ref[1][260 - B:]), what="reuse")
    dec.compaction = None
    assert dec.compaction is None
    out, it = gpu_decode(dec, llr)
    assert np.array_equal(out, ref[0]) and np.array_equal(it, ref[1]) and dec.compaction_stats() == (0, 260)
    dec.compaction = True
    assert dec.compaction == engine.LayeredDecoder.COMPACT_DEFAULT
    check(dec, None, llr, ref, what="on again")
    with pytest.raises(ValueError):
        dec.compaction = (0, 25)
    with pytest.raises(_lib.IBLError) as e:
        dec.compaction = (1, 101)
    assert f"rc={_lib.IBL_EINVAL}" in str(e.value) and dec.compaction == engine.LayeredDecoder.COMPACT_DEFAULT


def test_refusals_with_a_device(engine, small_graph):
    H, layers, _ = small()
    with pytest.raises(_lib.IBLError) as e:
        engine.LayeredDecoder(small_graph, layers, 5, 8, path="fused", compact=True)
    assert f"rc={_lib.IBL_EUNSUPPORTED}" in str(e.value) and "compaction needs the per-layer path" in str(e.value)
    fused = engine.LayeredDecoder(small_graph, layers, 5, 8, path="fused")
    with pytest.raises(_lib.IBLError) as e:
        fused.compaction_stats()
    assert "compaction needs the per-layer path" in str(e.value)
    fixed = engine.LayeredFixedDecoder(small_graph, layers, 5, 8)
    assert not hasattr(fixed, "compaction")
    L = _lib.load()
    for every in (2, 0):
        assert L.ibl_layered_set_compaction(fixed._h, every, 25) == _lib.IBL_EUNSUPPORTED
        assert L.ibl_last_error().decode() == "compaction is not built for the fixed-point decoder"


def test_driver_counts_equal():
    """Min_Sum_Layered_Decoder_class_irregular(compact=...) through ber.run_ber: the same seed gives the same
    Philox channel stream, so the decoder counts the same errors with and without compaction. At 2.0 dB (the
    Eb/N0 of the main input, whose reference has 57 of 260 codewords finished after 4 iterations and 33 running at
    10) a batch of 130 frees a tile before iteration 8 and some frames stay in error."""
    import informationbottleneckdecodingldpc_amd as pkg
    from informationbottleneckdecodingldpc_amd.ber import BERConfig, run_ber
    H, layers, _ = small()
    res = {}
    for compact in (None, (1, 1)):
        dec = pkg.Min_Sum_Layered_Decoder_class_irregular(H, 8, 16, 130, layers=layers, alpha=NAB[0], path="passes",
                                                          compact=compact)
        cfg = BERConfig(EbN0_dB_start=2.0, EbN0_dB_max_value=2.0, min_errors=10 ** 9, msg_at_time=130,
                        max_blocks=260, seed=5, llr_dtype=torch.float32)
        r = run_ber(dec, cfg)
        assert dec._dec.compaction == compact
        res[compact] = (list(r.errors), list(r.blocks), dec._dec.compaction_stats())
    print("driver counters:", res)
    assert res[None][1] == [260] and res[None][0][0] > 0
    assert res[None][:2] == res[(1, 1)][:2]
    assert res[None][2] == (0, 130) and res[(1, 1)][2][0] >= 1


def test_full_size(engine):
    """DVB-S2-structured N = 64800 rate 1/2, 90 layers, 70 columns (two tiles, the second of 6 lanes), 3 iterations:
    columns 0..5 AWGN at 1.0 dB, the other 64 noiseless — one compaction, 70 -> 6 columns, after iteration 1."""
    H = codes.dvbs2_structured(seed=3)
    layers = codes.dvbs2_layers(H)
    llr = awgn_llr(64800, 70, 1.0, seed=17)
    llr[:, 6:] = np.float32(4.0)
    ref = layered_decode(H, layers, llr, 3, *NAB)
    assert (ref[1][6:] == 1).all() and (ref[1][:6] == 3).all()
    dec = engine.LayeredDecoder(engine.Graph(H, "cuda:0"), layers, 3, 70, alpha=NAB[0], beta=NAB[1], path="auto",
                                compact=(1, 1))
    assert dec.path_in_use == "passes"
    assert check(dec, None, llr, ref, what="full size") == [(1, 70, 6)]
