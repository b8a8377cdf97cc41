"""GPU: the layered BP decoder (csrc/layered_bp_kernels.hip) on nonzero codewords, at the edges of its clamps and
under the caller patterns of tests/test_gpu_layered.py. The reference is always the float64 restatement
(tests/_layered_bp_ref.py), the bars are those of tests/test_gpu_layered_bp.py compare — every value within SURVEY
H5, no hard decision flipped outside H5's band around zero, iters equal except on excusable codewords, at most 2 %
of a batch rounded up — and the fused kernel and the per-layer kernels, wherever the fused kernel accepts the code,
are held to IDENTICAL bits and equal iters of each other. tests/test_cpu_layered_bp.py pins the premises of every
input here on the references alone.

The unconverged-column rule (precedent: test_gpu_layered_bp.py test_wlan_fused_small_llr_max_stays_converged): a
codeword the reference does not converge amplifies rounding differences from iteration to iteration — the numpy
float32 form of the reference itself leaves H5 on such a column of the saturating input on `mixed` — so it is held
to iters, to finite values, and to H5 after a separate decode of the whole batch with i_max = 1."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from informationbottleneckdecodingldpc_amd import _lib
from tests import _codewords as cw
from tests import _layered_bp_ref as br
from tests.test_gpu_layered_bp import compare, cut, gpu_decode

pytestmark = pytest.mark.gpu
PATHS = ("passes", "fused")


@pytest.fixture(scope="module")
def engine():
    from informationbottleneckdecodingldpc_amd import engine as e
    return e


@pytest.fixture(scope="module")
def graphs(engine):
    made = {}

    def graph(name):
        if name not in made:
            made[name] = engine.Graph(cw.code(name)[0], "cuda:0")
        return made[name]
    return graph


def fused_fits(H):
    """The fit rule of include/ibldpc.h "Layered BP": a codeword's 4 N + 4 E bytes within 160 KiB of LDS."""
    return 4 * H.shape[1] + 4 * sp.csr_matrix(H).nnz <= 160 * 1024


def decoders(engine, graphs, name, imax, max_batch, llr_max=150.0):
    """path -> decoder of tests/_codewords.py code(name), both paths where the fused kernel accepts the code (a
    refusal where the fit rule says it fits, or a handle where it does not, fails here)."""
    H, _, layers, _ = cw.code(name)
    made = {}
    for path in PATHS:
        if path == "fused" and not fused_fits(H):
            with pytest.raises(_lib.IBLError) as e:
                engine.LayeredBPDecoder(graphs(name), layers, imax, max_batch, llr_max=llr_max, path=path)
            assert f"rc={_lib.IBL_EUNSUPPORTED}" in str(e.value)
            continue
        made[path] = engine.LayeredBPDecoder(graphs(name), layers, imax, max_batch, llr_max=llr_max, path=path)
        assert made[path].path_in_use == path
    return made


def decode_all(decs, llr, early=True):
    """path -> (out, iters), the paths bit for bit equal."""
    got = {path: gpu_decode(dec, llr, early) for path, dec in decs.items()}
    first = got[next(iter(got))]
    for path, g in got.items():
        assert np.array_equal(g[1], first[1]), path
        assert np.array_equal(g[0].view(np.uint32), first[0].view(np.uint32)), path
    return got


def judge(got, ref, label, got1=None, ref1=None, free=()):
    """compare() on the columns the reference converges (ref[4]); the unconverged-column rule on the others: iters,
    finite values, and compare() of the i_max = 1 decode got1 with its reference ref1 on every column. `free`:
    columns held to finite values and H5 only (against br.reference_for_columns)."""
    out, it = got
    conv = np.array(ref[4], copy=True)
    held = np.ones(conv.size, dtype=bool)
    held[list(free)] = False
    assert np.isfinite(out).all(), label
    cols = np.flatnonzero(conv & held)
    compare((out[:, cols], it[cols]), cut(ref, cols=cols), f"{label}, the {cols.size} converged columns")
    rest = np.flatnonzero(~conv & held)
    if rest.size:
        differ = it[rest] != ref[1][rest]
        print(f"{label}, unconverged columns {rest.tolist()}: iters {it[rest].tolist()}, reference "
              f"{ref[1][rest].tolist()}, excusable {ref[2][rest].tolist()}")
        assert not (differ & ~ref[2][rest]).any()
        assert int((differ & ref[2][rest]).sum()) <= br.excuse_cap(conv.size)
        assert got1 is not None, "an unconverged column needs the i_max = 1 decode"
    if got1 is not None:
        assert (got1[1] == 1).all()
        compare(got1, ref1, f"{label}, i_max 1, every column")
    if len(free):
        free = np.array(sorted(free))
        bad = br.h5_violations(out[:, free], br.reference_for_columns(it[free], cut(ref, cols=free)))
        assert not bad.any(), (label, free.tolist())


# ---------------------------------------------------------------------------------------------------------------
# 1. nonzero codewords, the per-codeword stop
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wlan", "mixed", "dvb"])
def test_nonzero_codewords(engine, graphs, name):
    """br.spread_input(name) (tests/_codewords.py layered_input; on wlan the noise columns at half magnitude, why:
    there): nonzero codewords at 6 and 3 dB, the all-zero codeword and sign-random noise, B = 130 (N = 648, 400 with
    check degrees 2..16, 7200), i_max 8, the stop on and off, both paths (dvb: 4 N + 4 E = 129,596 bytes, one codeword a workgroup). The fused kernel's own syndrome loop meets
    decisions that are 1; odd tiles of 64 hold early stoppers only, so the per-layer path skips whole tiles and
    freezes finished lanes beside running ones. On every column the reference converges the decisions are the
    transmitted bits; the 8 noise columns report iters == 8.
    Reference iters (tests/test_cpu_layered_bp.py SPREAD_HIST): wlan [0,63,39,13,3,3,1,0,8], mixed
    [0,84,21,6,4,3,0,1,11], dvb [0,2,92,6,21,1,0,0,8]; excusable columns wlan none, mixed [1], dvb
    [3,19,35,51,59].
    Measured on an MI355X, both paths alike, stop on / off: wlan largest |difference| 8.3e-5 / 6.1e-4, largest
    relative difference 4.9e-5, no column excused; mixed 7.5e-5 / 5.6e-4, relative 1.1 (a value in the band),
    column 1 excused: the GPU stops it an iteration apart from the reference and is compared with the reference's
    values at its own stop; dvb 7.2e-5 / 3.9e-4, relative 0.028, none excused. No value outside H5, no flip."""
    H, _, layers, _ = cw.code(name)
    llr, bits, kinds = br.spread_input(name)
    decs = decoders(engine, graphs, name, cw.IMAX_LAYERED, cw.LAYERED_B)
    assert set(decs) == set(PATHS) and decs["fused"].geometry(1)[0] == (1 if name == "dvb" else 8)
    for early in (True, False):
        ref = br.spread_reference(name, early)
        conv = ref[4]
        for path, got in decode_all(decs, llr, early).items():
            compare(got, ref, f"{name} {path} early={early}")
            out, it = got
            assert np.array_equal((out < 0)[:, conv], (bits == 1)[:, conv])
            assert (it[kinds == cw.KIND_NOISE] == cw.IMAX_LAYERED).all()
            if early:
                assert (it[64:128] <= 4).all() and (it[:64] == cw.IMAX_LAYERED).any()
            else:
                assert (it == cw.IMAX_LAYERED).all()


@pytest.mark.parametrize("name", ["wlan", "mixed", "dvb"])
def test_nonzero_columns_alone(engine, graphs, name):
    """Eight columns of that batch — the earliest and the latest stopper, a noise column, 63, 64, 129 and two more
    — decoded alone on the same handle give the bits and iters they have in the batch
    (test_gpu_layered_bp.py test_freezing_and_independence, on nonzero codewords)."""
    llr, _, kinds = br.spread_input(name)
    _, r_it, _, _, conv = br.spread_reference(name)
    stopped = np.flatnonzero(conv & cw.converged(r_it))
    cols = [int(stopped[np.argmin(r_it[stopped])]), int(stopped[np.argmax(r_it[stopped])]),
            int(np.flatnonzero(kinds == cw.KIND_NOISE)[0]), 63, 64, 129]
    cols += [c for c in (31, 97, 100, 17, 5, 70) if c not in cols][:8 - len(set(cols))]
    cols = sorted(set(cols))
    assert len(cols) == 8 and len(set(r_it[cols].tolist())) >= 3
    for path, dec in decoders(engine, graphs, name, cw.IMAX_LAYERED, cw.LAYERED_B).items():
        out, it = gpu_decode(dec, llr)
        for c in cols:
            o1, i1 = gpu_decode(dec, llr[:, c:c + 1])
            assert i1[0] == it[c], (path, c)
            assert np.array_equal(o1[:, 0].view(np.uint32), out[:, c].view(np.uint32)), (path, c)


def test_group_loop_nonzero(engine, graphs):
    """The fused kernel's group loop on nonzero codewords: tests/test_gpu_codewords.py
    test_layered_fused_group_loop's construction — every workgroup decodes a second and a third group, the last
    group is ragged — on spread_input("wlan", B); 64 columns spread over the batch, the last cw + 1 included,
    against the reference, and the decisions of every stopped column of the batch against the transmitted bits.
    Measured on an MI355X (B = 4105): reference iters of the 64 columns [0,35,15,4,5,0,0,0,5], none excusable,
    largest |difference| 4.3e-5, largest relative difference 4.2e-5."""
    H, _, layers, _ = cw.code("wlan")
    cap = 1 << 16
    dec = engine.LayeredBPDecoder(graphs("wlan"), layers, cw.IMAX_LAYERED, cap)
    per, _, grid = dec.geometry(cap)
    B = per * (2 * grid + 1) + 1
    assert grid < -(-cap // per) and B <= cap, f"B = {B} (cw_per_group {per}, grid {grid}): raise cap"
    assert dec.geometry(B) == (per, 2 * grid + 2, grid)
    llr, bits, kinds = br.spread_input("wlan", B)
    third = 2 * per * grid
    cols = np.unique(np.concatenate([np.linspace(0, third - 1, 64 - (B - third)).astype(np.int64),
                                     np.arange(third, B)]))
    assert cols.size == 64 and (cols >= third).sum() == per + 1 and len(set(kinds[cols].tolist())) >= 3
    ref = br.reference_with_excusable(H, layers, llr[:, cols], cw.IMAX_LAYERED, record=True)
    assert len(set(ref[1].tolist())) >= 3
    out, it = gpu_decode(dec, llr)
    compare((out[:, cols], it[cols]), ref, "group loop, nonzero codewords")
    stopped = cw.converged(it)
    assert stopped.sum() >= B // 2 and np.array_equal((out < 0)[:, stopped], (bits == 1)[:, stopped])
    assert (it[kinds == cw.KIND_NOISE] == cw.IMAX_LAYERED).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. a saturating input that carries the codeword; 3. a small llr_max on every degree
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["saturating", "overflow"])
@pytest.mark.parametrize("name", ["mixed", "wlan"])
def test_saturating_codewords(engine, graphs, name, kind):
    """br.saturating_input: awgn_llr(3 dB) x 40, 1 % of the entries 2^126 ("overflow": 2^127, where |a| + |b| of two
    of them is inf in fp32; both inside the precondition), 1 % exactly 150, negated by the codeword's bits; B = 16,
    i_max 6, stop on and off, both paths. A degree-2 check sees |Q| > llr_max (the fmed3 of lay_bp<2>) and a
    box-plus two inputs beyond llr_max (the upper clamp of boxplus): the reference without either clamp leaves H5
    on converged columns (tests/test_cpu_layered_bp.py). Reference iters mixed [0,0,4,4,6,0,2], wlan
    [0,0,4,8,1,1,2]; 15 of 16 columns converge (not column 8), none is excusable. The converged columns are held to
    the bars and to the transmitted bits, column 8 by the unconverged-column rule.
    Measured on an MI355X, the same figures with 2^126 and 2^127: converged columns, mixed largest |difference|
    1.8e-3 (relative 1.3e-4 at most), wlan 5.7e-4 stop on and 7.2e-4 stop off (relative 2.2e-6); after one iteration,
    every column, mixed 1.2e-4 (relative 1.5e-4), wlan 1.9e-4 (3.3e-5). Column 8 reports 6 like the reference."""
    H, _, layers, _ = cw.code(name)
    C = br.edge_code(name)[2]
    llr = br.edge_input(kind, name)
    decs = decoders(engine, graphs, name, br.EDGE_IMAX, br.EDGE_B)
    got1 = decode_all(decoders(engine, graphs, name, 1, br.EDGE_B), llr)
    ref1 = br.edge_reference(kind, name, 1, True)
    for early in (True, False):
        ref = br.edge_reference(kind, name, br.EDGE_IMAX, early)
        conv = ref[4]
        assert conv.sum() == 15
        for path, got in decode_all(decs, llr, early).items():
            judge(got, ref, f"{kind} {name} {path} early={early}", got1[path], ref1)
            assert np.array_equal((got[0] < 0)[:, conv], (C == 1)[:, conv])


@pytest.mark.parametrize("name", ["mixed", "wlan"])
def test_frustrated_huge_entries(engine, graphs, name):
    """The saturating batch with the signs of its 2^126 entries drawn at random: the checks are frustrated, no
    codeword is near, and the float32 form of the reference is only measured within H5 after the first iteration.
    i_max 1, every column within the bars, finite everywhere. Reference iters [0,16], none excusable; measured on
    an MI355X: largest |difference| 1.2e-4 (mixed) and 1.7e-4 (wlan), largest relative 1.5e-4 and 3.3e-5."""
    llr = br.edge_input("frustrated", name)
    ref1 = br.edge_reference("frustrated", name, 1, True)
    for path, got in decode_all(decoders(engine, graphs, name, 1, br.EDGE_B), llr).items():
        assert np.isfinite(got[0]).all() and (got[1] == 1).all()
        compare(got, ref1, f"frustrated {name} {path} i_max 1")


def test_small_llr_max_every_degree(engine, graphs):
    """mixed (check degrees 2..16), awgn_llr(2 dB) negated by the codewords, llr_max = 7.5 through the constructor:
    every message of every degree body sits at its clamp. B = 16, i_max 6, stop on and off, both paths. Reference
    iters [0,0,0,2,2,1,11], columns 3, 9, 11, 13 and 15 converge, excusable [10] (after one iteration: [2]); the
    other columns by the unconverged-column rule. Measured on an MI355X: none excused, converged columns largest
    |difference| 1.5e-5 stop on, 2.1e-5 stop off (relative 2.2e-5); after one iteration 2.6e-6 (relative 2.4e-4)."""
    llr = br.small_llr_max_input()
    C = br.edge_code("mixed")[2]
    L = br.SMALL_LLR_MAX
    decs = decoders(engine, graphs, "mixed", br.EDGE_IMAX, br.EDGE_B, llr_max=L)
    got1 = decode_all(decoders(engine, graphs, "mixed", 1, br.EDGE_B, llr_max=L), llr)
    ref1 = br.edge_reference("small_llr_max", "mixed", 1, True, L)
    for early in (True, False):
        ref = br.edge_reference("small_llr_max", "mixed", br.EDGE_IMAX, early, L)
        conv = ref[4]
        for path, got in decode_all(decs, llr, early).items():
            judge(got, ref, f"llr_max {L} {path} early={early}", got1[path], ref1)
            assert np.array_equal((got[0] < 0)[:, conv], (C == 1)[:, conv])
            assert np.abs(got[0]).max() > L


# ---------------------------------------------------------------------------------------------------------------
# 4. zeros and ties; 5. unlike neighbours
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "wlan"])
def test_zeros_and_ties(engine, graphs, name):
    """tests/_layered_census.py quantised_llr: integers in [-3, 7] with about 5 % -0 and 5 % +0 entries — exact ties
    |a| == |b| and zeros of either sign in the box-plus. B = 16, i_max 6, both paths, THE STOP OFF: with the stop
    on every column (mixed) has values in the near-zero band, is excusable and leaves iters unconstrained, so that
    run would test nothing about the stop. Every value within H5 of the reference, the two paths bit for bit.
    Reference iters [0,0,0,0,0,0,16]; measured on an MI355X: largest |difference| 3.8e-6 (mixed), 4.4e-6 (wlan)."""
    llr = br.quantised_input(name)
    ref = br.edge_reference("quantised", name, br.EDGE_IMAX, False)
    for path, got in decode_all(decoders(engine, graphs, name, br.EDGE_IMAX, br.EDGE_B), llr, early=False).items():
        assert np.isfinite(got[0]).all() and (got[1] == br.EDGE_IMAX).all()
        bad = br.h5_violations(got[0], ref[0])
        print(f"quantised {name} {path}: H5 violations {int(bad.sum())}, max |diff| "
              f"{float(np.abs(got[0] - ref[0]).max()):.3g}")
        assert not bad.any()


@pytest.mark.parametrize("name", ["mixed", "wlan"])
def test_unlike_neighbours(engine, graphs, name):
    """tests/_layered_census.py mixed_batch_llr with its saturating columns (+-FLT_MAX: outside this decoder's
    precondition) replaced by columns of br.saturating_input; cw_per_group + 3 columns, so the waves of one
    workgroup do unlike things and stop at unlike times; i_max 6, stop on, both paths. The all-zero and the
    all-negative-zero column stop after one iteration with +0 in every entry: P = llr + 0 is +0, Q = +0 - (+-0) is
    +0, a clamp of +0 or a box-plus of zeros is +-0, and +0 + (+-0) is +0. The subnormal columns are held to finite
    values and H5 only, and H5's absolute term (1e-4) makes that vacuous for values around 2^-130: they are here as
    neighbours. Every other column by the bars, the unconverged ones (quantised, constant with random signs) by the
    unconverged-column rule. B = 11; reference iters by column, mixed [6,4,6,1,1,1,6,4,6,2,6], wlan
    [6,3,6,1,1,1,6,3,6,2,6]; excusable [0,2,3,4,8,10] (quantised, subnormal, zeros). Measured on an MI355X: no column
    excused, converged columns largest |difference| 1.8e-4 (mixed) and 4.9e-4 (wlan) on values of 1e2..1e38 (relative
    8.5e-7); after one iteration 1.2e-4 and 1.8e-4."""
    col = {k: i for i, k in enumerate(br.NEIGHBOUR_COLUMNS)}
    decs = decoders(engine, graphs, name, br.EDGE_IMAX, br.EDGE_B)
    B = decs["fused"].geometry(1)[0] + 3
    assert len(br.NEIGHBOUR_COLUMNS) <= B <= br.EDGE_B and decs["fused"].geometry(B)[1] == 2
    llr = br.neighbours_input(name, B)
    ref = br.edge_reference("neighbours", name, br.EDGE_IMAX, True, 150.0, B)
    ref1 = br.edge_reference("neighbours", name, 1, True, 150.0, B)
    got1 = decode_all(decoders(engine, graphs, name, 1, br.EDGE_B), llr)
    free = list(range(col["subnormal"], B, len(col)))
    assert len(set(ref[1].tolist())) >= 3
    for path, got in decode_all(decs, llr).items():
        out, it = got
        # the i_max = 1 decode: the subnormal columns are in the band and free in iters there too (all report 1)
        judge(got, ref, f"neighbours {name} {path}", got1[path], ref1, free=free)
        for z in (col["zeros"], col["negative_zeros"]):
            assert it[z] == 1 and (out[:, z] == 0).all() and not np.signbit(out[:, z]).any()


# ---------------------------------------------------------------------------------------------------------------
# 6. caller patterns on one Z = 27 handle of max_batch 129 per path
# ---------------------------------------------------------------------------------------------------------------
SENTINEL = -77


@pytest.fixture(scope="module", params=PATHS)
def z27(request, engine, graphs):
    """(decoder of max_batch 129 on the WLAN Z = 27 code, the first 16 columns of spread_input("wlan") — nonzero
    codewords, noise, the all-zero word — and their reference: iters [0,5,5,2,1,1,0,0,2], none excusable; measured
    on an MI355X in every pattern: largest |difference| 5.0e-5, largest relative difference 3.3e-5)."""
    H, _, layers, _ = cw.code("wlan")
    dec = engine.LayeredBPDecoder(graphs("wlan"), layers, cw.IMAX_LAYERED, 129, path=request.param)
    assert dec.path_in_use == request.param
    ref = br.spread_reference("wlan")
    return dec, np.ascontiguousarray(br.spread_input("wlan")[0][:, :16]), cut(ref, 16)


def test_in_place_and_no_iters(z27):
    """`iters=None`, and `out` the input tensor itself."""
    dec, llr, ref = z27
    t = torch.from_numpy(llr).to(dec.device)
    out = dec.decode(t.clone(), iters=None)
    blind = out.cpu().numpy()
    it = torch.full((16,), -1, dtype=torch.int32, device=dec.device)
    same = dec.decode(t, out=t, iters=it)
    assert same is t
    compare((t.cpu().numpy(), it.cpu().numpy()), ref, f"in place {dec.path_in_use}")
    assert np.array_equal(blind.view(np.uint32), t.cpu().numpy().view(np.uint32))
    assert len(set(ref[1].tolist())) >= 3


def test_sentinels_behind_iters(z27):
    """Three entries behind iters[B] keep their value; B = 16 and the ragged B = 13."""
    dec, llr, ref = z27
    for B in (16, 13):
        it = torch.full((B + 3,), SENTINEL, dtype=torch.int32, device=dec.device)
        out = dec.decode(torch.from_numpy(np.ascontiguousarray(llr[:, :B])).to(dec.device), iters=it)
        torch.cuda.synchronize(dec.device)
        it = it.cpu().numpy()
        assert (it[B:] == SENTINEL).all(), "iters written beyond B"
        compare((out.cpu().numpy(), it[:B]), cut(ref, B), f"sentinels {dec.path_in_use} B={B}")


def test_side_stream_behind_queued_work(z27):
    """A decode on a side stream behind work queued there: the input buffer holds noise until a copy on that same
    stream replaces it, and nothing runs on the default stream meanwhile. A kernel of the decode ordered on any
    other stream reads the noise (tests/test_gpu_callers.py _decode_on_side_stream)."""
    dec, llr, ref = z27
    dev = dec.device
    noise = torch.from_numpy(np.ascontiguousarray(br.spread_input("wlan")[0][:, 100:116])).to(dev)
    x = noise.clone()
    src = torch.from_numpy(llr).to(dev)
    out = torch.empty_like(x)
    it = torch.full((16,), SENTINEL, dtype=torch.int32, device=dev)
    busy = torch.ones(1 << 26, dtype=torch.float32, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        for _ in range(16):                      # a few milliseconds of memory-bound work ahead of the copy
            busy.mul_(1.0001)
        x.copy_(src)
        dec.decode(x, out=out, iters=it)
    side.synchronize()
    compare((out.cpu().numpy(), it.cpu().numpy()), ref, f"side stream {dec.path_in_use}")


def test_descending_reuse(z27):
    """One handle decodes B = 129, then 5, then 1, unlike inputs (columns of spread_input("wlan") from different
    offsets), each against a fresh reference: rows and R words left behind by the wider decode do not leak."""
    dec, _, _ = z27
    H, _, layers, _ = cw.code("wlan")
    full = br.spread_input("wlan")[0]
    ref = br.spread_reference("wlan")
    for B, first in ((129, 1), (5, 40), (1, 3)):
        cols = np.arange(first, first + B)
        got = gpu_decode(dec, full[:, cols])
        compare(got, cut(ref, cols=cols), f"reuse {dec.path_in_use} B={B}")
    assert len({int(ref[1][40]), int(ref[1][3]), int(ref[1][1])}) >= 2


def test_batch_too_large(z27):
    dec, llr, _ = z27
    t = torch.zeros((llr.shape[0], dec.max_batch + 1), dtype=torch.float32, device=dec.device)
    with pytest.raises(_lib.IBLError) as e:
        dec.decode(t)
    assert f"rc={_lib.IBL_EINVAL}" in str(e.value)
