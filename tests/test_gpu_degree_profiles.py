"""GPU: degree profiles no other test decodes, against the CPU oracles.

Part one, DVB-S2 low rates. The degree profiles of EN 302 307 rates 1/4, 1/3 and 2/5 at about one fifteenth of the
size: check degrees 4, 5 and 6 (and one check of one less), nearly every check folding both tail inputs (fold class
3), variable degrees {1, 2, 3, 12}. The IB decoder per pass with the degree-2 variable fold on and off, and its
small-batch kernels.

Part two, the check-16 / variable-8 pairing. Check-side and variable-side kernels are instantiated separately for
"max degree <= 8" and "<= 16" (row words per lane and chunk sizes differ: 512 against 1024 codewords); a code with
check degrees above 8 and variable degrees up to 8 pairs the wide check kernels with the narrow variable kernels:
ib_cn_fast<16> / ib_vn_fast<8>, the ib_*_small pairs, ib_fused<16, 8>, fl_cn / fl_vn, fl_*_small, fl_fused<.., 16, 8>
and the float fold through the degree-16 check bodies.

Bars (the project's, unchanged): IB bit-exact with equal stop iteration; fp32 min-sum bit-exact against the fp32
oracle, fp64 min-sum bit-exact, fp64 BP within 1e-9, fp32 BP within SURVEY H5 with no hard-decision flips outside
the band (tests/test_gpu_float.py _h5, _hard_flips); stop iterations equal."""
import functools

import numpy as np
import pytest
import torch

from informationbottleneckdecodingldpc_amd import codes, graph, tables
from oracle import oracle
from tests._codes import converging_case, exact_degree_code, ib_fold_census, mixed_code
from tests.test_gpu_float import _h5, _hard_flips, _llrs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

LOW_RATE = {   # name: (dvbs2_structured arguments, check degrees, (degree, class) census)
    "r14": (dict(n=6120, k=1800, groups_hi=1, deg_hi=12), {3: 1, 4: 4319}, {(3, 2): 1, (4, 1): 1, (4, 3): 4318}),
    "r13": (dict(n=6480, k=2160, groups_hi=2, deg_hi=12), {4: 1, 5: 4319}, {(4, 2): 1, (5, 1): 1, (5, 3): 4318}),
    "r25": (dict(n=6840, k=2520, groups_hi=3, deg_hi=12), {5: 1, 6: 4319}, {(5, 2): 1, (6, 1): 1, (6, 3): 4318}),
}
# x148m: check degrees exactly {3, 9, 12, 14}, so a matching decoder needs 11 raw + 4 composed = 15 check tables
# (16 LDS slots) and stays on the fast path; variable degrees {1, 2, 3, 5, 8}; 203 x 600, E = 2030
X148M = ({3: 42, 9: 50, 12: 50, 14: 61}, {1: 20, 2: 180, 3: 250, 5: 100, 8: 50})


@functools.lru_cache(maxsize=None)
def _H(name):
    if name in LOW_RATE:
        return codes.dvbs2_structured(seed=3, **LOW_RATE[name][0])
    if name == "x168":      # every check body up to 16 and every variable body up to 8: 310 x 600, E = 2761
        return mixed_code(np.arange(2, 17), np.arange(1, 9), 600, seed=31)
    if name == "x148m":
        return exact_degree_code(*X148M, seed=33)
    if name == "x148m_drawn":   # mixed_code moves check degrees off the set: 9 check degrees, see the test below
        return mixed_code(np.array([3, 9, 12, 14]), np.array([1, 2, 3, 5, 8]), 600, seed=33)
    if name == "hi8":       # check degrees {10: 1, 11: 2879}, variable degrees {1, 2, 3, 8}, E = 31,679
        return codes.dvbs2_structured(seed=3, n=7920, k=5040, groups_hi=6, deg_hi=8, deg_lo=3)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _g(name):
    return graph.build_graph(_H(name))


def _degrees(x):
    return {int(d): int(k) for d, k in zip(*np.unique(np.asarray(x), return_counts=True))}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _ib_case(name, B, imax, match, early):
    """Random T = 16 tables and channel and the oracle's decode (computed once, read-only afterwards)."""
    g = _g(name)
    tb = tables.random_tables(16, 16, g.d_c_max, g.d_v_max, imax, seed=imax * 7 + B)
    ch = np.random.default_rng(B).integers(0, 16, (g.n_v, B)).astype(np.int32)
    ref, ref_it = oracle.ib_decode(g, tb, ch, match=match, early_stop=early, return_iters=True)
    _frozen(ch, ref)
    return tb, ch, ref, int(ref_it)


@pytest.fixture(scope="module")
def eng():
    from informationbottleneckdecodingldpc_amd import engine
    return engine


@pytest.fixture(scope="module")
def graphs(eng):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = eng.Graph(_g(name), DEV)
        return cache[name]
    return get


def _ib_decode(dec, ch, early, ch_dtype=torch.int32, out_dtype=torch.int32):
    it = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = dec.decode(torch.tensor(ch, dtype=ch_dtype, device=DEV), out_dtype=out_dtype, early_stop=early, iters=it)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int32), int(it.item())


# ---------------------------------------------------------------------------------- part one: DVB-S2 low rates
@pytest.mark.parametrize("name", list(LOW_RATE))
def test_low_rate_profiles(name):
    """The premises: degree profile and fold census of each construction."""
    g = _g(name)
    assert _degrees(g.cn_deg) == LOW_RATE[name][1]
    assert set(_degrees(g.vn_deg)) == {1, 2, 3, 12}
    assert ib_fold_census(_H(name)) == (LOW_RATE[name][2], 4319)


@pytest.mark.parametrize("match,early", [(True, True), (False, False)], ids=["match-early", "nomatch-fixed"])
@pytest.mark.parametrize("name", list(LOW_RATE))
def test_low_rate_ib_fold_and_small(eng, graphs, name, match, early):
    """Per pass at B = 300 with the fold on and off, then the small-batch kernels on the same handle."""
    B, Bs, imax = 300, 9, 4
    tb, ch, ref, ref_it = _ib_case(name, B, imax, match, early)
    chs = np.ascontiguousarray(ch[:, :Bs])
    refs, refs_it = oracle.ib_decode(_g(name), tb, chs, match=match, early_stop=early, return_iters=True)
    for fold in (True, False):
        dec = eng.IBDecoder(graphs(name), tb, match, max_batch=B, path="passes", fold=fold)
        assert dec.fast_path and not dec.fused and dec.folded == 4319 and dec.fold == fold
        assert Bs <= dec.small_batch < B
        out, it = _ib_decode(dec, ch, early)
        assert it == ref_it, f"fold={fold}"
        np.testing.assert_array_equal(out, ref, err_msg=f"fold={fold}")
        out, it = _ib_decode(dec, chs, early, torch.uint8, torch.uint8)
        assert it == refs_it, f"small, fold={fold}"
        np.testing.assert_array_equal(out, refs, err_msg=f"small, fold={fold}")


@pytest.mark.parametrize("name", list(LOW_RATE))
def test_low_rate_ib_fold_converging(eng, graphs, name):
    """Tables that decode, 9 dB, the degree-1 variable's row set reliable: the batch stops inside the keeping
    passes (the oracle: L = 6, 5 and 7 for r14, r13 and r25)."""
    imax, B = 12, 240
    tb, ch, ref, ref_it = converging_case(_g(name), 9.0, imax, B, True)
    print(f"{name}: stop iteration L = {ref_it}")
    assert 2 <= ref_it < imax - 1
    for fold in (True, False):
        dec = eng.IBDecoder(graphs(name), tb, True, max_batch=B, path="passes", fold=fold)
        assert dec.fast_path and not dec.fused and dec.folded == 4319 and B > dec.small_batch
        out, it = _ib_decode(dec, ch, True)
        assert it == ref_it, f"fold={fold}"
        np.testing.assert_array_equal(out, ref, err_msg=f"fold={fold}")


# -------------------------------------------------------------------- part two: check-16 / variable-8 pairing
def test_pairing_codes():
    """The premises: every code pairs check degrees above 8 with variable degrees up to 8; x168 holds every body."""
    for name in ("x168", "x148m", "hi8"):
        g = _g(name)
        assert g.d_c_max > 8 and g.d_v_max <= 8, name
    g = _g("x168")
    assert set(_degrees(g.cn_deg)) == set(range(2, 17)) and set(_degrees(g.vn_deg)) == set(range(1, 9))
    assert (g.n_c, g.n_v, g.n_e) == (310, 600, 2761)
    g = _g("x148m")
    assert _degrees(g.cn_deg) == X148M[0] and _degrees(g.vn_deg) == X148M[1]
    g = _g("hi8")
    assert _degrees(g.cn_deg) == {10: 1, 11: 2879} and set(_degrees(g.vn_deg)) == {1, 2, 3, 8} and g.n_e == 31679


_DTYPES = [(torch.int32, torch.int32), (torch.uint8, torch.uint8), (torch.uint8, torch.int32),
           (torch.int32, torch.uint8)]
# way: fast = the per-pass kernels (small_batch = 0: check chunks of 512 codewords, variable chunks of 1024, so
# B = 1100 puts the ragged chunk at different positions on the two sides), small = the small-batch kernels,
# fused8 / fused4 = the on-chip kernel with 8 / 4 codewords per workgroup (IBL_FUSED_NCW)
IB_PAIRING = [(c, w, B) for c in ("x168", "x148m")
              for w, B in (("fast", 300), ("fast", 1100), ("small", 9), ("small", 130), ("fused8", 130),
                           ("fused4", 130))] + [("hi8", "fast", 300), ("hi8", "small", 9)]


@pytest.mark.parametrize("early", [False, True], ids=["fixed", "early"])
@pytest.mark.parametrize("case", range(len(IB_PAIRING)), ids=[f"{c}-{w}-B{B}" for c, w, B in IB_PAIRING])
def test_ib_check16_variable8(eng, graphs, monkeypatch, case, early):
    """x168 without matching (13 + 15 composed check tables would exceed the 16 LDS slots), x148m with matching,
    hi8 both ways; u8 and i32 in and out spread over the cases."""
    name, way, B = IB_PAIRING[case]
    match = {"x168": False, "x148m": True, "hi8": early}[name]
    imax = 4
    g = _g(name)
    tb, ch, ref, ref_it = _ib_case(name, B, imax, match, early)
    if way.startswith("fused"):
        monkeypatch.setenv("IBL_FUSED_NCW", way[5:])
    dec = eng.IBDecoder(graphs(name), tb, match, max_batch=B, path="fused" if way.startswith("fused") else "passes")
    assert g.d_c_max > 8 and g.d_v_max <= 8 and dec.fast_path and dec.folded == 0
    assert dec.fused == way.startswith("fused")
    if way == "fast":
        dec.small_batch = 0
    elif way == "small":
        assert B <= dec.small_batch
    elif way == "fused8":
        assert dec.fused_ncw(B) == 8
    else:   # the half-group kernel may be absent under the whole-group launch bounds (then whole groups run)
        print(f"{name}: IBL_FUSED_NCW=4 runs groups of {dec.fused_ncw(B)}")
        assert dec.fused_ncw(B) in (4, 8)
    ch_dtype, out_dtype = _DTYPES[(case + int(early)) % 4]
    out, it = _ib_decode(dec, ch, early, ch_dtype, out_dtype)
    assert it == ref_it
    np.testing.assert_array_equal(out, ref)


@pytest.mark.parametrize("early", [False, True], ids=["fixed", "early"])
def test_ib_drawn_degree_set_runs_generic(eng, graphs, early):
    """mixed_code([3, 9, 12, 14], [1, 2, 3, 5, 8], 600, seed=33) does not keep its check degrees to the set given:
    meeting the edge total and merging double edges leave 9 check degrees, and 11 raw + 9 composed check tables
    exceed the 16 LDS slots, so with matching the decoder takes the generic path (x148m above has the exact set).
    Still bit-exact."""
    g = _g("x148m_drawn")
    ncdeg = len(_degrees(g.cn_deg))
    assert g.d_c_max == 14 and g.d_v_max == 8 and g.d_c_max - 3 + ncdeg > 16
    tb, ch, ref, ref_it = _ib_case("x148m_drawn", 300, 4, True, early)
    dec = eng.IBDecoder(graphs("x148m_drawn"), tb, True, max_batch=300, path="passes")
    assert not dec.fast_path and not dec.fused
    out, it = _ib_decode(dec, ch, early)
    assert it == ref_it
    np.testing.assert_array_equal(out, ref)


@functools.lru_cache(maxsize=None)
def _float_case(name, kind, B, early, imax=6):
    """Channel LLRs (quantised alphabet, 2 dB), the fp64 oracle's decode and, for min-sum, the fp32 oracle's."""
    g = _g(name)
    llr = _llrs(g, B, 2.0, seed=kind + 11 + B, quantised=True)
    ref, ref_it = oracle.float_decode(g, kind, imax, llr, early_stop=early, return_iters=True)
    r32, r32_it = None, None
    if kind == oracle.MINSUM:
        r32, r32_it = oracle.float32_decode(g, imax, llr.astype(np.float32), early_stop=early, return_iters=True)
        r32 = r32.astype(np.float64)
        _frozen(r32)
    _frozen(llr, ref)
    return llr, ref, int(ref_it), r32, r32_it


# path="passes": B = 8 runs the small-batch kernels (threshold 64), 72 and 300 the per-pass kernels; path="auto":
# the fused kernel
FLOAT_PAIRING = [("x168", "passes", 8), ("x168", "passes", 72), ("x168", "passes", 300), ("x168", "auto", 9),
                 ("hi8", "passes", 72)]


@pytest.mark.parametrize("early", [False, True], ids=["fixed", "early"])
@pytest.mark.parametrize("prec", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("kind", [oracle.MINSUM, oracle.BP], ids=["minsum", "bp"])
@pytest.mark.parametrize("name,path,B", FLOAT_PAIRING, ids=[f"{c}-{p}-B{B}" for c, p, B in FLOAT_PAIRING])
def test_float_check16_variable8(eng, graphs, monkeypatch, name, path, B, kind, prec, early):
    """Min-sum and BP, fp32 and fp64, on every path; hi8 folds its 2879 staircase variables through the degree-16
    check instantiation and is also compared with a handle that does not fold (IBL_FL_FOLD=0)."""
    imax = 6
    g = _g(name)
    llr, ref, ref_it, r32, r32_it = _float_case(name, kind, B, early)

    def run(dec):
        it = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = dec.decode(torch.tensor(llr, dtype=prec, device=DEV), early_stop=early, iters=it)
        torch.cuda.synchronize()
        return out.double().cpu().numpy(), int(it.item())

    dec = eng.FloatDecoder(graphs(name), kind, imax, B, precision=prec, path=path)
    assert g.d_c_max > 8 and g.d_v_max <= 8
    assert dec.fused == (path == "auto")
    if path == "passes":
        assert dec.small_batch == 64
    if name == "hi8":
        assert dec.folded == 2879
    out, it = run(dec)
    if prec == torch.float64:
        assert it == ref_it
        if kind == oracle.MINSUM:
            np.testing.assert_array_equal(out, ref)
        else:
            np.testing.assert_allclose(out, ref, rtol=0, atol=1e-9)
    elif kind == oracle.MINSUM:
        assert it == r32_it
        np.testing.assert_array_equal(out, r32)
    else:
        assert it == ref_it
        bad = _h5(out, ref)
        assert bad.sum() == 0, f"{bad.sum()} of {bad.size} LLRs outside H5, max |x-y| {np.abs(out - ref).max():.3e}"
        assert _hard_flips(out, ref) == 0
    if name == "hi8":
        monkeypatch.setenv("IBL_FL_FOLD", "0")
        plain = eng.FloatDecoder(graphs(name), kind, imax, B, precision=prec, path=path)
        assert plain.folded == 0
        pout, pit = run(plain)
        assert pit == it
        np.testing.assert_array_equal(pout, out)
