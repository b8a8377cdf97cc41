"""GPU: the composite final step of the IB per-pass check chains against the CPU oracle. For one check degree D* >= 5
the last two table steps of outputs 0 .. D*-3 are one 4-byte read of a host-composed table and a nibble select
(csrc/plan.h ib_composite_image, the bodies cn_group_fold_cp of csrc/ib_kernels.hip), in the gathering pass 0, the
plain last pass, the folding passes and the keeping ones; every other degree runs the two-lookup bodies in the same
launches.

Bar: bit-exact cluster ids and equal stop iteration, composite on and composite off, both against oracle.ib_decode."""
import functools

import numpy as np
import pytest
import torch

from informationbottleneckdecodingldpc_amd import graph, tables
from oracle import oracle
from tests._codes import converging_case, fold_census_code

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _degs(D):
    return range(3, 9) if D is None else (D,)


@functools.lru_cache(maxsize=None)
def _g(D=None):
    """The fold census code (D = None: check degrees 3..8, 32 checks each), or its chains of check degree D alone
    (32 checks: 8, 8 and 16 of fold class 1, 2 and 3)."""
    return graph.build_graph(fold_census_code(degs=_degs(D)))


@functools.lru_cache(maxsize=None)
def _random_case(T, B, imax, match, early, D=None):
    """Random tables and channel of alphabet T and the oracle's decode (computed once, read-only afterwards)."""
    g = _g(D)
    tb = tables.random_tables(T, T, g.d_c_max, g.d_v_max, imax, seed=imax * 11 + B + T + (D or 0))
    ch = np.random.default_rng(B + T + (D or 0)).integers(0, T, (g.n_v, B)).astype(np.int32)
    ref, ref_it = oracle.ib_decode(g, tb, ch, match=match, early_stop=early, return_iters=True)
    ch.setflags(write=False)
    ref.setflags(write=False)
    return tb, ch, ref, int(ref_it)


@pytest.fixture(scope="module")
def eng():
    from informationbottleneckdecodingldpc_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _G(D=None):
    from informationbottleneckdecodingldpc_amd import engine
    return engine.Graph(_g(D), DEV)


def _decode_equals(dec, ch, early, ref, ref_it, what):
    it = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = dec.decode(torch.tensor(ch, device=DEV), out_dtype=torch.int32, early_stop=early, iters=it)
    torch.cuda.synchronize()
    assert int(it.item()) == ref_it, what
    np.testing.assert_array_equal(out.cpu().numpy(), ref, err_msg=what)


def _check_on_and_off(eng, G, tb, ch, match, early, ref, ref_it, degree, fold=True):
    """Composite on (the default), then off: the per-pass kernels above the small-batch threshold, each equal to the
    oracle. degree: the composite's check degree this code and matching setting must plan (0: none)."""
    for comp in (True, False):
        dec = eng.IBDecoder(G, tb, match, max_batch=ch.shape[1], path="passes", fold=fold, composite=comp)
        assert dec.fast_path and not dec.fused and ch.shape[1] > dec.small_batch and dec.fold == fold
        assert dec.composite == (degree if comp else 0)
        _decode_equals(dec, ch, early, ref, ref_it, f"composite={comp}")


# B (above the small-batch threshold of 224): 300 = a ragged first 1024-codeword chunk, 1100 = a full chunk plus a
# ragged one. i_max: 1 = the gathering pass 0 alone, unfolded; 2 = a folding gathering pass 0 and the plain last pass;
# 4 = the folding passes between them, with early stop the keeping ones.
@pytest.mark.parametrize("early", [False, True], ids=["fixed", "early"])
@pytest.mark.parametrize("match", [True, False], ids=["match", "nomatch"])
@pytest.mark.parametrize("imax", [1, 2, 4])
@pytest.mark.parametrize("B", [300, 1100])
@pytest.mark.parametrize("D", [5, 6, 7, 8])
def test_composite_one_degree(eng, D, B, imax, match, early):
    """One check degree at a time, all three fold classes: a wrong composite body names its degree. With matching
    the pass image holds D - 3 + 1 + 1 <= 7 tables, without it D - 2 + 1 <= 7: one super-region either way."""
    tb, ch, ref, ref_it = _random_case(16, B, imax, match, early, D)
    assert _g(D).d_c_max == D
    _check_on_and_off(eng, _G(D), tb, ch, match, early, ref, ref_it, degree=D)


@pytest.mark.parametrize("match", [True, False], ids=["match", "nomatch"])
@pytest.mark.parametrize("D", [3, 4])
def test_no_composite_below_degree_5(eng, D, match):
    tb, ch, ref, ref_it = _random_case(16, 300, 4, match, True, D)
    _check_on_and_off(eng, _G(D), tb, ch, match, True, ref, ref_it, degree=0)


@pytest.mark.parametrize("early", [False, True], ids=["fixed", "early"])
@pytest.mark.parametrize("B", [300, 1100])
def test_composite_census_code_without_matching(eng, B, early):
    """Degrees 3..8 with 32 checks each and 6 + 1 = 7 tables: the tie goes to degree 8, and degrees 3..7 run the
    two-lookup bodies in the same launches."""
    tb, ch, ref, ref_it = _random_case(16, B, 4, False, early)
    _check_on_and_off(eng, _G(), tb, ch, False, early, ref, ref_it, degree=8)


def test_census_code_with_matching_has_no_room(eng):
    """5 + 6 + 1 = 12 tables are three quads, two super-regions: the composite's 64 KiB do not fit behind them."""
    tb, ch, ref, ref_it = _random_case(16, 300, 4, True, True)
    _check_on_and_off(eng, _G(), tb, ch, True, True, ref, ref_it, degree=0)


@pytest.mark.parametrize("match,early,D", [(True, True, 7), (False, False, 8), (False, True, None)],
                         ids=["match-early-7", "nomatch-fixed-8", "nomatch-early-census"])
def test_composite_without_fold(eng, match, early, D):
    """fold=False: every pass runs the plain bodies (fold class 0), the composite's among them."""
    tb, ch, ref, ref_it = _random_case(16, 300, 4, match, early, D)
    _check_on_and_off(eng, _G(D), tb, ch, match, early, ref, ref_it, degree=D or 8, fold=False)


def test_composite_alphabet_8(eng):
    """T = 8: the composite's entries and nibbles past the alphabet are padding the chains never reach."""
    tb, ch, ref, ref_it = _random_case(8, 300, 4, True, True, 7)
    _check_on_and_off(eng, _G(7), tb, ch, True, True, ref, ref_it, degree=7)


def test_composite_early_stop_converging(eng):
    """Tables that decode: the batch stops inside the keeping passes, whose plain bodies take the composite step."""
    imax, B = 12, 240
    tb, ch, ref, ref_it = converging_case(_g(), 6.0, imax, B, False)
    assert 2 <= ref_it < imax - 1
    _check_on_and_off(eng, _G(), tb, ch, False, True, ref, ref_it, degree=8)


def test_set_composite_off_and_on_again(eng):
    """One handle: on, off, on. Each decode equals the oracle, and the property follows the switch."""
    tb, ch, ref, ref_it = _random_case(16, 300, 4, True, True, 7)
    dec = eng.IBDecoder(_G(7), tb, True, max_batch=300, path="passes")
    for on in (True, False, True):
        dec.composite = on
        assert dec.composite == (7 if on else 0)
        _decode_equals(dec, ch, True, ref, ref_it, f"composite={on}")
