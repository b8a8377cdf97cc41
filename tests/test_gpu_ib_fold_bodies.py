"""GPU: every folding check body of the IB per-pass fast path against the CPU oracle. With the degree-2 variable fold
on, a check runs one instantiation of the generated body per (check degree 3..8, fold class 1..3, keeping or plain,
gathering pass 0 or not): cn_compute_fold of csrc/ib_kernels.hip, 72 bodies. The fold census code
(tests/_codes.py fold_census_code; its census is asserted by tests/test_cpu_fold_census.py) has 8 checks or more
of every (degree, class); the pass counts and the early stop below reach gather / plain / keep.

Bar: bit-exact cluster ids and equal stop iteration, fold on and fold off, both against oracle.ib_decode."""
import functools

import numpy as np
import pytest
import torch

from informationbottleneckdecodingldpc_amd import graph, tables
from oracle import oracle
from tests._codes import converging_case, fold_census_code, ib_fold_census

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _degs(D):
    return range(3, 9) if D is None else (D,)


@functools.lru_cache(maxsize=None)
def _g(D=None):
    """The census code (D = None), or its chains of check degree D alone."""
    return graph.build_graph(fold_census_code(degs=_degs(D)))


@functools.lru_cache(maxsize=None)
def _folded(D=None):
    census, folded = ib_fold_census(fold_census_code(degs=_degs(D)))
    assert all(census.get((d, c), 0) >= 8 for d in _degs(D) for c in (1, 2, 3))
    return folded


@functools.lru_cache(maxsize=None)
def _random_case(T, B, imax, match, early, D=None):
    """Random tables and channel of alphabet T and the oracle's decode (computed once, read-only afterwards)."""
    g = _g(D)
    tb = tables.random_tables(T, T, g.d_c_max, g.d_v_max, imax, seed=imax * 7 + B + T)
    ch = np.random.default_rng(B + T).integers(0, T, (g.n_v, B)).astype(np.int32)
    ref, ref_it = oracle.ib_decode(g, tb, ch, match=match, early_stop=early, return_iters=True)
    ch.setflags(write=False)
    ref.setflags(write=False)
    return tb, ch, ref, int(ref_it)


@pytest.fixture(scope="module")
def eng():
    from informationbottleneckdecodingldpc_amd import engine
    return engine


@pytest.fixture(scope="module")
def G(eng):
    return eng.Graph(_g(), DEV)


def _check_both_folds(eng, G, tb, ch, match, early, ref, ref_it, folded=144):
    for fold in (True, False):   # fold on (the default), then off: each equals the oracle
        dec = eng.IBDecoder(G, tb, match, max_batch=ch.shape[1], path="passes", fold=fold)
        assert dec.fast_path and not dec.fused and ch.shape[1] > dec.small_batch
        assert dec.folded == folded and dec.fold == fold
        it = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = dec.decode(torch.tensor(ch, device=DEV), out_dtype=torch.int32, early_stop=early, iters=it)
        torch.cuda.synchronize()
        assert int(it.item()) == ref_it, f"fold={fold}"
        np.testing.assert_array_equal(out.cpu().numpy(), ref, err_msg=f"fold={fold}")


# B (above the small-batch threshold of 224): 300 = a ragged first 1024-codeword chunk, 1100 = a full chunk plus a
# ragged one. i_max: 1 = nothing folds, 2 = only the gathering pass 0 folds, 4 = the plain folding passes run; with
# early stop the keeping ones.
@pytest.mark.parametrize("early", [False, True], ids=["fixed", "early"])
@pytest.mark.parametrize("match", [True, False], ids=["match", "nomatch"])
@pytest.mark.parametrize("imax", [1, 2, 4])
@pytest.mark.parametrize("B", [300, 1100])
def test_fold_bodies_vs_oracle(eng, G, B, imax, match, early):
    tb, ch, ref, ref_it = _random_case(16, B, imax, match, early)
    assert _folded() == 144
    _check_both_folds(eng, G, tb, ch, match, early, ref, ref_it)


@pytest.mark.parametrize("early", [False, True], ids=["fixed", "early"])
@pytest.mark.parametrize("match", [True, False], ids=["match", "nomatch"])
@pytest.mark.parametrize("D", range(3, 9))
def test_fold_bodies_one_degree(eng, D, match, early):
    """One check degree at a time: the census code's chains of degree D alone (32 checks: 8, 8 and 16 of class 1, 2
    and 3; 24 folded variables), so a wrong body names its degree, and the largest check degree D moves the table
    slots of the pass images and of the fold."""
    tb, ch, ref, ref_it = _random_case(16, 300, 4, match, early, D)
    assert _g(D).d_c_max == D and _folded(D) == 24
    _check_both_folds(eng, eng.Graph(_g(D), DEV), tb, ch, match, early, ref, ref_it, folded=24)


@pytest.mark.parametrize("match,early", [(True, True), (False, False)], ids=["match-early", "nomatch-fixed"])
def test_fold_bodies_alphabet_8(eng, G, match, early):
    """T = 8: the syndrome bias of the folding bodies depends on T / 2."""
    tb, ch, ref, ref_it = _random_case(8, 300, 4, match, early)
    _check_both_folds(eng, G, tb, ch, match, early, ref, ref_it)


@pytest.mark.parametrize("match", [True, False], ids=["match", "nomatch"])
@pytest.mark.parametrize("ebn0", [6.0, 9.0])
def test_fold_bodies_early_stop_converging(eng, G, ebn0, match):
    """Tables that decode (the premise tests/test_cpu_fold_census.py asserts with the oracle alone): the batch stops
    inside the keeping passes, and the decision reads the variable-inbox rows they kept for the folded edges. 9 dB
    stops at the first keeping pass, 6 dB several passes later."""
    imax, B = 12, 240
    tb, ch, ref, ref_it = converging_case(_g(), ebn0, imax, B, match)
    assert 2 <= ref_it < imax - 1
    _check_both_folds(eng, G, tb, ch, match, True, ref, ref_it)
