"""CPU: the premises of tests/test_gpu_ib_fold_bodies.py. The fold census code holds every (check degree 3..8, fold
class 1..3) pair the IB check pass has a folding body for; the Python restatement of the fold rule
(tests/_codes.py ib_fold_classes) equals the C++ plan (csrc/plan.h plan_ib_fold, through the stand-alone program
tests/asan/fold_plan_check.cpp, built and run as tests/test_cpu_fold_plan.py does: nothing loaded into Python is
sanitized); and LLR tables at a stated SNR make the oracle stop inside the loop on that code."""
import numpy as np
import pytest
import scipy.sparse as sp

from informationbottleneckdecodingldpc_amd import graph
from tests._codes import converging_case, fold_census_code, ib_fold_census, ib_fold_classes, mixed_code
from tests.test_cpu_fold_plan import fold_plan_check, run_plan, small_dvb  # noqa: F401  (fixture)

PAIRS = [(D, c) for D in range(3, 9) for c in (1, 2, 3)]


def test_fold_census_code():
    """Every folding body's (degree, class) has at least 8 checks; shape and degrees as documented."""
    H = fold_census_code()
    census, folded = ib_fold_census(H)
    print("fold census (degree, class): checks =", {k: census.get(k, 0) for k in PAIRS}, "folded =", folded)
    for pair in PAIRS:
        assert census.get(pair, 0) >= 8, pair
    assert set(census) == set(PAIRS)
    assert H.shape == (192, 372) and H.nnz == 1056
    vd = np.bincount(H.indices, minlength=H.shape[1])
    assert dict(zip(*np.unique(vd, return_counts=True))) == {1: 48, 2: 144, 4: 180}
    assert folded == 144
    assert [census[(D, c)] for D, c in PAIRS] == [8, 8, 16] * 6
    g = graph.build_graph(H)
    assert g.d_c_max == 8 and g.d_v_max == 4


@pytest.mark.parametrize("D", range(3, 9))
def test_fold_census_code_one_degree(D):
    """The chains of one check degree alone: 8, 8 and 16 checks of class 1, 2 and 3, the largest check degree D."""
    H = fold_census_code(degs=(D,))
    assert ib_fold_census(H) == ({(D, 1): 8, (D, 2): 8, (D, 3): 16}, 24)
    g = graph.build_graph(H)
    assert g.d_c_max == D and g.d_v_max == 4 and g.n_c == 32


@pytest.mark.parametrize("name", ["census", "dvb_small", "mixed"])
def test_fold_classes_equal_the_plan(fold_plan_check, tmp_path, name):  # noqa: F811
    """ib_fold_classes against plan_ib_fold: class counts per check degree and the folded count."""
    H = {"census": fold_census_code, "dvb_small": small_dvb,
         "mixed": lambda: mixed_code(np.arange(2, 9), np.array([1, 2, 2, 2, 3, 4]), 900, seed=21)}[name]()
    out = run_plan(fold_plan_check, H, tmp_path)
    fc = ib_fold_classes(H)
    mine = {}
    for d, c in fc:
        mine.setdefault(str(int(d)), [0, 0, 0, 0])[int(c)] += 1
    assert out["by_degree"] == mine
    assert [sum(v[c] for v in out["by_degree"].values()) for c in range(4)] == out["classes"]
    assert ib_fold_census(H)[1] == out["folded"]
    if name == "mixed":   # the premise of comparing on a random graph at all: it folds something, not everything
        n2 = int((np.bincount(sp.csr_matrix(H).indices, minlength=H.shape[1]) == 2).sum())
        assert 0 < out["folded"] < n2


@pytest.mark.parametrize("match", [True, False])
@pytest.mark.parametrize("ebn0", [6.0, 9.0])
def test_census_code_converges_inside_the_loop(ebn0, match):
    """The converging case of the GPU test: with i_max = 12 and B = 240 the oracle stops at 2 <= L < i_max - 1,
    from pass 1 on (the keeping passes) and before the last pass."""
    imax = 12
    g = graph.build_graph(fold_census_code())
    _, _, ref, L = converging_case(g, ebn0, imax, 240, match)
    print(f"census code, {ebn0} dB, match={match}: stop iteration L = {L}")
    assert 2 <= L < imax - 1
