"""GPU: the row addressing of the IB per-pass fast kernels against the CPU oracle. Every message row is read and
written through a descriptor of its own (csrc/ib_kernels.hip load_row_at / store_row_at: scalar row base, the lane's
32-bit byte offset as the vector offset), in the check pass (plain, folding and keeping stores, to the variable inbox
and to the next check inbox), in the variable pass (heavy and light items) and in the item fetch of both.

The code (row_code below) has checks of degree 3..8 in chains that give every fold class, and variables of degree
1, 2, 3 and 8. Batches: 225 is the first above the small-batch kernels, 1023 a ragged last word of one chunk, 1025 a
ragged second chunk of one word, 2050 three chunks per heavy node and two per light one. The row pitch follows
max_batch, so a decoder made for more codewords than it decodes has rows longer than the batch.

The decode entry points take contiguous [N][B] tensors only (engine._check_tensor), so a column slice of a wider buffer
cannot be passed; the layouts that can reach the kernels are a row pitch above the batch (max_batch > B) and input /
output tensors whose base and rows are not 4-byte aligned (uint8, odd B, a view at an odd offset of a larger buffer).

Bar: bit-exact cluster ids and equal stop iteration against oracle.ib_decode, for fold, composite and vn_composite
each on and off, which also makes the switched-off decoders equal to the switched-on ones."""
import functools
import itertools

import numpy as np
import pytest
import torch

from informationbottleneckdecodingldpc_amd import graph, tables
from oracle import oracle
from tests._codes import ib_fold_census

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PER = 12       # chains per check degree
N8, N3 = 60, 200   # information variables of degree 8 and 3: 8 * 60 + 3 * 200 = 1080 = PER * 90 sockets


def row_code(seed=5):
    """Columns [information | chain parity | terminators]. For each check degree D in 3..8, PER chains of four checks
    of degree D: information degrees D-1, D-2, D-2, D-2, three staircase parity variables (degree 2) joining
    neighbouring checks and a degree-1 terminator on the last one, so a chain's checks have fold class 2, 3, 3, 1
    (tests/_codes.py fold_census_code, whose information part has degree 4 throughout). Here the information
    sockets go to N8 variables of degree 8 and N3 of degree 3, a check taking the columns with the most sockets left
    (random tie-break), which keeps them distinct within a check. 288 x 548, E = 1584."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    degs = range(3, 9)
    chains = len(degs) * PER
    n_info, n_par = N8 + N3, 3 * chains
    left = np.array([8] * N8 + [3] * N3, dtype=np.int64)
    assert left.sum() == sum(PER * (4 * D - 7) for D in degs)
    rows, cols = [], []
    order = rng.permutation([(D, k) for D in degs for k in range(PER)])   # degrees interleaved over the columns
    for chain, (D, _) in enumerate(order):
        for j, d_info in enumerate((D - 1, D - 2, D - 2, D - 2)):
            c = 4 * chain + j
            pick = np.lexsort((rng.random(n_info), -left))[:d_info]
            assert left[pick].min() > 0
            left[pick] -= 1
            par = [n_info + 3 * chain + i for i in (j - 1, j) if 0 <= i < 3]
            term = [n_info + n_par + chain] if j == 3 else []
            for v in list(pick) + par + term:
                rows.append(c)
                cols.append(int(v))
    assert left.max() == 0
    H = sp.csr_matrix((np.ones(len(rows), dtype=np.int64), (rows, cols)), shape=(4 * chains, n_info + n_par + chains))
    assert H.data.max() == 1
    return H


@functools.lru_cache(maxsize=None)
def _g():
    return graph.build_graph(row_code())


@functools.lru_cache(maxsize=None)
def _case(B, match, early, imax=3, T=16):
    """Random tables and channel and the oracle's decode (computed once, read-only afterwards)."""
    g = _g()
    tb = tables.random_tables(T, T, g.d_c_max, g.d_v_max, imax, seed=imax * 13 + B + T)
    ch = np.random.default_rng(B + T + 1).integers(0, T, (g.n_v, B)).astype(np.int32)
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


def _decoder(eng, G, tb, match, max_batch, fold=True, comp=True, vcomp=True):
    dec = eng.IBDecoder(G, tb, match, max_batch=max_batch, path="passes", fold=fold, composite=comp, vn_composite=vcomp)
    assert dec.fast_path and not dec.fused and dec.fold == fold and dec.folded == 3 * 6 * PER
    if not comp:
        assert dec.composite == 0
    if not vcomp:
        assert dec.vn_composite == 0
    return dec


def _equals(dec, ch_t, out, early, ref, ref_it, what):
    it = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = dec.decode(ch_t, out=out, early_stop=early, iters=it)
    torch.cuda.synchronize()
    assert int(it.item()) == ref_it, what
    np.testing.assert_array_equal(got.cpu().numpy().astype(np.int32), ref, err_msg=what)


def test_code_profile():
    H = row_code()
    g = _g()
    assert H.shape == (288, 548) and g.n_e == 1584
    assert dict(zip(*map(list, np.unique(g.vn_deg, return_counts=True)))) == {1: 72, 2: 216, 3: N3, 8: N8}
    assert dict(zip(*map(list, np.unique(g.cn_deg, return_counts=True)))) == {D: 4 * PER for D in range(3, 9)}
    census, folded = ib_fold_census(H)
    assert folded == 216
    assert census == {(D, c): (2 * PER if c == 3 else PER) for D in range(3, 9) for c in (1, 2, 3)}


@pytest.mark.parametrize("early", [False, True], ids=["fixed", "early"])
@pytest.mark.parametrize("match", [True, False], ids=["match", "nomatch"])
@pytest.mark.parametrize("B", [225, 1023, 1025, 2050])
def test_rows_every_switch(eng, G, B, match, early):
    """fold x composite x vn_composite, each on and off: the folding stores to the next check inbox (keeping ones with
    early stop) and the plain ones, composite and two-lookup bodies before them, rest list and full variable list.
    The check composite runs in the cases without matching, the variable composite (degree 8) in all."""
    tb, ch, ref, ref_it = _case(B, match, early)
    ch_t = torch.tensor(ch, device=DEV)
    seen = set()
    for fold, comp, vcomp in itertools.product((True, False), repeat=3):
        dec = _decoder(eng, G, tb, match, B, fold, comp, vcomp)
        assert B > dec.small_batch
        seen.add((dec.composite != 0, dec.vn_composite != 0))
        _equals(dec, ch_t, None, early, ref, ref_it, f"fold={fold} composite={comp} vn_composite={vcomp}")
    # with matching the six check degrees take 6 raw tables, 6 composed finals and the fold's: two super-regions, so
    # no check composite is planned (csrc/plan.h ib_composite_degree); without matching 6 raw tables and the fold's
    assert (not match, True) in seen, "no decoder of this case ran the composite bodies its tables allow"


@pytest.mark.parametrize("early", [False, True], ids=["fixed", "early"])
@pytest.mark.parametrize("B,max_batch", [(1025, 4096), (225, 1025), (2050, 2051)])
def test_rows_longer_than_the_batch(eng, G, B, max_batch, early):
    """A decoder made for max_batch codewords decodes B of them: the row pitch is max_batch's, the chunks B's."""
    tb, ch, ref, ref_it = _case(B, True, early)
    ch_t = torch.tensor(ch, device=DEV)
    for fold in (True, False):
        _equals(_decoder(eng, G, tb, True, max_batch, fold), ch_t, None, early, ref, ref_it, f"fold={fold}")


@pytest.mark.parametrize("shift", [1, 3])
@pytest.mark.parametrize("B", [1023, 1025])
def test_misaligned_input_and_output(eng, G, B, shift):
    """uint8 channel and output tensors that are views at an odd byte offset of larger buffers, odd B: neither their
    bases nor their rows are 4-byte aligned, and the message rows between them still are."""
    tb, ch, ref, ref_it = _case(B, True, True)
    n = ch.shape[0]
    src = torch.zeros(n * B + 8, dtype=torch.uint8, device=DEV)
    ch_t = src[shift:shift + n * B].view(n, B)
    ch_t.copy_(torch.tensor(ch.astype(np.uint8), device=DEV))
    dst = torch.full((n * B + 8,), 0xEE, dtype=torch.uint8, device=DEV)
    out = dst[shift:shift + n * B].view(n, B)
    for fold in (True, False):
        _equals(_decoder(eng, G, tb, True, B + 7, fold), ch_t, out, True, ref, ref_it, f"fold={fold}")
        torch.cuda.synchronize()
        edge = dst.cpu().numpy()
        assert (edge[:shift] == 0xEE).all() and (edge[shift + n * B:] == 0xEE).all(), "wrote outside the output"
