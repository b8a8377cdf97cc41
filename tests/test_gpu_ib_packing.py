"""GPU: the output packing and the first-level lookup addresses of the generated IB node bodies against the oracle.

The unrolled bodies (tools/gen_sched.py --unrolled -> csrc/ib_unrolled.inc) build every output word as one
``(t << 4k) | acc`` chain and take the address of a lookup whose two operands are raw input nibbles from a
word-level row / column byte. The check pass of the per-pass fast kernels of maximum degree 8 runs them as groups of
one codeword parity ({0, 2, 4, 6} then {1, 3, 5, 7}), the fused kernel's light bodies as consecutive groups; the
variable pass, the MAXD = 16 and the small-batch kernels keep the loop bodies of csrc/ib_sched.inc, whose
hand-written neighbours (fold_word, the degree-2 check body) pack through the same chain.
A wrong shift, selector or parity shows as a wrong nibble of some codeword of a word, a
wrong valid mask only in the ragged last word, lane or chunk - hence the batch sizes: 1 and 7 inside one word,
9 a ragged second word, 17 a ragged second lane (16 codewords a lane), 225 the smallest batch the default
threshold hands to the fast kernels, 1023 / 1025 around the 1024-codeword chunk (the light variable rows'
chunks are 2048). Batches up to 17 run twice: on the small-batch kernels, and with those switched off on the
fast kernels.

Codes: the N = 7200 DVB-S2-structured code (check degrees 6, 7, variable degrees 1, 2, 3, 8; 3599 folded
degree-2 variables: the folding bodies, with early stop the keeping FOLD = 2 body and fold_word); a mixed code
with every check degree 2..16 and variable degree 1..16 (the MAXD = 16 kernels, which keep the loop bodies
and have no fold; with matching its tables exceed the LDS and the decoder takes the generic kernels, which is
asserted); and a mixed code with every check degree 2..8 and variable degree 1..8, so that every unrolled
MAXD = 8 body runs, with matching too. Random T = 16
tables never converge, so the oracle runs every iteration with the stop on (asserted: its stop iteration is
i_max - 1); the fixed-iteration decode is then the same computation and shares that reference. Every decode is held
to ``oracle.ib_decode`` under ``np.array_equal`` with equal stop iteration, matching on and off, fold on and off,
early stop on and off, and the kernel path is asserted.
"""
import functools

import numpy as np
import pytest
import torch

from informationbottleneckdecodingldpc_amd import codes, graph, tables
from oracle import oracle
from tests._codes import mixed_code

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SMALL_DEFAULT = 224
# name -> (i_max, fast path with matching). i_max = 4 on the folding code: passes 1 and 2 are plain folding passes
# (keeping ones with the stop on), pass 0 the gathering one
CODES = {"dvbsmall": (4, True), "mixed16": (3, False), "mixed8": (3, True)}
# (B, small-batch kernels allowed)
BATCHES = [(1, True), (7, True), (9, True), (17, True), (1, False), (7, False), (9, False), (17, False),
           (225, True), (1023, True), (1025, True)]


@functools.lru_cache(maxsize=None)
def _g(name):
    H = {"dvbsmall": lambda: codes.dvbs2_structured(seed=3, n=7200, k=3600, groups_hi=4),
         "mixed16": lambda: mixed_code(np.arange(2, 17), np.arange(1, 17), 600, seed=15),
         "mixed8": lambda: mixed_code(np.arange(2, 9), np.arange(1, 9), 600, seed=8)}[name]()
    return graph.build_graph(H)


@functools.lru_cache(maxsize=None)
def _folded(name):
    """Degree-2 variables the check pass folds, by the plan's rule: in both of its checks the
    variable's edge is one of the last two inputs (ascending column) of a check of degree 3..8; the folding
    kernels exist for codes of maximum check degree 8."""
    g = _g(name)
    if g.d_c_max > 8:
        return 0
    n = 0
    for v in np.flatnonzero(g.vn_deg == 2):
        ok = True
        for r in g.csc_rows[g.vn_start[v]:g.vn_start[v] + 2]:
            cols = g.csr_cols[g.cn_start[r]:g.cn_start[r] + g.cn_deg[r]]
            ok = ok and 3 <= g.cn_deg[r] <= 8 and v in cols[-2:]
        n += ok
    return n


@functools.lru_cache(maxsize=None)
def _case(name, B, match):
    """Tables, channel values and the oracle's decode (stop on; it never stops), computed once and read-only."""
    g, imax = _g(name), CODES[name][0]
    tb = tables.random_tables(16, 16, g.d_c_max, g.d_v_max, imax, seed=imax * 5 + B)
    ch = np.random.default_rng(B + 1).integers(0, 16, (g.n_v, B)).astype(np.int32)
    ref, ref_it = oracle.ib_decode(g, tb, ch, match=match, early_stop=True, return_iters=True)
    ch.setflags(write=False)
    ref.setflags(write=False)
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


def test_codes_cover_the_bodies():
    """The degree profiles the cases rely on (no GPU work: fails before a vacuous run)."""
    g = _g("mixed16")
    assert set(np.unique(g.cn_deg)) == set(range(2, 17)) and set(np.unique(g.vn_deg)) == set(range(1, 17))
    d = _g("dvbsmall")
    assert set(np.unique(d.cn_deg)) == {6, 7} and set(np.unique(d.vn_deg)) == {1, 2, 3, 8}
    assert _folded("dvbsmall") == 3599 and _folded("mixed16") == 0
    m = _g("mixed8")
    assert set(np.unique(m.cn_deg)) == set(range(2, 9)) and set(np.unique(m.vn_deg)) == set(range(1, 9))


@pytest.mark.parametrize("match", [True, False], ids=["match", "nomatch"])
@pytest.mark.parametrize("B,small", BATCHES, ids=[f"B{b}-{'default' if s else 'small0'}" for b, s in BATCHES])
@pytest.mark.parametrize("name", list(CODES))
def test_packing_vs_oracle(eng, graphs, name, B, small, match):
    imax, fast_matched = CODES[name]
    want_fast = fast_matched or not match
    folded = _folded(name) if want_fast else 0
    tb, ch, ref, ref_it = _case(name, B, match)
    assert ref_it == imax - 1                        # the oracle never stopped: also the fixed-iteration reference
    for fold in (True, False):
        for early in (True, False):
            dec = eng.IBDecoder(graphs(name), tb, match, max_batch=B, path="passes", fold=fold)
            if not small:
                dec.small_batch = 0
            it = torch.full((1,), -1, dtype=torch.int32, device=DEV)
            out = dec.decode(torch.tensor(ch, device=DEV), out_dtype=torch.int32, early_stop=early, iters=it)
            torch.cuda.synchronize()
            out, it = out.cpu().numpy().astype(np.int32), int(it.item())
            fast = B > dec.small_batch
            bad = int(np.count_nonzero(out != ref))
            label = f"{name} B={B} match={match} fold={fold} early={early}"
            print(f"{label}: oracle it {ref_it}, device it {it}; fast_path={dec.fast_path} fused={dec.fused} "
                  f"small_batch={dec.small_batch} folded={dec.folded} -> "
                  f"{('fast per-pass' if fast else 'small-batch') if dec.fast_path else 'generic'} kernels; mismatches {bad} of {ref.size}")
            # the path: the fast IB path, per-pass launches, the small-batch or the fast kernels as the case names,
            # and the fold planned (it runs on the fast kernels only, when on)
            assert dec.fast_path == want_fast and not dec.fused
            if want_fast:
                assert dec.small_batch == (SMALL_DEFAULT if small else 0)
                assert fast == (B > SMALL_DEFAULT or not small)
            else:                                    # generic kernels: no small-batch kernels, no fold
                assert dec.small_batch == 0
            assert dec.folded == folded and dec.fold == fold
            assert it == ref_it, label
            assert np.array_equal(out, ref), f"{label}: {bad} cluster ids differ from the oracle"
