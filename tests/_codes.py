"""Test-only code constructions shared by the GPU parity tests."""
import numpy as np


def mixed_code(cdegs, vdegs, n, seed):
    """Random irregular code whose check / variable degrees cover the given sets (every fast-path
    body, incl. the column-fetched inputs of degrees 5..8, and the MAXD=16 bodies). Socket matching;
    double edges are merged, a draw that leaves a check of degree < 2 is redrawn."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    for _ in range(100):
        vd = np.concatenate([vdegs, rng.choice(vdegs, n - len(vdegs))])
        E = int(vd.sum())
        m = max(int(round(E / np.mean(cdegs))), len(cdegs))   # check total reachable within the degree range
        cd = np.concatenate([cdegs, rng.choice(cdegs, m - len(cdegs))])
        while cd.sum() != E:   # move the check total onto E within [min, max] of cdegs
            i = int(rng.integers(len(cdegs), m))
            step = 1 if cd.sum() < E else -1
            if min(cdegs) <= cd[i] + step <= max(cdegs):
                cd[i] += step
        rows = rng.permutation(np.repeat(np.arange(m), cd))
        cols = np.repeat(np.arange(n), vd)
        H = sp.csr_matrix((np.ones(E, dtype=np.int64), (rows, cols)), shape=(m, n))
        H.data[:] = 1
        c = np.diff(H.indptr)
        v = np.bincount(H.indices, minlength=n)
        if c.min() >= 2 and v.min() >= 1 and c.max() <= 16 and v.max() <= 16:
            return H
    raise RuntimeError("no simple mixed code drawn")


def exact_degree_code(cdeg_counts, vdeg_counts, seed):
    """Random code with exactly the given {degree: nodes} profiles on both sides (equal edge totals): socket
    matching, the sockets of a double edge swapped with random others until none is left. mixed_code moves check
    degrees off the given set to meet the edge total and merges double edges; this keeps the degree sets exact,
    which the number of tables of a matching decoder depends on."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    cd = np.repeat(list(cdeg_counts), list(cdeg_counts.values()))
    vd = np.repeat(list(vdeg_counts), list(vdeg_counts.values()))
    E = int(cd.sum())
    assert E == int(vd.sum()), (E, int(vd.sum()))
    m, n = len(cd), len(vd)
    rows = rng.permutation(np.repeat(np.arange(m), cd))
    cols = np.repeat(np.arange(n), vd)
    for _ in range(1000):
        key = rows.astype(np.int64) * n + cols
        order = np.argsort(key, kind="stable")
        dup = order[1:][key[order][1:] == key[order][:-1]]
        if dup.size == 0:
            H = sp.csr_matrix((np.ones(E, dtype=np.int64), (rows, cols)), shape=(m, n))
            assert np.array_equal(np.diff(H.indptr), cd) and np.array_equal(np.bincount(H.indices, minlength=n), vd)
            return H
        for i, j in zip(dup, rng.integers(0, E, dup.size)):   # one swap at a time: the socket multiset is kept
            rows[i], rows[j] = rows[j], rows[i]
    raise RuntimeError("double edges left")


def converging_case(g, ebn0, imax, B, match, T=16):
    """LLR tables and an all-zero-codeword channel sample at ebn0, the rows of the degree-1 variables set to the
    most reliable cluster (a degree-1 variable forwards its channel value unchanged, so a wrong one keeps its check
    unsatisfied and the batch-global stop never comes), and the oracle's decode with early stop:
    (tables, channel, output, stop iteration)."""
    from informationbottleneckdecodingldpc_amd import tables
    from informationbottleneckdecodingldpc_amd.channel import UniformQuantizer, sigma2_from_ebn0
    from oracle import oracle
    q = UniformQuantizer(sigma2_from_ebn0(ebn0, g.R_c), T)
    tb = tables.llr_tables(q.output_LLRs, g.d_c_max, g.d_v_max, imax)
    ch = q.sample_all_zero(g.n_v, B, np.random.default_rng(B)).astype(np.int32)
    ch[np.flatnonzero(np.asarray(g.vn_deg) == 1)] = T - 1
    ref, ref_it = oracle.ib_decode(g, tb, ch, match=match, early_stop=True, return_iters=True)
    ch.setflags(write=False)
    ref.setflags(write=False)
    return tb, ch, ref, int(ref_it)


def ib_fold_classes(H):
    """Per check (degree, fold class), int array [n_c][2]: the rule of csrc/plan.h plan_ib_fold, restated. A
    degree-2 variable folds iff in both of its checks its edge is one of the last two inputs in ascending column
    order and the check has degree >= 3; class bit 0 = the check's input D-2 is folded, bit 1 = its input D-1.
    (The rule alone: the IB decoder applies it only where its folding kernels exist, check degrees <= 8.)"""
    import scipy.sparse as sp
    A = sp.csr_matrix(H)
    A.sum_duplicates()
    A.sort_indices()
    n_c, n_v = A.shape
    deg = np.diff(A.indptr)
    out = np.zeros((n_c, 2), dtype=np.int64)
    out[:, 0] = deg
    C = sp.csc_matrix(A)
    C.sort_indices()

    def tail_pos(c, v):
        d = int(deg[c])
        k = int(np.searchsorted(A.indices[A.indptr[c]:A.indptr[c + 1]], v))
        return k - (d - 2) if d >= 3 and k >= d - 2 else -1

    for v in np.flatnonzero(np.diff(C.indptr) == 2):
        c1, c2 = (int(c) for c in C.indices[C.indptr[v]:C.indptr[v] + 2])
        a1, a2 = tail_pos(c1, v), tail_pos(c2, v)
        if a1 >= 0 and a2 >= 0:
            out[c1, 1] |= 1 << a1
            out[c2, 1] |= 1 << a2
    return out


def ib_fold_census(H):
    """({(degree, class): checks} over the folding classes 1..3, folded variables) of ib_fold_classes(H)."""
    fc = ib_fold_classes(H)
    pairs, counts = np.unique(fc[fc[:, 1] > 0], axis=0, return_counts=True)
    bits = int(((fc[:, 1] & 1) + (fc[:, 1] >> 1)).sum())   # every folded variable sets one bit in each of its checks
    return {(int(d), int(c)): int(k) for (d, c), k in zip(pairs, counts)}, bits // 2


def fold_census_code(per=8, seed=7, degs=range(3, 9)):
    """A small code with at least `per` checks of every (degree D, fold class) for D in degs and class 1, 2, 3: per
    (D, 1), per (D, 2) and 2 per (D, 3). Columns [information | chain parity | terminators]; for each D, `per`
    chains of four checks of degree D: information degrees D-1, D-2, D-2, D-2, three staircase parity variables
    joining neighbouring checks and one degree-1 terminator on the last check. The first check of a chain then
    folds its last input only (class 2), the middle two both tail inputs (class 3) and the last its input D-2
    (class 1: the terminator, the highest column, is its input D-1). Information sockets go to the columns used
    least so far (random tie-break) of a quarter as many columns as sockets, so every one gets degree 4.
    per = 8, D = 3..8: 180 information columns, 192 x 372, E = 1056, variable degrees {1: 48, 2: 144, 4: 180}."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    degs = list(degs)
    chains = len(degs) * per
    n_info = sum(per * (4 * D - 7) for D in degs) // 4
    n_par, n_c = 3 * chains, 4 * chains
    n = n_info + n_par + chains
    use = np.zeros(n_info, dtype=np.int64)
    rows, cols = [], []
    chain = 0
    for D in degs:
        for _ in range(per):
            for j, d_info in enumerate((D - 1, D - 2, D - 2, D - 2)):
                c = 4 * chain + j
                pick = np.lexsort((rng.random(n_info), use))[:d_info]   # least used first, ties at random
                use[pick] += 1
                par = [n_info + 3 * chain + i for i in (j - 1, j) if 0 <= i < 3]
                term = [n_info + n_par + chain] if j == 3 else []
                for v in list(pick) + par + term:
                    rows.append(c)
                    cols.append(int(v))
            chain += 1
    H = sp.csr_matrix((np.ones(len(rows), dtype=np.int64), (rows, cols)), shape=(n_c, n))
    assert H.data.max() == 1 and use.min() >= 1
    return H
