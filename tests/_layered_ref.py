"""numpy float32 restatement of the layered normalised / offset min-sum decoder (include/ibldpc.h "Layered
min-sum"): every operation is one numpy float32 operation (numpy rounds each and never fuses), vectorised over
the batch and over the checks of one degree of a layer (a layer's checks share no variable, so their order is
irrelevant)."""
import numpy as np
import scipy.sparse as sp


def layered_decode(H, layers, llr, imax, alpha=1.0, beta=0.0, llr_max=150.0, early_stop=True, hook=None,
                   stop_rule=None):
    """-> (out [N][B] float32, iters [B] int32). `hook` (tests/_layered_census.py) observes every update of the
    checks of one degree of a layer and changes nothing: hook(it, checks [n], D = P - R before the clamp, Q, pos,
    m1, m2, mag, R_new (all [n][d][B] or [n][B]), done [B]). `stop_rule(A, P) -> bool [B]` replaces the
    specification's stop test ("every check's decisions have even parity") by a wrong one, on purpose
    (tests/test_cpu_codewords.py: what an all-zero input cannot tell apart)."""
    A = sp.csr_matrix(H)
    A.sort_indices()
    indptr, cols = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    deg = np.diff(indptr)
    f32 = np.float32
    alpha, beta, L = f32(alpha), f32(beta), f32(llr_max)
    P = np.array(llr, dtype=f32, copy=True)
    n, B = P.shape
    R = np.zeros((indptr[-1], B), dtype=f32)
    # per layer and degree: edge ids [checks][d] (ascending column order) and their variables
    groups = []
    for layer in layers:
        layer = np.asarray(layer, dtype=np.int64)
        for d in np.unique(deg[layer]):
            cs = layer[deg[layer] == d]
            e = indptr[cs][:, None] + np.arange(d)[None, :]
            groups.append((cs, e, cols[e]))
    out = np.empty_like(P)
    iters = np.full(B, imax, dtype=np.int32)
    done = np.zeros(B, dtype=bool)
    for it in range(1, imax + 1):
        for cs, e, v in groups:
            D = P[v] - R[e]
            Q = np.clip(D, -L, L)                                 # [checks][d][B]
            neg = Q < 0
            a = np.abs(Q)
            pos = np.argmin(a, axis=1)                            # first position attaining the minimum
            m1 = np.take_along_axis(a, pos[:, None, :], axis=1)[:, 0, :]
            a2 = a.copy()
            np.put_along_axis(a2, pos[:, None, :], f32(np.inf), axis=1)
            m2 = a2.min(axis=1)
            s = np.logical_xor.reduce(neg, axis=1)
            is_pos = np.arange(a.shape[1])[None, :, None] == pos[:, None, :]
            mag = np.where(is_pos, m2[:, None, :], m1[:, None, :])
            mag = np.maximum(alpha * mag - beta, f32(0))          # product rounded, then the difference
            Rn = np.where(s[:, None, :] ^ neg, -mag, mag).astype(f32)
            R[e] = Rn
            P[v] = Q + Rn
            if hook is not None:
                hook(it, cs, D, Q, pos, m1, m2, mag, Rn, done)
        if early_stop:
            if stop_rule is None:
                x = (P < 0).astype(np.int32)
                ok = ((A @ x) % 2 == 0).all(axis=0) & ~done
            else:
                ok = np.asarray(stop_rule(A, P), dtype=bool) & ~done
            out[:, ok] = P[:, ok]
            iters[ok] = it
            done |= ok
            if done.all():
                break
    out[:, ~done] = P[:, ~done]
    return out, iters
