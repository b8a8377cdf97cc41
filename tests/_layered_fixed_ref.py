"""numpy integer restatement of the fixed-point layered min-sum decoder (include/ibldpc.h "Layered min-sum, fixed
point"), in the shape of tests/_layered_ref.py: vectorised over the batch and over the checks of one degree of a
layer. `fixed_decode_scalar` restates the same text with plain Python integers and loops and shares no code with
it. Both work in integer units: `quantise` is the input rule, `dequantise` the float32 output rule."""
import numpy as np
import scipy.sparse as sp

APP_MAX = 127
DEFAULTS = dict(alpha16=13, beta_q=0, q_max=31)


def quantise(llr, scale=2.0):
    """float32 [N][B] -> int8 integer units: one rounded fp32 product, rint (ties to even), clamped as a float.
    An int8 array is taken as integer units: max(x, -127)."""
    llr = np.asarray(llr)
    if llr.dtype == np.int8:
        return np.maximum(llr, np.int8(-APP_MAX))
    with np.errstate(over="ignore"):
        f = np.rint(llr.astype(np.float32) * np.float32(scale))
    return np.clip(f, np.float32(-APP_MAX), np.float32(APP_MAX)).astype(np.int8)


def dequantise(P, scale=2.0):
    """int8 integer units -> float32 LLR units: one correctly rounded fp32 division."""
    return np.asarray(P).astype(np.float32) / np.float32(scale)


def fixed_decode(H, layers, P0, imax, alpha16=13, beta_q=0, q_max=31, early_stop=True, hook=None):
    """P0: int8 [N][B] integer units (quantise). -> (out int8 [N][B], iters int32 [B]). `hook` observes every update
    of the checks of one degree of a layer and changes nothing: hook(it, checks [n], P_in, T, pos, m1, m2, mag_in
    (before the correction), mag, P_unclamped (T + R_new) (all [n][d][B] or [n][B]), done [B])."""
    A = sp.csr_matrix(H)
    A.sort_indices()
    indptr, cols = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    deg = np.diff(indptr)
    P = np.array(P0, dtype=np.int32, copy=True)
    assert P.min() >= -APP_MAX and P.max() <= APP_MAX
    n, B = P.shape
    R = np.zeros((indptr[-1], B), dtype=np.int32)
    groups = []
    for layer in layers:
        layer = np.asarray(layer, dtype=np.int64)
        for d in np.unique(deg[layer]):
            cs = layer[deg[layer] == d]
            e = indptr[cs][:, None] + np.arange(d)[None, :]
            groups.append((cs, e, cols[e]))
    out = np.empty((n, B), dtype=np.int8)
    iters = np.full(B, imax, dtype=np.int32)
    done = np.zeros(B, dtype=bool)
    for it in range(1, imax + 1):
        for cs, e, v in groups:
            Pin = P[v]
            T = Pin - R[e]                                         # [checks][d][B], not clamped
            neg = T < 0
            a = np.minimum(np.abs(T), q_max)                       # |Q|
            pos = np.argmin(a, axis=1)                             # first position attaining the minimum
            m1 = np.take_along_axis(a, pos[:, None, :], axis=1)[:, 0, :]
            a2 = a.copy()
            np.put_along_axis(a2, pos[:, None, :], 1 << 20, axis=1)
            m2 = a2.min(axis=1)
            s = np.logical_xor.reduce(neg, axis=1)
            is_pos = np.arange(a.shape[1])[None, :, None] == pos[:, None, :]
            mag_in = np.where(is_pos, m2[:, None, :], m1[:, None, :])
            mag = np.maximum(((alpha16 * mag_in + 8) >> 4) - beta_q, 0)
            Rn = np.where(s[:, None, :] ^ neg, -mag, mag)
            R[e] = Rn
            Pu = T + Rn
            P[v] = np.clip(Pu, -APP_MAX, APP_MAX)
            if hook is not None:
                hook(it, cs, Pin, T, pos, m1, m2, mag_in, mag, Pu, done)
        if early_stop:
            x = (P < 0).astype(np.int32)
            ok = ((A @ x) % 2 == 0).all(axis=0) & ~done
            out[:, ok] = P[:, ok]
            iters[ok] = it
            done |= ok
            if done.all():
                break
    out[:, ~done] = P[:, ~done]
    return out, iters


def fixed_decode_scalar(H, layers, P0, imax, alpha16=13, beta_q=0, q_max=31, early_stop=True):
    """The specification with Python integers: loops over codeword, layer, check and edge, one running "two
    smallest and first position" scan per check. -> (out int8 [N][B], iters int32 [B])."""
    A = sp.csr_matrix(H)
    A.sort_indices()
    rows = [[int(v) for v in A.indices[A.indptr[c]:A.indptr[c + 1]]] for c in range(A.shape[0])]
    order = [[int(c) for c in layer] for layer in layers]
    n, B = np.shape(P0)
    out = np.empty((n, B), dtype=np.int8)
    iters = np.empty(B, dtype=np.int32)
    for b in range(B):
        P = [int(x) for x in P0[:, b]]
        R = [[0] * len(r) for r in rows]
        it = 0
        while it < imax:
            it += 1
            for layer in order:
                for c in layer:
                    vs, Rc = rows[c], R[c]
                    t, neg = [], []
                    m1 = m2 = None
                    first, s = 0, False
                    for k, v in enumerate(vs):
                        x = P[v] - Rc[k]
                        q = min(max(x, -q_max), q_max)
                        a = -q if q < 0 else q
                        if m1 is None or a < m1:
                            m1, m2, first = a, m1, k
                        elif m2 is None or a < m2:
                            m2 = a
                        s ^= x < 0
                        t.append(x)
                        neg.append(x < 0)
                    c1 = max(((alpha16 * m1 + 8) >> 4) - beta_q, 0)
                    c2 = max(((alpha16 * m2 + 8) >> 4) - beta_q, 0)
                    for k, v in enumerate(vs):
                        mag = c2 if k == first else c1
                        r = -mag if s != neg[k] else mag
                        Rc[k] = r
                        P[v] = min(max(t[k] + r, -APP_MAX), APP_MAX)
            if early_stop and not any(sum(P[v] < 0 for v in vs) & 1 for vs in rows):
                break
        out[:, b] = P
        iters[b] = it
    return out, iters
