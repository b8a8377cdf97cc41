"""numpy restatement of the layered BP decoder (include/ibldpc.h "Layered BP"), vectorised over the batch and over
the checks of one degree of a layer like tests/_layered_ref.py, with a `dtype` argument:

  float64  THE REFERENCE: the box-plus as min + log1p(exp(-(|a|+|b|))) - log1p(exp(-||a|-|b||)), clamped to [0, L],
           sign from (a < 0) != (b < 0);
  float32  an emulation of the kernels' arithmetic: every operation one numpy float32 operation, the box-plus on
           exp2 / log2 with the kernels' constants and its one fused multiply-add evaluated exactly and rounded once.

Also here: the tolerance of the GPU comparison, the near-zero band, and the rule that finds the
codewords whose stop iteration the tolerance leaves open ("excusable")."""
import functools
import math

import numpy as np
import scipy.sparse as sp

REL, TOL_ABS = 1e-5, 1e-4          # |x - y| <= REL max(|x|, |y|) + TOL_ABS
BAND_ABS = 10 * TOL_ABS            # near-zero band: 10 x H5's absolute term, as margin
EXCUSE_CAP = 0.02                  # at most 2 % of a batch, rounded up, may be excused


def h5_violations(out, ref):
    """Entries outside H5."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    return np.abs(out - ref) > REL * np.maximum(np.abs(out), np.abs(ref)) + TOL_ABS


def in_band(P):
    """A value H5 leaves free to take either sign, with margin: |P| <= 1e-3 + 1e-5 |P|."""
    a = np.abs(np.asarray(P, np.float64))
    return a <= BAND_ABS + REL * a


def excuse_cap(B):
    return int(math.ceil(EXCUSE_CAP * B))


def boxplus(a, b, L, dtype):
    if dtype == np.float64:
        aa, ab = np.abs(a), np.abs(b)
        mag = np.minimum(aa, ab) + np.log1p(np.exp(-(aa + ab))) - np.log1p(np.exp(-np.abs(aa - ab)))
        mag = np.clip(mag, 0.0, L)
        return np.where((a < 0) != (b < 0), -mag, mag)
    f32 = np.float32
    k_log2e, k_ln2 = f32(1.4426950408889634), f32(0.6931471805599453)
    aa, ab = np.abs(a), np.abs(b)
    mn = np.minimum(aa, ab)
    with np.errstate(under="ignore"):
        u = np.exp2(-(aa + ab) * k_log2e)
        v = np.exp2(-np.abs(aa - ab) * k_log2e)
    dif = np.log2(f32(1) + u) - np.log2(f32(1) + v)
    # fmaf(ln2, dif, mn): the product of two float32 is exact in float64, the sum is rounded there and once more
    mag = (np.float64(k_ln2) * dif.astype(np.float64) + mn.astype(np.float64)).astype(f32)
    mag = np.clip(mag, f32(0), f32(L))
    return np.where((a < 0) != (b < 0), -mag, mag).astype(f32)


def check_update(Q, L, dtype):
    """Q [checks][d][B] -> R' [checks][d][B] by the specification's forward-backward order."""
    d = Q.shape[1]
    Rn = np.empty_like(Q)
    if d == 2:
        Rn[:, 0] = np.clip(Q[:, 1], -L, L)
        Rn[:, 1] = np.clip(Q[:, 0], -L, L)
        return Rn
    S = [None] * d
    S[d - 1] = Q[:, d - 1]
    for j in range(d - 2, 0, -1):
        S[j] = boxplus(Q[:, j], S[j + 1], L, dtype)
    Rn[:, 0] = S[1]
    F = Q[:, 0]
    for w in range(1, d - 1):
        Rn[:, w] = boxplus(F, S[w + 1], L, dtype)
        F = boxplus(Q[:, w], F, L, dtype)
    Rn[:, d - 1] = F
    return Rn


def layered_bp_decode(H, layers, llr, imax, llr_max=150.0, early_stop=True, dtype=np.float64, hook=None,
                      clamp_q=False):
    """-> (out [N][B] dtype, iters [B] int32). `hook(it, P)` sees P [N][B] at the end of every iteration (the
    columns of finished codewords go on changing there; `out` holds their frozen values) and changes nothing.
    `clamp_q` departs from the specification on purpose: Q = clamp(P - R), the layered min-sum rule
    (tests/test_cpu_layered_bp.py shows what it breaks)."""
    T = np.dtype(dtype).type
    A = sp.csr_matrix(H)
    A.sort_indices()
    indptr, cols = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    deg = np.diff(indptr)
    L = T(np.float32(llr_max))
    P = np.array(llr, dtype=T, copy=True)
    n, B = P.shape
    R = np.zeros((indptr[-1], B), dtype=T)
    groups = []
    for layer in layers:
        layer = np.asarray(layer, dtype=np.int64)
        for d in np.unique(deg[layer]):
            cs = layer[deg[layer] == d]
            e = indptr[cs][:, None] + np.arange(d)[None, :]
            groups.append((e, cols[e]))
    out = np.empty_like(P)
    iters = np.full(B, imax, dtype=np.int32)
    done = np.zeros(B, dtype=bool)
    for it in range(1, imax + 1):
        for e, v in groups:
            Q = P[v] - R[e]
            if clamp_q:
                Q = np.clip(Q, -L, L)
            Rn = check_update(Q, L, T)
            R[e] = Rn
            P[v] = Q + Rn
        if hook is not None:
            hook(it, P)
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


def syndrome_clean(H, P):
    """bool [B]: the hard decisions of column b satisfy every check."""
    A = sp.csr_matrix(H)
    return ((A @ (np.asarray(P) < 0).astype(np.int32)) % 2 == 0).all(axis=0)


# ---- the named inputs of tests/test_cpu_layered_bp.py and tests/test_gpu_layered_bp.py, and their references,
# computed once per process and never modified ----
@functools.lru_cache(maxsize=None)
def small_dvbs2():
    from informationbottleneckdecodingldpc_amd import codes
    H = codes.dvbs2_structured(seed=5, n=5400, k=1800, groups_hi=2, deg_hi=7, deg_lo=2)
    return H, codes.dvbs2_layers(H)


@functools.lru_cache(maxsize=None)
def dvb_input():
    from tests._layered_census import awgn_llr
    H, layers = small_dvbs2()
    return H, layers, awgn_llr(5400, 130, 1.0, seed=7)


@functools.lru_cache(maxsize=None)
def wlan_input(Z):
    from tests._layered_census import awgn_llr, wlan
    H, layers = wlan(Z)
    return H, layers, awgn_llr(H.shape[1], 32, 1.5, seed=7)


@functools.lru_cache(maxsize=None)
def dvb_reference(imax, early):
    H, layers, llr = dvb_input()
    return reference_with_excusable(H, layers, llr, imax, early_stop=early)


@functools.lru_cache(maxsize=None)
def wlan_reference(Z, imax, early, llr_max=150.0):
    H, layers, llr = wlan_input(Z)
    return reference_with_excusable(H, layers, llr, imax, llr_max=llr_max, early_stop=early)


def reference_with_excusable(H, layers, llr, imax, llr_max=150.0, early_stop=True):
    """The float64 reference and the codewords whose stop iteration H5 leaves open -> (out, iters, excusable
    bool [B]). A codeword is excusable when
      - at its reference stop iteration (imax for one that never stops) a variable lies in the near-zero band: a
        decoder within H5 may see another sign there and not stop, or
      - at an earlier iteration end the reference has no unsatisfied check free of in-band variables: every check
        that kept it running could be satisfied by a value within H5, so such a decoder may stop there.
    Without the early stop nothing is excusable (iters is imax everywhere)."""
    A = sp.csr_matrix(H)
    A.sort_indices()
    band_at, early_at = [], []

    def hook(it, P):
        band = in_band(P)
        x = (P < 0).astype(np.int32)
        unsat = (A @ x) % 2 == 1                                  # [n_c][B]
        has_band = (A @ band.astype(np.int32)) > 0
        band_at.append(band.any(axis=0))
        early_at.append(~(unsat & ~has_band).any(axis=0))         # no unsatisfied check free of in-band variables

    out, iters = layered_bp_decode(H, layers, llr, imax, llr_max, early_stop, np.float64, hook=hook)
    B = np.shape(llr)[1]
    exc = np.zeros(B, dtype=bool)
    if early_stop:
        for b in range(B):
            last = min(int(iters[b]), len(band_at))
            exc[b] = bool(band_at[last - 1][b]) or any(bool(early_at[i][b]) for i in range(last - 1))
    return out, iters, exc
