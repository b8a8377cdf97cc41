"""What pins the layered min-sum reference (tests/_layered_ref.py) and the inputs of its GPU tests:

  layered_decode_scalar  an independent restatement of include/ibldpc.h "Layered min-sum": plain loops over
                         codeword, layer, check and edge, one running "two smallest and first position" scan per
                         check, every operation one explicit numpy scalar operation (float32, or float64 for the
                         exact-arithmetic cross-check). It shares no code with layered_decode.
  layered_census         layered_decode with a counting hook: how often a run meets the arithmetic edges the
                         kernel is written around (ties, zeros, clamps, subnormals, zero corrected magnitudes).
  the input families     quantised / saturating / small llr_max / subnormal / mixed batch, seeded; the CPU tests
                         assert that each reaches its edge (tests/test_cpu_layered.py), the GPU tests decode them
                         (tests/test_gpu_layered.py)."""
import functools

import numpy as np
import scipy.sparse as sp

from tests._codes import mixed_code
from tests._layered_ref import layered_decode

AB = [(1.0, 0.0), (0.75, 0.0), (1.0, 0.5), (0.8125, 0.25)]
F32_MAX = np.finfo(np.float32).max
F32_MIN_NORMAL = np.float32(2.0 ** -126)


# ---------------------------------------------------------------------------------------------------------------
# independent scalar restatement
# ---------------------------------------------------------------------------------------------------------------
def layered_decode_scalar(H, layers, llr, imax, alpha=1.0, beta=0.0, llr_max=150.0, early_stop=True,
                          dtype=np.float32, on_iteration=None, zero_is_negative=False):
    """-> (out [N][B] dtype, iters [B] int32). The parameters are fp32 values in either dtype (the library takes
    floats). `on_iteration(b, it, P)` sees codeword b's APP values (a list of dtype scalars) after iteration it.
    `zero_is_negative` departs from the header on purpose: neg_e = (Q_e <= 0). The values must not change
    (tests/test_cpu_layered.py test_sign_of_a_zero_is_immaterial)."""
    T = dtype
    A = sp.csr_matrix(H)
    A.sort_indices()
    rows = [[int(v) for v in A.indices[A.indptr[c]:A.indptr[c + 1]]] for c in range(A.shape[0])]
    order = [[int(c) for c in layer] for layer in layers]
    al, be, L = T(np.float32(alpha)), T(np.float32(beta)), T(np.float32(llr_max))
    nL, zero, inf = -L, T(0), T(np.inf)
    n, B = np.shape(llr)
    out = np.empty((n, B), dtype=T)
    iters = np.empty(B, dtype=np.int32)
    for b in range(B):
        P = [T(x) for x in llr[:, b]]
        R = [[zero] * len(r) for r in rows]
        it = 0
        while it < imax:
            it += 1
            for layer in order:
                for c in layer:
                    vs, Rc = rows[c], R[c]
                    q, neg = [], []
                    m1, m2, first, s = inf, inf, 0, False
                    for k, v in enumerate(vs):
                        x = P[v] - Rc[k]
                        if x > L:
                            x = L
                        elif x < nL:
                            x = nL
                        ng = bool(x < zero) or (zero_is_negative and bool(x == zero))
                        a = -x if ng else x
                        if a < m1:
                            m1, m2, first = a, m1, k
                        elif a < m2:
                            m2 = a
                        s ^= ng
                        q.append(x)
                        neg.append(ng)
                    c1 = al * m1
                    c1 = c1 - be
                    if not c1 > zero:
                        c1 = zero
                    c2 = al * m2
                    c2 = c2 - be
                    if not c2 > zero:
                        c2 = zero
                    for k, v in enumerate(vs):
                        mag = c2 if k == first else c1
                        r = -mag if s != neg[k] else mag
                        Rc[k] = r
                        P[v] = q[k] + r
            if on_iteration is not None:
                on_iteration(b, it, P)
            if early_stop:
                clean = True
                for vs in rows:
                    par = False
                    for v in vs:
                        par ^= bool(P[v] < zero)
                    if par:
                        clean = False
                        break
                if clean:
                    break
        out[:, b] = P
        iters[b] = it
    return out, iters


# ---------------------------------------------------------------------------------------------------------------
# edge census
# ---------------------------------------------------------------------------------------------------------------
def layered_census(H, layers, llr, imax, alpha, beta, llr_max=150.0, early_stop=True):
    """-> (out, iters, counts): layered_decode's results and, over the check updates of codewords still running
    (not yet stopped when the iteration began):
      check_updates, edges       updates of one check of one codeword, and their edges
      ties                       check updates with m1 == m2
      q_zero                     edges with Q == 0
      clamped                    edges with |P - R| > llr_max
      subnormal_q                edges with 0 < |Q| < 2^-126
      mag_zero                   edges whose corrected magnitude max(alpha m - beta, 0) is 0
      q_zero_mag_zero            edges with Q == 0 whose corrected magnitude is 0 (P = 0 + R with R = +-0)
      q_zero_r_negzero           those of them whose R is -0 (the sign rule negates the zero magnitude)
      pairs                      the set of (degree, first-argmin position) seen
      argmin_moved               {degree: check updates whose argmin position differs from the previous iteration's}"""
    A = sp.csr_matrix(H)
    L = np.float32(llr_max)
    B = np.shape(llr)[1]
    cnt = dict(check_updates=0, edges=0, ties=0, q_zero=0, clamped=0, subnormal_q=0, mag_zero=0, q_zero_mag_zero=0,
               q_zero_r_negzero=0, pairs=set(), argmin_moved={})
    prev = np.full((A.shape[0], B), -1, dtype=np.int64)

    def hook(it, cs, D, Q, pos, m1, m2, mag, Rn, done):
        run = ~done
        d = Q.shape[1]
        n_run = int(run.sum())
        a = np.abs(Q)
        qz = (Q == 0)
        cnt["check_updates"] += Q.shape[0] * n_run
        cnt["edges"] += Q.shape[0] * d * n_run
        cnt["ties"] += int((m1 == m2)[:, run].sum())
        cnt["q_zero"] += int(qz[:, :, run].sum())
        cnt["clamped"] += int((np.abs(D) > L)[:, :, run].sum())
        cnt["subnormal_q"] += int(((a > 0) & (a < F32_MIN_NORMAL))[:, :, run].sum())
        cnt["mag_zero"] += int((mag == 0)[:, :, run].sum())
        cnt["q_zero_mag_zero"] += int((qz & (mag == 0))[:, :, run].sum())
        cnt["q_zero_r_negzero"] += int((qz & (Rn == 0) & np.signbit(Rn))[:, :, run].sum())
        cnt["pairs"].update((d, int(p)) for p in np.unique(pos[:, run]))
        moved = (prev[cs] >= 0) & (prev[cs] != pos)
        cnt["argmin_moved"][d] = cnt["argmin_moved"].get(d, 0) + int(moved[:, run].sum())
        prev[cs] = pos

    out, iters = layered_decode(H, layers, llr, imax, alpha, beta, llr_max, early_stop, hook=hook)
    return out, iters, cnt


# ---------------------------------------------------------------------------------------------------------------
# codes and input families of the GPU tests (float32 [N][B], seeded)
# ---------------------------------------------------------------------------------------------------------------
MIXED_DEGREES = list(range(2, 17))
MIXED_PAIRS = {(d, p) for d in MIXED_DEGREES for p in range(d)}   # 135 (degree, first-argmin position) pairs


@functools.lru_cache(maxsize=None)
def mixed():
    """The irregular code of every check degree 2..16 (test_irregular_non_qc's) and its greedy layers."""
    from informationbottleneckdecodingldpc_amd import codes
    H = mixed_code(np.arange(2, 17), np.array([2, 3, 3, 4, 6]), 400, seed=5)
    return H, codes.greedy_layers(H)


@functools.lru_cache(maxsize=None)
def wlan(Z):
    from informationbottleneckdecodingldpc_amd import codes
    H = codes.wlan_80211n(Z)
    return H, codes.qc_layers(H, Z)


def awgn_llr(n, B, ebn0_dB, seed, R=0.5):
    """LLRs of the all-zero codeword (BPSK +1) over AWGN: sigma^2 = 1 / (2 R 10^(Eb/N0 / 10)), LLR = 2 y / sigma^2."""
    s2 = 1.0 / (2.0 * R * 10 ** (ebn0_dB / 10))
    y = 1.0 + np.sqrt(s2) * np.random.default_rng(seed).standard_normal((n, B))
    return (2.0 * y / s2).astype(np.float32)


def quantised_llr(n, B, seed):
    """Integers in [-3, 7] (a fixed-point front end: ties and exact cancellations everywhere), about 5 % of the
    entries -0.0 and about 5 % +0.0."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 8, (n, B)).astype(np.float32)
    u = rng.random((n, B))
    x[u < 0.05] = -0.0
    x[(u >= 0.05) & (u < 0.10)] = 0.0
    return x


def saturating_llr(n, B, seed):
    """AWGN(3 dB) x 40 (most |P - R| beyond llr_max = 150 after an iteration), a few entries +-FLT_MAX and a few
    exactly +-150 (the clamp's own bounds)."""
    rng = np.random.default_rng(seed)
    x = awgn_llr(n, B, 3.0, seed) * np.float32(40)
    k = max(4, n * B // 100)
    at = rng.choice(n * B, 2 * k, replace=False)
    sign = rng.choice(np.array([-1.0, 1.0], np.float32), 2 * k)
    x.reshape(-1)[at[:k]] = sign[:k] * F32_MAX
    x.reshape(-1)[at[k:]] = sign[k:] * np.float32(150)
    return x


def subnormal_llr(n, B, seed, exponent=-130):
    """AWGN(3 dB) x 2^exponent: at -130 nearly every LLR is subnormal, at -120 the values cross the boundary
    between subnormal and normal numbers during the decode."""
    return awgn_llr(n, B, 3.0, seed) * np.float32(2.0 ** exponent)


BETA_SUBNORMAL = 2.0 ** -140

# name -> (input for a code H and a batch of B, the (alpha, beta, llr_max) it is decoded with).
# small_llr_max: plain AWGN at 2 dB for the code's own rate, decoded with llr_max = 7.5.
FAMILIES = {
    "quantised": (lambda H, B: quantised_llr(H.shape[1], B, seed=21), [(a, b, 150.0) for a, b in AB]),
    "saturating": (lambda H, B: saturating_llr(H.shape[1], B, seed=22),
                   [(1.0, 0.0, 150.0), (0.8125, 0.25, 150.0)]),
    "small_llr_max": (lambda H, B: awgn_llr(H.shape[1], B, 2.0, seed=23, R=1.0 - H.shape[0] / H.shape[1]),
                      [(1.0, 0.0, 7.5), (0.8125, 0.25, 7.5)]),
    "subnormal": (lambda H, B: subnormal_llr(H.shape[1], B, seed=24),
                  [(0.8125, 0.0, 150.0), (0.8125, BETA_SUBNORMAL, 150.0)]),
    "subnormal_boundary": (lambda H, B: subnormal_llr(H.shape[1], B, seed=25, exponent=-120),
                           [(0.8125, 0.0, 150.0), (0.8125, BETA_SUBNORMAL, 150.0)]),
}
FAMILY_B, FAMILY_IMAX = 16, 6

MIXED_BATCH_COLUMNS = ("quantised", "saturating", "subnormal", "zeros", "negative_zeros", "constant",
                       "constant_random_signs", "awgn")


def mixed_batch_llr(n, B, seed):
    """One batch whose neighbouring columns come from different families (column b is family b mod 8 of
    MIXED_BATCH_COLUMNS): the waves of one workgroup do unlike things and stop at unlike times."""
    rng = np.random.default_rng(seed)
    c = np.float32(2.5)
    src = {"quantised": quantised_llr(n, B, seed + 1), "saturating": saturating_llr(n, B, seed + 2),
           "subnormal": subnormal_llr(n, B, seed + 3), "zeros": np.zeros((n, B), np.float32),
           "negative_zeros": np.full((n, B), -0.0, np.float32), "constant": np.full((n, B), c, np.float32),
           "constant_random_signs": c * rng.choice(np.array([-1.0, 1.0], np.float32), (n, B)),
           "awgn": awgn_llr(n, B, 3.0, seed + 4)}
    x = np.empty((n, B), np.float32)
    for b in range(B):
        x[:, b] = src[MIXED_BATCH_COLUMNS[b % len(MIXED_BATCH_COLUMNS)]][:, b]
    return x
