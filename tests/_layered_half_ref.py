"""numpy emulation of the layered BP decoder with half-precision state (include/ibldpc.h "Layered BP, half-precision
state"): P and R are numpy float16 arrays, every operation is one numpy float32 operation, the check update is
tests/_layered_bp_ref.py check_update in its float32 form (with `ulp`, transcendentals moved by up to 1 ulp), and h is
a clamp to +-65504 followed by numpy's float32 -> float16 conversion, which rounds to nearest even and keeps subnormals.
It shares nothing with the library.

Also here: the named inputs of tests/test_cpu_layered_half.py and tests/test_gpu_layered_half.py, the code whose checks
all have degree 2 (no box-plus: the emulation is exact there and the GPU is held to its bits), and the tolerance of the
GPU's comparison by value, measured as tests/test_cpu_layered_half.py test_tolerance_constants states."""
import functools

import numpy as np
import scipy.sparse as sp

from tests import _layered_bp_ref as br

HALF_MAX = np.float32(65504.0)
IMAX = 8                        # iterations of the named inputs
DRAWS = 8                       # one_ulp draws per input (seeds 0..7)

# ---- the tolerance of the GPU comparison: |x - y| <= REL16 max(|x|, |y|) + ABS16 -------------------------------
# Measured (tests/test_cpu_layered_half.py test_tolerance_constants re-measures and holds them): the emulation with
# numpy's transcendentals against DRAWS draws of br.one_ulp (seeds 0..7) on named_input(name) for every name of
# NAMED, i_max 8, over the values after EVERY iteration (which covers the stop on, the stop off and a column frozen
# at any iteration), and on full_size_input() (N = 64800, B = 130, 2 iterations). MEASURED_ABS is the largest
# |x - y|, MEASURED_REL the largest |x - y| / max(|x|, |y|) over the entries with max(|x|, |y|) > 1. Per input:
#   wlan27_2.5dB  1.25 (on values of several hundred)   0.0043      stops [0, 0, 10, 55, 36, 17, 7, 2, 3]
#   wlan27_1.5dB  0.625                                  0.0555      45 of 130 never converge and amplify differences
#   mixed_3dB     1.25                                   0.0291
#   dvb           0.25                                   0.0089
#   full_size     0.0234                                 0.0043
# In no draw did a stop iteration differ on any input; no hard decision of a frozen output flipped on the named inputs
# (28 of 8 x 8.4 million did on full_size, all on values next to zero).
MEASURED = {
    "wlan27_2.5dB": (1.25, 0.00425531914893617),
    "wlan27_1.5dB": (0.625, 0.05545927209705372),
    "mixed_3dB": (1.25, 0.029080675422138838),
    "dvb": (0.25, 0.00889967637540453),
    "full_size": (0.0234375, 0.00429553264604811),
}
MEASURED_ABS = max(v[0] for v in MEASURED.values())
MEASURED_REL = max(v[1] for v in MEASURED.values())
MARGIN = 4                      # a handful of draws under-samples a heavy tail of rounding-boundary flips
ABS16 = MARGIN * MEASURED_ABS
REL16 = MARGIN * MEASURED_REL
BAND16 = 10 * ABS16             # hard decisions are compared outside this band around zero

NAMED = ("wlan27_2.5dB", "wlan27_1.5dB", "mixed_3dB", "dvb")


def h(x):
    """float32 -> float16: clamp to the finite halves, round to nearest even, subnormals kept."""
    return np.clip(np.asarray(x, np.float32), -HALF_MAX, HALF_MAX).astype(np.float16)


def f(y):
    return np.asarray(y, np.float16).astype(np.float32)


def violations(out, want):
    """Entries outside the tolerance."""
    o, w = np.asarray(out, np.float64), np.asarray(want, np.float64)
    return np.abs(o - w) > REL16 * np.maximum(np.abs(o), np.abs(w)) + ABS16


def hard_flips(out, want):
    """Hard decisions (by value) that differ where the emulation's value lies outside the band around zero."""
    o, w = np.asarray(out, np.float64), np.asarray(want, np.float64)
    return int((((o < 0) != (w < 0)) & (np.abs(w) > BAND16)).sum())


def layered_half_decode(H, layers, llr, imax, llr_max=150.0, early_stop=True, ulp=None, record=False):
    """-> (out [N][B] float32, iters [B] int32) or, with `record`, (out, iters, P_at float32 [imax][N][B]): f(P) after
    every iteration, the columns of finished codewords included (they go on changing there; the loop then runs to
    imax whatever stops). `ulp`: br.one_ulp(rng), another legitimate evaluation of the transcendentals."""
    f32 = np.float32
    A = sp.csr_matrix(H)
    A.sort_indices()
    indptr, cols = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    deg = np.diff(indptr)
    L = f32(llr_max)
    P = h(np.asarray(llr, f32) + f32(0))
    n, B = P.shape
    R = np.zeros((indptr[-1], B), dtype=np.float16)
    groups = []
    for layer in layers:
        layer = np.asarray(layer, dtype=np.int64)
        for d in np.unique(deg[layer]):
            cs = layer[deg[layer] == d]
            e = indptr[cs][:, None] + np.arange(d)[None, :]
            groups.append((e, cols[e]))
    out = np.empty((n, B), f32)
    iters = np.full(B, imax, dtype=np.int32)
    done = np.zeros(B, dtype=bool)
    P_at = []
    for it in range(1, imax + 1):
        for e, v in groups:
            Q = f(P[v]) - f(R[e])
            Rh = h(br.check_update(Q, L, f32, ulp=ulp))
            R[e] = Rh
            P[v] = h(Q + f(Rh))
        if record:
            P_at.append(f(P))
        if early_stop:
            x = (f(P) < 0).astype(np.int32)          # by value: a -0 decides 0
            ok = ((A @ x) % 2 == 0).all(axis=0) & ~done
            out[:, ok] = f(P[:, ok])
            iters[ok] = it
            done |= ok
            if done.all() and not record:
                break
    out[:, ~done] = f(P[:, ~done])
    if record:
        return out, iters, np.stack(P_at)
    return out, iters


def want_for(it, ref):
    """The values a decoder's `out` is compared with: ref = (out, iters, P_at) of layered_half_decode(record=True).
    A column whose `it` differs from the emulation's is compared with the emulation's values at the decoder's own
    stop iteration (br.reference_for_columns with every column open to that)."""
    out, r_it, P_at = ref
    return br.reference_for_columns(it, (out, r_it, np.ones(len(r_it), dtype=bool), P_at))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- the named inputs; computed once per process and never modified ----
@functools.lru_cache(maxsize=None)
def named_input(name):
    """-> (H, layers, llr [N][130] float32)."""
    from tests._layered_census import awgn_llr, mixed, wlan
    if name == "dvb":
        return br.dvb_input()
    if name == "mixed_3dB":
        H, layers = mixed()
        db = 3.0
    else:
        H, layers = wlan(27)
        db = float(name.split("_")[1][:-2])
    n = H.shape[1]
    llr = awgn_llr(n, 130, db, seed=7, R=1.0 - H.shape[0] / n)
    llr.setflags(write=False)
    return H, layers, llr


@functools.lru_cache(maxsize=None)
def named_reference(name):
    """(out, iters, P_at) of the emulation with the stop on; the stop-off output is P_at[-1], iters IMAX."""
    H, layers, llr = named_input(name)
    return _frozen(*layered_half_decode(H, layers, llr, IMAX, record=True))


FULL_B, FULL_IMAX = 130, 2


@functools.lru_cache(maxsize=None)
def full_size_input():
    from informationbottleneckdecodingldpc_amd import codes
    from tests._layered_census import awgn_llr
    H = codes.dvbs2_structured(seed=3)
    llr = awgn_llr(64800, FULL_B, 1.0, seed=13)
    llr.setflags(write=False)
    return H, codes.dvbs2_layers(H), llr


def measure(H, layers, llr, imax, draws=DRAWS):
    """-> (abs, rel, iters differ, hard flips): the emulation against `draws` one_ulp draws over the values after every
    iteration; `iters differ` counts stop iterations that differ in some draw, `hard flips` decisions (by value) of the
    frozen outputs that differ."""
    out, it, P_at = layered_half_decode(H, layers, llr, imax, record=True)
    a = r = 0.0
    differ = flips = 0
    for seed in range(draws):
        o, i, Pd = layered_half_decode(H, layers, llr, imax, ulp=br.one_ulp(np.random.default_rng(seed)), record=True)
        d = np.abs(Pd.astype(np.float64) - P_at)
        m = np.maximum(np.abs(Pd), np.abs(P_at)).astype(np.float64)
        a = max(a, float(d.max()))
        big = m > 1.0
        if big.any():
            r = max(r, float((d[big] / m[big]).max()))
        differ += int((i != it).sum())
        flips += int(((o < 0) != (out < 0)).sum())
    return a, r, differ, flips


# ---- the code whose checks all have degree 2 -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def degree2_code(n=400, seed=1):
    """-> (H csr [n_c][n], greedy layers): every check has degree 2, variable v has degree 1 + v % 6. A check of
    degree 2 has no box-plus, so every operation of its update is exact or one correctly rounded fp32 / binary16
    operation: the emulation gives the decoder's bits."""
    from informationbottleneckdecodingldpc_amd import codes
    stubs = np.repeat(np.arange(n), 1 + np.arange(n) % 6)
    assert stubs.size % 2 == 0
    rng = np.random.default_rng(seed)
    for _ in range(1000):
        p = rng.permutation(stubs).reshape(-1, 2)
        p.sort(axis=1)
        if (p[:, 0] != p[:, 1]).all() and np.unique(p, axis=0).shape[0] == p.shape[0]:
            break
    else:
        raise AssertionError("no simple pairing found")
    rows = np.repeat(np.arange(p.shape[0]), 2)
    H = codes.canonical_csr(sp.csr_matrix((np.ones(rows.size, np.int8), (rows, p.reshape(-1))), shape=(p.shape[0], n)))
    assert set(np.diff(H.indptr).tolist()) == {2}
    assert set(np.asarray(H.sum(axis=0)).ravel().tolist()) == set(range(1, 7))
    return H, codes.greedy_layers(H)


@functools.lru_cache(maxsize=None)
def degree2_input(B):
    """Columns by family, b mod 6: AWGN-like values; zeros of either sign; +-1e5 among moderate values (the stage-in
    clamp bites); -2^-26, +-2^-20 and other tiny values (h gives -0 and subnormal halves); small integers (ties);
    and values that are all >= 0 BY VALUE, half of them -2^-26: h makes those -0, every decision by value is 0 and the
    codeword stops after iteration 1 with -0 values left, where a decision read from the sign bit sees a 1."""
    H, _ = degree2_code()
    n = H.shape[1]
    rng = np.random.default_rng(40 + B)
    x = np.empty((n, B), np.float32)
    for b in range(B):
        fam = b % 6
        if fam == 0:
            c = (4.0 + 2.8 * rng.standard_normal(n)).astype(np.float32)
        elif fam == 1:
            c = rng.choice(np.array([0.0, -0.0, 1.5, -2.25], np.float32), n)
        elif fam == 2:
            c = (3.0 * rng.standard_normal(n)).astype(np.float32)
            c[rng.choice(n, n // 8, replace=False)] = np.float32(1e5) * rng.choice(np.array([-1, 1], np.float32), n // 8)
        elif fam == 3:
            c = rng.choice(np.array([-2.0 ** -26, 2.0 ** -20, -2.0 ** -20, 2.0 ** -25, -2.0 ** -24, 3 * 2.0 ** -16,
                                     -2.0 ** -14, 0.0], np.float32), n)
        elif fam == 4:
            c = rng.integers(-3, 8, n).astype(np.float32)
        else:
            c = rng.choice(np.array([-2.0 ** -26, -2.0 ** -26, -2.0 ** -26, 2.0 ** -20, 3 * 2.0 ** -16, 1.5],
                                    np.float32), n)
        x[:, b] = c
    x.setflags(write=False)
    return x
