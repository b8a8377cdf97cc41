"""numpy restatement of the layered BP decoder (include/ibldpc.h "Layered BP"), vectorised over the batch and over
the checks of one degree of a layer like tests/_layered_ref.py, with a `dtype` argument:

  float64  THE REFERENCE: the box-plus as min + log1p(exp(-(|a|+|b|))) - log1p(exp(-||a|-|b||)), clamped to [0, L],
           sign from (a < 0) != (b < 0);
  float32  an emulation of the kernels' arithmetic: every operation one numpy float32 operation, the box-plus on
           exp2 / log2 with the kernels' constants and its one fused multiply-add evaluated exactly and rounded once.

Also here: the tolerance of the GPU comparison, the near-zero band, the rule that finds the
codewords whose stop iteration the tolerance leaves open ("excusable"), the comparison of a decoder's columns with
the reference (compare_columns: an excused column that stopped at another iteration is judged against the
reference's values AT THAT iteration), and wrong variants of the decoder on purpose — stop rules and two dropped
clamps — for the premises of tests/test_cpu_layered_bp.py."""
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


def one_ulp(rng):
    """-> f(x): x float32 with every entry moved by -1, 0 or +1 ulp at random: what a transcendental that is accurate
    to 1 ulp, as the hardware's exp2 and log2 are, may give where numpy's gives x."""
    def move(x):
        s = rng.integers(-1, 2, np.shape(x))
        up, down = np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))
        return np.where(s == 0, x, np.where(s > 0, up, down)).astype(np.float32)
    return move


def boxplus(a, b, L, dtype, clamp=True, ulp=None):
    """`clamp=False` departs from the specification on purpose: the magnitude is bounded below by 0 only. `ulp`
    (one_ulp(rng); float32 form only) moves the result of each of the four transcendentals by up to 1 ulp."""
    if dtype == np.float64:
        aa, ab = np.abs(a), np.abs(b)
        mag = np.minimum(aa, ab) + np.log1p(np.exp(-(aa + ab))) - np.log1p(np.exp(-np.abs(aa - ab)))
        mag = np.clip(mag, 0.0, L if clamp else None)
        return np.where((a < 0) != (b < 0), -mag, mag)
    f32 = np.float32
    k_log2e, k_ln2 = f32(1.4426950408889634), f32(0.6931471805599453)
    aa, ab = np.abs(a), np.abs(b)
    mn = np.minimum(aa, ab)
    with np.errstate(under="ignore", over="ignore"):     # (|a| + |b|) log2(e) may be inf: exp2(-inf) is 0
        u = np.exp2(-(aa + ab) * k_log2e)
        v = np.exp2(-np.abs(aa - ab) * k_log2e)
    if ulp is None:
        dif = np.log2(f32(1) + u) - np.log2(f32(1) + v)
    else:
        dif = ulp(np.log2(f32(1) + ulp(u))) - ulp(np.log2(f32(1) + ulp(v)))
    # fmaf(ln2, dif, mn): the product of two float32 is exact in float64, the sum is rounded there and once more
    mag = (np.float64(k_ln2) * dif.astype(np.float64) + mn.astype(np.float64)).astype(f32)
    mag = np.clip(mag, f32(0), f32(L) if clamp else None)
    return np.where((a < 0) != (b < 0), -mag, mag).astype(f32)


def check_update(Q, L, dtype, clamp_deg2=True, clamp_boxplus=True, on_boxplus=None, ulp=None):
    """Q [checks][d][B] -> R' [checks][d][B] by the specification's forward-backward order. `clamp_deg2=False` and
    `clamp_boxplus=False` depart from the specification on purpose (the degree-2 messages are then plain copies of
    Q, the box-plus has no upper bound); `on_boxplus(a, b)` sees the two inputs of every box-plus and changes
    nothing."""
    d = Q.shape[1]
    Rn = np.empty_like(Q)
    if d == 2:
        Rn[:, 0] = np.clip(Q[:, 1], -L, L) if clamp_deg2 else Q[:, 1]
        Rn[:, 1] = np.clip(Q[:, 0], -L, L) if clamp_deg2 else Q[:, 0]
        return Rn

    def bp(a, b):
        if on_boxplus is not None:
            on_boxplus(a, b)
        return boxplus(a, b, L, dtype, clamp_boxplus, ulp)

    S = [None] * d
    S[d - 1] = Q[:, d - 1]
    for j in range(d - 2, 0, -1):
        S[j] = bp(Q[:, j], S[j + 1])
    Rn[:, 0] = S[1]
    F = Q[:, 0]
    for w in range(1, d - 1):
        Rn[:, w] = bp(F, S[w + 1])
        F = bp(Q[:, w], F)
    Rn[:, d - 1] = F
    return Rn


# ---- wrong stop rules, on purpose: those of tests/test_cpu_codewords.py, `stop_rule(A, P) -> bool [B]` ----
def no_decision_is_one(A, P):
    """Wrong: "the word is all-zero" for "the syndrome is zero"."""
    return ~(P < 0).any(axis=0)


def rotated_syndrome(A, P):
    """Wrong: the decisions gathered through variable index v - 1 instead of v."""
    x = np.roll((P < 0).astype(np.int32), 1, axis=0)
    return ((A @ x) % 2 == 0).all(axis=0)


WRONG_STOP_RULES = (no_decision_is_one, rotated_syndrome)


def layered_bp_decode(H, layers, llr, imax, llr_max=150.0, early_stop=True, dtype=np.float64, hook=None,
                      clamp_q=False, stop_rule=None, clamp_deg2=True, clamp_boxplus=True, check_hook=None,
                      run_all=False, ulp=None):
    """-> (out [N][B] dtype, iters [B] int32). `hook(it, P)` sees P [N][B] at the end of every iteration (the
    columns of finished codewords go on changing there; `out` holds their frozen values) and changes nothing.
    `clamp_q` departs from the specification on purpose: Q = clamp(P - R), the layered min-sum rule
    (tests/test_cpu_layered_bp.py shows what it breaks). So do `stop_rule(A, P) -> bool [B]` (a wrong stop test in
    place of "every check's decisions have even parity", as in tests/_layered_ref.py), `clamp_deg2=False` and
    `clamp_boxplus=False` (check_update): the default of each is the specification.
    `check_hook(it, Q [checks][d][B], done [B])` sees every check update's inputs before it runs and may return
    a callable that then sees the two inputs of each of its box-pluses; it changes nothing. `run_all` keeps the
    loop (and the hooks) going to imax after every codeword has stopped; out and iters are the same. `ulp`: boxplus's
    (float32 form: another evaluation of the same specification that is as legitimate as numpy's)."""
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
            on = check_hook(it, Q, done) if check_hook is not None else None
            Rn = check_update(Q, L, T, clamp_deg2, clamp_boxplus, on, ulp)
            R[e] = Rn
            P[v] = Q + Rn
        if hook is not None:
            hook(it, P)
        if early_stop:
            if stop_rule is None:
                x = (P < 0).astype(np.int32)
                ok = ((A @ x) % 2 == 0).all(axis=0) & ~done
            else:
                ok = np.asarray(stop_rule(A, P), dtype=bool) & ~done
            out[:, ok] = P[:, ok]
            iters[ok] = it
            done |= ok
            if done.all() and not run_all:
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


def reference_with_excusable(H, layers, llr, imax, llr_max=150.0, early_stop=True, record=False):
    """The float64 reference and the codewords whose stop iteration H5 leaves open -> (out, iters, excusable
    bool [B]), with `record` -> (out, iters, excusable, P_at float64 [imax][N][B]): P after every iteration, the
    columns of finished codewords included (they go on changing there), for compare_columns. A codeword is
    excusable when
      - at its reference stop iteration (imax for one that never stops) a variable lies in the near-zero band: a
        decoder within H5 may see another sign there and not stop, or
      - at an earlier iteration end the reference has no unsatisfied check free of in-band variables: every check
        that kept it running could be satisfied by a value within H5, so such a decoder may stop there.
    Without the early stop nothing is excusable (iters is imax everywhere)."""
    A = sp.csr_matrix(H)
    A.sort_indices()
    band_at, early_at, P_at = [], [], []

    def hook(it, P):
        if record:
            P_at.append(P.copy())
        band = in_band(P)
        x = (P < 0).astype(np.int32)
        unsat = (A @ x) % 2 == 1                                  # [n_c][B]
        has_band = (A @ band.astype(np.int32)) > 0
        band_at.append(band.any(axis=0))
        early_at.append(~(unsat & ~has_band).any(axis=0))         # no unsatisfied check free of in-band variables

    out, iters = layered_bp_decode(H, layers, llr, imax, llr_max, early_stop, np.float64, hook=hook, run_all=record)
    B = np.shape(llr)[1]
    exc = np.zeros(B, dtype=bool)
    if early_stop:
        for b in range(B):
            last = min(int(iters[b]), len(band_at))
            exc[b] = bool(band_at[last - 1][b]) or any(bool(early_at[i][b]) for i in range(last - 1))
    if record:
        return out, iters, exc, np.stack(P_at)
    return out, iters, exc


def reference_for_columns(it, ref):
    """The values a decoder's `out` is compared with, [N][B] float64. ref = (out, iters, excusable[, P_at]) of
    reference_with_excusable. A column whose `it` differs from the reference's and which is excusable stopped at
    another iteration than the reference and is frozen there: it is compared with the reference's P at the
    decoder's own stop iteration (P_at[it - 1]), not with the reference's frozen `out`. Every other column — equal
    iters, or not excusable (it then fails on iters) — is compared with `out` as before; without P_at, and for an
    `it` outside 1..imax, so is every column."""
    r_out, r_it, exc = ref[:3]
    want = np.array(r_out, dtype=np.float64, copy=True)
    if len(ref) > 3 and ref[3] is not None:
        P_at = ref[3]
        for b in np.flatnonzero((np.asarray(it) != r_it) & exc):
            if 1 <= int(it[b]) <= P_at.shape[0]:
                want[:, b] = P_at[int(it[b]) - 1][:, b]
    return want


def compare_columns(out, it, ref):
    """A decoder's (out, iters) against ref = (out, iters, excusable[, P_at]) -> dict of the findings the GPU tests
    assert on (tests/test_gpu_layered_bp.py compare): `bad` bool [N][B] the entries outside H5 of
    reference_for_columns, `flips` the hard decisions that differ from it outside H5's band around zero, `differ`
    bool [B] iters unequal, `unexcused` = differ & ~excusable, `excused` = the number of differ & excusable (capped
    at excuse_cap(B) by the caller), `want` the values compared with."""
    r_out, r_it, exc = ref[:3]
    want = reference_for_columns(it, ref)
    o = np.asarray(out, np.float64)
    differ = np.asarray(it) != r_it
    flips = int((((o < 0) != (want < 0)) & (np.abs(want) > REL * np.abs(want) + TOL_ABS)).sum())
    return dict(bad=h5_violations(o, want), flips=flips, differ=differ, unexcused=differ & ~exc,
                excused=int((differ & exc).sum()), want=want)


# ---- the inputs of tests/test_gpu_layered_bp_edges.py (premises: tests/test_cpu_layered_bp.py); read-only ----
EDGE_B, EDGE_IMAX = 16, 6
# both inside the precondition (|llr| + 16 llr_max < FLT_MAX). Two entries of HUGE in a box-plus: (|a| + |b|) log2(e)
# is 2.45e38, finite, and its exp2 is 0; two of HUGE_INF: |a| + |b| is already inf in fp32
HUGE, HUGE_INF = np.float32(2.0 ** 126), np.float32(2.0 ** 127)
SMALL_LLR_MAX = 7.5


def edge_code(name):
    """-> (H, layers, [N][EDGE_B] codewords) of tests/_codewords.py's "mixed" or "wlan"."""
    from tests import _codewords as cw
    H, _, layers, _ = cw.code(name)
    return H, layers, cw.codewords(name, EDGE_B)


def _rate(H):
    return 1.0 - H.shape[0] / H.shape[1]


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _recorded(H, layers, llr, imax, llr_max, early):
    """(out, iters, excusable, P_at (None without the stop: iters cannot differ there), converged)."""
    ref = reference_with_excusable(H, layers, llr, imax, llr_max=llr_max, early_stop=early, record=early)
    return _frozen(*ref[:3], ref[3] if early else None, syndrome_clean(H, ref[0]))


SATURATING_SEED = {"mixed": 22, "wlan": 22}


@functools.lru_cache(maxsize=None)
def saturating_input(name, random_huge_signs=False, huge=HUGE):
    """awgn_llr(3 dB at the code's rate) x 40 (most |P - R| beyond llr_max = 150 after an iteration), 1 % of the
    entries `huge` (2^126) and 1 % exactly 150, then every entry negated where the codeword's bit is 1: the huge entries
    agree with the codeword. `random_huge_signs`: the huge entries take random signs instead and frustrate their
    checks (no codeword is near; such a batch amplifies rounding from iteration 2 on and is decoded for one
    iteration only)."""
    from tests._layered_census import awgn_llr
    H, _, C = edge_code(name)
    n, B = C.shape
    seed = SATURATING_SEED[name]
    rng = np.random.default_rng(seed)
    x = awgn_llr(n, B, 3.0, seed, R=_rate(H)) * np.float32(40)
    k = max(4, n * B // 100)
    at = rng.choice(n * B, 2 * k, replace=False)
    x.reshape(-1)[at[:k]] = huge
    x.reshape(-1)[at[k:]] = np.float32(150)
    x = np.where(C == 1, -x, x).astype(np.float32)
    if random_huge_signs:
        x.reshape(-1)[at[:k]] = huge * rng.choice(np.array([-1.0, 1.0], np.float32), k)
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def small_llr_max_input():
    """mixed, awgn_llr(2 dB at the code's rate) negated by the codewords; decoded with llr_max = SMALL_LLR_MAX."""
    from tests._layered_census import awgn_llr
    H, _, C = edge_code("mixed")
    x = awgn_llr(H.shape[1], EDGE_B, 2.0, seed=23, R=_rate(H))
    return _frozen(np.where(C == 1, -x, x).astype(np.float32))


@functools.lru_cache(maxsize=None)
def quantised_input(name):
    """tests/_layered_census.py quantised_llr: integers in [-3, 7], about 5 % -0.0 and 5 % +0.0."""
    from tests._layered_census import quantised_llr
    H, _, _ = edge_code(name)
    return _frozen(quantised_llr(H.shape[1], EDGE_B, seed=21))


NEIGHBOUR_COLUMNS = ("quantised", "saturating", "subnormal", "zeros", "negative_zeros", "constant",
                     "constant_random_signs", "awgn")


@functools.lru_cache(maxsize=None)
def neighbours_input(name, B):
    """tests/_layered_census.py mixed_batch_llr (column b is family b mod 8 of NEIGHBOUR_COLUMNS) with its
    saturating columns, which carry +-FLT_MAX and so lie outside this decoder's precondition, replaced by the
    columns of saturating_input (b mod EDGE_B)."""
    from tests._layered_census import MIXED_BATCH_COLUMNS, mixed_batch_llr
    assert MIXED_BATCH_COLUMNS == NEIGHBOUR_COLUMNS
    H, _, _ = edge_code(name)
    x = mixed_batch_llr(H.shape[1], B, seed=31)
    sat = saturating_input(name)
    for b in range(NEIGHBOUR_COLUMNS.index("saturating"), B, len(NEIGHBOUR_COLUMNS)):
        x[:, b] = sat[:, b % EDGE_B]
    assert np.abs(x).max() == HUGE
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def edge_input(kind, name, B=None):
    return {"saturating": lambda: saturating_input(name), "frustrated": lambda: saturating_input(name, True),
            "overflow": lambda: saturating_input(name, huge=HUGE_INF),
            "small_llr_max": small_llr_max_input, "quantised": lambda: quantised_input(name),
            "neighbours": lambda: neighbours_input(name, B)}[kind]()


@functools.lru_cache(maxsize=None)
def edge_reference(kind, name, imax, early, llr_max=150.0, B=None):
    """The reference (_recorded: reference_with_excusable, P_at when the stop is on, and syndrome_clean of the
    final values as the last element, the convergence mask) of one of the inputs above: kind "saturating", "overflow"
    (saturating with HUGE_INF for HUGE), "frustrated", "small_llr_max", "quantised" or "neighbours" (with its B)."""
    H, layers, _ = edge_code(name)
    return _recorded(H, layers, edge_input(kind, name, B), imax, llr_max, early)


WLAN_NOISE_SCALE = np.float32(0.5)


@functools.lru_cache(maxsize=None)
def spread_input(name, B=None):
    """-> (LLRs, transmitted bits, kinds): tests/_codewords.py layered_input(name) — nonzero codewords at two noise
    levels, the all-zero codeword, sign-random noise; B = 130 unless given — with, on "wlan", the noise columns at
    half their magnitude. At full magnitude the WLAN code doubles a rounding difference on those columns, which
    never converge, in every iteration: the float32 form with transcendentals good to 1 ulp (one_ulp) leaves H5
    there by iteration 8 (1.44 and 1.34 times the bound in two draws), and so did an MI355X (1.24 times, 4 values
    of column 43), while no other column passes 0.1 of it. At half magnitude they still never stop, none is
    excusable, and the same draws stay at 0.02 of the bound (tests/test_cpu_layered_bp.py
    test_spread_inputs_bear_one_ulp_transcendentals). The other 122 columns, and with them the histogram of stops,
    are unchanged; "mixed" and "dvb" are as they are (0.07 and 0.52 of the bound on their noise columns)."""
    from tests import _codewords as cw
    llr, bits, kinds = cw.layered_input(name) if B is None else cw.layered_input(name, B)
    if name == "wlan":
        llr = np.array(llr, copy=True)
        llr[:, kinds == cw.KIND_NOISE] *= WLAN_NOISE_SCALE
        llr.setflags(write=False)
    return llr, bits, kinds


@functools.lru_cache(maxsize=None)
def spread_reference(name, early=True):
    """The reference on spread_input(name) (nonzero codewords, B = 130, i_max 8): (out, iters, excusable, P_at,
    converged = syndrome_clean of the final values)."""
    from tests import _codewords as cw
    H, _, layers, _ = cw.code(name)
    llr, _, _ = spread_input(name)
    return _recorded(H, layers, llr, cw.IMAX_LAYERED, 150.0, early)
