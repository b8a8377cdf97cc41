"""Nonzero codewords and their mirrored channel samples, shared by tests/test_cpu_codewords.py (which holds every
case to a stop inside the loop, on the references alone) and tests/test_gpu_codewords.py (which decodes them).

On a transmission of the all-zero codeword "the syndrome is zero" and "no decision is 1" become true together, so a
stop rule that mistakes one for the other, gathers its syndrome through a wrong variable or packs a decision at a
wrong bit passes every test whose input is all-zero. Here about half of the transmitted bits are 1:

  null_space_codewords   random codewords of any small code, by GF(2) elimination of H
  encoded_codewords      random codewords of a structured code through oracle.encoder_oracle
  mirrored_case          the 16-level channel sample of given codewords (cluster ids mirrored, LLRs negated by the
                         bits), the rows of degree-1 variables at the reliable level of the transmitted bit
  stop_spread_batch      one batch for the per-codeword stop of the layered decoders: codewords at two noise
                         levels, the all-zero codeword and sign-random noise, finished and running columns
                         alternating inside a tile and whole tiles that finish early
  the codes and cases    code / flood_input / flood_ref / layered_input / layered_ref / fixed_ref and the case
                         lists at the end, each reference computed once and read-only"""
import functools

import numpy as np
import scipy.sparse as sp

T_CH = 16
KIND_HI, KIND_LO, KIND_ZERO, KIND_NOISE = 0, 1, 2, 3
# even tiles of 64: finished (hi, zero) and running (lo, noise) columns side by side; odd tiles: all at the high
# Eb/N0, so the whole tile finishes early and is skipped (and freed by a compaction)
EVEN_TILE_PATTERN = (KIND_HI, KIND_LO, KIND_HI, KIND_NOISE, KIND_ZERO, KIND_LO, KIND_HI, KIND_LO)


def _info_bits(k, B, seed):
    return np.random.default_rng(seed).integers(0, 2, (k, B), dtype=np.uint8)


def _check_codewords(H, C):
    A = sp.csr_matrix(H).astype(np.int64)
    assert C.dtype == np.uint8 and C.shape[0] == A.shape[1]
    assert not ((A @ C.astype(np.int64)) & 1).any(), "H c != 0"
    assert C.any(axis=0).all(), "an all-zero column"
    return C


def null_space_codewords(H, B, seed):
    """[N][B] uint8 random codewords of H: dense GF(2) Gauss-Jordan elimination (codes of up to about 1000 columns),
    pivots taken from the highest column down so that the free variables are the lowest columns (for a systematic
    code with an invertible parity part: the information bits, drawn as encoded_codewords draws them), the free
    variables random and the pivots solved."""
    M = (np.asarray(sp.csr_matrix(H).todense()) & 1).astype(np.uint8)
    m, n = M.shape
    assert n <= 1200, "dense elimination: small codes only"
    piv_cols, r = [], 0
    for c in range(n - 1, -1, -1):
        if r == m:
            break
        hit = np.flatnonzero(M[r:, c])
        if hit.size == 0:
            continue
        p = r + int(hit[0])
        if p != r:
            M[[r, p]] = M[[p, r]]
        others = np.flatnonzero(M[:, c])
        others = others[others != r]
        M[others] ^= M[r]
        piv_cols.append(c)
        r += 1
    piv_cols = np.array(piv_cols, dtype=np.int64)
    free = np.setdiff1d(np.arange(n), piv_cols)
    C = np.zeros((n, B), dtype=np.uint8)
    C[free] = _info_bits(free.size, B, seed)
    # row i of the reduced matrix: x[piv_cols[i]] + sum over free columns = 0
    C[piv_cols] = ((M[:r][:, free].astype(np.int64) @ C[free].astype(np.int64)) & 1).astype(np.uint8)
    return _check_codewords(H, C)


def encoded_codewords(H, B, seed):
    """[N][B] uint8 systematic codewords of random information bits through the encoder oracle."""
    from oracle import encoder_oracle
    plan = encoder_oracle.EncoderPlan(H)
    C = np.ascontiguousarray(encoder_oracle.encode(plan, _info_bits(plan.K, B, seed)), dtype=np.uint8)
    return _check_codewords(H, C)


def quantiser(g, ebn0, T=T_CH):
    from informationbottleneckdecodingldpc_amd.channel import UniformQuantizer, sigma2_from_ebn0
    return UniformQuantizer(sigma2_from_ebn0(ebn0, g.R_c), T)


def mirrored_case(g, C, ebn0, seed, T=T_CH, offset=0):
    """-> (quantiser, cluster ids int32 [N][B], LLRs float32 [N][B]), read-only: the Philox channel sample of the
    codewords C (oracle.channel_sample: a bit 1 mirrors the cluster, t -> T-1-t), the LLRs those of the all-zero
    sample negated where the bit is 1 (output_LLRs is not exactly antisymmetric, so this is not output_LLRs of the
    mirrored id in the last bits), and the rows of degree-1 variables — they forward their channel value unchanged
    for ever — at the most reliable level of the transmitted bit."""
    from oracle import oracle
    q = quantiser(g, ebn0, T)
    N, B = C.shape
    assert N == g.n_v
    cdf = q.cdf_t_given_x_equals_zero
    ch = oracle.channel_sample(cdf, seed, offset, N, B, C)
    t0 = np.where(C == 1, T - 1 - ch, ch)
    deg1 = np.flatnonzero(np.asarray(g.vn_deg) == 1)
    t0[deg1] = T - 1
    ch[deg1] = np.where(C[deg1] == 1, 0, T - 1)
    L = q.output_LLRs.astype(np.float32)[t0]
    llr = np.where(C == 1, -L, L).astype(np.float32)
    ch = np.ascontiguousarray(ch, dtype=np.int32)
    ch.setflags(write=False)
    llr.setflags(write=False)
    return q, ch, llr


def spread_kinds(B, tile=64):
    """Column kinds of stop_spread_batch."""
    b = np.arange(B)
    pat = np.array(EVEN_TILE_PATTERN)[b % len(EVEN_TILE_PATTERN)]
    return np.where((b // tile) % 2 == 1, KIND_HI, pat).astype(np.int64)


def stop_spread_batch(g, C, seed, hi=6.0, lo=3.0, tile=64):
    """-> (LLRs float32 [N][B] read-only, transmitted bits uint8 [N][B] (zero on the zero and noise columns), kinds
    [B]) for the per-codeword stop. C: [N][B] nonzero codewords. Column b is, by spread_kinds: codeword b at `hi` dB,
    codeword b at `lo` dB, the all-zero codeword at `hi` dB, or the magnitudes of the `lo` sample with random signs
    (no codeword: it never stops)."""
    N, B = C.shape
    kinds = spread_kinds(B, tile)
    bits = np.where(np.isin(kinds, (KIND_HI, KIND_LO))[None, :], C, 0).astype(np.uint8)
    _, _, l_hi = mirrored_case(g, bits, hi, seed)
    _, _, l_lo = mirrored_case(g, bits, lo, seed + 1)
    llr = np.where((kinds == KIND_LO)[None, :], l_lo, l_hi).astype(np.float32)
    noise = np.flatnonzero(kinds == KIND_NOISE)
    sign = np.random.default_rng(seed + 2).choice(np.array([-1.0, 1.0], np.float32), (N, noise.size))
    llr[:, noise] = np.abs(l_lo[:, noise]) * sign
    llr.setflags(write=False)
    bits.setflags(write=False)
    return llr, bits, kinds


# ---------------------------------------------------------------------------------------------------------------
# codes: name -> (H, codewords by "encoder" or "null"); layered ones also carry their layers
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def code(name):
    """-> (H csr, build_graph(H), layers or None, how the codewords are made)."""
    from informationbottleneckdecodingldpc_amd import codes, graph
    from tests import _layered_census as lc, _layered_wide as lw, _minsum_corrected_ref as R
    from tests._codes import fold_census_code, mixed_code
    layers = None
    if name == "wlan":
        H, layers = lc.wlan(27)
        how = "encoder"
    elif name == "wlan54":          # N = 1296, the code of tests/test_gpu_ib.py's multi-group cases
        H, how = codes.wlan_80211n(54), "encoder"
    elif name == "mixed":
        H, layers = lc.mixed()
        how = "null"
    elif name == "fold":
        H, how = fold_census_code(), "null"
    elif name == "mixed16":
        H, how = mixed_code(np.arange(2, 17), np.array([2, 3, 3, 4, 6, 12, 16]), 500, seed=5), "null"
    elif name == "dvb":
        H, how = R.dvb_H(), "encoder"
        layers = codes.dvbs2_layers(H)
    elif name == "small30":
        H, layers = lw.small30()
        how = "encoder"
    elif name == "wide_mixed":
        H, layers = lw.wide_mixed()
        how = "null"
    else:
        raise KeyError(name)
    H = codes.canonical_csr(H)
    return H, graph.build_graph(H), layers, how


@functools.lru_cache(maxsize=None)
def codewords(name, B, seed=1):
    H, _, _, how = code(name)
    C = (encoded_codewords if how == "encoder" else null_space_codewords)(H, B, seed)
    C.setflags(write=False)
    return C


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


IMAX_FLOOD, IMAX_LAYERED, ALPHA_LAYERED = 10, 8, 0.8125
CORRECTED = (0.8125, 0.15)


@functools.lru_cache(maxsize=None)
def flood_input(name, B, ebn0):
    """-> (tables for the IB decoder, cluster ids, float32 LLRs, codewords) of one flooding case."""
    from informationbottleneckdecodingldpc_amd import tables
    _, g, _, _ = code(name)
    C = codewords(name, B)
    q, ch, llr = mirrored_case(g, C, ebn0, seed=B)
    tb = tables.llr_tables(q.output_LLRs, g.d_c_max, g.d_v_max, IMAX_FLOOD)
    return tb, ch, llr, C


def ib_match(name):
    """Matching on, except on the two codes of every check degree 2..16: their matching decoder needs more check
    tables than the fast path's 16 LDS slots and would run the generic kernels (tests/test_gpu_degree_profiles.py
    test_ib_drawn_degree_set_runs_generic), and they are here for the check-16 kernel pairings."""
    return name not in ("mixed", "mixed16")


@functools.lru_cache(maxsize=None)
def flood_ref(name, B, ebn0, family, early=True):
    """-> (reference output, stop iteration). family: "ib", "ms32", "ms64", "bp64", "corr32", "corr64"."""
    from oracle import oracle
    from tests import _minsum_corrected_ref as R
    _, g, _, _ = code(name)
    tb, ch, llr, _ = flood_input(name, B, ebn0)
    if family == "ib":
        out, it = oracle.ib_decode(g, tb, ch, match=ib_match(name), early_stop=early, return_iters=True)
    elif family == "ms32":
        out, it = oracle.float32_decode(g, IMAX_FLOOD, llr, early_stop=early, return_iters=True)
    elif family in ("ms64", "bp64"):
        out, it = oracle.float_decode(g, oracle.BP if family == "bp64" else oracle.MINSUM, IMAX_FLOOD,
                                      llr.astype(np.float64), early_stop=early, return_iters=True)
    else:
        dt = np.float32 if family == "corr32" else np.float64
        out, it = R.decode(g, CORRECTED[0], CORRECTED[1], IMAX_FLOOD, llr.astype(dt), dt, early_stop=early)
    return _frozen(out)[0], int(it)


def bp_oracle_is_the_true_boxplus(g, llr, llr_max=150.0):
    """Whether the fp64 BP oracle is a reference for the fp32 decoder on this input. The oracle evaluates the
    reference's log((1 + e^(a+b)) / (e^a + e^b)), whose e^(a+b) overflows for a + b > 709.78 and then gives llr_max
    instead of about min(a, b); the fp32 decoder's form does not overflow (csrc/float_kernels.hip boxplus). Only the
    first check pass can differ: it folds the raw channel values — above about 7 dB the top level's LLR is
    log(p0 / 1e-300), about 680 — while every later input is a message clamped to llr_max. So: that pass's messages
    (the oracle's fold order, oracle/float_oracle.inc) in both forms, float64, equal within 1e-9."""
    x = np.asarray(llr, dtype=np.float64)
    cols = np.asarray(g.csr_cols, dtype=np.int64)
    start, deg = np.asarray(g.cn_start, dtype=np.int64), np.asarray(g.cn_deg)

    def naive(a, b):
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            return np.clip(np.log((1.0 + np.exp(a + b)) / (np.exp(a) + np.exp(b))), -llr_max, llr_max)

    def true(a, b):
        aa, ab = np.abs(a), np.abs(b)
        mag = np.minimum(aa, ab) + np.log1p(np.exp(-(aa + ab))) - np.log1p(np.exp(-np.abs(aa - ab)))
        return np.clip(np.where((a < 0) != (b < 0), -mag, mag), -llr_max, llr_max)

    worst = 0.0
    for d in np.unique(deg):
        if d < 3:
            continue
        m = x[cols[start[deg == d][:, None] + np.arange(d)[None, :]]]      # [checks][d][B]
        for w in range(d):
            others = [v for v in range(d) if v != w]
            t_n = t_t = m[:, others[0]]
            for v in others[1:]:
                t_n, t_t = naive(m[:, v], t_n), true(m[:, v], t_t)
            bad = ~(np.abs(t_n - t_t) <= 1e-9)
            if bad.any():
                worst = max(worst, float(np.nanmax(np.abs(t_n - t_t)[bad])))
    return worst == 0.0


def decided_ones(out, family):
    """Hard decisions (1 = bit 1) of a reference or device output."""
    return (out < T_CH // 2) if family == "ib" else (out < 0)


# (high, low) Eb/N0 of stop_spread_batch: at 3 dB no codeword of the rate-9/10 code converges within 8 iterations
LAYERED_DB = {"small30": (6.0, 4.5)}
LAYERED_B = 130        # three tiles of 64, the last of two columns


@functools.lru_cache(maxsize=None)
def layered_input(name, B=LAYERED_B):
    """-> (LLRs, transmitted bits, kinds) of stop_spread_batch on a layered code."""
    _, g, _, _ = code(name)
    hi, lo = LAYERED_DB.get(name, (6.0, 3.0))
    return stop_spread_batch(g, codewords(name, B), seed=B, hi=hi, lo=lo)


@functools.lru_cache(maxsize=None)
def layered_ref(name, B=LAYERED_B, early=True):
    from tests._layered_ref import layered_decode
    H, _, layers, _ = code(name)
    llr, _, _ = layered_input(name, B)
    return _frozen(*layered_decode(H, layers, llr, IMAX_LAYERED, ALPHA_LAYERED, 0.0, early_stop=early))


@functools.lru_cache(maxsize=None)
def fixed_ref(name, params, B=LAYERED_B, early=True):
    from tests._layered_fixed_ref import fixed_decode, quantise
    H, _, layers, _ = code(name)
    llr, _, _ = layered_input(name, B)
    return _frozen(*fixed_decode(H, layers, quantise(llr, params[3]), IMAX_LAYERED, *params[:3], early_stop=early))


def converged(iters, imax=IMAX_LAYERED):
    """Columns the per-codeword stop finished (a column whose syndrome only clears in iteration imax is not
    checked any more and reports imax like one that never converges)."""
    return np.asarray(iters) < imax


# ---------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_codewords.py; tests/test_cpu_codewords.py asserts every one's stop on the references
# ---------------------------------------------------------------------------------------------------------------
# IB (llr_tables, matching as ib_match says): (code, B, Eb/N0). At 6 dB the batch-global stop of 260 codewords of the two mixed
# codes does not come before imax - 1: 9 dB there. 4100 is test_gpu_ib.py test_ib_fused_table_sets' batch.
IB_CASES = [("wlan", 130, 6.0), ("wlan54", 4100, 12.0),("dvb", 300, 6.0), ("fold", 260, 6.0), ("wlan", 9, 6.0),
            ("wlan", 24, 6.0), ("mixed", 24, 6.0), ("mixed16", 24, 6.0), ("mixed", 260, 9.0), ("mixed16", 260, 9.0)]
# flooding float decoders: (code, B) -> Eb/N0 of the plain (min-sum, BP) and of the corrected families; the
# corrected decoder needs imax - 1 iterations for 300 codewords of dvb at 6 dB: 10 dB there. 260 codewords of mixed
# do not converge at 6 dB, and at 9 dB the fp64 BP oracle is no reference (bp_oracle_is_the_true_boxplus): 8 dB.
FLOAT_CASES = {("mixed", 260): (8.0, 8.0), ("dvb", 300): (6.0, 10.0), ("mixed", 24): (6.0, 6.0),
               ("mixed", 5): (6.0, 6.0), ("wlan", 70): (6.0, 6.0)}
FLOAT_FAMILIES = ("ms32", "ms64", "bp64", "corr32", "corr64")


def fused_groups_db(family):
    """Eb/N0 of the fused float kernels' case past the first group (its B is read from the device's geometry):
    12 dB, where a batch of thousands stops at once; BP at 7.3 dB, the highest at which the channel LLRs leave the
    fp64 oracle's box-plus exact (bp_oracle_is_the_true_boxplus) and the batch still stops inside the loop."""
    return 7.3 if family == "bp64" else 12.0


LAYERED_CODES = ("wlan", "mixed", "dvb", "wide_mixed", "small30")
FIXED_CODES = ("dvb", "wide_mixed", "small30")


def float_db(name, B, family):
    plain, corr = FLOAT_CASES[(name, B)]
    return corr if family.startswith("corr") else plain
