"""Numpy reference of the corrected (normalised / offset) flooding min-sum decoder, and the inputs the CPU and
GPU tests of it share (include/ibldpc.h "Corrected min-sum").

``decode`` restates the whole decode, vectorised over checks of one degree and over the batch, in float32 or
float64, following oracle/float_oracle.inc's schedule and operation order: first send = the raw channel value;
check update = the closed form of the specification (M, s, t = a * M, u = t - b, r = max(u, 0)), every operation an
individually rounded numpy operation of the decoder's dtype; variable update = channel first, then the other edges
ascending, clamped to +-llr_max; syndrome on ``< 0`` of the variable-to-check messages after each iteration; APP
output unclamped; ``imax - 1`` iterations unless the batch-global stop comes first. At (1, 0) it equals
``oracle.float32_decode`` / ``oracle.float_decode(kind=0)`` bit for bit (tests/test_cpu_minsum_corrected.py), which
is what pins it.
"""
import numpy as np

from informationbottleneckdecodingldpc_amd.channel import UniformQuantizer, sigma2_from_ebn0

PAIRS = [(0.8125, 0.15), (1.0, 0.25), (0.75, 0.5)]
MIXED_PAIRS = PAIRS[:2]   # the halves family on the mixed code: (0.75, 0.5) zeroes too much to show anything


def _by_degree(start, deg):
    """[(degree, edge index array [nodes][degree], node indices)] of the nodes grouped by degree."""
    out = []
    for d in np.unique(deg):
        nodes = np.flatnonzero(deg == d)
        out.append((int(d), start[nodes][:, None].astype(np.int64) + np.arange(int(d))[None, :], nodes))
    return out


def decode(g, alpha, beta, imax, llr, dtype, early_stop=False, llr_max=150.0, fma=False, census=None):
    """(APP LLRs [N][B] of ``dtype``, iterations run). ``fma``: t and u replaced by one fused multiply-add (float32
    only: exact in float64, rounded once) — the arithmetic the decoder must NOT have. ``census``: a dict that
    receives the counts over all check passes: outputs, outputs zeroed by max(., 0) although M != 0, check x
    codeword pairs, and those with equal smallest and second-smallest magnitude."""
    F = np.dtype(dtype).type
    ch = np.ascontiguousarray(llr, dtype=F)
    B = ch.shape[1]
    a, b, lm, zero = F(alpha), F(beta), F(llr_max), F(0)
    cgroups = _by_degree(np.asarray(g.cn_start), np.asarray(g.cn_deg))
    vgroups = _by_degree(np.asarray(g.vn_start), np.asarray(g.vn_deg))
    tgt_cn, tgt_vn = np.asarray(g.tgt_cn, dtype=np.int64), np.asarray(g.tgt_vn, dtype=np.int64)
    cin = np.zeros((g.n_e, B), dtype=F)
    vin = np.zeros((g.n_e, B), dtype=F)
    for d, idx, nodes in vgroups:
        for w in range(d):
            cin[tgt_vn[idx[:, w]]] = ch[nodes]
    cnt = dict(outputs=0, zeroed=0, checks=0, tied=0)
    i, stop = 1, False
    with np.errstate(invalid="ignore", over="ignore"):
        while i < imax and not stop:
            for d, idx, _ in cgroups:
                m = cin[idx]                                   # [checks][d][B]
                mag = np.abs(m)
                two = np.sort(mag, axis=1)[:, :2]
                m1, m2 = two[:, 0], two[:, 1]
                neg = m < zero
                par = np.bitwise_xor.reduce(neg, axis=1)
                cnt["checks"] += m1.size
                cnt["tied"] += int((m1 == m2).sum())
                for w in range(d):
                    M = np.where(mag[:, w] == m1, m2, m1)      # min over the others (on a tie m2 == m1)
                    if fma:
                        assert F is np.float32
                        u = (np.float64(a) * M.astype(np.float64) - np.float64(b)).astype(np.float32)
                    else:
                        t = a * M
                        u = t - b
                    r = np.maximum(u, zero)
                    cnt["outputs"] += r.size
                    cnt["zeroed"] += int(((r == zero) & (M != zero)).sum())
                    vin[tgt_cn[idx[:, w]]] = np.where(par ^ neg[:, w], -r, r)
            for d, idx, nodes in vgroups:
                m = vin[idx]
                for w in range(d):
                    x = ch[nodes]
                    for v in range(d):
                        if v != w:
                            x = x + m[:, v]
                    cin[tgt_vn[idx[:, w]]] = np.clip(x, -lm, lm)
            if early_stop:
                neg = cin < zero
                syn = 0
                for d, idx, _ in cgroups:
                    syn += int(np.bitwise_xor.reduce(neg[idx], axis=1).sum())
                stop = syn == 0
            i += 1
        out = np.empty_like(ch)
        for d, idx, nodes in vgroups:
            m = vin[idx]
            x = ch[nodes]
            for v in range(d):
                x = x + m[:, v]
            out[nodes] = x
    if census is not None:
        census.update(cnt)
    assert out.dtype == F
    return out, i - 1


# ------------------------------------------------------------------ shared inputs
def quantised_llrs(g, B, ebn0, seed):
    """The 16-level quantised AWGN LLRs of an all-zero codeword (UniformQuantizer), float64."""
    q = UniformQuantizer(sigma2_from_ebn0(ebn0, g.R_c), 16)
    return q.llr_of(q.sample_all_zero(g.n_v, B, np.random.default_rng(seed)))


def halves_llrs(g, B, seed):
    """Integers in [-3, 7] x 0.5: exact in every precision, with many zeros, ties and both signs."""
    return np.random.default_rng(seed).integers(-3, 8, size=(g.n_v, B)).astype(np.float64) * 0.5


def awgn_llrs(g, B, ebn0, seed):
    """Continuous AWGN LLRs of the all-zero codeword."""
    s2 = sigma2_from_ebn0(ebn0, g.R_c)
    y = 1.0 + np.sqrt(s2) * np.random.default_rng(seed).standard_normal((g.n_v, B))
    return 2 * y / s2


def mixed_H():
    from tests._codes import mixed_code
    return mixed_code(np.arange(2, 17), np.arange(1, 17), 600, seed=15)


def dvb_H():
    from informationbottleneckdecodingldpc_amd import codes
    return codes.dvbs2_structured(seed=3, n=7200, k=3600, groups_hi=4)


def wlan_H():
    from informationbottleneckdecodingldpc_amd import codes
    return codes.wlan_80211n(27)
