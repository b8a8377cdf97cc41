"""What the tests of the wide flooding float decoders (a check of degree 17..32) share: the codes of
tests/_layered_wide.py, their AWGN inputs, and a numpy float32 restatement of the fp32 BP decoder.

``bp32_decode`` follows oracle/float_oracle.inc's schedule (as tests/_minsum_corrected_ref.decode does) with the fp32
decoder's check update: the overflow-free box-plus sgn(a) sgn(b) min(|a|, |b|) + ln(1 + e^-(|a|+|b|)) -
ln(1 + e^-||a|-|b||) on base-2 exp / log, clamped to [0, llr_max], and the forward-backward association order of
float_kernels.hip — S_j = m_j [+] S_{j+1} from S_{d-1} = m_{d-1}, output w = P_w [+] S_{w+1}, P_{w+1} = m_w [+] P_w
from P_1 = m_0 — at every degree. numpy's exp2 / log2 are not the device's instructions, so the restatement is not
bit-exact with the kernels; it shows that this ORDER of float32 operations stays within the project's fp32 BP criterion
of the fp64 oracle at the inputs the GPU tests then use (tests/test_cpu_float_wide.py)."""
import functools

import numpy as np

from tests._layered_census import awgn_llr
from tests._layered_wide import code_rate, small30, wide_mixed
from tests._minsum_corrected_ref import _by_degree

SEED = 41
REL, TOL_ABS = 1e-5, 1e-4          # the fp32 BP criterion (tests/test_gpu_float.py _h5)
CORRECTED = [(0.8125, 0.25), (1.0, 0.0)]


@functools.lru_cache(maxsize=None)
def wide_graph(name):
    from informationbottleneckdecodingldpc_amd import graph
    return graph.build_graph({"wide_mixed": wide_mixed, "small30": small30}[name]()[0])


@functools.lru_cache(maxsize=None)
def wide_llr(name, B, dB):
    """float32 AWGN LLRs of the all-zero codeword at the code's rate (read-only, shared)."""
    H = {"wide_mixed": wide_mixed, "small30": small30}[name]()[0]
    x = awgn_llr(H.shape[1], B, dB, seed=SEED, R=code_rate(H))
    x.setflags(write=False)
    return x


def h5(out, ref):
    """Entries outside the fp32 BP criterion."""
    return np.abs(out - ref) > REL * np.maximum(np.abs(out), np.abs(ref)) + TOL_ABS


_F = np.float32
_LOG2E, _LN2 = _F(1.4426950408889634), _F(0.6931471805599453)


def boxplus32(a, b, lm):
    aa, ab = np.abs(a), np.abs(b)
    mn = np.minimum(aa, ab)
    u = np.exp2(-(aa + ab) * _LOG2E)
    v = np.exp2(-np.abs(aa - ab) * _LOG2E)
    dif = np.log2(_F(1) + u) - np.log2(_F(1) + v)
    # one fused multiply-add: the product of two float32 is exact in float64
    mag = (np.float64(_LN2) * dif.astype(np.float64) + mn.astype(np.float64)).astype(_F)
    mag = np.clip(mag, _F(0), lm)
    return np.where((a < 0) != (b < 0), -mag, mag)


def bp32_check(m, lm):
    """Outputs [checks][d][B] of the inputs m [checks][d][B] (d >= 2), forward-backward in the kernels' order."""
    d = m.shape[1]
    out = np.empty_like(m)
    if d == 2:
        out[:, 0], out[:, 1] = np.clip(m[:, 1], -lm, lm), np.clip(m[:, 0], -lm, lm)
        return out
    S = [None] * d
    S[d - 1] = m[:, d - 1]
    for j in range(d - 2, 0, -1):
        S[j] = boxplus32(m[:, j], S[j + 1], lm)
    out[:, 0] = np.clip(S[1], -lm, lm)
    P = m[:, 0]
    for w in range(1, d - 1):
        out[:, w] = np.clip(boxplus32(P, S[w + 1], lm), -lm, lm)
        P = boxplus32(m[:, w], P, lm)
    out[:, d - 1] = np.clip(P, -lm, lm)
    return out


def bp32_decode(g, imax, llr, early_stop=False, llr_max=150.0):
    """(APP LLRs [N][B] float32, iterations run)."""
    ch = np.ascontiguousarray(llr, dtype=_F)
    B = ch.shape[1]
    lm, zero = _F(llr_max), _F(0)
    cgroups = _by_degree(np.asarray(g.cn_start), np.asarray(g.cn_deg))
    vgroups = _by_degree(np.asarray(g.vn_start), np.asarray(g.vn_deg))
    tgt_cn, tgt_vn = np.asarray(g.tgt_cn, dtype=np.int64), np.asarray(g.tgt_vn, dtype=np.int64)
    cin = np.zeros((g.n_e, B), dtype=_F)
    vin = np.zeros((g.n_e, B), dtype=_F)
    for d, idx, nodes in vgroups:
        for w in range(d):
            cin[tgt_vn[idx[:, w]]] = ch[nodes]
    i, stop = 1, False
    while i < imax and not stop:
        for d, idx, _ in cgroups:
            vin[tgt_cn[idx]] = bp32_check(cin[idx], lm)
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
            stop = sum(int(np.bitwise_xor.reduce(neg[idx], axis=1).sum()) for _, idx, _ in cgroups) == 0
        i += 1
    out = np.empty_like(ch)
    for d, idx, nodes in vgroups:
        m = vin[idx]
        x = ch[nodes]
        for v in range(d):
            x = x + m[:, v]
        out[nodes] = x
    assert out.dtype == _F
    return out, i - 1
