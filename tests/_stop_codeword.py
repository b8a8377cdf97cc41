"""Inputs and per-column references of the per-codeword stop on the fused flooding decoders (float and IB), shared by
tests/test_cpu_stop_codeword.py (which pins the premises on the oracles alone) and tests/test_gpu_stop_codeword.py.

The reference of column c is the oracle decoding that column alone with early_stop=True: the definition of
include/ibldpc.h "Per-codeword stop". Every reference is computed once and read-only."""
import functools

import numpy as np

from tests import _codewords as cw

IMAX = cw.IMAX_FLOOD
FAMILIES = ("ms32", "ms64", "corr32", "corr64", "bp64")
NAME = "wlan"


@functools.lru_cache(maxsize=None)
def spread_input(B):
    """-> (LLRs float32 [N][B], transmitted bits, kinds): codewords at 6 and 3 dB, the all-zero word, noise."""
    g = cw.code(NAME)[1]
    return cw.stop_spread_batch(g, cw.codewords(NAME, B), seed=7, hi=6.0, lo=3.0)


def high_db(family):
    """12 dB, where every column stops at its first possible pass; BP at 7.3 dB (cw.fused_groups_db: the highest at
    which the fp64 oracle's box-plus is exact)."""
    return cw.fused_groups_db(family)


@functools.lru_cache(maxsize=None)
def high_input(B, ebn0):
    return cw.flood_input(NAME, B, ebn0)[2]


def decode_columns(family, llr, imax=IMAX, early=True):
    """Oracle of `family` on every column of llr alone -> (out [N][B] in the family's dtype, iters int32 [B])."""
    from oracle import oracle
    from tests import _minsum_corrected_ref as R
    g = cw.code(NAME)[1]
    llr = np.asarray(llr)
    outs, its = [], []
    for c in range(llr.shape[1]):
        col = np.ascontiguousarray(llr[:, c:c + 1])
        if family == "ms32":
            o, it = oracle.float32_decode(g, imax, col.astype(np.float32), early_stop=early, return_iters=True)
        elif family in ("ms64", "bp64"):
            o, it = oracle.float_decode(g, oracle.BP if family == "bp64" else oracle.MINSUM, imax,
                                        col.astype(np.float64), early_stop=early, return_iters=True)
        else:
            dt = np.float32 if family == "corr32" else np.float64
            o, it = R.decode(g, cw.CORRECTED[0], cw.CORRECTED[1], imax, col.astype(dt), dt, early_stop=early)
        outs.append(o)
        its.append(int(it))
    out = np.concatenate(outs, axis=1)
    it = np.array(its, dtype=np.int32)
    out.setflags(write=False)
    it.setflags(write=False)
    return out, it


@functools.lru_cache(maxsize=None)
def spread_ref(family, B):
    return decode_columns(family, spread_input(B)[0])


@functools.lru_cache(maxsize=None)
def high_ref(family, B):
    return decode_columns(family, high_input(B, high_db(family)))


def batch_stop(family, llr, imax=IMAX):
    """The batch-global stop iteration of the same input (today's early_stop=True on the whole batch)."""
    from oracle import oracle
    from tests import _minsum_corrected_ref as R
    g = cw.code(NAME)[1]
    if family == "ms32":
        return int(oracle.float32_decode(g, imax, np.asarray(llr, np.float32), early_stop=True, return_iters=True)[1])
    if family in ("ms64", "bp64"):
        return int(oracle.float_decode(g, oracle.BP if family == "bp64" else oracle.MINSUM, imax,
                                       np.asarray(llr, np.float64), early_stop=True, return_iters=True)[1])
    dt = np.float32 if family == "corr32" else np.float64
    return int(R.decode(g, cw.CORRECTED[0], cw.CORRECTED[1], imax, np.asarray(llr, dt), dt, early_stop=True)[1])


def unsatisfied(out, H):
    """Per column: whether the hard decisions of `out` (1 = negative) violate a check of H."""
    bits = (np.asarray(out) < 0).astype(np.int64)
    return (((H.astype(np.int64) @ bits) & 1) != 0).any(axis=0)


# ---------------------------------------------------------------------------------------------------------------
# information-bottleneck decoder: the same construction on cluster ids
# ---------------------------------------------------------------------------------------------------------------
IB_CODES = {"wlan": (130, 6.0, 3.0), "reg39": (4100, 6.0, 3.5)}     # name -> (B, high, low Eb/N0)


@functools.lru_cache(maxsize=None)
def ib_code(name):
    """-> (H, graph, matching): "wlan" (Z = 27), or "reg39", the regular (3, 9) N = 900 code whose passes take two
    table quads (tests/test_gpu_ib.py test_ib_fused_table_sets)."""
    from informationbottleneckdecodingldpc_amd import codes, graph
    if name == "wlan":
        H, g, _, _ = cw.code("wlan")
        return H, g, cw.ib_match("wlan")
    H = codes.canonical_csr(codes.regular_code(900, 3, 9, seed=0))
    return H, graph.build_graph(H), True


@functools.lru_cache(maxsize=None)
def ib_input(name, B=None, imax=IMAX):
    """-> (tables of the high quantiser, cluster ids int32 [N][B], kinds): codeword b at the high or the low Eb/N0 or
    the all-zero word (cw.mirrored_case with seeds 7 / 8, columns by cw.spread_kinds), uniformly random ids on the
    noise columns."""
    from informationbottleneckdecodingldpc_amd import tables
    H, g, _ = ib_code(name)
    B0, hi, lo = IB_CODES[name]
    B = B0 if B is None else B
    C = cw.codewords("wlan", B) if name == "wlan" else cw.null_space_codewords(H, B, 1)
    kinds = cw.spread_kinds(B)
    bits = np.where(np.isin(kinds, (cw.KIND_HI, cw.KIND_LO))[None, :], C, 0).astype(np.uint8)
    q, c_hi, _ = cw.mirrored_case(g, bits, hi, 7)
    _, c_lo, _ = cw.mirrored_case(g, bits, lo, 8)
    ch = np.where((kinds == cw.KIND_LO)[None, :], c_lo, c_hi).astype(np.int32)
    noise = np.flatnonzero(kinds == cw.KIND_NOISE)
    ch[:, noise] = np.random.default_rng(9).integers(0, cw.T_CH, (g.n_v, noise.size))
    tb = tables.llr_tables(q.output_LLRs, g.d_c_max, g.d_v_max, imax)
    ch.setflags(write=False)
    return tb, ch, kinds


def ib_decode_columns(name, tb, ch, early=True):
    """oracle.ib_decode on every column alone -> (out int32 [N][B], iters int32 [B])."""
    from oracle import oracle
    _, g, match = ib_code(name)
    outs, its = [], []
    for c in range(ch.shape[1]):
        o, it = oracle.ib_decode(g, tb, np.ascontiguousarray(ch[:, c:c + 1]), match=match, early_stop=early,
                                 return_iters=True)
        outs.append(np.asarray(o).astype(np.int32))
        its.append(int(it))
    out = np.concatenate(outs, axis=1)
    it = np.array(its, dtype=np.int32)
    out.setflags(write=False)
    it.setflags(write=False)
    return out, it


@functools.lru_cache(maxsize=None)
def ib_ref(name, B=None, imax=IMAX):
    tb, ch, _ = ib_input(name, B, imax)
    return ib_decode_columns(name, tb, ch)


def ib_batch_stop(name, B=None):
    from oracle import oracle
    _, g, match = ib_code(name)
    tb, ch, _ = ib_input(name, B)
    return int(oracle.ib_decode(g, tb, ch, match=match, early_stop=True, return_iters=True)[1])


def ib_unsatisfied(out, H):
    bits = (np.asarray(out) < cw.T_CH // 2).astype(np.int64)
    return (((H.astype(np.int64) @ bits) & 1) != 0).any(axis=0)
