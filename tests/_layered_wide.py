"""Codes and inputs of the wide layered tests (check degrees 17..32): tests/test_cpu_layered_wide.py holds them to
what the GPU tests rest on, tests/test_gpu_layered_wide.py decodes them.

  wide_mixed   a small irregular code of every check degree 2..32, four checks each, with its greedy layers
  small30      a DVB-S2-structured N = 11160 rate 9/10 code (check degrees {29: 1, 30: 1079}, q = 3) with its three
               residue layers: the long-code shape, small enough for the fused kernel at 2 codewords per workgroup"""
import functools

import numpy as np
import scipy.sparse as sp

from tests._layered_census import awgn_llr
from tests._layered_fixed_ref import fixed_decode, quantise
from tests._layered_ref import layered_decode

WIDE_DEGREES = list(range(2, 33))
WIDE_PAIRS = {(d, p) for d in range(17, 33) for p in range(d)}   # 392 (degree, first-argmin position) pairs
WIDE_N, WIDE_PER_DEGREE = 400, 4
CENSUS_BATCHES, CENSUS_IMAX = (16, 130), 6
AWGN_DB, AWGN_SEED = 3.0, 41            # the AWGN input of the census and of the GPU tests on wide_mixed
WIDE_AB = [(1.0, 0.0), (0.8125, 0.25)]
WIDE_FAMILIES = ("quantised", "saturating", "subnormal")
FIXED_PARAMS = [(13, 0, 31, 2.0), (16, 1, 63, 3.3)]

SMALL30_DB, SMALL30_B, SMALL30_IMAX, SMALL30_SEED, SMALL30_ALPHA = 4.0, 130, 8, 7, 0.8125


@functools.lru_cache(maxsize=None)
def wide_mixed():
    """124 x 400: four checks of each degree 2..32, the degrees shuffled over the rows, every check's variables
    drawn without repetition (no double edge), the first draws walking a permutation of the variables so that each
    has degree >= 1. (tests/_codes.mixed_code stops at degree 16.)"""
    from informationbottleneckdecodingldpc_amd import codes
    rng = np.random.default_rng(11)
    degs = rng.permutation(np.repeat(WIDE_DEGREES, WIDE_PER_DEGREE))
    cover = rng.permutation(WIDE_N).tolist()
    rows, cols = [], []
    for c, d in enumerate(degs.tolist()):
        take = [cover.pop() for _ in range(min(d, len(cover)))]
        rest = np.setdiff1d(np.arange(WIDE_N), take)
        vs = np.concatenate([take, rng.choice(rest, d - len(take), replace=False)]).astype(np.int64)
        rows += [c] * d
        cols += vs.tolist()
    H = sp.csr_matrix((np.ones(len(rows), dtype=np.int64), (rows, cols)), shape=(len(degs), WIDE_N))
    H = codes.canonical_csr(H)
    assert H.nnz == len(rows) and not cover
    return H, codes.greedy_layers(H)


@functools.lru_cache(maxsize=None)
def small30():
    from informationbottleneckdecodingldpc_amd import codes
    H = codes.dvbs2_structured(seed=5, n=11160, k=10080, groups_hi=0, deg_hi=3, deg_lo=3)
    return H, codes.dvbs2_layers(H)


def code_rate(H):
    return 1.0 - H.shape[0] / H.shape[1]


@functools.lru_cache(maxsize=None)
def wide_awgn(B):
    H, _ = wide_mixed()
    x = awgn_llr(H.shape[1], B, AWGN_DB, seed=AWGN_SEED, R=code_rate(H))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def small30_llr(B=SMALL30_B):
    H, _ = small30()
    x = awgn_llr(H.shape[1], B, SMALL30_DB, seed=SMALL30_SEED, R=code_rate(H))
    x.setflags(write=False)
    return x


def _frozen(res):
    for r in res:
        r.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def small30_ref(early=True, B=SMALL30_B):
    """fp32 reference of small30 at alpha 0.8125, 8 iterations."""
    H, layers = small30()
    return _frozen(layered_decode(H, layers, small30_llr(B), SMALL30_IMAX, SMALL30_ALPHA, 0.0, early_stop=early))


@functools.lru_cache(maxsize=None)
def small30_fixed_ref(params=FIXED_PARAMS[0], early=True, B=SMALL30_B):
    H, layers = small30()
    return _frozen(fixed_decode(H, layers, quantise(small30_llr(B), params[3]), SMALL30_IMAX, *params[:3],
                                early_stop=early))
