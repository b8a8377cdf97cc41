"""Decode scripts of tests/test_gpu_callers.py: what one decoder handle is asked to decode, in order.

A script is a list of steps. A decode step is ``(kind, B, seed, early)``: ``kind`` names the family's input
generator ("noise": a batch the decoder never stops on, "conv": one it stops on before i_max - 1, "poison":
the float noise batch with +-inf entries), ``B`` the batch, ``seed`` the generator's seed, ``early`` the
early-stop argument. A setter step is ``("set", attribute, value)`` (``small_batch``, ``fold``). Generators are
deterministic, and the same family object generates the inputs of the CPU premise tests
(tests/test_cpu_callers.py) and of the GPU tests, and holds each step's oracle result (computed once per
distinct step, independently of every other step, read-only afterwards).

What the GPU tests rest on — noise steps never stop, conv steps stop inside the loop, a noise batch is at least
as wide as the converging batch after it — is asserted by tests/test_cpu_callers.py with the oracle alone, so
an edited seed cannot silently turn a stale-data test into a no-op.
"""
import functools

import numpy as np

from informationbottleneckdecodingldpc_amd import codes, graph, tables
from informationbottleneckdecodingldpc_amd.channel import UniformQuantizer, sigma2_from_ebn0
from oracle import oracle

MINSUM, BP = oracle.MINSUM, oracle.BP


def is_decode(step):
    return step[0] != "set"


def decode_steps(script):
    return [s for s in script if is_decode(s)]


def with_setters(script, setters):
    """`script` with ``("set", name, value)`` inserted ahead of decode step i (1-based) for every
    ``{i: (name, value)}`` of `setters`."""
    out, i = [], 0
    for s in script:
        if is_decode(s):
            i += 1
            if i in setters:
                out.append(("set",) + tuple(setters[i]))
        out.append(s)
    return out


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def llrs(g, B, ebn0, seed, quantised=True):
    """Channel LLRs of the all-zero codeword (tests/test_gpu_float.py `_llrs`): the 16-level quantiser's LLR
    alphabet, or (quantised=False) the unquantised 2 y / sigma^2 — doubles that float32 cannot represent."""
    q = UniformQuantizer(sigma2_from_ebn0(ebn0, g.R_c), 16)
    rng = np.random.default_rng(seed)
    if quantised:
        return q.llr_of(q.sample_all_zero(g.n_v, B, rng))
    y = 1.0 + np.sqrt(q.sigma_n2) * rng.standard_normal((g.n_v, B))
    return 2 * y / q.sigma_n2


# ---------------------------------------------------------------------------------------------- IB families
class IBFamily:
    """An IB decoder configuration (graph, tables, matching on) with its input generators and oracle."""

    def __init__(self, g, tb, q, max_batch):
        self.g, self.tb, self.q, self.max_batch = g, tb, q, max_batch
        self.imax = tb.imax
        self._inputs, self._refs = {}, {}

    def gen(self, kind, B, seed):
        """[N][B] int32 cluster ids. conv: the all-zero codeword through the family's channel; noise: random ids."""
        key = (kind, B, seed)
        if key not in self._inputs:
            rng = np.random.default_rng(seed)
            if kind == "conv":
                ch = self.q.sample_all_zero(self.g.n_v, B, rng).astype(np.int32)
            elif kind == "noise":
                ch = rng.integers(0, 16, (self.g.n_v, B)).astype(np.int32)
            else:
                raise ValueError(kind)
            self._inputs[key] = _frozen(ch)
        return self._inputs[key]

    def ref(self, step):
        """(oracle output int32 [N][B], oracle stop iteration) of one decode step."""
        kind, B, seed, early = step
        if step not in self._refs:
            out, it = oracle.ib_decode(self.g, self.tb, self.gen(kind, B, seed), match=True, early_stop=early,
                                       return_iters=True)
            self._refs[step] = (_frozen(out), it)
        return self._refs[step]


@functools.lru_cache(maxsize=None)
def _fold_H():
    return codes.dvbs2_structured(seed=3, n=7200, k=3600, groups_hi=4)


_FAMILIES = {}


def ib_wlan(wlan_H):
    """WLAN N = 1296: LLR tables of the 16-level uniform quantiser at 4.0 dB, i_max = 30, max_batch = 1030."""
    if "ib_wlan" not in _FAMILIES:
        g = graph.build_graph(wlan_H)
        q = UniformQuantizer(sigma2_from_ebn0(4.0, g.R_c), 16)
        _FAMILIES["ib_wlan"] = IBFamily(g, tables.llr_tables(q.output_LLRs, g.d_c_max, g.d_v_max, 30), q, 1030)
    return _FAMILIES["ib_wlan"]


def ib_fold():
    """The DVB-S2-shaped N = 7200 code of tests/test_gpu_ib_fold.py (3599 folded variables): tables at 9.0 dB,
    i_max = 12, max_batch = 260."""
    if "ib_fold" not in _FAMILIES:
        g = graph.build_graph(_fold_H())
        q = UniformQuantizer(sigma2_from_ebn0(9.0, g.R_c), 16)
        _FAMILIES["ib_fold"] = IBFamily(g, tables.llr_tables(q.output_LLRs, g.d_c_max, g.d_v_max, 12), q, 260)
    return _FAMILIES["ib_fold"]


def ib_evict(wlan_H):
    """WLAN N = 1296, random T = 16 tables, i_max = 3 (the captured-chain eviction script; noise inputs only)."""
    if "ib_evict" not in _FAMILIES:
        g = graph.build_graph(wlan_H)
        _FAMILIES["ib_evict"] = IBFamily(g, tables.random_tables(16, 16, g.d_c_max, g.d_v_max, 3, seed=21), None, 70)
    return _FAMILIES["ib_evict"]


def _conv(B, early=True):
    return ("conv", B, 100 + B, early)


def _noise(B):
    return ("noise", B, B, True)


# steps 1..10 of the WLAN reuse script: a wider, never-stopping batch ahead of every converging one, batches on
# both sides of the small-batch threshold (224), and early stop off / on again at one batch size
IB_WLAN_SCRIPT = [_noise(1030), _conv(1030), _conv(250), _noise(260), _conv(230), _conv(37), _conv(5),
                  _conv(37, early=False), _conv(37), _conv(1030)]
# the same steps with the small-batch threshold moved between them: 0 (per-pass kernels only), 1024 ahead of
# step 3 (B = 250 on the small kernels right after a per-pass decode), 0 ahead of step 7 (B = 5 on the fast
# kernels), the default 224 ahead of step 8
IB_WLAN_SCRIPT_THRESHOLDS = with_setters(IB_WLAN_SCRIPT, {1: ("small_batch", 0), 3: ("small_batch", 1024),
                                                          7: ("small_batch", 0), 8: ("small_batch", 224)})
# a fresh handle whose first decode of a batch size runs with early stop off: a converged IB batch decides the
# same saturated cluster ids after 10 iterations and after 29, so in the script above a chain with the wrong
# early-stop setting can only show in the stop iteration, and there only when the fixed-length chain came first
IB_WLAN_SCRIPT_OFF_FIRST = [_noise(40), _conv(37, early=False), _conv(37), _conv(5)]
# stop iterations the oracle gave when the scripts were written (asserted by tests/test_cpu_callers.py)
IB_WLAN_STOPS = {_noise(1030): 29, _conv(1030): 12, _conv(250): 16, _noise(260): 29, _conv(230): 11, _conv(37): 10,
                 _conv(5): 8, _noise(40): 29}

IB_FOLD_SCRIPT = [("noise", 260, 260, True), ("conv", 240, 240, True), ("set", "fold", False),
                  ("conv", 230, 230, True), ("set", "fold", True), ("conv", 230, 230, True),
                  ("conv", 33, 33, True), ("conv", 240, 240, True)]
IB_FOLD_STOPS = {("noise", 260, 260, True): 11, ("conv", 240, 240, True): 4, ("conv", 230, 230, True): 4,
                 ("conv", 33, 33, True): 3}

# 70 keys (B, early stop off) on one handle — more than the 64 captured chains a decoder keeps, so they are
# dropped once on the way — then the first keys again and one with early stop on
EVICT_BATCHES = list(range(1, 71))
IB_EVICT_SCRIPT = [("noise", B, B, False) for B in EVICT_BATCHES] + \
                  [("noise", B, B, False) for B in (1, 2, 3)] + [("noise", 70, 70, True)]
CHAIN_CACHE_BOUND = 64


# ------------------------------------------------------------------------------------------- float family
POISON_SHARE = 0.02      # share of +-inf entries of the poison step (raise it if the oracle ever stops on it)


class FloatFamily:
    """WLAN N = 1296 float decoders at one i_max: inputs (float64 arrays; the fp32 decoders get them rounded to
    float32) and the oracles of the three decoders that have one."""

    def __init__(self, g, imax, max_batch):
        self.g, self.imax, self.max_batch = g, imax, max_batch
        self._inputs, self._refs = {}, {}

    def gen(self, kind, B, seed):
        key = (kind, B, seed)
        if key not in self._inputs:
            if kind == "conv":
                x = llrs(self.g, B, 4.5, seed)
            elif kind == "noise":
                x = llrs(self.g, B, 0.5, seed)
            elif kind == "poison":      # the noise batch of the same seed, +-inf of random sign in POISON_SHARE of it
                x = llrs(self.g, B, 0.5, seed).copy()
                rng = np.random.default_rng(seed + 1000)
                pos = rng.random(x.shape) < POISON_SHARE
                x[pos] = np.where(rng.random(int(pos.sum())) < 0.5, np.inf, -np.inf)
            else:
                raise ValueError(kind)
            self._inputs[key] = _frozen(x)
        return self._inputs[key]

    def ref(self, step, kind, fp32):
        """(oracle APP LLRs as float64 [N][B], stop iteration) of one decode step for decoder `kind` in fp32
        (min-sum only: there is no fp32 BP oracle) or fp64."""
        key = (step, kind, fp32)
        if key not in self._refs:
            what, B, seed, early = step
            x = self.gen(what, B, seed)
            if fp32:
                assert kind == MINSUM
                out, it = oracle.float32_decode(self.g, self.imax, x.astype(np.float32), early_stop=early,
                                                return_iters=True)
                out = out.astype(np.float64)
            else:
                out, it = oracle.float_decode(self.g, kind, self.imax, x, early_stop=early, return_iters=True)
            self._refs[key] = (_frozen(out), it)
        return self._refs[key]


def float_wlan(wlan_H):
    """i_max = 20, max_batch = 132: the float reuse script's decoders."""
    if "float_wlan" not in _FAMILIES:
        _FAMILIES["float_wlan"] = FloatFamily(graph.build_graph(wlan_H), 20, 132)
    return _FAMILIES["float_wlan"]


def float_evict(wlan_H):
    """i_max = 3, max_batch = 70: the float captured-chain eviction script."""
    if "float_evict" not in _FAMILIES:
        _FAMILIES["float_evict"] = FloatFamily(graph.build_graph(wlan_H), 3, 70)
    return _FAMILIES["float_evict"]


def _fconv(B, early=True):
    return ("conv", B, 200 + B, early)


def _fnoise(B):
    return ("noise", B, 300 + B, True)


FLOAT_POISON = ("poison", 132, 300 + 132, True)
# steps 1..15; the setter steps apply to path="passes" handles only (the fused path ignores the threshold)
FLOAT_SCRIPT = [_fnoise(132), _fconv(130), _fnoise(72), _fconv(70), _fconv(37), _fconv(5),
                _fconv(37, early=False), _fconv(37), ("set", "small_batch", 0), _fconv(37), _fconv(5),
                ("set", "small_batch", 1024), _fconv(130), ("set", "small_batch", 64), _fconv(70)]
# min-sum handles: +-inf entries (legal for min-sum) in the widest batch, ahead of step 2
FLOAT_SCRIPT_MINSUM = FLOAT_SCRIPT[:1] + [FLOAT_POISON] + FLOAT_SCRIPT[1:]
# (step) -> (fp32 min-sum, fp64 min-sum, fp64 BP) oracle stop iterations when the script was written
FLOAT_STOPS = {_fconv(5): (7, 7, 7), _fconv(37): (8, 8, 8), _fconv(70): (10, 10, 8), _fconv(130): (9, 9, 8),
               _fnoise(72): (19, 19, 19), _fnoise(132): (19, 19, 19)}

FLOAT_EVICT_SCRIPT = [("noise", B, 300 + B, False) for B in EVICT_BATCHES] + \
                     [("noise", B, 300 + B, False) for B in (1, 2, 3)] + [("noise", 70, 370, True)]


# -------------------------------------------------------------------- dtype mixes and offsets (float, min-sum)
MIX_BATCHES = (3, 8, 70, 72)     # fp32 / fp64 words: ragged, whole (fused and small kernels); 70 / 72 per-pass
MIX_IMAX = 6
MIX_EARLY = dict(B=70, imax=20, ebn0=4.5, seed=270)      # the early-stop case: a converging unquantised batch


def mix_llrs(g, B, ebn0=1.5, seed=None):
    """Unquantised LLRs (float64, not float32-representable) of the dtype-mix and offset tests."""
    return _frozen(llrs(g, B, ebn0, 400 + B if seed is None else seed, quantised=False))


def mix_refs(g, x64, imax, early):
    """Oracle results for the four (decoder precision, LLR dtype) pairs fed the float64 array `x64` or its
    float32 rounding: {(fp32 decoder?, f32 input?): (APP LLRs float64, stop iteration)}. The fp32 decoder rounds
    a float64 input to nearest even (numpy's astype), the fp64 decoder widens a float32 input exactly."""
    x32 = x64.astype(np.float32)
    o32, it32 = oracle.float32_decode(g, imax, x32, early_stop=early, return_iters=True)
    o64, it64 = oracle.float_decode(g, MINSUM, imax, x64, early_stop=early, return_iters=True)
    o64w, it64w = oracle.float_decode(g, MINSUM, imax, x32.astype(np.float64), early_stop=early, return_iters=True)
    o32 = _frozen(o32.astype(np.float64))
    return {(True, True): (o32, it32), (True, False): (o32, it32),
            (False, False): (_frozen(o64), it64), (False, True): (_frozen(o64w), it64w)}
