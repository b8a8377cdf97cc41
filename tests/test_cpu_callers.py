"""Premises of the decode scripts of tests/_caller_scripts.py, checked with the oracle alone (no GPU).

tests/test_gpu_callers.py decodes these scripts on one decoder handle and expects every step to equal the
oracle although an earlier, wider and noisier batch left its data in the decoder's buffers. That only tests
anything while
  * a "noise" step really never stops (stop iteration == i_max - 1: every pass ran, every buffer and every
    syndrome flag of the handle was written),
  * a "conv" step really stops inside the loop (1 <= stop < i_max - 1: a stale unsatisfied check that leaked
    into the syndrome would delay or prevent the stop),
  * the noise batch is at least as wide as the converging batch after it (its columns lie beside the narrower
    batch's last word).
A later edit of a seed, an SNR or a batch size that breaks one of these fails here.
"""
import numpy as np
import pytest

from tests import _caller_scripts as cs


def _assert_widths(script):
    """Every noise / poison step is followed by a converging decode step that is not wider."""
    steps = cs.decode_steps(script)
    seen = 0
    for i, s in enumerate(steps):
        if s[0] == "conv":
            continue
        nxt = next((t for t in steps[i + 1:] if t[0] == "conv"), None)
        assert nxt is not None and nxt[1] <= s[1], (s, nxt)
        seen += 1
    assert seen >= 1


def _assert_ib_premises(fam, script, stops):
    _assert_widths(script)
    for step in sorted(set(cs.decode_steps(script))):
        kind, B, seed, early = step
        assert B <= fam.max_batch
        if not early:                       # a fixed-length decode: judged on the same batch with early stop on
            assert (kind, B, seed, True) in script
            continue
        _, it = fam.ref(step)
        if kind == "noise":
            assert it == fam.imax - 1, (step, it)
        else:
            assert 1 <= it < fam.imax - 1, (step, it)
        assert it == stops[step], (step, it)


def test_ib_wlan_script_premises(wlan_H):
    fam = cs.ib_wlan(wlan_H)
    _assert_ib_premises(fam, cs.IB_WLAN_SCRIPT, cs.IB_WLAN_STOPS)
    _assert_ib_premises(fam, cs.IB_WLAN_SCRIPT_OFF_FIRST, cs.IB_WLAN_STOPS)
    assert cs.decode_steps(cs.IB_WLAN_SCRIPT_OFF_FIRST)[1:3] == [("conv", 37, 137, False), ("conv", 37, 137, True)]
    # the threshold variant decodes the same steps in the same order
    assert cs.decode_steps(cs.IB_WLAN_SCRIPT_THRESHOLDS) == cs.IB_WLAN_SCRIPT
    assert [s[2] for s in cs.IB_WLAN_SCRIPT_THRESHOLDS if not cs.is_decode(s)] == [0, 1024, 0, 224]
    # early stop off and on again at one batch size, after a decode of it with early stop on
    i = cs.IB_WLAN_SCRIPT.index(("conv", 37, 137, False))
    assert ("conv", 37, 137, True) in cs.IB_WLAN_SCRIPT[:i] and cs.IB_WLAN_SCRIPT[i + 1] == ("conv", 37, 137, True)


def test_ib_fold_script_premises():
    fam = cs.ib_fold()
    _assert_ib_premises(fam, cs.IB_FOLD_SCRIPT, cs.IB_FOLD_STOPS)
    n2 = int((np.asarray(fam.g.vn_deg) == 2).sum())
    assert n2 == 3599                       # every one of them folds (asserted on the device handle)
    assert [s[1:] for s in cs.IB_FOLD_SCRIPT if not cs.is_decode(s)] == [("fold", False), ("fold", True)]


@pytest.mark.parametrize("script", ["ib", "float"])
def test_eviction_script_premises(script):
    sc = cs.IB_EVICT_SCRIPT if script == "ib" else cs.FLOAT_EVICT_SCRIPT
    keys = [(s[1], s[3]) for s in sc]
    first = keys[:len(cs.EVICT_BATCHES)]
    assert len(set(first)) == len(first) > cs.CHAIN_CACHE_BOUND       # the bound is passed on the way
    assert all(not e for _, e in first)
    assert keys[len(first):] == [(1, False), (2, False), (3, False), (70, True)]   # dropped keys come back


def test_float_script_premises(wlan_H):
    fam = cs.float_wlan(wlan_H)
    _assert_widths(cs.FLOAT_SCRIPT)
    _assert_widths(cs.FLOAT_SCRIPT_MINSUM)
    assert cs.decode_steps(cs.FLOAT_SCRIPT_MINSUM)[1] == cs.FLOAT_POISON
    for step in sorted(set(cs.decode_steps(cs.FLOAT_SCRIPT))):
        kind, B, seed, early = step
        assert B <= fam.max_batch
        if not early:
            assert (kind, B, seed, True) in cs.FLOAT_SCRIPT
            continue
        its = (fam.ref(step, cs.MINSUM, True)[1], fam.ref(step, cs.MINSUM, False)[1], fam.ref(step, cs.BP, False)[1])
        for it in its:
            if kind == "noise":
                assert it == fam.imax - 1, (step, its)
            else:
                assert 1 <= it < fam.imax - 1, (step, its)
        assert its == cs.FLOAT_STOPS[step], (step, its)
    # the poison step: +-inf entries present in both signs, and the oracle never stops on it
    x = fam.gen(*cs.FLOAT_POISON[:3])
    assert np.isposinf(x).sum() > 0 and np.isneginf(x).sum() > 0 and not np.isnan(x).any()
    assert abs(np.isinf(x).mean() - cs.POISON_SHARE) < 0.25 * cs.POISON_SHARE
    for fp32 in (True, False):
        out, it = fam.ref(cs.FLOAT_POISON, cs.MINSUM, fp32)
        assert it == fam.imax - 1, (fp32, it)
        assert not np.isnan(out).any()


def test_dtype_mix_premises(wlan_H):
    """The dtype-mix inputs are not float32-representable (so the conversion is visible in the result: the
    fp64 decoder's output differs between the float64 input and its float32 rounding), and the early-stop case
    converges for every (precision, input dtype) pair."""
    g = cs.float_wlan(wlan_H).g
    x = cs.mix_llrs(g, 8)
    assert (x.astype(np.float32).astype(np.float64) != x).mean() > 0.99
    refs = cs.mix_refs(g, x, cs.MIX_IMAX, False)
    assert (refs[(False, False)][0] != refs[(False, True)][0]).any()
    assert (refs[(False, False)][0].astype(np.float32) != refs[(True, False)][0].astype(np.float32)).any()
    e = cs.MIX_EARLY
    refs = cs.mix_refs(g, cs.mix_llrs(g, e["B"], e["ebn0"], e["seed"]), e["imax"], True)
    for key, (_, it) in refs.items():
        assert 1 <= it < e["imax"] - 1, (key, it)
