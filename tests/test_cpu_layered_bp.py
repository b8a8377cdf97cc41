"""CPU: the layered BP decoder's specification and host side (include/ibldpc.h "Layered BP") — the numpy
restatement against an independent scalar one, its float32 form against its float64 form, the instability of the
min-sum clamp rule that the specification avoids, the named inputs of the GPU tests and the premises of
tests/test_gpu_layered_bp_edges.py (nonzero codewords with a spread of stops, what the all-zero inputs cannot see,
the two clamps, exact ties), the new C ABI names, the
drop-in class's refusals, the host plan under AddressSanitizer / UndefinedBehaviorSanitizer as a stand-alone program
(tests/asan/layered_bp_plan_check.cpp; nothing loaded into Python is sanitized), and the private segments of the
new kernels in the built code object."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

from informationbottleneckdecodingldpc_amd import codes
from tests import _layered_bp_ref as br
from tests import _layered_census as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


small_dvbs2 = br.small_dvbs2


# ---------------------------------------------------------------------------------------------------------------
# an independent scalar restatement: per codeword, per check, leave-one-out folds of the other inputs in fp64
# ---------------------------------------------------------------------------------------------------------------
def _boxplus_scalar(a, b, L):
    import math
    aa, ab = abs(a), abs(b)
    mag = min(aa, ab) + math.log1p(math.exp(-(aa + ab))) - math.log1p(math.exp(-abs(aa - ab)))
    mag = min(max(mag, 0.0), L)
    return -mag if (a < 0) != (b < 0) else mag


def layered_bp_scalar(H, layers, llr, imax, llr_max):
    A = sp.csr_matrix(H)
    A.sort_indices()
    rows = [[int(v) for v in A.indices[A.indptr[c]:A.indptr[c + 1]]] for c in range(A.shape[0])]
    L = float(np.float32(llr_max))
    n, B = llr.shape
    out = np.empty((n, B))
    for b in range(B):
        P = [float(x) for x in llr[:, b]]
        R = [[0.0] * len(r) for r in rows]
        for _ in range(imax):
            for layer in layers:
                for c in layer:
                    vs, Rc = rows[int(c)], R[int(c)]
                    q = [P[v] - Rc[k] for k, v in enumerate(vs)]
                    for k, v in enumerate(vs):
                        others = [q[j] for j in range(len(vs)) if j != k]
                        t = others[0]
                        for x in others[1:]:
                            t = _boxplus_scalar(x, t, L)
                        t = min(max(t, -L), L)
                        Rc[k] = t
                        P[v] = q[k] + t
        out[:, b] = P
    return out


def test_restatement_equals_the_scalar_one():
    """The vectorised forward-backward restatement against plain loops with leave-one-out folds (another order of
    an associative operation: equal up to fp64 rounding), on every degree 2..16."""
    H, layers = lc.mixed()
    llr = lc.awgn_llr(H.shape[1], 4, 2.0, seed=3, R=1.0 - H.shape[0] / H.shape[1])
    ref, _ = br.layered_bp_decode(H, layers, llr, 3, early_stop=False, dtype=np.float64)
    sc = layered_bp_scalar(H, layers, llr, 3, 150.0)
    assert np.abs(ref - sc).max() <= 1e-9


# ---------------------------------------------------------------------------------------------------------------
# the named inputs of the GPU tests: shared with tests/test_gpu_layered_bp.py
# ---------------------------------------------------------------------------------------------------------------
dvb_input, wlan_input, dvb_reference, wlan_reference = br.dvb_input, br.wlan_input, br.dvb_reference, br.wlan_reference


@pytest.mark.parametrize("which,imax", [("dvb", 10), ("wlan81", 20), ("wlan27_2.5dB", 20)])
def test_float32_form_is_within_h5_of_the_float64_form(which, imax):
    """On the two stop-test inputs and on the input of the instability finding (llr_max 150, where all 64 codewords
    converge). A codeword that does NOT converge amplifies rounding differences from iteration to iteration: on WLAN
    Z = 27 at 1.5 dB, awgn_llr(648, 32, 1.5, seed=7), the codewords 5, 20 and 26 leave H5 from iterations 13, 14 and
    15 on (relative differences up to 0.3), every converged one stays inside."""
    if which == "dvb":
        H, layers, llr = dvb_input()
    elif which == "wlan27_2.5dB":
        H, layers = lc.wlan(27)
        llr = lc.awgn_llr(648, 64, 2.5, seed=7)
    else:
        H, layers, llr = wlan_input(int(which[4:]))
    r64, _ = br.layered_bp_decode(H, layers, llr, imax, early_stop=False, dtype=np.float64)
    r32, _ = br.layered_bp_decode(H, layers, llr, imax, early_stop=False, dtype=np.float32)
    assert r32.dtype == np.float32
    bad = br.h5_violations(r32, r64)
    assert not bad.any(), (int(bad.sum()), float(np.abs(r32 - r64).max()))


def test_clamping_q_is_unstable_and_the_specified_rule_is_not():
    """WLAN Z = 27 at 2.5 dB, llr_max 30, 12 iterations: the specified rule (Q not clamped) leaves all 64 codewords
    with a zero syndrome; the layered min-sum rule, Q = clamp(P - R), does not (it left none)."""
    H, layers = lc.wlan(27)
    A = sp.csr_matrix(H)
    llr = lc.awgn_llr(648, 64, 2.5, seed=7)

    def clean(P):
        return int((((A @ (P < 0).astype(np.int32)) % 2) == 0).all(axis=0).sum())

    good, _ = br.layered_bp_decode(H, layers, llr, 12, llr_max=30.0, early_stop=False)
    bad, _ = br.layered_bp_decode(H, layers, llr, 12, llr_max=30.0, early_stop=False, clamp_q=True)
    assert clean(good) == 64
    assert clean(bad) < 64
    print("clamped-Q variant: zero syndromes", clean(bad), "of 64")


def test_named_inputs_meet_their_conditions():
    _, it_d, exc_d = dvb_reference(10, True)
    H, layers, llr = dvb_input()
    A = sp.csr_matrix(H)
    out_d = dvb_reference(10, True)[0]
    unconverged = int((((A @ (out_d < 0).astype(np.int32)) % 2) != 0).any(axis=0).sum())
    print("dvb: stops", sorted(set(it_d.tolist())), "unconverged", unconverged, "excusable", int(exc_d.sum()))
    assert len(set(it_d.tolist())) >= 4 and unconverged >= 1
    assert int(exc_d.sum()) <= br.excuse_cap(130)
    _, it_w, exc_w = wlan_reference(81, 20, True)
    print("wlan81: stops", sorted(set(it_w.tolist())), "excusable", int(exc_w.sum()))
    assert int(exc_w.sum()) <= br.excuse_cap(32)
    _, _, exc_w27 = wlan_reference(27, 20, True)
    assert int(exc_w27.sum()) <= br.excuse_cap(32)


# ---------------------------------------------------------------------------------------------------------------
# the premises of tests/test_gpu_layered_bp_edges.py
# ---------------------------------------------------------------------------------------------------------------
# iterations of the float64 reference on tests/_codewords.py layered_input(name), B = 130, i_max 8, llr_max 150
SPREAD_HIST = {"wlan": [0, 63, 39, 13, 3, 3, 1, 0, 8], "mixed": [0, 84, 21, 6, 4, 3, 0, 1, 11],
               "dvb": [0, 2, 92, 6, 21, 1, 0, 0, 8]}
SPREAD_CONVERGED = {"wlan": 122, "mixed": 119, "dvb": 122}


def _findings(label, res, ref):
    print(f"{label}: H5 violations {int(res['bad'].sum())} in columns "
          f"{np.flatnonzero(res['bad'].any(axis=0)).tolist()}, "
          f"hard flips {res['flips']}, iters differ at {np.flatnonzero(res['differ']).tolist()} (excusable "
          f"{np.flatnonzero(ref[2]).tolist()}), reference iters {np.bincount(ref[1]).tolist()}")


@pytest.mark.parametrize("name", ["wlan", "mixed", "dvb"])
def test_spread_batches(name):
    """br.spread_input: nonzero codewords at two noise levels, the all-zero codeword and sign-random noise
    (tests/_codewords.py layered_input; on wlan the noise columns at half magnitude, see
    test_spread_inputs_bear_one_ulp_transcendentals), B = 130: the float64 reference stops at four or more distinct
    iterations, never stops a noise column and decides the transmitted bits on every column it converges. The float32 form against it under
    br.compare_columns: no value outside H5, no hard flip, iters unequal on excusable columns only and within the
    cap of 3 (measured: 0, 1 and 0 columns on wlan, mixed and dvb). On mixed that one column (1) stops an iteration
    apart; against the reference's FROZEN values it shows 398 entries outside H5, which is why compare_columns
    takes the reference's values at the decoder's own stop iteration."""
    from tests import _codewords as cw
    H, _, layers, _ = cw.code(name)
    llr, bits, kinds = br.spread_input(name)
    ref = br.spread_reference(name)
    out, it, exc, P_at, conv = ref
    imax = cw.IMAX_LAYERED
    same = np.array_equal(llr, cw.layered_input(name)[0])
    assert same == (name != "wlan") and np.array_equal(llr[:, kinds != cw.KIND_NOISE],
                                                       cw.layered_input(name)[0][:, kinds != cw.KIND_NOISE])
    assert imax == 8 and P_at.shape == (imax,) + llr.shape and llr.shape[1] == 130
    if not same:       # the stops are those of layered_input as it is: its noise columns never stop either
        assert np.array_equal(br.layered_bp_decode(H, layers, cw.layered_input(name)[0], imax)[1], it)
    hist = np.bincount(it, minlength=imax + 1).tolist()
    print(f"{name}: reference iters {hist}, converged {int(conv.sum())}, excusable {np.flatnonzero(exc).tolist()}")
    assert hist == SPREAD_HIST[name] and int(conv.sum()) == SPREAD_CONVERGED[name]
    assert len(set(it[conv].tolist())) >= 4
    assert (kinds == cw.KIND_NOISE).sum() == 8 and (it[kinds == cw.KIND_NOISE] == imax).all()
    assert not conv[kinds == cw.KIND_NOISE].any()
    assert np.array_equal((out < 0)[:, conv], (bits == 1)[:, conv])
    assert bits[:, conv].any(axis=0).sum() >= 100          # nonzero codewords among the converged
    # the recorded values are the frozen ones at each column's stop iteration
    assert all(np.array_equal(P_at[it[b] - 1][:, b], out[:, b]) for b in range(130))
    # odd tiles hold early stoppers only: whole-tile skips beside running tiles
    assert (it[64:128] <= 4).all() and (it[:64] == imax).any()
    o32, i32 = br.layered_bp_decode(H, layers, llr, imax, dtype=np.float32)
    res = br.compare_columns(o32, i32, ref)
    _findings(f"{name} float32 form", res, ref)
    assert not res["bad"].any() and res["flips"] == 0 and not res["unexcused"].any()
    assert res["excused"] <= br.excuse_cap(130) == 3
    if name == "mixed":
        assert np.flatnonzero(res["differ"]).tolist() == [1]
        frozen = br.h5_violations(o32, out)
        assert frozen[:, 1].sum() > 100 and not np.delete(frozen, 1, axis=1).any()


def _worst_share_of_h5(x, ref):
    """max over the rows of |x - ref| / (H5's bound), per column."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return (np.abs(x - ref) / (br.REL * np.maximum(np.abs(x), np.abs(ref)) + br.TOL_ABS)).max(axis=0)


@pytest.mark.parametrize("name,draws", [("wlan", 4), ("mixed", 2), ("dvb", 1)])
def test_spread_inputs_bear_one_ulp_transcendentals(name, draws):
    """Whether an input can be held to H5 on EVERY column for 8 iterations is a property of the input: the float32
    form with each transcendental moved by up to 1 ulp at random (br.one_ulp: the hardware's exp2 and log2 are good
    to about 1 ulp, numpy's are not the only legitimate ones) must stay well inside H5, stop off, i_max 8. It stays
    below 0.7 of the bound on br.spread_input (measured: wlan 0.10, mixed 0.25, dvb 0.52; the noise columns 0.02,
    0.07, 0.52). On tests/_codewords.py layered_input("wlan") as it is it does not: the noise columns, which never
    converge, double a rounding difference every iteration and leave H5 by iteration 8 (draws 0 and 1: 1.44 and
    1.34 times the bound; an MI355X: 1.24 times, on column 43), every other column stays at 0.1 of it or below.
    That is why spread_input halves those columns on wlan (seed and Eb/N0 are unchanged)."""
    from tests import _codewords as cw
    H, _, layers, _ = cw.code(name)
    llr, _, kinds = br.spread_input(name)
    noise = kinds == cw.KIND_NOISE
    want = br.layered_bp_decode(H, layers, llr, cw.IMAX_LAYERED, early_stop=False)[0]
    for draw in range(draws):
        got = br.layered_bp_decode(H, layers, llr, cw.IMAX_LAYERED, early_stop=False, dtype=np.float32,
                                   ulp=br.one_ulp(np.random.default_rng(draw)))[0]
        share = _worst_share_of_h5(got, want)
        print(f"{name} draw {draw}: worst share of H5's bound {share.max():.2f}, on the noise columns "
              f"{share[noise].max():.2f}")
        assert share.max() < 0.7
    if name == "wlan":
        assert (share[noise] < 0.05).all()
        full = cw.layered_input("wlan")[0]
        want = br.layered_bp_decode(H, layers, full, cw.IMAX_LAYERED, early_stop=False)[0]
        for draw in range(2):
            got = br.layered_bp_decode(H, layers, full, cw.IMAX_LAYERED, early_stop=False, dtype=np.float32,
                                       ulp=br.one_ulp(np.random.default_rng(draw)))[0]
            share = _worst_share_of_h5(got, want)
            print(f"layered_input(wlan) draw {draw}: noise columns {np.round(share[noise], 2).tolist()}, others "
                  f"{share[~noise].max():.2f}")
            assert share[noise].max() > 1.0 and share[~noise].max() < 0.15


def test_compare_columns_rule():
    """A decoder that is the reference itself passes; one column moved to another iteration's values passes only
    when that column is excusable and its iters says so; a non-excusable column is judged against the frozen
    values whatever its iters."""
    out, it, exc, P_at, _ = br.spread_reference("mixed")
    ref = (out, it, exc, P_at)
    res = br.compare_columns(out, it, ref)
    assert not res["bad"].any() and res["flips"] == 0 and not res["differ"].any() and res["excused"] == 0
    b = int(np.flatnonzero(exc)[0])
    other = int(it[b]) - 1 if it[b] == 8 else int(it[b]) + 1
    o2, i2 = out.copy(), it.copy()
    o2[:, b], i2[b] = P_at[other - 1][:, b], other
    res = br.compare_columns(o2, i2, ref)
    assert not res["bad"].any() and res["excused"] == 1 and not res["unexcused"].any()
    res = br.compare_columns(o2, it, ref)                      # the values moved, iters does not say so
    assert res["bad"][:, b].any() and not res["differ"].any()
    res = br.compare_columns(out, i2, ref)                     # iters moved, the values did not
    assert res["bad"][:, b].any()
    c = int(np.flatnonzero(~exc & (it < 7))[0])
    o3, i3 = out.copy(), it.copy()
    o3[:, c], i3[c] = P_at[it[c]][:, c], it[c] + 1
    res = br.compare_columns(o3, i3, ref)
    assert res["unexcused"][c] and res["bad"][:, c].any()
    assert np.array_equal(br.reference_for_columns(i3, (out, it, exc)), out)     # without P_at: as before


@pytest.mark.parametrize("rule", br.WRONG_STOP_RULES)
def test_wrong_stop_rules_pass_all_zero_and_fail_on_the_spread_batch(rule):
    """The reference with a wrong stop rule ("no decision is 1"; the syndrome gathered through variable v - 1): on
    the all-zero inputs of tests/test_gpu_layered_bp.py, wlan_input(27) at i_max 20 and dvb_input() at i_max 10,
    its iteration counts are those of the true rule, so no test on those inputs would notice; on the spread batch
    of the WLAN code (and of mixed) they differ on columns that are not excusable: every nonzero codeword the
    reference converges before i_max (measured: 114 of 130 on wlan, 111 on mixed, for both rules)."""
    from tests import _codewords as cw
    zero_inputs = (("wlan_input(27)", wlan_input(27), 20, wlan_reference(27, 20, True)[1]),
                   ("dvb_input()", dvb_input(), 10, dvb_reference(10, True)[1]))
    for what, (H, layers, llr), imax, true_it in zero_inputs:
        _, wrong_it = br.layered_bp_decode(H, layers, llr, imax, stop_rule=rule)
        print(f"{rule.__name__} on {what}: {np.bincount(wrong_it).tolist()} (true rule "
              f"{np.bincount(true_it).tolist()})")
        assert len(set(true_it.tolist())) >= 4 and np.array_equal(wrong_it, true_it)
    for name in ("wlan", "mixed"):
        H, _, layers, _ = cw.code(name)
        llr, bits, kinds = br.spread_input(name)
        _, it, exc, _, conv = br.spread_reference(name)
        _, wrong_it = br.layered_bp_decode(H, layers, llr, cw.IMAX_LAYERED, stop_rule=rule)
        differ = wrong_it != it
        print(f"{rule.__name__} on layered_input({name}): {int(differ.sum())} of 130 counts differ, "
              f"{int((differ & ~exc).sum())} of them not excusable")
        nonzero = bits.any(axis=0) & cw.converged(it)
        assert (differ & ~exc).sum() >= 1 and differ[nonzero].all() and nonzero.sum() >= 100
        assert np.array_equal(wrong_it[kinds == cw.KIND_ZERO], it[kinds == cw.KIND_ZERO])


def _clamp_census(H, layers, llr, imax, L):
    """Instruments the reference: per check update of a running codeword, in iterations that are run."""
    n = dict(deg2_beyond=0, two_beyond=0)

    def seen(it, Q, done):
        beyond = (np.abs(Q) > L)[:, :, ~done]
        if Q.shape[1] == 2:
            n["deg2_beyond"] += int(beyond.any(axis=1).sum())
        else:
            n["two_beyond"] += int((beyond.sum(axis=1) >= 2).sum())

    br.layered_bp_decode(H, layers, llr, imax, llr_max=L, check_hook=seen)
    return n


@pytest.mark.parametrize("name", ["mixed", "wlan"])
def test_saturating_input_meets_both_clamps(name):
    """br.saturating_input (seed 22, 3 dB: nothing had to be changed to meet the premises). Counted in the
    reference: a degree-2 check with |Q| > llr_max (mixed; the WLAN code has no check of degree 2) and a check of
    degree >= 3 with two |Q| > llr_max, on running codewords. The reference without the degree-2 clamp, and
    separately without the box-plus's upper clamp, leaves H5 on a column the true reference converges (measured:
    on all 15 of them). The reference converges 15 of 16 columns at a spread of stops and decides their bits; the
    float32 form is within H5 with no flip on those, finite everywhere, and within H5 on every column after one
    iteration — also when the huge entries take random signs. Two entries of 2^126 in one box-plus leave
    (|a| + |b|) log2(e) = 2.45e38 finite; "overflow" is the same input with 2^127 for 2^126, still inside the
    precondition, where |a| + |b| is inf in fp32: same stops, same bars."""
    H, layers, C = br.edge_code(name)
    llr = br.saturating_input(name)
    assert (np.abs(llr) == br.HUGE).sum() >= 64 and (np.abs(llr) == 150).sum() >= 64
    assert float(br.HUGE) + 16 * 150.0 < np.finfo(np.float32).max
    assert float(br.HUGE_INF) + 16 * 150.0 < np.finfo(np.float32).max
    with np.errstate(over="ignore"):
        assert np.isfinite((br.HUGE + br.HUGE) * np.float32(1.4426950408889634)) and np.isinf(br.HUGE_INF + br.HUGE_INF)
    out, it, exc, _, conv = br.edge_reference("saturating", name, br.EDGE_IMAX, True)
    census = _clamp_census(H, layers, llr, br.EDGE_IMAX, 150.0)
    print(f"{name} saturating: reference iters {np.bincount(it).tolist()}, converged {int(conv.sum())} of 16, "
          f"excusable {np.flatnonzero(exc).tolist()}, {census}")
    assert int(conv.sum()) == 15 and len(set(it[conv].tolist())) >= 3
    assert np.array_equal((out < 0)[:, conv], (C == 1)[:, conv])
    assert census["two_beyond"] > 0
    variants = [dict(clamp_boxplus=False)]
    if name == "mixed":
        assert census["deg2_beyond"] > 0
        variants.append(dict(clamp_deg2=False))
    else:
        assert 2 not in np.diff(sp.csr_matrix(H).indptr)
    for kw in variants:
        v_out, _ = br.layered_bp_decode(H, layers, llr, br.EDGE_IMAX, **kw)
        hit = br.h5_violations(v_out, out).any(axis=0) & conv
        print(f"   {kw}: outside H5 on converged columns {np.flatnonzero(hit).tolist()}")
        assert hit.any()
    for kind in ("saturating", "overflow"):
        x = br.edge_input(kind, name)
        k_out, k_it, _, _, k_conv = br.edge_reference(kind, name, br.EDGE_IMAX, True)
        assert int(k_conv.sum()) == 15 and np.array_equal(k_it, it)
        o32, i32 = br.layered_bp_decode(H, layers, x, br.EDGE_IMAX, dtype=np.float32)
        assert np.isfinite(o32).all() and np.array_equal(i32, k_it)
        assert not br.h5_violations(o32, k_out)[:, k_conv].any()
        assert not ((o32 < 0) != (k_out < 0))[:, k_conv].any()
    for kind in ("saturating", "overflow", "frustrated"):
        first = br.edge_reference(kind, name, 1, True)
        o1, i1 = br.layered_bp_decode(H, layers, br.edge_input(kind, name), 1, dtype=np.float32)
        res = br.compare_columns(o1, i1, first)
        assert not res["bad"].any() and res["flips"] == 0 and not res["differ"].any()
    huge = np.abs(llr) == br.HUGE
    signs = np.sign(br.saturating_input(name, True))[huge] * np.where(C == 1, -1, 1)[huge]
    assert (signs < 0).sum() >= 16 and (signs > 0).sum() >= 16


def test_small_llr_max_and_quantised_inputs():
    """br.small_llr_max_input (mixed, 2 dB, llr_max 7.5): the reference stops at several iterations and the float32
    form is within the bars on every column. br.quantised_input: zeros of either sign; with the stop on every
    column of mixed is excusable (iters unconstrained), so the GPU test runs it with the stop off."""
    H, layers, C = br.edge_code("mixed")
    ref = br.edge_reference("small_llr_max", "mixed", br.EDGE_IMAX, True, br.SMALL_LLR_MAX)
    out, it, exc, _, conv = ref
    print(f"small llr_max: reference iters {np.bincount(it).tolist()}, converged {np.flatnonzero(conv).tolist()}, "
          f"excusable {np.flatnonzero(exc).tolist()}")
    assert len(set(it[conv].tolist())) >= 3 and 1 <= (~conv).sum() and np.abs(out).max() > br.SMALL_LLR_MAX
    assert np.array_equal((out < 0)[:, conv], (C == 1)[:, conv])
    o32, i32 = br.layered_bp_decode(H, layers, br.small_llr_max_input(), br.EDGE_IMAX, llr_max=br.SMALL_LLR_MAX,
                                    dtype=np.float32)
    res = br.compare_columns(o32, i32, ref)
    assert not res["bad"].any() and res["flips"] == 0 and not res["unexcused"].any() and res["excused"] <= 1
    for name in ("mixed", "wlan"):
        q = br.quantised_input(name)
        assert (np.signbit(q) & (q == 0)).sum() >= 100 and (~np.signbit(q) & (q == 0)).sum() >= 100
        assert np.array_equal(q, np.rint(q))
        on = br.edge_reference("quantised", name, br.EDGE_IMAX, True)
        off = br.edge_reference("quantised", name, br.EDGE_IMAX, False)
        print(f"quantised {name}: excusable with the stop on {int(on[2].sum())} of 16")
        assert not off[2].any() and (off[1] == br.EDGE_IMAX).all()
        o32, i32 = br.layered_bp_decode(*br.edge_code(name)[:2], q, br.EDGE_IMAX, early_stop=False, dtype=np.float32)
        res = br.compare_columns(o32, i32, off)
        assert not res["bad"].any() and not res["differ"].any()
    assert br.edge_reference("quantised", "mixed", br.EDGE_IMAX, True)[2].all()


def test_ties_in_the_first_iteration():
    """The WLAN spread batch's LLRs are 16 levels at either noise level, their halves on the noise columns, and
    their negatives: box-pluses of iteration 1 meet |a| == |b| exactly (counted in the reference), and so do those
    of the quantised inputs."""
    from tests import _codewords as cw
    H, _, layers, _ = cw.code("wlan")
    llr, _, kinds = br.spread_input("wlan")
    assert np.unique(np.abs(llr[:, kinds != cw.KIND_NOISE])).size <= 32
    for what, x, Hc, lay in (("wlan spread", llr, H, layers),
                             ("quantised mixed", br.quantised_input("mixed"), *br.edge_code("mixed")[:2])):
        n = dict(ties=0, nonzero_ties=0, boxplus=0)

        def seen(it, Q, done):
            if it != 1 or Q.shape[1] == 2:
                return None

            def on(a, b):
                tie = np.abs(a) == np.abs(b)
                n["ties"] += int(tie.sum())
                n["nonzero_ties"] += int((tie & (a != 0)).sum())
                n["boxplus"] += tie.size
            return on

        br.layered_bp_decode(Hc, lay, x, 1, check_hook=seen)
        print(f"{what}: {n}")
        assert n["nonzero_ties"] >= 1 and n["boxplus"] > n["ties"]


# ---------------------------------------------------------------------------------------------------------------
# the library's new names
# ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_and_prototypes():
    from informationbottleneckdecodingldpc_amd import _build, _lib
    assert {"ibl_layered_create_bp", "ibl_layered_is_bp"} <= set(_lib.EXPORTS)
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    L = _lib.load()
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    assert list(L.ibl_layered_create_bp.argtypes[:2]) == [vp, i32]
    assert list(L.ibl_layered_create_bp.argtypes[4:9]) == [i32, f32, i32, i32, i32]
    assert len(L.ibl_layered_create_bp.argtypes) == 10
    assert L.ibl_layered_is_bp.argtypes[0] is vp
    with open(os.path.join(ROOT, "include", "ibldpc.h")) as fh:
        header = fh.read()
    proto = ("int ibl_layered_create_bp(const ibl_graph* g, int32_t n_layers, const int32_t* layer_ptr, "
             "const int32_t* layer_checks, int32_t imax, float llr_max, int32_t precision, int32_t max_batch, "
             "int32_t path, ibl_layered** out);")
    assert proto in " ".join(header.split())
    assert "int ibl_layered_is_bp(const ibl_layered* h, int32_t* bp);" in header
    assert "Layered BP:" in header and "layered BP are not built" not in header
    # host-only refusals: NULL arguments need no device
    bp = i32(7)
    assert L.ibl_layered_is_bp(None, ctypes.byref(bp)) == _lib.IBL_EINVAL
    h = vp()
    ptr = np.zeros(2, np.int32)
    assert L.ibl_layered_create_bp(None, 1, ptr, ptr, 5, 150.0, _lib.IBL_F32, 4, _lib.IBL_PATH_AUTO,
                                   ctypes.byref(h)) == _lib.IBL_EINVAL
    assert b"graph is NULL" in L.ibl_last_error()


def test_dropin_class_refusals():
    from informationbottleneckdecodingldpc_amd import BeliefPropagation_Layered_Decoder_class_irregular as Cls
    from informationbottleneckdecodingldpc_amd import ber
    from informationbottleneckdecodingldpc_amd.min_sum_layered_decoder_irreg import \
        Min_Sum_Layered_Decoder_class_irregular
    H, layers = lc.wlan(27)
    d = Cls(H, 10, 16, 4, Z=27, path="auto")
    assert isinstance(d, Min_Sum_Layered_Decoder_class_irregular)
    assert d.data_len == 324 and len(d.layers) == 12 and d.llr_max == 150.0 and d.last_iterations is None
    assert ber.decoder_kind(d) == "bp"
    assert hasattr(d, "decode_OpenCL_belief_propagation") and not hasattr(d, "decode_OpenCL_min_sum")
    assert d._DECODER_NAME == "layered BP"
    with pytest.raises(AttributeError):
        d.decode_OpenCL_min_sum(np.zeros((648, 1), np.float32))
    for kw in (dict(alpha=0.75), dict(beta=0.5), dict(fixed=True), dict(compact=True), dict(compact=(2, 25))):
        with pytest.raises(ValueError, match=next(iter(kw))):
            Cls(H, 10, 16, 4, Z=27, **kw)
    with pytest.raises(ValueError, match="path"):
        Cls(H, 10, 16, 4, Z=27, path="onchip")
    with pytest.raises(ValueError, match="not both"):
        Cls(H, 10, 16, 4, Z=27, layers=layers)


# ---------------------------------------------------------------------------------------------------------------
# host plan under the sanitizers
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bp_plan_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("asan") / "layered_bp_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "informationbottleneckdecodingldpc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "asan", "layered_bp_plan_check.cpp"), "-o", exe], check=True)
    return exe


def run_plan(exe, H, layers, max_batch, tmp_path):
    A = codes.canonical_csr(H)
    f = tmp_path / "g.bin"
    with open(f, "wb") as fh:
        np.array([A.shape[1], A.shape[0]], np.int32).tofile(fh)
        A.indptr.astype(np.int32).tofile(fh)
        A.indices.astype(np.int32).tofile(fh)
        np.array([len(layers)], np.int32).tofile(fh)
        np.concatenate([[0], np.cumsum([len(l) for l in layers])]).astype(np.int32).tofile(fh)
        np.concatenate([np.asarray(l, np.int32) for l in layers]).astype(np.int32).tofile(fh)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(f), str(max_batch)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout)
    assert out["failures"] == 0
    return out


@pytest.mark.parametrize("name,max_batch", [("dvbs2_small", 130), ("wlan27", 64), ("wlan81", 65), ("mixed", 9)])
def test_bp_plan_under_sanitizers(bp_plan_check, tmp_path, name, max_batch):
    if name == "dvbs2_small":
        H, layers = small_dvbs2()
    elif name == "mixed":
        H, layers = lc.mixed()
    else:
        H, layers = lc.wlan(int(name[4:]))
    A = codes.canonical_csr(H)
    n_c, n_v = A.shape
    E = int(A.nnz)
    out = run_plan(bp_plan_check, A, layers, max_batch, tmp_path)
    tiles = -(-max_batch // 64)
    assert out["valid"] == 0 and out["unsupported"] == -1 and out["n_e"] == E
    assert out["cw_bytes"] == 4 * n_v + 4 * E
    assert out["cw_per_group"] == min(8, (160 * 1024) // (4 * n_v + 4 * E))
    assert out["bytes_P"] == 4 * n_v * 64 * tiles and out["bytes_R"] == 4 * E * 64 * tiles
    assert out["bytes_total"] == (4 * n_v + 4 * E) * 64 * tiles + 16 * tiles + 4 + 8 * n_v * tiles


def test_bp_plan_names_the_first_wide_check(bp_plan_check, tmp_path):
    """A check of degree 17 passes the layer validation (the min-sum decoder runs it) and is named as unsupported."""
    H, layers = lc.mixed()
    A = sp.lil_matrix(codes.canonical_csr(H))
    c = int(np.argmax(np.diff(codes.canonical_csr(H).indptr) == 16))
    free = [v for v in range(A.shape[1]) if A[c, v] == 0]
    A[c, free[0]] = 1
    H17 = codes.canonical_csr(sp.csr_matrix(A))
    out = run_plan(bp_plan_check, H17, codes.greedy_layers(H17), 4, tmp_path)
    assert out["valid"] == 0 and out["unsupported"] == c


# ---------------------------------------------------------------------------------------------------------------
# the new kernels run without scratch
# ---------------------------------------------------------------------------------------------------------------
def test_bp_kernels_have_no_private_segment():
    """private_segment_fixed_size of every laybp_* kernel in the built code object is 0, read as
    tests/test_cpu_host.py reads it; ibl_layered_create_bp checks the same at run time."""
    from informationbottleneckdecodingldpc_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kstats import code_objects
    seen = {}
    for co in code_objects(_lib.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name],
                                 capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s+- \.", txt):
            m = re.search(r"\.name:\s+(\S+)", blk)
            p = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            if m and p and "laybp_" in m.group(1):
                seen[m.group(1)] = int(p.group(1))
    assert len(seen) == 4, seen   # laybp_fused, laybp_layer, laybp_layer_first, laybp_stage_in
    assert {k: v for k, v in seen.items() if v} == {}
