"""Census of the nonzero-codeword cases of tests/test_gpu_codewords.py, on the references alone (no GPU): every
case's stop lies strictly inside the loop, the decisions at the stop are the transmitted codeword, the ones reach
every check degree and every lane of a packed decision word — and two wrong stop rules that the all-zero inputs
of the older tests cannot tell from the true one give other iteration counts here. The stop iterations below were
measured on the references (oracle/, tests/_minsum_corrected_ref.py, tests/_layered_ref.py,
tests/_layered_fixed_ref.py) and are asserted as constants; none comes from a device."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import _codewords as cw
from tests import _layered_wide as lw
from tests._codes import ib_fold_classes
from tests._layered_ref import layered_decode

IMAX = cw.IMAX_FLOOD

# reference stop iterations (imax 10: the loop's last iteration is 9)
IB_STOPS = {("wlan", 130, 6.0): 6, ("wlan54", 4100, 12.0): 2, ("dvb", 300, 6.0): 8, ("fold", 260, 6.0): 5,
            ("wlan", 9, 6.0): 4, ("wlan", 24, 6.0): 5, ("mixed", 24, 6.0): 5, ("mixed16", 24, 6.0): 7,
            ("mixed", 260, 9.0): 2, ("mixed16", 260, 9.0): 5}
# (code, B) -> stops of ms32, ms64, bp64, corr32, corr64 at the case's Eb/N0 (cw.FLOAT_CASES)
FLOAT_STOPS = {("mixed", 260): (3, 3, 3, 2, 2), ("dvb", 300): (7, 7, 7, 3, 3), ("mixed", 24): (3, 4, 3, 4, 4),
               ("mixed", 5): (3, 3, 3, 2, 2), ("wlan", 70): (4, 4, 4, 6, 6)}
# batches of the sizes an MI355X gives the fused float kernels past the first group (2 x 4 x 256 + 5 in fp32,
# 2 x 2 x 256 + 5 in fp64), at cw.fused_groups_db; fp32 BP is compared with the fp64 oracle at the fp32 batch
FUSED_GROUPS_B = {"32": 2053, "64": 1029}
FUSED_GROUPS_STOPS, FUSED_GROUPS_BP32_STOP = (1, 1, 5, 2, 2), 6
# histograms of the per-codeword iteration counts on stop_spread_batch (imax 8: index 8 = never stopped)
LAYERED_HIST = {"wlan": [0, 62, 40, 13, 4, 2, 1, 0, 8], "mixed": [0, 82, 21, 6, 4, 4, 1, 1, 11],
                "dvb": [0, 1, 93, 4, 18, 6, 0, 0, 8], "wide_mixed": [0, 96, 3, 4, 1, 3, 1, 3, 19],
                "small30": [0, 41, 56, 4, 11, 7, 2, 1, 8]}
FIXED_HIST = {("dvb", (13, 0, 31, 2.0)): [0, 1, 93, 4, 16, 8, 0, 0, 8],
              ("dvb", (16, 1, 63, 3.3)): [0, 1, 93, 4, 20, 4, 0, 0, 8],
              ("wide_mixed", (13, 0, 31, 2.0)): [0, 96, 2, 3, 3, 2, 4, 1, 19],
              ("wide_mixed", (16, 1, 63, 3.3)): [0, 95, 4, 2, 3, 4, 1, 0, 21],
              ("small30", (13, 0, 31, 2.0)): [0, 43, 54, 5, 10, 5, 4, 1, 8],
              ("small30", (16, 1, 63, 3.3)): [0, 37, 60, 5, 8, 5, 5, 2, 8]}


def _share(C):
    return float(np.asarray(C).mean(axis=0).min())


def _degrees_with_two_ones(H, C, classes=None):
    """The (degree,) or (degree, fold class) keys of the checks that see at least two ones in some column."""
    A = sp.csr_matrix(H).astype(np.int64)
    seen = ((A @ np.asarray(C, dtype=np.int64)) >= 2).any(axis=1)
    deg = np.diff(A.indptr)
    keys = deg[:, None] if classes is None else classes
    return {tuple(int(x) for x in k) for k in keys[seen]}, {tuple(int(x) for x in k) for k in keys}


# ---------------------------------------------------------------------------------------------------------------
# the helper
# ---------------------------------------------------------------------------------------------------------------
def test_null_space_and_encoder_agree_on_wlan():
    H, _, _, _ = cw.code("wlan")
    a, b = cw.null_space_codewords(H, 24, seed=3), cw.encoded_codewords(H, 24, seed=3)
    assert a.shape == (648, 24) and np.array_equal(a, b)
    assert not np.array_equal(a, cw.null_space_codewords(H, 24, seed=4))


@pytest.mark.parametrize("name", ["wlan", "wlan54", "mixed", "fold", "mixed16", "dvb", "small30", "wide_mixed"])
def test_codewords(name):
    """H c = 0 and no all-zero column (asserted by the constructions), about half ones, at least a quarter in each."""
    H, g, _, how = cw.code(name)
    C = cw.codewords(name, 24)
    assert not ((sp.csr_matrix(H).astype(np.int64) @ C.astype(np.int64)) & 1).any() and C.any(axis=0).all()
    print(f"{name} ({how}): {H.shape[0]} x {H.shape[1]}, share of ones {C.mean():.3f}, least column {_share(C):.3f}")
    assert 0.45 < C.mean() < 0.55 and _share(C) >= 0.25


def test_mirrored_case_mirrors_the_all_zero_sample():
    from oracle import oracle
    _, g, _, _ = cw.code("fold")            # has degree-1 variables
    C = cw.codewords("fold", 12)
    q, ch, llr = cw.mirrored_case(g, C, 6.0, seed=9, offset=77)
    t0 = oracle.channel_sample(q.cdf_t_given_x_equals_zero, 9, 77, g.n_v, 12)
    deg1 = np.asarray(g.vn_deg) == 1
    assert deg1.sum() == 48
    t0[deg1] = 15
    assert ch.dtype == np.int32 and np.array_equal(ch, np.where(C == 1, 15 - t0, t0))
    L = q.output_LLRs.astype(np.float32)[t0]
    assert llr.dtype == np.float32 and np.array_equal(llr, np.where(C == 1, -L, L))
    assert ((llr < 0) == (ch < 8)).all()
    assert (np.abs(llr[deg1]) == L.max()).all() and ((llr[deg1] < 0) == (C[deg1] == 1)).all()
    assert not ch.flags.writeable and not llr.flags.writeable


# ---------------------------------------------------------------------------------------------------------------
# flooding decoders: one batch-global stop
# ---------------------------------------------------------------------------------------------------------------
def _flood_census(name, B, ebn0, family, want):
    out, it = cw.flood_ref(name, B, ebn0, family)
    C = cw.flood_input(name, B, ebn0)[3]
    print(f"{name} B={B} {ebn0} dB {family}: stop {it} (imax {IMAX}), ones {C.mean():.3f}, least column "
          f"{_share(C):.3f}")
    assert 0 < it < IMAX - 1
    assert it == want
    assert np.array_equal(cw.decided_ones(out, family), C == 1)
    assert _share(C) >= 0.25


@pytest.mark.parametrize("name,B,ebn0", cw.IB_CASES)
def test_ib_stops_inside_the_loop(name, B, ebn0):
    _flood_census(name, B, ebn0, "ib", IB_STOPS[(name, B, ebn0)])


@pytest.mark.parametrize("name,B", list(cw.FLOAT_CASES))
def test_float_stops_inside_the_loop(name, B):
    for family, want in zip(cw.FLOAT_FAMILIES, FLOAT_STOPS[(name, B)]):
        _flood_census(name, B, cw.float_db(name, B, family), family, want)


def test_fused_groups_batch_stops_inside_the_loop():
    for family, want in zip(cw.FLOAT_FAMILIES, FUSED_GROUPS_STOPS):
        B = FUSED_GROUPS_B[family[-2:]]
        _flood_census("wlan", B, cw.fused_groups_db(family), family, want)
    _flood_census("wlan", FUSED_GROUPS_B["32"], cw.fused_groups_db("bp64"), "bp64", FUSED_GROUPS_BP32_STOP)


def test_bp_oracle_is_a_reference_for_fp32():
    """Every fp32 BP case: the fp64 oracle's box-plus does not overflow on it. It does at 12 dB, and on 260
    codewords of mixed at 9 dB — the inputs these cases would otherwise have had."""
    cases = [(n, b, cw.float_db(n, b, "bp64")) for n, b in cw.FLOAT_CASES]
    cases += [("wlan", b, cw.fused_groups_db("bp64")) for b in FUSED_GROUPS_B.values()]
    for name, B, ebn0 in cases:
        llr = cw.flood_input(name, B, ebn0)[2]
        print(f"{name} B={B} {ebn0} dB: largest |LLR| {np.abs(llr).max():.1f}")
        assert cw.bp_oracle_is_the_true_boxplus(cw.code(name)[1], llr)
    for name, B, ebn0 in (("wlan", 70, 12.0), ("mixed", 260, 9.0)):
        assert not cw.bp_oracle_is_the_true_boxplus(cw.code(name)[1], cw.flood_input(name, B, ebn0)[2])


@pytest.mark.parametrize("name,B", sorted({(n, b) for n, b, _ in cw.IB_CASES} | set(cw.FLOAT_CASES)))
def test_ones_reach_every_check_degree(name, B):
    """Some check of every degree (on the fold code: of every (degree, fold class)) sees at least two ones in some
    column: a parity taken as "any one" instead of "an odd number", or read through a wrong variable, is then
    wrong somewhere."""
    H, _, _, _ = cw.code(name)
    classes = ib_fold_classes(H) if name == "fold" else None
    seen, present = _degrees_with_two_ones(H, cw.codewords(name, B), classes)
    print(f"{name} B={B}: {len(present)} kinds of check, all see two ones: {seen == present}")
    assert seen == present
    if name in ("mixed", "mixed16"):
        assert {d for d, in present} == set(range(2, 17))
    if name == "fold":
        assert {(d, c) for d in range(3, 9) for c in (1, 2, 3)} <= present


# ---------------------------------------------------------------------------------------------------------------
# layered decoders: the per-codeword stop on stop_spread_batch
# ---------------------------------------------------------------------------------------------------------------
def _layered_census(name, out, it, want_hist, what):
    H, _, _, _ = cw.code(name)
    llr, bits, kinds = cw.layered_input(name)
    imax = cw.IMAX_LAYERED
    hist = np.bincount(it, minlength=imax + 1).tolist()
    conv = cw.converged(it)
    code_cols = np.isin(kinds, (cw.KIND_HI, cw.KIND_LO))
    print(f"{name} {what}: iterations {hist}, converged {int(conv.sum())} of {it.size}, least share of ones on "
          f"the codeword columns {_share(bits[:, code_cols]):.3f}")
    assert hist == want_hist
    assert len(set(it[conv].tolist())) >= 3
    # a column that never stops reports imax (the flooding decoders' count for the same is imax - 1)
    assert (it[kinds == cw.KIND_NOISE] == imax).all()
    assert conv[kinds != cw.KIND_NOISE].sum() >= 0.8 * (kinds != cw.KIND_NOISE).sum()
    assert np.array_equal((out < 0)[:, conv], (bits == 1)[:, conv])
    assert _share(bits[:, code_cols & conv]) >= 0.25
    assert (conv & (kinds == cw.KIND_ZERO)).any()
    # finished beside running inside the first tile, and the whole second tile finished early
    first = it[:64]
    assert (first <= 2).sum() >= 16 and (first >= 3).sum() >= 16 and (it[64:128] <= 3).all()
    # every lane of a packed decision word (bit b of bits[tile][v] is codeword 64 tile + b) carries a 1
    lanes = {int(b) % 64 for b in np.flatnonzero(conv & bits.any(axis=0))}
    assert lanes == set(range(64))


@pytest.mark.parametrize("name", cw.LAYERED_CODES)
def test_layered_stops_spread(name):
    out, it = cw.layered_ref(name)
    _layered_census(name, out, it, LAYERED_HIST[name], "fp32")
    H, _, _, _ = cw.code(name)
    _, bits, kinds = cw.layered_input(name)
    seen, present = _degrees_with_two_ones(H, bits)
    assert seen == present
    if name == "mixed":
        assert {d for d, in present} == set(range(2, 17))
    if name == "wide_mixed":
        assert {d for d, in present} == set(range(2, 33))


@pytest.mark.parametrize("params", lw.FIXED_PARAMS)
@pytest.mark.parametrize("name", cw.FIXED_CODES)
def test_fixed_point_stops_spread(name, params):
    out, it = cw.fixed_ref(name, params)
    _layered_census(name, out, it, FIXED_HIST[(name, params)], f"fixed {params}")


# ---------------------------------------------------------------------------------------------------------------
# what the all-zero inputs cannot see
# ---------------------------------------------------------------------------------------------------------------
def no_decision_is_one(A, P):
    """Wrong: "the word is all-zero" for "the syndrome is zero"."""
    return ~(P < 0).any(axis=0)


def rotated_syndrome(A, P):
    """Wrong: the decisions gathered through variable index v - 1 instead of v."""
    x = np.roll((P < 0).astype(np.int32), 1, axis=0)
    return ((A @ x) % 2 == 0).all(axis=0)


@pytest.mark.parametrize("rule", [no_decision_is_one, rotated_syndrome])
def test_wrong_stop_rules_pass_all_zero_and_fail_here(rule):
    """The layered reference with a wrong stop rule: on small30_llr (the all-zero codeword, the input of
    tests/test_gpu_layered_wide.py) its iteration counts are those of the true rule, so no test on that input
    would notice; on stop_spread_batch they differ."""
    H, layers = lw.small30()
    B = 65
    true_it = lw.small30_ref(True)[1][:B]
    _, wrong_it = layered_decode(H, layers, lw.small30_llr()[:, :B], lw.SMALL30_IMAX, lw.SMALL30_ALPHA, 0.0,
                                 stop_rule=rule)
    print(f"{rule.__name__} on the all-zero input: {np.bincount(wrong_it).tolist()} (true rule "
          f"{np.bincount(true_it).tolist()})")
    assert len(set(true_it.tolist())) >= 3 and np.array_equal(wrong_it, true_it)
    for name in ("wlan", "mixed"):
        Hc, _, lay, _ = cw.code(name)
        llr, _, kinds = cw.layered_input(name)
        _, it = layered_decode(Hc, lay, llr, cw.IMAX_LAYERED, cw.ALPHA_LAYERED, 0.0, stop_rule=rule)
        ref_it = cw.layered_ref(name)[1]
        differ = it != ref_it
        print(f"{rule.__name__} on stop_spread_batch({name}): {int(differ.sum())} of {it.size} counts differ")
        assert differ[kinds == cw.KIND_HI].all() and differ[kinds == cw.KIND_LO].sum() >= 10
        assert np.array_equal(it[kinds == cw.KIND_ZERO], ref_it[kinds == cw.KIND_ZERO])
