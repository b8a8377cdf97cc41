"""Wide flooding float decoders on the device: codes with checks of degree 17..32 (tests/_layered_wide.py: wide_mixed,
every degree 2..32, fits the fused kernel; small30, DVB-S2-structured with degree-30 checks, per-pass and small-batch
only) against the CPU oracle, on the three kernel families, with the fold, the corrected kind, the per-codeword stop
and the reference-named classes. Tolerances are the project's: fp32 min-sum bit-exact, fp64 atol 1e-9 (min-sum
bit-exact), fp32 BP 1e-5 relative + 1e-4 (at the inputs tests/test_cpu_float_wide.py holds the fp32 order to),
corrected min-sum equal by value to tests/_minsum_corrected_ref.decode."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from informationbottleneckdecodingldpc_amd import _lib, codes, graph
from oracle import oracle
from tests import _float_wide_ref as R
from tests._layered_wide import small30, wide_mixed
from tests._minsum_corrected_ref import decode as corrected_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PREC = {"fp32": (torch.float32, np.float32), "fp64": (torch.float64, np.float64)}
PATHS = ["fused", "passes", "small"]
KINDS = {"ms": oracle.MINSUM, "bp": oracle.BP}


@pytest.fixture(scope="module")
def eng():
    from informationbottleneckdecodingldpc_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _G(name):
    from informationbottleneckdecodingldpc_amd import engine
    return engine.Graph(R.wide_graph(name), DEV)


def _make(eng, name, kind, prec, max_batch, path, imax, pair=(1.0, 0.0)):
    """path: "fused"; "passes" = the per-pass kernels (small batch off); "small" = the small-batch kernels."""
    dec = eng.FloatDecoder(_G(name), KINDS[kind], imax, max_batch, precision=PREC[prec][0],
                           path="fused" if path == "fused" else "passes", alpha=pair[0], beta=pair[1])
    assert dec.wide
    assert dec.fused == (path == "fused")
    if path != "fused":
        dec.small_batch = max_batch if path == "small" else 0
        assert dec.small_batch == (max_batch if path == "small" else 0)
    return dec


def _run(dec, llr, prec, early):
    it = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    out = dec.decode(torch.from_numpy(np.array(llr)).to(DEV).to(PREC[prec][0]), early_stop=early, iters=it)
    torch.cuda.synchronize()
    assert out.dtype == PREC[prec][0]
    return out, int(it.item())


@functools.lru_cache(maxsize=None)
def _ref(name, B, dB, imax, kind, prec, early):
    """Oracle decode (computed once, read-only): fp32 min-sum in float32, everything else in fp64 — fp32 BP is held to
    the fp64 oracle."""
    g, llr = R.wide_graph(name), R.wide_llr(name, B, dB)
    if kind == "ms" and prec == "fp32":
        out, it = oracle.float32_decode(g, imax, llr, early_stop=early, return_iters=True)
    else:
        out, it = oracle.float_decode(g, KINDS[kind], imax, llr.astype(np.float64), early_stop=early, return_iters=True)
    out.setflags(write=False)
    return out, it


def _compare(out, it, ref, ref_it, kind, prec, what):
    out = out.cpu().numpy()
    assert it == ref_it, what
    if kind == "ms":
        assert out.dtype == ref.dtype and np.array_equal(out.view(np.uint8), ref.view(np.uint8)), what
    elif prec == "fp64":
        np.testing.assert_allclose(out, ref, rtol=0, atol=1e-9, err_msg=str(what))
    else:
        bad = R.h5(out.astype(np.float64), ref)
        print(f"{what}: max |x-y| = {np.abs(out - ref).max():.3e}, outside: {int(bad.sum())}")
        assert bad.sum() == 0, what
        assert int((((out < 0) != (ref < 0)) & (np.abs(ref) > R.REL * np.abs(ref) + R.TOL_ABS)).sum()) == 0, what


# ------------------------------------------------------------------ 1. oracle parity on wide_mixed, every path
@pytest.mark.parametrize("B", [3, 9, 130])
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("kind", list(KINDS))
def test_wide_mixed_vs_oracle(eng, kind, prec, path, B):
    """Every check degree 2..32 at 3.0 dB, 6 iterations, fixed and with the batch stop (which does not come). B = 3
    and 9 leave a ragged last word and group; B = 130 exceeds the small-batch default of 64."""
    dec = _make(eng, "wide_mixed", kind, prec, B, path, 6)
    for early in (False, True):
        ref, ref_it = _ref("wide_mixed", B, 3.0, 6, kind, prec, early)
        out, it = _run(dec, R.wide_llr("wide_mixed", B, 3.0), prec, early)
        _compare(out, it, ref, ref_it, kind, prec, (kind, prec, path, B, early))


# ------------------------------------------------------------------ 2. chunk boundary of the per-pass kernels
@pytest.mark.parametrize("prec,B", [("fp32", 260), ("fp64", 130)])
def test_per_pass_chunk_boundary(eng, prec, B):
    """fp32 at B = 260: two 256-codeword chunks, the second ragged; fp64 at B = 130: two 128-codeword chunks."""
    dec = _make(eng, "wide_mixed", "ms", prec, B, "passes", 6)
    ref, ref_it = _ref("wide_mixed", B, 3.0, 6, "ms", prec, False)
    out, it = _run(dec, R.wide_llr("wide_mixed", B, 3.0), prec, False)
    _compare(out, it, ref, ref_it, "ms", prec, (prec, B))


# ------------------------------------------------------------------ 3. small30
@pytest.mark.parametrize("kind,prec,B,path", [("ms", "fp32", 9, "small"), ("ms", "fp32", 130, "passes"),
                                              ("ms", "fp64", 9, "small"), ("bp", "fp32", 9, "small"),
                                              ("bp", "fp64", 9, "small")])
def test_small30_vs_oracle(eng, kind, prec, B, path):
    """Degree-29 and degree-30 checks, too large for the fused kernel: B = 9 takes the small-batch kernels by default,
    B = 130 the per-pass kernels with the fold. Fixed at 4.0 dB (8 iterations); with the stop at 5.5 dB (imax 12) the
    stop iteration is the oracle's 5 (B = 9) or 6 (B = 130)."""
    dec = eng.FloatDecoder(_G("small30"), KINDS[kind], 8, B, precision=PREC[prec][0])
    assert dec.wide and not dec.fused and dec.small_batch == 64 and dec.folded == 1079
    ref, ref_it = _ref("small30", B, 4.0, 8, kind, prec, False)
    out, it = _run(dec, R.wide_llr("small30", B, 4.0), prec, False)
    _compare(out, it, ref, ref_it, kind, prec, (kind, prec, B, "fixed"))
    dec = eng.FloatDecoder(_G("small30"), KINDS[kind], 12, B, precision=PREC[prec][0])
    ref, ref_it = _ref("small30", B, 5.5, 12, kind, prec, True)
    assert ref_it == (5 if B == 9 else 6)
    out, it = _run(dec, R.wide_llr("small30", B, 5.5), prec, True)
    _compare(out, it, ref, ref_it, kind, prec, (kind, prec, B, "stop"))


# ------------------------------------------------------------------ 4. the families agree bit for bit
@pytest.mark.parametrize("B", [9, 130])
@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("kind,pair", [("ms", (1.0, 0.0)), ("bp", (1.0, 0.0)), ("ms", R.CORRECTED[0])])
def test_families_agree(eng, kind, pair, prec, B):
    llr = R.wide_llr("wide_mixed", B, 3.0)
    outs = [_run(_make(eng, "wide_mixed", kind, prec, B, path, 6, pair), llr, prec, False)[0] for path in PATHS]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    # bit for bit: the sign of a zero too
    assert torch.equal(torch.signbit(outs[0]), torch.signbit(outs[1])) and torch.equal(torch.signbit(outs[1]), torch.signbit(outs[2]))


# ------------------------------------------------------------------ 5. the fold
@pytest.mark.parametrize("early", [False, True])
@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("kind", list(KINDS))
def test_fold_equals_unfolded(eng, kind, prec, early, monkeypatch):
    """small30 per pass folds its 1079 staircase variables into wide check items; outputs and iters equal those of a
    decoder created with IBL_FL_FOLD=0. With the stop (5.5 dB, imax 12) the folded passes also write the variable inbox."""
    B, dB, imax = 9, (5.5 if early else 4.0), (12 if early else 8)
    llr = R.wide_llr("small30", B, dB)
    res = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("IBL_FL_FOLD", fold)
        dec = _make(eng, "small30", kind, prec, B, "passes", imax)
        assert dec.folded == (1079 if fold == "1" else 0)
        res[fold] = _run(dec, llr, prec, early)
    assert res["1"][1] == res["0"][1]
    assert torch.equal(res["1"][0], res["0"][0])
    if early:
        assert res["1"][1] == 5


# ------------------------------------------------------------------ 6. corrected min-sum
@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("pair", R.CORRECTED)
@pytest.mark.parametrize("name,path", [("wide_mixed", "fused"), ("wide_mixed", "passes"), ("wide_mixed", "small"),
                                       ("small30", "passes")])
def test_corrected_vs_reference(eng, name, path, pair, prec):
    B, dB, imax = 9, (3.0 if name == "wide_mixed" else 4.0), (6 if name == "wide_mixed" else 8)
    llr = R.wide_llr(name, B, dB)
    ref, ref_it = corrected_ref(R.wide_graph(name), pair[0], pair[1], imax, llr.astype(PREC[prec][1]), PREC[prec][1])
    dec = _make(eng, name, "ms", prec, B, path, imax, pair)
    assert dec.correction == pair
    out, it = _run(dec, llr, prec, False)
    assert it == ref_it
    assert out.cpu().numpy().dtype == ref.dtype and np.array_equal(out.cpu().numpy(), ref)


# ------------------------------------------------------------------ 7. second group of the fused kernel
def test_fused_past_the_second_group(eng):
    """wide_mixed on the fused kernel with more than two groups per workgroup and a ragged last group: fixed iterations
    against the oracle, a converging batch (9.0 dB) against its stop iteration, and fp32 BP against the per-pass path."""
    max_b = 16392
    dec = _make(eng, "wide_mixed", "ms", "fp32", max_b, "fused", 6)
    grid = dec.fused_geometry(max_b)[1]
    B = 4 * 2 * grid + 5
    assert grid > 0 and B <= max_b, f"grid {grid}: needs max_batch >= {B}"
    ngroups, g2 = dec.fused_geometry(B)
    print(f"fused geometry: B={B}: ngroups={ngroups} grid={g2}")
    assert g2 == grid and ngroups > 2 * grid and B % 4 != 0
    ref, ref_it = _ref("wide_mixed", B, 3.0, 6, "ms", "fp32", False)
    out, it = _run(dec, R.wide_llr("wide_mixed", B, 3.0), "fp32", False)
    _compare(out, it, ref, ref_it, "ms", "fp32", "fixed")
    # 9.0 dB as it is: a batch this large holds a wrong degree-1 variable, whose check stays unsatisfied, so the
    # oracle runs to imax - 1; with the degree-1 variables' values made positive it stops at 2 and the kernel runs
    # its second pass to that iteration
    g = R.wide_graph("wide_mixed")
    llr = np.array(R.wide_llr("wide_mixed", B, 9.0))
    for fix in (False, True):
        if fix:
            d1 = np.asarray(g.vn_deg) == 1
            llr[d1] = np.abs(llr[d1])
        ref, ref_it = oracle.float32_decode(g, 6, llr, early_stop=True, return_iters=True)
        assert (1 <= ref_it <= 3) if fix else ref_it == 5
        out, it = _run(dec, llr, "fp32", True)
        _compare(out, it, ref, ref_it, "ms", "fp32", ("stop", fix))
    del dec
    llr = R.wide_llr("wide_mixed", B, 3.0)
    a = _run(_make(eng, "wide_mixed", "bp", "fp32", B, "fused", 6), llr, "fp32", False)[0]
    b = _run(_make(eng, "wide_mixed", "bp", "fp32", B, "passes", 6), llr, "fp32", False)[0]
    assert torch.equal(a, b)


# ------------------------------------------------------------------ 8. per-codeword stop
def test_per_codeword_stop(eng):
    """wide_mixed at 7.0 dB, 37 codewords on the fused kernel: fp32 min-sum columns and iters equal the oracle's
    decode of each column alone; fp32 BP and fp64 min-sum columns equal a batch-stop decode of that column on the
    same handle."""
    B, imax = 37, 12
    llr = R.wide_llr("wide_mixed", B, 7.0)
    g = R.wide_graph("wide_mixed")
    for kind, prec in (("ms", "fp32"), ("bp", "fp32"), ("ms", "fp64")):
        dec = _make(eng, "wide_mixed", kind, prec, B, "fused", imax)
        x = torch.from_numpy(np.array(llr)).to(DEV).to(PREC[prec][0])
        its = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        out = dec.decode(x, early_stop="codeword", iters=its)
        torch.cuda.synchronize()
        out, its = out.cpu().numpy(), its.cpu().numpy()
        one = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        for c in range(B):
            if kind == "ms" and prec == "fp32":
                r, r_it = oracle.float32_decode(g, imax, llr[:, c:c + 1], early_stop=True, return_iters=True)
                r = r[:, 0]
            else:
                r = dec.decode(x[:, c:c + 1].contiguous(), early_stop=True, iters=one).cpu().numpy()[:, 0]
                r_it = int(one.item())
            assert its[c] == r_it, (kind, prec, c)
            assert np.array_equal(np.ascontiguousarray(out[:, c]).view(np.uint8),
                                  np.ascontiguousarray(r).view(np.uint8)), (kind, prec, c)
        assert len(set(its.tolist())) >= 2, (kind, prec)


# ------------------------------------------------------------------ 9. the reference-named classes
def test_dropin_classes_on_small30():
    """msg_at_time = 2 (the reference driver's batch), numpy in and out, early stop as the classes decode."""
    from informationbottleneckdecodingldpc_amd.bp_decoder_irreg import BeliefPropagationDecoderClassIrregular
    from informationbottleneckdecodingldpc_amd.min_sum_decoder_irreg import Min_Sum_Decoder_class_irregular
    H, g = small30()[0], R.wide_graph("small30")
    llr = np.ascontiguousarray(R.wide_llr("small30", 9, 5.5)[:, :2])
    ms = Min_Sum_Decoder_class_irregular(H, 12, 16, 2)
    ms.init_OpenCL_decoding(2)
    assert ms.wide and ms._dec.wide
    out = ms.decode_OpenCL_min_sum(llr)
    ref = oracle.float32_decode(g, 12, llr, early_stop=True)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    buf = ms.decode_OpenCL_min_sum(torch.from_numpy(llr).to(DEV), buffer_in=True, return_buffer=True)
    assert ms.return_errors_all_zero(buf) == float((ref[:ms.data_len] < 0).sum())
    bp = BeliefPropagationDecoderClassIrregular(H, 12, 16, 2, precision=torch.float64)
    bp.init_OpenCL_decoding(2)
    assert bp.wide and bp._dec.wide
    out = bp.decode_OpenCL_belief_propagation(llr.astype(np.float64))
    ref = oracle.float_decode(g, oracle.BP, 12, llr.astype(np.float64), early_stop=True)
    np.testing.assert_allclose(out, ref, rtol=0, atol=1e-9)
    assert bp.return_errors_all_zero(out) == float((ref[:bp.data_len] < 0).sum())


# ------------------------------------------------------------------ 10. refusals that stay
def test_refusals_and_narrow_handles(eng):
    def two_checks(d):   # a check of degree d and a degree-3 check that shares its last variable
        M = sp.lil_matrix((2, d + 2), dtype=np.int64)
        M[0, :d] = 1
        M[1, d - 1:] = 1
        return codes.canonical_csr(M.tocsr())
    H = two_checks(33)
    for create in (lambda G: eng.FloatDecoder(G, 0, 5, 4), lambda G: eng.FloatDecoder(G, 1, 5, 4, precision=torch.float64),
                   lambda G: eng.FloatDecoder(G, 0, 5, 4, alpha=0.75)):
        with pytest.raises(_lib.IBLError) as e:
            create(eng.Graph(graph.build_graph(H), DEV))
        assert f"rc={_lib.IBL_EUNSUPPORTED}" in str(e.value) and "check degrees <= 32" in str(e.value) and "33" in str(e.value)
    V = sp.lil_matrix((17, 18), dtype=np.int64)
    V[:, 0] = 1
    for r in range(17):
        V[r, 1 + r] = 1
    with pytest.raises(_lib.IBLError) as e:
        eng.FloatDecoder(eng.Graph(graph.build_graph(codes.canonical_csr(V.tocsr())), DEV), 0, 5, 4)
    assert f"rc={_lib.IBL_EUNSUPPORTED}" in str(e.value) and "variable degrees <= 16" in str(e.value) and "17" in str(e.value)
    assert eng.FloatDecoder(eng.Graph(graph.build_graph(two_checks(32)), DEV), 0, 5, 4).wide   # 32 is accepted
    narrow = eng.FloatDecoder(eng.Graph(graph.build_graph(codes.wlan_80211n(27)), DEV), 0, 5, 4)
    assert narrow.wide is False
