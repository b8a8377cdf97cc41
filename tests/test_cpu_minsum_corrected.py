"""CPU: the corrected (normalised / offset) flooding min-sum — its numpy reference pinned to the oracle, cross-checked
by a scalar restatement, the conditions its GPU test inputs must meet, the C ABI's parameter checks (no device), the
new kernels' code-object metadata and the drop-in classes' refusals (include/ibldpc.h "Corrected min-sum")."""
import ctypes
import os
import re

import numpy as np
import pytest

from informationbottleneckdecodingldpc_amd import graph
from oracle import oracle
from tests import _minsum_corrected_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from informationbottleneckdecodingldpc_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    return _lib


@pytest.fixture(scope="module")
def graphs():
    return {"mixed": graph.build_graph(R.mixed_H()), "wlan": graph.build_graph(R.wlan_H()),
            "dvb": graph.build_graph(R.dvb_H())}


def _inputs(graphs, name, B):
    g = graphs[name]
    return g, (R.halves_llrs(g, B, 15) if name == "mixed" else R.quantised_llrs(g, B, 2.0, 3))


# ------------------------------------------------------------------ 1. oracle pin
@pytest.mark.parametrize("name", ["mixed", "wlan"])
@pytest.mark.parametrize("early", [True, False])
def test_reference_at_1_0_is_the_oracle(graphs, name, early):
    """(1, 0) is plain min-sum: outputs and stop iteration of the oracle, fp32 and fp64. On the mixed code the
    early-stop run ends at iteration 5 of 5 (measured), so the stop bookkeeping is exercised to the last pass."""
    g, llr = _inputs(graphs, name, 24)
    o32, i32 = oracle.float32_decode(g, 6, llr.astype(np.float32), early_stop=early, return_iters=True)
    r32, j32 = R.decode(g, 1.0, 0.0, 6, llr, np.float32, early_stop=early)
    assert j32 == i32
    assert r32.dtype == np.float32 and np.array_equal(r32, o32)
    o64, i64 = oracle.float_decode(g, oracle.MINSUM, 6, llr, early_stop=early, return_iters=True)
    r64, j64 = R.decode(g, 1.0, 0.0, 6, llr, np.float64, early_stop=early)
    assert j64 == i64
    assert r64.dtype == np.float64 and np.array_equal(r64, o64)


def test_reference_stops_early_where_the_oracle_does(graphs):
    """A converging batch: the stop iteration is below imax - 1 and equal."""
    g = graphs["wlan"]
    llr = R.quantised_llrs(g, 8, 6.0, 2).astype(np.float32)
    o, i = oracle.float32_decode(g, 12, llr, early_stop=True, return_iters=True)
    r, j = R.decode(g, 1.0, 0.0, 12, llr, np.float32, early_stop=True)
    assert i < 11 and j == i and np.array_equal(r, o)


# ------------------------------------------------------------------ 2. scalar cross-check
def _scalar_decode(g, alpha, beta, imax, llr, dtype, early_stop, llr_max=150.0):
    """Plain loops over codeword, check, edge with one running two-smallest scan; shares no code with R.decode."""
    F = np.dtype(dtype).type
    a, b, lm = F(alpha), F(beta), F(llr_max)
    n_v, B = llr.shape
    cs, cd, tc = (np.asarray(x).tolist() for x in (g.cn_start, g.cn_deg, g.tgt_cn))
    vs, vd, tv = (np.asarray(x).tolist() for x in (g.vn_start, g.vn_deg, g.tgt_vn))
    out = np.zeros((n_v, B), dtype=F)
    cins, vins = [], []
    chs = [[F(x) for x in llr[:, col]] for col in range(B)]
    for col in range(B):
        ch = chs[col]
        cin = [F(0)] * g.n_e
        for n in range(n_v):
            for w in range(vd[n]):
                cin[tv[vs[n] + w]] = ch[n]
        cins.append(cin)
        vins.append([F(0)] * g.n_e)
    i, stop = 1, False
    while i < imax and not stop:
        syn = 0
        for col in range(B):
            cin, vin, ch = cins[col], vins[col], chs[col]
            for c in range(len(cd)):
                s, d = cs[c], cd[c]
                m1 = m2 = F(np.inf)
                k1 = -1
                par = False
                for j in range(d):
                    x = cin[s + j]
                    ax = -x if x < 0 else x
                    par ^= bool(x < 0)
                    if ax < m1:
                        m1, m2, k1 = ax, m1, j
                    elif ax < m2:
                        m2 = ax
                for w in range(d):
                    M = m2 if w == k1 else m1
                    t = F(a * M)
                    u = F(t - b)
                    r = u if u > 0 else F(0)
                    sgn = par ^ bool(cin[s + w] < 0)
                    vin[tc[s + w]] = F(-r) if sgn else r
            for n in range(n_v):
                s, d = vs[n], vd[n]
                for w in range(d):
                    x = ch[n]
                    for v in range(d):
                        if v != w:
                            x = F(x + vin[s + v])
                    cin[tv[s + w]] = lm if x > lm else (F(-lm) if x < -lm else x)
            if early_stop:
                for c in range(len(cd)):
                    p = False
                    for j in range(cd[c]):
                        p ^= bool(cin[cs[c] + j] < 0)
                    syn += p
        stop = early_stop and syn == 0
        i += 1
    for col in range(B):
        for n in range(n_v):
            x = chs[col][n]
            for v in range(vd[n]):
                x = F(x + vins[col][vs[n] + v])
            out[n, col] = x
    return out, i - 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("pair", R.PAIRS)
def test_scalar_restatement_agrees(pair, dtype):
    from tests._codes import mixed_code
    g = graph.build_graph(mixed_code(np.arange(2, 17), np.arange(1, 17), 60, seed=4))
    noisy = 2.0 + 2.5 * np.random.default_rng(9).standard_normal((g.n_v, 2))   # inexact products, few ties
    llr = np.concatenate([R.halves_llrs(g, 2, 9), noisy], axis=1).astype(dtype)
    assert np.isfinite(llr).all()
    for early in (False, True):
        ref, it = R.decode(g, pair[0], pair[1], 5, llr, dtype, early_stop=early)
        out, jt = _scalar_decode(g, pair[0], pair[1], 5, llr, dtype, early)
        assert jt == it
        assert np.array_equal(out, ref)


# ------------------------------------------------------------------ 3. census of the GPU inputs
# (code, pair) -> measured at B = 12, imax 6, fp32 with the seeds of _inputs: zeroed-though-nonzero share, tied share
#   wlan (0.8125, 0.15) 5.8 % / 11.1 %   wlan (1, 0.25) 9.6 % / 11.5 %   wlan (0.75, 0.5) 44.0 % / 14.9 %
#   dvb  (0.8125, 0.15) 5.4 % / 10.8 %   dvb  (1, 0.25) 9.1 % / 11.3 %   dvb  (0.75, 0.5) 42.9 % / 14.2 %
#   mixed halves (0.8125, 0.15) 32.0 % / 9.6 %   mixed halves (1, 0.25) 28.0 % / 29.6 %
CENSUS_CASES = [(n, p) for n in ("wlan", "dvb") for p in R.PAIRS] + [("mixed", p) for p in R.MIXED_PAIRS]


@pytest.mark.parametrize("name,pair", CENSUS_CASES)
def test_gpu_inputs_reach_the_zeroing_and_the_ties(graphs, name, pair):
    """The inputs of tests/test_gpu_minsum_corrected.py make max(., 0) zero a real share of nonzero magnitudes (but
    not most of them) and make the smallest and second-smallest magnitude tie in a real share of the checks: conditions
    on the inputs, so that the GPU equality tests can show a wrong offset, clamp or tie rule."""
    g, llr = _inputs(graphs, name, 12)
    c = {}
    R.decode(g, pair[0], pair[1], 6, llr, np.float32, census=c)
    zeroed, tied = c["zeroed"] / c["outputs"], c["tied"] / c["checks"]
    print(f"{name} {pair}: zeroed though nonzero {zeroed:.3f}, tied checks {tied:.3f}")
    # These are the 2 dB inputs, which every fixed-iteration GPU run uses: those runs pin the arithmetic. The GPU
    # early-stop runs use 10 dB / 12 dB inputs (degree-1 variables at the top level) so that the reference stops before
    # imax - 1; nearly all their LLRs are the top level, they are not censused, and they pin only the stop iteration
    # and the outputs of a decode that ends early.
    assert 0.03 <= zeroed <= 0.60
    assert tied >= 0.05


# ------------------------------------------------------------------ 4. contraction is visible
@pytest.mark.parametrize("name", ["wlan", "dvb"])
def test_a_fused_multiply_add_would_show(graphs, name):
    """t = a * M, u = t - b as one fused multiply-add changes the decode on the quantised inputs (measured: 49 % of
    the WLAN outputs, 52 % of the DVB-S2 ones), so the GPU equality tests tell a contracted kernel from a correct one."""
    g, llr = _inputs(graphs, name, 12)
    two, _ = R.decode(g, 0.8125, 0.15, 6, llr, np.float32)
    one, _ = R.decode(g, 0.8125, 0.15, 6, llr, np.float32, fma=True)
    differ = float((two != one).mean())
    print(f"{name}: outputs that differ under contraction {differ:.3f}")
    assert differ > 0.05


def test_contraction_after_one_operation_and_where_it_cannot_show():
    """One operation on random fp32 magnitudes: about a third of the values differ (measured 34 %). With alpha = 1 the
    product is exact, so nothing can differ — the halves family at (1, 0.25) alone would not see contraction, which is
    why the quantised family is needed as well."""
    rng = np.random.default_rng(5)
    M = rng.uniform(0.0, 20.0, 100000).astype(np.float32)
    a, b = np.float32(0.8125), np.float32(0.15)
    two = a * M - b
    one = (np.float64(a) * M.astype(np.float64) - np.float64(b)).astype(np.float32)
    share = float((two != one).mean())
    print(f"one operation: {share:.3f} differ")
    assert 0.2 < share < 0.5
    g = graph.build_graph(R.mixed_H())
    llr = R.halves_llrs(g, 12, 15)
    two, _ = R.decode(g, 1.0, 0.25, 6, llr, np.float32)
    one, _ = R.decode(g, 1.0, 0.25, 6, llr, np.float32, fma=True)
    assert np.array_equal(two, one)


# ------------------------------------------------------------------ 5. meaning
def test_normalisation_halves_the_frame_errors(graphs):
    """WLAN Z = 27, AWGN 2.0 dB, 400 frames of default_rng(21), imax 20, no stop, fp32: frame errors at (0.8125, 0) are
    at most half of plain min-sum's. Measured with this seed: 18 against 63 (bit errors 315 against 3327)."""
    g = graphs["wlan"]
    llr = R.awgn_llrs(g, 400, 2.0, 21).astype(np.float32)
    fe = {}
    for pair in ((1.0, 0.0), (0.8125, 0.0)):
        out, _ = R.decode(g, pair[0], pair[1], 20, llr, np.float32)
        bad = out < 0
        fe[pair] = (int(bad.any(axis=0).sum()), int(bad.sum()))
    print(f"frame / bit errors: plain {fe[(1.0, 0.0)]}, alpha 0.8125 {fe[(0.8125, 0.0)]}")
    assert fe[(1.0, 0.0)][0] > 0
    assert 2 * fe[(0.8125, 0.0)][0] <= fe[(1.0, 0.0)][0]


# ------------------------------------------------------------------ 6. C ABI without a device
def test_header_declares_the_corrected_entry_points():
    txt = open(os.path.join(ROOT, "include", "ibldpc.h")).read()
    assert "Corrected min-sum" in txt
    assert re.search(r"int ibl_float_create_corrected\(const ibl_graph\* g, double alpha, double beta, int32_t imax,\s+"
                     r"double llr_max,\s+int32_t precision, int32_t max_batch, ibl_float\*\* out\);", txt)
    assert "int ibl_float_correction(const ibl_float* h, double* alpha, double* beta);" in txt


def test_create_corrected_checks_its_parameters_before_the_graph(lib):
    L = lib.load()
    EINVAL = lib.IBL_EINVAL

    def create(alpha=0.8125, beta=0.15, imax=6, prec=lib.IBL_F32, max_batch=4, out=True):
        h = ctypes.c_void_p()
        rc = L.ibl_float_create_corrected(None, alpha, beta, imax, 150.0, prec, max_batch,
                                          ctypes.byref(h) if out else None)
        assert not h.value
        return rc, L.ibl_last_error().decode()

    rc_ok, msg_ok = create()
    assert rc_ok == EINVAL and "graph is NULL" in msg_ok
    for alpha in (0.0, -0.5, 1.0625, float("inf"), float("nan")):
        rc, msg = create(alpha=alpha)
        assert rc == EINVAL and "alpha" in msg, (alpha, rc, msg)
    for beta in (-0.25, float("inf"), float("nan")):
        rc, msg = create(beta=beta)
        assert rc == EINVAL and "beta" in msg, (beta, rc, msg)
    for kw, word in ((dict(imax=0), "imax"), (dict(max_batch=0), "max_batch"), (dict(prec=lib.IBL_I32), "precision"),
                     (dict(out=False), "out is NULL")):
        rc, msg = create(**kw)
        assert rc == EINVAL and word in msg, (kw, rc, msg)
    # the domain holds for the values converted to the decoder's precision: an alpha that rounds to 0 and a beta that
    # rounds to infinity in fp32 are refused there and pass the parameter checks of an fp64 decoder
    for kw, word in ((dict(alpha=1e-50), "alpha"), (dict(beta=1e300), "beta")):
        rc, msg = create(**kw)
        assert rc == EINVAL and word in msg, (kw, rc, msg)
        rc, msg = create(prec=lib.IBL_F64, **kw)
        assert rc == EINVAL and "graph is NULL" in msg, (kw, rc, msg)
    rc, msg = create(beta=-0.0)
    assert rc == EINVAL and "graph is NULL" in msg
    a, b = ctypes.c_double(), ctypes.c_double()
    assert L.ibl_float_correction(None, ctypes.byref(a), ctypes.byref(b)) == EINVAL


# ------------------------------------------------------------------ 7. no private segment
def test_corrected_kernels_have_no_private_segment(lib):
    """Every corrected instantiation (check-body kind 2: fl_cn and fl_cn_small at both MAXD, fl_fused in its three
    shapes, each in fp32 and fp64 = 14 kernels) is in the built code object with private_segment_fixed_size 0."""
    import subprocess
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kstats import code_objects
    seen = {}
    for co in code_objects(lib.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name],
                                 capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s+- \.", txt):
            m = re.search(r"\.name:\s+(\S+)", blk)
            p = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            if m and p and re.search(r"fl_(cn|cn_small|fused)ILi2E", m.group(1)):
                seen[m.group(1)] = int(p.group(1))
    assert len(seen) == 14, sorted(seen)
    assert {k: v for k, v in seen.items() if v} == {}


# ------------------------------------------------------------------ 8. drop-in refusals
def test_drop_in_classes_take_or_refuse_the_correction():
    from informationbottleneckdecodingldpc_amd.bp_decoder_irreg import BeliefPropagationDecoderClassIrregular
    from informationbottleneckdecodingldpc_amd.min_sum_decoder_irreg import Min_Sum_Decoder_class_irregular
    H = R.wlan_H()
    with pytest.raises(ValueError):
        BeliefPropagationDecoderClassIrregular(H, 6, 16, 4, alpha=0.8)
    with pytest.raises(ValueError):
        BeliefPropagationDecoderClassIrregular(H, 6, 16, 4, beta=0.25)
    BeliefPropagationDecoderClassIrregular(H, 6, 16, 4)
    assert Min_Sum_Decoder_class_irregular(H, 6, 16, 4).correction == (1.0, 0.0)
    assert Min_Sum_Decoder_class_irregular(H, 6, 16, 4, alpha=0.8125, beta=0.15).correction == (0.8125, 0.15)
    with pytest.raises(TypeError):
        Min_Sum_Decoder_class_irregular(H, 6, 16, 4, 0.8125)   # keyword-only
