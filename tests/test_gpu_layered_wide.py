"""GPU: the layered min-sum decoder at check degrees 17..32 — the wide kernels of csrc/layered_kernels.hip
(lay_fused_wide, lay_layer_wide, layfix_layer_wide and the wide staging and row-move kernels) against the numpy
restatements of the specification (tests/_layered_ref.py, tests/_layered_fixed_ref.py): outputs and per-codeword
iteration counts bit for bit, no tolerance. The codes and inputs are those of tests/_layered_wide.py;
tests/test_cpu_layered_wide.py holds them to every (degree, first-argmin position) pair of degrees 17..32."""
import functools

import numpy as np
import pytest
import torch

from tests import _layered_wide as lw
from tests._layered_census import FAMILIES, wlan
from tests._layered_fixed_ref import dequantise, fixed_decode, quantise
from tests._layered_ref import layered_decode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from informationbottleneckdecodingldpc_amd import engine as e
    return e


@pytest.fixture(scope="module")
def mixed_graph(engine):
    return engine.Graph(lw.wide_mixed()[0], "cuda:0")


@pytest.fixture(scope="module")
def small_graph(engine):
    return engine.Graph(lw.small30()[0], "cuda:0")


def same(out, ref):
    """torch.equal: same dtype, shape and values, no tolerance (as the other layered suites compare: a zero's sign
    is not part of the value; include/ibldpc.h)."""
    a = torch.from_numpy(np.array(out))      # copies: the shared references are read-only
    b = torch.from_numpy(np.array(ref))
    return a.dtype == b.dtype and torch.equal(a, b)


def gpu_decode(dec, x, early, **kw):
    it = torch.full((x.shape[1],), -1, dtype=torch.int32, device=dec.device)
    out = dec.decode(torch.from_numpy(np.array(x, order="C")).to(dec.device), early_stop=early, iters=it, **kw)
    return out.cpu().numpy(), it.cpu().numpy()


def check(dec, x, early, ref, what="", **kw):
    out, it = gpu_decode(dec, x, early, **kw)
    r_out, r_it = ref
    if out.dtype == np.float32 and r_out.dtype == np.int8:
        r_out = dequantise(r_out, dec.scale)
    print(f"{what} early={early} B={x.shape[1]} -> {out.dtype}: iters {np.bincount(r_it).tolist()}, iters equal "
          f"{np.array_equal(it, r_it)}, out mismatches {int((out != r_out).sum())}")
    assert np.array_equal(it, r_it)
    assert np.array_equal(out, r_out) and same(out, r_out)
    return out, it


@functools.lru_cache(maxsize=None)
def mixed_ref(B, a, b, early):
    H, layers = lw.wide_mixed()
    return lw._frozen(layered_decode(H, layers, lw.wide_awgn(B), lw.CENSUS_IMAX, a, b, early_stop=early))


@pytest.mark.parametrize("ab", lw.WIDE_AB)
@pytest.mark.parametrize("B", [9, 16, 130])
@pytest.mark.parametrize("path", ["passes", "fused"])
def test_wide_mixed_awgn(engine, mixed_graph, path, B, ab):
    """Every check degree 2..32, greedy layers of uneven size: B = 9 (the first columns of the 16), 16, and 130 (a
    ragged second tile on the per-layer path; 17 groups of 8, the last ragged, on the fused one), fixed iterations
    and the early stop."""
    H, layers = lw.wide_mixed()
    a, b = ab
    src = 16 if B == 9 else B
    dec = engine.LayeredDecoder(mixed_graph, layers, lw.CENSUS_IMAX, B, alpha=a, beta=b, path=path)
    assert dec.wide is True and dec.path_in_use == path
    assert dec.geometry(B)[0] == (8 if path == "fused" else 0)
    for early in (True, False):
        ref = mixed_ref(src, a, b, early)
        check(dec, lw.wide_awgn(src)[:, :B], early, (ref[0][:, :B], ref[1][:B]), f"{path} ab={ab}")


@pytest.mark.parametrize("family", lw.WIDE_FAMILIES)
@pytest.mark.parametrize("B", lw.CENSUS_BATCHES)
@pytest.mark.parametrize("path", ["passes", "fused"])
def test_wide_mixed_families(engine, mixed_graph, path, B, family):
    """Ties and zeros of either sign, the clamp with +-FLT_MAX inputs, and subnormals through the wide bodies."""
    H, layers = lw.wide_mixed()
    gen, params = FAMILIES[family]
    x = gen(H, B)
    for a, b, L in params:
        dec = engine.LayeredDecoder(mixed_graph, layers, lw.CENSUS_IMAX, B, alpha=a, beta=b, llr_max=L, path=path)
        assert dec.wide and dec.path_in_use == path
        for early in (True, False):
            ref = layered_decode(H, layers, x, lw.CENSUS_IMAX, a, b, L, early_stop=early)
            check(dec, x, early, ref, f"{family} {path} a={a} b={b}")


def test_auto_picks_fused_by_the_wide_fit_rule(engine, mixed_graph, small_graph):
    """4 N + 16 n_c: wide_mixed 3,584 B (8 codewords per workgroup), small30 61,920 B (2)."""
    for G, (H, layers), cw in ((mixed_graph, lw.wide_mixed(), 8), (small_graph, lw.small30(), 2)):
        dec = engine.LayeredDecoder(G, layers, 2, 5, path="auto")
        assert dec.path_in_use == "fused" and dec.wide and dec.geometry(5)[:2] == (cw, -(-5 // cw))


def test_too_long_for_the_fused_kernel(engine):
    """N = 43200 rate 9/10 (check degrees 28, 29): 4 N + 16 n_c = 241,920 B does not fit 160 KiB; the message
    names the wide rule and auto takes the per-layer kernels."""
    from informationbottleneckdecodingldpc_amd import _lib, codes
    H = codes.dvbs2_structured(seed=5, n=43200, k=38880, groups_hi=0, deg_hi=3, deg_lo=3)
    assert int(np.diff(H.indptr).max()) == 29 and 4 * 43200 + 16 * 4320 == 241920
    layers = codes.dvbs2_layers(H)
    G = engine.Graph(H, "cuda:0")
    with pytest.raises(_lib.IBLError) as e:
        engine.LayeredDecoder(G, layers, 2, 4, path="fused")
    assert f"rc={_lib.IBL_EUNSUPPORTED}" in str(e.value) and "4 N + 16 n_c = 241920" in str(e.value)
    dec = engine.LayeredDecoder(G, layers, 2, 4, path="auto")
    assert dec.path_in_use == "passes" and dec.wide


def test_small30_fused(engine, small_graph):
    """Degree 30 on chip: 2 codewords per workgroup, B = 5 leaves a ragged last group; the early stop at 4.0 dB."""
    H, layers = lw.small30()
    dec = engine.LayeredDecoder(small_graph, layers, lw.SMALL30_IMAX, 5, alpha=lw.SMALL30_ALPHA, path="fused")
    assert dec.wide and dec.path_in_use == "fused" and dec.geometry(5)[:2] == (2, 3)
    for early in (True, False):
        ref = lw.small30_ref(early)
        check(dec, lw.small30_llr()[:, :5], early, (ref[0][:, :5], ref[1][:5]), "small30 fused")


def test_small30_per_layer_and_compaction(engine, small_graph):
    """Three residue layers of 360 checks of degree 30, B = 130, 8 iterations with the early stop; then the same
    decode compacted after every iteration (13 codewords are done after iteration 4 and 43 after 5: the 87 left fit
    two of the three tiles), whose row move covers the fourth state array."""
    H, layers = lw.small30()
    ref = lw.small30_ref(True)
    dec = engine.LayeredDecoder(small_graph, layers, lw.SMALL30_IMAX, lw.SMALL30_B, alpha=lw.SMALL30_ALPHA,
                                path="passes")
    assert dec.wide and dec.path_in_use == "passes"
    out, it = check(dec, lw.small30_llr(), True, ref, "small30 passes")
    assert dec.compaction_stats() == (0, lw.SMALL30_B)
    cdec = engine.LayeredDecoder(small_graph, layers, lw.SMALL30_IMAX, lw.SMALL30_B, alpha=lw.SMALL30_ALPHA,
                                 path="passes", compact=(1, 1))
    c_out, c_it = check(cdec, lw.small30_llr(), True, ref, "small30 compacted")
    n, extent = cdec.compaction_stats()
    print("compactions", n, "extent", extent)
    assert n >= 1 and extent < lw.SMALL30_B
    assert same(c_out, out) and np.array_equal(c_it, it)
    check(dec, lw.small30_llr(), False, lw.small30_ref(False), "small30 passes")


def test_compaction_refusals_stay(engine, small_graph):
    from informationbottleneckdecodingldpc_amd import _lib
    H, layers = lw.small30()
    with pytest.raises(_lib.IBLError, match="per-layer path"):
        engine.LayeredDecoder(small_graph, layers, 2, 5, path="fused", compact=True)


FIXED_B = 260


@functools.lru_cache(maxsize=None)
def fixed_case(code, params, early):
    """-> (float32 input, its quantisation, reference (out int8, iters)) for B = 260."""
    if code == "small30":
        x = lw.small30_llr(FIXED_B)
        return x, quantise(x, params[3]), lw.small30_fixed_ref(params, early, FIXED_B)
    H, layers = lw.wide_mixed()
    x = lw.wide_awgn(FIXED_B)
    xq = quantise(x, params[3])
    return x, xq, lw._frozen(fixed_decode(H, layers, xq, lw.CENSUS_IMAX, *params[:3], early_stop=early))


@pytest.mark.parametrize("params", lw.FIXED_PARAMS)
@pytest.mark.parametrize("code", ["wide_mixed", "small30"])
def test_fixed_point(engine, mixed_graph, small_graph, code, params):
    """B = 260: a second tile of 256 with 4 codewords. float32 and int8 in and out, both stop modes; the int8 input
    is the quantised float input, the float32 output the int8 output divided by scale."""
    G, (H, layers), imax = ((mixed_graph, lw.wide_mixed(), lw.CENSUS_IMAX) if code == "wide_mixed" else
                            (small_graph, lw.small30(), lw.SMALL30_IMAX))
    a16, bq, qm, scale = params
    dec = engine.LayeredFixedDecoder(G, layers, imax, FIXED_B, alpha16=a16, beta_q=bq, q_max=qm, scale=scale)
    assert dec.wide is True and dec.path_in_use == "passes"
    for early in (True, False):
        x, xq, ref = fixed_case(code, params, early)
        for src in (x, xq):
            for dt in (torch.float32, torch.int8):
                if early or (src is x) == (dt is torch.float32):     # fixed iterations: f32 -> f32 and i8 -> i8
                    check(dec, src, early, ref, f"{code} {params} {src.dtype}", out_dtype=dt)


def test_drop_in_class(engine, small_graph):
    """Min_Sum_Layered_Decoder_class_irregular on small30, fp32 and fixed=True, gives the engine's result."""
    import informationbottleneckdecodingldpc_amd as pkg
    H, layers = lw.small30()
    x = np.array(lw.small30_llr()[:, :65])
    xt = torch.from_numpy(x).to("cuda:0")
    for fixed in (False, True):
        d = pkg.Min_Sum_Layered_Decoder_class_irregular(H, lw.SMALL30_IMAX, 16, 65, layers=layers,
                                                        alpha=lw.SMALL30_ALPHA, path="auto", fixed=fixed)
        got = d.decode_OpenCL_min_sum(x)
        got_it = d.last_iterations.cpu().numpy()
        assert d._dec.wide and d._dec.path_in_use == ("passes" if fixed else "fused")
        if fixed:
            dec = engine.LayeredFixedDecoder(small_graph, layers, lw.SMALL30_IMAX, 65, alpha16=13)
            ref = lw.small30_fixed_ref(lw.FIXED_PARAMS[0], True)
            want = dequantise(ref[0][:, :65], 2.0)
        else:
            dec = engine.LayeredDecoder(small_graph, layers, lw.SMALL30_IMAX, 65, alpha=lw.SMALL30_ALPHA, path="auto")
            ref = lw.small30_ref(True)
            want = ref[0][:, :65]
        it = torch.full((65,), -1, dtype=torch.int32, device=dec.device)
        out = dec.decode(xt, iters=it).cpu().numpy()
        assert same(got, out) and np.array_equal(got_it, it.cpu().numpy())
        assert same(got, want) and np.array_equal(got_it, ref[1][:65])


def test_narrow_handles_are_not_wide(engine):
    """WLAN Z = 27 (check degrees 7, 8): narrow on every kernel family; the existing suites cover its values."""
    H, layers = wlan(27)
    G = engine.Graph(H, "cuda:0")
    for path in ("fused", "passes"):
        assert engine.LayeredDecoder(G, layers, 2, 8, path=path).wide is False
    assert engine.LayeredFixedDecoder(G, layers, 2, 8).wide is False
