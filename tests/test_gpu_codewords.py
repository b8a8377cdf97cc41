"""GPU: every decoder's early stop and decisions on transmissions of nonzero codewords (tests/_codewords.py).

On the all-zero codeword "the syndrome is zero" and "no decision is 1" come true together, so the other GPU tests
that pin a stop iteration cannot tell a wrong stop rule, a syndrome gathered through a wrong variable or a decision
packed at a wrong bit from the right one (tests/test_cpu_codewords.py shows two such rules passing there). Here
about half of the transmitted bits are 1 and every reference stop lies strictly inside the loop; that file asserts
it on the CPU for each case below, with the stop iterations as constants.

Bars, as in the decoders' own test files: np.array_equal on every output value and an equal stop iteration (IB,
fp32 / fp64 min-sum and corrected min-sum, layered fp32 and fixed point: per-codeword iteration vectors); fp64 BP
within 1e-9 of the fp64 oracle; fp32 BP within H5 of it with no hard-decision flip; and everywhere the device's
decisions on the converging columns are the transmitted bits. Every case also decodes the same input once with
early_stop=False."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import _codewords as cw
from tests import _layered_compact_ref as cr
from tests import _layered_wide as lw
from tests._layered_fixed_ref import dequantise, quantise
from tests._layered_ref import layered_decode
from tests.test_gpu_float import _h5, _hard_flips

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMAX = cw.IMAX_FLOOD


@pytest.fixture(scope="module")
def eng():
    from informationbottleneckdecodingldpc_amd import engine
    return engine


_graphs = {}


def device_graph(eng, name):
    if name not in _graphs:
        _graphs[name] = eng.Graph(cw.code(name)[1], DEV)
    return _graphs[name]


# ---------------------------------------------------------------------------------------------------------------
# IB
# ---------------------------------------------------------------------------------------------------------------
IB_RUNS = {
    # id: ((code, B, Eb/N0), decoder arguments, IBL_FUSED_NCW)
    "fused_8": (("wlan", 130, 6.0), dict(path="fused"), "8"),
    "fused_4": (("wlan", 130, 6.0), dict(path="fused"), "4"),
    "fused_groups": (("wlan54", 4100, 12.0), dict(path="fused"), None),     # 513 groups of 8: past the first group
    "passes_fold": (("dvb", 300, 6.0), dict(path="passes"), None),
    "passes_no_fold": (("dvb", 300, 6.0), dict(path="passes", fold=False), None),
    "fold_bodies": (("fold", 260, 6.0), dict(path="passes"), None),
    "small_9": (("wlan", 9, 6.0), dict(path="passes"), None),
    "small_24": (("wlan", 24, 6.0), dict(path="passes"), None),
    "generic": (("wlan", 24, 6.0), dict(path="passes", force_generic=True), None),
    "check16_var8_small": (("mixed", 24, 6.0), dict(path="passes"), None),
    "check16_var16_small": (("mixed16", 24, 6.0), dict(path="passes"), None),
    "check16_var8": (("mixed", 260, 9.0), dict(path="passes"), None),
    "check16_var16": (("mixed16", 260, 9.0), dict(path="passes"), None),
    "check16_var8_fused": (("mixed", 260, 9.0), dict(path="fused"), None),
}


def _ib_decode(dec, ch, early, dt):
    it = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    out = dec.decode(torch.from_numpy(np.array(ch)).to(DEV).to(dt).contiguous(), out_dtype=dt, early_stop=early,
                     iters=it)
    torch.cuda.synchronize()
    assert out.dtype == dt
    return out.cpu().numpy().astype(np.int32), int(it.item())


@pytest.mark.parametrize("run", list(IB_RUNS))
def test_ib(eng, run, monkeypatch):
    (name, B, ebn0), kw, ncw = IB_RUNS[run]
    assert (name, B, ebn0) in cw.IB_CASES
    if ncw is not None:
        monkeypatch.setenv("IBL_FUSED_NCW", ncw)
    tb, ch, _, C = cw.flood_input(name, B, ebn0)
    ref, ref_it = cw.flood_ref(name, B, ebn0, "ib")
    assert 0 < ref_it < IMAX - 1
    dec = eng.IBDecoder(device_graph(eng, name), tb, cw.ib_match(name), B, **kw)
    generic = bool(kw.get("force_generic"))
    assert dec.fast_path == (not generic) and dec.fused == (kw["path"] == "fused")
    if ncw is not None:
        assert dec.fused_ncw(B) == int(ncw)
    if name in ("dvb", "fold") and kw.get("fold", True):
        assert dec.folded > 0
    if kw.get("fold") is False:
        assert dec.fold is False
    if not dec.fused and not generic:
        assert (B <= dec.small_batch) == (B <= 24)
    for dt in (torch.uint8, torch.int32):
        out, it = _ib_decode(dec, ch, True, dt)
        print(f"{run} {dt}: stop {it} (reference {ref_it}), mismatches {int((out != ref).sum())}")
        assert it == ref_it
        assert np.array_equal(out, ref)
        assert np.array_equal(out < cw.T_CH // 2, C == 1)
    full, full_it = cw.flood_ref(name, B, ebn0, "ib", early=False)
    out, it = _ib_decode(dec, ch, False, torch.uint8)
    assert it == full_it and np.array_equal(out, full)


# ---------------------------------------------------------------------------------------------------------------
# flooding float decoders
# ---------------------------------------------------------------------------------------------------------------
KINDS = {"minsum": (oracle.MINSUM, {}, "ms"), "bp": (oracle.BP, {}, "bp"),
         "corrected": (oracle.MINSUM, dict(alpha=cw.CORRECTED[0], beta=cw.CORRECTED[1]), "corr")}
PRECS = {"fp32": (torch.float32, np.float32), "fp64": (torch.float64, np.float64)}
FLOAT_RUNS = {"passes": ("mixed", 260, "passes"), "passes_fold": ("dvb", 300, "passes"),
              "small_24": ("mixed", 24, "passes"), "small_5": ("mixed", 5, "passes"), "fused": ("wlan", 70, "fused")}


def _family(kind, prec):
    return "bp64" if kind == "bp" else KINDS[kind][2] + prec[2:]


def _float_decode(dec, llr, early, tdt):
    it = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    out = dec.decode(torch.from_numpy(np.array(llr)).to(DEV).to(tdt), early_stop=early, iters=it)
    torch.cuda.synchronize()
    assert out.dtype == tdt
    return out.cpu().numpy(), int(it.item())


def _float_compare(out, ref, kind, prec, what):
    if kind != "bp":
        assert out.dtype == ref.dtype and np.array_equal(out, ref), what
    elif prec == "fp64":
        np.testing.assert_allclose(out, ref, rtol=0, atol=1e-9, err_msg=what)
    else:
        o = out.astype(np.float64)
        bad = _h5(o, ref)
        assert bad.sum() == 0, f"{what}: {bad.sum()} LLRs outside H5, max |x-y| {np.abs(o - ref).max():.3e}"
        assert _hard_flips(o, ref) == 0, what


def _float_case(eng, dec, name, B, ebn0, kind, prec):
    """Decode the mirrored case with and without the early stop and compare with the family's reference."""
    tdt, ndt = PRECS[prec]
    family = _family(kind, prec)
    _, _, llr, C = cw.flood_input(name, B, ebn0)
    ref, ref_it = cw.flood_ref(name, B, ebn0, family)
    assert 0 < ref_it < IMAX - 1
    if kind == "bp" and prec == "fp32":     # the fp64 formula overflows where the fp32 one does not
        assert cw.bp_oracle_is_the_true_boxplus(cw.code(name)[1], llr)
    out, it = _float_decode(dec, llr.astype(ndt), True, tdt)
    print(f"{name} B={B} {ebn0} dB {kind} {prec}: stop {it} (reference {ref_it})")
    assert it == ref_it
    _float_compare(out, ref, kind, prec, "early stop")
    assert np.array_equal(out < 0, C == 1)
    full, full_it = cw.flood_ref(name, B, ebn0, family, early=False)
    out, it = _float_decode(dec, llr.astype(ndt), False, tdt)
    assert it == full_it
    _float_compare(out, full, kind, prec, "fixed iterations")


@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("run", list(FLOAT_RUNS))
def test_float(eng, run, kind, prec):
    name, B, path = FLOAT_RUNS[run]
    k, corr, _ = KINDS[kind]
    dec = eng.FloatDecoder(device_graph(eng, name), k, IMAX, B, precision=PRECS[prec][0], path=path, **corr)
    assert dec.fused == (path == "fused")
    if path == "passes":
        assert (B <= dec.small_batch) == (B <= 24)
    if name == "dvb":
        assert dec.folded > 0
    _float_case(eng, dec, name, B, cw.float_db(name, B, _family(kind, prec)), kind, prec)


@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_float_fused_past_the_first_group(eng, kind, prec):
    """tests/test_gpu_minsum_corrected.py's recipe: B = 2 x (codewords per group) x grid + 5 read from the device's
    geometry, so every workgroup runs a second group and the last group is ragged; 12 dB (BP: 7.3 dB,
    cw.fused_groups_db), where the reference stops before imax - 1 (asserted on the reference, for the B this
    device gives)."""
    cwl = 4 if prec == "fp32" else 2
    cap = 16384
    k, corr, _ = KINDS[kind]
    dec = eng.FloatDecoder(device_graph(eng, "wlan"), k, IMAX, cap, precision=PRECS[prec][0], path="fused", **corr)
    _, grid = dec.fused_geometry(cap)
    B = 2 * cwl * grid + 5
    assert dec.fused and grid > 0 and B <= cap, (grid, B)
    assert dec.fused_geometry(B) == (2 * grid + -(-5 // cwl), grid)
    _float_case(eng, dec, "wlan", B, cw.fused_groups_db(_family(kind, prec)), kind, prec)


# ---------------------------------------------------------------------------------------------------------------
# layered decoders: per-codeword stop on stop_spread_batch
# ---------------------------------------------------------------------------------------------------------------
def _layered_decode(dec, x, early, **kw):
    it = torch.full((x.shape[1],), -1, dtype=torch.int32, device=dec.device)
    out = dec.decode(torch.from_numpy(np.array(x, order="C")).to(dec.device), early_stop=early, iters=it, **kw)
    return out.cpu().numpy(), it.cpu().numpy()


def _layered_check(dec, x, bits, ref, what, early=True, **kw):
    out, it = _layered_decode(dec, x, early, **kw)
    r_out, r_it = ref
    if out.dtype == np.float32 and r_out.dtype == np.int8:
        r_out = dequantise(r_out, dec.scale)
    print(f"{what} early={early} B={x.shape[1]} -> {out.dtype}: iterations {np.bincount(r_it).tolist()}, equal "
          f"{np.array_equal(it, r_it)}, out mismatches {int((out != r_out).sum())}")
    assert np.array_equal(it, r_it)
    assert out.dtype == r_out.dtype and np.array_equal(out, r_out)
    if early:
        conv = cw.converged(r_it)
        assert conv.any() and np.array_equal((out < 0)[:, conv], (bits == 1)[:, conv])
    return out, it


def _layered(eng, name, path, B=cw.LAYERED_B, **kw):
    _, _, layers, _ = cw.code(name)
    dec = eng.LayeredDecoder(device_graph(eng, name), layers, cw.IMAX_LAYERED, B, alpha=cw.ALPHA_LAYERED, path=path,
                             **kw)
    assert dec.path_in_use == path and dec.wide == (name in ("wide_mixed", "small30"))
    return dec


@pytest.mark.parametrize("name", ["wlan", "mixed", "wide_mixed"])
def test_layered_fused(eng, name):
    dec = _layered(eng, name, "fused")
    llr, bits, _ = cw.layered_input(name)
    _layered_check(dec, llr, bits, cw.layered_ref(name), f"{name} fused")
    _layered_check(dec, llr, bits, cw.layered_ref(name, early=False), f"{name} fused", early=False)


def test_layered_fused_group_loop(eng):
    """tests/test_gpu_layered.py test_group_loop's batch (every workgroup decodes a second and a third group, the
    last group ragged) filled with stop_spread_batch: 64 columns spread over the batch, the last ones included."""
    H, g, layers, _ = cw.code("wlan")
    G = device_graph(eng, "wlan")
    cap = 20000
    dec = eng.LayeredDecoder(G, layers, cw.IMAX_LAYERED, cap, alpha=cw.ALPHA_LAYERED)
    per, _, grid = dec.geometry(cap)
    B = per * (2 * grid + 1) + 1
    assert B <= cap, f"B = {B} codewords (cw_per_group {per}, grid {grid}) exceeds {cap}"
    assert dec.geometry(B) == (per, 2 * grid + 2, grid)
    llr, bits, kinds = cw.layered_input("wlan", B)
    third = 2 * per * grid
    cols = np.unique(np.concatenate([np.linspace(0, third - 1, 64 - (B - third)).astype(np.int64),
                                     np.arange(third, B)]))
    assert cols.size == 64 and len(set(kinds[cols].tolist())) >= 3
    ref = layered_decode(H, layers, llr[:, cols], cw.IMAX_LAYERED, cw.ALPHA_LAYERED, 0.0)
    assert len(set(ref[1].tolist())) >= 3
    out, it = _layered_decode(dec, llr, True)
    assert np.array_equal(it[cols], ref[1]) and np.array_equal(out[:, cols], ref[0])
    conv = cw.converged(it)
    assert conv.sum() >= B // 2 and np.array_equal((out < 0)[:, conv], (bits == 1)[:, conv])


@pytest.mark.parametrize("form", ["gather", "packed"])
def test_layered_per_layer_syndrome_forms(eng, monkeypatch, form):
    """dvb with its residue layers, B = 130 (three tiles, the last of two columns), both syndrome forms."""
    monkeypatch.setenv("IBL_LAY_SYNDROME", form)
    dec = _layered(eng, "dvb", "passes")
    llr, bits, _ = cw.layered_input("dvb")
    _layered_check(dec, llr, bits, cw.layered_ref("dvb"), f"dvb {form}")
    _layered_check(dec, llr, bits, cw.layered_ref("dvb", early=False), f"dvb {form}", early=False)


@pytest.mark.parametrize("name,compact", [("dvb", True), ("dvb", (1, 1)), ("small30", (1, 1)), ("wide_mixed", None)])
def test_layered_per_layer_compaction(eng, name, compact):
    """The per-layer path with the running codewords moved together (dvb: the default pair and after every
    iteration; small30: the wide state), at least once (compaction_stats equals the restated policy's count and
    extent); wide_mixed without."""
    dec = _layered(eng, name, "passes", compact=compact)
    llr, bits, _ = cw.layered_input(name)
    ref = cw.layered_ref(name)
    _layered_check(dec, llr, bits, ref, f"{name} compact={compact}")
    if compact is None:
        assert dec.compaction_stats() == (0, cw.LAYERED_B)
    else:
        every, pct = dec.compaction
        events, extent, _ = cr.compactions(ref[1], cw.LAYERED_B, cw.IMAX_LAYERED, every, pct)
        print("policy", events, "-> extent", extent, "device", dec.compaction_stats())
        assert len(events) >= 1 and dec.compaction_stats() == (len(events), extent)
    _layered_check(dec, llr, bits, cw.layered_ref(name, early=False), f"{name} compact={compact}", early=False)


@pytest.mark.parametrize("params", lw.FIXED_PARAMS)
@pytest.mark.parametrize("name", cw.FIXED_CODES)
def test_layered_fixed_point(eng, name, params):
    """float32 and int8 in and out (the int8 input is the quantised float input, the float32 output the int8 output
    divided by scale); fixed iterations float32 -> float32 and int8 -> int8."""
    _, _, layers, _ = cw.code(name)
    a16, bq, qm, scale = params
    dec = eng.LayeredFixedDecoder(device_graph(eng, name), layers, cw.IMAX_LAYERED, cw.LAYERED_B, alpha16=a16,
                                  beta_q=bq, q_max=qm, scale=scale)
    assert dec.path_in_use == "passes"
    x, bits, _ = cw.layered_input(name)
    xq = quantise(x, scale)
    for early in (True, False):
        ref = cw.fixed_ref(name, params, early=early)
        for src in (x, xq):
            for dt in (torch.float32, torch.int8):
                if early or (src is x) == (dt is torch.float32):
                    _layered_check(dec, src, bits, ref, f"{name} {params} {src.dtype}", early=early, out_dtype=dt)
