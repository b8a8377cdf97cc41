"""GPU: the decode entry points the way callers use them — one handle for many decodes, channel / output dtypes
other than the decoder's own, buffers at element-aligned offsets, side streams and in-place outputs.

Every other GPU parity test makes a fresh decoder per decode, passes the decoder's own dtype in torch-allocated
(256-byte aligned) buffers on the default stream. The kernels behind ibl_ib_decode / ibl_float_decode branch on
exactly those things: packed rows (small-batch kernels) against ldb rows (per-pass kernels) in the same buffers,
syndrome sites masking the padding codewords of a ragged word (where an earlier, wider batch left its data),
captured pass chains keyed by (B, early stop), cast branches of the float staging and decision kernels, vector
loads and stores gated on pointer alignment.

Reference: the CPU oracles, run independently for every step (tests/_caller_scripts.py; their premises are
asserted without a GPU by tests/test_cpu_callers.py). Bars, as everywhere in the suite:
  * IB: bit-exact cluster ids, equal stop iteration;
  * min-sum fp32 (vs the fp32 oracle) and fp64: bit-exact APP LLRs, equal stop iteration;
  * BP fp64: |x - y| <= 1e-9, equal stop iteration;
  * BP fp32 (no fp32 BP oracle): bit-equal to a FRESH decoder's output with its stop iteration, and SURVEY H5
    (|x - y| <= 1e-5 max(|x|, |y|) + 1e-4) against the fp64 oracle on every codeword the fp64 oracle decodes
    (no decided error) — on a converging step that is the whole batch, and the stop iteration equals the
    oracle's; the codewords of a noise batch that fp64 BP does not decode are where the fp32 and fp64
    trajectories separate (tests/test_gpu_float.py test_float32_bp_wlan1944_converged_codewords), H5 says
    nothing about them.
Every step's outputs and stop iteration are read back before the next step is issued.
"""
import ctypes

import numpy as np
import pytest
import torch

from informationbottleneckdecodingldpc_amd import _lib, tables
from oracle import oracle
from tests import _caller_scripts as cs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MINSUM, BP = cs.MINSUM, cs.BP
F32, F64, U8, I32 = torch.float32, torch.float64, torch.uint8, torch.int32
REL, TOL_ABS = 1e-5, 1e-4


@pytest.fixture(scope="module")
def eng():
    from informationbottleneckdecodingldpc_amd import engine
    return engine


@pytest.fixture(scope="module")
def wlan(eng, wlan_H):
    """(edge graph, device graph) of the WLAN N = 1296 fixture code."""
    g = cs.float_wlan(wlan_H).g
    return g, eng.Graph(g, DEV)


def _iters():
    return torch.full((1,), -7, dtype=I32, device=DEV)


# =============================================================== A. scripted reuse: one handle, many decodes
def _ib_step(dec, fam, step, label, dtype=I32):
    """One decode step on `dec`, read back and compared with the oracle (outputs and stop iteration)."""
    kind, B, seed, early = step
    ref, ref_it = fam.ref(step)
    it = _iters()
    ch = torch.tensor(fam.gen(kind, B, seed)).to(DEV).to(dtype)
    out = dec.decode(ch, out_dtype=dtype, early_stop=early, iters=it)
    got, got_it = out.cpu().numpy().astype(np.int32), int(it.item())
    assert got_it == ref_it, f"{label}: stop iteration {got_it}, oracle {ref_it}"
    np.testing.assert_array_equal(got, ref, err_msg=label)


def _run_ib_script(dec, fam, script, label, after_step=None):
    """Decode `script` on the one handle `dec`; int32 and uint8 buffers alternate from step to step."""
    n = 0
    for s in script:
        if not cs.is_decode(s):
            setattr(dec, s[1], s[2])
            continue
        n += 1
        _ib_step(dec, fam, s, f"{label} step {n} {s} small_batch={dec.small_batch}", (I32, U8)[n & 1])
        if after_step is not None:
            after_step(n)


@pytest.mark.parametrize("handle", ["fused", "passes", "passes-thresholds", "generic", "passes-off-first"])
def test_ib_reuse_script(eng, wlan_H, handle):
    """The WLAN reuse script on one handle per decode path: every step equals the oracle although the wider,
    never-stopping batch before it left its columns beside the narrower batch's ragged last word and its
    syndrome flags behind. "passes" alternates between ldb rows (B > 224) and packed rows in the same buffers;
    "passes-thresholds" moves the small-batch threshold between the steps; "passes-off-first" is the short
    script whose first B = 37 decode runs with early stop off, then on."""
    fam = cs.ib_wlan(wlan_H)
    G = eng.Graph(fam.g, DEV)
    dec = eng.IBDecoder(G, fam.tb, True, fam.max_batch, force_generic=handle == "generic",
                        path="fused" if handle == "fused" else "passes")
    assert dec.fast_path == (handle != "generic") and dec.fused == (handle == "fused")
    if handle == "passes":
        assert dec.small_batch == 224
    script = {"passes-thresholds": cs.IB_WLAN_SCRIPT_THRESHOLDS,
              "passes-off-first": cs.IB_WLAN_SCRIPT_OFF_FIRST}.get(handle, cs.IB_WLAN_SCRIPT)
    _run_ib_script(dec, fam, script, handle)
    if handle == "passes-thresholds":
        assert dec.small_batch == 224


def _ib_timing(dec, on):
    L = _lib.load()
    _lib.check(L.ibl_ib_timing(dec._h, int(on)), "ibl_ib_timing")
    if not on:      # read and discard the timers
        cn_ms, vn_ms, cn_n, vn_n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int32(), ctypes.c_int32()
        _lib.check(L.ibl_ib_timing_read(dec._h, ctypes.byref(cn_ms), ctypes.byref(cn_n), ctypes.byref(vn_ms),
                                        ctypes.byref(vn_n)), "ibl_ib_timing_read")
        return cn_n.value, vn_n.value
    return None


def test_ib_reuse_chain_launched_pass_by_pass(eng, wlan_H, monkeypatch):
    """The small-batch chain launched pass by pass instead of replayed from its captured graph — what a handle
    does while timing is on (the benchmark's roofline run) and what a handle created under IBL_SMALL_GRAPH=0
    always does — gives the same results. Timing is switched on for steps 4..7 (the noise batch, then B = 230
    per pass, B = 37 and B = 5 on the small kernels) of a handle that ran the whole script with graphs, then off
    again for a replayed step; the second handle runs the whole script without graphs."""
    fam = cs.ib_wlan(wlan_H)
    G = eng.Graph(fam.g, DEV)
    dec = eng.IBDecoder(G, fam.tb, True, fam.max_batch, path="passes")
    _run_ib_script(dec, fam, cs.IB_WLAN_SCRIPT, "passes")
    _ib_timing(dec, True)
    for n in (4, 5, 6, 7):
        _ib_step(dec, fam, cs.IB_WLAN_SCRIPT[n - 1], f"timing on, step {n}")
    cn_n, vn_n = _ib_timing(dec, False)
    assert cn_n > 0 and vn_n > 0
    for n in (6, 7):
        _ib_step(dec, fam, cs.IB_WLAN_SCRIPT[n - 1], f"timing off again, step {n}")
    monkeypatch.setenv("IBL_SMALL_GRAPH", "0")
    nograph = eng.IBDecoder(G, fam.tb, True, fam.max_batch, path="passes")
    monkeypatch.delenv("IBL_SMALL_GRAPH")
    _run_ib_script(nograph, fam, cs.IB_WLAN_SCRIPT, "IBL_SMALL_GRAPH=0")


def test_ib_fold_reuse_script(eng):
    """The per-pass path with the degree-2 variable fold (second check inbox, fold plan) on one handle: noise,
    converging batches, the fold switched off and on again between decodes, a small-kernel batch in between."""
    fam = cs.ib_fold()
    dec = eng.IBDecoder(eng.Graph(fam.g, DEV), fam.tb, True, fam.max_batch, path="passes")
    assert dec.fast_path and not dec.fused and dec.folded == 3599 and dec.small_batch == 224

    def check(_):
        assert dec.folded == 3599

    _run_ib_script(dec, fam, cs.IB_FOLD_SCRIPT, "fold", after_step=check)
    assert dec.fold is True


def test_ib_chain_eviction(eng, wlan_H):
    """70 (B, early stop off) keys on one handle: more captured chains than a decoder keeps, so they are dropped
    once on the way; then the first keys again (captured anew) and B = 70 with early stop on."""
    fam = cs.ib_evict(wlan_H)
    dec = eng.IBDecoder(eng.Graph(fam.g, DEV), fam.tb, True, fam.max_batch, path="passes")
    assert dec.fast_path and not dec.fused and dec.small_batch >= 70
    _run_ib_script(dec, fam, cs.IB_EVICT_SCRIPT, "evict")


def _h5_bad(out, ref):
    return np.abs(out - ref) > REL * np.maximum(np.abs(out), np.abs(ref)) + TOL_ABS


def _float_step(eng, dec, fam, G, step, label):
    kind, B, seed, early = step
    prec, fp32 = dec.precision, dec.precision == F32
    x = torch.tensor(fam.gen(kind, B, seed)).to(DEV).to(prec)
    it = _iters()
    out = dec.decode(x, early_stop=early, iters=it)
    got, got_it = out.double().cpu().numpy(), int(it.item())
    if dec.kind == BP and fp32:
        fresh = eng.FloatDecoder(G, BP, fam.imax, B, precision=F32, path="fused" if dec.fused else "passes")
        fit = _iters()
        want = fresh.decode(x, early_stop=early, iters=fit).double().cpu().numpy()
        assert got_it == int(fit.item()), f"{label}: stop iteration {got_it}, fresh decoder {int(fit.item())}"
        np.testing.assert_array_equal(got, want, err_msg=label)
        ref, ref_it = fam.ref(step, BP, False)
        if kind == "conv":
            assert got_it == ref_it, f"{label}: stop iteration {got_it}, fp64 oracle {ref_it}"
        ok = (ref < 0).sum(0) == 0            # codewords the fp64 oracle decodes
        if kind == "conv" and early:
            assert ok.all()
        bad = _h5_bad(got[:, ok], ref[:, ok])
        assert bad.sum() == 0, f"{label}: {bad.sum()} LLRs outside H5, max |x-y| {np.abs(got[:, ok] - ref[:, ok]).max():.3e}"
    else:
        ref, ref_it = fam.ref(step, dec.kind, fp32)
        assert got_it == ref_it, f"{label}: stop iteration {got_it}, oracle {ref_it}"
        if dec.kind == MINSUM:
            np.testing.assert_array_equal(got, ref, err_msg=label)
        else:
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9, err_msg=label)
    assert dec.input_violations() == 0, label          # +-inf is legal for min-sum (the poison step)


def _run_float_script(eng, dec, fam, G, script, label):
    n = 0
    for s in script:
        if not cs.is_decode(s):
            if not dec.fused:                  # the fused path ignores the threshold
                setattr(dec, s[1], s[2])
            continue
        n += 1
        _float_step(eng, dec, fam, G, s, f"{label} step {n} {s} small_batch={dec.small_batch}")


@pytest.mark.parametrize("path", ["fused", "passes"])
@pytest.mark.parametrize("prec", [F32, F64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("kind", [MINSUM, BP], ids=["minsum", "bp"])
def test_float_reuse_script(eng, wlan, wlan_H, kind, prec, path):
    """The float reuse script on one handle: wide noise batches (for min-sum also one with +-inf entries, whose
    inf - inf must not leak out of stale lanes) ahead of converging ones, batches on both sides of the
    small-batch threshold (per-pass kernels with the fold above it), early stop off and on, the threshold moved
    between decodes. No violation is counted on any step."""
    g, G = wlan
    fam = cs.float_wlan(wlan_H)
    dec = eng.FloatDecoder(G, kind, fam.imax, fam.max_batch, precision=prec, path=path)
    assert dec.fused == (path == "fused")
    if path == "passes":
        assert dec.folded > 0 and dec.small_batch == 64
    script = cs.FLOAT_SCRIPT_MINSUM if kind == MINSUM else cs.FLOAT_SCRIPT
    _run_float_script(eng, dec, fam, G, script, f"kind={kind} {prec} {path}")


def test_float_chain_eviction(eng, wlan, wlan_H):
    """As test_ib_chain_eviction, for the fp32 min-sum small-batch chains (threshold raised to 1024)."""
    g, G = wlan
    fam = cs.float_evict(wlan_H)
    dec = eng.FloatDecoder(G, MINSUM, fam.imax, fam.max_batch, precision=F32, path="passes")
    dec.small_batch = 1024
    _run_float_script(eng, dec, fam, G, cs.FLOAT_EVICT_SCRIPT, "evict")


# ================================================================================= B. float dtype mixes
_MIX = {}


def _mix_case(g, B, imax=cs.MIX_IMAX, early=False, ebn0=1.5, seed=None):
    key = (B, imax, early, ebn0, seed)
    if key not in _MIX:
        x = cs.mix_llrs(g, B, ebn0, seed)
        _MIX[key] = (x, cs.mix_refs(g, x, imax, early))
    return _MIX[key]


def _assert_mixes(eng, G, g, path, B, imax, early, x64, refs):
    """All eight (decoder precision, LLR dtype, output dtype) combinations of one min-sum decode: an LLR of
    the other dtype is converted to the decoder's precision by round-to-nearest-even (float64 -> fp32; the
    other direction is exact), the decode is the oracle's of the converted values bit for bit, and the result
    is converted to the output dtype the same way."""
    x = {F64: torch.tensor(x64).to(DEV), F32: torch.tensor(x64.astype(np.float32)).to(DEV)}
    for prec in (F32, F64):
        dec = eng.FloatDecoder(G, MINSUM, imax, B, precision=prec, path=path)
        assert dec.fused == (path == "fused")
        for in_dt in (F32, F64):
            ref, ref_it = refs[(prec == F32, in_dt == F32)]
            for out_dt in (F32, F64):
                label = f"{path} B={B} decoder {prec}, LLRs {in_dt}, output {out_dt}"
                it = _iters()
                out = dec.decode(x[in_dt], out_dtype=out_dt, early_stop=early, iters=it)
                assert out.dtype == out_dt
                got = out.cpu().numpy()
                assert int(it.item()) == ref_it, label
                if out_dt == F64:      # fp32 results widen exactly (ref holds them widened)
                    np.testing.assert_array_equal(got, ref, err_msg=label)
                else:                  # fp64 results round to nearest even; fp32 results are unchanged
                    np.testing.assert_array_equal(got, ref.astype(np.float32), err_msg=label)
        assert dec.input_violations() == 0


@pytest.mark.parametrize("B", cs.MIX_BATCHES)
@pytest.mark.parametrize("path", ["fused", "passes"])
def test_float_dtype_mixes(eng, wlan, path, B):
    """i_max = 6, early stop off, unquantised LLRs (not float32-representable, so the conversion shows). B = 3
    and 8: a ragged and a whole word of the fused and small-batch kernels; B = 70 and 72: ragged and aligned
    rows of the per-pass decision kernel (float4 / float2 / double2 stores against the scalar tail)."""
    g, G = wlan
    x64, refs = _mix_case(g, B)
    _assert_mixes(eng, G, g, path, B, cs.MIX_IMAX, False, x64, refs)


@pytest.mark.parametrize("path", ["fused", "passes"])
def test_float_dtype_mixes_early_stop(eng, wlan, path):
    """The same eight combinations on a converging batch with early stop on (i_max = 20): the stop iteration is
    the oracle's for the converted values."""
    g, G = wlan
    e = cs.MIX_EARLY
    x64, refs = _mix_case(g, e["B"], e["imax"], True, e["ebn0"], e["seed"])
    for key, (_, it) in refs.items():
        assert 1 <= it < e["imax"] - 1, (key, it)
    _assert_mixes(eng, G, g, path, e["B"], e["imax"], True, x64, refs)


@pytest.mark.parametrize("path,B", [("fused", 8), ("passes", 72)])
def test_float_bp_fp64_to_f32_output(eng, wlan, path, B):
    """BP fp64 with a float32 output: the device's fp64 result lies within 1e-9 of the oracle's, which can move
    it across one float32 rounding boundary and no further: |out - float32(ref)| <= one float32 spacing."""
    g, G = wlan
    x64 = cs.mix_llrs(g, B)
    ref = oracle.float_decode(g, BP, cs.MIX_IMAX, x64)
    dec = eng.FloatDecoder(G, BP, cs.MIX_IMAX, B, precision=F64, path=path)
    out = dec.decode(torch.tensor(x64).to(DEV), out_dtype=F32, early_stop=False)
    assert out.dtype == F32
    got = out.cpu().numpy().astype(np.float64)
    ref32 = ref.astype(np.float32)
    err = np.abs(got - ref32.astype(np.float64))
    assert (err <= np.spacing(np.abs(ref32)).astype(np.float64)).all(), err.max()
    assert dec.input_violations() == 0


@pytest.mark.parametrize("path,B", [("fused", 8), ("passes", 8), ("passes", 72)])
def test_float_f64_llrs_beyond_float32(eng, wlan, path, B):
    """float64 LLRs of +-1e300 into the fp32 decoders round to +-inf: min-sum (where +-inf is a known bit)
    equals the fp32 oracle on +-inf, and the fp32 BP decoder counts exactly those entries as violations."""
    g, G = wlan
    x64 = cs.mix_llrs(g, B).copy()
    rng = np.random.default_rng(B)
    pos = rng.random(x64.shape) < 0.01
    assert pos.sum() >= 5
    x64[pos] = np.where(rng.random(int(pos.sum())) < 0.5, 1e300, -1e300)
    with np.errstate(over="ignore"):
        x32 = x64.astype(np.float32)
    assert np.isinf(x32).sum() == pos.sum()
    ref = oracle.float32_decode(g, cs.MIX_IMAX, x32).astype(np.float64)
    assert not np.isnan(ref).any() and np.isinf(ref).sum() >= pos.sum()
    xd = torch.tensor(x64).to(DEV)
    ms = eng.FloatDecoder(G, MINSUM, cs.MIX_IMAX, B, precision=F32, path=path)
    got = ms.decode(xd, early_stop=False).double().cpu().numpy()
    np.testing.assert_array_equal(got, ref)
    assert ms.input_violations() == 0
    bp = eng.FloatDecoder(G, BP, cs.MIX_IMAX, B, precision=F32, path=path)
    bp.decode(xd, early_stop=False)
    assert bp.input_violations(raise_on_error=False) == int(pos.sum())


# ========================================================================================= C. offsets
_SENTINEL = {U8: 0xAB, I32: -123456789, F32: -7.25e7, F64: -7.25e7}


class _Offset:
    """A contiguous [n][B] view `off` bytes into a sentinel-filled buffer (the buffer itself 256-byte aligned),
    with the elements before and after the view checked afterwards."""

    def __init__(self, n, B, dtype, off):
        es = torch.empty(0, dtype=dtype).element_size()
        assert off % es == 0                     # the documented requirement: the element type's alignment
        k, tail = off // es, 64
        self.buf = torch.full((k + n * B + tail,), _SENTINEL[dtype], dtype=dtype, device=DEV)
        self.view = self.buf[k:k + n * B].view(n, B)
        self.k, self.end = k, k + n * B
        assert self.buf.data_ptr() % 256 == 0 and self.view.data_ptr() % 256 == off and self.view.is_contiguous()

    def assert_surroundings_untouched(self, label):
        s = _SENTINEL[self.buf.dtype]
        assert bool((self.buf[:self.k] == s).all()) and bool((self.buf[self.end:] == s).all()), \
            f"{label}: elements outside the [N][B] view were written"


@pytest.fixture(scope="module")
def ib_offset_setup(eng, wlan):
    """Random T = 16 tables (i_max = 4), one decoder per path for up to 272 codewords, and the oracle's decode
    of each batch size (computed once, read-only)."""
    g, G = wlan
    tb = tables.random_tables(16, 16, g.d_c_max, g.d_v_max, 4, seed=31)
    decs = {p: eng.IBDecoder(G, tb, True, 272, path=p) for p in ("passes", "fused")}
    assert decs["passes"].small_batch == 224 and decs["fused"].fused
    data = {}
    for B in (64, 264, 272):
        ch = np.random.default_rng(500 + B).integers(0, 16, (g.n_v, B)).astype(np.int32)
        ref = oracle.ib_decode(g, tb, ch, match=True, early_stop=False)
        ch.setflags(write=False)
        ref.setflags(write=False)
        data[B] = (ch, ref)
    return decs, data


# (B, channel dtype, channel byte offset, output dtype, output byte offset). B = 264 is 33 words, the first
# size the per-pass path stages with the vector kernel (up to 256 it stages word by word); B = 272 has
# B % 16 == 0, so a base of 8 mod 16 takes the one-word vector loads and not the four-word ones; B = 64 runs
# the small-batch decision kernel on path="passes". Output offsets leave B % 4 == 0, so only the pointer
# clears the vector stores.
IB_OFFSET_CASES = [
    (264, U8, 1, I32, 0), (264, U8, 8, I32, 0), (272, U8, 8, U8, 0),
    (264, I32, 4, I32, 0), (264, I32, 8, I32, 0),
    (264, U8, 0, U8, 1), (264, U8, 0, U8, 2), (264, I32, 0, I32, 4),
    (264, U8, 0, I32, 0), (264, I32, 0, U8, 0),
    (64, U8, 0, U8, 1), (64, I32, 0, I32, 4),
]


@pytest.mark.parametrize("B,ch_dt,ch_off,out_dt,out_off", IB_OFFSET_CASES,
                         ids=[f"B{c[0]}-{str(c[1])[6:]}+{c[2]}-{str(c[3])[6:]}+{c[4]}" for c in IB_OFFSET_CASES])
@pytest.mark.parametrize("path", ["passes", "fused"])
def test_ib_offset_buffers(ib_offset_setup, wlan, path, B, ch_dt, ch_off, out_dt, out_off):
    """Channel and output buffers at byte offsets that keep only the element type's alignment: the decode
    equals the oracle and writes nothing outside the [N][B] output elements."""
    g, _ = wlan
    decs, data = ib_offset_setup
    ch, ref = data[B]
    src, dst = _Offset(g.n_v, B, ch_dt, ch_off), _Offset(g.n_v, B, out_dt, out_off)
    src.view.copy_(torch.tensor(ch).to(DEV))
    label = f"{path} B={B} channel {ch_dt}+{ch_off} output {out_dt}+{out_off}"
    out = decs[path].decode(src.view, out=dst.view, early_stop=False)
    assert out.data_ptr() == dst.view.data_ptr()
    np.testing.assert_array_equal(out.cpu().numpy().astype(np.int32), ref, err_msg=label)
    dst.assert_surroundings_untouched(label)
    np.testing.assert_array_equal(src.view.cpu().numpy().astype(np.int32), ch, err_msg=label + " (channel changed)")


# (decoder precision, LLR dtype, LLR byte offset, output dtype, output byte offset): each offset keeps the
# element's alignment and breaks the vector width (16 bytes; 8 for the fp64 decoder's float2 stores)
FLOAT_OFFSET_CASES = [(F32, F32, 4, F32, 0), (F64, F64, 8, F64, 0), (F32, F32, 0, F32, 4), (F64, F64, 0, F64, 8),
                      (F64, F64, 0, F32, 4)]


@pytest.mark.parametrize("prec,in_dt,in_off,out_dt,out_off", FLOAT_OFFSET_CASES,
                         ids=[f"{str(c[0])[6:]}-{str(c[1])[6:]}+{c[2]}-{str(c[3])[6:]}+{c[4]}"
                              for c in FLOAT_OFFSET_CASES])
@pytest.mark.parametrize("path,B", [("fused", 8), ("passes", 72), ("passes", 8)])
def test_float_offset_buffers(eng, wlan, path, B, prec, in_dt, in_off, out_dt, out_off):
    """Min-sum (i_max = 4) with LLR and output buffers off the vector alignment, whole words (B % 4 == 0) so that
    only the pointer decides: bit-equal to the oracle, nothing written outside the output elements. B = 8 on
    path="passes" takes the small-batch kernels, B = 72 the per-pass ones."""
    g, G = wlan
    x64, refs = _mix_case(g, B, imax=4)
    ref, _ = refs[(prec == F32, in_dt == F32)]
    src, dst = _Offset(g.n_v, B, in_dt, in_off), _Offset(g.n_v, B, out_dt, out_off)
    src.view.copy_(torch.tensor(x64).to(DEV).to(in_dt))
    dec = eng.FloatDecoder(G, MINSUM, 4, B, precision=prec, path=path)
    label = f"{path} B={B} decoder {prec} LLRs {in_dt}+{in_off} output {out_dt}+{out_off}"
    out = dec.decode(src.view, out=dst.view, early_stop=False)
    want = ref if out_dt == F64 else ref.astype(np.float32)
    np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=label)
    dst.assert_surroundings_untouched(label)
    assert dec.input_violations() == 0


# ============================================================================ D. streams and in-place
def _decode_on_side_stream(dec, noise, real, dtype):
    """Decode `real` on a side stream behind unrelated work queued there; the input buffer held `noise` until
    a copy on that same stream replaced it, and nothing runs on the default stream meanwhile. A decode kernel
    (or replayed chain) ordered on any other stream reads the noise."""
    x = torch.tensor(noise).to(DEV).to(dtype)
    src = torch.tensor(real).to(DEV).to(dtype)
    out = torch.empty_like(x)
    it = _iters()
    busy = torch.ones(1 << 26, dtype=F32, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(16):                      # a few milliseconds of memory-bound work ahead of the copy
            busy.mul_(1.0001)
        x.copy_(src)
        dec.decode(x, out=out, early_stop=True, iters=it)
    side.synchronize()
    return out, int(it.item())


@pytest.mark.parametrize("path", ["passes", "fused"])
def test_ib_side_stream_and_in_place(eng, wlan_H, path):
    """The converging B = 37 batch (small-batch chain replayed from its captured graph on path="passes") and
    B = 230 (per-pass kernels) on a side stream, then both in place (output buffer = channel buffer, uint8 and
    int32) with no iteration counter requested."""
    fam = cs.ib_wlan(wlan_H)
    dec = eng.IBDecoder(eng.Graph(fam.g, DEV), fam.tb, True, 260, path=path)
    for B in (37, 230):
        assert (path == "passes") == (not dec.fused) and (B <= dec.small_batch) == (B == 37)
        step = ("conv", B, 100 + B, True)
        ref, ref_it = fam.ref(step)
        out, it = _decode_on_side_stream(dec, fam.gen("noise", B, B), fam.gen(*step[:3]), U8)
        assert it == ref_it, (path, B)
        np.testing.assert_array_equal(out.cpu().numpy().astype(np.int32), ref, err_msg=f"{path} B={B} side stream")
        for dt in (U8, I32):
            t = torch.tensor(fam.gen(*step[:3])).to(DEV).to(dt)
            r = dec.decode(t, out=t, early_stop=True, iters=None)
            assert r.data_ptr() == t.data_ptr()
            np.testing.assert_array_equal(t.cpu().numpy().astype(np.int32), ref, err_msg=f"{path} B={B} in place {dt}")


@pytest.mark.parametrize("path", ["passes", "fused"])
def test_float_side_stream_and_in_place(eng, wlan, wlan_H, path):
    """fp32 min-sum: B = 37 (small-batch chain on path="passes") and B = 70 (per-pass kernels with the fold) on
    a side stream, then in place; no violation counted."""
    g, G = wlan
    fam = cs.float_wlan(wlan_H)
    dec = eng.FloatDecoder(G, MINSUM, fam.imax, fam.max_batch, precision=F32, path=path)
    for B in (37, 70):
        step = ("conv", B, 200 + B, True)
        ref, ref_it = fam.ref(step, MINSUM, True)
        out, it = _decode_on_side_stream(dec, fam.gen("noise", B, 300 + B), fam.gen(*step[:3]), F32)
        assert it == ref_it, (path, B)
        np.testing.assert_array_equal(out.double().cpu().numpy(), ref, err_msg=f"{path} B={B} side stream")
        assert dec.input_violations() == 0
        t = torch.tensor(fam.gen(*step[:3])).to(DEV).to(F32)
        r = dec.decode(t, out=t, early_stop=True, iters=None)
        assert r.data_ptr() == t.data_ptr()
        np.testing.assert_array_equal(t.double().cpu().numpy(), ref, err_msg=f"{path} B={B} in place")
        assert dec.input_violations() == 0
