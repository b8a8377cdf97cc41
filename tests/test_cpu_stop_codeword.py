"""CPU: the premises of tests/test_gpu_stop_codeword.py on the oracles alone, so that its cases cannot pass
vacuously, and what the per-codeword stop offers without a device (header symbol, argument validation).

For each batch the GPU tests decode (tests/_stop_codeword.py): the per-column stops spread inside the groups a
workgroup holds (IB 8 or 4, float 4 fp32 / 2 fp64 codewords), some column never stops, some whole group stops early,
and the batch-global stop of the same batch is imax - 1, so a decoder that kept the batch rule would fail the
comparison."""
import os
import re

import numpy as np
import pytest

from tests import _codewords as cw
from tests import _stop_codeword as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LM = sc.IMAX - 1


def _groups(it, n):
    """Stop passes of the whole groups of n consecutive columns (group g = columns n g .. n g + n - 1)."""
    full = (len(it) // n) * n
    return np.asarray(it[:full]).reshape(-1, n)


@pytest.mark.parametrize("B", [24, 23])
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_spread_batch_premises(family, B):
    llr, _, kinds = sc.spread_input(B)
    out, it = sc.spread_ref(family, B)
    H = cw.code(sc.NAME)[0]
    print(f"{family} B={B}: per-column stops {it.tolist()}")
    assert it.min() >= 1 and it.max() == LM
    # a group of 4 holds three distinct stops; a group of 2 can hold two at the most
    assert max(len(set(g)) for g in _groups(it, 4)) >= 3
    assert max(len(set(g)) for g in _groups(it, 2)) == 2
    # a column that never stops: imax - 1 iterations and still unsatisfied
    never = (it == LM) & sc.unsatisfied(out, H)
    assert never.any() and never[kinds == cw.KIND_NOISE].all()
    # a running and a stopped column side by side, and a whole group (of 2) that stops before imax - 1
    assert any(g.max() < LM for g in _groups(it, 2))
    assert any(g.min() < LM and g.max() == LM for g in _groups(it, 4))
    # the batch rule stops nowhere before imax - 1
    assert sc.batch_stop(family, llr) == LM


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_every_second_tile_stops_early(family):
    """B = 130: columns 64..127 are all codewords at 6 dB, so whole groups of 4 and of 2 leave early there while
    the tiles around them hold columns that never stop."""
    out, it = sc.spread_ref(family, 130)
    assert it[64:128].max() < LM and it[:64].max() == LM
    assert len(set(it[64:128].tolist())) >= 2
    assert sc.batch_stop(family, sc.spread_input(130)[0]) == LM


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_high_snr_batch_stops_at_the_first_pass(family):
    B = 70
    out, it = sc.high_ref(family, B)
    print(f"{family} {sc.high_db(family)} dB: stops {np.bincount(it).tolist()}")
    assert (it == 1).any() and it.max() < LM
    if family != "bp64":     # 12 dB: every column at the first possible pass
        assert (it == 1).all()
    C = cw.codewords(sc.NAME, B)
    assert np.array_equal(out < 0, C == 1)


@pytest.mark.parametrize("name", list(sc.IB_CODES))
def test_ib_batch_premises(name):
    H = sc.ib_code(name)[0]
    out, it = sc.ib_ref(name)
    _, _, kinds = sc.ib_input(name)
    print(f"{name}: stops {np.bincount(it).tolist()}, first columns {it[:16].tolist()}")
    assert it.min() >= 1 and it.max() == LM
    assert max(len(set(g)) for g in _groups(it, 8)) >= 3 and max(len(set(g)) for g in _groups(it, 4)) >= 3
    never = (it == LM) & sc.ib_unsatisfied(out, H)
    assert never.any() and never[kinds == cw.KIND_NOISE].all()
    # whole groups of 8 that stop before imax - 1 (the tiles of early stoppers), and mixed ones
    assert any(g.max() < LM for g in _groups(it, 8))
    assert any(g.min() < LM and g.max() == LM for g in _groups(it, 8))
    assert sc.ib_batch_stop(name) == LM
    if name == "reg39":     # stops from pass 1 on, and a single group of 8 spanning 1 .. imax - 1
        assert (it == 1).any()
        assert any(g.min() == 1 and g.max() == LM for g in _groups(it, 8))


def test_ib_small_batch_premises():
    """B = 24 (the same-handle cross-check) and imax 1 / 2."""
    out, it = sc.ib_ref("wlan", 24)
    assert len(set(it.tolist())) >= 4 and it.max() == LM and sc.ib_batch_stop("wlan", 24) == LM
    for imax in (1, 2):
        assert (sc.ib_ref("wlan", 24, imax)[1] == imax - 1).all()


def test_imax_one_and_two():
    llr = sc.spread_input(24)[0]
    for imax in (1, 2):
        for family in ("ms32", "bp64"):
            _, it = sc.decode_columns(family, llr, imax=imax)
            assert (it == imax - 1).all()


def test_header_declares_the_entry_point():
    from informationbottleneckdecodingldpc_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ibldpc.h")).read()
    assert "Per-codeword stop" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    norm = lambda s: [" ".join(a.split()) for a in s.split(",")]
    L = _lib.load()
    for fam, dt in (("float", _lib.IBL_F32), ("ib", _lib.IBL_U8)):
        m = re.search(r"int\s+ibl_%s_decode_each\s*\(([^)]*)\)" % fam, code)
        assert m, f"ibl_{fam}_decode_each is not declared"
        # the arguments of the family's decode without early_stop
        ref = re.search(r"int\s+ibl_%s_decode\s*\(([^)]*)\)" % fam, code).group(1)
        assert norm(m.group(1)) == [a for a in norm(ref) if a != "int32_t early_stop"]
        assert f"ibl_{fam}_decode_each" in _lib.EXPORTS
        assert getattr(L, f"ibl_{fam}_decode_each")(None, None, dt, 1, None, dt, None, None) == _lib.IBL_EINVAL
        assert b"NULL" in L.ibl_last_error()


def test_the_entry_point_reads_no_environment():
    """tests/test_cpu_host.py's rule for the decode functions, on the new ones: nothing a decode computes or costs
    depends on an environment variable read at decode time."""
    csrc = os.path.join(ROOT, "informationbottleneckdecodingldpc_amd", "csrc")
    for fn, pats, run in (
            ("capi_float.hip", (r"\nint\nibl_float_decode_each\(.*?\n}\n", r"\nint float_each_fused\(.*?\n}\n",
                                r"\nFlFusedArgs float_fused_args\(.*?\n}\n",
                                r"\nstatic int float_decode_check\(.*?\n}\n"), "float_each_fused"),
            ("capi_ib.hip", (r"\nint\nibl_ib_decode_each\(.*?\n}\n", r"\nint ib_each_fused\(.*?\n}\n",
                             r"\nIbFusedArgs ib_fused_args\(.*?\n}\n", r"\nstatic int ib_decode_check\(.*?\n}\n"),
             "ib_each_fused")):
        body = re.sub(r"#if IBL_DIAG.*?#endif", "", open(os.path.join(csrc, fn)).read(), flags=re.S)
        for pat in pats:
            found = re.findall(pat, body, flags=re.S)
            assert len(found) == 1, pat
            for reader in ("getenv", "env_on", "small_batch_env", "fused_vwin"):
                assert reader not in found[0], (pat, reader)
        # one staging launch and one kernel launch: no flag words, no finalize, no second pass
        each = re.findall(r"\nint %s\(.*?\n}\n" % run, body, flags=re.S)[0]
        assert each.count("launch_") == 2 and "launch_finalize" not in each and "flags" not in each


def test_arguments_are_validated_without_a_device():
    from informationbottleneckdecodingldpc_amd import engine
    from informationbottleneckdecodingldpc_amd.bp_decoder_irreg import BeliefPropagationDecoderClassIrregular
    from informationbottleneckdecodingldpc_amd.min_sum_decoder_irreg import Min_Sum_Decoder_class_irregular
    from informationbottleneckdecodingldpc_amd.discrete_LDPC_decoder import Discrete_LDPC_Decoder_class
    from informationbottleneckdecodingldpc_amd.discrete_LDPC_decoder_irreg import Discrete_LDPC_Decoder_class_irregular
    H = cw.code(sc.NAME)[0]
    tb = sc.ib_input("wlan", 24)[0]
    ib_args = {Discrete_LDPC_Decoder_class: (H, sc.IMAX, 16, 16, tb.cn, tb.vn, 8),
               Discrete_LDPC_Decoder_class_irregular: (H, sc.IMAX, 16, 16, tb.cn, tb.vn, tb.match_cn, tb.match_vn, 8)}
    for cls, args in ib_args.items():
        with pytest.raises(ValueError, match="stop"):
            cls(*args, stop="each")
        for stop in ("batch", "codeword"):
            d = cls(*args, stop=stop)
            assert d.stop == stop and d.last_iters is None
        assert cls(*args).stop == "batch"
    with pytest.raises(TypeError):
        Discrete_LDPC_Decoder_class(*ib_args[Discrete_LDPC_Decoder_class], "codeword")     # keyword-only
    for dcls in (engine.FloatDecoder, engine.IBDecoder):     # no handle: the mode is checked before anything else
        dec = object.__new__(dcls)
        for bad in ("batch", "each", ""):
            with pytest.raises(ValueError, match="early_stop"):
                dcls.decode(dec, None, early_stop=bad)
        dec._h = None
    for cls in (Min_Sum_Decoder_class_irregular, BeliefPropagationDecoderClassIrregular):
        with pytest.raises(ValueError, match="stop"):
            cls(H, sc.IMAX, 16, 8, stop="each")
        with pytest.raises(TypeError):
            cls(H, sc.IMAX, 16, 8, np.float32, 150.0, 1.0, 0.0, "codeword")     # keyword-only
        for stop in ("batch", "codeword"):
            d = cls(H, sc.IMAX, 16, 8, stop=stop)
            assert d.stop == stop and d.last_iters is None
        assert cls(H, sc.IMAX, 16, 8).stop == "batch"
