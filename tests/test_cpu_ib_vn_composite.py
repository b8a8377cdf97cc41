"""CPU: the host side of the IB variable chains' composite final step (csrc/plan.h ib_vn_slots, ib_vn_composite_degree,
ib_vn_composite_pass) under AddressSanitizer and UndefinedBehaviorSanitizer — a stand-alone program,
tests/asan/vn_composite_image_check.cpp; nothing loaded into Python is sanitized.

The image: every one of its 256 x 16 nibbles equals F[L[t, m], y], with L and F read from the reference-layout
vectors by numpy alone (raw table D - 3, and raw table D - 2 through the matching row of degree D). The plan: the
tables and final slots of the image of a list of variables, which degree gets the composite, and whether its 64 KiB
fit the LDS behind those tables."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from informationbottleneckdecodingldpc_amd import codes, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("asan") / "vn_composite_image_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "informationbottleneckdecodingldpc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "asan", "vn_composite_image_check.cpp"), "-o", exe], check=True)
    return exe


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return json.loads(r.stdout)


def raw_table(tb, k, l):
    """Raw table l of variable pass k, [T][T], from the reference layout (alphabets Tc = T): VM tables of T x T a
    pass."""
    T, VM = tb.T, tb.VM
    base = k * VM * T * T + l * T * T
    return np.asarray(tb.vn[base: base + T * T]).reshape(T, T)


@pytest.mark.parametrize("k", [0, 2], ids=["pass0", "pass2"])
@pytest.mark.parametrize("match", [True, False], ids=["match", "nomatch"])
@pytest.mark.parametrize("T,VM,D", [(16, 8, 8), (16, 8, 5), (8, 8, 8), (8, 6, 6), (16, 7, 7)])
def test_vn_composite_image_is_the_composition(checker, tmp_path, T, VM, D, match, k):
    tb = tables.random_tables(T, T, 4, VM, 4, seed=100 * T + 10 * VM + D)
    assert tb.vn.size == tb.imax * VM * T * T
    f = tmp_path / "t.bin"
    with open(f, "wb") as fh:
        np.array([T, VM, int(match), k, D, tb.vn.size, tb.match_vn.size], np.int32).tofile(fh)
        np.asarray(tb.vn, np.int32).tofile(fh)
        np.asarray(tb.match_vn, np.int32).tofile(fh)
    img = np.array(run(checker, "image", f)["img"], dtype=np.uint64)
    assert img.shape == (512,)
    # nibble y of entry (t, m): dword y >> 3 (img[256 h + 16 t + m]), nibble y & 7
    got = np.empty((16, 16, 16), dtype=np.int64)
    for y in range(16):
        got[:, :, y] = ((img[256 * (y >> 3):256 * (y >> 3) + 256] >> np.uint64(4 * (y & 7))) & np.uint64(15)).reshape(16, 16)
    L = np.zeros((16, 16), dtype=np.int64)
    F = np.zeros((16, 16), dtype=np.int64)
    L[:T, :T] = raw_table(tb, k, D - 3)
    F[:T, :T] = raw_table(tb, k, D - 2)
    if match:
        mrow = np.asarray(tb.match_vn).reshape(tb.imax, VM, T)[k, D - 1]
        F[:T, :T] = mrow[F[:T, :T]]
    want = F[L]   # [t][m][y] = F[L[t, m], y]; the entries an alphabet below 16 pads read L = 0
    np.testing.assert_array_equal(got, want)
    assert got[:T, :T, :T].max() < T and (T == 16 or not got[:, :, T:].any())


def plan(exe, deg, vm, match, tmp_path):
    f = tmp_path / "d.bin"
    with open(f, "wb") as fh:
        np.array([len(deg), vm], np.int32).tofile(fh)
        np.asarray(deg, np.int32).tofile(fh)
    return run(exe, "plan", f, int(match))


def rest_degrees(H):
    """(degrees of all variables, degrees of the variables the IB fold leaves to the variable pass): a degree-2
    variable folds iff in both of its checks its edge is one of the last two inputs (ascending column order) of a
    check of degree >= 3 — the rule of csrc/plan.h plan_ib_fold, restated."""
    A = codes.canonical_csr(H)
    vdeg = np.bincount(A.indices, minlength=A.shape[1])
    tail = np.zeros(A.shape[1], dtype=np.int64)
    for c in range(A.shape[0]):
        cols = A.indices[A.indptr[c]:A.indptr[c + 1]]
        if len(cols) >= 3:
            tail[cols[-2:]] += 1
    folded = (vdeg == 2) & (tail == 2)
    return vdeg, vdeg[~folded]


def dvb(D, a, b):
    return codes.dvbs2_structured(seed=3, n=2880 + 360 * (a + b), k=360 * (a + b), groups_hi=a, deg_hi=D, deg_lo=3)


def test_rest_image_of_the_dvbs2_profile(checker, tmp_path):
    """Variable degrees {1: 1, 2: 2879, 3: 2880, 8: 720}, every degree-2 variable folded. With matching the full
    image holds V_0..V_5 and the finals of degrees 2, 3, 8: nine tables, two super-regions, no composite. The rest
    list holds no degree-2 variable: eight tables, the finals of degrees 3 and 8 at slots 6 and 7, one super-region,
    and degree 8 gets the composite."""
    vdeg, rest = rest_degrees(dvb(8, 2, 8))
    assert dict(zip(*map(list, np.unique(vdeg, return_counts=True)))) == {1: 1, 2: 2879, 3: 2880, 8: 720}
    assert len(vdeg) - len(rest) == 2879 and set(rest) == {1, 3, 8}
    full = plan(checker, vdeg, 8, True, tmp_path)
    assert (full["tables"], full["nraw"], full["table_lds"], full["degree"]) == (9, 6, 131072, 0)
    assert full["deg"] == [1, 2, 3, 8] and [full["fslot"][d] for d in (2, 3, 8)] == [6, 7, 8]
    r = plan(checker, rest, 8, True, tmp_path)
    assert (r["tables"], r["nraw"], r["table_lds"], r["degree"]) == (8, 6, 65536, 8)
    assert r["deg"] == [1, 3, 8] and [r["fslot"][d] for d in (3, 8)] == [6, 7]
    # without matching a degree's final table is raw table d - 2: seven tables either way, degree 8 with the fold off too
    for deg in (vdeg, rest):
        n = plan(checker, deg, 8, False, tmp_path)
        assert (n["tables"], n["nraw"], n["degree"]) == (7, 7, 8) and [n["fslot"][d] for d in (3, 8)] == [1, 6]


@pytest.mark.parametrize("D,a,b", [(7, 1, 3), (6, 1, 6), (5, 2, 2)])
def test_rest_image_of_the_smaller_profiles(checker, tmp_path, D, a, b):
    vdeg, rest = rest_degrees(dvb(D, a, b))
    assert set(vdeg) == {1, 2, 3, D} and set(rest) == {1, 3, D}
    r = plan(checker, rest, D, True, tmp_path)
    assert (r["tables"], r["nraw"], r["degree"]) == (D, D - 2, D) and [r["fslot"][d] for d in (3, D)] == [D - 2, D - 1]


def test_a_degree_2_variable_left_in_the_rest_list(checker, tmp_path):
    """(8, 1, 0): 2878 of the 2879 degree-2 variables fold. The one left needs its final table: 6 + 2 = 8 tables with
    matching, still one super-region, the composite beside the degree-2 final. With a degree-3 variable as well the
    count is 9 and the composite is refused."""
    vdeg, rest = rest_degrees(dvb(8, 1, 0))
    assert len(vdeg) - len(rest) == 2878 and sorted(set(rest)) == [1, 2, 8]
    r = plan(checker, rest, 8, True, tmp_path)
    assert (r["tables"], r["degree"]) == (8, 8) and [r["fslot"][d] for d in (2, 8)] == [6, 7]
    r = plan(checker, list(rest) + [3], 8, True, tmp_path)
    assert (r["tables"], r["table_lds"], r["degree"]) == (9, 131072, 0)


def test_degree_choice_and_ties(checker, tmp_path):
    """The degree in 5..8 with the most nodes; ties go to the larger; degrees below 5 never count."""
    assert plan(checker, [3] * 40 + [5] * 12 + [6] * 10, 6, False, tmp_path)["degree"] == 5
    assert plan(checker, [3] * 40 + [5] * 10 + [6] * 10, 6, False, tmp_path)["degree"] == 6
    assert plan(checker, [5] * 4 + [6] * 4 + [7] * 4 + [8] * 4, 8, False, tmp_path)["degree"] == 8
    assert plan(checker, [2] * 50 + [3] * 50 + [4] * 50, 4, False, tmp_path)["degree"] == 0
    assert plan(checker, [3] * 40 + [5] * 20 + [6] * 20 + [7] * 60 + [8] * 20, 8, False, tmp_path)["degree"] == 7


def test_refusals(checker, tmp_path):
    """A variable of degree 9 anywhere in the code: the per-pass kernel is the max-degree-16 one, which has no
    composite body, whatever the pass walks. More than eight tables: two super-regions, no room."""
    assert plan(checker, [3] * 70 + [9] * 10, 9, False, tmp_path)["degree"] == 0
    assert plan(checker, [3] * 70 + [8] * 10, 9, False, tmp_path)["degree"] == 0
    r = plan(checker, [2, 3, 4, 5, 8, 8], 8, True, tmp_path)   # 6 raw + 5 finals
    assert (r["tables"], r["degree"]) == (11, 0)
    r = plan(checker, [3, 8, 8], 8, True, tmp_path)
    assert (r["tables"], r["degree"]) == (8, 8)
