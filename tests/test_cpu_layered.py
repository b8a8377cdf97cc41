"""CPU: the layered min-sum decoder's host side — layer constructions (codes.qc_layers / greedy_layers /
validate_layers), the C ABI's host-only ibl_layers_validate, the device plan (csrc/layered_plan.h) under
AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program, tests/asan/layered_plan_check.cpp; nothing
loaded into Python is sanitized), and the numpy reference the GPU tests compare against: pinned by an independent
scalar restatement (float32, and float64 where the arithmetic is exact), and the inputs of the GPU tests held to
the arithmetic edges they are there for (tests/_layered_census.py)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from informationbottleneckdecodingldpc_amd import codes
from tests import _layered_census as lc
from tests._layered_ref import layered_decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from informationbottleneckdecodingldpc_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    return _lib


@pytest.fixture(scope="module")
def reg96():
    return codes.regular_code(96, 3, 6, seed=1)


def as_sets(layers):
    return [frozenset(int(c) for c in l) for l in layers]


@pytest.mark.parametrize("Z", [27, 81])
def test_qc_layers_are_the_block_rows(Z):
    H = codes.wlan_80211n(Z)
    layers = codes.qc_layers(H, Z)
    assert len(layers) == 12 and all(len(l) == Z for l in layers)
    assert [int(l[0]) for l in layers] == [i * Z for i in range(12)]
    codes.validate_layers(H, layers)
    # taking checks in row order, every check of a block row conflicts with none of its own row and with some
    # check of every earlier block row: the greedy partition is the block rows
    assert as_sets(codes.greedy_layers(H)) == as_sets(layers)
    with pytest.raises(ValueError):
        codes.qc_layers(H, Z + 1)


def test_greedy_layers_uneven(reg96):
    layers = codes.greedy_layers(reg96)
    codes.validate_layers(reg96, layers)
    assert [len(l) for l in layers] == [8, 8, 7, 7, 7, 6, 3, 2]
    assert sorted(int(c) for l in layers for c in l) == list(range(48))


def bad_layer_cases(H):
    """(name, H, layers, word expected in the message)."""
    A = codes.canonical_csr(H)
    good = [l.tolist() for l in codes.greedy_layers(A)]
    missing = [list(l) for l in good]
    gone = missing[-1].pop()
    dup = [list(l) for l in good]
    dup[-1].append(dup[0][0])
    # two checks of one layer sharing a variable: move a check of layer 1 that conflicts with layer 0 into layer 0
    share = [list(l) for l in good]
    vars0 = set(A.indices[np.concatenate([np.arange(A.indptr[c], A.indptr[c + 1]) for c in good[0]])].tolist())
    mover = next(c for c in good[1] if vars0 & set(A.indices[A.indptr[c]:A.indptr[c + 1]].tolist()))
    share[1].remove(mover)
    share[0].append(mover)
    # a degree-1 check: drop all but the first entry of the last row
    B = A.tolil()
    keep = A.indices[A.indptr[-2]]
    B[A.shape[0] - 1, :] = 0
    B[A.shape[0] - 1, keep] = 1
    B = codes.canonical_csr(B.tocsr())
    return [("missing", A, missing, f"check {gone} is in no layer"),
            ("duplicate", A, dup, f"check {dup[0][0]} is listed twice"),
            ("shared", A, share, f"and {mover} of layer 0 share variable"),
            ("degree1", B, [l.tolist() for l in codes.greedy_layers(B)], f"check {A.shape[0] - 1} has degree 1")]


def test_layers_validate_capi_agrees_with_python(lib, reg96):
    for H in (codes.wlan_80211n(27), codes.wlan_80211n(81), reg96):
        A = codes.canonical_csr(H)
        for layers in (codes.greedy_layers(A), [np.array([c]) for c in range(A.shape[0])]):
            codes.validate_layers(A, layers)
            lib.layers_validate(A.shape[1], A.shape[0], A.indptr, A.indices, layers)
    for name, A, layers, word in bad_layer_cases(reg96):
        with pytest.raises(ValueError) as ep:
            codes.validate_layers(A, layers)
        assert word in str(ep.value), (name, str(ep.value))
        with pytest.raises(lib.IBLError) as ec:
            lib.layers_validate(A.shape[1], A.shape[0], A.indptr, A.indices, layers)
        assert word in str(ec.value), (name, str(ec.value))
        nl, ptr, chk = lib.pack_layers(layers)
        rc = lib.load().ibl_layers_validate(A.shape[1], A.shape[0], A.indptr.astype(np.int32),
                                            A.indices.astype(np.int32), nl, ptr, chk)
        assert rc == (lib.IBL_EUNSUPPORTED if name == "degree1" else lib.IBL_EINVAL), name


@pytest.fixture(scope="module")
def layered_plan_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("asan") / "layered_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "informationbottleneckdecodingldpc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "asan", "layered_plan_check.cpp"), "-o", exe], check=True)
    return exe


def run_plan(exe, H, layers, tmp_path):
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
    r = subprocess.run([exe, str(f)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout)
    assert out["failures"] == 0
    return out


@pytest.mark.parametrize("name", ["wlan27", "wlan81", "reg96"])
def test_layered_plan_under_sanitizers(layered_plan_check, tmp_path, reg96, name):
    H = {"wlan27": lambda: codes.wlan_80211n(27), "wlan81": lambda: codes.wlan_80211n(81), "reg96": lambda: reg96}[name]()
    A = codes.canonical_csr(H)
    layers = codes.greedy_layers(A)
    out = run_plan(layered_plan_check, A, layers, tmp_path)
    deg = np.diff(A.indptr)
    # tasks: per layer and degree, ceil(count / 64)
    want = sum(-(-int((deg[l] == d).sum()) // 64) for l in layers for d in np.unique(deg[l]))
    assert out["valid"] == 0 and out["n_layers"] == len(layers) and out["n_tasks"] == want
    assert out["cw_bytes"] == 4 * A.shape[1] + 12 * A.shape[0]
    assert out["cw_per_group"] == min(8, 160 * 1024 // out["cw_bytes"])
    if name == "wlan81":
        assert out["cw_bytes"] == 19440 and out["cw_per_group"] == 8
    # the refused layer lists go through the same code under the sanitizers
    if name == "reg96":
        for case, B, bad, word in bad_layer_cases(A):
            o = run_plan(layered_plan_check, B, bad, tmp_path)
            assert o["valid"] == (-2 if case == "degree1" else -1) and word in o["error"], (case, o)


def test_reference_noiseless_and_fixed_iterations():
    H = codes.wlan_80211n(27)
    layers = codes.qc_layers(H, 27)
    llr = np.full((H.shape[1], 3), 4.0, np.float32)
    out, iters = layered_decode(H, layers, llr, 6)
    assert iters.tolist() == [1, 1, 1] and (out > 0).all()
    out2, iters2 = layered_decode(H, layers, llr, 6, early_stop=False)
    assert iters2.tolist() == [6, 6, 6] and (out2 > 0).all()
    # plain min-sum on a noiseless word only ever adds positive messages; the correction shrinks them
    out3, it3 = layered_decode(H, layers, llr, 1, alpha=0.75, beta=0.5)
    assert it3.tolist() == [1, 1, 1] and (out3 >= 4.0).all() and (out3 <= out).all() and (out3 < out).any()


# ---------------------------------------------------------------------------------------------------------------
# the reference against an independent scalar restatement
# ---------------------------------------------------------------------------------------------------------------
def small_code(name):
    if name == "wlan27":
        return lc.wlan(27)
    H = codes.regular_code(96, 3, 6, seed=1)
    return H, codes.greedy_layers(H)


SCALAR_INPUTS = ["awgn", "mixed_batch"] + list(lc.FAMILIES)


@pytest.mark.parametrize("family", SCALAR_INPUTS)
@pytest.mark.parametrize("code", ["wlan27", "reg96"])
def test_scalar_restatement_equals_vectorised(code, family):
    """Two restatements of the header that share no code (argmin / put_along_axis against one running scan per
    check) give the same float32 values and iteration counts: all four (alpha, beta), early stop on and off,
    B = 4 (8 for the mixed batch: one column of each kind), 5 iterations."""
    H, layers = small_code(code)
    n = H.shape[1]
    llr_max = 150.0
    params = list(lc.AB)
    if family == "awgn":
        llr = lc.awgn_llr(n, 4, 2.0, seed=40)
    elif family == "mixed_batch":
        llr = lc.mixed_batch_llr(n, 8, seed=41)
    else:
        gen, own = lc.FAMILIES[family]
        llr = gen(H, 4)
        llr_max = own[0][2]
        params += [(a, b) for a, b, _ in own if (a, b) not in params]   # the subnormal beta
    for a, b in params:
        for early in (True, False):
            ref = layered_decode(H, layers, llr, 5, a, b, llr_max, early)
            out, it = lc.layered_decode_scalar(H, layers, llr, 5, a, b, llr_max, early)
            assert out.dtype == np.float32
            assert np.array_equal(it, ref[1]), (a, b, early, it.tolist(), ref[1].tolist())
            assert np.array_equal(out, ref[0]), (a, b, early, int((out != ref[0]).sum()))
            if family == "mixed_batch":   # all-zero columns stop at once with an all-zero output
                z = [lc.MIXED_BATCH_COLUMNS.index(k) for k in ("zeros", "negative_zeros")]
                assert (out[:, z] == 0).all() and (it[z] == (1 if early else 5)).all()


@pytest.mark.parametrize("code", ["wlan27", "reg96"])
def test_sign_of_a_zero_is_immaterial(code):
    """Whether a Q of value zero counts as negative cannot change any value: a zero Q makes m1 = 0, so every
    other edge of the check gets a message of magnitude max(alpha 0 - beta, 0) = 0 whatever its sign, and the
    zero edge's own message takes the XOR of the OTHER edges' signs. A kernel may therefore read neg_e off the
    sign bit of Q whether or not a -0 can occur (csrc/layered_kernels.hip keeps -0 out all the same), and no
    test that compares values can tell: shown here on inputs that are full of zeros of both signs."""
    H, layers = small_code(code)
    for llr in (lc.quantised_llr(H.shape[1], 4, seed=42), lc.mixed_batch_llr(H.shape[1], 8, seed=43)):
        assert (llr == 0).sum() > 20 and np.signbit(llr[llr == 0]).any()
        for a, b in lc.AB:
            for early in (True, False):
                ref = layered_decode(H, layers, llr, 5, a, b, early_stop=early)
                out, it = lc.layered_decode_scalar(H, layers, llr, 5, a, b, early_stop=early, zero_is_negative=True)
                assert np.array_equal(it, ref[1]) and np.array_equal(out, ref[0]), (a, b, early)


def representable_in_f32(x):
    x = np.asarray(x, dtype=np.float64)
    return x.astype(np.float32).astype(np.float64) == x


def exact_in_double(H, layers, llr, imax, a, b):
    """The float64 scalar run equals the float32 reference exactly, and (the premise) every APP value of the
    float64 run is a float32 number after every iteration."""
    for early in (True, False):
        seen = []

        def premise(cw, it, P):
            seen.append(it)
            assert representable_in_f32(P).all(), (a, b, cw, it)

        out64, it64 = lc.layered_decode_scalar(H, layers, llr, imax, a, b, early_stop=early, dtype=np.float64,
                                               on_iteration=premise)
        assert out64.dtype == np.float64 and seen and max(seen) == it64.max()
        assert representable_in_f32(out64).all()
        ref = layered_decode(H, layers, llr, imax, a, b, early_stop=early)
        assert np.array_equal(it64, ref[1])
        assert np.array_equal(out64, ref[0].astype(np.float64)), int((out64 != ref[0]).sum())


@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("code", ["wlan27", "reg96"])
def test_reference_exact_in_double(code, beta):
    """Where no operation rounds, float32 and float64 must agree exactly. LLRs that are multiples of 0.5 in
    [-8, 8] with alpha = 1 and beta in {0, 0.5}: every intermediate is a multiple of 0.5 below 2 llr_max."""
    H, layers = small_code(code)
    half = (np.random.default_rng(50).integers(-16, 17, (H.shape[1], 4)) * 0.5).astype(np.float32)
    exact_in_double(H, layers, half, 8, 1.0, beta)


def stacked_code(n, d, n_layers, seed):
    """n_layers layers, each a random partition of the n variables into n / d checks of degree d."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    per = n // d
    rows = np.concatenate([np.repeat(np.arange(l * per, (l + 1) * per), d) for l in range(n_layers)])
    cols = np.concatenate([rng.permutation(n) for _ in range(n_layers)])
    H = sp.csr_matrix((np.ones(rows.size, np.int64), (rows, cols)), shape=(n_layers * per, n))
    layers = [np.arange(l * per, (l + 1) * per) for l in range(n_layers)]
    codes.validate_layers(H, layers)
    return H, layers


@pytest.mark.parametrize("n_layers,imax", [(2, 3), (3, 2)])
def test_reference_exact_in_double_normalised(n_layers, imax):
    """alpha = 0.75 on integer LLRs in [-8, 8]. A product by 0.75 adds at most two fractional bits, and a value
    passes through at most one product per layer and iteration (a layer's message feeds the next layer's within
    the same iteration), so after imax iterations of a code of n_layers layers it has at most 2 n_layers imax = 12
    fractional bits, and with |value| < 2 llr_max < 2^9 at most 21 significant bits: nothing rounds in float32.
    (On the 12 layers of the WLAN code, or the 8 greedy layers of the (3, 6) code, this bound is 24 or 16 bits
    after ONE iteration, and values of the float64 run are in fact no float32 numbers after the first or second
    iteration, so those codes cannot serve here.) exact_in_double asserts the premise after every iteration."""
    H, layers = stacked_code(96, 6, n_layers, seed=3)
    ints = np.random.default_rng(51).integers(-8, 9, (96, 4)).astype(np.float32)
    exact_in_double(H, layers, ints, imax, 0.75, 0.0)


# ---------------------------------------------------------------------------------------------------------------
# conditions on the inputs of the GPU tests (tests/test_gpu_layered.py decodes the same arrays)
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def census():
    """(code, family, alpha, beta, early) -> counts, computed once per (code, family)."""
    cache = {}

    def get(code, family):
        if (code, family) not in cache:
            H, layers = lc.mixed() if code == "mixed" else lc.wlan(27)
            gen, params = lc.FAMILIES[family]
            llr = gen(H, lc.FAMILY_B)
            runs = {}
            for a, b, L in params:
                for early in (True, False):
                    out, it, cnt = lc.layered_census(H, layers, llr, lc.FAMILY_IMAX, a, b, L, early)
                    ref = layered_decode(H, layers, llr, lc.FAMILY_IMAX, a, b, L, early)
                    assert np.array_equal(out, ref[0]) and np.array_equal(it, ref[1])   # the hook changes nothing
                    runs[(a, b, early)] = cnt
            cache[(code, family)] = runs
        return cache[(code, family)]
    return get


@pytest.mark.parametrize("family", list(lc.FAMILIES))
@pytest.mark.parametrize("code", ["mixed", "wlan27"])
def test_gpu_inputs_reach_their_edges(census, code, family):
    """Each input family of the GPU tests meets the arithmetic edge it exists for, as a fraction of the check
    updates / edges of codewords still running; on the code of degrees 2..16 every run also visits every
    (degree, first-argmin position) pair and moves the argmin of some check of every degree between iterations.
    These are conditions on the inputs: the thresholds do not move, a generator that misses them is wrong."""
    for (a, b, early), c in census(code, family).items():
        tag = (code, family, a, b, early)
        print(tag, {k: v for k, v in c.items() if k not in ("pairs", "argmin_moved")})
        assert c["check_updates"] > 0 and c["edges"] > 2 * c["check_updates"]
        if family == "quantised":
            assert c["ties"] > 0 and c["q_zero"] > 0, tag
            if a == 1.0:
                assert c["ties"] >= 0.10 * c["check_updates"], tag
                assert c["q_zero"] >= 0.01 * c["edges"], tag
            if b > 0:
                assert c["q_zero_mag_zero"] > 0 and c["q_zero_r_negzero"] > 0, tag
        elif family in ("saturating", "small_llr_max"):
            assert c["clamped"] >= 0.05 * c["edges"], tag
        elif family == "subnormal":
            assert c["subnormal_q"] >= 0.50 * c["edges"], tag
            if b > 0:
                assert c["mag_zero"] > 0, tag
        elif family == "subnormal_boundary":
            assert 0 < c["subnormal_q"] < 0.5 * c["edges"], tag   # values on both sides of 2^-126
        if code == "mixed":
            assert c["pairs"] == lc.MIXED_PAIRS, (tag, sorted(lc.MIXED_PAIRS - c["pairs"]))
            assert sorted(c["argmin_moved"]) == lc.MIXED_DEGREES and min(c["argmin_moved"].values()) > 0, tag


def test_mixed_batch_columns():
    """The mixed batch: the all-zero columns (+0.0 and -0.0) stop after one iteration with an all-zero output, the
    constant column ties in every check of the first layer, the random-sign column starts from a non-zero
    syndrome, and the columns stop at unlike times."""
    for H, layers in (lc.mixed(), lc.wlan(27)):
        n = H.shape[1]
        llr = lc.mixed_batch_llr(n, 11, seed=31)
        col = {k: i for i, k in enumerate(lc.MIXED_BATCH_COLUMNS)}
        assert np.signbit(llr[:, col["negative_zeros"]]).all() and not np.signbit(llr[:, col["zeros"]]).any()
        for a, b in lc.AB:
            out, it = layered_decode(H, layers, llr, lc.FAMILY_IMAX, a, b)
            for z in (col["zeros"], col["negative_zeros"]):
                assert it[z] == 1 and (out[:, z] == 0).all()
            assert len(set(it.tolist())) >= 2
        x = (llr[:, col["constant_random_signs"]] < 0).astype(np.int64)
        assert ((H @ x) % 2 != 0).any()
        one = llr[:, [col["constant"]]]
        _, _, c = lc.layered_census(H, layers, one, 1, 1.0, 0.0, early_stop=False)
        # every check whose variables are still untouched ties at all positions: the whole first layer at least
        assert c["check_updates"] == H.shape[0] and c["ties"] >= len(layers[0])
