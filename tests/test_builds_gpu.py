"""The Newton-matrix builds  A[rows] diag(theta) A[rows]' + diag  as the solver launches them, against the same product in long double.

Three families, through the C ABI hooks asm_test_build_flagged (k_tile_nzflags -> k_syrk with a chunk list, as Dev::schur_syrk launches a
row-list build) and asm_test_build_split (Dev::ns_newton_matrix, the statements of a null-space iteration up to the factorisation: split-K
k_syrk + k_ns_reduce_lower, or the plain build + k_ns_copy_lower + k_diag_prepare) and asm_test_build_dispatch (a handle set up by
asm_sublp_setup: Dev::schur_syrk with Pattern flags on rows and on the transposed copy, Dev::schur_rows, Dev::schur_banded_cols_dev,
Dev::ns_build_S0 - the structural-pair kernels k_schur_sparse and k_ns_s0_sparse where the handle has a banded order).

Two kinds of assertion.  (a) The rounding bound of ANY summation order of the K_eff non-zero products of an entry, with or without FMA:
|S_ij - ref_ij| <= gamma_n (|A| |theta| |A|' + |diag|)_ij, n = K_eff + 2 (+ the slice count for a split build), element by element, constant 1
(tests/util.py: rounding_bound_ratio).  It is a theorem, not a tuned tolerance - and it is a net for TERMS only: a float64 BLAS product
reaches 1e-2 ... 1e-4 of it (the bound grows like K, rounding like sqrt K), so what it catches is a dropped, doubled or mis-weighted term of
relative size above K u (one omitted 32-column chunk is ten orders above that).  (b) Anything finer - order of summation, a wrong last bit,
a flag, a placement - is pinned by the exact statements the code makes: the flagged build is bitwise the dense sweep, the flags are the
NumPy flags, every split-K slice is bitwise the plain build of its columns, the reduction is the left-to-right sum of the slices, and what a
kernel does not own keeps the caller's pre-fill.  `pytest -s` prints the largest ratio of (a) per case."""
import ctypes as C

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = C.c_void_p()
    assert hip_lib.asm_create(0, C.byref(h)) == 0
    yield h
    hip_lib.asm_destroy(h)


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _flagged(lib, h, A, idx, Ms, theta, diag, tile, use_flags):
    """S buffer (pitch = Ms rounded up to 32, plus one extra tile of rows, pre-filled), flags and executed share of one build."""
    M, K = A.shape
    T = tile if tile > 0 else util.pick_tile(Ms)
    nt = (Ms + 32 * T - 1) // (32 * T)
    ldS = (Ms + 31) // 32 * 32 + 32
    S = np.full((ldS, ldS), util.SENTINEL)
    flags = np.full((nt, K // 32), 255, np.uint8)
    frac = C.c_double(-1.0)
    rc = lib.asm_test_build_flagged(h, _d(A), M, K, idx.ctypes.data_as(C.POINTER(C.c_int32)) if idx is not None else None, Ms, _d(theta), _d(diag), tile,
                                    use_flags, _d(S), ldS, flags.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(frac))
    assert rc == 0, lib.asm_last_error(h)
    return S, flags, frac.value


def _untouched_outside_lower(S, Ms):
    """Strict upper triangle and everything beyond row / column Ms still hold the pre-fill."""
    own = np.zeros(S.shape, bool)
    own[:Ms, :Ms] = np.tril(np.ones((Ms, Ms), bool))
    return bool(np.all(S[~own] == util.SENTINEL))


@pytest.mark.parametrize("case", range(len(util.FLAGGED_CASES)), ids=[c[0] for c in util.FLAGGED_CASES])
def test_flagged_build(hip_lib, handle, case):
    name, Ms, K, tile, gathered, with_diag = util.FLAGGED_CASES[case]
    A, idx, theta, diag = util.flagged_operand(100 + case, Ms, K, tile, gathered, with_diag)
    T = tile if tile > 0 else util.pick_tile(Ms)
    S, flags, frac = _flagged(hip_lib, handle, A, idx, Ms, theta, diag, tile, 1)
    S_dense, flags2, _ = _flagged(hip_lib, handle, A, idx, Ms, theta, diag, tile, 0)
    # (b) exact statements
    want = util.tile_chunk_flags(A, idx, Ms, 32 * T)
    assert np.array_equal(flags, want) and np.array_equal(flags2, want)
    assert frac == util.executed_fraction(want)
    assert _untouched_outside_lower(S, Ms) and _untouched_outside_lower(S_dense, Ms)
    assert np.array_equal(S, S_dense)               # skipped products are exact zeros, the list keeps increasing k: bitwise the dense sweep
    # (a) the rounding bound, element by element
    B = A[idx] if idx is not None else A
    ref, mag, keff = util.build_reference(B, theta, diag)
    ratio, exact = util.rounding_bound_ratio(S, ref, mag, keff)
    print("ratio flagged %-12s Ms %4d K %5d tile %d executed %.3f: %.3e" % (name, Ms, K, T, frac, ratio))
    assert exact and ratio <= 1.0


def test_flagged_build_without_row_list_reads_only_the_first_rows(hip_lib, handle):
    """idx == NULL with Ms < M: tiles, flags and product are those of the first Ms rows (the rows below are dense and must not leak in)."""
    name, Ms, K, tile, _, with_diag = util.FLAGGED_CASES[0]
    B, _, theta, diag = util.flagged_operand(77, Ms, K, tile, False, with_diag)
    A = np.vstack([B, np.random.default_rng(5).standard_normal((40, K))])
    S, flags, frac = _flagged(hip_lib, handle, A, None, Ms, theta, diag, tile, 1)
    want = util.tile_chunk_flags(A, None, Ms, 32 * tile)
    assert np.array_equal(flags, want) and frac == util.executed_fraction(want) and _untouched_outside_lower(S, Ms)
    ratio, exact = util.rounding_bound_ratio(S, *util.build_reference(B, theta, diag))
    print("ratio flagged first-rows: %.3e" % ratio)
    assert exact and ratio <= 1.0


def _split(lib, h, G, theta, nsplit, rel, absv):
    k, K = G.shape
    ld = (k + 31) // 32 * 32
    parts = np.full((nsplit, ld, ld), util.SENTINEL)
    S = np.full((ld, ld), util.SENTINEL)
    N0 = np.full((ld, ld), util.SENTINEL)
    d0 = np.full(ld, util.SENTINEL)
    rc = lib.asm_test_build_split(h, _d(G), k, K, _d(theta), nsplit, rel, absv, _d(parts), _d(S), _d(N0), _d(d0))
    assert rc == 0, lib.asm_last_error(h)
    return parts, S, N0, d0


def _plain_lower(lib, h, G, theta, k0, k1):
    """Lower triangle (k x k, the rest zero) of the unsplit k_syrk build of the columns [k0, k1) with the solver's tile for k; an empty range is all zeros."""
    k = G.shape[0]
    if k1 <= k0:
        return np.zeros((k, k))
    S, _, _ = _flagged(lib, h, np.ascontiguousarray(G[:, k0:k1]), None, k, np.ascontiguousarray(theta[k0:k1]), None, util.pick_tile(k), 0)
    return np.tril(S[:k, :k])


@pytest.mark.parametrize("k,nch,counts", util.SPLIT_CASES, ids=["k%d-c%d" % (c[0], c[1]) for c in util.SPLIT_CASES])
def test_split_build(hip_lib, handle, k, nch, counts):
    K = 32 * nch
    G, theta = util.split_operand(1000 * k + nch, k, K)
    ref, mag, keff = util.build_reference(G, theta)
    low = np.tril(np.ones((k, k), bool))
    di = np.arange(k)
    whole = _plain_lower(hip_lib, handle, G, theta, 0, K)
    for nsplit in counts:
        # powers of two next to the solver's 1e-13, 1e-30: rel v is exact, so v + (rel v + absv) is one value whether the compiler fuses it or not
        rel, absv = 2.0 ** -43, 2.0 ** -100
        parts, S, N0, d0 = _split(hip_lib, handle, G, theta, nsplit, rel, absv)
        if nsplit == 1:
            assert np.all(parts == util.SENTINEL)
            v = whole
        else:
            ranges = util.split_ranges(K, nsplit)
            for s, (k0, k1) in enumerate(ranges):
                # slice s is bitwise the plain build of its columns, whatever the placement (8 slices: slice-major); an empty slice is zeros
                assert np.array_equal(np.tril(parts[s, :k, :k]), _plain_lower(hip_lib, handle, G, theta, k0, k1)), (nsplit, s)
                assert _untouched_outside_lower(parts[s], k), (nsplit, s)
            v = np.tril(parts[0, :k, :k]).copy()
            for s in range(1, nsplit):
                v = v + np.tril(parts[s, :k, :k])              # the fixed order of k_ns_reduce_lower
        # S: the sum below the diagonal, the regularised diagonal, nothing else; diag0 and N0: the unregularised values
        want_S = v.copy()
        want_S[di, di] = v[di, di] + (rel * v[di, di] + absv)
        assert np.array_equal(S[:k, :k][low], want_S[low]), nsplit
        assert _untouched_outside_lower(S, k), nsplit
        assert np.array_equal(d0[:k], v[di, di]) and np.all(d0[k:] == util.SENTINEL), nsplit
        want_N0 = np.full(N0.shape, util.SENTINEL)
        want_N0[:k, :k][low] = v[low]
        if k <= 256:                                           # small systems keep the copy in full (mirrored)
            full = v + np.tril(v, -1).T
            want_N0[:k, :k] = full
        assert np.array_equal(N0, want_N0), nsplit
        ratio, exact = util.rounding_bound_ratio(N0, ref, mag, keff, extra=nsplit)
        print("ratio split k %3d K %5d nsplit %d: %.3e" % (k, K, nsplit, ratio))
        assert exact and ratio <= 1.0, nsplit


# ------------------------------------------------------------------------------------------------ production dispatch on a set-up handle
def _dispatch_cases():
    from activesetmethods_amd import acopf
    pr = acopf.acopf_problem(acopf.synthetic_case("case118", 1), "case118")
    x = pr.x0.copy()
    case118 = dict(n=pr.n, m=pr.m, j_row=pr.j_row, j_col=pr.j_col, dE=pr.eval_jac_g(x, np.zeros(pr.nnz)), c_lb=pr.g_L, c_ub=pr.g_U, v_lb=pr.x_L, v_ub=pr.x_U)
    return {
        "sparse": util.random_subproblem(41, 600, 380, 0.012, 0.2, 5),             # no narrow band: Pattern and per-call flags
        "sparse-tall": util.random_subproblem(42, 900, 700, 0.006, 0.0, 8),
        "banded": util.banded_subproblem(501, 400, 600, 120, 30),                  # reverse Cuthill-McKee band of rows and columns
        "banded-eq": util.banded_subproblem(503, 500, 520, 300, 0),
        "eqrich": util.equality_rich_subproblem(81, 300, 260, 160),                # S0 without a band (2 bw >= nE)
        "eqrich-big": util.equality_rich_subproblem(82, 500, 470, 200),
        "case118": case118,
    }


DISPATCH_NAMES = ["sparse", "sparse-tall", "banded", "banded-eq", "eqrich", "eqrich-big", "case118"]


def _dispatch(lib, h, dE, which, ld, idx, theta, diag, M, n):
    S = np.full((ld, ld), util.SENTINEL)
    Ah = np.zeros((M, n))
    info = np.zeros(12, np.int64)
    I32 = C.POINTER(C.c_int32)
    rc = lib.asm_test_build_dispatch(h, _d(dE), which, idx.ctypes.data_as(I32) if idx is not None else None, len(idx) if idx is not None else 0, _d(theta), _d(diag),
                                     _d(S), _d(Ah), info.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None)
    assert rc == 0, lib.asm_last_error(h)
    return S, Ah, info


def _check_build(label, build, B, theta, diag, band):
    """One build of B diag(theta) B' + diag (dim = rows of B) in a pre-filled factor buffer: twice bit-identical, nothing written outside the
    lower triangle, bound (a); band > 0 (structural-pair build): no pre-fill left inside the band, beyond it no product exists and the entry
    is the pre-fill or a cleared 0.0."""
    dim = B.shape[0]
    S = build()
    assert np.array_equal(S, build()), label                       # no atomics: a repeat gives the same bits
    assert _untouched_outside_lower(S, dim), label
    ref, mag, keff = util.build_reference(B, theta, diag)
    X = S[:dim, :dim].copy()
    if band > 0:
        i, j = np.indices((dim, dim))
        low = j <= i
        inside = low & (i - j <= band)
        assert not np.any(X[inside] == util.SENTINEL), label        # pairless places inside the band are cleared, whatever was there
        beyond = low & ~inside
        assert np.all(keff[beyond] == 0) and np.all((X[beyond] == 0.0) | (X[beyond] == util.SENTINEL)), label
        X[beyond] = 0.0
    ratio, exact = util.rounding_bound_ratio(X, ref, mag, keff)
    print("ratio dispatch %-40s dim %4d: %.3e" % (label, dim, ratio))
    assert exact and ratio <= 1.0, label
    return ratio


@pytest.mark.parametrize("name", DISPATCH_NAMES)
def test_dispatch_builds(hip_lib, name):
    from tests.test_sublp_parity_gpu import _abi_setup
    lib = hip_lib
    sp = _dispatch_cases()[name]
    dE = np.ascontiguousarray(sp["dE"], dtype=np.float64)
    h = C.c_void_p()
    assert lib.asm_create(0, C.byref(h)) == 0
    try:
        assert _abi_setup(lib, h, sp) == 0, lib.asm_last_error(h)
        info = np.zeros(12, np.int64)
        M0 = sp["m"] * 2 + 8
        rows_o, cols_o, e_o = np.full(M0, -1, np.int32), np.full(sp["n"], -1, np.int32), np.full(M0, -1, np.int32)
        I32 = C.POINTER(C.c_int32)
        assert lib.asm_test_build_dispatch(h, _d(dE), -1, None, 0, None, None, None, None, info.ctypes.data_as(C.POINTER(C.c_int64)), rows_o.ctypes.data_as(I32),
                                           cols_o.ctypes.data_as(I32), e_o.ctypes.data_as(I32)) == 0, lib.asm_last_error(h)
        M, n, row_band, col_band, ld, nE, s0_band, ld0, col_ok, nz_ok, _, sparse = (int(v) for v in info)
        assert n == sp["n"] and sp["m"] <= M <= M0 and sparse == 1
        rng = np.random.default_rng(7)
        th_n = 10.0 ** rng.uniform(-4.0, 4.0, n)                     # an interior point near convergence: eight decades
        th_M = 10.0 ** rng.uniform(-4.0, 4.0, M)
        dg_M = 10.0 ** rng.uniform(-3.0, 3.0, M)
        dg_n = 10.0 ** rng.uniform(-3.0, 3.0, n)
        _, Ah, _ = _dispatch(lib, h, dE, 0, ld, None, th_n, dg_M, M, n)
        # all rows through Dev::schur_syrk (Pattern flags when the handle has them; a banded handle builds this matrix from its pairs instead)
        _check_build("%s rows pattern=%d" % (name, nz_ok), lambda: _dispatch(lib, h, dE, 0, ld, None, th_n, dg_M, M, n)[0], Ah, th_n, dg_M, 0)
        # row lists through Dev::schur_rows: all rows, a third, the list with one row taken out of a pair-dense region in the middle
        base = rows_o[:M].astype(np.int32) if row_band > 0 else np.arange(M, dtype=np.int32)
        third = base[np.sort(rng.choice(M, M // 3, replace=False))]
        # ... the row with the most structural pairs (rows sharing a column with it) among the middle half of the order
        pairs = ((Ah != 0).astype(np.float64) @ (Ah != 0).T.astype(np.float64) > 0).sum(axis=1)[base]
        mid = M // 4 + int(np.argmax(pairs[M // 4:3 * M // 4]))
        assert pairs[mid] >= np.median(pairs) and pairs[mid] > 1
        lists = {"all": base, "third": third, "minus-one": np.delete(base, mid)}
        for lname, idx in lists.items():
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            dg = dg_M[:len(idx)].copy()
            _check_build("%s list %s band %d" % (name, lname, row_band), lambda: _dispatch(lib, h, dE, 2, ld, idx, th_n, dg, M, n)[0], Ah[idx], th_n, dg, row_band)
        if col_ok:
            _check_build("%s cols" % name, lambda: _dispatch(lib, h, dE, 1, ld, None, th_M, dg_n, M, n)[0], np.ascontiguousarray(Ah.T), th_M, dg_n, 0)
        if col_band > 0:
            BT = np.ascontiguousarray(Ah.T[cols_o])
            _check_build("%s cols banded %d" % (name, col_band), lambda: _dispatch(lib, h, dE, 3, ld, None, th_M, dg_n, M, n)[0], BT, th_M, dg_n, col_band)
        if nE > 0:
            fm = th_n.copy()
            fm[rng.random(n) < 0.1] = 0.0                              # fixed columns drop out of S0
            BE = Ah[e_o[:nE]]
            _check_build("%s S0 band %d" % (name, s0_band), lambda: _dispatch(lib, h, dE, 4, ld0, None, fm, None, M, n)[0], BE, fm, None, s0_band)
    finally:
        lib.asm_destroy(h)


def test_dispatch_cases_reach_every_build(hip_lib):
    """The handles of test_dispatch_builds take every branch of the dispatch between them (asked of freshly set-up handles)."""
    from tests.test_sublp_parity_gpu import _abi_setup
    seen = set()
    for name, sp in _dispatch_cases().items():
        h = C.c_void_p()
        assert hip_lib.asm_create(0, C.byref(h)) == 0
        try:
            assert _abi_setup(hip_lib, h, sp) == 0
            info = np.zeros(12, np.int64)
            assert hip_lib.asm_test_build_dispatch(h, _d(np.ascontiguousarray(sp["dE"], dtype=np.float64)), -1, None, 0, None, None, None, None,
                                                   info.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None) == 0
            seen.add("pattern" if info[9] else "rows-dense")
            seen.add("rows-banded" if info[2] > 0 else "rows-percall")
            seen.add("cols-banded" if info[3] > 0 else ("cols-syrk" if info[8] else "no-cols"))
            if info[5] > 0:
                seen.add("s0-banded" if info[6] > 0 else "s0-syrk")
        finally:
            hip_lib.asm_destroy(h)
    assert {"pattern", "rows-percall", "rows-banded", "cols-banded", "cols-syrk", "s0-banded", "s0-syrk"} <= seen, sorted(seen)
