"""The twins of tests/skeleton_twins.py against the specification and against exact arithmetic, on every case the GPU test runs.

  - the scaling twin equals oracle.lp_solver.scale_lp bit for bit: the twin follows the kernels statement by statement, the oracle is written
    with whole-array NumPy expressions - that both give the same bits makes the twin the specification and not a restatement of the kernel
  - the long-double references of the products and norms are within 1/1024 of the device's bar of the values mpmath gives at 256 bits: a
    reference that needed the bar itself would fail here
  - the cases are what the GPU test needs them to be: pattern kinds, chunk edges, threshold values that round either way"""
import mpmath
import numpy as np
import pytest

from tests import skeleton_twins as T

NAMES = [s[0] for s in T.SHAPES]
ROOM = 1.0 / 1024


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_twin_is_the_oracle(name):
    case, runs = T.runs(name)
    for r in runs:
        c, rho, Ah = T.oracle_scale(r["J"], r["lb"], r["ub"])
        assert _bits(c) == _bits(r["c"]), (name, r["vkind"])
        assert _bits(rho) == _bits(r["rho"]), (name, r["vkind"])
        assert _bits(Ah) == _bits(r["Ah"]), (name, r["vkind"])
        # the statement the header gives: Ah = diag(1 / rho) J diag(c), exactly (powers of two inside the specified range)
        assert np.array_equal(r["Ah"] * r["rho"][:, None], r["J"] * r["c"])
        mags = np.abs(np.concatenate([r["J"][r["J"] != 0], r["Ah"][r["Ah"] != 0], r["c"], r["rho"]]))
        assert mags.min() >= 2.0 ** -400 and mags.max() <= 2.0 ** 400


def _mp_dot_rows(A, x):
    xm = [mpmath.mpf(float(v)) for v in x]
    out = []
    for row in A:
        nz = np.nonzero(row)[0]
        out.append(mpmath.fdot([mpmath.mpf(float(row[j])) for j in nz], [xm[j] for j in nz]))
    return out


def _worst(ld, mp_vals, mag, L):
    """Largest |ld - mp| / bar over the entries, in mpmath."""
    worst = mpmath.mpf(0)
    for v, e, g, l in zip(ld, mp_vals, mag, L):
        hi = float(v)                                  # a long double is the exact sum of two doubles
        err = abs(mpmath.mpf(hi) + mpmath.mpf(float(v - T.LD(hi))) - e)
        if err == 0:
            continue
        bar = (int(l) + 2) * mpmath.mpf(T.EPS) * mpmath.mpf(float(g))
        assert bar > 0
        worst = max(worst, err / bar)
    return float(worst)


@pytest.mark.parametrize("name", NAMES)
def test_references_hold_their_bound(name):
    case, runs = T.runs(name)
    Lx, Ly = T.product_bars(case, case["kind"] == "sparse")
    with mpmath.workprec(256):
        for r in runs:
            for A in (r["J"], r["Ah"]):
                ax, magx, aty, magy = T.products_ref(A, case["x"], case["y"])
                assert _worst(ax, _mp_dot_rows(A, case["x"]), magx, Lx) <= ROOM, (name, r["vkind"])
                assert _worst(aty, _mp_dot_rows(A.T, case["y"]), magy, Ly) <= ROOM, (name, r["vkind"])
            J = r["J"][:case["m"]]
            nr = T.norms_ref(J)
            exact = [mpmath.sqrt(mpmath.fsum(mpmath.mpf(float(a)) ** 2 for a in row[row != 0])) for row in J]
            assert _worst(nr, exact, [float(v) for v in nr], Lx[:case["m"]]) <= ROOM, (name, r["vkind"])


@pytest.mark.parametrize("name", NAMES)
def test_cases_are_what_they_claim(name):
    case, runs = T.runs(name)
    n, m, M = case["n"], case["m"], case["M"]
    nnzS = int(T.pattern_of(case).sum())
    sparse, fast, _, _ = T.EXPECT[case["kind"]]
    assert (nnzS * 16 <= M * n and case["kind"] != "fast") == bool(sparse)
    assert (len(case["adj"]) == 0 and len(case["j_row"]) == m * n
            and np.array_equal((case["j_row"] - 1) * n + case["j_col"] - 1, np.arange(m * n))) == bool(fast)
    if case["kind"] in ("general", "sparse", "padded"):
        assert M > m
    if case["kind"] == "general":
        keys = (case["j_row"] - 1) * n + case["j_col"] - 1
        assert len(np.unique(keys)) < len(keys)                       # duplicates
    if case["kind"] in ("sparse", "padded"):
        P = T.pattern_of(get_sparse(name))
        assert set(T.COL_DEAL) <= set(P[:m].sum(axis=0).tolist()) and set(T.ROW_DEAL) <= set(P[:m].sum(axis=1).tolist())
    if name in T.CHUNKS:
        assert T.chunks(M) == T.CHUNKS[name]
    if name == "chunk-M4100":
        R, chunk = T.chunks(M)
        assert M > 4096 and (M + 31) // 32 > T.TMAXCHUNKS and 0 < M - (R - 1) * chunk < chunk
    if name == "sparse-520x260":
        assert m > 256
    if case["kind"] == "fast" and m >= 3 and n >= 3:
        # a column reduction that loses the last row of the first chunk, the first row of the second or the last row of all changes rel
        R, chunk = T.chunks(M)
        for lost in sorted({chunk - 1, chunk if R > 1 else chunk - 1, M - 1}):
            keep = np.arange(M) != lost
            for r in (runs[0], runs[1]):
                a = np.abs(r["J"]) / r["rmax"][:, None]
                assert not np.array_equal(a[keep].max(axis=0), r["rel"]), (name, lost, r["vkind"])
    if m >= 3 and n >= 3:
        for r in runs:
            J = r["J"]
            assert (np.abs(J).max(axis=1) == 0).any() and (r["rho"][np.abs(J).max(axis=1) == 0] == 1.0).all()      # rmax -> 1, rho = 1
            zc = np.abs(J).max(axis=0) == 0
            assert zc.any() and (r["rel"][zc] == 0).all()
            box = np.maximum(r["ub"], -r["lb"])
            with np.errstate(invalid="ignore"):
                assert np.array_equal(r["c"][zc], T.pow2_round(np.minimum(box[zc], 1.0)))
            free = np.isinf(box)
            assert free.any() and (r["rel"][free] > 0).all()
            assert np.array_equal(r["c"][free], T.pow2_round(1.0 / r["rel"][free]))
    # the threshold run rounds either way, and sits on the literal itself
    thr = runs[T.VALUE_KINDS.index("threshold")]
    f = np.frexp(np.abs(thr["dE"][thr["dE"] != 0]))[0]
    assert set(np.unique(f)) <= {np.nextafter(T.T_SQRT_HALF, 0.0), T.T_SQRT_HALF, np.nextafter(T.T_SQRT_HALF, 1.0)}
    if M >= 8:
        assert len(np.unique(f)) == 3
        fr = np.frexp(np.abs(thr["J"] * thr["c"]).max(axis=1))[0]
        assert (fr < T.T_SQRT_HALF).any() and (fr >= T.T_SQRT_HALF).any()
    # the last run leaves stale entries in the range rows: the oracle's J there is not what a fresh assembly gives
    if case["kind"] in ("general", "sparse"):
        fresh = T.Oracle(case).assemble(runs[-1]["dE"])
        assert not np.array_equal(fresh[m:], runs[-1]["J"][m:]) and np.array_equal(fresh[:m], runs[-1]["J"][:m])


def get_sparse(name):
    return T.get_case(name.replace("padded", "sparse"))


def test_pow2_round_threshold():
    """1 / 2 <= f < the literal rounds down, f >= the literal up; nothing positive gives 1."""
    t = T.T_SQRT_HALF
    for e in (-300, -1, 0, 7, 300):
        s = np.ldexp(1.0, e)
        assert T.pow2_round(np.nextafter(t, 0.0) * s) == s / 2 and T.pow2_round(t * s) == s and T.pow2_round(np.nextafter(t, 1.0) * s) == s
        assert T.pow2_round(0.5 * s) == s / 2 and T.pow2_round(np.nextafter(1.0, 0.0) * s) == s
    assert T.pow2_round(0.0) == 1.0 and T.pow2_round(-3.0) == 1.0
