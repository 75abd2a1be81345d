"""The basis set-up of the null-space form (Solver::ns_setup with ns_reproject, ns_basis_from, ns_ortho and the cold column selection), one
launch site at a time through asm_test_ns_setup_stages: the solver's own launch-site members on the form's own buffers of a handle that
asm_sublp_setup has set up, against the twins of tests/util.py (tw_nss_*, nss_*; chained against the oracle in tests/test_ns_setup_cpu.py).
The conventions are those of tests/test_ns_stages_gpu.py:
(a) the rounding bound |out - twin| <= gamma_K mag, element by element with constant 1 (k_ns_rows_e, k_ns_gi: K = entries of the row; k_ns_pj:
    entries of the column on the equality rows + 1; the Gram build: ldn; k_ns_ortho: row c from the device's own rows before it, K = c + 1);
(b) exact statements, bit for bit against float64 NumPy (k_ns_rhs_cols, k_ns_gather_t, k_ns_set_diag, k_ns_diag, k_ns_count_big, the zeros
    of fixed and padded columns);
(c) the launch sites that are algorithms (trsm_rows, the k x k factor, ns_ortho's product branch) against the same algorithm in long double on
    the factor the device returned; allowance: ten times the error of the same algorithm in float64 NumPy on the same data.
Every buffer is pre-filled with util.SENTINEL or the loaded value; what a stage does not own comes back bit for bit - rows k .. cap - 1 of G,
R and X in particular.  grid_out is compared with the rule of each launch site.  `pytest -s` prints the largest ratio of (a) per kernel."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

LD = np.longdouble
SENT = util.SENTINEL
ERR_ARG = -1
KIND = {nm: i for i, nm in enumerate(util.NSS_KINDS)}
CASES = list(util.NSS_CASES)
RATIOS = {}


def note(kernel, ratio):
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
    print("ratio (a) %-12s %.3e (largest so far %.3e)" % (kernel, ratio, RATIOS[kernel]))


def _p(a, typ=C.c_double):
    return None if a is None else a.ctypes.data_as(C.POINTER(typ))


def stage(kind, flag=0, thr=0.0):
    return (KIND[kind], int(flag), float(thr))


class Case:
    """A handle set up for a case, its layout, the device operand and the reference set-up in float64 on that operand."""

    def __init__(self, lib, name):
        from activesetmethods_amd import _lib
        self.lib, self.name = lib, name
        self.sp, self.fm, kres = util.nss_case(name)
        self.dE = np.ascontiguousarray(self.sp["dE"], np.float64)
        self.h = util.abi_create(lib)
        assert util.abi_setup(lib, self.h, self.sp) == 0, lib.asm_last_error(self.h)
        info = np.zeros(12, np.int64)
        M0, n = 2 * self.sp["m"] + 8, self.sp["n"]
        assert lib.asm_test_build_dispatch(self.h, _p(self.dE), -1, None, 0, None, None, None, None, _p(info, C.c_int64), None, None, None) == 0
        M = int(info[0])
        assert info[1] == n and M <= M0 and info[5] >= 64, "the case has no null-space form"
        Ah = np.zeros((M, n))
        assert lib.asm_test_build_dispatch(self.h, _p(self.dE), -1, None, 0, None, None, None, Ah.ctypes.data_as(_lib._D), _p(info, C.c_int64), None, None, None) == 0
        self.M, self.n, nE = M, n, int(info[5])
        # the reference set-up on the device operand needs the lists first
        lay, idx = np.zeros(16, np.int64), np.zeros(M, np.int32)
        assert self._call(1, 1, None, lay, idx, None, {}, 0, None, None) == 0, lib.asm_last_error(self.h)
        self.op = util.NssOp(Ah, idx[:nE], idx[nE:M], self.fm)
        self.ref = util.nss_chain(self.op, np.float64, M=M)
        assert self.ref["path"] == "cold"
        self.k, self.J = self.ref["k"], self.ref["J"].astype(np.int32)
        self.kres = self.k if kres is None else kres
        self.lay = self.layout(self.k, self.kres)
        self.idx = idx
        # the device orders the equality rows itself: the banded case must be banded there (k_ns_s0_sparse, band-limited substitutions, the
        # band argument of the transposed copy), the dense ones dense
        # (the 64 equality rows of the wide cases, four entries each in 900 columns, come out banded as well: band 4)
        banded = name == "banded" or name.startswith("wide")
        assert (self.lay.band > 0) == banded and (not banded or 2 * self.lay.band < self.lay.nE), (name, self.lay.band)

    def _call(self, k, kres, J, lay, idx, stages, bufs, Zk, hint, outs, fm=None):
        from activesetmethods_amd import _lib
        fm = self.fm if fm is None else fm
        ns = 0 if stages is None else len(stages)
        arr = (_lib.NssStage * max(ns, 1))(*[_lib.NssStage(*s) for s in (stages or [])])
        o = outs or {}
        b = lambda nm: _p(bufs.get(nm))
        return self.lib.asm_test_ns_setup_stages(self.h, _p(self.dE), _p(fm), k, kres, _p(J, C.c_int32), _p(lay, C.c_int64), _p(idx, C.c_int32), b("G"), b("R"), b("X"),
                                                 b("SN"), b("Y"), b("T"), b("d"), _p(o.get("f0")), _p(o.get("Lt")), Zk, _p(hint, C.c_int32), 0 if hint is None else len(hint),
                                                 None if stages is None else arr, ns, _p(o.get("grid"), C.c_uint32), _p(o.get("res"), C.c_int32), _p(o.get("setup"), C.c_int32))

    def layout(self, k, kres):
        lay = np.zeros(16, np.int64)
        assert self._call(k, kres, None, lay, None, None, {}, 0, None, None) == 0, self.lib.asm_last_error(self.h)
        L = types.SimpleNamespace(**{nm: int(lay[i]) for i, nm in enumerate(util.NSS_LAYOUT)})
        op = self.op
        assert (L.ldn, L.nEp, L.nIp, L.ldg, L.nE, L.nI, L.n, L.M) == (op.ldn, op.nEp, op.nIp, op.ldg, op.nE, op.nI, op.n, op.M)
        assert L.cap == util.nss_kcap(kres) and L.fld == util.nss_kcap(kres) and L.wb == util.nss_wb(L.fld) and L.ld0 == L.nEp
        return L

    def run(self, stages, k=None, J=None, G=None, R=None, X=None, SN=None, Y=False, T=False, d=None, Zk=0, hint=None, fm=None, expect=0, big=True):
        """One call.  G, R, X, SN: the loaded values (whole buffers), or None for the pre-fill; Y, T: True / an array to have them in the call."""
        L, k = self.lay, self.k if k is None else k
        fill = lambda a, shape: np.full(shape, SENT) if a is None else np.ascontiguousarray(a, np.float64).copy()
        bufs = {"R": fill(R, (L.cap, L.nEp)), "X": fill(X, (L.cap, L.nEp))}
        if big:
            bufs.update(G=fill(G, (L.cap, L.ldg)), SN=fill(SN, (L.fld, L.fld)))
        if Y is not False:
            bufs["Y"] = fill(None if Y is True else Y, (2, L.ldn, L.nEp))
        if T is not False:
            bufs["T"] = fill(None if T is True else T, (L.ldT, L.ldT))
        if d is not None:
            bufs["d"] = fill(d, (L.ldn,))
        before = {nm: a.copy() for nm, a in bufs.items()}
        outs = {"f0": np.zeros((L.nEp, L.nEp)), "Lt": np.zeros((L.nEp, L.nEp)), "grid": np.zeros(max(len(stages), 1), np.uint32),
                "res": np.zeros(max(len(stages), 1), np.int32), "setup": np.full(4 + L.n, -1, np.int32)}
        Jd = None if J is None else np.ascontiguousarray(J, np.int32)
        hd = None if hint is None else np.ascontiguousarray(hint, np.int32)
        rc = self._call(k, self.kres, Jd, np.zeros(16, np.int64), None, [stage(*s) if isinstance(s, tuple) else stage(s) for s in stages], bufs, Zk, hd, outs, fm)
        assert rc == expect, (rc, self.lib.asm_last_error(self.h))
        r = types.SimpleNamespace(before=before, k=k, **bufs, **outs)
        for nm in bufs:
            assert np.all(np.isfinite(bufs[nm])) or nm in ("SN", "T"), nm      # (a guarded pivot squares to infinity nowhere: 1e128 is stored)
        return r

    def close(self):
        assert self.lib.asm_destroy(self.h) == 0


@pytest.fixture(scope="module")
def cases(hip_lib):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(hip_lib, name)
        return made[name]
    yield get
    for c in made.values():
        c.close()
    print()
    for kern, r in sorted(RATIOS.items()):
        print("largest ratio (a) %-12s %.3e" % (kern, r))


def same(r, names, rows=None):
    """The buffers `names` came back bit for bit (rows: only from that row on)."""
    for nm in names:
        a, b = getattr(r, nm), r.before[nm]
        if rows is not None:
            a, b = a[rows:], b[rows:]
        assert np.array_equal(a, b), nm


def rand_rows(c, seed, k=None):
    """Basis rows to load: k rows of ldg random entries (fixed and padded columns included - the kernels must not let them count) under
    SENTINEL rows."""
    L, k = c.lay, c.k if k is None else k
    G = np.full((L.cap, L.ldg), SENT)
    G[:k] = np.random.default_rng(seed).standard_normal((k, L.ldg))
    return G


# ------------------------------------------------------------------------------------------------ (b) exact launch sites
@pytest.mark.parametrize("name", CASES)
def test_rhs_cols_and_gather(cases, name):
    c = cases(name)
    L, k, op = c.lay, c.k, c.op
    r = c.run([("rhs_cols", 0)], J=c.J, big=False)
    assert r.grid[0] == k
    assert np.array_equal(r.R[:k], util.tw_nss_rhs_cols(op, c.J))
    same(r, ["R"], rows=k)
    same(r, ["X"])
    if (c.fm == 0).any():      # a fixed column in the list: an all-zero row
        J2 = c.J.copy()
        J2[k // 2] = np.nonzero(c.fm == 0)[0][0]
        r = c.run([("rhs_cols", 0)], J=J2, big=False)
        assert np.array_equal(r.R[:k], util.tw_nss_rhs_cols(op, J2)) and not r.R[k // 2].any()
    r = c.run([("rhs_cols", 1)], Y=True, big=False)
    assert r.grid[0] == L.n
    assert np.array_equal(r.Y[0, :L.n], util.tw_nss_rhs_cols(op))
    assert np.array_equal(r.Y[0, L.n:], r.before["Y"][0, L.n:]) and np.array_equal(r.Y[1], r.before["Y"][1])
    same(r, ["R", "X"])
    G = rand_rows(c, 5)
    r = c.run(["gather_t"], J=c.J, G=G)
    assert tuple(r.grid) == ((k + 255) // 256,)
    want = r.before["SN"].copy()
    low = np.tril(np.ones((k, k), bool))
    want[:k, :k][low] = util.tw_nss_gather_t(G, c.J)[low]
    assert np.array_equal(r.SN, want)      # the strictly upper part and everything beyond column k are not the kernel's
    same(r, ["G", "R", "X"])


def test_set_diag_diag_and_count_big(cases):
    c = cases("small-fixed")
    L, n = c.lay, c.lay.n
    rng = np.random.default_rng(2)
    T0 = rng.standard_normal((L.ldT, L.ldT))
    for flag in (0, 1):
        r = c.run([("set_diag", flag), "diag"], T=T0, d=np.full(L.ldn, SENT), big=False)
        assert tuple(r.grid) == ((n + 255) // 256, (n + 255) // 256)
        want = T0.copy()
        want[:n, :n][np.tril(np.ones((n, n), bool))] = 0.0
        if flag == 0:
            want[np.arange(n), np.arange(n)] = c.fm
        assert np.array_equal(r.T, want)
        assert np.array_equal(r.d[:n], np.diag(want)[:n]) and np.all(r.d[n:] == SENT)
    r = c.run(["diag"], T=T0, d=np.full(L.ldn, SENT), big=False)
    assert np.array_equal(r.d[:n], np.diag(T0)[:n]) and np.array_equal(r.T, T0)
    # counts 0, 1, 63, 64, 65 and 1025 as orders of one loaded diagonal: every order ends on a planted entry (index N - 1) but the first,
    # which ends just below NS_BIG; the entries between the planted ones are just below it too
    c = cases("wide")
    L = c.lay
    assert L.ldT >= 1100
    below = np.nextafter(util.NS_BIG, 0.0)
    T0 = np.full((L.ldT, L.ldT), util.NS_BIG * 4)      # off the diagonal nothing counts
    dg = np.full(L.ldT, below)
    planted = [10] + list(range(20, 82)) + [90, 95] + list(range(100, 1060))
    dg[planted] = util.NS_BIG
    dg[95], dg[1059] = 1e300, np.inf
    T0[np.arange(L.ldT), np.arange(L.ldT)] = dg
    orders = [10, 11, 82, 91, 96, 1060, 0, L.ldT]
    r = c.run([("count_big", N) for N in orders], T=T0, big=False)
    assert [int(v) for v in r.res] == [int((dg[:N] >= util.NS_BIG).sum()) for N in orders]
    assert [int(v) for v in r.res][:6] == [0, 1, 63, 64, 65, 1025] and np.all(r.grid == 1)
    assert np.array_equal(r.T, T0)


@pytest.mark.parametrize("name", ["small-dep", "dense", "banded", "wide"])
def test_cold_substitution(cases, name):
    """The head of the cold selection: all n columns as right-hand sides, forward substitution only (dense and banded f0, a dropped pivot)."""
    c = cases(name)
    L, op = c.lay, c.op
    r = c.run(["s0_factor", ("rhs_cols", 1), ("trsm", 0)], Y=True, big=False)
    assert r.res[0] == c.ref["dropped"] and tuple(r.grid) == (0, L.n, 0)
    rhs = util.tw_nss_rhs_cols(op)
    assert np.array_equal(r.Y[0, :L.n], rhs)      # (one wide block: the right-hand sides are not updated in place)
    L0 = np.tril(r.f0[:L.nE, :L.nE])
    check_c(r.Y[1, :L.n, :L.nE], util.nss_trsm_rows(L0, rhs[:, :L.nE], False), util.nss_trsm_rows(L0, rhs[:, :L.nE], False, np.float64), name + " cold trsm_rows")
    assert np.array_equal(r.Y[:, L.n:], r.before["Y"][:, L.n:]) and np.array_equal(r.Y[1, :L.n, L.nE:], r.before["Y"][1, :L.n, L.nE:])
    same(r, ["R", "X"])
    # the pre-fill of the padding of Y did not outlive the call (include/asm_hip.h): a cold set-up on the same handle finds its basis
    path, kk, dropped, Jd = setup_result(c.run(["setup"], big=False))
    assert (path, kk, dropped) == (util.NSS_PATHS["cold"], c.k, c.ref["dropped"]) and np.array_equal(Jd, c.J)


# ------------------------------------------------------------------------------------------------ (a) the sparse products and the Gram build
@pytest.mark.parametrize("name", CASES)
def test_products_on_loaded_rows(cases, name):
    c = cases(name)
    L, k, op = c.lay, c.k, c.op
    G = rand_rows(c, 11)
    r = c.run(["rows_e"], G=G)
    assert tuple(r.grid) == ((L.nEp + 255) // 256,)
    val, mag, K = util.tw_nss_rows_e(op, G[:k])
    note("k_ns_rows_e", util.bound_ratio(r.R[:k], val, mag, K[None, :]))
    assert util.bound_ratio(r.R[:k], val, mag, K[None, :]) <= 1.0
    assert not r.R[:k, L.nE:].any()
    same(r, ["R"], rows=k)
    same(r, ["G", "X", "SN"])
    r = c.run(["gi"], G=G)
    assert tuple(r.grid) == ((L.nIp + 255) // 256,)
    val, mag, K = util.tw_nss_gi(op, G[:k])
    note("k_ns_gi", util.bound_ratio(r.G[:k, L.ldn:], val, mag, K[None, :]))
    assert util.bound_ratio(r.G[:k, L.ldn:], val, mag, K[None, :]) <= 1.0
    assert not r.G[:k, L.ldn + L.nI:].any()
    assert np.array_equal(r.G[:, :L.ldn], G[:, :L.ldn])
    same(r, ["G"], rows=k)
    same(r, ["R", "X", "SN"])
    W = np.full((L.cap, L.nEp), SENT)
    W[:k] = np.random.default_rng(12).standard_normal((k, L.nEp))
    for second in (0, 1):
        r = c.run([("pj", second)], J=c.J, G=G, R=W)
        assert tuple(r.grid) == ((L.ldn + 255) // 256,)
        val, mag, K = util.tw_nss_pj(op, W[:k], c.J, G[:k] if second else None)
        ratio = util.bound_ratio(r.G[:k, :L.ldn], val, mag, K[None, :])
        note("k_ns_pj/%d" % second, ratio)
        assert ratio <= 1.0
        assert not r.G[:k, :L.n][:, c.fm == 0].any() and not r.G[:k, L.n:L.ldn].any()
        assert np.array_equal(r.G[:, L.ldn:], G[:, L.ldn:])
        same(r, ["G"], rows=k)
        same(r, ["R", "X", "SN"])
    r = c.run(["gram"], G=G)
    ref, mag, _ = util.build_reference(G[:k, :L.ldn], np.ones(L.ldn))
    ratio, exact = util.rounding_bound_ratio(r.SN[:k, :k], ref, mag, np.tril(np.full((k, k), L.ldn)))
    note("gram", ratio)
    assert ratio <= 1.0
    want = r.before["SN"].copy()
    want[:k, :k][np.tril(np.ones((k, k), bool))] = r.SN[:k, :k][np.tril(np.ones((k, k), bool))]
    assert np.array_equal(r.SN, want)
    same(r, ["G", "R", "X"])


# ------------------------------------------------------------------------------------------------ the chain, stage by stage
def check_c(dev, ref, f64, what, order=0):
    """(c): the device against the long-double algorithm, allowance ten times float64 NumPy's error on the same data.  At order 1 the algorithm
    is a square root or a division, which NumPy rounds correctly - its error can be anything down to zero and measures nothing (the sibling file
    exempts k = 1 for the same reason); there the allowance is at least gamma_3: pivot, square root / reciprocal, product, one rounding each."""
    scale = max(float(np.abs(ref).max()), 1e-300)
    allow = 10.0 * float(np.abs(np.asarray(f64, LD) - ref).max()) / scale
    if order == 1:
        allow = max(allow, float(util.gamma(3)))
    err = float(np.abs(np.asarray(dev, LD) - ref).max()) / scale
    print("%s: device error %.2e, float64 NumPy %.2e" % (what, err, allow / 10))
    assert err <= allow, "%s: device error %.2e > 10 x %.2e" % (what, err, allow / 10)


def check_trsm(c, r, rhs, k, what):
    """Forward result in X, forward + backward result in R, against the substitutions on the factor the device returned."""
    L = c.lay
    assert L.nEp <= 1024      # one wide block: the backward sweep leaves the forward result in X
    L0 = np.tril(r.f0[:L.nE, :L.nE])
    for backward, out in ((False, r.X), (True, r.R)):
        ref = util.nss_trsm_rows(L0, rhs[:, :L.nE], backward)
        check_c(out[:k, :L.nE], ref, util.nss_trsm_rows(L0, rhs[:, :L.nE], backward, np.float64), "%s %s trsm_rows backward=%d" % (c.name, what, backward))
    assert not r.R[:k, L.nE:].any()
    assert np.array_equal(r.X[:k, L.nE:], r.before["X"][:k, L.nE:])
    same(r, ["R", "X"], rows=k)


def check_factor_ortho(c, r, Sin, Gin, what):
    """FACTOR_N + ORTHO of one call: the factor by (c), the rows by (c) on the product branch and by (a) on k_ns_ortho."""
    L, k = c.lay, r.k
    assert r.res[0] == 0, what
    low = np.tril(np.ones((k, k), bool))
    Lf = np.where(low, r.SN[:k, :k], 0.0)
    Sl = np.where(low, Sin[:k, :k], 0.0)
    one = np.ones(k)
    # "the same algorithm in float64 NumPy" is the device's, restated from the panel kernels in util.nss_chol_blocked: 64-wide steps, the
    # diagonal block in 16-wide sub-blocks with reciprocal-square-root pivots, its explicit inverse by 16 x 16 blocks, the panel a product
    # with that inverse.  On P[J, J] of index-order columns (cond ~ 1e5) it leaves ten times what a column loop with divisions leaves, in
    # the same columns as the device.  Printed besides: the loop's error and the factor's residual over Higham's bound gamma_{k+1} |L||L'|.
    ref = util.nss_chol_guard(Sl, one, util.NS_WARM_THR)
    loop = float(np.abs(util.nss_chol_guard(Sl, one, util.NS_WARM_THR, np.float64).astype(LD) - ref).max() / np.abs(ref).max())
    if k <= 512:      # (measured only: the long-double products of a larger order take seconds)
        res, mag, _ = util.build_reference(Lf, np.ones(k))
        back, _ = util.rounding_bound_ratio(Sl, res, mag, np.tril(np.full((k, k), k - 1)))
        print("%s %s factor: float64 column loop errs %.2e; residual |S - L L'| / (gamma_{k+1} |L||L'|) = %.3e" % (c.name, what, loop, back))
    check_c(Lf, ref, util.nss_chol_blocked(Sl, one, util.NS_WARM_THR), "%s %s factor" % (c.name, what), k)
    if k <= L.wb:
        assert r.grid[1] == 0
        check_c(r.G[:k, :L.ldn], util.nss_ortho(Lf, Gin[:k, :L.ldn]), util.nss_ortho(Lf, Gin[:k, :L.ldn], np.float64), "%s %s ortho (product)" % (c.name, what), k)
    else:
        assert r.grid[1] == (L.ldn + 255) // 256
        val, mag, K = util.tw_nss_ortho_rows(Lf, Gin[:k, :L.ldn], r.G[:k, :L.ldn])
        ratio = util.bound_ratio(r.G[:k, :L.ldn], val, mag, K)
        note("k_ns_ortho", ratio)
        assert ratio <= 1.0
    assert np.array_equal(r.G[:, L.ldn:], Gin[:, L.ldn:])
    same(r, ["G"], rows=k)
    same(r, ["R", "X"])


_CHAIN = {}


def chain(c, fresh=False):
    """ns_basis_from(J) of the case one launch site at a time, every stage checked; its final Gt (shared by the tests below)."""
    if c.name in _CHAIN and not fresh:
        return _CHAIN[c.name]
    L, k, op, J = c.lay, c.k, c.op, c.J
    W = c.ref["dropped"]
    r1 = c.run(["s0_factor", ("rhs_cols", 0), ("trsm", 1)], J=J, big=False)
    assert r1.res[0] == W
    band = L.band if L.band > 0 else L.nE
    i, j = np.indices((L.nE, L.nE))
    inb = (j <= i) & (i - j <= band)
    assert np.array_equal(r1.Lt[:L.nE, :L.nE].T[inb], r1.f0[:L.nE, :L.nE][inb])      # the transposed copy, inside the band
    if W:
        assert (np.diag(r1.f0)[:L.nE] >= util.NS_BIG).sum() == W
    check_trsm(c, r1, util.tw_nss_rhs_cols(op, J), k, "first pass")
    r2 = c.run([("pj", 0), "gather_t"], J=J, R=r1.R)
    val, mag, K = util.tw_nss_pj(op, r1.R[:k], J)
    ratio = util.bound_ratio(r2.G[:k, :L.ldn], val, mag, K[None, :])
    note("k_ns_pj/0", ratio)
    assert ratio <= 1.0
    low = np.tril(np.ones((k, k), bool))
    assert np.array_equal(r2.SN[:k, :k][low], util.tw_nss_gather_t(r2.G, J)[low])
    r3 = c.run([("factor_n", 0, util.NS_WARM_THR), "ortho"], G=r2.G, SN=r2.SN)
    check_factor_ortho(c, r3, r2.SN, r2.G, "first pass")
    # second pass = ns_reproject
    r4 = c.run(["rows_e"], G=r3.G, big=True)
    val, mag, K = util.tw_nss_rows_e(op, r3.G[:k])
    ratio = util.bound_ratio(r4.R[:k], val, mag, K[None, :])
    note("k_ns_rows_e", ratio)
    assert ratio <= 1.0
    r5 = c.run(["s0_factor", ("trsm", 1)], R=r4.R, big=False)
    assert np.array_equal(r5.f0, r1.f0)
    check_trsm(c, r5, r4.R[:k], k, "second pass")
    r6 = c.run([("pj", 1), "gram"], J=J, G=r3.G, R=r5.R)
    val, mag, K = util.tw_nss_pj(op, r5.R[:k], J, r3.G[:k])
    ratio = util.bound_ratio(r6.G[:k, :L.ldn], val, mag, K[None, :])
    note("k_ns_pj/1", ratio)
    assert ratio <= 1.0
    ref, mag, _ = util.build_reference(r6.G[:k, :L.ldn], np.ones(L.ldn))
    ratio, _ = util.rounding_bound_ratio(r6.SN[:k, :k], ref, mag, np.tril(np.full((k, k), L.ldn)))
    note("gram", ratio)
    assert ratio <= 1.0
    r7 = c.run([("factor_n", 0, util.NS_WARM_THR), "ortho", "gi"], G=r6.G, SN=r6.SN)
    Gin = r6.G.copy()
    Gin[:k, L.ldn:] = r7.G[:k, L.ldn:]      # (GI' is the third stage's)
    check_factor_ortho(c, r7, r6.SN, Gin, "second pass")
    val, mag, K = util.tw_nss_gi(op, r7.G[:k])
    ratio = util.bound_ratio(r7.G[:k, L.ldn:], val, mag, K[None, :])
    note("k_ns_gi", ratio)
    assert ratio <= 1.0 and not r7.G[:k, L.ldn + L.nI:].any()
    _CHAIN[c.name] = r7.G
    return r7.G


_REFS = {}


def ref_chain(c, kind, Gw=None):
    """The float64 NumPy chain on the case's operand from the retained columns ("columns") or from the basis rows Gw ("basis"), once."""
    if (c.name, kind) not in _REFS:
        _REFS[(c.name, kind)] = util.nss_chain(c.op, np.float64, hint_J=c.J, warm_Z=None if Gw is None else Gw[:c.k, :c.lay.n], M=c.M)
    return _REFS[(c.name, kind)]


def neighbour(c, Gt):
    """The basis of a neighbouring LP: the case's own, every entry perturbed by 1e-3 relative, under SENTINEL rows."""
    Gw = np.full((c.lay.cap, c.lay.ldg), SENT)
    Gw[:c.k] = Gt[:c.k] * (1.0 + 1e-3 * np.random.default_rng(3).standard_normal((c.k, c.lay.ldg)))
    return Gw


def quality(c, Gt, ref64, what):
    """The three measures of the whole chain on a returned Gt, in long double on the device operand: within ten times the float64 NumPy
    chain's on the same data, and A_EF Z = 0 to 1e-13 as the active-set solves require."""
    L, k = c.lay, ref64["k"]
    dev = util.nss_quality(c.op, Gt[:k, :L.ldn], Gt[:k, L.ldn:])
    lvl = ref64.setdefault("quality", util.nss_quality(c.op, ref64["Zt"], ref64["GI"]))
    print("%s %s: |A_EF Zt'| %.1e (%.1e)  |Zt Zt' - I| %.1e (%.1e)  |GI' - (A_I Zt')'| %.1e (%.1e)   (float64 NumPy chain)" %
          (c.name, what, dev[0], lvl[0], dev[1], lvl[1], dev[2], lvl[2]))
    # (one basis row: the float64 chain's measures are a handful of roundings that may cancel to nothing, as in the sibling file's k = 1;
    # an entry of the row carries gamma_4 - pivot, square root, reciprocal, product - and the measures twice that)
    floor = 2.0 * float(util.gamma(4)) if k == 1 else 0.0
    for a, b in zip(dev, lvl):
        assert a <= max(10.0 * b, floor), what
    assert dev[0] <= 1e-13, what


@pytest.mark.parametrize("name", CASES)
def test_basis_from_stage_by_stage(cases, name):
    """Every launch site of ns_basis_from(J) in the solver's order, each on what the one before returned."""
    c = cases(name)
    Gt = chain(c, fresh=True)
    quality(c, Gt, ref_chain(c, "columns"), "stages")


@pytest.mark.parametrize("name", CASES)
def test_composites_equal_the_stages(cases, name):
    """ns_basis_from and ns_reproject as members: the same launches as the stages, so the same bits; a neighbouring LP's basis re-projected."""
    c = cases(name)
    L, k = c.lay, c.k
    Gt = chain(c)
    r = c.run(["s0_factor", "basis_from"], J=c.J)
    assert tuple(r.res) == (c.ref["dropped"], 1) and r.grid[1] == k
    assert np.array_equal(r.G[:k], Gt[:k])
    same(r, ["G", "R", "X"], rows=k)
    Gw = neighbour(c, Gt)
    r = c.run(["s0_factor", ("reproject", 0, util.NS_ZWARM_THR)], J=c.J, G=Gw)
    assert r.res[1] == 1 and r.grid[1] == (L.nEp + 255) // 256
    assert ref_chain(c, "basis", Gw)["path"] == "basis"
    quality(c, r.G, ref_chain(c, "basis", Gw), "reproject")
    same(r, ["G", "R", "X"], rows=k)


# ------------------------------------------------------------------------------------------------ ns_setup: the three paths and the refusals
def setup_result(r):
    s = r.setup
    return int(s[0]), int(s[1]), int(s[2]), s[4:4 + int(s[3])].copy()


@pytest.mark.parametrize("name", CASES)
def test_setup_paths(cases, name):
    c = cases(name)
    L, k, J = c.lay, c.k, c.J
    Gt = chain(c)
    W = c.ref["dropped"]
    r = c.run(["setup"])
    path, kk, dropped, Jd = setup_result(r)
    assert (path, kk, dropped) == (util.NSS_PATHS["cold"], k, W) and np.array_equal(Jd, J) and r.res[0] == 1
    assert np.array_equal(r.G[:k], Gt[:k])      # the cold selection ends in ns_basis_from on the same columns
    same(r, ["G", "R", "X"], rows=k)
    r = c.run(["setup"], hint=J)
    path, kk, dropped, Jd = setup_result(r)
    assert (path, kk, dropped) == (util.NSS_PATHS["columns"], k, W) and np.array_equal(Jd, J)
    assert np.array_equal(r.G[:k], Gt[:k])
    Gw = neighbour(c, Gt)
    ref = ref_chain(c, "basis", Gw)
    assert ref["path"] == "basis"
    r = c.run(["setup"], hint=J, G=Gw, Zk=k)
    path, kk, dropped, Jd = setup_result(r)
    assert (path, kk, dropped) == (util.NSS_PATHS["basis"], k, W) and np.array_equal(Jd, J)
    quality(c, r.G, ref, "setup from the previous basis")
    # a carried basis of another dimension is not tried
    r = c.run(["setup"], hint=J, G=Gw, Zk=k + 1)
    assert setup_result(r)[0] == util.NSS_PATHS["columns"] and np.array_equal(r.G[:k], Gt[:k])


def test_refusals(cases):
    c = cases("small")
    L, k = c.lay, c.k
    Gt = chain(c)
    J = c.J.copy()
    J[3] = J[2]
    assert util.nss_chain(c.op, np.float64, hint_J=J, M=c.M)["path"] == "cold"
    r = c.run(["s0_factor", "basis_from"], J=J)
    assert tuple(r.res) == (0, 0)
    r = c.run(["setup"], hint=J)
    path, kk, dropped, Jd = setup_result(r)
    assert path == util.NSS_PATHS["cold"] and np.array_equal(Jd, c.J) and np.array_equal(r.G[:k], Gt[:k])
    Gw = np.full((L.cap, L.ldg), SENT)
    Gw[:k] = Gt[:k]
    Gw[4] = Gw[9]
    assert util.nss_chain(c.op, np.float64, warm_Z=Gw[:k, :L.n], M=c.M)["path"] == "cold"
    r = c.run(["s0_factor", ("reproject", 0, util.NS_ZWARM_THR)], J=c.J, G=Gw)
    assert r.res[1] == 0
    r = c.run(["setup"], G=Gw, Zk=k)
    assert setup_result(r)[0] == util.NSS_PATHS["cold"] and np.array_equal(r.G[:k], Gt[:k])


def test_stale_rows(cases, hip_lib):
    """Two LPs of one skeleton on one handle: first the one with fewer fixed columns (k = 30), then the one with more (k = 24) in the same
    reservation - everything the first left in the k-sized buffers is still there.  The second result equals a fresh handle's bit for bit."""
    c = cases("small-reserve")
    assert c.kres == 30 and c.k == 24
    free = np.ones(c.n)
    ref1 = util.nss_chain(c.op.with_fm(free), np.float64, M=c.M)
    assert ref1["k"] == 30
    r1 = c.run(["setup"], k=30, fm=free)
    assert setup_result(r1)[:2] == (util.NSS_PATHS["cold"], 30) and np.array_equal(setup_result(r1)[3], ref1["J"])
    r2 = c.run(["setup"], G=r1.G, R=r1.R, X=r1.X, SN=r1.SN)      # (loading what the first call returned leaves the buffers as they were)
    fresh = Case(hip_lib, "small-reserve")
    try:
        r3 = fresh.run(["setup"])
    finally:
        fresh.close()
    assert setup_result(r2)[:3] == setup_result(r3)[:3] == (util.NSS_PATHS["cold"], 24, 0)
    assert np.array_equal(setup_result(r2)[3], setup_result(r3)[3])
    assert np.array_equal(r2.G[:24], r3.G[:24])
    assert np.array_equal(r2.G[24:], r1.G[24:])      # rows 24 .. 29 of the first LP's basis are nobody's now


def test_argument_errors_are_refused(cases, hip_lib):
    c = cases("small")
    k, n = c.k, c.n
    bad_fm = c.fm.copy()
    bad_fm[3] = 0.5
    J_hi, J_neg = c.J.copy(), c.J.copy()
    J_hi[0], J_neg[1] = n, -1
    for kw in (dict(k=0), dict(k=n + 1), dict(fm=bad_fm), dict(J=J_hi), dict(J=J_neg), dict(hint=J_hi), dict(Zk=-1), dict(Zk=c.lay.cap + 1)):
        c.run(["setup"], expect=ERR_ARG, **kw)
    for stages in ([("trsm", 1)], [("trsm", 0)], ["ortho"], ["ortho", ("factor_n", 0, 1e-6)], ["reproject"], ["basis_from"], [("pj", 2)], [("pj", -1)],
                   [("count_big", c.lay.ldT + 1)]):
        c.run(stages, J=c.J, expect=ERR_ARG)
    for stages in ([("rhs_cols", 0)], [("pj", 0)], ["gather_t"], ["s0_factor", "basis_from"]):
        c.run(stages, J=None, expect=ERR_ARG)
    lay = np.zeros(16, np.int64)
    assert c._call(k, k - 1, None, lay, None, None, {}, 0, None, None) == ERR_ARG                                       # k_reserve < k
    assert c._call(k, int(1.5 * util.NS_MAX_RATIO * c.M + 8) + 1, None, lay, None, None, {}, 0, None, None) == ERR_ARG     # beyond what ns_setup admits
    from activesetmethods_amd import _lib
    bad = (_lib.NssStage * 1)(_lib.NssStage(len(util.NSS_KINDS), 0, 0.0))
    g, rs = np.zeros(1, np.uint32), np.zeros(1, np.int32)
    assert hip_lib.asm_test_ns_setup_stages(c.h, _p(c.dE), _p(c.fm), k, k, None, _p(lay, C.c_int64), None, None, None, None, None, None, None, None, None, None, 0, None, 0,
                                            bad, 1, _p(g, C.c_uint32), _p(rs, C.c_int32), None) == ERR_ARG
    # a skeleton without the form
    h = util.abi_create(hip_lib)
    try:
        sp = util.random_subproblem(7, 96, 48)
        assert util.abi_setup(hip_lib, h, sp) == 0
        dE = np.ascontiguousarray(sp["dE"], np.float64)
        assert hip_lib.asm_test_ns_setup_stages(h, _p(dE), _p(np.ones(96)), 1, 1, None, _p(lay, C.c_int64), None, None, None, None, None, None, None, None, None, None, 0, None,
                                                0, None, 0, None, None, None) == ERR_ARG
    finally:
        assert hip_lib.asm_destroy(h) == 0
    # the handle still works
    r = c.run(["setup"])
    assert setup_result(r)[0] == util.NSS_PATHS["cold"]
