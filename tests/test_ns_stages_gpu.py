"""The kernels of one null-space interior-point iteration and of ns_finish_y (asm_ns_kernels.hip.h), one launch site at a time, as the solver
launches them.

The hook asm_test_ns_stages loads a caller-made state into buffers laid out with the solver's pitches, builds the CSC view and the index lists
with the solver's routines, factors the reduced matrix with the solver's factorisation and runs a list of stages through the launch-site members
the solver itself uses.  Assertions:
(a) the rounding bound |out - twin| <= gamma_k mag, element by element with constant 1, against the long-double twins of tests/util.py;
(b) exact statements, bit for bit against float64 NumPy (gathers, scatters, zeros on equality rows / fixed and padded columns, maxima, the two
    updates against each other, the guard of k_ns_update_dev);
(c) the reduced solves against the same algorithm in long double on the factor the device returned; allowance: ten times the error of the same
    algorithm in float64 NumPy on the same data.
Every buffer is pre-filled with util.SENTINEL or the loaded value; what a stage does not own comes back bit for bit.  grid_out is compared with
the documented rule of each launch site.  `pytest -s` prints the largest ratio of (a) per kernel."""
import ctypes as C

import numpy as np
import pytest

from activesetmethods_amd import _lib
from tests import util

pytestmark = pytest.mark.gpu
SC, LD, NSV = util.SC, util.LD, util.NS_VEC
KIND = {nm: i for i, nm in enumerate(util.NS_STAGE_KINDS)}
ERR_ARG = -1
# (n, M, k, nI): ldn padding 19 / 0 / 31 / 20; nI = 0, a single inequality row, nI > ldn; k on the one-workgroup path up to 256, 257 and 300 beyond
CASES = [(45, 40, 1, 0), (256, 255, 63, 1), (257, 257, 64, 100), (300, 330, 65, 70), (45, 330, 30, 300), (300, 255, 137, 60), (256, 257, 256, 40),
         (300, 330, 257, 70), (300, 330, 300, 70)]
IDS = ["n%d-M%d-k%d-nI%d" % c for c in CASES]
RATIOS = {}


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = C.c_void_p()
    assert hip_lib.asm_create(0, C.byref(h)) == 0
    yield h
    hip_lib.asm_destroy(h)
    for nm in sorted(RATIOS):
        print("largest ratio of (a), %-18s %.3f" % (nm, RATIOS[nm]))


_STATES = {}


def state(case):
    if case not in _STATES:
        _STATES[case] = util.ns_state(40 + CASES.index(case), *case)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _STATES[case].items()}


def stage(kind, **kw):
    s = _lib.NsStage()
    s.kind = KIND[kind]
    for k, v in kw.items():
        if k == "x":
            for i, e in enumerate(v):
                s.x[i] = int(e)
        else:
            setattr(s, k, {"A": 0, "C": 1}.get(v, v) if k in ("D", "B") else v)
    return s


def same(a, b):
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def blocks(cnt, per=256):
    return -(-cnt // per)


def grid_all(st):
    return blocks(max(st["n"], st["M"], 1))


def bound(name, out, tw):
    r = util.bound_ratio(out, *tw)
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    assert r <= 1.0, (name, r)


HEAD = "ldn Mp nEp nIp ldg fld nE nI end nscal scal th G g_rows S Linv linv_len N0 part small_use".split()


class Run:
    """One call of the hook on the state `st` (N, N0: the matrices of the solves; default the state's own)."""

    def __init__(self, lib, h, st, stages, extra=None, N=None, N0=None, hseq=7, expect=0, ptr=None, col=None, k=None):
        n, M, k = st["n"], st["M"], st["k"] if k is None else k
        self.st = st
        lo = np.zeros(20 + 16 + len(util.IPM_VECTORS), np.int64)
        rt = np.ascontiguousarray(st["rtype"], np.int32)
        u32 = C.POINTER(C.c_uint32)
        rc = lib.asm_test_ns_stages(h, n, M, k, st["scale_q"], _lib.i32ptr(rt), None, None, None, None, None, _lib.i64ptr(lo), None, None, 0, None, None, None, 0, None)
        if expect and rc != 0:
            self.rc = rc
            return
        assert rc == 0, lib.asm_last_error(h)
        for nm, v in zip(HEAD, lo[:20]):
            setattr(self, nm, int(v))
        self.nsv = [int(v) for v in lo[20:36]]
        self.off = {nm: int(o) for nm, o in zip(util.IPM_VECTORS, lo[36:])}
        nE, nI = int((rt == 0).sum()), int((rt != 0).sum())
        assert (self.ldn, self.Mp, self.nEp, self.nIp) == ((n + 31) // 32 * 32, (M + 15) // 16 * 16, (nE + 31) // 32 * 32, (max(nI, 1) + 31) // 32 * 32)
        assert (self.ldg, self.fld, self.nE, self.nI, self.g_rows, self.small_use) == (self.ldn + self.nIp, (k + 31) // 32 * 32, nE, nI, k + 1, util.NS_SMALL_USE)
        ne = 0 if extra is None else len(extra)
        blk = np.full(self.end + ne, util.SENTINEL)
        for nm in util.IPM_VECTORS:
            if nm in st and len(st[nm]):
                blk[self.off[nm]:self.off[nm] + len(st[nm])] = st[nm]
        blk[self.scal:self.scal + self.nscal] = st["scal"]
        blk[self.th:self.th + self.ldg] = 0.0
        blk[self.th:self.th + n] = st["th"]
        blk[self.th + self.ldn:self.th + self.ldn + nI] = st["thI"]
        for nm, w in NSV.items():
            blk[self.nsv[w]:self.nsv[w] + len(st[nm])] = st[nm]
        G = blk[self.G:self.G + k * self.ldg].reshape(k, self.ldg)
        G[:] = 0.0
        G[:, :n] = st["Zt"][:k]
        G[:, self.ldn:self.ldn + nI] = st["GI"][:k]
        if ne:
            blk[self.end:] = extra
        N0 = st["N0"] if N0 is None else N0
        N = st["N"] if N is None else N
        self.N0m, self.Nm = np.ascontiguousarray(N0[:k, :k]), np.ascontiguousarray(N[:k, :k])
        self.inp = blk.copy()
        self.hscal, self.hseq = np.full(self.nscal, util.SENTINEL), np.array([hseq], np.uint32)
        self.hscal_in = self.hscal.copy()
        ptr = st["ptr"] if ptr is None else ptr
        col = st["col"] if col is None else col
        nnz = len(st["col"])
        self.idx = np.full(n + 1 + 3 * nnz + nE + 2 * M + nI + 4, -99, np.int32)
        arr = (_lib.NsStage * max(len(stages), 1))(*stages)
        grid = np.zeros(max(len(stages), 1), np.uint32)
        self.rc = lib.asm_test_ns_stages(h, n, M, k, st["scale_q"], _lib.i32ptr(rt), _lib.i32ptr(np.ascontiguousarray(ptr, np.int32)),
                                         _lib.i32ptr(np.ascontiguousarray(col, np.int32)), _lib.dptr(st["vals"]), _lib.dptr(self.Nm), _lib.dptr(self.N0m), _lib.i64ptr(lo),
                                         _lib.i32ptr(self.idx), _lib.dptr(blk), len(blk), _lib.dptr(self.hscal), self.hseq.ctypes.data_as(u32), arr, len(stages),
                                         grid.ctypes.data_as(u32))
        if expect:
            assert self.rc == expect      # (every check of the hook comes before its first allocation and launch)
            return
        assert self.rc == 0, lib.asm_last_error(h)
        self.out, self.k = blk, k
        self.grid = [int(g) for g in grid[:len(stages)]]

    def v(self, nm, full=False):
        if nm in NSV:
            o, ln = self.nsv[NSV[nm]], (self.k if nm in ("ru", "du", "rr", "dd") else (self.st["M"] if nm in ("yM", "bI") else self.st["n"]))
            if full:
                ln = self.ldn
        else:
            o, ln = self.off[nm], util.ipm_vec_len(self.st, nm)
            if full:
                ln = self.ldn if nm in util.IPM_N else self.Mp
        return self.out[o:o + ln]

    def x(self, off, cnt):
        return self.out[self.end + off:self.end + off + cnt]

    def sc(self, nm):
        return float(self.out[self.scal + SC[nm]])

    def dev(self):
        """The state with every vector as the device returned it."""
        d = dict(self.st)
        for nm in util.IPM_VECTORS:
            if nm in d and len(d[nm]):
                d[nm] = self.v(nm).copy()
        for nm in NSV:
            d[nm] = self.v(nm).copy()
        return d

    def only(self, vecs=(), full=(), scal=(), extra=(), regions=(), pub=False):
        """Everything outside the named vectors (true lengths; `full`: up to the pitch), scalars, caller ranges and (offset, length) regions is bit
        for bit what went in - except N0 (stored by the hook), the scratch of Zt' u and, after a factorisation, the factor and its inverses."""
        own = np.zeros(len(self.out), bool)
        for nm in tuple(vecs) + tuple(full):
            f = nm in full
            o = self.nsv[NSV[nm]] if nm in NSV else self.off[nm]
            own[o:o + len(self.v(nm, f))] = True
        for nm in scal:
            own[self.scal + SC[nm]] = True
        for off, cnt in extra:
            own[self.end + off:self.end + off + cnt] = True
        for off, cnt in regions:
            own[off:off + cnt] = True
        own[self.part:self.end] = True
        N0 = self.out[self.N0:self.N0 + self.fld ** 2].reshape(self.fld, self.fld)
        N0in = self.inp[self.N0:self.N0 + self.fld ** 2].reshape(self.fld, self.fld).copy()
        k = self.k
        tri = np.tril(np.ones((k, k), bool))
        N0in[:k, :k][tri] = self.N0m[tri]
        if k <= util.NS_SMALL_USE:
            N0in[:k, :k][tri.T] = self.N0m.T[tri.T]
        assert same(N0, N0in), "N0 is not stored as ns_newton_matrix stores it"
        own[self.N0:self.N0 + self.fld ** 2] = True
        bits = lambda a: a.view(np.int64)
        assert np.array_equal(bits(self.out)[~own], bits(self.inp)[~own]), "a stage wrote outside what it owns"
        assert pub or (same(self.hscal, self.hscal_in) and self.hseq[0] == 7)

    def factor(self):
        S = self.out[self.S:self.S + self.fld ** 2].reshape(self.fld, self.fld)
        return S[:self.k, :self.k].copy()


def test_layout_csc_view_and_index_lists(hip_lib, handle):
    for case in CASES[:6]:
        st = state(case)
        r = Run(hip_lib, handle, st, [])
        r.only()
        n, M, nnz, A = st["n"], st["M"], len(st["col"]), st["A"]
        ix = r.idx
        sc_ptr, sc_row, sc_pos = ix[:n + 1], ix[n + 1:n + 1 + nnz], ix[n + 1 + nnz:n + 1 + 2 * nnz]
        o = n + 1 + 2 * nnz
        E, Epos, I, Ipos = ix[o:o + r.nE], ix[o + r.nE:o + r.nE + M], ix[o + r.nE + M:o + r.nE + M + r.nI], ix[o + r.nE + M + r.nI:o + r.nE + 2 * M + r.nI]
        assert np.array_equal(np.diff(sc_ptr), (A != 0).sum(0)) and sc_ptr[0] == 0
        rows_of = np.repeat(np.arange(M), np.diff(st["ptr"]))
        for j in range(n):
            seg = slice(sc_ptr[j], sc_ptr[j + 1])
            assert np.array_equal(sc_row[seg], np.flatnonzero(A[:, j])) and np.array_equal(st["col"][sc_pos[seg]], np.full(seg.stop - seg.start, j))
            assert np.array_equal(rows_of[sc_pos[seg]], sc_row[seg])
        assert np.array_equal(np.sort(E), st["E"]) and np.array_equal(I, st["I"])
        want_e, want_i = np.full(M, -1), np.full(M, -1)
        want_e[E], want_i[I] = np.arange(r.nE), np.arange(r.nI)
        assert np.array_equal(Epos, want_e) and np.array_equal(Ipos, want_i)
        st["Eidx"] = E


@pytest.mark.parametrize("case", CASES[:6], ids=IDS[:6])
def test_theta(hip_lib, handle, case):
    st = state(case)
    st["th"], st["thI"] = np.full(st["n"], 3.0), np.full(len(st["I"]), 5.0)
    r = Run(hip_lib, handle, st, [stage("theta", rho_p=util.IPM_RHO_P)])
    ex = util.ns_theta_exact(st, util.IPM_RHO_P)
    th = r.out[r.th:r.th + r.ldg]
    want = np.zeros(r.ldg)
    want[:st["n"]], want[r.ldn:r.ldn + r.nI] = ex["th"], ex["thI"]
    assert same(th, want) and same(r.v("thp_inv"), ex["thp_inv"]) and same(r.v("dS"), ex["dS"])
    assert np.all(th[:st["n"]][st["ub"] == st["lb"]] == 0)
    assert r.grid == [max(grid_all(st), blocks(max(r.ldn, r.nIp)))]
    r.only(vecs=["thp_inv", "dS"], regions=[(r.th, r.ldg)])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_iter_setup_stages(hip_lib, handle, case):
    """k_ns_e0, gemv_rows, ns_gemv_t_dense, k_ns_e1 (Solver::ns_split_e), then k_ns_spmvn_wm_neg and k_ns_spmvt_kx."""
    st = state(case)
    n, M, k = st["n"], st["M"], st["k"]
    fr = st["ub"] > st["lb"]
    ex = np.concatenate([st["pbar"], np.full(64, util.SENTINEL)])      # pbar (ldn)
    base = Run(hip_lib, handle, st, []).end
    r = Run(hip_lib, handle, st, [stage("e0", x=[base])], extra=ex)
    d0 = np.zeros(r.ldn)
    d0[:n] = np.where(fr, st["p"] - st["pbar"], 0.0)
    assert same(r.v("ht", True), d0) and r.grid == [blocks(r.ldn)]
    r.only(full=["ht"])
    # Zt d0 and Zt' (Zt d0), through the caller's vectors
    u = np.random.default_rng(5).standard_normal(k)
    ex = np.concatenate([d0, np.full(k, util.SENTINEL), u, np.full(r.ldn, util.SENTINEL)])
    r = Run(hip_lib, handle, st, [stage("zt", x=[base, base + r.ldn]), stage("gemv_t", x=[base + r.ldn + k, base + r.ldn + 2 * k])], extra=ex)
    bound("gemv_rows", r.x(r.ldn, k), util.tw_ns_zt(st, d0[:n]))
    zu = r.x(r.ldn + 2 * k, r.ldn)
    bound("gemv_t", zu[:n], util.tw_ns_gemv_t(st, u))
    assert np.all(zu[n:] == 0)      # (Zt is zero in the padding columns)
    R = min(-(-k // 32), 128)
    chunk = -(-k // R)
    assert r.grid == [blocks(k, 4), blocks(r.ldn) if k <= util.NS_SMALL_USE else blocks(r.ldn) * -(-k // chunk)]
    r.only(extra=[(r.ldn, k), (r.ldn + 2 * k, r.ldn)])
    st["ht"] = d0[:n]
    r = Run(hip_lib, handle, st, [stage("e1")])
    e = np.full(r.ldn, 0.0)
    e[:n] = np.where(fr, st["ht"] - st["v"], 0.0)
    assert same(r.v("e", True), e) and r.grid == [blocks(r.ldn)]
    r.only(full=["e"])
    # dpbar = -e over the whole pitch (threads beyond M negate too), the residual measure cleared, wM
    st = state(case)
    st["scal"][SC["NSERR"]] = 0.37
    r = Run(hip_lib, handle, st, [stage("wm_neg")])
    tw = util.tw_ns_wm_neg(st)
    e_in = r.inp[r.nsv[14]:r.nsv[14] + r.ldn]
    assert same(r.v("dpb", True), -e_in) and r.sc("NSERR") == 0.0 and not np.signbit(r.sc("NSERR"))
    bound("k_ns_spmvn_wm_neg", r.v("yM"), tw["yM"])
    assert np.all(r.v("yM")[st["rtype"] == 0] == 0)
    assert r.grid == [max(blocks(M), blocks(r.ldn))]
    r.only(full=["dpb"], vecs=["yM"], scal=["NSERR"])
    r = Run(hip_lib, handle, st, [stage("kx")])
    bound("k_ns_spmvt_kx", r.v("kdpb"), util.tw_ns_kx(st)["kdpb"])
    assert fr[n - 2] and r.v("kdpb")[n - 2] != st["th"][n - 2] * st["dpb"][n - 2]      # the seven entries of the last free column are in the sum
    assert np.all(r.v("kdpb", True)[:n][~fr] == 0) and np.all(r.v("kdpb", True)[n:] == 0) and r.grid == [blocks(r.ldn * 8)]
    r.only(full=["kdpb"])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_newton_stages(hip_lib, handle, case, mode):
    """k_ns_rhs1_bi, k_ns_spmvt_ht, ru = Zt v, the direction (k_gemv_t_small_dp, or Zt' du + k_ns_dp) and k_ns_spmvn_rows, each from the same state."""
    st = state(case)
    n, M, k = st["n"], st["M"], st["k"]
    fr, eq = st["ub"] > st["lb"], st["rtype"] == 0
    base, D = ("A", "C") if mode else ("A", "A")
    r = Run(hip_lib, handle, st, [stage("rhs1_bi", mode=mode, B=base, res=1.0)])
    d = r.dev()
    tw = util.tw_ns_rhs1_bi(st, base, mode, 1.0, d)
    for nm in ("rcL", "rcU", "rcg", "hp", "tmpn", "bI"):
        bound("k_ns_rhs1_bi", r.v(nm), tw[nm])
    assert same(r.v("yM"), tw["yM_exact"]) and np.all(r.v("bI")[eq] == 0) and np.all(r.v("yM")[eq] == 0) and np.all(r.v("hp")[~fr] == 0)
    assert r.grid == [grid_all(st)]
    r.only(vecs=["rcL", "rcU", "rcg", "hp", "tmpn", "bI", "yM"])
    r = Run(hip_lib, handle, st, [stage("ht", res=1.0)])
    tw = util.tw_ns_ht(st, 1.0, r.dev())
    bound("k_ns_spmvt_ht", r.v("ht"), tw["ht"])
    bound("k_ns_spmvt_ht", r.v("v"), tw["v"])
    assert fr[n - 2] and r.v("ht")[n - 2] != st["hp"][n - 2]      # the seven entries of the last free column are in the sum
    for nm in ("ht", "v"):
        assert np.all(r.v(nm, True)[:n][~fr] == 0) and np.all(r.v(nm, True)[n:] == 0)
    assert r.grid == [blocks(r.ldn * 8)]
    r.only(full=["ht", "v"])
    r = Run(hip_lib, handle, st, [stage("ru")])
    bound("gemv_rows", r.v("ru"), util.tw_ns_zt(st, st["v"]))
    assert r.grid == [blocks(k, 4)]
    r.only(vecs=["ru"])
    r = Run(hip_lib, handle, st, [stage("direction", D=D, res=1.0)])
    tw = util.tw_ns_dp(st, D, 1.0, r.dev())
    name = "k_gemv_t_small_dp" if k <= util.NS_SMALL_USE else "k_ns_dp"
    for nm in (".dp", ".dmuL", ".dmuU"):
        bound(name, r.v(D + nm), tw[D + nm])
        assert np.all(r.v(D + nm)[~fr] == 0)
    assert np.all(r.v(D + ".dp", True)[n:] == 0) and r.grid == [blocks(r.ldn)]
    r.only(full=[D + ".dp"], vecs=[D + ".dmuL", D + ".dmuU"] + ([] if k <= util.NS_SMALL_USE else ["v"]), regions=[] if k <= util.NS_SMALL_USE else [(r.nsv[3], r.ldn)])
    if k > util.NS_SMALL_USE:      # k_ns_dp alone, Z du given
        zu = np.concatenate([np.random.default_rng(3).standard_normal(n), np.zeros(r.ldn - n)])
        r = Run(hip_lib, handle, st, [stage("dp", D=D, res=1.0, x=[r.end])], extra=zu)
        bound("k_ns_dp", r.v(D + ".dp"), util.tw_ns_dp(st, D, 1.0, r.dev(), zu=zu[:n])[D + ".dp"])
        r.only(full=[D + ".dp"], vecs=[D + ".dmuL", D + ".dmuU"])
    r = Run(hip_lib, handle, st, [stage("rows", D=D)])
    d = r.dev()
    tw = util.tw_ns_rows(st, D, d)
    for nm, key in ((D + ".dy", D + ".dy"), (D + ".dg", D + ".dg"), ("yM", "yM")):
        bound("k_ns_spmvn_rows", r.v(nm), tw[key])
        assert np.all(r.v(nm)[eq] == 0)
    assert same(r.v(D + ".dpi"), tw[D + ".dpi_exact"]) and r.grid == [blocks(M)]
    r.only(vecs=[D + ".dy", D + ".dpi", D + ".dg", "yM"])


def spd(seed, k, cond):
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((k, k)))[0]
    N0 = (Q * np.logspace(0, np.log10(cond), k)) @ Q.T if k > 1 else np.array([[2.5]])
    N0 = 0.5 * (N0 + N0.T)
    N = N0.copy()
    d = np.arange(k)
    N[d, d] = N0[d, d] + (1e-13 * N0[d, d] + 1e-30)
    return N0, N


def solve_checks(r, st, N0, ru, du, nserr, prev, name):
    """(c): du against the long-double twin of the algorithm on the device's own factor, allowance ten times float64 NumPy's error on the same
    data; SC_NSERR against its statement recomputed in long double from the device's du, to the rounding bound of that product."""
    Lf = r.factor()
    ref, _ = util.tw_ns_reduced_solve(Lf, N0, ru)
    f64, _ = util.tw_ns_reduced_solve(Lf, N0, ru, np.float64)
    scale = float(np.abs(ref).max())
    allow = 10.0 * float(np.abs(f64.astype(LD) - ref).max()) / scale
    err = float(np.abs(du.astype(LD) - ref).max()) / scale
    print("%s k=%d: du error %.2e, float64 NumPy %.2e" % (name, len(ru), err, allow / 10))
    assert allow > 0 and err <= allow
    val, mag, kk = util.tw_ns_symv_res(N0, du, ru)
    m = max(1.0, float(np.abs(ru).max()))
    b = util.gamma(kk) * mag      # the device's residual entries lie within b of the exact ones
    lo, hi = float(max(((np.abs(val) - b) / m).max(), 0.0)), float(((np.abs(val) + b) / m).max())
    want_lo, want_hi = max(prev, lo), max(prev, hi)
    assert want_lo * (1 - 4 * util.U) <= nserr <= want_hi * (1 + 4 * util.U), (nserr, want_lo, want_hi)


@pytest.mark.parametrize("cond", [1e2, 1e8])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 137, 256, 257, 300])
def test_reduced_solves(hip_lib, handle, k, cond):
    case = (300, 330, k, 70)
    st = util.ns_state(11, *case)
    N0, N = spd(k, k, cond)
    rng = np.random.default_rng(k)
    st["ru"] = rng.standard_normal(k)
    b2 = rng.standard_normal(k)
    st["scal"][SC["NSERR"]] = 0.0
    ex = np.concatenate([b2, np.full(k, util.SENTINEL)])
    probe = Run(hip_lib, handle, st, [], N=N, N0=N0)
    r = Run(hip_lib, handle, st, [stage("factor"), stage("chol_solve", x=[probe.end, probe.end + k]), stage("reduced_solve")], extra=ex, N=N, N0=N0)
    small = k <= util.NS_SMALL_USE
    assert r.grid == [0, 1 if small else 0, 1 if small else blocks(k, 4)]
    r.only(vecs=["du"] + ([] if small else ["rr", "dd"]), scal=["NSERR"], extra=[(k, k)], regions=[(r.S, r.fld ** 2 + r.linv_len)])
    S = r.out[r.S:r.S + r.fld ** 2].reshape(r.fld, r.fld)
    assert np.all(S[k:, :] == 0) and np.all(S[:, k:] == 0), "the factorisation wrote beyond order k"
    Lf = r.factor()
    # Dev::chol_solve_dev (k_small_solve up to 256) against the substitution in long double on the returned factor
    ref = util.ns_ld_chol_solve(Lf, None, b2)
    from scipy.linalg import solve_triangular
    f64 = solve_triangular(np.tril(Lf).T, solve_triangular(np.tril(Lf), b2, lower=True), lower=False)
    allow = 10.0 * float(np.abs(f64.astype(LD) - ref).max())
    err = float(np.abs(r.x(k, k).astype(LD) - ref).max())
    print("chol_solve_dev k=%d cond %.0e: error %.2e, float64 NumPy %.2e" % (k, cond, err, allow / 10))
    assert err <= allow or k == 1
    if k == 1:      # (one division each way: float64 NumPy is almost exact and measures no allowance; the quotient to four roundings instead)
        assert abs(r.x(1, 1)[0] - b2[0] / N[0, 0]) <= 4 * util.U * abs(b2[0] / N[0, 0])
    solve_checks(r, st, N0, st["ru"], r.v("du"), r.sc("NSERR"), 0.0, "reduced solve cond %.0e" % cond)


@pytest.mark.parametrize("k", [137, 300])
def test_nserr_accumulates_over_two_solves_and_keeps_a_larger_value(hip_lib, handle, k):
    st = util.ns_state(12, 300, 330, k, 70)
    N0, N = spd(k + 1, k, 1e8)
    rng = np.random.default_rng(k)
    st["ru"] = rng.standard_normal(k)
    st["scal"][SC["NSERR"]] = 0.25
    # cleared by k_ns_spmvn_wm_neg, then two solves of the same system: the second keeps the first one's value (same data: equal)
    r = Run(hip_lib, handle, st, [stage("wm_neg"), stage("factor"), stage("reduced_solve")], N=N, N0=N0)
    one = r.sc("NSERR")
    solve_checks(r, st, N0, st["ru"], r.v("du"), one, 0.0, "after clearing")
    r2 = Run(hip_lib, handle, st, [stage("wm_neg"), stage("factor"), stage("reduced_solve"), stage("reduced_solve")], N=N, N0=N0)
    assert r2.sc("NSERR") == one and same(r2.v("du"), r.v("du"))
    # a larger earlier value stays
    r3 = Run(hip_lib, handle, st, [stage("factor"), stage("reduced_solve")], N=N, N0=N0)
    assert r3.sc("NSERR") == 0.25 and one < 0.25


def test_relres_drops_a_nan_and_keeps_its_slot(hip_lib, handle):
    """One ordinary k_ns_relres launch on the caller's vectors: a NaN in the residual is dropped by the maxima (fmax), as by the oracle's max()."""
    st, k = state(CASES[5]), CASES[5][2]
    rng = np.random.default_rng(k)
    rr, rhs = rng.standard_normal(k), rng.standard_normal(k)
    rr[k // 2] = np.nan
    st["scal"][SC["NSERR"]] = 1e-3
    b = Run(hip_lib, handle, st, []).end
    r4 = Run(hip_lib, handle, st, [stage("relres", x=[b, b + k])], extra=np.concatenate([rr, rhs]))
    assert r4.sc("NSERR") == util.ns_relres_exact(1e-3, rr, rhs) and r4.grid == [1]
    r4.only(scal=["NSERR"])


def test_both_solve_paths_agree_at_256_and_257(hip_lib, handle):
    """The same 256 x 256 system through k_ns_reduced_solve (k = 256) and, bordered by a unit row, through the multi-launch sequence (k = 257)."""
    N0, N = spd(77, 256, 1e8)
    ru = np.random.default_rng(8).standard_normal(256)
    B0, B = np.eye(257), np.eye(257)
    B0[:256, :256], B[:256, :256] = N0, N
    B[256, 256] = 1.0 + (1e-13 + 1e-30)
    out = []
    for k, a0, a, b in ((256, N0, N, ru), (257, B0, B, np.concatenate([ru, [0.5]]))):
        st = util.ns_state(13, 300, 330, k, 70)
        st["ru"] = b
        r = Run(hip_lib, handle, st, [stage("factor"), stage("reduced_solve")], N=a, N0=a0)
        ref, _ = util.tw_ns_reduced_solve(r.factor(), a0, b)
        f64, _ = util.tw_ns_reduced_solve(r.factor(), a0, b, np.float64)
        out.append((r.v("du")[:256].copy(), 10.0 * float(np.abs(f64.astype(LD) - ref).max())))
    assert np.abs(out[0][0] - out[1][0]).max() <= out[0][1] + out[1][1]


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[5], CASES[7]], ids=[IDS[0], IDS[2], IDS[5], IDS[7]])
def test_multi_launch_pieces_and_finish_y_kernels(hip_lib, handle, case):
    """k_ns_symv_res, k_ns_add, k_ns_relres, k_ns_dinf with their own operands; k_ns_gather_e, k_ns_scatter_e (add = 0 and 1), k_ns_rowvec_e, k_ns_fill."""
    st = state(case)
    n, M, k = st["n"], st["M"], st["k"]
    rng = np.random.default_rng(21)
    x, rhs = rng.standard_normal(k), rng.standard_normal(k)
    probe = Run(hip_lib, handle, st, [])
    b, nE = probe.end, probe.nE
    E = probe.idx[n + 1 + 2 * len(st["col"]):][:nE]
    ex = np.concatenate([x, rhs, np.full(2 * k, util.SENTINEL)])
    st["scal"][SC["NSERR"]] = 1e-9
    r = Run(hip_lib, handle, st, [stage("symv_res", x=[b, b + k, b + 2 * k]), stage("add", x=[b, b + k, b + 3 * k], len=k), stage("relres", x=[b + 2 * k, b + k]),
                                  stage("dinf", x=[b], pub=41)], extra=ex)
    N0 = st["N0"] if k <= util.NS_SMALL_USE else np.tril(st["N0"]) + np.tril(st["N0"], -1).T
    bound("k_ns_symv_res", r.x(2 * k, k), util.tw_ns_symv_res(N0, x, rhs))
    assert same(r.x(3 * k, k), x + rhs)
    assert r.sc("NSERR") == util.ns_relres_exact(1e-9, r.x(2 * k, k), rhs)
    assert r.sc("DINF") == float(np.abs(x).max()) / st["scale_q"]
    assert r.grid == [blocks(k, 4), blocks(k), 1, 1]
    want = r.out[r.scal:r.scal + r.nscal]
    assert same(r.hscal, want) and r.hseq[0] == 41      # published through the host-mapped block, then the sequence word
    r.only(scal=["NSERR", "DINF"], extra=[(2 * k, 2 * k)], pub=True)
    rM, tE = rng.standard_normal(M), rng.standard_normal(nE)
    outM = rng.standard_normal(M)
    ex = np.concatenate([rM, np.full(nE, util.SENTINEL), tE, outM, outM, np.full(M, util.SENTINEL), np.full(33, util.SENTINEL)])
    o_g, o_t, o_s0, o_s1, o_rv, o_f = M, M + nE, M + 2 * nE, 2 * M + 2 * nE, 3 * M + 2 * nE, 4 * M + 2 * nE
    r = Run(hip_lib, handle, st, [stage("gather_e", x=[b, b + o_g], scale=-0.5), stage("scatter_e", x=[b + o_t, b + o_s0], add=0),
                                  stage("scatter_e", x=[b + o_t, b + o_s1], add=1), stage("rowvec_e", x=[b + o_t, b + o_rv]),
                                  stage("fill", x=[b + o_f], val=1.0, len=31)], extra=ex)
    assert same(r.x(o_g, nE), -0.5 * rM[E])
    s0, s1, rv = outM.copy(), outM.copy(), np.zeros(M)
    s0[E], rv[E] = 0.0 + tE, tE
    s1[E] = outM[E] + tE
    assert same(r.x(o_s0, M), s0) and same(r.x(o_s1, M), s1) and same(r.x(o_rv, M), rv) and same(r.x(o_f, 33), [1.0] * 31 + [util.SENTINEL] * 2)
    assert r.grid == [blocks(nE), blocks(nE), blocks(nE), blocks(M), 1]
    r.only(extra=[(o_g, nE), (o_s0, 2 * M), (o_rv, M), (o_f, 31)])


@pytest.mark.parametrize("case", CASES[:6], ids=IDS[:6])
def test_updates(hip_lib, handle, case):
    st = state(case)
    n, M = st["n"], st["M"]
    fr, eq = st["ub"] > st["lb"], st["rtype"] == 0
    eta, rerr = 0.995, 1e-6
    st["scal"][SC["AP"]], st["scal"][SC["AD"]], st["scal"][SC["NSERR"]] = 0.75, 1.3, rerr      # exactly at the bound: the update happens
    al, be = min(1.0, eta * 0.75), min(1.0, eta * 1.3)
    owned = ["p", "tL", "tU", "muL", "muU", "g", "pi", "y"]
    r = Run(hip_lib, handle, st, [stage("update", D="C", al=al, be=be, es=1.0 - al)])
    tw = util.tw_ns_update(st, "C", al, be, 1.0 - al, r.dev())
    for nm in owned:
        bound("k_ns_update", r.v(nm), tw[nm])
    e_in = r.inp[r.nsv[14]:r.nsv[14] + r.ldn]
    assert same(r.v("e", True), e_in * (1.0 - al))
    assert np.all(r.v("tL")[~fr] == 1) and np.all(r.v("tU")[~fr] == 1) and np.all(r.v("g")[eq] == 1) and r.grid == [grid_all(st)]
    r.only(vecs=owned, full=["e"])
    r2 = Run(hip_lib, handle, st, [stage("update_dev", D="C", eta=eta, rerr=rerr)])
    assert same(r2.out, r.out) and r2.grid == [grid_all(st)]
    st["scal"][SC["NSERR"]] = float(np.nextafter(rerr, 1.0))      # above the bound: every vector, e included, untouched
    r3 = Run(hip_lib, handle, st, [stage("update_dev", D="C", eta=eta, rerr=rerr)])
    r3.only()


def twin_chain(st, Lf, eta, ap, ad, f64):
    """The iteration from the twins: every stage the float64 rounding of its long-double value, the reduced solve in long double on the device's
    own factor.  f64: the same algorithm with every sum of products and the reduced solve in plain float64 NumPy (the measured allowance)."""
    t = {kk: (v.copy() if isinstance(v, np.ndarray) else v) for kk, v in st.items()}
    fr, on, A, Zt = t["ub"] > t["lb"], t["th"] != 0, t["A"], t["Zt"]
    thI = np.zeros(t["M"])
    thI[t["I"]] = t["thI"]
    r64 = lambda v: np.asarray(v, np.float64)
    t.update(util.ns_theta_exact(t, util.IPM_RHO_P))
    d0 = np.where(fr, t["p"] - t["pbar"], 0.0)
    zz = Zt.T @ (Zt @ d0) if f64 else r64(util.tw_ns_gemv_t(t, r64(util.tw_ns_zt(t, d0)[0]))[0])
    t["e"] = np.where(fr, d0 - zz, 0.0)
    t["dpb"] = -t["e"]
    t["yM"] = thI * (A @ t["dpb"]) if f64 else r64(util.tw_ns_wm_neg(t)["yM"][0])
    t["kdpb"] = np.where(on, t["th"] * t["dpb"] + A.T @ t["yM"], 0.0) if f64 else r64(util.tw_ns_kx(t)["kdpb"][0])
    nserr = 0.0
    for mode, base, D in ((0, "A", "A"), (1, "A", "C")):
        util._f(util.tw_rhs1(t, base, mode), t, ["rcL", "rcU", "rcg"])
        util._f(util.tw_rhs1(t, base, mode, dev=dict(t, hp=t["hp"])), t, ["hp"])
        util._f(util.tw_rhs1(t, base, mode, dev=t), t, ["tmpn"])
        util._f(util.tw_ns_rhs1_bi(t, base, mode, 1.0, dict(t)), t, ["bI"])
        t["yM"] = util.tw_ns_rhs1_bi(t, base, mode, 1.0, dict(t))["yM_exact"]
        if f64:
            t["ht"] = np.where(on, t["hp"] + A.T @ t["yM"], 0.0)
        else:
            util._f(util.tw_ns_ht(t, 1.0, dict(t)), t, ["ht"])
        util._f(util.tw_ns_ht(t, 1.0, dict(t)), t, ["v"])
        t["ru"] = Zt @ t["v"] if f64 else r64(util.tw_ns_zt(t, t["v"])[0])
        t["du"] = r64(util.tw_ns_reduced_solve(Lf, t["N0"], t["ru"], np.float64 if f64 else LD)[0])
        nserr = util.ns_relres_exact(nserr, r64(util.tw_ns_symv_res(t["N0"], t["du"], t["ru"])[0]), t["ru"])
        if f64:
            t[D + ".dp"] = np.where(on, t["dpb"] + Zt.T @ t["du"], 0.0)
        else:
            util._f(util.tw_ns_dp(t, D, 1.0, dict(t)), t, [D + ".dp"])
        util._f(util.tw_ns_dp(t, D, 1.0, dict(t)), t, [D + ".dmuL", D + ".dmuU"])
        if f64:
            t[D + ".dy"] = thI * (t["bI"] - A @ t[D + ".dp"])
        else:
            util._f(util.tw_ns_rows(t, D, dict(t)), t, [D + ".dy"])
        t[D + ".dpi"] = util.tw_ns_rows(t, D, dict(t))[D + ".dpi_exact"]
        t2 = util.tw_ns_rows(t, D, dict(t))
        t[D + ".dg"], t["yM"] = r64(t2[D + ".dg"][0]), (thI * (A @ t[D + ".dp"]) if f64 else r64(t2["yM"][0]))
        if mode == 0:
            t["scal"][SC["SM"]] = 0.3 * t["scal"][SC["MU"]]
    al, be = min(1.0, eta * ap), min(1.0, eta * ad)
    new_pi = r64(util.tw_update(t, "C", al, be, {"pi": t["pi"]})["pi"][0])
    tu = util.tw_ns_update(t, "C", al, be, 1.0 - al, {"pi": new_pi})
    util._f(tu, t)
    return t, tu["e_exact"], nserr


@pytest.mark.parametrize("k", [137, 257])
def test_one_chained_iteration(hip_lib, handle, k):
    """theta~, the split of e, dpbar / K dpbar, the predictor, the corrector and the update on a 300-column LP, against the same chain of twins.
    (k = 300 has no positive definite N on a 300-column LP with fixed columns: the multi-launch path is chained at k = 257.)"""
    st = util.ns_state(31, 300, 330, k, 70, mu=1e-2)
    n = st["n"]
    f = Run(hip_lib, handle, st, [stage("factor")])
    Lf = f.factor()
    eta, ap, ad = 0.995, 0.8, 0.6
    t, e_tw, nserr = twin_chain(st, Lf, eta, ap, ad, False)
    t64, e_64, _ = twin_chain(st, Lf, eta, ap, ad, True)
    # the device: SM as the twin loads it (0 is not read in mode 0), AP / AD for k_ns_update_dev
    st["scal"][SC["SM"]], st["scal"][SC["AP"]], st["scal"][SC["AD"]] = 0.3 * st["scal"][SC["MU"]], ap, ad
    probe = Run(hip_lib, handle, st, [])
    b = probe.end
    ex = np.concatenate([st["pbar"], np.zeros(probe.ldn - n)])
    stages = [stage("theta", rho_p=util.IPM_RHO_P), stage("factor"), stage("e0", x=[b]), stage("zt", x=[probe.nsv[2], probe.nsv[12]]), stage("gemv_t", x=[probe.nsv[12], probe.nsv[3]]), stage("e1"),
              stage("wm_neg"), stage("kx"), stage("newton", mode=0, B="A", D="A"), stage("newton", mode=1, B="A", D="C"),
              stage("update_dev", D="C", eta=eta, rerr=1e-6)]
    r = Run(hip_lib, handle, st, stages, extra=ex)
    assert r.sc("NSERR") <= 1e-6
    # allowance: the rule of tests/test_ns_stages_cpu.py on this very data - ten times what the same chain in plain float64 NumPy (another
    # evaluation order of every sum and of the reduced solve) differs from the long-double twin chain by
    names = ("p", "tL", "tU", "muL", "muU", "g", "pi", "y")
    rel = lambda a, b_: float(np.abs(a - b_).max() / max(np.abs(b_).max(), 1e-300))
    level = max([rel(t64[nm], t[nm]) for nm in names] + [rel(e_64, e_tw)])
    worst = max([rel(r.v(nm), t[nm]) for nm in names] + [rel(r.v("e"), e_tw)])
    print("chained iteration k=%d: device vs twin chain %.2e, float64 NumPy vs twin chain %.2e, NSERR device %.2e twin %.2e" % (k, worst, level, r.sc("NSERR"), nserr))
    assert level > 0 and worst <= 10.0 * level


def test_argument_errors_are_refused(hip_lib, handle):
    st = state(CASES[3])
    col = st["col"].copy()
    col[len(col) // 2] = st["n"]
    Run(hip_lib, handle, st, [stage("kx")], col=col, expect=ERR_ARG)
    Run(hip_lib, handle, st, [stage("reduced_solve"), stage("factor")], expect=ERR_ARG)
    r = Run(hip_lib, handle, st, [stage("kx")], k=st["n"] + 1, expect=ERR_ARG)
    assert r.rc == ERR_ARG
    ptr = st["ptr"].copy()
    ptr[3], ptr[4] = ptr[4] + 1, ptr[3]
    Run(hip_lib, handle, st, [stage("kx")], ptr=ptr, expect=ERR_ARG)
    st["rtype"][1] = 2
    r = Run(hip_lib, handle, st, [stage("kx")], expect=ERR_ARG)
    assert r.rc == ERR_ARG
