"""The interior-point stage kernels (asm_ipm_kernels.hip.h), one launch at a time, as the solver launches them.

The hook asm_test_ipm_stages loads a caller-made state into an arena laid out by Solver::ipm_bind and runs a list of stages through the
launch-site members the solver itself uses.  Three kinds of assertion:
(a) the rounding bound |out - ref| <= gamma_k mag, element by element with constant 1, against the long-double twin of tests/util.py (k = the
    operation count of the statement plus one; valid with or without FMA contraction) - a theorem, not a tuned tolerance;
(b) exact statements wherever no a*b +/- c shape exists: bitwise equal to float64 NumPy (step lengths, maxima, theta, the start point,
    copies, constants of fixed columns and equality rows, snapshot round trips, SC_SPEC / SC_STOP logic, publishing, rcnt == 0);
(c) the ratio test takes its minimum from exactly the eligible entries: a unique binding ratio planted at the edges of wavefronts, sweeps,
    workgroup shares and index ranges, among decoys that must be ignored.
Every buffer is pre-filled with util.SENTINEL or the loaded value; what a stage does not own comes back bit for bit (padding up to the
pitches, P.aty in k_ipm_dir, rpart beyond gridDim * 8 included).  `pytest -s` prints the largest ratio of (a) per case."""
import ctypes as C

import numpy as np
import pytest

from activesetmethods_amd import _lib
from tests import util

pytestmark = pytest.mark.gpu
SC = util.SC
KIND = {nm: i for i, nm in enumerate(util.IPM_STAGE_KINDS)}
MUS = util.IPM_MUS
CASE_IDS = ["n%d-M%d-ns%d" % c for c in util.IPM_CASES]


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = C.c_void_p()
    assert hip_lib.asm_create(0, C.byref(h)) == 0
    yield h
    hip_lib.asm_destroy(h)


def stage(kind, **kw):
    s = _lib.IpmStage()
    s.kind = KIND[kind]
    for k, v in kw.items():
        if k in ("x", "ix", "len"):
            for i, e in enumerate(v):
                getattr(s, k)[i] = int(e)
        else:
            setattr(s, k, {"A": 0, "C": 1}.get(v, v) if k in ("D", "B") else v)
    return s


class Layout:
    def __init__(self, lib, h, n, M, ns):
        out = np.zeros(8 + len(util.IPM_VECTORS), np.int64)
        rc = lib.asm_test_ipm_stages(h, n, M, ns, 1, 1.0, _lib.i64ptr(out), None, 0, None, 0, None, None, None, None, None, None, 0, None)
        assert rc == 0, lib.asm_last_error(h)
        self.ldn, self.Mp, self.nsp, self.arena, self.snap, self.ints, self.nscal, self.scal = (int(v) for v in out[:8])
        self.off = {nm: int(o) for nm, o in zip(util.IPM_VECTORS, out[8:])}
        assert self.nscal == len(util.IPM_SCALARS)
        assert (self.ldn, self.Mp, self.nsp) == ((n + 31) // 32 * 32, (max(M, 1) + 15) // 16 * 16, (max(ns, 1) + 15) // 16 * 16)


class Run:
    """One call of the hook.  `prev`: continue from the buffers another run returned instead of loading the state."""

    def __init__(self, lib, h, st, stages, extra=None, iextra=None, prev=None, hseq=7, snap=None):
        n, M, ns = st["n"], st["M"], st["ns"]
        self.st, self.lay = st, Layout(lib, h, n, M, ns)
        lay = self.lay
        ne = 0 if extra is None else len(extra)
        if prev is None:
            blk = np.full(lay.arena + ne, util.SENTINEL)
            for nm in util.IPM_VECTORS:
                blk[lay.off[nm]:lay.off[nm] + len(st[nm])] = st[nm]
            blk[lay.scal:lay.scal + lay.nscal] = st["scal"]
            if ne:
                blk[lay.arena:] = extra
            self.snap = np.full(lay.snap, util.SENTINEL) if snap is None else snap.copy()
            self.rpart = np.full(64 * 8, util.SENTINEL)
            self.rcnt = np.zeros(1, np.uint32)
            self.hscal = np.full(lay.nscal, util.SENTINEL)
            self.hseq = np.array([hseq], np.uint32)
        else:
            blk = prev.out.copy()
            self.snap, self.rpart, self.rcnt, self.hscal, self.hseq = prev.snap.copy(), prev.rpart.copy(), prev.rcnt.copy(), prev.hscal.copy(), prev.hseq.copy()
        ints = np.full(lay.ints + (0 if iextra is None else len(iextra)), -1, np.int32)
        ints[:M] = st["rtype"]
        ints[lay.Mp:lay.Mp + M] = st["rs0"]
        ints[2 * lay.Mp:2 * lay.Mp + M] = st["rs1"]
        ints[3 * lay.Mp:3 * lay.Mp + ns] = st["srow"]
        if iextra is not None:
            ints[lay.ints:] = iextra
        self.inp = blk.copy()
        self.rpart_in, self.hscal_in, self.hseq_in, self.snap_in = self.rpart.copy(), self.hscal.copy(), self.hseq.copy(), self.snap.copy()
        arr = (_lib.IpmStage * max(len(stages), 1))(*stages)
        self.grid = np.zeros(max(len(stages), 1), np.uint32)
        u32 = C.POINTER(C.c_uint32)
        rc = lib.asm_test_ipm_stages(h, n, M, ns, st["ncomp"], st["scale_q"], _lib.i64ptr(np.zeros(8 + len(util.IPM_VECTORS), np.int64)), _lib.dptr(blk), len(blk),
                                     _lib.i32ptr(ints), len(ints), _lib.dptr(self.snap), _lib.dptr(self.rpart), self.rcnt.ctypes.data_as(u32), _lib.dptr(self.hscal),
                                     self.hseq.ctypes.data_as(u32), arr, len(stages), self.grid.ctypes.data_as(u32))
        assert rc == 0, lib.asm_last_error(h)
        self.out = blk
        self.grid = [int(g) for g in self.grid[:len(stages)]]

    def v(self, nm):
        o = self.lay.off[nm]
        return self.out[o:o + util.ipm_vec_len(self.st, nm)]

    def x(self, off, cnt):
        return self.out[self.lay.arena + off:self.lay.arena + off + cnt]

    def sc(self, nm):
        return float(self.out[self.lay.scal + SC[nm]])

    def only(self, vecs=(), scal=(), extra=(), snap=False, red=0, pub=False):
        """Everything outside the named vectors (true lengths), scalars and [off, off + cnt) ranges of the caller's vectors is bit for bit
        what went in; so are the snapshot, rpart beyond red * 8 entries, the host-mapped block and the sequence word unless named."""
        own = np.zeros(len(self.out), bool)
        for nm in vecs:
            o = self.lay.off[nm]
            own[o:o + util.ipm_vec_len(self.st, nm)] = True
        for nm in scal:
            own[self.lay.scal + SC[nm]] = True
        for off, cnt in extra:
            own[self.lay.arena + off:self.lay.arena + off + cnt] = True
        bits = lambda a: a.view(np.int64)
        assert np.array_equal(bits(self.out)[~own], bits(self.inp)[~own]), "a stage wrote outside what it owns"
        assert snap or np.array_equal(bits(self.snap), bits(self.snap_in))
        assert np.array_equal(bits(self.rpart)[red * 8:], bits(self.rpart_in)[red * 8:])
        assert pub or (np.array_equal(bits(self.hscal), bits(self.hscal_in)) and self.hseq[0] == self.hseq_in[0])
        assert self.rcnt[0] == 0


def same(a, b):
    """Bitwise equality of float64 arrays / scalars (distinguishes -0.0 from 0.0, treats equal NaNs as equal)."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def bound(run, tw, names, worst, tag):
    for nm in names:
        val, mag, k = tw[nm]
        out = run.sc(nm) if nm in SC else run.v(nm)
        r = util.bound_ratio(out, val, mag, k)
        worst[tag + ":" + nm] = max(worst.get(tag + ":" + nm, 0.0), r)
        assert r <= 1.0, (tag, nm, r)


def grids(st):
    return util.ipm_red_grid(st["n"], st["M"], st["ns"]), util.ipm_grid_all(st["n"], st["M"], st["ns"])


make_state = util.ipm_stage_state


@pytest.mark.parametrize("case", range(len(util.IPM_CASES)), ids=CASE_IDS)
def test_every_stage_alone(hip_lib, handle, case):
    st = make_state(case)
    n, M, ns = st["n"], st["M"], st["ns"]
    gr, ga = grids(st)
    fr, ineq = st["ub"] > st["lb"], st["rtype"] != 0
    worst = {}
    go = lambda stages, **kw: Run(hip_lib, handle, st, stages, **kw)

    # k_ipm_measures
    r = go([stage("measures", pub=0)])
    assert r.grid == [gr]
    r.only(vecs=["rp", "rdp", "rds"], scal=["PINF", "DINF", "MU", "YMAX", "RPMAX"], red=gr if gr > 1 else 0)
    bound(r, util.tw_measures(st), ["rp", "rdp", "rds", "MU"], worst, "measures")
    for nm, want in util.ipm_measures_exact(st, r.v("rp"), r.v("rdp"), r.v("rds")).items():
        assert same(r.sc(nm), want), nm
    assert same(r.v("rdp")[~fr], np.zeros(int((~fr).sum())))
    # k_ipm_theta
    r = go([stage("theta", rho_p=util.IPM_RHO_P)])
    assert r.grid == [ga]
    r.only(vecs=["thp_inv", "ths_inv", "dS"])
    for nm, want in util.ipm_theta_exact(st, util.IPM_RHO_P).items():
        assert same(r.v(nm), want), nm
    # k_ipm_rhs1, three modes, base direction A and C
    for mode, base, tp, td in ((0, "A", 0.0, 0.0), (1, "A", 0.0, 0.0), (1, "C", 0.0, 0.0), (2, "C", 0.8, 0.55)):
        r = go([stage("rhs1", mode=mode, B=base, tp=tp, td=td)])
        assert r.grid == [ga]
        r.only(vecs=["rcL", "rcU", "rcs", "rcg", "hp", "hs", "tmpn"])
        dev = {nm: r.v(nm) for nm in ("rcL", "rcU", "rcs", "hp")}
        bound(r, util.tw_rhs1(st, base, mode, tp, td, dev), ["rcL", "rcU", "rcs", "rcg", "hp", "hs", "tmpn"], worst, "rhs1-%d" % mode)
        assert same(r.v("hp")[~fr], np.zeros(int((~fr).sum())))
    # k_ipm_rhs2
    for res in (1.0, 0.0):
        r = go([stage("rhs2", res=res)])
        assert r.grid == [ga]
        r.only(vecs=["rhs"])
        bound(r, util.tw_rhs2(st, res), ["rhs"], worst, "rhs2")
    # k_vec_mul as the solver uses it (tN *= thp_inv)
    lay = Layout(hip_lib, handle, n, M, ns)
    r = go([stage("vec_mul", x=[lay.off["tN"], lay.off["thp_inv"]], len=[n])])
    assert r.grid == [(n + 255) // 256]
    r.only(vecs=["tN"])
    assert same(r.v("tN"), st["tN"] * st["thp_inv"])
    # k_ipm_res
    r = go([stage("res", D="C", pub=0, spec=0)])
    assert r.grid == [1]
    r.only(vecs=["res"], scal=["EMAX", "RMAX"])
    bound(r, util.tw_res(st, "C"), ["res"], worst, "res")
    for nm, want in util.ipm_res_exact(st, r.v("res"), 0, 0.0, 0.0).items():
        assert same(r.sc(nm), want), nm
    # k_pcg_start / step1 / step2
    r = go([stage("pcg_start")])
    r.only(vecs=["pcg"], scal=["RZ", "RZ0", "STOP"])
    assert same(r.v("pcg"), st["corr"]) and same(r.sc("RZ0"), r.sc("RZ")) and same(r.sc("STOP"), 0.0)
    bound(r, util.tw_pcg_start(st), ["RZ"], worst, "pcg_start")
    tw = util.tw_pcg_step1(st, "A")
    r = go([stage("pcg_step1", D="A", pub=0)])
    if tw["ok"]:
        assert tw["kappa"] < 1e3
        r.only(vecs=["A.dy", "res"], scal=["EMAX"])
        bound(r, {"A.dy": tw["x"], "res": tw["res"]}, ["A.dy", "res"], worst, "pcg_step1")
        assert same(r.sc("EMAX"), float(np.abs(r.v("res")).max(initial=0.0)))
    else:
        assert M == 0
        r.only(scal=["STOP"])
        assert same(r.sc("STOP"), 1.0)
    tw = util.tw_pcg_step2(st)
    r = go([stage("pcg_step2")])
    r.only(vecs=["pcg"], scal=["RZ"])
    assert tw["kappa"] < 1e3                                      # (the magnitude of pcg is scaled by it: a cancelling r'z would make the bound vacuous)
    bound(r, tw, ["RZ", "pcg"], worst, "pcg_step2")
    # k_ipm_dir
    for D in ("A", "C"):
        r = go([stage("dir", D=D)])
        assert r.grid == [ga]
        own = [D + "." + c for c in ("dp", "dmuL", "dmuU", "ds", "dmus", "dpi", "dg")]
        r.only(vecs=own)                                           # (P.aty and D.dy among what is not touched)
        dev = {nm: r.v(nm) for nm in own}
        bound(r, util.tw_dir(st, D, dev), [nm for nm in own if not nm.endswith("dpi")], worst, "dir")
        assert same(r.v(D + ".dpi"), util.ipm_dir_exact(st, D)[D + ".dpi"])
        assert same(r.v(D + ".dmuL")[~fr], np.zeros(int((~fr).sum()))) and same(r.v(D + ".dg")[~ineq], np.zeros(int((~ineq).sum())))
    # k_ipm_steps
    for D in ("A", "C"):
        r = go([stage("steps", D=D, pub=0)])
        assert r.grid == [gr]
        r.only(scal=["AP", "AD"], red=gr if gr > 1 else 0)
        for nm, want in util.ipm_steps_exact(st, D).items():
            assert same(r.sc(nm), want), nm
    # k_ipm_muaff
    for sexp in (2, 3, 4):
        r = go([stage("muaff", D="A", sexp=sexp)])
        assert r.grid == [gr]
        r.only(scal=["SM"], red=gr if gr > 1 else 0)
        tw = util.tw_muaff(st, "A", sexp)
        bound(r, tw, ["SM"], worst, "muaff")
        # The exact statement SM = r^sexp mu needs the accumulator the device summed, and only a multi-workgroup launch leaves it behind (the
        # partials in rpart, added in workgroup order); a single workgroup keeps it in a register, so there the bound on the power is all
        # that can be asserted - it does not tell r*r*r from another evaluation of the power, the exact check at grid > 1 does.
        if gr > 1:
            acc = 0.0
            for w in range(gr):
                acc += r.rpart[8 * w]
            assert util.bound_ratio(acc, *tw["acc"]) <= 1.0
            assert same(r.sc("SM"), util.ipm_sm_exact(acc, st["ncomp"], st["scal"][SC["MU"]], sexp))
    # k_ipm_diradd
    r = go([stage("diradd", D="A", B="C")])
    assert r.grid == [ga]
    comps = ("dp", "dmuL", "dmuU", "ds", "dmus", "dg", "dy", "dpi")
    r.only(vecs=["A." + c for c in comps])
    for c in comps:
        assert same(r.v("A." + c), st["A." + c] + st["C." + c]), c
    # k_ipm_update
    r = go([stage("update", D="C", al=0.37, be=0.81)])
    assert r.grid == [ga]
    own = ["p", "tL", "tU", "muL", "muU", "s", "ts", "mus", "g", "pi", "y"]
    r.only(vecs=own)
    bound(r, util.tw_update(st, "C", 0.37, 0.81, {"pi": r.v("pi")}), own, worst, "update")
    nf, ne = int((~fr).sum()), int((~ineq).sum())
    assert same(r.v("tL")[~fr], np.ones(nf)) and same(r.v("tU")[~fr], np.ones(nf)) and same(r.v("g")[~ineq], np.ones(ne))
    assert same(r.v("y")[ineq], (st["rtype"] * r.v("pi"))[ineq])
    # k_ipm_init_p / k_ipm_init_rest
    for origin in (0, 1):
        r = go([stage("init_p", origin=origin)])
        assert r.grid == [ga]
        r.only(vecs=["p", "s"])
        for nm, want in util.ipm_init_exact(st, origin, 1.0).items():
            assert same(r.v(nm), want), nm
    for muf in (1.0, 0.3):
        r = go([stage("init_rest", mu_factor=muf)])
        assert r.grid == [ga]
        want = util.ipm_init_rest_exact(st, muf)
        r.only(vecs=list(want))
        for nm in want:
            assert same(r.v(nm), want[nm]), nm
        assert same(r.v("muL")[~fr], np.zeros(nf)) and same(r.v("pi")[~ineq], np.zeros(ne)) and same(r.v("g")[~ineq], np.ones(ne))
    # column-form helpers on vectors of the caller's: dinv | th | r | u | w | out, pitched by Mp / ldn with the pre-fill between them
    Mp, ldn = lay.Mp, lay.ldn
    op = util.ipm_helper_operands(case, st)
    ex = np.full(5 * Mp + ldn, util.SENTINEL)
    o_dinv, o_th, o_r, o_u, o_w, o_out = 0, Mp, Mp + ldn, 2 * Mp + ldn, 3 * Mp + ldn, 4 * Mp + ldn
    ex[o_r:o_r + M], ex[o_w:o_w + M] = op["r"], op["w"]
    A0 = lay.arena
    r = go([stage("col_prep", rho_p=util.IPM_RHO_P, fixed=util.COL_FIXED, x=[A0 + o_dinv, A0 + o_th])], extra=ex)
    assert r.grid == [ga]
    r.only(extra=[(o_dinv, M), (o_th, n)])
    dinv, th = util.ipm_col_prep_exact(st, util.IPM_RHO_P, util.COL_FIXED)
    assert same(r.x(o_dinv, M), dinv) and same(r.x(o_th, n), th)
    ex[o_dinv:o_dinv + M] = dinv
    r = go([stage("col_scale", x=[A0 + o_dinv, A0 + o_r, A0 + o_u])], extra=ex)
    assert r.grid == [(M + 255) // 256]
    r.only(extra=[(o_u, M)])
    assert same(r.x(o_u, M), dinv * ex[o_r:o_r + M])
    ex[o_u:o_u + M] = dinv * ex[o_r:o_r + M]
    r = go([stage("col_finish", x=[A0 + o_dinv, A0 + o_u, A0 + o_w, A0 + o_out])], extra=ex)
    assert r.grid == [(M + 255) // 256]
    r.only(extra=[(o_out, M)])
    rr = util.bound_ratio(r.x(o_out, M), *util.tw_col_finish(dinv, ex[o_u:o_u + M], ex[o_w:o_w + M]))
    worst["col_finish"] = rr
    assert rr <= 1.0
    # reduced-row helpers: kept rows E (a non-monotone list), dropped rows I with their diagonal; CSR rows with 0 .. 9 entries
    if M > 0:
        E, I, ptr, col = op["E"], op["I"], op["ptr"], op["col"]
        nE, nI, nnz, cnt = len(E), len(I), len(col), np.diff(ptr)
        iex = np.concatenate([E, I, ptr, col]).astype(np.int32)
        i_E, i_I, i_ptr, i_col = lay.ints, lay.ints + nE, lay.ints + M, lay.ints + 2 * M + 1
        # doubles: r (M) | ce (nE) | ze (nE) | dI (nI) | z (M) | vals (nnz) | out (M), one pre-filled entry between neighbours
        sizes = [M, nE, nE, nI, M, nnz, M]
        offs = np.concatenate([[0], np.cumsum([s + 1 for s in sizes])])[:-1]
        ex = np.full(int(sum(sizes)) + len(sizes), util.SENTINEL)
        o_r, o_ce, o_ze, o_dI, o_z, o_vals, o_out = (int(o) for o in offs)
        ex[o_r:o_r + M], ex[o_ze:o_ze + nE] = op["r"], op["ze"]
        ex[o_dI:o_dI + nI], ex[o_vals:o_vals + nnz] = op["dI"], op["vals"]
        r = go([stage("red_gather", ix=[i_E], len=[nE, M], x=[A0 + o_r, A0 + o_ce])], extra=ex, iextra=iex)
        assert r.grid == [(nE + 255) // 256]
        r.only(extra=[(o_ce, nE)])
        assert same(r.x(o_ce, nE), ex[o_r:o_r + M][E])
        r = go([stage("red_scatter", ix=[i_E, i_I], len=[nE, nI, M], x=[A0 + o_ze, A0 + o_dI, A0 + o_r, A0 + o_z])], extra=ex, iextra=iex)
        assert r.grid == [(M + 255) // 256]
        r.only(extra=[(o_z, M)])
        z = np.empty(M)
        z[E] = ex[o_ze:o_ze + nE]
        z[I] = ex[o_r:o_r + M][I] / ex[o_dI:o_dI + nI]
        assert same(r.x(o_z, M), z)
        r = go([stage("sdiag_csr", ix=[i_ptr, i_col], len=[M, n], x=[A0 + o_vals, lay.off["thp_inv"], A0 + o_out])], extra=ex, iextra=iex)
        assert r.grid == [(M + 255) // 256]
        r.only(extra=[(o_out, M)])
        rr = util.bound_ratio(r.x(o_out, M), *util.tw_sdiag_csr(ptr, col, ex[o_vals:o_vals + nnz], st["thp_inv"]))
        worst["sdiag_csr"] = rr
        assert rr <= 1.0 and same(r.x(o_out, M)[cnt == 0], np.zeros(int((cnt == 0).sum())))
    top = max(worst.values())
    print("ratio stages %-24s mu %.0e grid %2d: largest %.3e (%s)" % (CASE_IDS[case], st["scal"][SC["MU"]], gr, top, max(worst, key=worst.get)))


@pytest.mark.parametrize("case", range(len(util.IPM_CASES)), ids=CASE_IDS)
def test_ratio_test_takes_exactly_the_eligible_entries(hip_lib, handle, case):
    """A note on the clamped loads.  A thread with t beyond a range re-reads that range's LAST element (index clamped) and must not count
    it.  Selecting with `t <= len` instead of `t < len` counts it once more - and into a minimum that is no change at all: for the column
    range (n >= 1 always) and for a non-empty slack range the mutant is equivalent, no output of k_ipm_steps can differ, and the sums of
    k_ipm_muaff / k_ipm_measures, where a second count would show, run their own unclamped loops.  Where it is NOT equivalent is an empty
    range: with M = 0 the clamped index 0 reads the padding (row type -1 and the pre-fill of g, dg, pi, dpi), which then enters the minimum
    as -1; the case n256-M0-ns0 catches exactly that (with ns = 0 the kernel substitutes ts = 1, ds = 0, so nothing is read)."""
    base = util.ipm_decoy_state(case, MUS)
    gr, _ = grids(base)
    want0 = util.ipm_steps_exact(base, "A")
    r = Run(hip_lib, handle, base, [stage("steps", D="A", pub=0)])
    assert r.grid == [gr] and same(r.sc("AP"), want0["AP"]) and same(r.sc("AD"), want0["AD"])      # the decoys alone change nothing
    npos = 0
    for rg, pos in util.ipm_planted_positions(base):
        st, ap, ad = util.ipm_plant(base, "A", rg, pos)
        r = Run(hip_lib, handle, st, [stage("steps", D="A", pub=0), stage("muaff", D="A", sexp=3)])
        assert r.grid == [gr, gr]
        assert same(r.sc("AP"), ap) and same(r.sc("AD"), ad), (rg, pos, r.sc("AP"), ap, r.sc("AD"), ad)
        st2 = dict(st, scal=st["scal"].copy())
        st2["scal"][SC["AP"]], st2["scal"][SC["AD"]] = ap, ad
        assert util.bound_ratio(r.sc("SM"), *util.tw_muaff(st2, "A", 3)["SM"]) <= 1.0, (rg, pos)      # every pair counted once on the same data
        npos += 1
    # ties: the same binding ratio at two places of different ranges
    st, ap, ad = util.ipm_plant(base, "A", "n", 0)
    if base["M"] > 0:
        st, ap2, ad2 = util.ipm_plant(st, "A", "M", base["M"] - 1, ratios=(ap, ad))
        assert (ap2, ad2) == (ap, ad)
    r = Run(hip_lib, handle, st, [stage("steps", D="A", pub=0)])
    assert same(r.sc("AP"), ap) and same(r.sc("AD"), ad)
    # no negative component at all: both steps are 1
    st = dict(base)
    for c in ("dp", "ds", "dg", "dmuL", "dmuU", "dmus", "dpi"):
        st["A." + c] = np.abs(base["A." + c])
    st["A.dp"] = np.where(base["ub"] > base["lb"], 0.0, -1.0)      # (dp enters with both signs: only the fixed columns keep a negative one)
    r = Run(hip_lib, handle, st, [stage("steps", D="A", pub=0)])
    assert same(r.sc("AP"), 1.0) and same(r.sc("AD"), 1.0)
    print("ratio test %-24s grid %2d: %d planted positions" % (CASE_IDS[case], gr, npos))


MULTI = [i for i, c in enumerate(util.IPM_CASES) if util.ipm_red_grid(*c) > 1]


@pytest.mark.parametrize("case", MULTI, ids=[CASE_IDS[i] for i in MULTI])
def test_reductions_back_to_back_share_the_arrival_counter(hip_lib, handle, case):
    """measures, steps, muaff, steps queued as one list (no host synchronisation in between) give the bits of the four run one at a time, a
    repeated launch gives the same bits, and the counter is 0 after every one."""
    st = make_state(case)
    seq = [stage("measures", pub=0), stage("steps", D="A", pub=0), stage("muaff", D="A", sexp=3), stage("steps", D="C", pub=0)]
    one = Run(hip_lib, handle, st, seq)
    assert one.rcnt[0] == 0
    step = None
    for s in seq:
        step = Run(hip_lib, handle, st, [s], prev=step)
        assert step.rcnt[0] == 0
    assert same(one.out, step.out) and same(one.rpart, step.rpart)
    again = Run(hip_lib, handle, st, seq)
    assert same(again.out, one.out) and same(again.rpart, one.rpart)
    twice = Run(hip_lib, handle, st, seq + seq)
    assert twice.rcnt[0] == 0
    for nm in ("PINF", "DINF", "MU", "YMAX", "RPMAX", "AP", "AD", "SM"):
        assert same(twice.sc(nm), one.sc(nm)), nm


@pytest.mark.parametrize("case", [3, 6, 12], ids=[CASE_IDS[i] for i in (3, 6, 12)])
def test_publishing(hip_lib, handle, case):
    """pub != 0: the host-mapped block equals the device block and the sequence word is pub; pub == 0: both untouched."""
    st = make_state(case)
    brk = dict(st, scal=st["scal"].copy())
    brk["scal"][SC["RZ"]] = -1.0                     # early-return branch of k_pcg_step1
    for name, s, state in (("measures", stage("measures", pub=41), st), ("steps", stage("steps", D="C", pub=42), st), ("res", stage("res", D="A", pub=43, spec=1, crel=1e-10), st),
                           ("step1", stage("pcg_step1", D="A", pub=44), st), ("step1-stop", stage("pcg_step1", D="A", pub=45), brk)):
        r = Run(hip_lib, handle, state, [s])
        assert same(r.hscal, r.out[r.lay.scal:r.lay.scal + r.lay.nscal]) and r.hseq[0] == s.pub, name
        s.pub = 0
        q = Run(hip_lib, handle, state, [s])
        assert same(q.hscal, q.hscal_in) and q.hseq[0] == 7 and same(q.out, r.out), name
    assert same(r.sc("STOP"), 1.0)


@pytest.mark.parametrize("case", [2, 4, 8], ids=[CASE_IDS[i] for i in (2, 4, 8)])
def test_res_verdict_and_pcg_breakdown(hip_lib, handle, case):
    st = make_state(case)
    r0 = Run(hip_lib, handle, st, [stage("res", D="A", pub=0, spec=0)])
    emax, rmax = r0.sc("EMAX"), r0.sc("RMAX")
    assert same(r0.sc("SPEC"), st["scal"][SC["SPEC"]])                       # spec = 0 leaves it alone
    # threshold max(crel rmax, floor) just below, at and just above emax, through the floor and through crel
    for thr, bad in ((np.nextafter(emax, np.inf), 0.0), (emax, 0.0), (np.nextafter(emax, 0.0), 1.0)):
        for old in (0.0, 1.0):
            s2 = dict(st, scal=st["scal"].copy())
            s2["scal"][SC["SPEC"]] = old
            r = Run(hip_lib, handle, s2, [stage("res", D="A", pub=0, spec=1, crel=0.0, floor_=thr)])
            r.only(vecs=["res"], scal=["EMAX", "RMAX", "SPEC"])
            assert same(r.sc("SPEC"), bad)                                   # spec = 1 sets
            r = Run(hip_lib, handle, s2, [stage("res", D="A", pub=0, spec=2, crel=0.0, floor_=thr)])
            assert same(r.sc("SPEC"), max(old, bad))                         # spec = 2 ORs
            assert same(r.v("res"), r0.v("res"))
    crel = emax / rmax
    for c in (crel, np.nextafter(crel, 0.0), np.nextafter(crel, np.inf)):
        r = Run(hip_lib, handle, st, [stage("res", D="A", pub=0, spec=1, crel=c, floor_=0.0)])
        assert same(r.sc("SPEC"), 1.0 if emax > max(c * rmax, 0.0) else 0.0)
    # k_pcg_step1: every breakdown branch stops and leaves x, res and EMAX alone; the normal branch leaves STOP alone
    tw = util.tw_pcg_step1(st, "A")
    assert tw["ok"]
    acc = float(tw["acc"])
    neg = dict(st, sres=-st["sres"] - 2.0 * st["dS"] * st["pcg"])            # p'Sp < 0
    nan = dict(st, sres=st["sres"].copy())
    nan["sres"][st["M"] // 2] = np.nan                                       # NaN accumulator
    cases = [("p'Sp<=0", neg, None), ("nan", nan, None), ("rz<=1e-30rz0", st, (1e-31, 1.0)), ("rz>=1e12p'Sp", st, (1e13 * acc, 1e13 * acc))]
    for name, state, rz in cases:
        for stop0 in (0.0, 0.25):
            s2 = dict(state, scal=state["scal"].copy())
            s2["scal"][SC["STOP"]] = stop0
            if rz:
                s2["scal"][SC["RZ"]], s2["scal"][SC["RZ0"]] = rz
            r = Run(hip_lib, handle, s2, [stage("pcg_step1", D="A", pub=0)])
            r.only(scal=["STOP"])
            assert same(r.sc("STOP"), 1.0), name
    s2 = dict(st, scal=st["scal"].copy())
    s2["scal"][SC["STOP"]] = 0.25
    r = Run(hip_lib, handle, s2, [stage("pcg_step1", D="A", pub=0)])
    assert same(r.sc("STOP"), 0.25)


@pytest.mark.parametrize("case", [1, 2, 7, 11], ids=[CASE_IDS[i] for i in (1, 2, 7, 11)])
def test_snapshot_round_trip(hip_lib, handle, case):
    st = make_state(case)
    lay = Layout(hip_lib, handle, st["n"], st["M"], st["ns"])
    it = ["p", "tL", "tU", "muL", "muU", "g", "y", "pi", "s", "ts", "mus"]
    e = np.random.default_rng(case).standard_normal(lay.ldn)
    for with_e in (0, 1):
        save = Run(hip_lib, handle, st, [stage("snapshot", dir=0, with_e=with_e, x=[lay.arena])], extra=e)
        save.only(snap=True)                                                 # a save writes the snapshot only
        rows = save.snap[:5 * lay.ldn].reshape(5, lay.ldn)
        for k, nm in enumerate(it[:5]):
            assert same(rows[k][:st["n"]], st[nm]) and np.all(rows[k][st["n"]:] == util.SENTINEL)
        erow = save.snap[5 * lay.ldn:6 * lay.ldn]
        assert same(erow, e) if with_e else np.all(erow == util.SENTINEL)
        # scramble the iterate (and e), then restore from the snapshot the save wrote
        rng = np.random.default_rng(3 + case)
        sc = dict(st)
        for nm in it:
            sc[nm] = rng.standard_normal(len(st[nm]))
        rest = Run(hip_lib, handle, sc, [stage("snapshot", dir=1, with_e=with_e, x=[lay.arena])], extra=rng.standard_normal(lay.ldn), snap=save.snap)
        rest.only(vecs=it, extra=[(0, lay.ldn)] if with_e else [])             # a restore writes the iterate (and e) only
        for nm in it:
            assert same(rest.v(nm), st[nm]), nm
        if with_e:
            assert same(rest.x(0, lay.ldn), e)


@pytest.mark.parametrize("case", [0, 5], ids=[CASE_IDS[i] for i in (0, 5)])
def test_centring_is_zero_without_complementarity(hip_lib, handle, case):
    st = make_state(case)
    st["scal"][SC["MU"]] = 0.0
    for sexp in (2, 3, 4):
        r = Run(hip_lib, handle, st, [stage("muaff", D="A", sexp=sexp)])
        assert same(r.sc("SM"), 0.0)
