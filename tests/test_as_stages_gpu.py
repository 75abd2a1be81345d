"""The active-set and optimal-face kernels (asm_as_kernels.hip.h), one launch at a time, as the solver launches them.

The hook asm_test_as_stages loads a caller-made state into arenas laid out by Solver::as_bind and runs a list of stages through the launch-site
members the solver itself uses.  Per kernel and case, one hook call and these assertions:
(a) rounding-bound outputs: |out - twin| <= gamma_k magnitude with constant 1 against the long-double twin of tests/util.py;
(b) exact outputs - sets, counters, index lists, masks, padding that k_as_setup owns, clips, gathers, scatters, the pack layout - bitwise /
    integer equal to the twin;
(c) ownership: every double and int of the two blocks that the kernel does not own comes back bit for bit (pre-fill util.SENTINEL / util.ISENT or
    the loaded state);
(d) geometry: grid_out equals the formula of the launch site;
(e) planted ties decide as < / <= / >= dictate, and k_face_ns_step reports an eligible entry with the minimal ratio;
(g) the one-workgroup kernels give bit-identical blocks when run twice.
`pytest -s` prints the largest ratio of (a) per kernel."""
import ctypes as C

import numpy as np
import pytest

from activesetmethods_amd import _lib
from tests import util

pytestmark = pytest.mark.gpu
KIND = {nm: i for i, nm in enumerate(util.AS_KINDS)}
AC, AS = util.AC, util.AS
CASES = [(c, rp) for c in util.AS_CASES for rp in (0, 1)]
CASE_IDS = ["n%d-M%d-ns%d-%s" % (c + (("natural", "rperm")[rp],)) for c, rp in CASES]
WORST = {}


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = C.c_void_p()
    assert hip_lib.asm_create(0, C.byref(h)) == 0
    yield h
    hip_lib.asm_destroy(h)
    for k in sorted(WORST):
        print("largest ratio of (a), %-14s %.3f" % (k, WORST[k]))


def stage(kind, **kw):
    s = _lib.AsStage()
    s.kind = KIND[kind]
    for k, v in kw.items():
        if k in ("x", "set"):
            for i, e in enumerate(v):
                getattr(s, k)[i] = int(e)
        else:
            setattr(s, k, v)
    return s


class Layout:
    def __init__(self, lib, h, n, M, ns):
        out = np.zeros(9 + len(util.AS_VECTORS) + len(util.AS_IVECTORS), np.int64)
        rc = lib.asm_test_as_stages(h, n, M, ns, 1.0, _lib.i64ptr(out), None, 0, None, 0, None, 0, None, 0, None)
        assert rc == 0, lib.asm_last_error(h)
        self.ldn, self.Mp, self.nsp, self.ndbl, self.nint, self.scal, nscal, self.cnt, ncnt = (int(v) for v in out[:9])
        assert (nscal, ncnt) == (len(AS), len(AC))
        assert (self.ldn, self.Mp, self.nsp) == ((n + 31) // 32 * 32, (max(M, 1) + 15) // 16 * 16, (max(ns, 1) + 15) // 16 * 16)
        nv = len(util.AS_VECTORS)
        self.off = {nm: int(o) for nm, o in zip(util.AS_VECTORS, out[9:9 + nv])}
        self.ioff = {nm: int(o) for nm, o in zip(util.AS_IVECTORS, out[9 + nv:])}


class Run:
    """One call of the hook on the state `st`; `extra`: doubles of the caller's behind the block."""

    def __init__(self, lib, h, st, stages, extra=None, Ah=None, refuse=False):
        n, M, ns = st["n"], st["M"], st["ns"]
        self.st, self.lay = st, Layout(lib, h, n, M, ns)
        lay = self.lay
        ne = 0 if extra is None else len(extra)
        blk = np.full(lay.ndbl + ne, util.SENTINEL)
        for nm in util.AS_VECTORS:
            blk[lay.off[nm]:lay.off[nm] + len(st[nm])] = st[nm]
        blk[lay.scal:lay.scal + len(AS)] = st["scal"]
        if ne:
            blk[lay.ndbl:] = extra
        ib = np.full(lay.nint, util.ISENT, np.int32)
        for nm in util.AS_IVECTORS:
            ib[lay.ioff[nm]:lay.ioff[nm] + len(st[nm])] = st[nm]
        ib[lay.ioff["rperm"] + M:lay.ioff["rperm"] + lay.Mp] = 0
        ib[lay.cnt:lay.cnt + len(AC)] = st["cnt"]
        self.inp, self.iinp = blk.copy(), ib.copy()
        arr = (_lib.AsStage * max(len(stages), 1))(*stages)
        grid = np.zeros(max(len(stages), 1), np.uint32)
        ahp, ahr = (None, 0) if Ah is None else (_lib.dptr(Ah), Ah.shape[0])
        rc = lib.asm_test_as_stages(h, n, M, ns, st["scale_q"], _lib.i64ptr(np.zeros(200, np.int64)), _lib.dptr(blk), len(blk), _lib.i32ptr(ib), len(ib), ahp, ahr,
                                    arr, len(stages), grid.ctypes.data_as(C.POINTER(C.c_uint32)))
        self.rc, self.out, self.iout = rc, blk, ib
        assert rc == 0 or refuse, lib.asm_last_error(h)
        self.grid = [int(g) for g in grid[:len(stages)]]

    def state(self):
        """The state as the call left it."""
        s2 = dict(self.st)
        for nm in util.AS_VECTORS + util.AS_IVECTORS:
            s2[nm] = self.v(nm).copy()
        s2["cnt"] = self.iout[self.lay.cnt:self.lay.cnt + len(AC)].copy()
        s2["scal"] = self.out[self.lay.scal:self.lay.scal + len(AS)].copy()
        return s2

    def v(self, nm, cnt=None):
        if nm in self.lay.ioff:
            o = self.lay.ioff[nm]
            return self.iout[o:o + (len(self.st[nm]) if cnt is None else cnt)]
        o = self.lay.off[nm]
        return self.out[o:o + (len(self.st[nm]) if cnt is None else cnt)]

    def check(self, tw, tag, extra_own=()):
        """(a), (b) and (c) for one kernel's twin result."""
        ex, bnd = tw[0], tw[1]
        lay = self.lay
        down = np.zeros(len(self.out), bool)
        iown = np.zeros(len(self.iout), bool)
        bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.int64)
        for nm, want in ex.items():
            if nm.startswith("cnt."):
                o = lay.cnt + AC[nm[4:]]
                assert self.iout[o] == want, (tag, nm, int(self.iout[o]), want)
                iown[o] = True
            elif nm.startswith("scal."):
                o = lay.scal + AS[nm[5:]]
                assert bits(self.out[o:o + 1])[0] == bits(np.array([want]))[0], (tag, nm, self.out[o], want)
                down[o] = True
            elif nm in lay.ioff:
                o = lay.ioff[nm]
                got = self.iout[o:o + len(want)]
                assert np.array_equal(got, want), (tag, nm, np.nonzero(got != want)[0][:8])
                iown[o:o + len(want)] = True
            else:
                o = lay.off[nm]
                got = self.out[o:o + len(want)]
                assert np.array_equal(bits(got), bits(want)), (tag, nm, np.nonzero(bits(got) != bits(want))[0][:8])
                down[o:o + len(want)] = True
        for nm, b in bnd.items():
            val, mag, k = b[:3]
            if nm.startswith("scal."):
                o = lay.scal + AS[nm[5:]]
                got = self.out[o:o + 1]
                down[o] = True
            else:
                o = lay.off[nm]
                val = np.atleast_1d(val)
                got = self.out[o:o + len(val)]
                own = np.ones(len(val), bool) if len(b) < 4 else b[3]
                down[o:o + len(val)] |= own
                got, val, mag = got[own], val[own], np.atleast_1d(mag)[own]
                k = k[own] if isinstance(k, np.ndarray) else k
            r = util.bound_ratio(got, val, mag, k)
            WORST[tag] = max(WORST.get(tag, 0.0), r)
            assert r <= 1.0, (tag, nm, r)
        for o, c in extra_own:
            down[o:o + c] = True
        assert np.array_equal(bits(self.out)[~down], bits(self.inp)[~down]), (tag, "a double the kernel does not own changed", np.nonzero(bits(self.out) != bits(self.inp))[0][:8])
        assert np.array_equal(self.iout[~iown], self.iinp[~iown]), (tag, "an int the kernel does not own changed", np.nonzero((self.iout != self.iinp) & ~iown)[0][:8])


def after(st, run, names):
    """The state with the named vectors / counters as the device left them."""
    s2 = dict(st)
    for nm in names:
        if nm == "cnt":
            s2["cnt"] = run.iout[run.lay.cnt:run.lay.cnt + len(AC)].copy()
        else:
            s2[nm] = run.v(nm).copy()
    return s2


@pytest.mark.parametrize("case,rp", CASES, ids=CASE_IDS)
def test_kernels_one_launch_each(hip_lib, handle, case, rp):
    n, M, ns = case
    st = util.as_state(100 + n % 97 + rp, n, M, ns)
    bk = util.AsBook()
    L = Layout(hip_lib, handle, n, M, ns)
    off = L.off
    gA, gM1, gN = util.as_grid_all(n, M, ns), (M + 255) // 256 + 1, (n + 255) // 256
    go = lambda stages, **kw: Run(hip_lib, handle, st, stages, **kw)
    # identify
    r = go([stage("identify", set=[3])]); r.check(util.tw_as_identify(st, 3, bk), "identify"); assert r.grid == [gA]
    # clip0, null and given source
    r = go([stage("clip0", x=[-1, off["zero"]])]); r.check(util.tw_as_clip0(st, None, "zero", bk), "clip0"); assert r.grid == [gN]
    r = go([stage("clip0", x=[off["ip.p"], off["pref"]])]); r.check(util.tw_as_clip0(st, "ip.p", "pref", bk), "clip0")
    r = go([stage("sl")]); r.check(util.tw_as_sl(st), "sl"); assert r.grid == [gM1]
    r = go([stage("sl_values")]); r.check(util.tw_as_sl(st, True), "sl_values"); assert r.grid == [gM1]
    r = go([stage("smax", x=[off["ip.s"], off["s"]])]); r.check(util.tw_as_smax(st, "ip.s", "s"), "smax"); assert r.grid == [(ns + 255) // 256]
    # setup: owns the padding of Fmask, p, pB, pF up to ldn and of Hmask up to Mp
    for cur, pref in ((0, None), (4, "pref")):
        r = go([stage("setup", set=[cur], rperm=rp, x=[-1 if pref is None else off[pref]])])
        r.check(util.tw_as_setup(st, cur, pref, rp, bk, L.ldn, L.Mp), "setup"); assert r.grid == [1]
        r2 = go([stage("setup", set=[cur], rperm=rp, x=[-1 if pref is None else off[pref]])])
        assert np.array_equal(r.out.view(np.int64), r2.out.view(np.int64)) and np.array_equal(r.iout, r2.iout)
    nH = int(st["cnt"][AC["NH"]])
    for yref in (None, "ip.y"):
        r = go([stage("rhs", x=[-1 if yref is None else off[yref]])]); r.check(util.tw_as_rhs(st, yref, bk), "rhs"); assert r.grid == [gA]
    gH = (nH + 255) // 256
    r = go([stage("res_p", k=nH)]); r.check(util.tw_as_res_p(st), "res_p"); assert r.grid == [gH]
    r = go([stage("gather_h", k=nH)]); r.check(util.tw_as_gather_h(st), "gather_h"); assert r.grid == [gH]
    r = go([stage("add_yh", k=nH)]); r.check(util.tw_as_add_yh(st), "add_yh"); assert r.grid == [gH]
    for src, acc in (("u", 1), ("yH", 0), ("uacc", 0)):
        r = go([stage("scatter_h", x=[off[src]], accumulate=acc)]); r.check(util.tw_as_scatter_h(st, src, acc, bk), "scatter_h"); assert r.grid == [gM1]
    r = go([stage("add_f")]); r.check(util.tw_as_add_f(st), "add_f"); assert r.grid == [gN]
    r = go([stage("rd")]); r.check(util.tw_as_rd(st), "rd"); assert r.grid == [gN]
    for wy in (0, 1):
        r = go([stage("merge", with_y=wy)]); r.check(util.tw_as_merge(st, wy, bk), "merge"); assert r.grid == [gA]
    # finish: AC_NDIFF == -1 without prev; the other counters and scalars keep their pre-fill
    for hp in (0, 1):
        stg = [stage("finish", set=[0, 1, 2], have_prev=hp, tol_p=util.TOL_P, tol_d=util.TOL_D)]
        r = go(stg); r.check(util.tw_as_finish(st, 0, 1, 2, hp, util.TOL_P, util.TOL_D, bk), "finish"); assert r.grid == [1]
        r2 = go(stg)
        assert np.array_equal(r.out.view(np.int64), r2.out.view(np.int64)) and np.array_equal(r.iout, r2.iout)
    for co in (0, 1):
        stg = [stage("primal_finish", set=[4, 3], tol_p=util.TOL_P, tol_m=util.FACE_TOL_M, check_only=co)]
        r = go(stg); r.check(util.tw_face_primal_finish(st, 4, 3, util.TOL_P, util.FACE_TOL_M, co, bk), "primal_finish"); assert r.grid == [1]
        r2 = go(stg)
        assert np.array_equal(r.out.view(np.int64), r2.out.view(np.int64)) and np.array_equal(r.iout, r2.iout)
    # the release arm needs a feasible point: the same state with every violation taken away
    sf = dict(st)
    sf["p"] = np.clip(st["p"], st["lb"], st["ub"])
    sf["t"] = st["r"] + st["rtype"] * 0.5 - st["sl"]
    sf["S4.sst"] = np.zeros(ns, np.int32)
    sf["ksoft"] = np.full(M, -1, np.int32)
    stg = [stage("primal_finish", set=[4, 3], tol_p=util.TOL_P, tol_m=util.FACE_TOL_M)]
    r = Run(hip_lib, handle, sf, stg); r.check(util.tw_face_primal_finish(sf, 4, 3, util.TOL_P, util.FACE_TOL_M, 0, bk), "primal_finish")
    stg = [stage("dual_finish", set=[5], tol_m=util.FACE_TOL_M)]
    r = go(stg); r.check(util.tw_face_dual_finish(st, 5, util.FACE_TOL_M, bk), "dual_finish"); assert r.grid == [1]
    r2 = go(stg)
    assert np.array_equal(r.out.view(np.int64), r2.out.view(np.int64)) and np.array_equal(r.iout, r2.iout)
    r = go([stage("kkt", set=[5])]); r.check(util.tw_face_kkt(st, 5, bk), "kkt"); assert r.grid == [1]
    # ns_step: the ratio test is exact given the activities and slack values the device wrote
    for s_ in (st, sf):
        stg = [stage("ns_step", set=[4], tol_p=util.TOL_P, x=[off["pa"], off["sa"], off["acta"]])]
        r = Run(hip_lib, handle, s_, stg)
        ex, bnd, info = util.tw_face_ns_step(s_, 4, util.TOL_P, bk, dev=(r.v("act").copy(), r.v("s").copy()))
        r.check((ex, bnd), "ns_step"); assert r.grid == [1]
        own = util.tw_face_ns_step(s_, 4, util.TOL_P, util.AsBook())[2]                # the decision from the twin's own float64 act / s: the same
        assert (own["nviol"], own.get("fam"), own.get("e")) == (info["nviol"], info.get("fam"), info.get("e"))
        if info["nviol"]:
            fam, e = int(r.iout[L.cnt + AC["NCHG"]]), int(r.iout[L.cnt + AC["NDIFF"]])
            idx, ratios = info["cand"][fam]
            assert 0 <= e < (M, ns, n, n)[fam] and e in idx and ratios[list(idx).index(e)] == info["alpha"]
        r2 = Run(hip_lib, handle, s_, stg)
        assert np.array_equal(r.out.view(np.int64), r2.out.view(np.int64)) and np.array_equal(r.iout, r2.iout)
    # ns_combine, ns_z, ns_unmark, ns_col
    rng = np.random.default_rng(n + M)
    for k in (0, 3):
        Z = np.full((max(k, 1), L.ldn), util.SENTINEL); Z[:, :n] = rng.standard_normal((max(k, 1), n))
        u = rng.standard_normal(max(k, 1))
        r = go([stage("ns_combine", k=k, x=[off["pf"], L.ndbl, L.ndbl + Z.size, off["p"]])], extra=np.concatenate([Z.ravel(), u]))
        r.check(({}, {"p": util.tw_face_ns_combine(st["pf"], Z[:k, :n], u[:k])}), "ns_combine"); assert r.grid == [gN]
    tz = util.tw_face_ns_z(st)
    r = go([stage("ns_z", x=[off["zf"]])]); r.check(({}, {"zf": tz[1]["z"]}), "ns_z"); assert r.grid == [gN]
    for fam, e in ((0, M - 1), (1, ns - 1), (2, n - 1), (3, 0)):
        if e < 0:
            continue
        r = go([stage("ns_unmark", set=[4], fam=fam, e=e)]); r.check(util.tw_face_ns_unmark(st, 4, fam, e, bk), "ns_unmark"); assert r.grid == [1]
        if M > 0:
            # the kernel reads one row of the matrix: the others stay zero pages
            Ah = np.zeros((M, L.ldn))
            arow = rng.standard_normal(n)
            row = util.as_col_row(st, fam, e)
            if row >= 0:
                Ah[row, :n] = arow
                Ah[row, n:] = util.SENTINEL
            stg = [stage("ns_col", fam=fam, e=e, x=[off["pf"], off["actf"]])]
            r = go(stg, Ah=Ah); r.check(util.tw_face_ns_col(st, arow, fam, e, "pf", "actf", bk), "ns_col"); assert r.grid == [1]
            r2 = go(stg, Ah=Ah)
            assert np.array_equal(r.out.view(np.int64), r2.out.view(np.int64))
    # pack: doubles, then int32 behind them
    nd = 2 * n + 2 * M + ns
    ni = M + n + ns
    r = go([stage("pack", set=[2], x=[L.ndbl])], extra=np.full(nd + (ni + 1) // 2 + 2, util.SENTINEL)); assert r.grid == [gA]
    d, i = util.tw_as_pack(st, 2)
    assert np.array_equal(r.out[L.ndbl:L.ndbl + nd].view(np.int64), d.view(np.int64))
    assert np.array_equal(r.out[L.ndbl + nd:].view(np.int32)[:ni], i)
    assert np.array_equal(r.out[L.ndbl + nd:].view(np.int32)[ni:], r.inp[L.ndbl + nd:].view(np.int32)[ni:])          # behind the last integer: untouched
    assert np.array_equal(r.out[:L.ndbl].view(np.int64), r.inp[:L.ndbl].view(np.int64)) and np.array_equal(r.iout, r.iinp)
    r = go([stage("copy_sets", set=[1, 5])]); r.check(util.tw_as_copy_sets(st, 1, 5), "copy_sets"); assert r.grid == [gA]


@pytest.mark.parametrize("nH", [0, 1, 256, 257, 512])
def test_device_count_grids(hip_lib, handle, nH):
    """(d) the grids sized from the host's copy of the device count: none at nH = 0 (nothing is launched, nothing changes), one up to 256."""
    st = util.as_state(3, 700, 600, 100)
    st["cnt"][AC["NH"]] = nH
    st["Hidx"][:nH] = np.arange(nH)
    bk = util.AsBook()
    for kind, tw in (("res_p", util.tw_as_res_p), ("gather_h", util.tw_as_gather_h), ("add_yh", util.tw_as_add_yh)):
        r = Run(hip_lib, handle, st, [stage(kind, k=nH)])
        assert r.grid == [(nH + 255) // 256]
        r.check(tw(st), kind)
    r = Run(hip_lib, handle, st, [stage("rhs", x=[-1])]); r.check(util.tw_as_rhs(st, None, bk), "rhs")


TIES = [(k, w) for k, ws in util.AS_TIES.items() for w in ws]


@pytest.mark.parametrize("kernel,which", TIES, ids=["%s-%s" % t for t in TIES])
def test_planted_ties(hip_lib, handle, kernel, which):
    """(e) a quantity exactly on its threshold: the device decides as the comparison operator dictates (the twin compares exactly)."""
    st, planted = util.as_tie_state(kernel, which)
    bk = util.AsBook()
    tp, td, tm = util.TIE_TOL_P, util.TIE_TOL_D, util.TIE_TOL_M
    L = Layout(hip_lib, handle, st["n"], st["M"], st["ns"])
    if kernel == "identify":
        r = Run(hip_lib, handle, st, [stage("identify", set=[3])]); r.check(util.tw_as_identify(st, 3, bk), kernel)
    elif kernel == "finish":
        r = Run(hip_lib, handle, st, [stage("finish", set=[0, 1, 2], have_prev=1, tol_p=tp, tol_d=td)]); r.check(util.tw_as_finish(st, 0, 1, 2, 1, tp, td, bk), kernel)
    elif kernel == "dual_finish":
        r = Run(hip_lib, handle, st, [stage("dual_finish", set=[5], tol_m=tm)]); r.check(util.tw_face_dual_finish(st, 5, tm, bk), kernel)
    elif kernel == "primal_finish":
        if which.startswith("rel"):
            st["p"] = np.where(st["S4.bst"] == 0, np.clip(st["p"], st["lb"], st["ub"]), st["p"])
            st["t"] = st["r"] + st["rtype"] * 0.5 - st["sl"]
            st["S4.sst"][:] = 0
            st["ksoft"][:] = -1
        r = Run(hip_lib, handle, st, [stage("primal_finish", set=[4, 3], tol_p=tp, tol_m=tm)]); r.check(util.tw_face_primal_finish(st, 4, 3, tp, tm, 0, bk), kernel)
    else:
        r = Run(hip_lib, handle, st, [stage("ns_step", set=[4], tol_p=tp, x=[L.off["pa"], L.off["sa"], L.off["acta"]])])
        ex, bnd, info = util.tw_face_ns_step(st, 4, tp, bk, dev=(r.v("act").copy(), r.v("s").copy()))
        r.check((ex, bnd), kernel)
    assert len(planted) > 0 and (kernel == "ns_step" or bk.cls["tie"] >= len(planted)) and bk.cls["between"] == 0


PAIRS = [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3], [0], [1], [2], [3], [3, 2, 1, 0]]


@pytest.mark.parametrize("fams", PAIRS, ids=["fam" + "".join(map(str, f)) for f in PAIRS])
@pytest.mark.parametrize("spots", [(0, 2099), (63, 64), (1023, 1024), (1500, 70)], ids=["ends", "wavefront", "sweep", "reversed"])
def test_ns_step_equal_ratios(hip_lib, handle, fams, spots):
    """(e) exactly equal minimal ratios across families and within a family: rows < slacks < lower < upper, then the lowest index; decoys with a
    smaller ratio that are ineligible are ignored."""
    st, planted = util.as_ratio_tie_state(fams, spots)
    bk = util.AsBook()
    L = Layout(hip_lib, handle, st["n"], st["M"], st["ns"])
    r = Run(hip_lib, handle, st, [stage("ns_step", set=[4], tol_p=util.TIE_TOL_P, x=[L.off["pa"], L.off["sa"], L.off["acta"]])])
    ex, bnd, info = util.tw_face_ns_step(st, 4, util.TIE_TOL_P, bk, dev=(r.v("act").copy(), r.v("s").copy()))
    want = min(planted)
    assert info["nviol"] == len(planted) and info["alpha"] == 0.25 and (info["fam"], info["e"]) == want
    r.check((ex, bnd), "ns_step")
    assert (int(r.iout[L.cnt + AC["NCHG"]]), int(r.iout[L.cnt + AC["NDIFF"]])) == want


def test_hook_refuses_out_of_range(hip_lib, handle):
    """Indices and offsets outside the blocks return ASM_ERR_ARG before anything is launched."""
    st = util.as_state(1, 100, 90, 40)
    L = Layout(hip_lib, handle, 100, 90, 40)

    def rc(stages, mod=None):
        s2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
        if mod:
            mod(s2)
        r = Run(hip_lib, handle, s2, stages, refuse=True)
        if r.rc != 0:                                   # refused with ASM_ERR_ARG, nothing launched: both blocks come back as they went in
            assert r.rc == -1, r.rc
            assert np.array_equal(r.out.view(np.int64), r.inp.view(np.int64)) and np.array_equal(r.iout, r.iinp)
            return 1
        return 0
    assert rc([stage("identify", set=[3])]) == 0
    assert rc([stage("identify", set=[6])]) == 1
    assert rc([stage("clip0", x=[-1, L.ndbl - 50])]) == 1
    assert rc([stage("ns_unmark", set=[4], fam=1, e=40)]) == 1
    assert rc([stage("ns_unmark", set=[4], fam=4, e=0)]) == 1
    assert rc([stage("res_p", k=91)]) == 1
    assert rc([stage("merge", with_y=1)], lambda s: s["hpos"].__setitem__(3, 4000)) == 1
    assert rc([stage("rhs", x=[-1])], lambda s: s["Hidx"].__setitem__(0, 90)) == 1
    assert rc([stage("finish", set=[0, 1, 2], tol_p=1e-9, tol_d=1e-6)], lambda s: s["ksoft"].__setitem__(0, 40)) == 1
    assert rc([stage("sl")], lambda s: s["srow"].__setitem__(0, 90)) == 1
    assert rc([stage("sl")], lambda s: s["rs1"].__setitem__(0, 40)) == 1
    assert rc([stage("sl")], lambda s: s["rperm"].__setitem__(0, -1)) == 1
    assert rc([stage("ns_step", set=[4], tol_p=1e-9, x=[L.off["pa"], L.off["sa"], L.ndbl - 10])]) == 1
    assert rc([stage("ns_col", fam=0, e=0, x=[L.off["pf"], L.off["actf"]])]) == 1          # no matrix given


def test_ns_step_without_a_ratio(hip_lib, handle):
    """A violated inequality whose ratio is not a number (an infinite anchor margin: inf / inf) is counted, but no entry reproduces the step: the
    kernel marks nothing, moves nothing and reports NCHG = NDIFF = -1.  (A NaN anchor is no such case: fmax drops it and the ratio is 0.)"""
    st, planted = util.as_ratio_tie_state([0], (70,), decoys=False)
    (fam, i), = planted
    assert st["rtype"][i] == 1
    st["acta"][i] = np.inf
    L = Layout(hip_lib, handle, st["n"], st["M"], st["ns"])
    r = Run(hip_lib, handle, st, [stage("ns_step", set=[4], tol_p=util.TIE_TOL_P, x=[L.off["pa"], L.off["sa"], L.off["acta"]])])
    ex, bnd, info = util.tw_face_ns_step(dict(st, acta=np.where(np.isfinite(st["acta"]), st["acta"], 2.0)), 4, util.TIE_TOL_P, util.AsBook())
    assert info["nviol"] == 1
    keep = {"ksoft": ex["ksoft"], "cnt.NVIOL": 1, "cnt.NCHG": -1, "cnt.NDIFF": -1, "scal.HARDRES": ex["scal.HARDRES"]}
    r.check((keep, {"act": bnd["act"], "s": bnd["s"]}), "ns_step")          # sets and anchors: not owned, so bit for bit what went in


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("seed", [3, 4])
def test_chained_round(hip_lib, handle, mode, seed):
    """(f) setup -> rhs -> sweeps -> merge -> tail with the kernels in place of the twins (products and H-solves by the test, in long double),
    against oracle.eqp + kkt_measures + correct on the same working set."""
    from oracle import lp_solver as O
    st0, A = util.as_chain_lp(seed)
    L = Layout(hip_lib, handle, st0["n"], st0["M"], st0["ns"])
    p_ref, y_ref = ("pref", "ip.y") if mode == 0 else (None, None)

    def do(st, kind, **kw):
        x = {"setup": [-1 if kw.get("p_ref") is None else L.off[kw.get("p_ref")]], "rhs": [-1 if kw.get("y_ref") is None else L.off[kw.get("y_ref")]],
             "scatter_h": [L.off.get(kw.get("src"), 0)]}.get(kind, [])
        a = {k: v for k, v in kw.items() if k in ("k", "accumulate", "with_y")}
        return Run(hip_lib, handle, st, [stage(kind, set=[kw.get("cur", 0)], x=x, **a)]).state()
    fin = util.as_chain(st0, A, 0, mode, p_ref, y_ref, do)
    ref = util.as_chain(st0, A, 0, mode, p_ref, y_ref, util.as_twin_do(util.AsBook()))
    err, lp, sets = util.as_chain_errors(st0, A, fin, mode, p_ref, y_ref)
    print("chained round mode %d seed %d: " % (mode, seed) + ", ".join("%s error %.2e, oracle against itself %.2e" % (k, e[0], e[1]) for k, e in err.items()))
    assert all(e[2] <= 1.0 for e in err.values()), err
    for nm in ("Hidx", "hpos", "Fidx", "fpos", "ksoft", "cnt"):
        assert np.array_equal(fin[nm], ref[nm]), nm
    if mode != 1:
        bk = util.AsBook()
        r = Run(hip_lib, handle, fin, [stage("finish", set=[0, 1, 2], have_prev=0, tol_p=util.TOL_P, tol_d=util.TOL_D)])
        r.check(util.tw_as_finish(fin, 0, 1, 2, 0, util.TOL_P, util.TOL_D, bk), "finish")
        out = r.state()
        (nrow, nb, nss), nchg = O.correct(lp, fin["p"], out["s"], fin["y"], sets)
        assert np.array_equal(nrow, out["S1.rowst"]) and np.array_equal(nb, out["S1.bst"]) and np.array_equal(nss, out["S1.sst"]) and nchg == out["cnt"][AC["NCHG"]]
        assert bk.cls["between"] == 0
