"""The null-space set-up with its factor-independent part on the side stream beside the factorisation of a banded S0 (ASM_NS_S0SIDE, Solver::
ns_factor_S0): k_ns_rows_e for the previous basis, the wide-block inverses block by block, (level 2) the forward half of the block substitution
one wide block behind the panel launches, the transposed copy of the factor.  Only the stream and the time of issue of existing launches change,
so every value must equal the ASM_NS_S0SIDE=0 handle's bit for bit.

The shape: util.banded_subproblem(506, 1500, 1950, 1200, 0) - 1 200 equality rows, measured on the device operand: band 23 of S0 in the
reverse Cuthill-McKee order, k = 300 (no dropped pivot), M = 1950, pitch nEp = 1216, so ns_alloc_factor picks wb = 512 and the factor has three
wide blocks [0,512), [512,1024), [1024,1200) - the last one short - made by the panel launches [0,512), [512,1024), [1024,1200) of the
band-panel path.  n - nE = 300 <= 0.3 M = 585: the form qualifies.  The seed is
one for which the oracle's NullSpace, util.nss_chain and the library's own cold selection all find a basis, also with the duplicated row
(the selection is threshold-bound on this generator: seeds 504 and 505 end without the form in one of the three).

What shows that the side sequence ran at all: with a carried basis of Zk rows and an LP whose k is smaller, rows k .. Zk-1 of R (levels 1, 2)
and of X (level 2) are written by the speculative launches and by nothing else - level 0 leaves the pre-fill there
(test_speculation_undone_by_fixed_columns).  That is the eligibility check of this file: the library's own rule (Dev::band_panels_ok) is observed,
not restated.  End to end (test_two_solves_on_one_skeleton_do_not_depend_on_the_knob): ONE asm_sublp_setup, then two solves - the second one's
set-up finds the first one's basis (asm_solve_stats.ns_path 1), which is the flagship's steady state at case1354pegase's size: wb = 1024, eleven
wide blocks, an event every second panel launch, the speculative rows used."""
import ctypes as C

import numpy as np
import pytest

from activesetmethods_amd import acopf
from tests import util
from tests.test_ns_setup_gpu import SENT, Case, quality, setup_result, stage      # the hook's driver and the reference's measures, as that file has them

pytestmark = pytest.mark.gpu

LEVELS = (0, 1, 2)
SHAPE = (506, 1500, 1950, 1200, 0)
CHOL_NBI = 512
ERR_STATE = -3


def _p(a, typ=C.c_double):
    return None if a is None else a.ctypes.data_as(C.POINTER(typ))


def create(lib, level):
    """A handle made with ASM_NS_S0SIDE=level in the environment (the knobs are read at asm_create)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("ASM_NS_S0SIDE", str(level))
        return util.abi_create(lib)


class Shape(Case):
    """tests.test_ns_setup_gpu.Case for a sub-problem of this file, on a handle of one knob level; the reference set-up comes from `first`
    (the same operand) when given."""

    def __init__(self, lib, level, sp, fm, name, first=None):
        self.lib, self.name, self.level = lib, name, level
        self.sp, self.fm = sp, fm
        self.dE = np.ascontiguousarray(sp["dE"], np.float64)
        self.h = create(lib, level)
        assert util.abi_setup(lib, self.h, sp) == 0, lib.asm_last_error(self.h)
        info = np.zeros(12, np.int64)
        assert lib.asm_test_build_dispatch(self.h, _p(self.dE), -1, None, 0, None, None, None, None, _p(info, C.c_int64), None, None, None) == 0
        self.M, self.n, nE = int(info[0]), sp["n"], int(info[5])
        assert info[1] == self.n and nE >= 64, "the case has no null-space form"
        lay, idx = np.zeros(16, np.int64), np.zeros(self.M, np.int32)
        assert self._call(1, 1, None, lay, idx, None, {}, 0, None, None) == 0, lib.asm_last_error(self.h)
        self.idx = idx
        if first is None:
            self.op = self.operand(self.dE)
            self.ref = util.nss_chain(self.op, np.float64, M=self.M)
            assert self.ref["path"] == "cold"
        else:
            assert np.array_equal(idx, first.idx)
            self.op, self.ref = first.op, first.ref
        self.k, self.J = self.ref["k"], self.ref["J"].astype(np.int32)
        self.kres = self.k
        self.lay = self.layout(self.k, self.kres)

    def operand(self, dE):
        """The device operand (assembled and scaled by the library) for the Jacobian values dE, with the case's lists and mask."""
        from activesetmethods_amd import _lib
        dE = np.ascontiguousarray(dE, np.float64)
        info, Ah = np.zeros(12, np.int64), np.zeros((self.M, self.n))
        assert self.lib.asm_test_build_dispatch(self.h, _p(dE), -1, None, 0, None, None, None, Ah.ctypes.data_as(_lib._D), _p(info, C.c_int64), None, None, None) == 0
        nE = int(info[5])
        return util.NssOp(Ah, self.idx[:nE], self.idx[nE:self.M], self.fm)


def warm_rows(c, Zt):
    """Rows to load as the previous LP's basis: Zt (k x n) in the first columns, zeros to the pitch, under SENTINEL rows."""
    G = np.full((c.lay.cap, c.lay.ldg), SENT)
    G[:Zt.shape[0]] = 0.0
    G[:Zt.shape[0], :c.n] = Zt
    return G


def equal_runs(a, b, k, what, rows_rx=None):
    """Two returned set-ups are the same bits: the basis (whole buffer), the factor of S0 and its transposed copy, path / k / dropped / columns,
    and the right-hand-side blocks (rows_rx: only their first rows - beyond them level 0 and the speculative launches differ by design)."""
    assert np.array_equal(a.setup, b.setup), what
    for nm in ("G", "f0", "Lt"):
        assert np.array_equal(getattr(a, nm), getattr(b, nm)), (what, nm)
    for nm in ("R", "X"):
        assert np.array_equal(getattr(a, nm)[:rows_rx], getattr(b, nm)[:rows_rx]), (what, nm)


@pytest.fixture(scope="module")
def shapes(hip_lib):
    """One handle per knob level on the three-block shape, the loaded basis (the float64 reference basis of a slightly perturbed operand) and the
    reference set-up from it."""
    sp = util.banded_subproblem(*SHAPE)
    fm = np.ones(sp["n"])
    made = []
    try:
        for lv in LEVELS:
            made.append(Shape(hip_lib, lv, sp, fm, "three-blocks", made[0] if made else None))
        c = made[0]
        L = c.lay
        # the layout the side sequence needs: banded, wb = 512 for S0 (ns_alloc_factor: pitch in (1024, 1536]), three wide blocks, more than one
        # panel launch.  Whether the library then takes the sequence (Dev::band_panels_ok is its own rule) is not re-derived here: it is
        # OBSERVED by test_speculation_undone_by_fixed_columns, through the rows only the speculative launches write
        assert L.band > 0 and util.nss_wb(L.ld0) == 512 and L.nE > 2 * 512 and L.nE > CHOL_NBI + 128
        print("three-blocks: band %d, k %d, dropped %d, nEp %d, M %d" % (L.band, c.k, c.ref["dropped"], L.nEp, c.M))
        assert L.band <= 64 and (c.k, c.ref["dropped"], L.nEp) == (300, 0, 1216) and 100 <= c.k <= 400
        assert c.n - L.nE <= 0.3 * c.M
        dE2 = c.dE * (1.0 + 1e-3 * np.random.default_rng(7).standard_normal(c.dE.shape))
        pert = util.nss_chain(c.operand(dE2), np.float64, hint_J=c.J, M=c.M)
        assert pert["path"] in ("columns", "cold") and pert["k"] == c.k
        Gw = warm_rows(c, pert["Zt"])
        ref = util.nss_chain(c.op, np.float64, hint_J=c.J, warm_Z=Gw[:c.k, :c.n], M=c.M)
        assert ref["path"] == "basis"
        yield made, Gw, ref
    finally:
        for c in made:
            c.close()


@pytest.fixture(scope="module")
def warm_runs(shapes):
    """Stage `setup` with the loaded basis (Zk = k) on every level's handle, once."""
    made, Gw, ref = shapes
    return [c.run(["setup"], hint=c.J, G=Gw, Zk=c.k) for c in made]


def test_bit_for_bit_against_the_knob(shapes, warm_runs):
    made, Gw, ref = shapes
    k = made[0].k
    for r in warm_runs:
        assert setup_result(r)[:3] == (util.NSS_PATHS["basis"], k, 0) and r.res[0] == 1
    for lv, r in zip(LEVELS[1:], warm_runs[1:]):
        equal_runs(r, warm_runs[0], k, "level %d" % lv)      # (R and X whole: with Zk = k the speculative launches are the path's own)
    assert not np.array_equal(warm_runs[0].G[:k], Gw[:k])     # the projection did real work


def test_against_the_reference(shapes, warm_runs):
    made, Gw, ref = shapes
    c, r = made[2], warm_runs[2]
    k = c.k
    quality(c, r.G, ref, "level 2, set-up from the previous basis")
    for nm in ("G", "R", "X"):      # rows k .. cap - 1 are nobody's
        assert np.array_equal(getattr(r, nm)[k:], r.before[nm][k:]), nm
        assert np.all(getattr(r, nm)[k:] == SENT), nm
    assert not r.R[:k, c.lay.nE:].any()
    # the transposed copy made on the side stream, inside the band
    nE, band = c.lay.nE, c.lay.band
    i, j = np.indices((nE, nE))
    inb = (j <= i) & (i - j <= band)
    assert np.array_equal(r.Lt[:nE, :nE].T[inb], r.f0[:nE, :nE][inb])


def test_speculation_undone_by_fixed_columns(shapes):
    """Zk = k loaded, five of the retained columns fixed in this LP: k is five less, the carried basis is not tried."""
    made, Gw, ref = shapes
    k, J = made[0].k, made[0].J
    fm2 = made[0].fm.copy()
    fm2[J[::60]] = 0.0
    J2 = np.ascontiguousarray(J[fm2[J] > 0], np.int32)
    k2 = len(J2)
    assert k2 == k - 5
    runs = [c.run(["setup"], k=k2, hint=J2, G=Gw, Zk=k, fm=fm2) for c in made]
    path, kk, dropped, _ = setup_result(runs[0])
    assert path in (util.NSS_PATHS["columns"], util.NSS_PATHS["cold"]) and (kk, dropped) == (k2, 0)
    for lv, r in zip(LEVELS[1:], runs[1:]):
        equal_runs(r, runs[0], k2, "level %d" % lv, rows_rx=k2)
    # the speculative rows: written where the level sends them to the side stream, the pre-fill elsewhere
    nE = made[0].lay.nE
    assert np.all(runs[0].R[k2:] == SENT) and np.all(runs[0].X[k2:] == SENT)
    assert np.all(runs[1].R[k2:k, :nE] != SENT) and np.all(runs[1].X[k2:] == SENT)
    assert np.all(runs[2].R[k2:k, :nE] != SENT) and np.all(runs[2].X[k2:k, :nE] != SENT)
    for r in runs:
        assert np.all(r.R[k:] == SENT) and np.all(r.X[k:] == SENT) and np.all(r.G[k:] == SENT)


def test_speculation_undone_by_a_dropped_pivot(hip_lib, shapes):
    """The duplicated equality row of small-dep: one dropped pivot of S0, so k = Zk + 1."""
    made, Gw, ref = shapes
    sp = util.banded_subproblem(*SHAPE)
    eq = np.nonzero(sp["c_lb"] == sp["c_ub"])[0]
    a, b = int(eq[0]), int(eq[1])
    rows = np.asarray(sp["j_row"]) - 1
    ia, ib = np.nonzero(rows == a)[0], np.nonzero(rows == b)[0]
    assert len(ia) == len(ib) == 4      # (the generator deals per_row = 4 entries to every row)
    sp["j_col"], sp["dE"] = sp["j_col"].copy(), sp["dE"].copy()
    sp["j_col"][ib], sp["dE"][ib] = sp["j_col"][ia], 2.0 * sp["dE"][ia]
    sp["c_lb"], sp["c_ub"] = sp["c_lb"].copy(), sp["c_ub"].copy()
    sp["c_lb"][b] = sp["c_ub"][b] = 2.0 * sp["c_lb"][a]
    k = made[0].k
    dep = []
    try:
        for lv in LEVELS:
            dep.append(Shape(hip_lib, lv, sp, np.ones(sp["n"]), "three-blocks-dep", dep[0] if dep else None))
        c = dep[0]
        assert c.ref["dropped"] == 1 and c.k == k + 1 and c.lay.band > 0 and c.lay.nEp == 1216 and c.lay.cap == made[0].lay.cap
        runs = [d.run(["setup"], hint=c.J, G=Gw, Zk=k) for d in dep]
        path, kk, dropped, _ = setup_result(runs[0])
        assert path in (util.NSS_PATHS["columns"], util.NSS_PATHS["cold"]) and (kk, dropped) == (k + 1, 1)
        for lv, r in zip(LEVELS[1:], runs[1:]):
            equal_runs(r, runs[0], k + 1, "level %d" % lv)
    finally:
        for d in dep:
            d.close()


def test_reservation_outgrown_while_the_side_stream_has_work(shapes, warm_runs):
    """A reservation of 128 rows with 100 carried rows, an LP of k = 300: ns_reserve re-makes the k-sized buffers the side stream was given.  The
    hook reports the outgrown reservation as a state error; the handle then gives the same set-up as before."""
    made, Gw, ref = shapes
    c = made[2]
    cap1 = util.nss_kcap(1)
    assert 100 <= cap1 < c.k
    G1 = np.ascontiguousarray(Gw[:cap1]).copy()
    G1[100:] = SENT
    bufs = {"G": G1, "R": np.full((cap1, c.lay.nEp), SENT), "X": np.full((cap1, c.lay.nEp), SENT)}
    outs = {"grid": np.zeros(1, np.uint32), "res": np.zeros(1, np.int32), "setup": np.full(4 + c.n, -1, np.int32)}
    rc = c._call(1, 1, None, np.zeros(16, np.int64), None, [stage("setup")], bufs, 100, None, outs)
    assert rc == ERR_STATE and b"larger than k_reserve" in c.lib.asm_last_error(c.h), c.lib.asm_last_error(c.h)
    r = c.run(["setup"], hint=c.J, G=Gw, Zk=c.k)
    equal_runs(r, warm_runs[0], c.k, "after the outgrown reservation")


def test_three_set_ups_on_one_handle_are_identical(shapes, warm_runs):
    made, Gw, ref = shapes
    c = made[2]
    for _ in range(2):      # (warm_runs holds the first)
        equal_runs(c.run(["setup"], hint=c.J, G=Gw, Zk=c.k), warm_runs[2], c.k, "repeat")


def acopf_lp(name):
    """The first normal-phase LP of the synthetic grid `name` at load 0.5 (the LP of tests/test_ns_overlap_gpu.py)."""
    pr = acopf.acopf_problem(acopf.synthetic_case(name, 1, 0.5), name)
    x = np.asarray(pr.x0, float).copy()
    return dict(n=pr.n, m=pr.m, j_row=pr.j_row, j_col=pr.j_col, dE=pr.eval_jac_g(x, np.zeros(pr.nnz)), df=pr.eval_grad_f(x, np.zeros(pr.n)),
                f=pr.eval_f(x), E=pr.eval_g(x, np.zeros(pr.m)), x_k=x.copy(), c_lb=pr.g_L, c_ub=pr.g_U, v_lb=pr.x_L, v_ub=pr.x_U, delta=1000.0)


def two_solves(lib, level, sp):
    """ONE set-up and two solves of the LP on a handle of the knob level: [(raw outputs, statistics)] of both."""
    h = create(lib, level)
    try:
        assert util.abi_setup(lib, h, sp) == 0, lib.asm_last_error(h)
        res = []
        for _ in range(2):
            out, stt = util.abi_solve(lib, h, sp)
            assert out[0] == 1
            res.append((out, {nm: stt[nm] for nm in ("ipm_iters", "ns_iters", "path", "nfact", "ns_dim", "ns_cold", "ns_path")}))
        return res
    finally:
        lib.asm_destroy(h)


@pytest.mark.parametrize("name", ["three-blocks", "case1354pegase"])
def test_two_solves_on_one_skeleton_do_not_depend_on_the_knob(hip_lib, name):
    """asm_sublp_setup once, then the LP twice: the skeleton - the form, the k-sized buffers, Zk, the retained columns - lives on, so the second
    solve's set-up re-projects the first one's basis (ns_path 1) and, at levels 1 and 2, uses the rows the side stream made before k was known."""
    sp = util.banded_subproblem(*SHAPE) if name == "three-blocks" else acopf_lp(name)
    k = 300 if name == "three-blocks" else 519
    runs = [two_solves(hip_lib, lv, sp) for lv in LEVELS]
    first, second = runs[0][0][1], runs[0][1][1]
    assert first["ns_dim"] == k and first["ns_iters"] > 0 and first["ns_path"] == util.NSS_PATHS["cold"], first
    assert second["ns_dim"] == k and second["ns_path"] == util.NSS_PATHS["basis"], second      # (its warm attempt may spare the iterations)
    for run in runs[1:]:
        for (out, stt), (out0, stt0) in zip(run, runs[0]):
            assert stt == stt0, (stt, stt0)
            assert out == out0


@pytest.mark.parametrize("name", ["banded", "dense"])
def test_ineligible_shapes_keep_the_sequence(hip_lib, name):
    """One wide block (banded: nE = 300) and a dense S0: today's sequence whatever the knob - nothing speculative is written."""
    sp, fm, _ = util.nss_case(name)
    made = []
    try:
        for lv in LEVELS:
            made.append(Shape(hip_lib, lv, sp, fm, name, made[0] if made else None))
        c = made[0]
        assert (c.lay.band > 0) == (name == "banded") and c.lay.nE <= util.nss_wb(c.lay.ld0)
        k = c.k
        cold = c.run(["setup"])
        assert setup_result(cold)[:2] == (util.NSS_PATHS["cold"], k)
        Gw = np.full((c.lay.cap, c.lay.ldg), SENT)
        Gw[:k] = cold.G[:k] * (1.0 + 1e-3 * np.random.default_rng(3).standard_normal((k, c.lay.ldg)))
        runs = [d.run(["setup"], hint=c.J, G=Gw, Zk=k) for d in made]
        assert setup_result(runs[0])[:2] == (util.NSS_PATHS["basis"], k)
        for lv, r in zip(LEVELS[1:], runs[1:]):
            equal_runs(r, runs[0], k, "level %d" % lv)
        # a carried basis of another dimension: no level writes a speculative row
        Gw1 = Gw.copy()
        Gw1[k] = Gw[0]
        runs = [d.run(["setup"], hint=c.J, G=Gw1, Zk=k + 1) for d in made]
        for lv, r in zip(LEVELS, runs):
            assert setup_result(r)[0] == util.NSS_PATHS["columns"]
            assert np.all(r.R[k:] == SENT) and np.all(r.X[k:] == SENT), lv
            equal_runs(r, runs[0], k, "level %d" % lv)
    finally:
        for d in made:
            d.close()
