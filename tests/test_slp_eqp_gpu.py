"""SLP-EQP on the device (include/asm_hip.h, "SLP-EQP": asm_eqp_trial, asm_slp_run_eqp): the trial step against its parts - the working
set of eqp.lp_working_set, d = t dx from a separate asm_kkt_step call on that set, the merit values of asm_slp_merit, every skipped
code - on hs071 and on a small QP with a range row and bound variables; the native driver against SlpEQP on the HIP optimizer with
device_eval, bit for bit; convergence against asm_slp_run_tr on hs071 and the 14-bus ACOPF (n = 118, m = 189); enabled = 0; a
Trust-Region run on a handle that ran SLP-EQP before; argument and state errors."""
import ctypes as C

import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import _lib, eqp
from tests.test_kkt_step_cpu import hs071_start
from tests.test_nlparams_gpu import _handle_for
from tests.test_slp_eqp_cpu import HS071_X, grid14_function_model

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
INF = float("inf")
EQP, TR = "SLP-EQP", "Trust Region"
STEP_FIELDS = ("status", "cg_iters", "n_free", "n_rows", "dropped_pivots", "boundary", "res_stat", "res_feas", "theta", "norm_normal", "norm_step", "model")


def small_qp():
    """min 1/2 ||v - (-1, 2, 3, 5)||^2 over 0 <= v1 <= 10, v2 and v3 free, -1 <= v4 <= 1, with the rows
        r0: v2 + v3 == 4,   r1: 0 <= v2 - v3 + v4 <= 1 (a range row: adj = [1]),   r2: v2 - v3 + v4 <= 1 (the same function, one-sided)."""
    from activesetmethods_amd.moi_evaluator import FunctionModel
    from activesetmethods_amd.nlexpr import ExprBlock, variables
    v1, v2, v3, v4 = variables(4)
    fm = FunctionModel(4, np.array([0.0, -INF, -INF, -1.0]), np.array([10.0, INF, INF, 1.0]))
    fm.nlp = ExprBlock([(v2 + v3, 4.0, 4.0), (v2 - v3 + v4, 0.0, 1.0), (v2 - v3 + v4, -INF, 1.0)],
                       objective=0.5 * (v1 + 1.0) ** 2 + 0.5 * (v2 - 2.0) ** 2 + 0.5 * (v3 - 3.0) ** 2 + 0.5 * (v4 - 5.0) ** 2, n=4)
    return fm


def wide_qp_case():
    """n = 700, m = 300, so that both kernels run on three workgroups: min 1/2 ||v - c||^2 (in the function store) with 150 equalities
    v[2i] + v[2i+1] == 1 and 150 range rows 0 <= v[2i] - v[2i+1] <= 1 on the next 300 variables, 100 variables without rows, bounds
    [-2, 2]; a point with a third of the odd and of the rowless variables on a bound and LP states drawn at random (a range row or its twin, never both)."""
    from activesetmethods_amd.moi_evaluator import FunctionModel, ScalarFunction
    from activesetmethods_amd.nlexpr import ExprBlock, variables
    n, m = 700, 300
    rng = np.random.default_rng(5)
    c = rng.uniform(-3.0, 3.0, n)
    v = variables(n)
    fm = FunctionModel(n, np.full(n, -2.0), np.full(n, 2.0))
    fm.objective = ScalarFunction(0.0, [(-c[j], j + 1) for j in range(n)], [(1.0, j + 1, j + 1) for j in range(n)])
    fm.nlp = ExprBlock([(v[2 * i] + v[2 * i + 1], 1.0, 1.0) for i in range(150)] + [(v[2 * i] - v[2 * i + 1], 0.0, 1.0) for i in range(150, 300)], n=n)
    x = rng.uniform(-1.5, 1.5, n)
    side = np.where((np.arange(n) % 2 == 1) | (np.arange(n) >= 600), rng.integers(-1, 2, n), 0)      # every row keeps a free variable: independent rows
    x = np.where(side == -1, -2.0, np.where(side == 1, 2.0, x))
    lp_bnd = np.where(side != 0, side, np.where(rng.random(n) < 0.2, rng.integers(-1, 2, n), 0)).astype(np.int32)      # some stopped short of a bound
    which = rng.integers(0, 3, 150)                                                            # range rows: inactive, the row, its twin
    lp_rows = np.concatenate([rng.integers(0, 2, 150), which == 1, which == 2]).astype(np.int32)
    return fm, x, rng.uniform(-1.0, 1.0, m), lp_rows, lp_bnd, 30.0, rng.uniform(1.0, 2.0, m), 0


def trial_cases():
    """name -> (fm, x, lam, the LP's row_state [m + n_adj], its bound_state, radius, nu, the skipped code expected)."""
    fm, _, x, lam = hs071_start()
    qp = small_qp()
    one = np.ones(3)
    return {
        # hs071 near its solution: both rows active, x1 at its lower bound
        "hs071": (fm, x, lam, [1, 1], [-1, 0, 0, 0], 1.0, np.array([1.5, 0.7]), 0),
        # the same point with a small radius: the step ends on the boundary of its region
        "hs071 small radius": (fm, x, lam, [1, 1], [-1, 0, 0, 0], 1e-5, np.array([1.5, 0.7]), 0),
        # the equality alone although the LP calls it inactive; v1 at its lower and v4 at its upper bound in B
        "qp equality": (qp, np.array([0.0, 1.0, 3.0, 1.0]), np.array([0.1, 0.0, 0.0]), [0, 0, 0, 0], [-1, 0, 0, 1], 10.0, one, 0),
        # the range row at g_U through its twin; v4 held by the LP at -1 although x4 = 0: free; the step is cut at v4's upper bound
        "qp twin": (qp, np.array([0.0, 2.5, 1.5, 0.0]), np.array([0.1, -0.2, 0.0]), [1, 0, 0, 1], [-1, 0, 0, -1], 10.0, one, 0),
        # the range row at g_L
        "qp lower": (qp, np.array([2.0, 1.5, 2.5, 1.0]), np.array([0.0, 0.3, 0.0]), [1, 1, 0, 0], [0, 0, 0, 1], 0.5, one, 0),
        # every variable of hs071 at its lower bound: one working row, no free variable
        "rows exceed": (fm, np.ones(4), lam, [0, 0], [-1, -1, -1, -1], 1.0, np.array([1.5, 0.7]), 1),
        # the range row through its twin and its one-sided copy: dependent working rows
        "dependent": (qp, np.array([0.0, 2.5, 1.5, 0.0]), np.array([0.1, -0.2, 0.0]), [0, 0, 1, 1], [0, 0, 0, 0], 10.0, one, 2),
        # v1 sits on its lower bound, the LP calls it free and the step points outwards: t = 0
        "zero step": (qp, np.array([0.0, 1.5, 2.5, 0.5]), np.array([0.1, 0.0, 0.0]), [0, 0, 0, 0], [0, 0, 0, 0], 10.0, one, 3),
        "wide": wide_qp_case(),
    }


# ------------------------------------------------------------------------------------------------ 1. the trial step against its parts
@pytest.mark.parametrize("name", sorted(trial_cases()))
def test_trial_equals_its_parts(name):
    fm, x, lam, lp_rows, lp_bnd, radius, nu, skipped = trial_cases()[name]
    pr = fm.to_problem(name)
    lp_rows, lp_bnd = np.array(lp_rows, np.int32), np.array(lp_bnd, np.int32)
    opt = _handle_for(pr, fm)
    f, df, E = opt.eval_functions(x)
    d, lam_new, mU, mL, rs, bs, info = opt.eqp_trial(x, lam, lp_rows, lp_bnd, radius, nu)
    again = opt.eqp_trial(x, lam, lp_rows, lp_bnd, radius, nu)
    want_rs, want_bs, at = eqp.lp_working_set(pr, x, (lp_rows, lp_bnd), 1e-8)
    if name == "wide":                                     # every kind of row and variable occurs
        assert 150 < want_rs.sum() < 300 and len(set(at[150:][want_rs[150:] == 1])) == 2 and set(want_bs) == {-1, 0, 1} and (want_bs != lp_bnd).any()
    print("%s: W %r B %r skipped %d status %d boundary %d cg %d t %.17g ||d|| %.3e phi %.17g -> %.17g" %
          (name, rs.tolist()[:8], bs.tolist()[:8], info.skipped, info.status, info.boundary, info.cg_iters, info.t, info.norm_d, info.phi0, info.phi1))
    assert rs.tolist() == want_rs.tolist() and bs.tolist() == want_bs.tolist()
    assert info.skipped == skipped and (info.n_rows, info.n_free) == (int(want_rs.sum()), int((want_bs == 0).sum()))
    assert all(np.array_equal(a, b) for a, b in zip(again[:6], (d, lam_new, mU, mL, rs, bs)))
    assert all(getattr(again[6], k) == getattr(info, k) for k, _ in info._fields_)
    if skipped == 1:
        assert not d.any() and not lam_new.any() and not mU.any() and not mL.any() and info.t == 0.0
        opt.close()
        return
    rw = np.where(want_rs == 1, E - at, 0.0)
    dx, dlam, dz, step = opt.kkt_step(x, lam, want_rs, want_bs, df, rw, radius)
    assert all(getattr(info, k) == getattr(step, k) for k in STEP_FIELDS)
    if skipped == 2:
        assert step.status == 3 and not d.any() and not lam_new.any()
        opt.close()
        return
    t = eqp.fraction_to_box(dx, pr.x_L - x, pr.x_U - x)
    assert info.t == t and info.norm_d_inf == np.abs(t * dx).max()
    # (two sums of n squares in different orders: each within n eps of the exact sum, relative; the root halves it, t dx rounds once more)
    assert abs(info.norm_d - np.linalg.norm(t * dx)) <= pr.n * np.finfo(float).eps * np.linalg.norm(t * dx)
    if skipped == 3:
        assert t == 0.0 and not d.any() and not lam_new.any()
        opt.close()
        return
    assert np.array_equal(d, t * dx) and np.array_equal(lam_new, dlam)
    assert np.array_equal(mU, np.where(want_bs == 1, dz, 0.0)) and np.array_equal(mL, np.where(want_bs == -1, dz, 0.0))
    phi0 = opt.slp_merit(0, 0.0, d, nu, {}, False, 0.0)
    phi1 = opt.slp_merit(0, 1.0, d, nu, {}, False, 0.0)
    assert (info.phi0, info.phi1) == (phi0, phi1)
    slack = 4 * np.finfo(float).eps * (1.0 + np.abs(x + d))                 # (t dx reaches a bound to rounding)
    assert np.all(x + d >= pr.x_L - slack) and np.all(x + d <= pr.x_U + slack)
    if name == "hs071 small radius":
        assert info.boundary != 0 or info.theta < 1.0
    if name == "wide":
        assert 0.0 < t < 1.0 and info.boundary != 0
    if name == "qp twin":
        assert 0.0 < t < 1.0 and abs((x + d)[3] - 1.0) <= 4 * np.finfo(float).eps
    # nothing of the iterate was overwritten: the evaluator still holds x
    assert opt.slp_merit(0, 0.0, d, nu, {}, False, 0.0) == phi0
    opt.close()


# ------------------------------------------------------------------------------------------------ 2. the drivers
def _models():
    from activesetmethods_amd import acopf
    return {"hs071": (A.problems.hs071_function_model, {}), "grid14": (grid14_function_model, dict(max_iter=60)),
            # the same grid at three times the load: the first LP is infeasible, the run spends some ten LPs in restoration, leaves it and
            # then makes its trials
            "grid14-restoration": (lambda: acopf.function_model(acopf.synthetic_grid(14, 5, 20, 1, 1.5), nlp="expr"), dict(max_iter=60))}


def _native(fm, algorithm, opt=None, **kw):
    pr = fm.to_problem("model")
    own = opt is None
    opt = _handle_for(pr, fm) if own else opt
    run = opt.slp_run(pr.x0, A.Parameters(algorithm=algorithm, device_eval=True, **kw))
    if own:
        opt.close()
    return run


@pytest.fixture(scope="module")
def runs():
    """name -> (native SLP-EQP, native Trust Region, model and SlpEQP of the host driver on the HIP optimizer), each on a fresh handle."""
    out = {}
    for name, (make, kw) in _models().items():
        mdl = A.Model.from_problem(make().to_problem(name), A.Parameters(algorithm=EQP, device_eval=True, **kw))
        slp = A.optimize(mdl)
        slp.optimizer.close()
        out[name] = (_native(make(), EQP, **kw), _native(make(), TR, **kw), mdl, slp)
    return out


def _same_bits(a, b):
    assert (a.ret, a.iter, a.lp_solves, a.restoration_solves, a.paths) == (b.ret, b.iter, b.lp_solves, b.restoration_solves, b.paths)
    assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("x", "lam", "mult_x_U", "mult_x_L", "E"))
    assert (a.obj_val, a.delta, a.accepted, a.rejected, a.shrunk, a.expanded) == (b.obj_val, b.delta, b.accepted, b.rejected, b.shrunk, b.expanded)


@pytest.mark.parametrize("name", ["hs071", "grid14", "grid14-restoration"])
def test_native_driver_equals_the_host_driver(runs, name):
    """Iterates, multipliers, radii and counters, bit for bit.  (asm_slp_run_tr's documented caveat - ||grad f|| of the first iteration is
    summed in index order here and by NumPy there - does not show on these models.)  The native entry returns no trace, so the iterates
    compared are the final ones, as for asm_slp_run_tr; every earlier iterate enters them."""
    run, _, mdl, slp = runs[name]
    print("%s: native status %d iter %d lp %d %r radius %.17g | host status %d iter %d lp %d %r radius %.17g" %
          (name, run.ret, run.iter, run.lp_solves, run.eqp_counts, run.Delta_E, slp.ret, slp.iter, slp.lp_solves, slp.eqp_counts, slp.Delta_E))
    assert (run.ret, run.iter, run.lp_solves) == (slp.ret, slp.iter, slp.lp_solves)
    assert run.eqp_counts == slp.eqp_counts and run.Delta_E == slp.Delta_E and run.delta == slp.Delta
    assert np.array_equal(run.x, slp.x) and np.array_equal(run.lam, slp.lam)
    assert np.array_equal(run.mult_x_U, slp.mult_x_U) and np.array_equal(run.mult_x_L, slp.mult_x_L) and np.array_equal(run.E, slp.E)
    assert run.obj_val == mdl.obj_val and mdl.statistics["eqp"] == dict(slp.eqp_counts, radius=slp.Delta_E)
    assert run.restoration_solves == sum(1 for r in slp.trace if r["fr"])
    if name == "grid14-restoration":      # restoration first, trials after it: the clearing of the LP's set and its return are both on the path
        assert run.restoration_solves > 1 and slp.trace[1]["fr"] and not slp.trace[-1]["fr"] and run.eqp_counts["attempts"] > 0


@pytest.mark.parametrize("name", ["hs071", "grid14"])
def test_converges_in_fewer_iterations_than_trust_region(runs, name):
    run, tr = runs[name][:2]
    c = run.eqp_counts
    print("%s: SLP-EQP status %d iter %d lp %d %r | Trust Region status %d iter %d lp %d" % (name, run.ret, run.iter, run.lp_solves, c, tr.ret, tr.iter, tr.lp_solves))
    assert run.ret == 0 and run.iter < tr.iter
    assert c["accepted"] >= 1 and c["attempts"] == c["accepted"] + c["rejected"] + c["skipped_rows"] + c["skipped_dependent"] + c["skipped_zero"]
    if name == "hs071":
        assert np.abs(run.x - HS071_X).max() <= 1e-5


@pytest.mark.parametrize("name", ["hs071", "grid14"])
def test_disabled_is_the_trust_region_run_bit_for_bit(runs, name):
    make, kw = _models()[name]
    off = _native(make(), EQP, eqp=False, **kw)
    _same_bits(off, runs[name][1])
    assert off.eqp_counts == dict.fromkeys(off.eqp_counts, 0) and off.Delta_E == A.Parameters().tr_size


@pytest.mark.parametrize("name", ["hs071", "grid14"])
def test_trust_region_after_an_eqp_run_on_the_same_handle(runs, name):
    """The handle runs SLP-EQP, drops the LP's retained active sets and basis columns (asm_sublp_reset_warm: every run leaves those behind,
    a Trust-Region run too) and then runs Trust Region: the bits of a Trust-Region run on a fresh handle."""
    make, kw = _models()[name]
    fm = make()
    opt = _handle_for(fm.to_problem(name), fm)
    first = _native(fm, EQP, opt, **kw)
    opt.reset_warm()
    second = _native(fm, TR, opt, **kw)
    opt.close()
    assert np.array_equal(first.x, runs[name][0].x) and first.eqp_counts == runs[name][0].eqp_counts
    _same_bits(second, runs[name][1])


def test_trust_region_after_trust_region_with_the_reset_is_a_fresh_run(runs):
    """What the reset above is for, shown on the Trust-Region driver alone: a second run on the same handle after asm_sublp_reset_warm gives
    the bits of a fresh handle."""
    make, kw = _models()["grid14"]
    fm = make()
    opt = _handle_for(fm.to_problem("grid14"), fm)
    _same_bits(_native(fm, TR, opt, **kw), runs["grid14"][1])
    opt.reset_warm()
    _same_bits(_native(fm, TR, opt, **kw), runs["grid14"][1])
    opt.close()


def test_native_optimize_selects_the_driver():
    mdl = A.Model.from_problem(A.problems.hs071_problem(), A.Parameters(algorithm=EQP, device_eval=True))
    run = A.optimize(mdl, native=True)
    assert mdl.status == 0 and run.eqp_counts["accepted"] >= 1 and mdl.statistics["eqp"]["radius"] == run.Delta_E
    assert np.abs(mdl.x - HS071_X).max() <= 1e-5


# ------------------------------------------------------------------------------------------------ 3. errors
def test_argument_and_state_errors_leave_the_handle_usable():
    lib = _lib.load()
    fm, pr, x, lam = hs071_start()
    n, m = pr.n, pr.m
    nu = np.array([1.5, 0.7])
    good_rows, good_bnd = np.array([1, 1], np.int32), np.array([-1, 0, 0, 0], np.int32)
    D, I = _lib.dptr, _lib.i32ptr

    def call(opt, rows=good_rows, bnd=good_bnd, radius=1.0, tol=1e-8, par=None):
        d, ln, mU, mL = np.empty(n), np.empty(m), np.empty(n), np.empty(n)
        rs, bs, info = np.zeros(m, np.int32), np.zeros(n, np.int32), _lib.EqpInfo()
        return lib.asm_eqp_trial(opt._h, D(x), D(lam), I(rows), I(bnd), radius, D(nu), tol, par, D(d), D(ln), D(mU), D(mL), I(rs), I(bs), C.byref(info))

    bare = A.HipSubOptimizer(A.QpData(np.zeros(n), 0.0, np.zeros(pr.nnz), np.zeros(m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    assert call(bare) == ERR_STATE                                        # no evaluator
    bare.close()
    opt = _handle_for(pr, fm)
    assert call(opt) == ERR_STATE                                         # before asm_eval_functions
    f, df, E = opt.eval_functions(x)
    opt.upload(opt.jacobian_values(), df, f, E, x)
    assert call(opt) == ERR_STATE                                         # inputs from asm_sublp_upload: the evaluator's data are not theirs
    opt.eval_functions(x + 1e-3)
    assert call(opt) == ERR_STATE                                         # x is not the point of the last evaluation
    opt.eval_functions(x)
    for tol in (-1e-8, float("nan")):
        assert call(opt, tol=tol) == ERR_ARG
    for radius in (0.0, -1.0, float("nan")):
        assert call(opt, radius=radius) == ERR_ARG
    assert call(opt, rows=np.array([2, 0], np.int32)) == ERR_ARG
    assert call(opt, rows=np.array([-1, 1], np.int32)) == ERR_ARG
    assert call(opt, bnd=np.array([2, 0, 0, 0], np.int32)) == ERR_ARG
    assert call(opt, par=C.byref(_lib.KktStepParams(10, 1e-12, 1.5))) == ERR_ARG
    assert call(opt, par=C.byref(_lib.KktStepParams(-1, 1e-12, 0.8))) == ERR_ARG
    assert lib.asm_eqp_trial(opt._h, D(x), D(lam), I(good_rows), I(good_bnd), 1.0, D(nu), 1e-8, None, None, None, None, None, None, None, None) == ERR_ARG
    with pytest.raises(ValueError):
        opt.eqp_trial(x, lam, [1, 1, 0], good_bnd, 1.0, nu)
    # asm_slp_run_eqp
    from activesetmethods_amd import batch
    sp = batch.slp_params(A.Parameters(algorithm=EQP, device_eval=True))
    x0 = np.ascontiguousarray(pr.x0, np.float64)
    res = _lib.SlpResult()
    for ep in ((0.0, 1e3, 1e-8), (INF, 1e3, 1e-8), (0.4, 0.0, 1e-8), (0.4, 1e3, -1.0), (float("nan"), 1e3, 1e-8)):
        par = _lib.SlpEqpParams(*ep, 1)
        assert lib.asm_slp_run_eqp(opt._h, C.byref(sp), 0.4, C.byref(par), D(x0), None, None, None, None, None, C.byref(res), None, None) == ERR_ARG, ep
    ok = _lib.SlpEqpParams(0.4, 1e3, 1e-8, 1)
    assert lib.asm_slp_run_eqp(opt._h, C.byref(sp), 0.0, C.byref(ok), D(x0), None, None, None, None, None, C.byref(res), None, None) == ERR_ARG
    assert lib.asm_slp_run_eqp(opt._h, C.byref(sp), 0.4, None, D(x0), None, None, None, None, None, C.byref(res), None, None) == ERR_ARG
    # the handle works on
    opt.eval_functions(x)
    assert call(opt) == 0
    run = opt.slp_run(pr.x0, A.Parameters(algorithm=EQP, device_eval=True))
    assert run.ret == 0
    opt.close()
    # the Ohm's-law kernel has no second derivatives: refused as asm_kkt_step refuses it
    from activesetmethods_amd import acopf
    ohm = acopf.function_model(acopf.synthetic_grid(14, 5, 20, 1, 0.5)).to_problem("grid14 ohm")
    o2 = _handle_for(ohm)
    with pytest.raises(A.AsmHipError):
        o2.slp_run(ohm.x0, A.Parameters(algorithm=EQP, device_eval=True))
    assert o2.slp_run(ohm.x0, A.Parameters(algorithm=TR, device_eval=True, max_iter=3)).lp_solves >= 1
    o2.close()
