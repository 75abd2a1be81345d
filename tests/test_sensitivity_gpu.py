"""Solution sensitivities on the device through the C ABI (include/asm_hip.h: asm_eval_data_cross, asm_kkt_solve,
asm_solution_sensitivity): the cross derivatives against the host twin (nlexpr.ExprBlock.data_cross) - bit for bit on arithmetic tapes -
the KKT solve against the dense NumPy solve on constructed QPs, its result statuses, the composed call against closed forms, no
interference with the SLP state, argument and state errors."""
import ctypes as C

import numpy as np
import pytest

from activesetmethods_amd import acopf, nlexpr, problems, sensitivity
from activesetmethods_amd.moi_evaluator import FunctionModel
from activesetmethods_amd.nlexpr import ExprBlock, parameters, variables
from tests.test_nlexpr_cpu import _model
from tests.test_nlhess_cpu import all_ops_model
from tests.test_nlparams_cpu import random_param_block
from tests.test_nlparams_gpu import _handle_for, _same_run
from tests.test_sensitivity_cpu import KKT_BAR, KKT_SHAPES, PARAMETRIC_VALUES, TWIN_ERR_MEASURED, kkt_instance, rel_err

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
INF = float("inf")
# device against twin with math-library ops: the last-bit differences of sin, cos, exp and log (and pow) between the device and host
# math libraries, carried through a few operations of size O(1) - the bar the expression tests use for values of such tapes
LIBM_BAR = 1e-12
# the KKT bar: 10 x the error the NumPy twin of the algorithm shows against the dense solve on the same instances
# (tests/test_sensitivity_cpu.py: measured 1.51e-13 -> 1.51e-12), the factor for the other summation order of the device
# reductions and the device Cholesky; never below 1e-12
assert KKT_BAR == max(10.0 * TWIN_ERR_MEASURED, 1e-12) and 1.5e-12 < KKT_BAR < 1.52e-12


def hs071_param_model():
    """hs071 with its two right-hand sides as parameters: x1 x2 x3 x4 - p0 >= 0, sum xi^2 - p1 == 0, (p0, p1) = (25, 40)."""
    x1, x2, x3, x4 = variables(4)
    p = parameters([25.0, 40.0])
    fm = FunctionModel(4, np.ones(4), np.full(4, 5.0))
    fm.start = {1: 1.0, 2: 5.0, 3: 5.0, 4: 1.0}
    fm.nlp = ExprBlock([(x1 * x2 * x3 * x4 - p[0], 0.0, INF), (x1 ** 2 + x2 ** 2 + x3 ** 2 + x4 ** 2 - p[1], 0.0, 0.0)],
                       objective=x1 * x4 * (x1 + x2 + x3) + x3, n=4, parameters=p)
    return fm


def _twin_cross(fm, x, lam, dc):
    """(u [n], w [m]) of the host twin for a FunctionModel: the block's rows follow the function store's."""
    off = fm.nlp_constraint_offset
    u, wb = fm.nlp.data_cross(x, np.asarray(lam, float)[off:], dc, fm.objective_scale)
    uu, w = np.zeros(fm.n), np.zeros(fm.m)
    uu[:len(u)] = u
    w[off:] = wb
    return uu, w


def _exact_cross_models():
    x = variables(3)
    p = parameters([3.0, -0.5])
    shared = ExprBlock([(p[0] * x[0] * x[1], 0.0, 0.0), (x[0] * x[1] / x[2], 0.0, 0.0), (x[0] * (p[0] * x[0]) + p[1], 0.0, 0.0), (abs(x[2] - p[0]), 0.0, 1.0)],
                       objective=p[0] * x[0] * x[0] + x[1] * p[1] + 2.5 * x[2], n=3, parameters=p)       # a constant in rows and a term; row 1 has none
    out = [("hs071 rhs parameters", hs071_param_model()), ("parametric", problems.parametric_function_model(0.5, 4.0)), ("shared constant", _model(shared, 3))]
    for rows in (1, 257):                                                                                 # one row; two workgroups
        v = np.random.default_rng(rows).uniform(-1.5, 1.5, 3)
        blk, n = random_param_block(40 + rows, v, n=4, rows=rows, exact=True)
        out.append(("random arithmetic, %d rows" % rows, _model(blk, n)))
    return out


def test_data_cross_is_bit_identical_on_arithmetic_tapes():
    for name, fm in _exact_cross_models():
        assert set(fm.nlp.tape.op.tolist()) <= {nlexpr.CONST, nlexpr.VAR, nlexpr.ADD, nlexpr.SUB, nlexpr.MUL, nlexpr.DIV, nlexpr.NEG, nlexpr.POWI,
                                                nlexpr.ABS, nlexpr.MIN, nlexpr.MAX}, name
        opt = _handle_for(fm.to_problem(name), fm)
        rng = np.random.default_rng(len(name))
        for rep in range(2):
            x = fm.start_point() + 0.3 * rng.uniform(-1, 1, fm.n)
            lam, dc = rng.standard_normal(fm.m), rng.standard_normal(len(fm.nlp.device[2]))
            u, w = opt.data_cross(x, lam, dc)
            tu, tw = _twin_cross(fm, x, lam, dc)
            assert np.array_equal(u, tu) and np.array_equal(w, tw), (name, rep, np.abs(u - tu).max(), np.abs(w - tw).max())
            assert np.any(tu != 0.0) or np.any(tw != 0.0)        # (additive right-hand sides move w only)
        opt.close()


def test_data_cross_without_constants_and_with_a_const_exponent():
    x = variables(2)
    nc = _model(ExprBlock([(x[0] * x[1], 0.0, 0.0)], objective=x[0] * x[0], n=2), 2)
    opt = _handle_for(nc.to_problem(), nc)
    u, w = opt.data_cross(np.array([0.3, 0.7]), np.ones(2), np.zeros(0))
    assert not u.any() and not w.any() and u.shape == (2,) and w.shape == (2,)
    opt.close()
    q = parameters([2.5])
    pw = _model(ExprBlock([(nlexpr.pow(x[0], q[0]) + q[0] * x[1], 0.0, 0.0)], n=2, parameters=q), 2)
    opt = _handle_for(pw.to_problem(), pw)
    xv, lam, dc = np.array([1.3, 0.4]), np.array([0.5, 1.0]), np.array([1.0])
    u, w = opt.data_cross(xv, lam, dc)
    tu, tw = _twin_cross(pw, xv, lam, dc)
    # g = x0^q + q x1:  w = dg/dq = x0^q log x0 + x1,  u = -lam d/dq grad g = -(x0^(q-1) (1 + q log x0), 1); pow and log are the
    # libraries': the closed form and the twin at LIBM_BAR, what no library value enters bit for bit
    lx = float(np.log(1.3))
    want_w, want_u0 = 1.3 ** 2.5 * lx + 0.4, -(1.3 ** 1.5 * (1.0 + 2.5 * lx))
    assert w[0] == 0.0 and u[1] == -1.0 and tw[0] == 0.0 and tu[1] == -1.0
    assert abs(w[1] - want_w) <= LIBM_BAR * abs(want_w) and abs(u[0] - want_u0) <= LIBM_BAR * abs(want_u0)
    assert abs(w[1] - tw[1]) <= LIBM_BAR * abs(want_w) and abs(u[0] - tu[0]) <= LIBM_BAR * abs(want_u0)
    opt.close()


def _branch_case(name="case118"):
    return acopf.function_model(acopf.synthetic_case(name, 1, 0.5), nlp="expr", branch_params=True)


def test_data_cross_with_math_library_ops():
    rng = np.random.default_rng(5)
    fa = all_ops_model()
    fb = _branch_case()
    for name, fm, x in (("all ops", fa, rng.uniform(0.4, 1.1, 4)), ("acopf case118 branch parameters", fb, fb.start_point() + 0.01 * rng.standard_normal(fb.n))):
        opt = _handle_for(fm.to_problem(name), fm)
        lam, dc = rng.standard_normal(fm.m), rng.standard_normal(len(fm.nlp.device[2]))
        u, w = opt.data_cross(x, lam, dc)
        tu, tw = _twin_cross(fm, x, lam, dc)
        eu, ew = rel_err(u, tu), rel_err(w, tw)
        print("%s: rel |u - twin| = %.3e, rel |w - twin| = %.3e (max |u| %.3e)" % (name, eu, ew, np.abs(tu).max()))
        assert eu <= LIBM_BAR and ew <= LIBM_BAR and np.any(tu != 0.0) and np.any(tw != 0.0), (name, eu, ew)
        opt.close()


# ------------------------------------------------------------------------------------------------ asm_kkt_solve
@pytest.fixture(scope="module")
def kkt_cases():
    """shape -> (instance, kkt_reference's answer), once for the module."""
    out = {}
    for shape in KKT_SHAPES:
        inst = kkt_instance(*shape)
        out[shape] = (inst, sensitivity.kkt_reference(*inst))
    return out


def _residuals(inst, dx, dlam):
    fm, x, lam, rs, bs, ru, rw = inst
    H, J = sensitivity.lagrangian_hessian(fm, x, lam), sensitivity.dense_jacobian(fm, x)
    F, W = bs == 0, rs == 1
    stat = (H @ dx - J[W].T @ dlam[W] + ru)[F]
    feas = J[W] @ dx + rw[W]
    return (float(np.abs(stat).max()) if F.any() else 0.0), (float(np.abs(feas).max()) if W.any() else 0.0)


@pytest.mark.parametrize("shape", KKT_SHAPES, ids=lambda s: "n%d_B%d_W%d" % s)
def test_kkt_solve_against_the_dense_solve(kkt_cases, shape):
    inst, (rx, rl, rz) = kkt_cases[shape]
    fm, x, lam, rs, bs, ru, rw = inst
    n, nB, nW = shape
    opt = _handle_for(fm.to_problem(), fm)
    dx, dlam, dz, info = opt.kkt_solve(x, lam, rs, bs, ru, rw)
    ex, el, ez = rel_err(dx, rx), rel_err(dlam, rl), rel_err(dz, rz)
    print("shape %r: status %d, %d CG iterations, rel err dx %.3e dlam %.3e dz %.3e (bar %.3e), res %.3e / %.3e"
          % (shape, info.status, info.cg_iters, ex, el, ez, KKT_BAR, info.res_stat, info.res_feas))
    assert info.status == 0 and info.n_free == n - nB and info.n_rows == nW and info.dropped_pivots == 0
    assert (info.cg_iters == 0) == (n - nB == nW) and info.cg_iters <= 2 * (n - nB - nW) + 20
    assert ex <= KKT_BAR and el <= KKT_BAR and ez <= KKT_BAR, (shape, ex, el, ez)
    assert np.all(dx[bs != 0] == 0.0) and np.all(dlam[rs == 0] == 0.0) and np.all(dz[bs == 0] == 0.0)
    ws, wf = _residuals(inst, dx, dlam)
    scale = max(1.0, float(np.abs(ru).max()), float(np.abs(rw).max()))
    assert abs(info.res_stat - ws) <= KKT_BAR * scale and abs(info.res_feas - wf) <= KKT_BAR * scale, (info.res_stat, ws, info.res_feas, wf)
    # dz == NULL is allowed, and the answer repeats bit for bit
    d2, l2 = np.empty(n), np.empty(fm.m)
    from activesetmethods_amd import _lib
    i2 = _lib.KktInfo()
    a = lambda v: np.ascontiguousarray(v, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    s32 = lambda v: np.ascontiguousarray(v, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert opt._lib.asm_kkt_solve(opt._h, a(x), a(lam), s32(rs), s32(bs), a(ru), a(rw), None, a(d2), a(l2), None, C.byref(i2)) == 0
    assert np.array_equal(d2, dx) and np.array_equal(l2, dlam) and i2.cg_iters == info.cg_iters
    opt.close()


def test_kkt_solve_result_statuses(kkt_cases):
    """Ordinary inputs with another answer than "solved": the call returns normally and the handle works on."""
    neg = np.full(8, 4.0)
    neg[2] = -50.0
    fm, x, lam, rs, bs, ru, rw = kkt_instance(8, 0, 2, seed=3, diag=neg)       # a negative eigenvalue on null(A)
    opt = _handle_for(fm.to_problem(), fm)
    dx, dlam, dz, info = opt.kkt_solve(x, lam, rs, bs, ru, rw)
    assert info.status == 2 and np.all(np.isfinite(dx)) and np.all(np.isfinite(dlam)) and np.all(np.isfinite(dz))
    bs2 = bs.copy()
    bs2[2] = 1                                                          # the next call on the handle, the negative direction at a bound: convex
    got, ref = opt.kkt_solve(x, lam, rs, bs2, ru, rw), sensitivity.kkt_reference(fm, x, lam, rs, bs2, ru, rw)
    assert got[3].status == 0 and rel_err(got[0], ref[0]) <= KKT_BAR and rel_err(got[1], ref[1]) <= KKT_BAR and rel_err(got[2], ref[2]) <= KKT_BAR
    opt.close()
    fm, x, lam, rs, bs, ru, rw = kkt_instance(12, 2, 4, seed=4, duplicate_row=True)
    opt = _handle_for(fm.to_problem(), fm)
    dx, dlam, dz, info = opt.kkt_solve(x, lam, rs, bs, ru, rw)
    assert info.status == 3 and info.dropped_pivots >= 1 and np.all(np.isfinite(dx)) and np.all(np.isfinite(dlam))
    rs1 = rs.copy()
    rs1[1] = 0                                                          # without the duplicate the same handle solves
    got, ref = opt.kkt_solve(x, lam, rs1, bs, ru, rw), sensitivity.kkt_reference(fm, x, lam, rs1, bs, ru, rw)
    assert got[3].status == 0 and rel_err(got[0], ref[0]) <= KKT_BAR and rel_err(got[1], ref[1]) <= KKT_BAR
    opt.close()
    inst, ref = kkt_cases[(200, 20, 130)]
    fm, x, lam, rs, bs, ru, rw = inst
    opt = _handle_for(fm.to_problem(), fm)
    dx, dlam, dz, info = opt.kkt_solve(x, lam, rs, bs, ru, rw, max_iter=1, rtol=1e-12)
    assert info.status == 1 and info.cg_iters == 1 and np.all(np.isfinite(dx))
    assert opt.kkt_solve(x, lam, rs, bs, ru, rw)[3].status == 0
    with pytest.raises(ValueError):
        opt.kkt_solve(x, lam, rs, bs, ru, rw, max_iter=3)
    with pytest.raises(ValueError):
        opt.kkt_solve(x[:-1], lam, rs, bs, ru, rw)
    opt.close()


# ------------------------------------------------------------------------------------------------ asm_solution_sensitivity
@pytest.mark.parametrize("a,p", PARAMETRIC_VALUES)
def test_solution_sensitivity_reproduces_the_closed_forms(a, p):
    fm = problems.parametric_function_model(a, p)
    s = float(np.sqrt(p))
    x, lam = np.array([s, s]), np.array([a + 1.0 + 0.5 / s, s * (1.0 - a) - 0.5])
    rs, bs = sensitivity.working_set(fm.to_problem(), x, lam, np.zeros(2), np.zeros(2))
    assert rs.tolist() == [1, 1] and bs.tolist() == [0, 0]
    opt = _handle_for(fm.to_problem(), fm)
    want = {0: (np.zeros(2), np.array([1.0, -s])), 1: (np.full(2, 0.5 / s), np.array([-0.25 / p ** 1.5, (1.0 - a) / (2.0 * s)]))}
    for k in range(2):
        dc = np.zeros(2)
        dc[k] = 1.0
        dx, dlam, dz, info = sensitivity.solution_sensitivity(opt, fm, x, lam, rs, bs, dc)
        assert info.status == 0 and info.cg_iters == 0 and not dz.any()
        assert rel_err(dx, want[k][0]) <= KKT_BAR and rel_err(dlam, want[k][1]) <= KKT_BAR, (k, dx, dlam)
    opt.close()


def test_solution_sensitivity_on_hs071_equals_the_reference_fed_with_the_twin():
    import activesetmethods_amd as A
    fm = hs071_param_model()
    pr = fm.to_problem("hs071 rhs parameters")
    opt = _handle_for(pr, fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm="Trust Region", max_iter=60, device_eval=True), 0)
    rs, bs = sensitivity.working_set(pr, run.x, run.lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    assert run.ret == 0 and rs.tolist() == [1, 1] and bs.tolist() == [-1, 0, 0, 0]
    for dc in (np.array([1.0, 0.0]), np.array([0.0, 1.0]), np.array([0.3, -0.2])):
        u, w = _twin_cross(fm, run.x, run.lam, dc)
        ref = sensitivity.kkt_reference(fm, run.x, run.lam, rs, bs, u, w)
        dx, dlam, dz, info = opt.solution_sensitivity(run.x, run.lam, rs, bs, dc)
        print("hs071 dc %r: status %d, %d CG iterations, dx %r" % (dc.tolist(), info.status, info.cg_iters, dx.tolist()))
        assert info.status == 0 and info.n_free == 3 and info.n_rows == 2
        assert rel_err(dx, ref[0]) <= KKT_BAR and rel_err(dlam, ref[1]) <= KKT_BAR and rel_err(dz, ref[2]) <= KKT_BAR
        assert np.any(dx != 0.0)
    opt.close()


def test_solution_sensitivity_on_the_branch_parameter_acopf():
    """case118-sized ACOPF with its branch admittances as data (seed 1, load 0.5): point and multipliers of a short asm_slp_run, the set
    from working_set; the dense KKT residual K sol - rhs of the device's answer, recomputed in NumPy, stays under the bar relative to
    the size of its terms."""
    import activesetmethods_amd as A
    fm = _branch_case()
    pr = fm.to_problem("acopf branch parameters")
    opt = _handle_for(pr, fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm="Line Search", max_iter=60, device_eval=True), 6)
    x, lam = run.x, run.lam
    rs, bs = sensitivity.working_set(pr, x, lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    H, J = sensitivity.lagrangian_hessian(fm, x, lam), sensitivity.dense_jacobian(fm, x)
    F, W = np.nonzero(bs == 0)[0], np.nonzero(rs == 1)[0]
    Aw = J[np.ix_(W, F)]
    sv = np.linalg.svd(Aw, compute_uv=False)
    print("acopf: n %d, m %d, |F| %d, |W| %d, singular values of A in [%.3e, %.3e]" % (fm.n, fm.m, len(F), len(W), sv[-1], sv[0]))
    assert len(W) <= len(F) and sv[-1] > 1e-5 * sv[0]                   # full-rank working rows at this seed and load (checked on the host)
    dc = np.random.default_rng(9).standard_normal(len(fm.nlp.device[2]))
    u, w = opt.data_cross(x, lam, dc)
    dx, dlam, dz, info = opt.solution_sensitivity(x, lam, rs, bs, dc)
    r1 = (H @ dx - J[W].T @ dlam[W] + u)
    r2 = J[W] @ dx + w[W]
    size = max(1.0, float(np.abs(u).max()), float(np.abs(w).max()), float(np.abs(H).max() * np.abs(dx).max()), float(np.abs(J).max() * np.abs(dlam).max()))
    e1, e2 = float(np.abs(r1[F]).max()) / size, float(np.abs(r2).max()) / size if len(W) else 0.0
    print("acopf: status %d, %d CG iterations, relative residuals %.3e / %.3e (bar %.3e), info %.3e / %.3e" % (info.status, info.cg_iters, e1, e2, KKT_BAR, info.res_stat, info.res_feas))
    assert info.status == 0 and 0 < info.cg_iters <= 2 * (len(F) - len(W)) + 20
    assert np.all(dx[bs != 0] == 0.0) and np.all(dlam[rs == 0] == 0.0) and np.all(dz[F] == 0.0)
    assert np.array_equal(dz[bs != 0], r1[bs != 0]) or rel_err(dz[bs != 0], r1[bs != 0]) <= KKT_BAR
    assert e1 <= KKT_BAR and e2 <= KKT_BAR, (e1, e2)
    opt.close()


# ------------------------------------------------------------------------------------------------ isolation, errors
def test_the_new_calls_do_not_interfere():
    """A 3-LP asm_slp_run returns the same bits with the three calls made before it and between two runs as without; the retained active
    set, the null-space basis and the Jacobian values of the LP are unchanged across a call."""
    import activesetmethods_amd as A
    for fm, alg in ((hs071_param_model(), "Trust Region"), (_branch_case(), "Line Search")):
        pr = fm.to_problem()
        par = A.Parameters(algorithm=alg, max_iter=60, device_eval=True)
        rng = np.random.default_rng(3)
        lam, dc = rng.standard_normal(pr.m), rng.standard_normal(len(fm.nlp.device[2]))
        ru, rw = rng.standard_normal(pr.n), rng.standard_normal(pr.m)
        outs = []
        for calls in (False, True):
            opt = _handle_for(pr, fm)

            def new_calls(x, lm):
                rs, bs = sensitivity.working_set(pr, x, lm, np.zeros(pr.n), np.zeros(pr.n), tol=1e-6)
                if rs.sum() > (bs == 0).sum():
                    rs[:] = 0
                opt.data_cross(x, lm, dc)
                opt.kkt_solve(x, lm, rs, bs, ru, rw)
                opt.solution_sensitivity(x, lm, rs, bs, dc)
            f0 = opt.eval_functions(pr.x0)
            if calls:
                new_calls(pr.x0 + 0.01, lam)
            run = opt.slp_run(pr.x0, par, 3)
            state = (opt.active_set(), opt.ns_basis(), opt.jacobian_values())
            if calls:
                new_calls(run.x, run.lam)
                after = (opt.active_set(), opt.ns_basis(), opt.jacobian_values())
                assert all(np.array_equal(p, q) for p, q in zip(state[0], after[0])) and np.array_equal(state[1], after[1]) and np.array_equal(state[2], after[2])
            run2 = opt.slp_run(pr.x0, par, 3)
            outs.append((f0, run, run2))
            opt.close()
        (fa, ra, ra2), (fb, rb, rb2) = outs
        assert 1 <= ra.lp_solves <= 3
        _same_run(ra, rb)
        _same_run(ra2, rb2)
        assert fa[0] == fb[0] and np.array_equal(fa[1], fb[1]) and np.array_equal(fa[2], fb[2])


def test_argument_and_state_errors():
    import activesetmethods_amd as A
    from activesetmethods_amd import _lib
    lib = _lib.load()
    fm = hs071_param_model()
    pr = fm.to_problem()
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    x, lam, dc, ru, rw = pr.x0.copy(), np.array([0.5, -0.3]), np.ones(len(fm.nlp.device[2])), np.ones(4), np.ones(2)
    u, w, dx, dlam, dz = np.zeros(4), np.zeros(2), np.zeros(4), np.zeros(2), np.zeros(4)
    rs, bs = np.array([1, 1], np.int32), np.array([-1, 0, 0, 0], np.int32)
    info = _lib.KktInfo()
    D, I = _lib.dptr, _lib.i32ptr
    cross = lambda a: lib.asm_eval_data_cross(opt._h, *a)
    kkt = lambda a: lib.asm_kkt_solve(opt._h, *a)
    sens = lambda a: lib.asm_solution_sensitivity(opt._h, *a)
    ca = [D(x), D(lam), D(dc), D(u), D(w)]
    ka = [D(x), D(lam), I(rs), I(bs), D(ru), D(rw), None, D(dx), D(dlam), D(dz), C.byref(info)]
    sa = [D(x), D(lam), I(rs), I(bs), D(dc), None, D(dx), D(dlam), D(dz), C.byref(info)]
    assert cross(ca) == ERR_STATE and kkt(ka) == ERR_STATE and sens(sa) == ERR_STATE                     # before asm_eval_setup
    opt.eval_setup(fm)
    f0 = opt.eval_functions(pr.x0)
    assert cross(ca) == 0 and kkt(ka) == 0 and sens(sa) == 0
    for bad in range(5):
        a = list(ca)
        a[bad] = None
        assert cross(a) == ERR_ARG, bad
    for bad in (0, 1, 2, 3, 4, 5, 7, 8, 10):                                                             # par and dz may be NULL
        a = list(ka)
        a[bad] = None
        assert kkt(a) == ERR_ARG, bad
    for bad in (0, 1, 2, 3, 4, 6, 7, 9):
        a = list(sa)
        a[bad] = None
        assert sens(a) == ERR_ARG, bad
    assert lib.asm_kkt_solve(None, *ka) == ERR_ARG
    for brs, bbs in ((np.array([2, 1], np.int32), bs), (rs, np.array([2, 0, 0, 0], np.int32)), (rs, np.array([-1, 1, 1, 0], np.int32))):   # a state of 2; |W| > |F|
        a = list(ka)
        a[2], a[3] = I(brs), I(bbs)
        assert kkt(a) == ERR_ARG
        b = list(sa)
        b[2], b[3] = I(brs), I(bbs)
        assert sens(b) == ERR_ARG
    f1 = opt.eval_functions(pr.x0)                                                                        # the handle still evaluates
    assert f0[0] == f1[0] and np.array_equal(f0[1], f1[1]) and np.array_equal(f0[2], f1[2])
    tu, tw = _twin_cross(fm, x, lam, dc)
    gu, gw = opt.data_cross(x, lam, dc)
    assert np.array_equal(gu, tu) and np.array_equal(gw, tw)
    with pytest.raises(ValueError):
        opt.data_cross(x, lam, dc[:-1])
    opt.close()
    for fk in (acopf.function_model(acopf.synthetic_case("case118", 1, 0.5)), problems.synthetic_dense_function_model(40, 10)):      # kinds 1 and 2
        pk = fk.to_problem()
        ok = _handle_for(pk, fk)
        z = lambda k: np.zeros(max(k, 1))
        rs0, bs0 = np.zeros(pk.m, np.int32), np.zeros(pk.n, np.int32)
        nd = len(fk.nlp.device[2])
        assert lib.asm_eval_data_cross(ok._h, D(pk.x0), D(z(pk.m)), D(z(nd)), D(z(pk.n)), D(z(pk.m))) == ERR_ARG
        assert lib.asm_kkt_solve(ok._h, D(pk.x0), D(z(pk.m)), I(rs0), I(bs0), D(z(pk.n)), D(z(pk.m)), None, D(z(pk.n)), D(z(pk.m)), None, C.byref(info)) == ERR_ARG
        assert lib.asm_solution_sensitivity(ok._h, D(pk.x0), D(z(pk.m)), I(rs0), I(bs0), D(z(nd)), None, D(z(pk.n)), D(z(pk.m)), None, C.byref(info)) == ERR_ARG
        with pytest.raises(A.AsmHipError, match="second derivatives"):
            ok.kkt_solve(pk.x0, np.zeros(pk.m), rs0, bs0, np.zeros(pk.n), np.zeros(pk.m))
        f, df, E = ok.eval_functions(pk.x0)
        assert np.isfinite(f) and np.all(np.isfinite(E))
        ok.close()
