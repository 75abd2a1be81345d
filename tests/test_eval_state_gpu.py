"""The device evaluator's vector block and lifetime (csrc/asm_hip.hip: EvLayout, EvalState) at the smallest shapes where an offset
can go wrong: asm_slp_norms, asm_slp_merit, asm_slp_step_quality and asm_slp_line_search on models with (n, m) = (2, 1), (5, 3) with a
range row in an expression block (M = m + 1, so Mp and ldn are no multiples of m and n), (33, 31) and (3, 0), against the oracle's
formulas and against each other bit for bit; and one handle through two evaluator set-ups and a new skeleton."""
import numpy as np
import pytest

from tests.test_kkt_step_cpu import hs071_start
from tests.test_nlparams_gpu import _handle_for

pytestmark = pytest.mark.gpu
INF = float("inf")


def _tiny_model(name):
    from activesetmethods_amd.moi_evaluator import FunctionModel, ScalarFunction
    from activesetmethods_amd.nlexpr import ExprBlock, variables
    if name == "2x1":                # function store alone
        fm = FunctionModel(2, np.array([-2.0, -1.0]), np.array([1.5, 3.0]))
        fm.objective = ScalarFunction(0.5, [(1.0, 1), (-0.5, 2)], [(2.0, 1, 1), (1.0, 2, 2), (0.5, 1, 2)])
        fm.add_constraint(ScalarFunction(0.25, [(1.0, 2)], [(1.0, 1, 2)]), "ge", 1.0)
    elif name == "5x3":              # one affine row of the store, two expression rows, the second with two distinct finite bounds
        v = variables(5)
        fm = FunctionModel(5, np.array([-1.0, -2.0, -INF, 0.0, -3.0]), np.array([1.0, INF, 2.0, 4.0, 3.0]))
        fm.objective = ScalarFunction(1.0, [(1.0, 1), (-2.0, 5)], [(1.0, 3, 3), (2.0, 2, 4)])
        fm.add_constraint(ScalarFunction(0.5, [(1.0, 1), (-2.0, 4), (1.0, 5)]), "le", 1.0)
        fm.nlp = ExprBlock([(v[0] * v[1] + v[2] ** 2, 0.5, 0.5), (v[1] - v[3] * v[4] + v[0], -0.25, 1.25)], n=5)
    elif name == "33x31":            # 10 rows of the store, 21 expression rows of which every third is a range row
        n = 33
        rng = np.random.default_rng(33)
        v = variables(n)
        fm = FunctionModel(n, np.where(np.arange(n) % 5 == 0, -INF, -2.0), np.where(np.arange(n) % 7 == 0, INF, 2.0))
        fm.objective = ScalarFunction(0.0, [(float(rng.standard_normal()), j + 1) for j in range(n)], [(1.0 + 0.1 * j, j + 1, j + 1) for j in range(n)])
        for i, kind in zip(range(10), ("le", "ge", "eq") * 4):
            a, b, c = (int(k) + 1 for k in rng.choice(n, 3, replace=False))
            fm.add_constraint(ScalarFunction(float(rng.standard_normal()), [(1.0, a), (-1.5, b)], [(0.5, a, c)] if i % 2 else []), kind, float(rng.standard_normal()))
        rows = []
        for i in range(21):
            a, b, c = (int(k) for k in rng.choice(n, 3, replace=False))
            g = v[a] * v[b] - 0.5 * v[c] ** 2 + v[(a + 1) % n]
            lo = float(rng.standard_normal())
            rows.append((g, lo, lo + 1.5) if i % 3 == 0 else (g, lo, INF) if i % 3 == 1 else (g, lo, lo))
        fm.nlp = ExprBlock(rows, n=n)
    else:                            # "3x0": no rows at all
        fm = FunctionModel(3, np.array([-1.0, -INF, 0.0]), np.array([1.0, 2.0, INF]))
        fm.objective = ScalarFunction(0.5, [(1.0, 1), (-1.0, 3)], [(1.0, 1, 1), (0.5, 2, 3)])
    return fm


TINY = {"2x1": (2, 1, 0), "5x3": (5, 3, 1), "33x31": (33, 31, 7), "3x0": (3, 0, 0)}       # name -> (n, m, range rows)


@pytest.fixture(scope="module")
def tiny():
    """name -> a handle after asm_eval_functions at a point outside some bounds, with a step, penalties, slacks and the oracle's driver on
    the same data; made once per model, shared by the tests (they only read it) and closed after the last of them."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = _tiny_state(name)
        return made[name]
    yield get
    for state in made.values():
        state[0].close()


def _tiny_state(name):
    from oracle import slp as O
    fm = _tiny_model(name)
    pr = fm.to_problem(name)
    both = (pr.g_L > -INF) & (pr.g_U < INF)
    assert (pr.n, pr.m, int((both & (pr.g_L != pr.g_U)).sum())) == TINY[name]
    rng = np.random.default_rng(pr.n)
    x = rng.uniform(-2.5, 2.5, pr.n)
    opt = _handle_for(pr, fm)
    f, df, E = opt.eval_functions(x)
    om = O.Model(pr.n, pr.m, pr.x_L, pr.x_U, pr.g_L, pr.g_U, pr.j_str, pr.eval_f, pr.eval_g, pr.eval_grad_f, pr.eval_jac_g, O.Parameters())
    osl = O.SlpLS(om)
    osl.x = x.copy(); osl.f = f; osl.df = df.copy(); osl.E = E.copy()
    osl.nu = np.abs(rng.standard_normal(pr.m)) + 0.1
    osl.p = 0.3 * rng.standard_normal(pr.n)
    osl.prim_infeas = O.norm_violations(E, pr.g_L, pr.g_U, x, pr.x_L, pr.x_U, np.inf)
    osl.p_slack = {i: ([abs(rng.standard_normal()), abs(rng.standard_normal())] if both[i] else [abs(rng.standard_normal())]) for i in range(pr.m)}
    return opt, pr, x, (f, df, E), osl


def _near(got, want, tol):
    return abs(got - want) <= tol * max(1.0, abs(want))


@pytest.mark.parametrize("name", sorted(TINY))
def test_reductions_equal_the_oracle_at_tiny_shapes(name, tiny):
    """asm_slp_norms within 1e-12, asm_slp_merit (mode 0 at alpha 0, 1, 0.37; mode 1) and asm_slp_step_quality within 1e-11, relative, of
    common.jl:35-98 and slp.jl:79-147 as the oracle restates them, in both phases."""
    from oracle import slp as O
    from oracle.subproblem import compute_jacobian_matrix
    opt, pr, x, (f, df, E), osl = tiny(name)
    rng = np.random.default_rng(5)
    lam = rng.standard_normal(pr.m); mU = 0.1 * rng.standard_normal(pr.n); mL = 0.1 * rng.standard_normal(pr.n)
    J, _ = compute_jacobian_matrix(pr.m, pr.n, pr.j_row - 1, pr.j_col - 1, pr.eval_jac_g(x, np.zeros(pr.nnz)))
    ref = (O.norm_violations(E, pr.g_L, pr.g_U, x, pr.x_L, pr.x_U, np.inf), O.norm_violations(E, pr.g_L, pr.g_U, x, pr.x_L, pr.x_U, 1),
           O.KT_residuals(df, lam, mU, mL, J), O.norm_complementarity(E, pr.g_L, pr.g_U, lam))
    got = opt.slp_norms(lam, mU, mL)
    print(name, "norms", got, ref)
    assert all(_near(a, b, 1e-12) for a, b in zip(got, ref)), (got, ref)
    assert ref[0] > 0.0             # the point violates something: the norms are not trivially zero
    for fr in (False, True):
        osl.feasibility_restoration = fr
        phis = {}
        for alpha in (0.0, 1.0, 0.37):
            phis[alpha] = osl.compute_phi(osl.x, alpha, osl.p)
            got = opt.slp_merit(0, alpha, osl.p, osl.nu, osl.p_slack, fr, osl.prim_infeas)
            assert _near(got, phis[alpha], 1e-11), (fr, alpha, got, phis[alpha])
        D = osl.compute_derivative()
        got = opt.slp_merit(1, 0.0, osl.p, osl.nu, osl.p_slack, fr, osl.prim_infeas)
        assert _near(got, D, 1e-11), (fr, got, D)
        got = opt.step_quality(osl.p, osl.nu, osl.p_slack, fr, osl.prim_infeas)
        assert all(_near(a, b, 1e-11) for a, b in zip(got, (D, phis[0.0], phis[1.0]))), (fr, got, D, phis)


@pytest.mark.parametrize("name", sorted(TINY))
def test_step_quality_equals_three_merit_calls_at_tiny_shapes(name, tiny):
    opt, pr, x, _, osl = tiny(name)
    p, nu, ps, prim = osl.p, osl.nu, osl.p_slack, osl.prim_infeas
    for fr in (False, True):
        got = opt.step_quality(p, nu, ps, fr, prim)
        want = (opt.slp_merit(1, 0.0, p, nu, ps, fr, prim), opt.slp_merit(0, 0.0, p, nu, ps, fr, prim), opt.slp_merit(0, 1.0, p, nu, ps, fr, prim))
        assert np.array_equal(np.array(got), np.array(want)), (fr, got, want)
        assert opt.step_quality(p, nu, ps, fr, prim) == got


@pytest.mark.parametrize("name", sorted(TINY))
def test_line_search_equals_trial_by_trial_merit_at_tiny_shapes(name, tiny):
    """asm_slp_line_search against the loop of slp_line_search.jl:222-244 built from asm_slp_merit calls, bit for bit.  phi0 and D are
    arguments, so each case sets the line phi0 + eta alpha D to pass just above the merit value of trial k and far below the earlier
    ones: the search must stop at trial k exactly - in the first batch of eight, at its last trial, at the first of the second batch,
    inside the second and the third; and once with a line no trial reaches, which ends below min_alpha after 40 trials."""
    opt, pr, x, _, osl = tiny(name)
    p, nu, ps, prim = 3.0 * osl.p, osl.nu, osl.p_slack, osl.prim_infeas
    eta, tau, min_alpha = 0.4, 0.7, 1e-6
    for fr in (False, True):
        alphas, a = [], 1.0
        for _ in range(18):
            alphas.append(a)
            a *= tau
        phi = [opt.slp_merit(0, a, p, nu, ps, fr, prim) for a in alphas]
        scale = max(1.0, max(abs(v) for v in phi))
        cases = [(k, phi[k] + 1e-6 * scale + 1e4 * scale * alphas[k], -1e4 * scale / eta) for k in (0, 3, 7, 8, 10, 17)]
        cases.append((None, opt.slp_merit(0, 0.0, p, nu, ps, fr, prim), -1e9 * scale))
        for k, phi0, dd in cases:
            alpha, trials = 1.0, 0
            while True:
                phi_a = opt.slp_merit(0, alpha, p, nu, ps, fr, prim)
                trials += 1
                if not (phi_a > phi0 + eta * alpha * dd):
                    ok = True
                    break
                if alpha < min_alpha:
                    ok = False
                    break
                alpha *= tau
            assert (ok, trials) == ((True, k + 1) if k is not None else (False, 40)), (name, fr, k, ok, trials)
            got = opt.slp_line_search(p, nu, ps, fr, prim, phi0, dd, eta, tau, min_alpha)
            assert got == (alpha, phi_a, trials, ok), (name, fr, k, got, alpha, phi_a, trials, ok)


def _second_model():
    """The skeleton of hs071_start's model (4 variables, an inequality and an equality over all of them, two parameters) with other
    quadratic terms: another Hessian pattern."""
    from activesetmethods_amd.moi_evaluator import FunctionModel
    from activesetmethods_amd.nlexpr import ExprBlock, parameters, variables
    x1, x2, x3, x4 = variables(4)
    p = parameters([25.0, 40.0])
    fm = FunctionModel(4, np.ones(4), np.full(4, 5.0))
    fm.nlp = ExprBlock([(x1 * x2 + 2.0 * x3 * x4 + x1 * x1 - p[0], 0.0, INF), (x1 + x2 ** 2 + 3.0 * x3 ** 2 + x4 - p[1], 0.0, 0.0)],
                       objective=x1 * x1 + x2 * x2 + x3 * x4 + 2.0 * x4 * x4 + x3, n=4, parameters=p)
    return fm


def _five_calls(opt, x, lam):
    """Every lazily made part of the evaluator: Hessian values and product, the KKT solve, the cross derivatives, the SLP-EQP trial."""
    f, df, E = opt.eval_functions(x)
    rows, cols = opt.hessian_structure()
    out = [np.array([f]), df, E, rows, cols, opt.eval_hessian_lagrangian(x, 1.0, -lam), opt.hessian_product(x, 1.0, -lam, np.arange(1.0, 5.0))]
    rs, bs = np.array([1, 1], np.int32), np.array([-1, 0, 0, 0], np.int32)
    dx, dlam, dz, info = opt.kkt_solve(x, lam, rs, bs, df, np.array([0.01, -0.02]))
    out += [dx, dlam, dz, np.frombuffer(bytes(info), np.uint8)]
    out += list(opt.data_cross(x, lam, np.linspace(1.0, -0.5, len(opt._ev_keep[2]))))       # (the block's constants are data too)
    t = opt.eqp_trial(x, lam, [1, 1], [-1, 0, 0, 0], 1.0, np.array([1.5, 0.7]))
    out += list(t[:6]) + [np.frombuffer(bytes(t[6]), np.uint8)]
    return out


def test_one_handle_through_two_evaluators_and_a_new_skeleton():
    """asm_eval_setup twice on one handle, every lazily made part in between: the second evaluator answers as a fresh handle does, bit for
    bit, with the other model's Hessian pattern.  asm_sublp_setup then ends the evaluator: every entry returns the state error, and the
    handle solves an uploaded LP as a fresh one does."""
    import activesetmethods_amd as A
    from activesetmethods_amd import _lib
    from activesetmethods_amd.subproblem import AsmHipError
    fm1, pr1, x, lam = hs071_start()
    fm2 = _second_model()
    pr2 = fm2.to_problem("second")
    assert pr2.j_str == pr1.j_str and np.array_equal(pr2.g_L, pr1.g_L) and np.array_equal(pr2.g_U, pr1.g_U)
    opt = _handle_for(pr1, fm1)
    first = _five_calls(opt, x, lam)
    opt.eval_setup(fm2)
    second = _five_calls(opt, x, lam)
    fresh1, fresh2 = _handle_for(pr1, fm1), _handle_for(pr2, fm2)
    want1, want2 = _five_calls(fresh1, x, lam), _five_calls(fresh2, x, lam)
    assert len(first) == len(want1) and all(np.array_equal(a, b) for a, b in zip(first, want1))
    assert len(second) == len(want2) and all(np.array_equal(a, b) for a, b in zip(second, want2))
    assert not (len(first[3]) == len(second[3]) and np.array_equal(first[3], second[3]) and np.array_equal(first[4], second[4]))     # another pattern
    assert second[5].any() and second[11].any() and second[13].any()
    # a new skeleton: the evaluator is gone with everything made after it
    c_lb, c_ub, v_lb, v_ub = (np.ascontiguousarray(a, np.float64) for a in (pr1.g_L, pr1.g_U, pr1.x_L, pr1.x_U))
    opt._check(opt._lib.asm_sublp_setup(opt._h, pr1.n, pr1.m, len(opt.j_row), _lib.i64ptr(opt.j_row), _lib.i64ptr(opt.j_col), _lib.dptr(c_lb), _lib.dptr(c_ub),
                                        _lib.dptr(v_lb), _lib.dptr(v_ub)))
    entries = {
        "eval_functions": lambda: opt.eval_functions(x),
        "eval_constraints": lambda: opt.eval_constraints(x),
        "hessian": lambda: opt.eval_hessian_lagrangian(x, 1.0, -lam),
        "hessian_product": lambda: opt.hessian_product(x, 1.0, -lam, np.ones(4)),
        "kkt_solve": lambda: opt.kkt_solve(x, lam, [1, 1], [-1, 0, 0, 0], np.ones(4), np.zeros(2)),
        "data_cross": lambda: opt.data_cross(x, lam, np.ones(len(opt._ev_keep[2]))),
        "data_gradient": lambda: opt.eval_data_gradient(x, lam),
        "set_data": lambda: opt.set_eval_data([26.0]),
        "eqp_trial": lambda: opt.eqp_trial(x, lam, [1, 1], [-1, 0, 0, 0], 1.0, np.array([1.5, 0.7])),
    }
    for name, call in entries.items():
        with pytest.raises(AsmHipError, match="asm_eval_setup first"):
            call()
    df, E, dE = want1[1], want1[2], pr1.eval_jac_g(x, np.zeros(pr1.nnz))
    sols = []
    for o in (opt, fresh1):
        o.data = A.QpData(df, float(want1[0][0]), dE, E, pr1.g_L, pr1.g_U, pr1.x_L, pr1.x_U)
        sols.append(o.sub_optimize(x, 0.5))
    assert sols[0][5] == sols[1][5] == _lib.OPTIMAL
    assert all(np.array_equal(a, b) for a, b in zip(sols[0][:4], sols[1][:4]))
    for o in (opt, fresh1, fresh2):
        o.close()
