"""KKT solves and solution sensitivities of a scenario batch, the host side (include/asm_hip.h, "Scenario batches: KKT solves and
sensitivities"): the NumPy statement of the bound right-hand sides the device makes, the stacked working sets, the condition the GPU
test of the hs071 scenarios relies on - checked on the twins - and the exports of the library and the header.  No GPU."""
import os
import re

import numpy as np
import pytest

from activesetmethods_amd import _lib, batch, problems, sensitivity
from tests.test_sensitivity_cpu import rel_err
from tests.test_sensitivity_gpu import _twin_cross, hs071_param_model
from tests.test_sensitivity_multi_cpu import KKT_MULTI_BAR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"asm_bound_sensitivity_multi": ("asm_handle* h", 13), "asm_batch_kkt_solve": ("asm_batch* b", 14),
               "asm_batch_solution_sensitivity": ("asm_batch* b", 14), "asm_batch_bound_sensitivity": ("asm_batch* b", 14)}
HS071_SCENARIOS = 4


def hs071_scenario_models(count=HS071_SCENARIOS):
    """hs071 with its two right-hand sides as parameters, (p0, p1) = (25 + s, 40 + 0.5 s) for s = 0 .. count - 1: one model per scenario,
    the same tape, other data."""
    out = []
    for s in range(count):
        fm = hs071_param_model()
        fm.nlp.set_parameter_values([25.0 + s, 40.0 + 0.5 * s])
        out.append(fm)
    return out


def test_bound_rhs_states_what_the_kernel_writes():
    m, n = 7, 5
    rows = [3, 0, 3, 6]                                            # a duplicate row
    RU, RW = sensitivity.bound_rhs(m, n, rows)
    assert RU.shape == (4, n) and RW.shape == (4, m) and RU.dtype == RW.dtype == np.float64 and not RU.any()
    want = np.zeros((4, m))
    for c, r in enumerate(rows):
        want[c, r] = -1.0
    assert np.array_equal(RW, want)
    delta = np.array([0.5, -2.0, 3.0, 1e-3])
    RU2, RW2 = sensitivity.bound_rhs(m, n, rows, delta)
    assert not RU2.any() and np.array_equal(RW2, want * delta[:, None]) and RW2[0, 3] == -0.5 and RW2[2, 3] == -3.0 and RW2[1, 0] == 2.0
    one = sensitivity.bound_rhs(m, n, 2)
    assert one[0].shape == (1, n) and one[1].shape == (1, m) and one[1][0, 2] == -1.0 and np.count_nonzero(one[1]) == 1
    for bad in ([m], [-1], [[0, 1]]):
        with pytest.raises(ValueError):
            sensitivity.bound_rhs(m, n, bad)
    with pytest.raises(ValueError):
        sensitivity.bound_rhs(m, n, rows, delta[:-1])
    # what bound_jacobian feeds asm_kkt_solve_multi is this statement with unit moves
    fm = problems.parametric_function_model(0.5, 4.0)
    seen = {}

    class Recorder:
        def kkt_solve_multi(self, x, lam, rs, bs, RU, RW, max_iter=None, rtol=None):
            seen["rhs"] = (RU, RW)
            return np.zeros((len(RU), fm.n)), np.zeros((len(RU), fm.m)), None, [dict(status=0)] * len(RU)
    sensitivity.bound_jacobian(Recorder(), fm, np.ones(2), np.zeros(2), np.ones(2, np.int32), np.zeros(2, np.int32), [1, 0])
    ru, rw = sensitivity.bound_rhs(fm.m, fm.n, [1, 0])
    assert np.array_equal(seen["rhs"][0], ru) and np.array_equal(seen["rhs"][1], rw)


class _Run:
    def __init__(self, x, lam, n):
        self.x, self.lam, self.mult_x_U, self.mult_x_L = x, lam, np.zeros(n), np.zeros(n)


@pytest.fixture(scope="module")
def hs071_points():
    """Per scenario (fm, problem, x*, lam*) with x* from SciPy SLSQP at the model's start and lam* the least-squares multipliers of the
    stationarity equations on the free variables (the sign convention of the SLP drivers: grad f = J' lam)."""
    from scipy.optimize import minimize
    out = []
    for fm in hs071_scenario_models():
        pr = fm.to_problem("hs071 scenario")
        g = lambda x, pr=pr: np.asarray(pr.eval_g(np.asarray(x, float), np.zeros(pr.m)), float)
        res = minimize(lambda x, pr=pr: pr.eval_f(np.asarray(x, float)), pr.x0, jac=lambda x, pr=pr: np.asarray(pr.eval_grad_f(np.asarray(x, float), np.zeros(pr.n)), float),
                       bounds=list(zip(pr.x_L, pr.x_U)), method="SLSQP", options=dict(ftol=1e-14, maxiter=200),
                       constraints=[dict(type="ineq", fun=lambda x, g=g: g(x)[0]), dict(type="eq", fun=lambda x, g=g: g(x)[1])])
        x = np.clip(res.x, pr.x_L, pr.x_U)
        F = x > pr.x_L + 1e-6
        J, gf = sensitivity.dense_jacobian(fm, x), np.asarray(pr.eval_grad_f(x, np.zeros(pr.n)), float)
        lam = np.linalg.lstsq(J[:, F].T, gf[F], rcond=None)[0]
        assert np.abs(J[:, F].T @ lam - gf[F]).max() <= 1e-6 and np.abs(g(x)).max() <= 1e-8, (res.message, x)
        out.append((fm, pr, x, lam))
    return out


def test_working_sets_stack_the_per_problem_calls(hs071_points):
    prs = [p[1] for p in hs071_points]
    runs = [_Run(p[2], p[3], p[1].n) for p in hs071_points]
    rs, bs = batch.working_sets(prs, runs)
    assert rs.shape == (HS071_SCENARIOS, 2) and bs.shape == (HS071_SCENARIOS, 4) and rs.dtype == bs.dtype == np.int32
    for s, (pr, r) in enumerate(zip(prs, runs)):
        one = sensitivity.working_set(pr, r.x, r.lam, r.mult_x_U, r.mult_x_L, tol=1e-6)
        assert np.array_equal(rs[s], one[0]) and np.array_equal(bs[s], one[1])
    # both rows and x1 at its lower bound in all four scenarios: what the GPU test of the batch expects of the device's points
    assert rs.tolist() == [[1, 1]] * HS071_SCENARIOS and bs.tolist() == [[-1, 0, 0, 0]] * HS071_SCENARIOS
    tight = batch.working_sets(prs, runs, tol=0.0)                 # (the tolerance reaches the per-problem call)
    assert np.array_equal(tight[0][0], sensitivity.working_set(prs[0], runs[0].x, runs[0].lam, runs[0].mult_x_U, runs[0].mult_x_L, tol=0.0)[0])
    with pytest.raises(ValueError):
        batch.working_sets(prs, runs[:-1])
    with pytest.raises(ValueError):
        batch.working_sets([], [])


def test_the_hs071_scenarios_stay_inside_the_condition_of_the_gpu_test(hs071_points):
    """Along the two unit data directions the twin of the device algorithm solves every column of every scenario (status 0, at least one
    CG iteration: one free direction on null(A)) and agrees with the dense solve to the bar of the multi tests."""
    rs, bs = np.array([1, 1], np.int32), np.array([-1, 0, 0, 0], np.int32)
    worst = 0.0
    for s, (fm, pr, x, lam) in enumerate(hs071_points):
        RU, RW = np.zeros((2, fm.n)), np.zeros((2, fm.m))
        for c, dc in enumerate(np.eye(2)):
            RU[c], RW[c] = _twin_cross(fm, x, lam, dc)
        DX, DLAM, DZ, infos = sensitivity.kkt_pcg_multi(fm, x, lam, rs, bs, RU, RW)
        ref = sensitivity.kkt_reference_multi(fm, x, lam, rs, bs, RU, RW)
        errs = [rel_err(g, w) for g, w in zip((DX, DLAM, DZ), ref)]
        print("scenario %d: status %r, CG iterations %r, twin against dense %.3e %.3e %.3e" % ((s, [i["status"] for i in infos], [i["cg_iters"] for i in infos]) + tuple(errs)))
        assert all(i["status"] == 0 and i["cg_iters"] >= 1 for i in infos), s
        assert max(errs) <= KKT_MULTI_BAR, (s, errs)
        assert np.any(DX != 0.0)
        worst = max(worst, *errs)
    print("largest twin-to-dense difference over the 8 columns: %.3e (bar %.3e)" % (worst, KKT_MULTI_BAR))


def test_the_library_exports_the_new_entries():
    text = open(os.path.join(ROOT, "include", "asm_hip.h")).read()
    lib = _lib.load()
    for name, (first, nargs) in NEW_ENTRIES.items():
        assert re.search(r"^int %s\(%s," % (name, re.escape(first)), text, re.M), name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs, name
        assert getattr(lib, name) is not None, name
    assert "Scenario batches: KKT solves and sensitivities" in text


def test_the_batch_wrappers_check_shapes_before_the_call():
    """HipBatch's three methods and HipSubOptimizer.bound_sensitivity_multi raise ValueError before they reach the C call: stand-in objects
    with the sizes and no library."""
    import activesetmethods_amd as A

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("the C call %s was reached" % name)
    hb = object.__new__(batch.HipBatch)
    hb.n, hb.m, hb.n_dpar, hb._lib, hb._b = 4, 2, 3, NoLibrary(), None
    S = 2
    x, lam, rs, bs = np.zeros((S, 4)), np.zeros((S, 2)), np.zeros((S, 2), np.int32), np.zeros((S, 4), np.int32)
    with pytest.raises(ValueError):
        hb.kkt_solve_multi(x, lam, rs, bs, np.zeros((S, 3, 5)), np.zeros((S, 3, 2)))
    with pytest.raises(ValueError):
        hb.kkt_solve_multi(x, lam, rs, bs, np.zeros((S, 3, 4)), np.zeros((S, 2, 2)))
    with pytest.raises(ValueError):
        hb.kkt_solve_multi(x, lam, rs, bs, np.zeros((3, 4)), np.zeros((3, 2)))
    with pytest.raises(ValueError):
        hb.kkt_solve_multi(x, lam[:1], rs, bs, np.zeros((S, 3, 4)), np.zeros((S, 3, 2)))
    for DC in (np.zeros((3, 2)), np.zeros(3), np.zeros((S + 1, 3, 3)), np.zeros((0, 3))):
        with pytest.raises(ValueError):
            hb.solution_sensitivity_multi(x, lam, rs, bs, DC)
    with pytest.raises(ValueError):
        hb.bound_sensitivity(x, lam, rs, bs, [])
    with pytest.raises(ValueError):
        hb.bound_sensitivity(x, lam, rs, bs, [0, 1], delta=[1.0])
    with pytest.raises(ValueError):
        hb.bound_sensitivity(x, lam, rs, bs[:, :-1], [0])
    with pytest.raises(AssertionError, match="asm_batch_kkt_solve"):
        hb.kkt_solve_multi(x, lam, rs, bs, np.zeros((S, 3, 4)), np.zeros((S, 3, 2)))
    for DC in (np.zeros((3, 3)), np.zeros((S, 3, 3))):
        with pytest.raises(AssertionError, match="asm_batch_solution_sensitivity"):
            hb.solution_sensitivity_multi(x, lam, rs, bs, DC)
    with pytest.raises(AssertionError, match="asm_batch_bound_sensitivity"):
        hb.bound_sensitivity(x, lam, rs, bs, [1, 1, 0])
    opt = object.__new__(A.HipSubOptimizer)
    opt.n, opt.m, opt._lib, opt._h = 4, 2, NoLibrary(), None
    with pytest.raises(ValueError):
        opt.bound_sensitivity_multi(x[0], lam[0], rs[0], bs[0], [])
    with pytest.raises(ValueError):
        opt.bound_sensitivity_multi(x[0], lam[0], rs[0], bs[0], [0, 1], delta=[1.0, 2.0, 3.0])
    with pytest.raises(AssertionError, match="asm_bound_sensitivity_multi"):
        opt.bound_sensitivity_multi(x[0], lam[0], rs[0], bs[0], [0, 1])
