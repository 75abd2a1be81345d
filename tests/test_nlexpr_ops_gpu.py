"""The expression ops after COS on the device (include/asm_hip.h, "Expression block"; expr_forward / expr_reverse / expr_libm of
csrc/asm_eval_kernels.hip.h) against the host twin (activesetmethods_amd/nlexpr.py), the tape checks of asm_eval_setup, the batched
line search, the native drivers and a scenario batch."""
import numpy as np
import pytest

from activesetmethods_amd import nlexpr
from tests.test_nlexpr_cpu import _model
from tests.test_nlexpr_gpu import _assert_same, _close, _handle_for, _ls_state, _python_and_native
from tests.test_nlexpr_ops_cpu import ops_function_model, random_ops_block

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sense", ["MIN_SENSE", "MAX_SENSE", "FEASIBILITY_SENSE"])
@pytest.mark.parametrize("exact", [False, True])
def test_device_equals_host_twin(sense, exact):
    """f, grad f, g, the Jacobian values and asm_eval_constraints: bit for bit with + - * / abs min max; within 1e-13 relative
    once the math-library ops enter (device math library against NumPy's)."""
    for seed in range(4):
        block, n = random_ops_block(seed + 30, exact=exact)
        fm = _model(block, n, sense)
        pr = fm.to_problem()
        opt = _handle_for(pr, fm)
        rng = np.random.default_rng(seed + 70)
        for _ in range(3):
            x = rng.uniform(-1.0, 1.0, n)
            f, df, E = opt.eval_functions(x)
            want = (pr.eval_f(x), pr.eval_grad_f(x, np.zeros(n)), pr.eval_g(x, np.zeros(pr.m)), pr.eval_jac_g(x, np.zeros(pr.nnz)))
            got = (f, df, E, opt.jacobian_values())
            assert all(np.all(np.isfinite(w)) for w in want)
            ft, Et = opt.eval_constraints(0.5 * x)
            want_t = (pr.eval_f(0.5 * x), pr.eval_g(0.5 * x, np.zeros(pr.m)))
            if exact:
                assert f == want[0] and all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:]))
                assert ft == want_t[0] and np.array_equal(Et, want_t[1])
            else:
                assert all(_close(g, w, 1e-13) for g, w in zip(got, want)), (seed, [np.max(np.abs(np.asarray(g) - w)) for g, w in zip(got, want)])
                assert _close(ft, want_t[0], 1e-13) and _close(Et, want_t[1], 1e-13)
        opt.close()


def _with_ipar(ipar):
    from activesetmethods_amd.moi_evaluator import NlpBlock
    fm = ops_function_model()
    b = fm.nlp
    fm.nlp = NlpBlock(b.g_L, b.g_U, b.rows, b.cols, b.eval_g, b.eval_jac_g, device=("expr", np.asarray(ipar, np.int64), b.device[2]),
                      has_objective=b.has_objective, eval_f=b.eval_f, eval_grad_f=b.eval_grad_f)
    return fm


def test_eval_setup_rejects_a_bad_b_of_the_new_binary_ops_and_keeps_the_handle():
    """POW, ATAN2, MIN and MAX whose b is the node itself, a later node or negative: ASM_ERR_ARG with a message from asm_eval_setup and
    asm_batch_eval_setup; the handle keeps its evaluator; the valid tape is accepted after."""
    import copy
    from activesetmethods_amd import AsmHipError, batch
    fm = ops_function_model()
    pr = fm.to_problem("ops")
    opt = _handle_for(pr)
    x = np.array([1.3, 0.8])
    before = opt.eval_functions(x)
    R, T, L, ptr, op, a, b = nlexpr.parse_ipar(fm.nlp.device[1])
    row_of = np.searchsorted(ptr, np.arange(L), side="right") - 1
    checked = set()
    for k in range(L):
        o = int(op[k])
        if o not in (nlexpr.POW, nlexpr.ATAN2, nlexpr.MIN, nlexpr.MAX):
            continue
        loc = k - int(ptr[row_of[k]])
        for bad_b in (loc, loc + 3, -1):
            bb = b.copy()
            bb[k] = bad_b
            ip = np.concatenate([[R, T, L], ptr, op, a, bb])
            with pytest.raises(AsmHipError, match="error -1.*operand b is not an earlier node"):
                opt.eval_setup(_with_ipar(ip))
            bad_pr = copy.copy(pr)
            bad_pr.function_model = _with_ipar(ip)
            with pytest.raises(AsmHipError, match=r"batch error -1: asm_eval_setup \(slot 0\): .*operand b"):
                batch.HipBatch(bad_pr, 2)
            after = opt.eval_functions(x)
            assert after[0] == before[0] and all(np.array_equal(u, v) for u, v in zip(after[1:], before[1:])), (o, bad_b)
        checked.add(o)
    assert checked == {nlexpr.POW, nlexpr.ATAN2, nlexpr.MIN, nlexpr.MAX}
    opt.eval_setup(_with_ipar(fm.nlp.device[1]))
    again = opt.eval_functions(x)
    assert again[0] == before[0] and all(np.array_equal(u, v) for u, v in zip(again[1:], before[1:]))
    opt.close()


@pytest.mark.parametrize("fr", [False, True])
def test_device_line_search_equals_trial_by_trial_merit(fr):
    """asm_slp_line_search (eight trial points per set of launches) on the known-answer model: same alpha, merit value and trial count
    as one asm_slp_merit call per trial."""
    pr = ops_function_model().to_problem("ops")
    slp = _ls_state(pr)
    opt = slp.optimizer
    rng = np.random.default_rng(13)
    nu = np.abs(rng.standard_normal(pr.m)) + 0.1
    ps = np.abs(rng.standard_normal(2 * pr.m))
    both = (pr.g_L > -np.inf) & (pr.g_U < np.inf)
    ps[1::2][~both] = np.nan
    S = type("S", (), {"raw": ps})()
    prim, eta, tau, min_alpha = 0.37, 0.4, 0.7, 1e-6
    for scale, dd in ((1e-3, -1.0), (0.05, -5.0), (0.2, -50.0), (0.2, -1e9), (0.1, 1e3)):
        p = scale * rng.uniform(-1.0, 1.0, pr.n)               # x + alpha p stays in [0.05, 3.2]^2, inside every row's domain
        phi0 = opt.slp_merit(0, 0.0, p, nu, S, fr, prim)
        alpha, trials = 1.0, 0
        while True:
            phi_a = opt.slp_merit(0, alpha, p, nu, S, fr, prim)
            trials += 1
            if not (phi_a > phi0 + eta * alpha * dd):
                ok = True
                break
            if alpha < min_alpha:
                ok = False
                break
            alpha *= tau
        got = opt.slp_line_search(p, nu, S, fr, prim, phi0, dd, eta, tau, min_alpha)
        assert np.isfinite(phi_a)
        assert got[3] == ok and got[0] == alpha and got[2] == trials and got[1] == phi_a, (scale, dd, got, alpha, phi_a, trials, ok)
    opt.close()


@pytest.mark.parametrize("alg", ["Line Search", "Trust Region"])
def test_known_answer_model_native_reaches_the_optimum(alg):
    """The native driver reaches (1, 1) with status 0 and equals the Python driver with device evaluation bit for bit."""
    mh, mn, _ = _python_and_native(ops_function_model().to_problem("ops"), alg)
    assert mn.status == 0 and np.allclose(mn.x, [1.0, 1.0], rtol=1e-4), mn.x
    _assert_same(mh, mn)


def test_known_answer_batch_equals_per_scenario_runs_bit_for_bit():
    """Eight scenarios of the known-answer model (other variable bounds) through asm_batch_slp_run (8 slots, and 3) equal asm_slp_run
    per scenario on one handle bit for bit; all reach (1, 1)."""
    import activesetmethods_amd as A
    from activesetmethods_amd import batch
    from tests.test_batch_gpu import _native_run
    prs = [ops_function_model(x_L=(0.25 + 0.05 * s, 0.25 + 0.03 * s), x_U=(3.0 - 0.1 * s, 3.0 - 0.05 * s)).to_problem("ops %d" % s)
           for s in range(8)]
    par = A.Parameters(algorithm="Line Search", max_iter=100, device_eval=True)
    hb = batch.HipBatch(prs[0], 8)
    runs8, stats, _ = batch.solve_batch_lockstep(prs, par, 8, batch=hb)
    J = hb.ns_basis()
    hb.close()
    assert stats["scenarios"] == 8 and stats["converged"] == 8, stats
    hb3 = batch.HipBatch(prs[0], 3)
    hb3.set_ns_basis(J)
    runs3, _, _ = batch.solve_batch_lockstep(prs, par, 3, batch=hb3)
    hb3.close()
    opt = _handle_for(prs[0])
    for s, pr in enumerate(prs):
        opt.set_bounds(A.QpData(None, 0.0, None, None, pr.g_L, pr.g_U, pr.x_L, pr.x_U))
        one = _native_run(opt, pr, par, J)
        assert one.ret == 0 and np.allclose(one.x, [1.0, 1.0], rtol=1e-4), (s, one.x)
        for r in (runs8[s], runs3[s]):
            assert r.ret == one.ret and r.iter == one.iter and r.lp_solves == one.lp_solves and r.paths == one.paths
            assert np.array_equal(r.x, one.x) and np.array_equal(r.lam, one.lam)
            assert np.array_equal(r.mult_x_U, one.mult_x_U) and np.array_equal(r.mult_x_L, one.mult_x_L)
            assert r.obj_val == one.obj_val
    opt.close()
