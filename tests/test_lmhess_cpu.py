"""CPU checks of the limited-memory Hessian (include/asm_hip.h, "Limited-memory Hessian"): the NumPy twin lmhess.LMHessian - its compact
product against the textbook recursion, the window, the skip rule, the secant equation - the hess= hook of the KKT twins, the
parameter checks, the batch refusals and SlpEQP with hessian_type="limited-memory" on a CPU stand-in sub-optimizer."""
import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import acopf, batch, eqp, sensitivity
from activesetmethods_amd.lmhess import LMHessian
from tests.test_host_cpu import _OracleBackedSubOptimizer
from tests.test_kkt_step_cpu import HS071_RADIUS, HS071_TOL, KKT_STEP_BAR, hs071_start, step_errors
from tests.test_slp_eqp_cpu import HS071_X, run as eqp_run

PRODUCT_BAR = 1e-12
# (n, memory, pushes): memory 1, 3 (five pushes: the window moves twice) and 32.  At n = 4 at most four pairs are pushed into the large
# memory - more could not be independent and S S' would be singular to working precision; at n = 1 088 forty, so that the ring wraps.
STORES = [(4, 1, 2), (4, 3, 5), (4, 32, 4), (1088, 1, 2), (1088, 3, 5), (1088, 32, 40)]


def spd_pairs(n, count, seed=0, cond=100.0):
    """count pairs (s, y = A s) with A symmetric positive definite, eigenvalues spread evenly over [1, cond]: s'y >= ||s||^2 > 0."""
    rng = np.random.default_rng(1000 * n + seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    Am = (Q * np.linspace(1.0, cond, n)) @ Q.T
    Am = 0.5 * (Am + Am.T)
    S = rng.standard_normal((count, n))
    return S, S @ Am


def filled(n, memory, pushes, seed=0, cond=100.0):
    lm = LMHessian(n, memory)
    S, Y = spd_pairs(n, pushes, seed, cond)
    for s, y in zip(S, Y):
        assert lm.push_pair(s, y)
    return lm, S, Y


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("n,memory,pushes", STORES)
def test_product_against_the_recursion(n, memory, pushes):
    lm, S, Y = filled(n, memory, pushes)
    V = np.random.default_rng(7).standard_normal((5, n))
    B = lm.dense()
    err = rel(lm.product(V), V @ B)
    print("n %d memory %d pushes %d: pairs %d sigma %.4g, product against dense() %.2e" % (n, memory, pushes, lm.pairs, lm.sigma, err))
    assert lm.pairs == min(memory, pushes) and err <= PRODUCT_BAR
    assert lm.product(V[0]).shape == (n,) and rel(lm.product(V[0]), lm.product(V)[0]) <= PRODUCT_BAR      # (a vector and a row: BLAS may sum them in another order)
    # B is symmetric positive definite, and the secant equation holds for the newest pair
    assert np.abs(B - B.T).max() <= 1e-12 * np.abs(B).max() and np.linalg.eigvalsh(0.5 * (B + B.T)).min() > 0.0
    assert rel(lm.product(S[-1]), Y[-1]) <= 1e-10


def test_the_window_keeps_the_newest_pairs():
    lm, S, Y = filled(4, 3, 5)
    last = LMHessian(4, 3)
    for s, y in zip(S[2:], Y[2:]):
        last.push_pair(s, y)
    V = np.eye(4)
    assert np.array_equal(lm.product(V), last.product(V)) and lm.sigma == last.sigma
    assert lm.info() == dict(memory=3, pairs=3, pushed=5, skipped_zero=0, skipped_curvature=0, sigma=lm.sigma)


def test_the_skip_rule():
    lm, S, Y = filled(6, 4, 2)
    before, sigma = lm.product(np.eye(6)), lm.sigma
    assert not lm.push_pair(np.zeros(6), Y[0])                      # ||s|| = 0
    assert not lm.push_pair(S[0], -Y[0])                            # s'y < 0
    assert not lm.push_pair(S[0], np.zeros(6))                      # s'y = 0 meets the inequality with y = 0, but every stored pair has s'y > 0
    assert np.array_equal(lm.product(np.eye(6)), before) and lm.sigma == sigma
    info = lm.info()
    assert (info["pairs"], info["pushed"], info["skipped_zero"], info["skipped_curvature"]) == (2, 5, 1, 2)


def test_no_pairs_is_the_identity():
    lm = LMHessian(5, 3)
    V = np.random.default_rng(1).standard_normal((2, 5))
    assert np.array_equal(lm.product(V), V) and np.array_equal(lm.dense(), np.eye(5)) and lm.sigma == 1.0
    assert lm.end(np.zeros(5), np.zeros(5)) is None and lm.info()["pushed"] == 0          # no pending begin: nothing
    lm.begin(np.zeros(5), np.zeros(5))
    assert lm.end(np.ones(5), 2.0 * np.ones(5)) is True and lm.sigma == 2.0 and lm.end(np.ones(5), np.ones(5)) is None
    for bad in (0, 33):
        with pytest.raises(ValueError):
            LMHessian(5, bad)


def test_kkt_step_twin_with_the_operator_against_the_reference_with_the_matrix():
    """eqp.kkt_step_pcg(..., hess=lm.product) against eqp.kkt_step_reference(..., hess=lm.dense()) on hs071, at the bar and with the
    decisions test_kkt_step_cpu.py asks of that pair of functions."""
    fm, pr, x, lam = hs071_start()
    rs, bs = sensitivity.working_set(pr, x, lam, np.zeros(4), np.zeros(4), HS071_TOL)
    lm, _, _ = filled(4, 3, 3, seed=2, cond=10.0)
    ru = np.asarray(fm.eval_grad_f(x, np.zeros(4)), float)
    rw = np.where(rs == 1, np.asarray(pr.eval_g(x, np.zeros(2)), float) - np.where(np.isfinite(pr.g_L), pr.g_L, pr.g_U), 0.0)
    for radius in (0.25 * HS071_RADIUS, HS071_RADIUS, float("inf")):
        twin = eqp.kkt_step_pcg(fm, x, lam, rs, bs, ru, rw, radius, hess=lm.product)
        ref = eqp.kkt_step_reference(fm, x, lam, rs, bs, ru, rw, radius, hess=lm.dense())
        errs = step_errors(twin, ref)
        print("hs071 radius %g: boundary %d, %d iterations, errors %s" % (radius, twin[3]["boundary"], twin[3]["cg_iters"], " ".join("%.1e" % e for e in errs)))
        assert (twin[3]["boundary"], twin[3]["cg_iters"], twin[3]["status"]) == (ref[3]["boundary"], ref[3]["cg_iters"], ref[3]["status"])
        assert max(errs) <= KKT_STEP_BAR
    multi = eqp.kkt_step_pcg_multi(fm, x, lam, rs, bs, np.tile(ru, (2, 1)), np.tile(rw, (2, 1)), [HS071_RADIUS, 0.25 * HS071_RADIUS], hess=lm.product)
    one = eqp.kkt_step_pcg(fm, x, lam, rs, bs, ru, rw, HS071_RADIUS, hess=lm.dense())
    assert rel(multi[0][0], one[0]) <= KKT_STEP_BAR
    solve = sensitivity.kkt_pcg(fm, x, lam, rs, bs, ru, rw, hess=lm.product)
    assert rel(solve[0], eqp.kkt_step_pcg(fm, x, lam, rs, bs, ru, rw, float("inf"), hess=lm.product)[0]) == 0.0


def test_without_the_hook_nothing_changes():
    """hess=None is the call without the argument, bit for bit, and equals handing over the model's own Hessian."""
    from activesetmethods_amd.moi_evaluator import lagrangian_hessian
    fm, pr, x, lam = hs071_start()
    rs, bs = sensitivity.working_set(pr, x, lam, np.zeros(4), np.zeros(4), HS071_TOL)
    ru, rw = np.array([1.0, -2.0, 0.5, 0.25]), np.array([0.1, -0.2])
    H = lagrangian_hessian(fm, x, lam)
    for f, tail in ((eqp.kkt_step_pcg, (HS071_RADIUS,)), (eqp.kkt_step_reference, (HS071_RADIUS,)), (sensitivity.kkt_pcg, ())):
        plain, none, own = (f(fm, x, lam, rs, bs, ru, rw, *tail, **kw) for kw in ({}, dict(hess=None), dict(hess=H)))
        for got in (none, own):
            assert all(np.array_equal(a, b) for a, b in zip(got[:3], plain[:3])) and got[3] == plain[3]
    with pytest.raises(ValueError):
        eqp.kkt_step_pcg(fm, x, lam, rs, bs, ru, rw, 1.0, hess=np.eye(3))


def test_parameters():
    p = A.Parameters()
    assert p.hessian_type == "none" and p.lm_memory == 10
    for ok in ("none", "exact", "limited-memory"):
        assert A.Parameters(hessian_type=ok).hessian_type == ok
    for bad in (dict(hessian_type="other"), dict(lm_memory=0), dict(lm_memory=33)):
        with pytest.raises(ValueError):
            A.Parameters(**bad)


def test_the_batch_entries_refuse_the_limited_memory_type():
    par = A.Parameters(algorithm="SLP-EQP", device_eval=True, hessian_type="limited-memory")
    with pytest.raises(ValueError, match="per handle"):
        batch.check_batch_kkt_form(par)
    with pytest.raises(ValueError, match="per handle"):
        batch.HipBatch.slp_run(None, *([np.zeros((1, 1))] * 5), par)                     # refused before the batch is touched
    with pytest.raises(ValueError, match="per handle"):
        batch.solve_batch_lockstep([], par, 2)
    with pytest.raises(ValueError, match="per handle"):
        batch.solve_batch_dynamic(lambda i: None, 0, par, 2, None)
    batch.check_batch_kkt_form(A.Parameters(algorithm="SLP-EQP", hessian_type="exact"))


def lm_host_factory(fm, pr, ctx):
    """The oracle-backed LP of tests/test_slp_eqp_cpu.py with the twin behind the four entries SlpEQP calls in the limited-memory mode.
    The stand-in evaluates grad f - J' lam at the driver's x (ctx["slp"], set once the driver exists), as the device does from HBM."""
    class Opt(_OracleBackedSubOptimizer):
        def set_hessian_type(self, kind, memory=10):
            assert kind == "limited-memory"
            ctx["set"] = ctx.get("set", 0) + 1
            ctx["lm"] = LMHessian(fm.n, memory)

        def _grad_lag(self, lam):
            x = ctx["slp"].x
            return x, np.asarray(fm.eval_grad_f(x, np.zeros(fm.n)), float) - sensitivity.dense_jacobian(fm, x).T @ np.asarray(lam, float)

        def lm_begin(self, lam):
            assert not ctx["slp"].feasibility_restoration
            ctx["lm"].begin(*self._grad_lag(lam))

        def lm_end(self, lam):
            ctx["lm"].end(*self._grad_lag(lam))

        def eqp_trial(self, x, lam, lp_rows, lp_bnd, radius, nu, tol):
            return eqp.eqp_trial_host(fm, pr, x, lam, lp_rows, lp_bnd, radius, nu, tol, hess=ctx["lm"].product)
    return Opt


def lm_run(fm, name, **kw):
    pr = fm.to_problem(name)
    ctx = {}
    mdl = A.Model.from_problem(pr, A.Parameters(algorithm="SLP-EQP", hessian_type="limited-memory", external_optimizer=lm_host_factory(fm, pr, ctx), **kw))
    slp = ctx["slp"] = A.SlpEQP(mdl)
    slp.run()
    return mdl, slp, ctx


def test_slp_eqp_with_the_limited_memory_hessian_on_hs071():
    """Status 0 and the known optimum within the drivers' tolerances; the iteration counts beside the exact-Hessian and Trust-Region
    runs of the same start are printed ("Limited-memory Hessian"), not asserted."""
    fm = A.problems.hs071_function_model()
    mdl, slp, ctx = lm_run(fm, "hs071")
    c, info = slp.eqp_counts, ctx["lm"].info()
    exact, tr = eqp_run(fm, "SLP-EQP", "hs071")[1], eqp_run(fm, "Trust Region", "hs071")[1]
    print("hs071: limited-memory status %d iter %d lp %d %r %r | exact iter %d | Trust Region iter %d" % (slp.ret, slp.iter, slp.lp_solves, c, info, exact.iter, tr.iter))
    assert mdl.status == 0 and np.abs(mdl.x - HS071_X).max() <= 1e-5
    assert ctx["set"] == 1 and info["pairs"] > 0
    assert c["attempts"] == c["accepted"] + c["rejected"] + c["skipped_rows"] + c["skipped_dependent"] + c["skipped_zero"]


def test_slp_eqp_with_the_limited_memory_hessian_needs_no_second_derivatives():
    """The 14-bus grid with the hand-written Ohm's-law block (nlp_kind 1: no Hessian anywhere) runs SLP-EQP in this mode."""
    fm = acopf.function_model(acopf.synthetic_grid(14, 5, 20, 1, 0.5))
    mdl, slp, ctx = lm_run(fm, "grid14 ohm", max_iter=60)
    c = slp.eqp_counts
    print("grid14 (Ohm's-law block): status %d iter %d lp %d %r %r" % (slp.ret, slp.iter, slp.lp_solves, c, ctx["lm"].info()))
    assert c["attempts"] > 0 and ctx["lm"].info()["pushed"] > 0
    assert c["attempts"] == c["accepted"] + c["rejected"] + c["skipped_rows"] + c["skipped_dependent"] + c["skipped_zero"]
