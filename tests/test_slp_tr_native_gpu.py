"""The native Trust-Region SLP caller (include/asm_hip.h: asm_slp_step_quality, asm_slp_run_tr, asm_batch_slp_run_tr) against the host
driver SlpTR.run (activesetmethods_amd/slp.py, run!(::SlpTR) of slp_trust_region.jl:87-251) with Parameters(device_eval=True).

Both make the same library calls in the same order, so a native run equals the host driver's BIT FOR BIT: status, counts, iterates,
multipliers, radius, the solver paths of its LPs; and a scenario batch equals the per-handle runs bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TR = "Trust Region"


def _toy_function_model():
    """The toy NLP of test/ext_solver.jl:12-18 with its three nonlinear rows stated as quadratic functions."""
    from activesetmethods_amd.moi_evaluator import FunctionModel, ScalarFunction
    fm = FunctionModel(2)
    fm.objective = ScalarFunction(0.0, [(1.0, 1)], [(2.0, 1, 1)])                      # X^2 + X
    fm.add_constraint(ScalarFunction(0.0, [(1.0, 1)]), "ge", -2.0)                      # X >= -2
    fm.add_constraint(ScalarFunction(0.0, [(-1.0, 1)], [(2.0, 1, 1)]), "eq", 2.0)       # X^2 - X == 2
    fm.add_constraint(ScalarFunction(0.0, [], [(1.0, 1, 2)]), "eq", 1.0)                # X Y == 1
    fm.add_constraint(ScalarFunction(0.0, [], [(1.0, 1, 2)]), "ge", 0.0)                # X Y >= 0
    return fm


def _case118():
    from activesetmethods_amd import acopf
    return acopf.function_model(acopf.synthetic_case("case118", 1, 1.0)).to_problem("case118-sized")


def _case300():
    from activesetmethods_amd import acopf
    return acopf.function_model(acopf.synthetic_case("case300", 1, 0.5)).to_problem("case300-sized")


def _handle_for(pr):
    import activesetmethods_amd as A
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(pr.function_model)
    return opt


def _host_tr(pr, par, max_lp_solves=None):
    """SlpTR.run with a record of every step_quality: (rho, radius before, radius after, ret after)."""
    import activesetmethods_amd as A
    mdl = A.Model.from_problem(pr, par)
    slp = A.SlpTR(mdl)
    steps = []
    inner = slp.step_quality

    def recorded():
        d0 = slp.Delta
        rho = inner()
        steps.append((rho, d0, slp.Delta, slp.ret))
        return rho
    slp.step_quality = recorded
    slp.run(max_lp_solves)
    slp.optimizer.close()
    return mdl, slp, steps


def _native_tr(opt, pr, par, max_lp_solves=0, J=None):
    from activesetmethods_amd import _lib
    if J is not None:
        Jc = np.ascontiguousarray(J, np.int32)
        assert _lib.load().asm_sublp_set_ns_basis(opt._h, _lib.i32ptr(Jc), len(Jc)) == 0
    return opt.slp_run(pr.x0, par, max_lp_solves)


def _assert_same_run(run, mdl, slp, steps):
    assert run.ret == slp.ret and run.iter == slp.iter and run.lp_solves == slp.lp_solves and run.ls_trials == 0
    assert run.restoration_solves == sum(1 for r in slp.trace if r["fr"])
    for a, b in ((run.x, slp.x), (run.lam, slp.lam), (run.mult_x_U, slp.mult_x_U), (run.mult_x_L, slp.mult_x_L), (run.E, mdl.g)):
        assert np.array_equal(a, b)
    assert run.obj_val == mdl.obj_val
    assert (run.prim_infeas, run.dual_infeas, run.compl) == (slp.prim_infeas, slp.dual_infeas, slp.compl)
    hist = [0] * 12
    for r in slp.trace:
        hist[r["stats"]["path"]] += 1
    assert run.paths == hist
    assert run.delta == slp.Delta
    go = [s for s in steps if s[3] not in (0, 2, 6)]          # steps after which the loop went on
    assert run.accepted == sum(1 for s in go if s[0] >= 0) and run.rejected == sum(1 for s in go if not s[0] >= 0)
    assert run.shrunk == sum(1 for s in steps if s[2] < s[1]) and run.expanded == sum(1 for s in steps if s[2] > s[1])
    # the same accepted / rejected split from the trace: consecutive normal-phase LPs at a changed / unchanged x
    if run.restoration_solves == 0:
        moved = [not np.array_equal(a["x"], b["x"]) for a, b in zip(slp.trace, slp.trace[1:])]
        assert run.accepted == sum(moved) and run.rejected == len(moved) - sum(moved)


@pytest.mark.parametrize("phase", ["normal", "restoration"])
def test_step_quality_equals_three_merit_calls_bit_for_bit(phase):
    """asm_slp_step_quality (one upload, one launch for the three quantities, one read-back) against asm_slp_merit three times on the same
    device state: compute_derivative, compute_phi(x, 0, p), compute_phi(x, 1, p) - the same doubles."""
    import activesetmethods_amd as A
    from activesetmethods_amd import _lib
    fr = phase == "restoration"
    if not fr:
        pr, par = _case118(), A.Parameters(algorithm=TR, device_eval=True)
    else:
        pr, par = _case300(), A.Parameters(algorithm=TR, tr_size=0.05, device_eval=True)     # INFEASIBLE at x0, then the restoration LP
    slp = A.SlpTR(A.Model.from_problem(pr, par))
    slp.run(max_lp_solves=1)
    # LP by LP until the last one is an optimal LP of the wanted phase (the device holds its iterate: the step is never evaluated there)
    while not (slp.trace[-1]["status"] == _lib.OPTIMAL and slp.trace[-1]["fr"] == fr) and slp.lp_solves < 40:
        slp.run(max_lp_solves=slp.lp_solves + 1, resume=True)
    last = slp.trace[-1]
    assert last["status"] == _lib.OPTIMAL and last["fr"] == fr
    if fr:
        assert slp.trace[0]["status"] == _lib.INFEASIBLE
    opt = slp.optimizer
    p, ps = slp.p, slp.p_slack
    nu, prim = slp.nu, slp.prim_infeas
    assert np.isfinite(prim)
    got = opt.step_quality(p, nu, ps, fr, prim)
    want = (opt.slp_merit(1, 0.0, p, nu, ps, fr, prim), opt.slp_merit(0, 0.0, p, nu, ps, fr, prim), opt.slp_merit(0, 1.0, p, nu, ps, fr, prim))
    assert np.array_equal(np.array(got), np.array(want)), (got, want)
    # and again after the trial evaluation of the merit calls: nothing of the iterate was overwritten
    assert opt.step_quality(p, nu, ps, fr, prim) == got
    opt.close()


def _instances():
    import activesetmethods_amd as A
    from activesetmethods_amd import problems
    return {
        "toy": (lambda: _toy_function_model().to_problem("toy"), A.Parameters(algorithm=TR, device_eval=True)),
        "dense": (lambda: problems.synthetic_dense_function_model(200, 100).to_problem("dense"), A.Parameters(algorithm=TR, max_iter=100, device_eval=True)),
        "case118": (_case118, A.Parameters(algorithm=TR, max_iter=100, device_eval=True)),
        "case300-restoration": (_case300, A.Parameters(algorithm=TR, tr_size=0.05, max_iter=30, device_eval=True)),
    }


@pytest.mark.parametrize("name", ["toy", "dense", "case118", "case300-restoration"])
def test_native_trust_region_equals_the_host_driver(name):
    make, par = _instances()[name]
    pr = make()
    mdl, slp, steps = _host_tr(pr, par)
    opt = _handle_for(pr)
    run = _native_tr(opt, pr, par)
    opt.close()
    _assert_same_run(run, mdl, slp, steps)
    assert len(steps) > 0
    if name == "toy":
        assert run.ret == 0 and np.allclose(run.x, [-1.0, -1.0], rtol=1e-4)
    if name == "case300-restoration":
        assert run.restoration_solves > 0


def test_native_trust_region_lp_cap():
    """asm_slp_params.max_lp_solves = k: exactly k LPs, status -5, the iterate of SlpTR.run(max_lp_solves=k)."""
    import activesetmethods_amd as A
    pr = _case118()
    par = A.Parameters(algorithm=TR, max_iter=100, device_eval=True)
    for k in (1, 4):
        mdl, slp, steps = _host_tr(pr, par, max_lp_solves=k)
        opt = _handle_for(pr)
        run = _native_tr(opt, pr, par, max_lp_solves=k)
        opt.close()
        assert run.lp_solves == slp.lp_solves == k and run.ret == slp.ret == -5
        assert np.array_equal(run.x, slp.x) and run.delta == slp.Delta


def test_trust_region_batch_equals_per_scenario_runs_bit_for_bit():
    """Eight case300-sized scenarios through asm_batch_slp_run_tr with eight slots in two groups and with three slots (slots take the next
    scenario when they finish one), and through solve_batch_lockstep: every run equals the per-handle asm_slp_run_tr run from the batch's
    reference basis columns, the trust-region record included; launches are shared across the slots."""
    import activesetmethods_amd as A
    from activesetmethods_amd import acopf, batch
    base = acopf.synthetic_case("case300", 1, 0.5)
    prs = [acopf.function_model(acopf.scenario_case(base, s)).to_problem("case300-sized scenario %d" % s) for s in range(8)]
    par = A.Parameters(algorithm=TR, max_iter=40, device_eval=True)
    stack = lambda k: np.stack([getattr(p, k) for p in prs])
    hb = batch.HipBatch(prs[0], 8, groups=2)
    assert hb.groups == 2
    runs8 = hb.slp_run(stack("g_L"), stack("g_U"), stack("x_L"), stack("x_U"), stack("x0"), par)
    bst = hb.stats()
    J = hb.ns_basis()
    runs_ls, stats, _ = batch.solve_batch_lockstep(prs, par, 8, batch=hb)
    hb.close()
    assert len(J) > 0 and bst["launches"] < bst["ops"], bst
    assert stats["scenarios"] == 8
    hb3 = batch.HipBatch(prs[0], 3)
    hb3.set_ns_basis(J)
    runs3 = hb3.slp_run(stack("g_L"), stack("g_U"), stack("x_L"), stack("x_U"), stack("x0"), par)
    hb3.close()
    opt = _handle_for(prs[0])
    for s, pr in enumerate(prs):
        opt.set_bounds(A.QpData(None, 0.0, None, None, pr.g_L, pr.g_U, pr.x_L, pr.x_U))
        one = _native_tr(opt, pr, par, J=J)
        for r in (runs8[s], runs3[s], runs_ls[s]):
            assert r.ret == one.ret and r.iter == one.iter and r.lp_solves == one.lp_solves and r.paths == one.paths
            assert r.restoration_solves == one.restoration_solves
            assert np.array_equal(r.x, one.x) and np.array_equal(r.lam, one.lam) and np.array_equal(r.E, one.E)
            assert np.array_equal(r.mult_x_U, one.mult_x_U) and np.array_equal(r.mult_x_L, one.mult_x_L)
            assert r.obj_val == one.obj_val
            assert (r.delta, r.accepted, r.rejected, r.shrunk, r.expanded) == (one.delta, one.accepted, one.rejected, one.shrunk, one.expanded)
    opt.close()


def test_trust_region_argument_errors_leave_the_handle_usable():
    """tr_size 0, -1, NaN: ASM_ERR_ARG (handle and batch); asm_slp_run_tr before asm_eval_setup: ASM_ERR_STATE; then the handle solves."""
    import activesetmethods_amd as A
    from activesetmethods_amd import _lib, batch
    lib = _lib.load()
    pr = _toy_function_model().to_problem("toy")
    par = A.Parameters(algorithm=TR, device_eval=True)
    sp = batch.slp_params(par)
    x0 = np.ascontiguousarray(pr.x0, np.float64)
    x = np.empty(pr.n); lam = np.empty(pr.m); mU = np.empty(pr.n); mL = np.empty(pr.n); g = np.empty(pr.m)
    res, tr = _lib.SlpResult(), _lib.SlpTrInfo()
    call = lambda o, d: lib.asm_slp_run_tr(o._h, C.byref(sp), d, _lib.dptr(x0), _lib.dptr(x), _lib.dptr(lam), _lib.dptr(mU), _lib.dptr(mL), _lib.dptr(g),
                                           C.byref(res), C.byref(tr))
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    assert call(opt, 0.4) == -3                               # ASM_ERR_STATE: no evaluator
    opt.eval_setup(pr.function_model)
    for d in (0.0, -1.0, float("nan"), float("inf")):
        assert call(opt, d) == -1, d                          # ASM_ERR_ARG
    run = opt.slp_run(pr.x0, par)
    assert run.ret == 0 and np.allclose(run.x, [-1.0, -1.0], rtol=1e-4)
    opt.close()
    hb = batch.HipBatch(pr, 2)
    f64 = lambda a: np.ascontiguousarray(np.stack([a, a]), np.float64)
    gl, gu, xl, xu, xs = map(f64, (pr.g_L, pr.g_U, pr.x_L, pr.x_U, pr.x0))
    X = np.empty((2, pr.n)); L = np.empty((2, pr.m)); U = np.empty((2, pr.n)); W = np.empty((2, pr.n)); G = np.empty((2, pr.m))
    R = (_lib.SlpResult * 2)()
    for d in (0.0, -1.0, float("nan")):
        rc = lib.asm_batch_slp_run_tr(hb._b, 2, _lib.dptr(gl), _lib.dptr(gu), _lib.dptr(xl), _lib.dptr(xu), _lib.dptr(xs), C.byref(sp), d, _lib.dptr(X),
                                      _lib.dptr(L), _lib.dptr(U), _lib.dptr(W), _lib.dptr(G), R, None)
        assert rc == -1, d
    runs = hb.slp_run(gl, gu, xl, xu, xs, par)
    hb.close()
    assert all(r.ret == 0 and np.allclose(r.x, [-1.0, -1.0], rtol=1e-4) for r in runs)


@pytest.mark.parametrize("alg", ["Line Search", TR])
def test_native_optimize_fills_the_model_as_the_host_driver(alg):
    """optimize(model, native=True) leaves the model as optimize(model) with device_eval=True does."""
    import activesetmethods_amd as A
    from activesetmethods_amd import batch
    models = []
    for native in (False, True):
        mdl = A.Model.from_problem(_toy_function_model().to_problem("toy"), A.Parameters(algorithm=alg, device_eval=True))
        out = A.optimize(mdl, native=native)
        if not native:
            out.optimizer.close()
        models.append((mdl, out))
    (mh, sh), (mn, rn) = models
    assert isinstance(rn, batch.NativeRun) and (rn.delta is None) == (alg != TR)
    assert mn.status == mh.status == 0 and mn.obj_val == mh.obj_val
    for k in ("x", "g", "mult_g", "mult_x_U", "mult_x_L"):
        assert np.array_equal(getattr(mn, k), getattr(mh, k)), k
    assert mn.statistics["iter"] == mh.statistics["iter"] and mn.statistics["lp_solves"] == mh.statistics["lp_solves"]
