"""NLP-block data on the device (include/asm_hip.h: asm_eval_set_data, asm_eval_data_gradient, asm_batch_set_scenario_data,
asm_batch_data_gradient): new data without a new set-up is bit-identical to a fresh set-up, the data gradient kernels equal their host
twin (nlexpr.py: ExprBlock.data_gradient), and per-scenario data in a batch equals per-handle runs bit for bit."""
import ctypes as C

import numpy as np
import pytest

from activesetmethods_amd import acopf, problems
from tests.test_nlparams_cpu import random_param_block

pytestmark = pytest.mark.gpu
LS, TR = "Line Search", "Trust Region"
ERR_ARG, ERR_STATE = -1, -3


def _handle_for(pr, fm=None):
    import activesetmethods_amd as A
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(fm if fm is not None else pr.function_model)
    return opt


def _run(opt, pr, par, J=None, max_lp_solves=0):
    """asm_slp_run / asm_slp_run_tr on one handle from the basis columns J (None: selected by the run's first LP)."""
    from activesetmethods_amd import _lib
    if J is not None:
        Jc = np.ascontiguousarray(J, np.int32)
        assert _lib.load().asm_sublp_set_ns_basis(opt._h, _lib.i32ptr(Jc), len(Jc)) == 0
    return opt.slp_run(pr.x0, par, max_lp_solves)


def _same_run(r, one):
    assert r.ret == one.ret and r.iter == one.iter and r.lp_solves == one.lp_solves and r.paths == one.paths
    assert r.restoration_solves == one.restoration_solves
    assert np.array_equal(r.x, one.x) and np.array_equal(r.lam, one.lam) and np.array_equal(r.E, one.E)
    assert np.array_equal(r.mult_x_U, one.mult_x_U) and np.array_equal(r.mult_x_L, one.mult_x_L)
    assert r.obj_val == one.obj_val
    assert (r.delta, r.accepted, r.rejected, r.shrunk, r.expanded) == (one.delta, one.accepted, one.rejected, one.shrunk, one.expanded)


def _evals(opt, xs):
    out = []
    for x in xs:
        f, df, E = opt.eval_functions(x)
        ft, Et = opt.eval_constraints(0.5 * x + 0.25)
        out.append((f, df, E, opt.jacobian_values(), ft, Et))
    return out


def _kind_pair(kind):
    """(function model A, function model B with other data, the dpar of B, SLP parameters) for NLP kind 1, 2 or 3."""
    import activesetmethods_amd as A
    if kind == 1:
        base = acopf.synthetic_case("case118", 1, 0.5)
        fa, fb = acopf.function_model(base), acopf.function_model(acopf.line_scenario_case(base, 3))
        par = A.Parameters(algorithm=LS, max_iter=60, device_eval=True)
    elif kind == 2:
        fa = problems.synthetic_dense_function_model(200, 80)
        fb = problems.synthetic_dense_function_model(200, 80)
        _, ipar, dpar = fb.nlp.device
        rng = np.random.default_rng(4)
        fb.nlp.device = ("dense_quadratic", ipar, dpar * (1.0 + 0.05 * rng.uniform(-1, 1, len(dpar))))
        par = A.Parameters(algorithm=LS, max_iter=60, device_eval=True)
    else:
        fa, fb = problems.parametric_function_model(0.5, 4.0), problems.parametric_function_model(0.7, 5.0)
        par = A.Parameters(algorithm=LS, max_iter=60, device_eval=True)
    return fa, fb, np.asarray(fb.nlp.device[2], np.float64), par


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_set_data_equals_a_fresh_setup(kind):
    """asm_eval_set_data with B's dpar on a handle set up with A's: asm_eval_functions, the Jacobian values, asm_eval_constraints and one
    asm_slp_run (same basis columns) equal those of a handle set up with B, bit for bit; the pattern never changes."""
    fa, fb, dpar_b, par = _kind_pair(kind)
    pa, pb = fa.to_problem("A"), fb.to_problem("B")
    assert pa.j_str == pb.j_str
    import activesetmethods_amd as A
    oa, ob = _handle_for(pa, fa), _handle_for(pb, fb)
    oa.set_eval_data(dpar_b)
    cap = 6 if kind == 2 else 0
    _run(ob, pb, par, max_lp_solves=cap)                  # basis columns for both runs
    J = ob.ns_basis()
    runs = []
    for o in (oa, ob):
        o.set_bounds(A.QpData(None, 0.0, None, None, pb.g_L, pb.g_U, pb.x_L, pb.x_U))      # drops the retained active sets
        runs.append(_run(o, pb, par, J=J if len(J) else None, max_lp_solves=cap))
    run_a, run_b = runs
    _same_run(run_a, run_b)
    assert kind == 2 or run_b.ret == 0
    rng = np.random.default_rng(kind)
    xs = [pb.x0, pb.x0 + 0.01 * rng.standard_normal(pb.n), run_b.x]
    for ea, eb in zip(_evals(oa, xs), _evals(ob, xs)):
        assert ea[0] == eb[0] and ea[4] == eb[4]
        assert all(np.array_equal(u, v) for u, v in zip(ea[1:4] + ea[5:], eb[1:4] + eb[5:]))
    # a partial write: only the given range changes
    if kind == 3:
        oa.set_eval_data([0.5], 0)                 # back to a = 0.5, p stays 5.0
        fc = problems.parametric_function_model(0.5, 5.0)
        oc = _handle_for(fc.to_problem(), fc)
        for ea, ec in zip(_evals(oa, xs), _evals(oc, xs)):
            assert ea[0] == ec[0] and all(np.array_equal(u, v) for u, v in zip(ea[1:4], ec[1:4]))
        oc.close()
    oa.close()
    ob.close()


def test_argument_and_state_errors():
    from activesetmethods_amd import _lib, batch
    lib = _lib.load()
    fm = problems.parametric_function_model()
    pr = fm.to_problem()
    import activesetmethods_amd as A
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    v = np.ones(4)
    x, lam, out = np.ones(2), np.ones(2), np.zeros(4)
    assert lib.asm_eval_set_data(opt._h, 0, 1, _lib.dptr(v)) == ERR_STATE                      # before asm_eval_setup
    assert lib.asm_eval_data_gradient(opt._h, _lib.dptr(x), _lib.dptr(lam), _lib.dptr(out)) == ERR_STATE
    opt.eval_setup(fm)
    f0 = opt.eval_functions(pr.x0)
    for off, cnt in ((-1, 1), (0, 3), (2, 1), (1, 2), (0, -1)):
        assert lib.asm_eval_set_data(opt._h, off, cnt, _lib.dptr(v)) == ERR_ARG, (off, cnt)
    assert lib.asm_eval_set_data(opt._h, 0, 1, None) == ERR_ARG
    assert lib.asm_eval_data_gradient(opt._h, None, _lib.dptr(lam), _lib.dptr(out)) == ERR_ARG
    f1 = opt.eval_functions(pr.x0)                                                              # nothing changed
    assert f0[0] == f1[0] and np.array_equal(f0[1], f1[1]) and np.array_equal(f0[2], f1[2])
    opt.close()
    fk = acopf.function_model(acopf.synthetic_case("case118", 1, 0.5))
    pk = fk.to_problem()
    ok = _handle_for(pk, fk)
    with pytest.raises(A.AsmHipError, match="expression blocks"):
        ok.eval_data_gradient(pk.x0, np.zeros(pk.m))
    ok.close()
    hb = batch.HipBatch(pr, 2)
    t = np.ones((3, 2))
    assert lib.asm_batch_set_scenario_data(hb._b, 3, 1, 2, _lib.dptr(t)) == ERR_ARG             # range outside dpar
    assert lib.asm_batch_set_scenario_data(hb._b, 3, 0, 2, None) == ERR_ARG
    hb.set_scenario_data(t)                                                                     # 3 scenarios
    st = lambda k: np.stack([getattr(pr, k)] * 2)
    with pytest.raises(A.AsmHipError):
        hb.data_gradient(st("x0"), np.zeros((2, 2)))                                            # 2 scenarios against a table of 3
    r = lib.asm_batch_slp_run(hb._b, 2, *(_lib.dptr(st(k)) for k in ("g_L", "g_U", "x_L", "x_U", "x0")),
                              C.byref(batch.slp_params(A.Parameters(algorithm=LS))), None, None, None, None, None,
                              (_lib.SlpResult * 2)())
    assert r == ERR_ARG
    with pytest.raises(ValueError):
        hb.scenario_data([problems.hs071_problem()])                                            # another tape: not a data scenario
    hb.close()


@pytest.mark.parametrize("exact", [True, False])
def test_device_data_gradient_equals_the_host_twin(exact):
    """Random parameterised blocks under both senses: bit for bit with + - * / abs min max, 1e-12 relative with the math library;
    after asm_eval_set_data the device gradient follows the host twin's set_parameter_values."""
    from tests.test_nlexpr_cpu import _model
    for seed in range(3):
        v = np.random.default_rng(seed).uniform(-1.5, 1.5, 3)
        blk, n = random_param_block(seed, v, exact=exact)
        for sense in ("MIN_SENSE", "MAX_SENSE"):
            fm = _model(blk, n, sense)
            pr = fm.to_problem()
            opt = _handle_for(pr, fm)
            rng = np.random.default_rng(seed + 17)
            nr = pr.m - blk.m
            for step in range(3):
                if step == 2:
                    w = v + 0.3
                    opt.set_eval_data(w)
                    blk.set_parameter_values(w)
                x, lam = rng.uniform(-1, 1, n), rng.standard_normal(pr.m)
                got = opt.eval_data_gradient(x, lam)
                want = blk.data_gradient(x, lam[nr:], fm.objective_scale)
                assert got.shape == want.shape == (len(blk.device[2]),)
                if exact:
                    assert np.array_equal(got, want), (seed, sense, step)
                else:
                    assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))), (seed, sense, step)
            blk.set_parameter_values(v)
            opt.close()


def test_data_gradient_at_the_native_solution_and_on_the_expression_acopf():
    """At the native SLP solution of the parameterised model the data gradient is dV/d(a, p) of the closed form; on the expression ACOPF
    with branch parameters the device gradient equals the host twin to 1e-12 relative."""
    import activesetmethods_amd as A
    fm = problems.parametric_function_model(0.5, 4.0)
    pr = fm.to_problem()
    opt = _handle_for(pr, fm)
    par = A.Parameters(algorithm=LS, max_iter=60, device_eval=True, tol_direction=1e-12, tol_residual=1e-10, tol_infeas=1e-12)
    run = opt.slp_run(pr.x0, par)
    xs, V, dV = problems.parametric_solution(0.5, 4.0)
    assert run.ret == 0 and np.allclose(run.x, xs, rtol=1e-9)
    assert np.allclose(opt.eval_data_gradient(run.x, run.lam), dV, rtol=1e-8)
    opt.close()
    c = acopf.line_scenario_case(acopf.synthetic_case("case118", 1, 0.5), 2)
    fe = acopf.function_model(c, nlp="expr", branch_params=True)
    pe = fe.to_problem()
    oe = _handle_for(pe, fe)
    rng = np.random.default_rng(8)
    x = pe.x0 + 0.05 * rng.standard_normal(pe.n)
    lam = rng.standard_normal(pe.m)
    got = oe.eval_data_gradient(x, lam)
    want = fe.nlp.data_gradient(x, lam[pe.m - fe.nlp.m:], fe.objective_scale)
    assert np.all((got == want) | (np.abs(got - want) <= 1e-12 * np.abs(want)))
    oe.close()


def _line_problems(nlp, n=8):
    base = acopf.synthetic_case("case300", 1, 0.5)
    kw = dict(nlp="expr", branch_params=True) if nlp == "expr" else {}
    return [acopf.function_model(acopf.line_scenario_case(base, s), **kw).to_problem("case300-sized line scenario %d" % s) for s in range(n)]


@pytest.mark.parametrize("alg", [LS, TR])
@pytest.mark.parametrize("nlp", ["acopf_ohm", "expr"])
def test_line_scenario_batch_equals_per_handle_runs(nlp, alg):
    """Eight case300-sized line scenarios (branch admittances differ, one tape) through solve_batch_lockstep - the scenario data table - with
    eight slots in two groups and with three slots (refill): every run equals asm_eval_set_data + the per-handle run from the batch's basis
    columns, bit for bit; with Line Search all converge (Trust Region, like the load-scenario batch, runs into its iteration cap on these
    grids, so only the equality is pinned).  The batch data gradient equals the per-handle one."""
    import activesetmethods_amd as A
    from activesetmethods_amd import batch
    prs = _line_problems(nlp)
    dpars = [np.asarray(p.function_model.nlp.device[2], np.float64) for p in prs]
    assert not np.array_equal(dpars[0], dpars[1])
    par = A.Parameters(algorithm=alg, max_iter=100 if alg == LS else 40, device_eval=True)
    hb = batch.HipBatch(prs[0], 8, groups=2)
    assert hb.groups == 2
    runs8, stats, bst = batch.solve_batch_lockstep(prs, par, 8, batch=hb)
    J = hb.ns_basis()
    assert stats["scenarios"] == 8 and (alg == TR or stats["converged"] == 8), [r.ret for r in runs8]
    assert len(J) > 0 and bst["launches"] < bst["ops"], bst
    if nlp == "expr":
        X = np.stack([r.x for r in runs8])
        L = np.stack([r.lam for r in runs8])
        G = hb.data_gradient(X, L)
    hb.close()
    hb3 = batch.HipBatch(prs[0], 3)
    hb3.set_ns_basis(J)
    runs3, _, _ = batch.solve_batch_lockstep(prs, par, 3, batch=hb3)
    hb3.close()
    opt = _handle_for(prs[0])
    for s, pr in enumerate(prs):
        opt.set_bounds(A.QpData(None, 0.0, None, None, pr.g_L, pr.g_U, pr.x_L, pr.x_U))
        opt.set_eval_data(dpars[s])
        one = _run(opt, pr, par, J=J)
        assert alg == TR or one.ret == 0
        for r in (runs8[s], runs3[s]):
            _same_run(r, one)
        if nlp == "expr":
            assert np.array_equal(G[s], opt.eval_data_gradient(runs8[s].x, runs8[s].lam))
    opt.close()


def test_table_then_no_table_restores_the_setup_data():
    """Scenarios of the parameterised model with their own (a, p) through the table, then the same batch without one: the second call
    equals a batch that never had a table (slots that solved table scenarios restore the setup data); batch data gradients equal the
    per-handle ones bit for bit in both states."""
    import activesetmethods_amd as A
    from activesetmethods_amd import batch
    par = A.Parameters(algorithm=TR, max_iter=60, device_eval=True)
    vals = [(0.5, 4.0), (0.6, 4.5), (0.3, 3.0), (0.7, 6.0), (0.45, 5.5)]
    prs = [problems.parametric_function_model(a, p).to_problem("parametric %d" % s) for s, (a, p) in enumerate(vals)]
    stack = lambda k, ps=prs: np.stack([getattr(p, k) for p in ps])
    hb = batch.HipBatch(prs[0], 2)
    data = hb.scenario_data(prs)
    assert data.shape == (5, 2) and np.array_equal(data, np.asarray(vals))
    runs_t = hb.slp_run(stack("g_L"), stack("g_U"), stack("x_L"), stack("x_U"), stack("x0"), par, data=data)
    Gt = hb.data_gradient(np.stack([r.x for r in runs_t]), np.stack([r.lam for r in runs_t]))
    for s, (a, p) in enumerate(vals):
        xs, V, dV = problems.parametric_solution(a, p)
        assert runs_t[s].ret == 0 and np.allclose(runs_t[s].x, xs, rtol=1e-5), (s, runs_t[s].x)
        assert np.allclose(Gt[s], dV, rtol=1e-4), (s, Gt[s], dV)
    plain = [prs[0]] * 5
    runs_0 = hb.slp_run(stack("g_L", plain), stack("g_U", plain), stack("x_L", plain), stack("x_U", plain), stack("x0", plain), par)
    G0 = hb.data_gradient(np.stack([r.x for r in runs_t]), np.stack([r.lam for r in runs_t]))
    J = hb.ns_basis()
    hb.close()
    fresh = batch.HipBatch(prs[0], 2)
    if len(J):
        fresh.set_ns_basis(J)
    runs_f = fresh.slp_run(stack("g_L", plain), stack("g_U", plain), stack("x_L", plain), stack("x_U", plain), stack("x0", plain), par)
    fresh.close()
    for r, f in zip(runs_0, runs_f):
        _same_run(r, f)
    opt = _handle_for(prs[0])
    for s, r in enumerate(runs_t):
        opt.set_eval_data(data[s])
        assert np.array_equal(Gt[s], opt.eval_data_gradient(r.x, r.lam))
    opt.set_eval_data(data[0])
    for s, r in enumerate(runs_t):
        assert np.array_equal(G0[s], opt.eval_data_gradient(r.x, r.lam))
    opt.close()
