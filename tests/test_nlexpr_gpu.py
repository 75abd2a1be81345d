"""Expression NLP blocks on the device (nlp_kind 3 of include/asm_hip.h, the k_nlp_expr_* kernels of csrc/asm_eval_kernels.hip.h)
against their host twin (activesetmethods_amd/nlexpr.py), the hand-written ACOPF kernel, the Python drivers, the CPU oracle and
the per-handle runs of a scenario batch."""
import numpy as np
import pytest

from activesetmethods_amd import acopf, nlexpr, problems
from tests.test_nlexpr_cpu import HS071_ORACLE_STATUS, HS071_ORACLE_X, _model, random_expr_block
from tests.util import rel_err

pytestmark = pytest.mark.gpu


def _handle_for(pr, fm=None):
    import activesetmethods_amd as A
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(fm if fm is not None else pr.function_model)
    return opt


def _close(a, b, tol):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))


@pytest.mark.parametrize("sense", ["MIN_SENSE", "MAX_SENSE", "FEASIBILITY_SENSE"])
@pytest.mark.parametrize("smooth", [False, True])
def test_device_equals_host_twin(sense, smooth):
    """f, grad f, g and the Jacobian values at several points, and asm_eval_constraints: bit for bit with + - * / unary - and
    integer powers; within 1e-13 relative once sqrt / exp / log / sin / cos enter (device math library against NumPy's).  The
    block's objective overrides the store's (3 + x1) and carries the sense scale."""
    for seed in range(3):
        block, n = random_expr_block(seed + (10 if smooth else 0), smooth=smooth)
        fm = _model(block, n, sense)
        pr = fm.to_problem()
        opt = _handle_for(pr, fm)
        rng = np.random.default_rng(seed + 40)
        for _ in range(3):
            x = rng.uniform(-1.0, 1.0, n)
            f, df, E = opt.eval_functions(x)
            want = (pr.eval_f(x), pr.eval_grad_f(x, np.zeros(n)), pr.eval_g(x, np.zeros(pr.m)), pr.eval_jac_g(x, np.zeros(pr.nnz)))
            got = (f, df, E, opt.jacobian_values())
            ft, Et = opt.eval_constraints(0.5 * x)
            want_t = (pr.eval_f(0.5 * x), pr.eval_g(0.5 * x, np.zeros(pr.m)))
            if smooth:
                assert all(_close(g, w, 1e-13) for g, w in zip(got, want))
                assert _close(ft, want_t[0], 1e-13) and _close(Et, want_t[1], 1e-13)
            else:
                assert f == want[0] and all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:]))
                assert ft == want_t[0] and np.array_equal(Et, want_t[1])
            scale = fm.objective_scale
            assert _close(f, scale * block.eval_f(x), 1e-13) and (scale == 0.0 or f != scale * (3.0 + x[0]))
        opt.close()


def _ls_state(pr):
    import activesetmethods_amd as A
    mdl = A.Model.from_problem(pr, A.Parameters(algorithm="Line Search", max_iter=50, device_eval=True))
    slp = A.SlpLS(mdl)
    slp.run(max_lp_solves=2)
    slp.eval_functions()
    return slp


@pytest.mark.parametrize("fr", [False, True])
def test_device_line_search_equals_trial_by_trial_merit(fr):
    """asm_slp_line_search evaluates eight trial points per set of launches (trial index in the grid of the expression kernels, the
    objective from the terms of each trial): same alpha, merit value and trial count as one asm_slp_merit call per trial."""
    pr = problems.hs071_problem()
    slp = _ls_state(pr)
    opt = slp.optimizer
    rng = np.random.default_rng(12)
    nu = np.abs(rng.standard_normal(pr.m)) + 0.1
    ps = np.abs(rng.standard_normal(2 * pr.m))
    both = (pr.g_L > -np.inf) & (pr.g_U < np.inf)
    ps[1::2][~both] = np.nan
    S = type("S", (), {"raw": ps})()
    prim, eta, tau, min_alpha = 0.37, 0.4, 0.7, 1e-6
    for scale, dd in ((1e-3, -1.0), (0.3, -5.0), (3.0, -50.0), (3.0, -1e9), (0.5, 1e3)):
        p = scale * rng.standard_normal(pr.n)
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
        assert got[3] == ok and got[0] == alpha and got[2] == trials and got[1] == phi_a, (scale, dd, got, alpha, phi_a, trials, ok)
    opt.close()


def _with_ipar(fm, ipar, dpar=None):
    from activesetmethods_amd.moi_evaluator import NlpBlock
    b = fm.nlp
    bad = NlpBlock(b.g_L, b.g_U, b.rows, b.cols, b.eval_g, b.eval_jac_g, device=("expr", np.asarray(ipar, np.int64),
                   b.device[2] if dpar is None else dpar), has_objective=b.has_objective, eval_f=b.eval_f, eval_grad_f=b.eval_grad_f)
    fm2 = problems.hs071_function_model()
    fm2.nlp = bad
    return fm2


def test_eval_setup_rejects_malformed_tapes_and_keeps_the_handle():
    """Each malformed tape returns ASM_ERR_ARG with a message, from asm_eval_setup and from asm_batch_eval_setup (whose message names the
    slot); the handle keeps its evaluator and a valid tape is accepted after.  asm_eval_functions: ASM_ERR_ARG for a null x, ASM_ERR_STATE
    before asm_eval_setup."""
    import copy
    import ctypes as C
    import activesetmethods_amd as A
    from activesetmethods_amd import AsmHipError, _lib, batch
    lib = _lib.load()
    fm = problems.hs071_function_model()
    pr = fm.to_problem()
    opt = _handle_for(pr)
    x = np.array([1.5, 4.0, 3.5, 1.2])
    before = opt.eval_functions(x)
    R, T, L, ptr, op, a, b = (np.array(v) if hasattr(v, "__len__") else v for v in nlexpr.parse_ipar(fm.nlp.device[1]))
    k_mul = int(np.nonzero(op == nlexpr.MUL)[0][0])            # row 0: x1 * x2 ... (node 2)
    k_pow = int(np.nonzero(op == nlexpr.POWI)[0][0])
    k_var = int(np.nonzero(op == nlexpr.VAR)[0][0])

    def tape(**ch):
        o, aa, bb, pp = op.copy(), a.copy(), b.copy(), ptr.copy()
        for (arr, k, v) in ch.get("set", []):
            {"op": o, "a": aa, "b": bb, "ptr": pp}[arr][k] = v
        return np.concatenate([[R, T, L], pp, o, aa, bb])
    cases = {
        "forward reference": tape(set=[("b", k_mul, 2)]),
        "out-of-row reference": tape(set=[("a", k_mul, -1)]),
        "unknown op": tape(set=[("op", k_mul, nlexpr.OP_COUNT)]),
        "variable out of range": tape(set=[("a", k_var, pr.n)]),
        "POWI exponent 0": tape(set=[("b", k_pow, 0)]),
        "POWI exponent 65": tape(set=[("b", k_pow, 65)]),
        "constant out of range": tape(set=[("op", k_var, nlexpr.CONST), ("a", k_var, 99)]),
        "size mismatch": tape()[:-1],
        "row count": np.concatenate([[R + 1], tape()[1:]]),
        "pattern size": tape(set=[("a", k_var, 3)]),     # row 0 would use x4 twice and lose x1: 3 entries for 4
        "empty row": tape(set=[("ptr", 1, 0)]),
    }
    for name, ip in cases.items():
        with pytest.raises(AsmHipError, match="error -1") as ei:
            opt.eval_setup(_with_ipar(fm, ip))
        assert "expression block" in str(ei.value) or "ipar" in str(ei.value), (name, str(ei.value))
        bad_pr = copy.copy(pr)
        bad_pr.function_model = _with_ipar(fm, ip)
        with pytest.raises(AsmHipError, match=r"batch error -1: asm_eval_setup \(slot 0\): ") as eb:
            batch.HipBatch(bad_pr, 2)
        assert "expression block" in str(eb.value) or "ipar" in str(eb.value), (name, str(eb.value))
        after = opt.eval_functions(x)
        assert after[0] == before[0] and all(np.array_equal(u, v) for u, v in zip(after[1:], before[1:])), name
    opt.eval_setup(_with_ipar(fm, tape()))
    again = opt.eval_functions(x)
    assert again[0] == before[0] and np.array_equal(again[1], before[1]) and np.array_equal(again[2], before[2])
    f, df, E = C.c_double(0.0), np.zeros(pr.n), np.zeros(pr.m)
    xc = np.ascontiguousarray(x)
    assert lib.asm_eval_functions(opt._h, None, C.byref(f), _lib.dptr(df), _lib.dptr(E)) == -1        # ASM_ERR_ARG: null x
    opt.close()
    fresh = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    assert lib.asm_eval_functions(fresh._h, _lib.dptr(xc), C.byref(f), _lib.dptr(df), _lib.dptr(E)) == -3   # ASM_ERR_STATE: no evaluator
    fresh.close()
    # the same entries as the tape's pattern, in another order: not the pattern of a sorted row
    jc = pr.j_col.copy()
    jc[[0, 1]] = jc[[1, 0]]
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, jc)
    with pytest.raises(AsmHipError, match="error -1.*differs from the pattern"):
        opt.eval_setup(fm)
    opt.close()


def _python_and_native(pr, alg):
    import activesetmethods_amd as A
    mh = A.Model.from_problem(pr, A.Parameters(algorithm=alg, device_eval=True))
    sh = A.optimize(mh)
    sh.optimizer.close()
    mn = A.Model.from_problem(pr, A.Parameters(algorithm=alg, device_eval=True))
    rn = A.optimize(mn, native=True)
    return mh, mn, rn


def _assert_same(mh, mn):
    assert mn.status == mh.status and mn.obj_val == mh.obj_val
    for k in ("x", "g", "mult_g", "mult_x_U", "mult_x_L"):
        assert np.array_equal(getattr(mn, k), getattr(mh, k)), k
    assert mn.statistics["iter"] == mh.statistics["iter"] and mn.statistics["lp_solves"] == mh.statistics["lp_solves"]


@pytest.mark.parametrize("alg", ["Line Search", "Trust Region"])
def test_toy_as_expressions_native_reaches_the_known_answer(alg):
    """examples/toy_example.jl as written (three @NLconstraint rows as a tape): the native driver reaches X = Y = -1 with status 0
    and equals the Python driver with device evaluation bit for bit."""
    mh, mn, _ = _python_and_native(problems.toy_expr_problem(), alg)
    assert mn.status == 0 and np.allclose(mn.x, [-1.0, -1.0], rtol=1e-4)
    _assert_same(mh, mn)


def test_hs071_native_equals_python_driver_and_oracle():
    """HS071 (expression objective and constraints), Trust Region: native = Python driver bit for bit; status and x as the CPU
    oracle's run (tests/test_nlexpr_cpu.py pins it) to 1e-6."""
    mh, mn, _ = _python_and_native(problems.hs071_problem(), "Trust Region")
    _assert_same(mh, mn)
    assert mn.status == HS071_ORACLE_STATUS
    assert np.all(np.abs(mn.x - HS071_ORACLE_X) <= 1e-6), mn.x


def test_acopf_expression_block_matches_the_ohm_kernel():
    """case118: the expression rows on the device within 1e-13 of the hand-written Ohm's-law kernel (Jacobian entries matched
    by (row, col)); f and grad f (the store's objective) identical."""
    case = acopf.synthetic_case("case118", 2)
    pe = acopf.function_model(case, nlp="expr").to_problem("case118 expr")
    po = acopf.function_model(case).to_problem("case118 ohm")
    oe, oo = _handle_for(pe), _handle_for(po)
    rng = np.random.default_rng(9)
    for x in (pe.x0, pe.x0 + 0.02 * rng.standard_normal(pe.n)):
        fe, dfe, Ee = oe.eval_functions(x)
        fo, dfo, Eo = oo.eval_functions(x)
        assert fe == fo and np.array_equal(dfe, dfo)
        assert _close(Ee, Eo, 1e-13)
        de = dict(zip(zip(pe.j_row.tolist(), pe.j_col.tolist()), oe.jacobian_values()))
        do = dict(zip(zip(po.j_row.tolist(), po.j_col.tolist()), oo.jacobian_values()))
        assert de.keys() == do.keys() and all(abs(de[k] - do[k]) <= 1e-13 * max(1.0, abs(do[k])) for k in do)
    oe.close()
    oo.close()


def test_acopf_expression_slp_run_follows_the_ohm_kernel_run():
    """case118, Line Search, 15 iterations with device evaluation: the expression block's run follows the Ohm's-law kernel's
    (same LP statuses and phases, steps within 1e-8), the bar of test_acopf_slp_run_device_evaluation_matches_host_evaluation."""
    import activesetmethods_amd as A
    case = acopf.synthetic_case("case118", 1)
    runs = []
    for nlp in ("expr", "acopf_ohm"):
        pr = acopf.function_model(case, nlp=nlp).to_problem("case118")
        m = A.Model.from_problem(pr, A.Parameters(algorithm="Line Search", max_iter=15, device_eval=True))
        s = A.optimize(m)
        s.optimizer.close()
        runs.append((m, s))
    (me, se), (mo, so) = runs
    assert len(se.trace) == len(so.trace)
    for a, b in zip(se.trace, so.trace):
        assert a["status"] == b["status"] and a["fr"] == b["fr"]
        assert rel_err(a["p"], b["p"]) < 1e-8
    assert rel_err(me.x, mo.x) < 1e-8


def test_expression_batch_equals_per_scenario_runs_bit_for_bit():
    """Eight case300-sized scenarios with the Ohm's-law rows as expressions through asm_batch_slp_run (8 slots in 2 groups, and 3
    slots) equal asm_slp_run per scenario on one handle bit for bit; all converge."""
    import activesetmethods_amd as A
    from activesetmethods_amd import batch
    from tests.test_batch_gpu import _native_run
    base = acopf.synthetic_case("case300", 1, 0.5)
    prs = [acopf.function_model(acopf.scenario_case(base, s), nlp="expr").to_problem("case300-sized expr %d" % s) for s in range(8)]
    par = A.Parameters(algorithm="Line Search", max_iter=100, device_eval=True)
    hb = batch.HipBatch(prs[0], 8, groups=2)
    assert hb.groups == 2
    runs8, stats, bst = batch.solve_batch_lockstep(prs, par, 8, batch=hb)
    J = hb.ns_basis()
    hb.close()
    assert stats["scenarios"] == 8 and stats["converged"] == 8, stats
    assert bst["ops"] >= 2 * bst["launches"], bst
    hb3 = batch.HipBatch(prs[0], 3)
    hb3.set_ns_basis(J)
    runs3, _, _ = batch.solve_batch_lockstep(prs, par, 3, batch=hb3)
    hb3.close()
    opt = _handle_for(prs[0])
    for s, pr in enumerate(prs):
        opt.set_bounds(A.QpData(None, 0.0, None, None, pr.g_L, pr.g_U, pr.x_L, pr.x_U))
        one = _native_run(opt, pr, par, J)
        for r in (runs8[s], runs3[s]):
            assert r.ret == one.ret == 0 and r.iter == one.iter and r.lp_solves == one.lp_solves and r.paths == one.paths
            assert np.array_equal(r.x, one.x) and np.array_equal(r.lam, one.lam)
            assert np.array_equal(r.mult_x_U, one.mult_x_U) and np.array_equal(r.mult_x_L, one.mult_x_L)
            assert r.obj_val == one.obj_val
    opt.close()
