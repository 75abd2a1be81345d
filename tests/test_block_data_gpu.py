"""Value and solution sensitivities of the Ohm's-law block (nlp_kind 4) and of the dense quadratic block (nlp_kind 5) with respect to
their own data, through the C ABI (include/asm_hip.h, "Data derivatives of the block kernels"): asm_eval_data_gradient and
asm_eval_data_cross against the NumPy twins (NlpBlock.data_gradient / data_cross) and against the expression form with the coefficients
as parameters, asm_solution_sensitivity(_multi) on them, asm_batch_data_gradient, no interference with the SLP state, and the refusals
that stay."""
import ctypes as C

import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import _lib, acopf, batch, problems, sensitivity
from tests.test_batch_eqp_gpu import _stack
from tests.test_block_data_cpu import block_cross, block_gradient, points
from tests.test_nlhess_cpu import PARITY
from tests.test_nlparams_gpu import _handle_for, _same_run
from tests.test_ohm_hess_cpu import grid
from tests.test_sensitivity_cpu import KKT_BAR, rel_err
from tests.test_sensitivity_gpu import LIBM_BAR

pytestmark = pytest.mark.gpu
LS = "Line Search"
ERR_ARG, ERR_STATE = -1, -3


def _same_bits(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. Ohm's-law block against the twin
@pytest.mark.parametrize("name", ["grid3", "grid14", "case300"])        # case300: 411 branches, the second workgroup partly full
def test_ohm_block_against_the_twin(name):
    fm = acopf.function_model(grid(name), hessian=True)
    opt = _handle_for(fm.to_problem(name), fm)
    kept = []
    for rep, x, lam, dc in points(fm, len(name)):
        g, (u, w) = opt.eval_data_gradient(x, lam), opt.data_cross(x, lam, dc)
        tg, (tu, tw) = block_gradient(fm, x, lam), block_cross(fm, x, lam, dc)
        eg, eu, ew = rel_err(g, tg), rel_err(u, tu), rel_err(w, tw)
        print("%s point %d: rel err gradient %.3e, u %.3e, w %.3e (bar %.1e)" % (name, rep, eg, eu, ew, LIBM_BAR))
        assert g.shape == tg.shape and u.shape == (fm.n,) and w.shape == (fm.m,)
        assert np.any(tg != 0.0) and np.any(tu != 0.0) and np.any(tw != 0.0)
        assert eg <= LIBM_BAR and eu <= LIBM_BAR and ew <= LIBM_BAR, (name, rep, eg, eu, ew)
        assert not w[:fm.nlp_constraint_offset].any()                                   # the rows of the function store: no data
        assert np.array_equal(opt.eval_data_gradient(x, lam), g) and _same_bits(opt.data_cross(x, lam, dc), (u, w))      # a second call: equal bits
        kept.append((x, lam, dc, g, u, w))
    # the block is linear in its data: its derivatives do not depend on it
    dpar = np.asarray(fm.nlp.device[2], float)
    opt.set_eval_data(1.5 * dpar + 0.25)
    for x, lam, dc, g, u, w in kept:
        assert np.array_equal(opt.eval_data_gradient(x, lam), g) and _same_bits(opt.data_cross(x, lam, dc), (u, w))
    opt.close()


# ------------------------------------------------------------------------------------------------ 2. dense block against the twin
@pytest.mark.parametrize("n,m", [(23, 7), (300, 5)])                  # 300 variables: a second workgroup, partly full
def test_dense_block_against_the_twin(n, m):
    fm = problems.synthetic_dense_function_model(n, m, hessian=True)
    opt = _handle_for(fm.to_problem(), fm)
    for rep, x, lam, dc in points(fm, n + m):
        g, (u, w) = opt.eval_data_gradient(x, lam), opt.data_cross(x, lam, dc)
        tg, (tu, tw) = block_gradient(fm, x, lam), block_cross(fm, x, lam, dc)
        bar = PARITY * max(1.0, float(np.abs(tw).max()))
        print("dense (%d, %d) point %d: max |w - twin| %.3e (bar %.3e)" % (n, m, rep, float(np.abs(w - tw).max()), bar))
        assert np.array_equal(g, tg) and np.array_equal(u, tu), (n, m, rep)
        assert np.all(np.abs(w - tw) <= bar), (n, m, rep)
        assert np.any(tu != 0.0) and (rep == 0 or (np.any(tw != 0.0) and np.any(tg != 0.0)))        # (the start point is x = 0)
        assert np.array_equal(opt.eval_data_gradient(x, lam), g) and _same_bits(opt.data_cross(x, lam, dc), (u, w))
    opt.close()


# ------------------------------------------------------------------------------------------------ 3. the multi entry
@pytest.fixture(scope="module")
def grid14_solution():
    """(fm, pr, x, lam, row_state, bound_state) at the point of a short asm_slp_run on the 14-bus grid, kind 4."""
    fm = acopf.function_model(grid("grid14"), hessian=True)
    pr = fm.to_problem("grid14")
    opt = _handle_for(pr, fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm=LS, max_iter=60, device_eval=True), 12)
    opt.close()
    rs, bs = sensitivity.working_set(pr, run.x, run.lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    print("grid14: %d LPs, |W| %d, |F| %d" % (run.lp_solves, rs.sum(), (bs == 0).sum()))
    assert rs.sum() <= (bs == 0).sum() and np.any(run.lam[fm.nlp_constraint_offset:] != 0.0)
    return fm, pr, run.x, run.lam, rs, bs


def _column_bits(out, c):
    DX, DLAM, DZ, infos = out
    return (DX[c].tobytes(), DLAM[c].tobytes(), DZ[c].tobytes()) + tuple(getattr(infos[c], k) for k, _ in infos[c]._fields_)


def test_multi_columns_depend_on_their_own_direction_only(grid14_solution):
    fm, pr, x, lam, rs, bs = grid14_solution
    nd = len(fm.nlp.device[2])
    idx = np.array([0, nd // 2 + 1, nd - 1])
    DC = np.random.default_rng(4).standard_normal((70, nd))               # two chunks, the second of 6 columns
    DC[:3] = 0.0
    DC[np.arange(3), idx] = 1.0
    opt = _handle_for(pr, fm)
    all70, first3 = opt.solution_sensitivity_multi(x, lam, rs, bs, DC), opt.solution_sensitivity_multi(x, lam, rs, bs, DC[:3])
    assert [i.status for i in all70[3]] == [0] * 70 and np.all(np.isfinite(all70[0])) and np.any(all70[0][69] != 0.0)
    for c in range(3):
        assert _column_bits(all70, c) == _column_bits(first3, c), c
    Jx, Jl = sensitivity.solution_jacobian(opt, fm, x, lam, rs, bs, idx)
    assert np.array_equal(Jx, first3[0].T) and np.array_equal(Jl, first3[1].T)
    # ... and they are the single entry's answer for that direction, to the KKT bar
    for c in (0, 64, 69):
        dx, dlam, dz, info = opt.solution_sensitivity(x, lam, rs, bs, DC[c])
        u, w = block_cross(fm, x, lam, DC[c])
        ref = sensitivity.kkt_reference(fm, x, lam, rs, bs, u, w)
        errs = [rel_err(all70[k][c], ref[k]) for k in range(3)] + [rel_err(g, r) for g, r in zip((dx, dlam, dz), ref)]
        print("grid14 column %d: rel err against the dense solve, multi %.3e %.3e %.3e, single %.3e %.3e %.3e (bar %.3e)" % (c, *errs, KKT_BAR))
        assert info.status == 0 and max(errs) <= KKT_BAR, (c, errs)
    opt.close()


# ------------------------------------------------------------------------------------------------ 4. residuals on the case118-sized grid
def test_solution_sensitivity_on_the_case118_sized_ohm_block():
    """The instance of test_sensitivity_gpu.test_solution_sensitivity_on_the_branch_parameter_acopf (seed 1, load 0.5) on the Ohm's-law
    kernel: the dense KKT residuals of the device's answer, recomputed in NumPy with the twin's (u, w), stay under the bar."""
    fm = acopf.function_model(acopf.synthetic_case("case118", 1, 0.5), hessian=True)
    pr = fm.to_problem("acopf ohm block")
    opt = _handle_for(pr, fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm=LS, max_iter=60, device_eval=True), 6)
    x, lam = run.x, run.lam
    rs, bs = sensitivity.working_set(pr, x, lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    H, J = sensitivity.lagrangian_hessian(fm, x, lam), sensitivity.dense_jacobian(fm, x)
    F, W = np.nonzero(bs == 0)[0], np.nonzero(rs == 1)[0]
    sv = np.linalg.svd(J[np.ix_(W, F)], compute_uv=False)
    print("acopf: n %d, m %d, |F| %d, |W| %d, singular values of A in [%.3e, %.3e]" % (fm.n, fm.m, len(F), len(W), sv[-1], sv[0]))
    assert len(W) <= len(F) and sv[-1] > 1e-5 * sv[0]                   # full-rank working rows (checked on the host)
    dc = np.random.default_rng(9).standard_normal(len(fm.nlp.device[2]))
    u, w = block_cross(fm, x, lam, dc)
    dx, dlam, dz, info = opt.solution_sensitivity(x, lam, rs, bs, dc)
    r1 = (H @ dx - J[W].T @ dlam[W] + u)
    r2 = J[W] @ dx + w[W]
    size = max(1.0, float(np.abs(u).max()), float(np.abs(w).max()), float(np.abs(H).max() * np.abs(dx).max()), float(np.abs(J).max() * np.abs(dlam).max()))
    e1, e2 = float(np.abs(r1[F]).max()) / size, float(np.abs(r2).max()) / size if len(W) else 0.0
    print("acopf: status %d, %d CG iterations, relative residuals %.3e / %.3e (bar %.3e), info %.3e / %.3e" % (info.status, info.cg_iters, e1, e2, KKT_BAR, info.res_stat, info.res_feas))
    assert info.status == 0 and 0 < info.cg_iters <= 2 * (len(F) - len(W)) + 20
    assert np.all(dx[bs != 0] == 0.0) and np.all(dlam[rs == 0] == 0.0) and np.all(dz[F] == 0.0)
    assert np.any(dx != 0.0) and e1 <= KKT_BAR and e2 <= KKT_BAR, (e1, e2)
    opt.close()


# ------------------------------------------------------------------------------------------------ 5. the two forms at one point
def test_the_kernel_form_against_the_expression_form():
    case = grid("grid14")
    fk, fe = acopf.function_model(case, hessian=True), acopf.function_model(case, nlp="expr", branch_params=True)
    nd = len(fk.nlp.device[2])
    assert len(fe.nlp.device[2]) == nd                                   # the same 8 n_branch entries, the same layout
    ok, oe = _handle_for(fk.to_problem(), fk), _handle_for(fe.to_problem(), fe)
    for rep, x, lam, dc in points(fk, 7):
        gk, ge = ok.eval_data_gradient(x, lam), oe.eval_data_gradient(x, lam)
        (uk, wk), (ue, we) = ok.data_cross(x, lam, dc), oe.data_cross(x, lam, dc)
        eg, eu, ew = rel_err(gk, ge), rel_err(uk, ue), rel_err(wk, we)
        print("grid14 point %d, kind 4 against kind 3: rel err gradient %.3e, u %.3e, w %.3e (bar %.1e)" % (rep, eg, eu, ew, LIBM_BAR))
        assert np.any(ue != 0.0) and np.any(we != 0.0) and eg <= LIBM_BAR and eu <= LIBM_BAR and ew <= LIBM_BAR, (rep, eg, eu, ew)
    ok.close()
    oe.close()


# ------------------------------------------------------------------------------------------------ 6. the scenario batch
def test_batch_data_gradient_equals_fresh_handles():
    """Four line scenarios of the 14-bus grid on two slots (they refill): the batch gradient at the batch's runs equals the per-handle one
    on a fresh handle with the scenario's data; a Line-Search run of the batch returns the same bits before and after the call."""
    base = grid("grid14")
    fms = [acopf.function_model(acopf.line_scenario_case(base, s), hessian=True) for s in range(4)]
    prs = [fm.to_problem("line scenario %d" % s) for s, fm in enumerate(fms)]
    par = A.Parameters(algorithm=LS, max_iter=40, device_eval=True)
    hb = batch.HipBatch(prs[0], 2)
    data = hb.scenario_data(prs)
    assert data.shape == (4, len(fms[0].nlp.device[2])) and not np.array_equal(data[0], data[1])
    hb.slp_run(*_stack(prs), par, data=data)
    J = hb.ns_basis()                                                     # every compared run starts from these basis columns
    hb.set_ns_basis(J)
    before = hb.slp_run(*_stack(prs), par, data=data)
    X, L = np.stack([r.x for r in before]), np.stack([r.lam for r in before])
    G = hb.data_gradient(X, L)
    hb.set_ns_basis(J)
    after = hb.slp_run(*_stack(prs), par, data=data)
    hb.close()
    assert G.shape == data.shape and {r.slot for r in before} == {0, 1}
    for s in range(4):
        _same_run(before[s], after[s])
        opt = _handle_for(prs[s], fms[s])
        want = opt.eval_data_gradient(before[s].x, before[s].lam)
        opt.close()
        assert np.array_equal(G[s], want) and np.any(want != 0.0), s


# ------------------------------------------------------------------------------------------------ 7. isolation, errors
def test_the_new_calls_do_not_interfere():
    fm = acopf.function_model(grid("grid14"), hessian=True)
    pr = fm.to_problem()
    par = A.Parameters(algorithm=LS, max_iter=60, device_eval=True)
    rng = np.random.default_rng(3)
    lam, DC = rng.standard_normal(pr.m), rng.standard_normal((3, len(fm.nlp.device[2])))
    outs = []
    for calls in (False, True):
        opt = _handle_for(pr, fm)

        def new_calls(x, lm):
            rs, bs = sensitivity.working_set(pr, x, lm, np.zeros(pr.n), np.zeros(pr.n), tol=1e-6)
            if rs.sum() > (bs == 0).sum():
                rs[:] = 0
            opt.eval_data_gradient(x, lm)
            opt.data_cross(x, lm, DC[0])
            opt.solution_sensitivity(x, lm, rs, bs, DC[0])
            opt.solution_sensitivity_multi(x, lm, rs, bs, DC)
        if calls:
            new_calls(pr.x0 + 0.01, lam)
        f0 = opt.eval_functions(pr.x0)
        run = opt.slp_run(pr.x0, par, 3)
        if calls:
            new_calls(run.x, run.lam)
        f1 = opt.eval_functions(run.x)
        run2 = opt.slp_run(pr.x0, par, 3)
        outs.append((f0, f1, run, run2))
        opt.close()
    (fa0, fa1, ra, ra2), (fb0, fb1, rb, rb2) = outs
    assert 1 <= ra.lp_solves <= 3
    _same_run(ra, rb)
    _same_run(ra2, rb2)
    for fa, fb in ((fa0, fb0), (fa1, fb1)):
        assert fa[0] == fb[0] and np.array_equal(fa[1], fb[1]) and np.array_equal(fa[2], fb[2])


def test_argument_and_state_errors():
    lib = _lib.load()
    D, I = _lib.dptr, _lib.i32ptr
    info = _lib.KktInfo()
    for fm in (acopf.function_model(grid("grid3"), hessian=True), problems.synthetic_dense_function_model(9, 4, hessian=True)):
        pr = fm.to_problem()
        nd = len(fm.nlp.device[2])
        opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
        x, lam, dc = pr.x0 + 0.01, np.ones(pr.m), np.ones(nd)
        out, u, w, dx, dlam, dz = np.zeros(nd), np.zeros(pr.n), np.zeros(pr.m), np.zeros(pr.n), np.zeros(pr.m), np.zeros(pr.n)
        rs, bs = np.zeros(pr.m, np.int32), np.zeros(pr.n, np.int32)
        grad = lambda a: lib.asm_eval_data_gradient(opt._h, *a)
        cross = lambda a: lib.asm_eval_data_cross(opt._h, *a)
        sens = lambda a: lib.asm_solution_sensitivity(opt._h, *a)
        multi = lambda a: lib.asm_solution_sensitivity_multi(opt._h, *a)
        ga = [D(x), D(lam), D(out)]
        ca = [D(x), D(lam), D(dc), D(u), D(w)]
        sa = [D(x), D(lam), I(rs), I(bs), D(dc), None, D(dx), D(dlam), D(dz), C.byref(info)]
        ma = [D(x), D(lam), I(rs), I(bs), 1, D(dc), None, D(dx), D(dlam), D(dz), C.byref(info)]
        assert grad(ga) == ERR_STATE and cross(ca) == ERR_STATE and sens(sa) == ERR_STATE and multi(ma) == ERR_STATE      # before asm_eval_setup
        opt.eval_setup(fm)
        f0 = opt.eval_functions(pr.x0)
        assert grad(ga) == 0 and cross(ca) == 0
        for args, call, nulls in ((ga, grad, (0, 1, 2)), (ca, cross, (0, 1, 2, 3, 4)), (sa, sens, (0, 1, 2, 3, 4, 6, 7, 9)), (ma, multi, (0, 1, 2, 3, 5, 7, 8, 10))):
            for bad in nulls:
                a = list(args)
                a[bad] = None
                assert call(a) == ERR_ARG, (call, bad)
        with pytest.raises(ValueError):
            opt.data_cross(x, lam, dc[:-1])
        f1 = opt.eval_functions(pr.x0)                                                                        # the handle still evaluates
        assert f0[0] == f1[0] and np.array_equal(f0[1], f1[1]) and np.array_equal(f0[2], f1[2])
        assert _same_bits(opt.data_cross(x, lam, dc), (u, w)) and np.array_equal(opt.eval_data_gradient(x, lam), out)
        opt.close()
    for fk in (acopf.function_model(grid("grid14")), problems.synthetic_dense_function_model(40, 10)):      # kinds 1 and 2: refused as before
        pk = fk.to_problem()
        ok = _handle_for(pk, fk)
        z = lambda k: np.zeros(max(k, 1))
        rs0, bs0 = np.zeros(pk.m, np.int32), np.zeros(pk.n, np.int32)
        nd = len(fk.nlp.device[2])
        assert lib.asm_eval_data_cross(ok._h, D(pk.x0), D(z(pk.m)), D(z(nd)), D(z(pk.n)), D(z(pk.m))) == ERR_ARG
        assert lib.asm_solution_sensitivity(ok._h, D(pk.x0), D(z(pk.m)), I(rs0), I(bs0), D(z(nd)), None, D(z(pk.n)), D(z(pk.m)), None, C.byref(info)) == ERR_ARG
        assert lib.asm_eval_data_gradient(ok._h, D(pk.x0), D(z(pk.m)), D(z(nd))) == ERR_ARG
        with pytest.raises(A.AsmHipError, match="expression blocks"):
            ok.eval_data_gradient(pk.x0, np.zeros(pk.m))
        with pytest.raises(A.AsmHipError, match="expression blocks"):
            ok.data_cross(pk.x0, np.zeros(pk.m), np.zeros(nd))
        hb = batch.HipBatch(pk, 2)
        with pytest.raises(A.AsmHipError, match="expression blocks"):
            hb.data_gradient(pk.x0[None, :], np.zeros((1, pk.m)))
        hb.close()
        ok.close()
