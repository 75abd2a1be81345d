"""The Hessian of the Lagrangian on the device through the C ABI (include/asm_hip.h: asm_eval_hessian_structure, asm_eval_hessian_lagrangian,
asm_eval_hessian_product) against the host twin (moi_evaluator.FunctionModel, nlexpr.ExprBlock.hessian_values): pattern exactly, values and
products bit for bit on arithmetic tapes and to the parity bar with math-library ops, no interference with the SLP state, argument errors."""
import ctypes as C

import numpy as np
import pytest

from activesetmethods_amd import acopf, problems
from tests.test_nlhess_cpu import PARITY, all_ops_model, arithmetic_model, parity_cases, store_model
from tests.test_nlparams_gpu import _handle_for, _same_run

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3


def _twin(fm, x, sigma, lam):
    h = fm.hessian_lagrangian_structure()
    return fm.eval_hessian_lagrangian(np.asarray(x, float), sigma, np.asarray(lam, float), np.zeros(len(h)))


def test_structure_equals_the_twin_exactly():
    models = [(name, fm) for name, fm, _, _ in parity_cases()] + [("store", store_model()), ("hs071", problems.hs071_function_model()),
                                                                 ("arithmetic", arithmetic_model())]
    for name, fm in models:
        pr = fm.to_problem(name)
        opt = _handle_for(pr, fm)
        rows, cols = opt.hessian_structure()
        assert list(zip(rows.tolist(), cols.tolist())) == fm.hessian_lagrangian_structure(), name
        nnz = C.c_int64(-1)
        assert opt._lib.asm_eval_hessian_structure(opt._h, C.byref(nnz), None, None) == 0 and nnz.value == len(rows)
        opt.close()


def _exact_models():
    out = []
    for sense in ("MIN_SENSE", "MAX_SENSE"):
        hs = problems.hs071_function_model()
        hs.sense = sense
        te = problems.toy_expr_function_model()
        te.sense = sense
        out += [("hs071 " + sense, hs, hs.start_point()), ("toy " + sense, te, np.array([-1.3, 0.8])),
                ("arithmetic " + sense, arithmetic_model(sense), np.array([0.45, 1.05, 0.7, 0.9])), ("store " + sense, store_model(sense=sense), np.array([0.1, 0.2, 0.3]))]
    return out


def test_values_and_products_are_bit_identical_on_arithmetic_tapes():
    for name, fm, x0 in _exact_models():
        pr = fm.to_problem(name)
        opt = _handle_for(pr, fm)
        rng = np.random.default_rng(len(name))
        for rep in range(3):
            x = x0 if rep == 0 else x0 + 0.05 * rng.uniform(-1, 1, fm.n)
            lam, v = rng.standard_normal(fm.m), rng.standard_normal(fm.n)
            for sigma in (1.0, 0.0):
                want = _twin(fm, x, sigma, lam)
                assert np.array_equal(opt.eval_hessian_lagrangian(x, sigma, lam), want), (name, rep, sigma)
                assert np.array_equal(opt.hessian_product(x, sigma, lam, v), fm.hessian_lagrangian_product(x, sigma, lam, v)), (name, rep, sigma)
        opt.close()


def _library_models():
    rng = np.random.default_rng(11)
    out = [("all ops " + s, all_ops_model(s), rng.uniform(0.4, 1.1, 4)) for s in ("MIN_SENSE", "MAX_SENSE")]
    for case in ("case118", "case1354pegase"):
        fe = acopf.function_model(acopf.synthetic_case(case, 1, 0.5), nlp="expr")
        out.append(("acopf %s expr" % case, fe, fe.start_point() + 0.01 * rng.standard_normal(fe.n)))
    return out


def test_values_and_products_with_math_library_ops_meet_the_parity_bar():
    for name, fm, x in _library_models():
        pr = fm.to_problem(name)
        opt = _handle_for(pr, fm)
        rng = np.random.default_rng(len(name))
        lam, v = rng.standard_normal(fm.m), rng.standard_normal(fm.n)
        for sigma in (1.0, 0.0):
            want, got = _twin(fm, x, sigma, lam), opt.eval_hessian_lagrangian(x, sigma, lam)
            bar = PARITY * max(1.0, float(np.abs(want).max()))
            print("%s sigma %g: max |H_device - H_twin| = %.3e, bar %.3e" % (name, sigma, float(np.abs(got - want).max()), bar))
            assert np.all(np.abs(got - want) <= bar), (name, sigma)
            wp, gp = fm.hessian_lagrangian_product(x, sigma, lam, v), opt.hessian_product(x, sigma, lam, v)
            assert np.all(np.abs(gp - wp) <= PARITY * max(1.0, float(np.abs(wp).max()))), (name, sigma)
        opt.close()


def test_hessian_calls_do_not_interfere():
    """asm_eval_functions, asm_eval_constraints and a 3-LP asm_slp_run give the same bits with Hessian calls between them as without;
    asm_eval_set_data followed by a Hessian call equals a fresh set-up with the changed data."""
    import activesetmethods_amd as A
    for fm, alg in ((problems.hs071_function_model(), "Trust Region"), (problems.parametric_function_model(0.5, 4.0), "Line Search")):
        pr = fm.to_problem()
        par = A.Parameters(algorithm=alg, max_iter=60, device_eval=True)
        rng = np.random.default_rng(3)
        xs = [pr.x0, pr.x0 + 0.01 * rng.standard_normal(pr.n)]
        lam, v = rng.standard_normal(pr.m), rng.standard_normal(pr.n)
        outs = []
        for hess in (False, True):
            opt = _handle_for(pr, fm)
            got = []
            for x in xs:
                f, df, E = opt.eval_functions(x)
                if hess:
                    opt.eval_hessian_lagrangian(0.5 * x + 0.1, 1.0, lam)
                dE = opt.jacobian_values()
                ft, Et = opt.eval_constraints(0.5 * x + 0.25)
                if hess:
                    opt.hessian_product(x, 0.5, lam, v)
                    opt.hessian_structure()
                got.append((f, df, E, dE, ft, Et))
            run = opt.slp_run(pr.x0, par, 3)
            if hess:
                opt.eval_hessian_lagrangian(run.x, 1.0, -run.lam)
            run2 = opt.slp_run(pr.x0, par, 3)
            outs.append((got, run, run2))
            opt.close()
        (ga, ra, ra2), (gb, rb, rb2) = outs
        assert 1 <= ra.lp_solves <= 3
        _same_run(ra, rb)
        _same_run(ra2, rb2)
        for ea, eb in zip(ga, gb):
            assert ea[0] == eb[0] and ea[4] == eb[4]
            assert all(np.array_equal(p, q) for p, q in zip(ea[1:4] + ea[5:], eb[1:4] + eb[5:]))
    fa, fb = problems.parametric_function_model(0.5, 4.0), problems.parametric_function_model(0.7, 5.0)
    pa, pb = fa.to_problem(), fb.to_problem()
    oa, ob = _handle_for(pa, fa), _handle_for(pb, fb)
    x, lam = np.array([2.1, 1.9]), np.array([0.4, -1.2])
    before = oa.eval_hessian_lagrangian(x, 1.0, lam)
    oa.set_eval_data(np.asarray(fb.nlp.device[2], np.float64))
    after = oa.eval_hessian_lagrangian(x, 1.0, lam)
    assert np.array_equal(after, ob.eval_hessian_lagrangian(x, 1.0, lam)) and np.array_equal(after, _twin(fb, x, 1.0, lam))
    assert not np.array_equal(before, after)
    oa.close()
    ob.close()


def test_argument_and_state_errors():
    import activesetmethods_amd as A
    from activesetmethods_amd import _lib
    lib = _lib.load()
    fm = problems.hs071_function_model()
    pr = fm.to_problem()
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    x, lam, v, vals, out = np.ones(4), np.ones(2), np.ones(4), np.zeros(16), np.zeros(4)
    nnz = C.c_int64(0)
    rows, cols = np.zeros(16, np.int64), np.zeros(16, np.int64)
    assert lib.asm_eval_hessian_structure(opt._h, C.byref(nnz), None, None) == ERR_STATE                 # before asm_eval_setup
    assert lib.asm_eval_hessian_lagrangian(opt._h, _lib.dptr(x), 1.0, _lib.dptr(lam), _lib.dptr(vals)) == ERR_STATE
    assert lib.asm_eval_hessian_product(opt._h, _lib.dptr(x), 1.0, _lib.dptr(lam), _lib.dptr(v), _lib.dptr(out)) == ERR_STATE
    opt.eval_setup(fm)
    f0 = opt.eval_functions(pr.x0)
    assert lib.asm_eval_hessian_structure(opt._h, None, None, None) == ERR_ARG
    assert lib.asm_eval_hessian_structure(opt._h, C.byref(nnz), _lib.i64ptr(rows), None) == ERR_ARG
    assert lib.asm_eval_hessian_structure(None, C.byref(nnz), None, None) == ERR_ARG
    assert lib.asm_eval_hessian_lagrangian(opt._h, None, 1.0, _lib.dptr(lam), _lib.dptr(vals)) == ERR_ARG
    assert lib.asm_eval_hessian_lagrangian(opt._h, _lib.dptr(x), 1.0, None, _lib.dptr(vals)) == ERR_ARG
    assert lib.asm_eval_hessian_lagrangian(opt._h, _lib.dptr(x), 1.0, _lib.dptr(lam), None) == ERR_ARG
    for bad in range(4):
        a = [_lib.dptr(x), _lib.dptr(lam), _lib.dptr(v), _lib.dptr(out)]
        a[bad] = None
        assert lib.asm_eval_hessian_product(opt._h, a[0], 1.0, a[1], a[2], a[3]) == ERR_ARG, bad
    f1 = opt.eval_functions(pr.x0)                                                                        # the handle still evaluates
    assert f0[0] == f1[0] and np.array_equal(f0[1], f1[1]) and np.array_equal(f0[2], f1[2])
    assert np.array_equal(opt.eval_hessian_lagrangian(pr.x0, 1.0, lam), _twin(fm, pr.x0, 1.0, lam))
    opt.close()
    for fk in (acopf.function_model(acopf.synthetic_case("case118", 1, 0.5)), problems.synthetic_dense_function_model(40, 10)):      # kinds 1 and 2
        pk = fk.to_problem()
        ok = _handle_for(pk, fk)
        assert lib.asm_eval_hessian_structure(ok._h, C.byref(nnz), None, None) == ERR_ARG
        with pytest.raises(A.AsmHipError, match="second derivatives"):
            ok.eval_hessian_lagrangian(pk.x0, 1.0, np.zeros(pk.m))
        with pytest.raises(A.AsmHipError, match="second derivatives"):
            ok.hessian_product(pk.x0, 1.0, np.zeros(pk.m), np.ones(pk.n))
        f, df, E = ok.eval_functions(pk.x0)
        assert np.isfinite(f) and np.all(np.isfinite(E))
        ok.close()
