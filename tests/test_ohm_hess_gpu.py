"""Second derivatives of the Ohm's-law block (nlp_kind 4: k_nlp_ohm_hess + the occurrence gather) and of the dense quadratic block
(nlp_kind 5: k_nlp_dense_hess) through the C ABI: pattern, values and products against the host twins; kinds 4 / 5 against kinds 1 / 2
for everything those already do; the KKT step, SLP-EQP per handle and the scenario batch on the new kinds."""
import functools

import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import acopf, batch, eqp, problems, sensitivity
from tests.test_batch_eqp_gpu import _fresh_handle_run, _same_run as _same_eqp_run, _stack
from tests.test_kkt_step_cpu import KKT_STEP_BAR, step_errors
from tests.test_nlhess_cpu import PARITY
from tests.test_nlparams_gpu import _handle_for, _same_run
from tests.test_ohm_hess_cpu import grid

pytestmark = pytest.mark.gpu
EQP, TR = "SLP-EQP", "Trust Region"
S = 4


def _twin(fm, x, sigma, lam):
    h = fm.hessian_lagrangian_structure()
    return fm.eval_hessian_lagrangian(np.asarray(x, float), sigma, np.asarray(lam, float), np.zeros(len(h)))


def _bits(out, c):
    """Everything asm_kkt_step_multi returned for column c, as comparable bits."""
    info = out[3][c]
    return (out[0][c].tobytes(), out[1][c].tobytes(), out[2][c].tobytes()) + tuple(getattr(info, k) for k, _ in info._fields_)


def _structure(opt):
    rows, cols = opt.hessian_structure()
    return list(zip(rows.tolist(), cols.tolist()))


# ------------------------------------------------------------------------------------------------ 1. pattern, values, products
@pytest.mark.parametrize("name", ["grid3", "grid14", "case300"])        # case300: 411 branches, the second workgroup partly full
def test_ohm_block_against_the_twin(name):
    fm = acopf.function_model(grid(name), hessian=True)
    opt = _handle_for(fm.to_problem(name), fm)
    assert _structure(opt) == fm.hessian_lagrangian_structure()
    rng = np.random.default_rng(len(name))
    x0 = fm.start_point()
    for rep in range(2):
        x = x0 if rep == 0 else x0 + 0.05 * rng.standard_normal(fm.n)
        lam, v = rng.standard_normal(fm.m), rng.standard_normal(fm.n)
        for sigma in (1.0, 0.0):
            want, got = _twin(fm, x, sigma, lam), opt.eval_hessian_lagrangian(x, sigma, lam)
            bar = PARITY * max(1.0, float(np.abs(want).max()))
            wp, gp = fm.hessian_lagrangian_product(x, sigma, lam, v), opt.hessian_product(x, sigma, lam, v)
            print("%s point %d sigma %g: max |H_device - H_twin| = %.3e (bar %.3e), product %.3e" %
                  (name, rep, sigma, float(np.abs(got - want).max()), bar, float(np.abs(gp - wp).max())))
            assert np.all(np.abs(got - want) <= bar), (name, rep, sigma)
            assert np.all(np.abs(gp - wp) <= PARITY * max(1.0, float(np.abs(wp).max()))), (name, rep, sigma)
            assert np.array_equal(opt.eval_hessian_lagrangian(x, sigma, lam), got)                  # two calls on one handle: equal bits
            assert np.array_equal(opt.hessian_product(x, sigma, lam, v), gp)
    opt.close()


@pytest.mark.parametrize("n,m", [(23, 7), (300, 5)])                  # 300 variables: a second workgroup, partly full
def test_dense_block_is_bit_identical_to_the_twin(n, m):
    fm = problems.synthetic_dense_function_model(n, m, hessian=True)
    opt = _handle_for(fm.to_problem(), fm)
    assert _structure(opt) == fm.hessian_lagrangian_structure()
    rng = np.random.default_rng(n)
    for rep in range(2):
        x, lam, v = rng.standard_normal(n), rng.standard_normal(fm.m), rng.standard_normal(n)
        for sigma in (1.0, 0.0):
            got = opt.eval_hessian_lagrangian(x, sigma, lam)
            assert np.array_equal(got, _twin(fm, x, sigma, lam)), (rep, sigma)
            gp = opt.hessian_product(x, sigma, lam, v)
            assert np.array_equal(gp, fm.hessian_lagrangian_product(x, sigma, lam, v)), (rep, sigma)
            assert np.array_equal(opt.eval_hessian_lagrangian(x, sigma, lam), got) and np.array_equal(opt.hessian_product(x, sigma, lam, v), gp)
    opt.close()


# ------------------------------------------------------------------------------------------------ 2. kinds 4 / 5 are kinds 1 / 2 for what those do
def _first_order(fm, hessian_calls):
    """Values, Jacobian, a trial point and a 3-iteration Trust-Region run of a handle, optionally with Hessian calls in between."""
    pr = fm.to_problem()
    opt = _handle_for(pr, fm)
    rng = np.random.default_rng(3)
    xs, lam = (pr.x0, pr.x0 + 0.01 * rng.standard_normal(pr.n)), rng.standard_normal(pr.m)
    out = []
    for x in xs:
        f, df, E = opt.eval_functions(x)
        if hessian_calls:
            opt.eval_hessian_lagrangian(0.5 * x + 0.1, 1.0, lam)
        dE = opt.jacobian_values()
        ft, Et = opt.eval_constraints(0.5 * x + 0.25)
        out.append((f, df, E, dE, ft, Et))
    run = opt.slp_run(pr.x0, A.Parameters(algorithm=TR, max_iter=3, device_eval=True))
    opt.close()
    return out, run


@pytest.mark.parametrize("which", ["ohm", "dense"])
def test_first_order_bits_equal_the_kind_without_second_derivatives(which):
    if which == "ohm":
        case = grid("grid14")
        plain, hess = acopf.function_model(case), acopf.function_model(case, hessian=True)
    else:
        plain, hess = problems.synthetic_dense_function_model(40, 10), problems.synthetic_dense_function_model(40, 10, hessian=True)
    (ea, ra), (eb, rb) = _first_order(plain, False), _first_order(hess, True)
    assert ra.lp_solves >= 1
    _same_run(ra, rb)
    for a, b in zip(ea, eb):
        assert a[0] == b[0] and a[4] == b[4]
        assert all(np.array_equal(p, q) for p, q in zip(a[1:4] + a[5:], b[1:4] + b[5:]))


def test_set_eval_data_reaches_the_hessian():
    base = grid("grid14")
    fa, fb = acopf.function_model(base, hessian=True), acopf.function_model(acopf.line_scenario_case(base, 1), hessian=True)
    oa, ob = _handle_for(fa.to_problem(), fa), _handle_for(fb.to_problem(), fb)
    rng = np.random.default_rng(6)
    x, lam, v = fa.start_point() + 0.02 * rng.standard_normal(fa.n), rng.standard_normal(fa.m), rng.standard_normal(fa.n)
    before = oa.eval_hessian_lagrangian(x, 1.0, lam)
    oa.set_eval_data(np.asarray(fb.nlp.device[2], np.float64))
    after = oa.eval_hessian_lagrangian(x, 1.0, lam)
    assert np.array_equal(after, ob.eval_hessian_lagrangian(x, 1.0, lam)) and not np.array_equal(before, after)
    assert np.array_equal(oa.hessian_product(x, 1.0, lam, v), ob.hessian_product(x, 1.0, lam, v))
    oa.close()
    ob.close()


# ------------------------------------------------------------------------------------------------ 3. the KKT step
def test_kkt_step_on_the_ohm_block():
    """The 14-bus grid near its start point, every equality row in the working set and every variable free (|W| = 109, |F| = 118; the
    singular values of A lie in [0.22, 65]): asm_kkt_step against eqp.kkt_step_pcg at three radii, both KKT forms against each other, a
    column of asm_kkt_step_multi alone and among others."""
    fm = acopf.function_model(grid("grid14"), hessian=True)
    pr = fm.to_problem("grid14 ohm hess")
    rng = np.random.default_rng(4)
    x = pr.x0 + 0.02 * rng.standard_normal(pr.n)
    lam = 0.1 * rng.standard_normal(pr.m)
    rs, bs = (pr.g_L == pr.g_U).astype(np.int32), np.zeros(pr.n, np.int32)
    J = sensitivity.dense_jacobian(fm, x)
    ru = fm.eval_grad_f(x, np.zeros(pr.n)) - J.T @ lam
    rw = np.where(rs == 1, pr.eval_g(x, np.zeros(pr.m)) - pr.g_L, 0.0)
    radii = np.array([0.4, 2.0, 50.0])
    opt = _handle_for(pr, fm)
    steps = {}
    for form in ("dense", "sparse"):
        opt.set_kkt_form(form)
        steps[form] = [opt.kkt_step(x, lam, rs, bs, ru, rw, r) for r in radii]
        if form == "dense":
            RU, RW = np.tile(ru, (3, 1)), np.tile(rw, (3, 1))
            multi = opt.kkt_step_multi(x, lam, rs, bs, RU, RW, radii)
            alone = [opt.kkt_step_multi(x, lam, rs, bs, RU[c:c + 1], RW[c:c + 1], radii[c:c + 1]) for c in range(3)]
    opt.close()
    for c, r in enumerate(radii):
        ref = eqp.kkt_step_pcg(fm, x, lam, rs, bs, ru, rw, r)
        for form in ("dense", "sparse"):
            got = steps[form][c]
            errs = step_errors(got, ref)
            print("radius %g %s: status %d boundary %d cg %d (twin %d), rel err %s" % (r, form, got[3].status, got[3].boundary, got[3].cg_iters, ref[3]["cg_iters"],
                                                                                     " ".join("%.2e" % e for e in errs)))
            assert (got[3].status, got[3].boundary, got[3].n_rows, got[3].n_free) == (ref[3]["status"], ref[3]["boundary"], 109, 118)
            assert max(errs) <= KKT_STEP_BAR, (r, form, errs)
        d, s = steps["dense"][c], steps["sparse"][c]
        assert max(step_errors(s, (d[0], d[1], d[2], {k: getattr(d[3], k) for k in ("model", "theta", "norm_step", "norm_normal")}))) <= KKT_STEP_BAR
        assert max(step_errors((multi[0][c], multi[1][c], multi[2][c], multi[3][c]), ref)) <= KKT_STEP_BAR
        assert _bits(multi, c) == _bits(alone[c], 0), c


# ------------------------------------------------------------------------------------------------ 4. SLP-EQP on a handle
def test_slp_eqp_native_equals_the_host_driver():
    make = lambda: acopf.function_model(grid("grid14"), hessian=True)
    mdl = A.Model.from_problem(make().to_problem("grid14 ohm hess"), A.Parameters(algorithm=EQP, device_eval=True, max_iter=60))
    slp = A.optimize(mdl)
    slp.optimizer.close()
    fm = make()
    pr = fm.to_problem("grid14 ohm hess")
    opt = _handle_for(pr, fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm=EQP, device_eval=True, max_iter=60))
    opt.close()
    print("grid14 ohm hess: native status %d iter %d lp %d %r | host status %d iter %d lp %d %r" %
          (run.ret, run.iter, run.lp_solves, run.eqp_counts, slp.ret, slp.iter, slp.lp_solves, slp.eqp_counts))
    assert run.ret == 0 and mdl.status == 0
    assert (run.ret, run.iter, run.lp_solves) == (slp.ret, slp.iter, slp.lp_solves)
    assert run.eqp_counts == slp.eqp_counts and run.eqp_counts["accepted"] > 0 and run.Delta_E == slp.Delta_E and run.delta == slp.Delta
    assert np.array_equal(run.x, slp.x) and np.array_equal(run.lam, slp.lam) and np.array_equal(run.E, slp.E)
    assert np.array_equal(run.mult_x_U, slp.mult_x_U) and np.array_equal(run.mult_x_L, slp.mult_x_L)


# ------------------------------------------------------------------------------------------------ 5. the scenario batch
def _scenarios(kind):
    base = grid("grid14")
    make = acopf.scenario_case if kind == "load" else acopf.line_scenario_case
    return [acopf.function_model(make(base, s), hessian=True) for s in range(S)]


@functools.lru_cache(maxsize=None)
def _points():
    fm = _scenarios("load")[0]
    rng = np.random.default_rng(8)
    X = np.stack([fm.start_point() + 0.02 * rng.uniform(-1, 1, fm.n) for _ in range(S)])
    out = X, rng.standard_normal((S, fm.m)), rng.standard_normal((S, fm.n)), np.array([1.0, 0.5, 0.0, 2.0])
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("kind", ["load", "line"])
def test_batch_hessians_equal_fresh_handles(kind):
    """Four scenarios on two slots: the load scenarios share the block's data, the line scenarios bring theirs through the data table."""
    fms = _scenarios(kind)
    prs = [fm.to_problem("%s scenario %d" % (kind, s)) for s, fm in enumerate(fms)]
    X, L, V, sig = _points()
    want_v, want_p = [], []
    for s, fm in enumerate(fms):
        opt = _handle_for(prs[s], fm)
        want_v.append(opt.eval_hessian_lagrangian(X[s], float(sig[s]), L[s]))
        want_p.append(opt.hessian_product(X[s], float(sig[s]), L[s], V[s]))
        opt.close()
    hb = batch.HipBatch(prs[0], 2)
    data = hb.scenario_data(prs)
    assert (data is None) == (kind == "load")
    if data is not None:
        assert data.shape == (S, len(fms[0].nlp.device[2]))
        hb.set_scenario_data(data)
    rows, cols = hb.hessian_structure()
    assert list(zip(rows.tolist(), cols.tolist())) == fms[0].hessian_lagrangian_structure()
    got_v, got_p = hb.eval_hessian_lagrangian(X, sig, L), hb.hessian_product(X, sig, L, V)
    hb.close()
    assert np.array_equal(got_v, np.stack(want_v)) and np.array_equal(got_p, np.stack(want_p))
    if kind == "line":
        assert not np.array_equal(data[0], data[1])              # the scenarios' data do differ


def test_batch_slp_eqp_equals_fresh_handles():
    prs = [fm.to_problem("load scenario %d" % s) for s, fm in enumerate(_scenarios("load"))]
    par = A.Parameters(algorithm=EQP, max_iter=60, device_eval=True)
    hb = batch.HipBatch(prs[0], 2)
    runs = hb.slp_run(*_stack(prs), par)
    J = hb.ns_basis()
    hb.close()
    ones = [_fresh_handle_run(pr, par, J) for pr in prs]
    print("iter", [r.iter for r in ones], "ret", [r.ret for r in ones], "eqp", [r.eqp_counts for r in ones])
    for r, one in zip(runs, ones):
        _same_eqp_run(r, one)
    assert {r.slot for r in runs} == {0, 1} and sum(r.eqp_counts["accepted"] for r in ones) >= 1


def test_kinds_without_second_derivatives_are_refused_on_a_batch_as_before():
    for fm in (acopf.function_model(grid("grid14")), problems.synthetic_dense_function_model(40, 10)):
        pr = fm.to_problem()
        hb = batch.HipBatch(pr, 2)
        with pytest.raises(A.AsmHipError, match="second derivatives"):
            hb.hessian_structure()
        with pytest.raises(A.AsmHipError, match="second derivatives"):
            hb.eval_hessian_lagrangian(pr.x0[None, :], 1.0, np.zeros((1, pr.m)))
        hb.close()
