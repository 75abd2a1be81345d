"""Derivatives of the Ohm's-law block and of the dense quadratic block with respect to their own data, on the host
(acopf.function_model(..., hessian=True), problems.synthetic_dense_function_model(..., hessian=True): NlpBlock.data_gradient /
data_cross, the twins of k_nlp_ohm_data_grad, k_nlp_ohm_cross, k_nlp_dense_data_grad and k_nlp_dense_cross_w / _u): against the
expression twin of the same rows with the coefficients as parameters, against the blocks' own values and Jacobians by linearity,
the unchanged defaults, and through the dense KKT solve at a solution."""
import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import acopf, problems, sensitivity
from tests.test_nlhess_cpu import PARITY
from tests.test_ohm_hess_cpu import grid
from tests.test_sensitivity_cpu import KKT_BAR, rel_err
from tests.test_slp_eqp_cpu import run as host_run

LIBM_BAR = 1e-12                # tests/test_sensitivity_gpu.py: the bar of values that go through sin and cos (it needs a GPU to import)
OHM_GRIDS = ("grid3", "grid14", "case118")
DENSE_SHAPES = ((23, 7), (300, 5))


def block_cross(fm, x, lam, dc):
    """(u [n], w [m]) of the block's twin for a FunctionModel: the block's rows follow the function store's."""
    off = fm.nlp_constraint_offset
    u, wb = fm.nlp.data_cross(x, np.asarray(lam, float)[off:], dc, fm.objective_scale)
    uu, w = np.zeros(fm.n), np.zeros(fm.m)
    uu[:len(u)] = u
    w[off:] = wb
    return uu, w


def block_gradient(fm, x, lam):
    return fm.nlp.data_gradient(x, np.asarray(lam, float)[fm.nlp_constraint_offset:], fm.objective_scale)


def points(fm, seed):
    """(x, lam, dc) at the start point and at a perturbed one."""
    rng = np.random.default_rng(seed)
    x0 = fm.start_point()
    for rep in range(2):
        yield rep, (x0 if rep == 0 else x0 + 0.05 * rng.standard_normal(fm.n)), rng.standard_normal(fm.m), rng.standard_normal(len(fm.nlp.device[2]))


@pytest.fixture(scope="module")
def ohm_pairs():
    """grid -> (kernel form with derivatives, expression form with the coefficients as parameters), once for the module."""
    return {g: (acopf.function_model(grid(g), hessian=True), acopf.function_model(grid(g), nlp="expr", branch_params=True)) for g in OHM_GRIDS}


# ------------------------------------------------------------------------------------------------ 1. against the expression twin
@pytest.mark.parametrize("name", OHM_GRIDS)
def test_ohm_twins_against_the_expression_twin(ohm_pairs, name):
    fk, fe = ohm_pairs[name]
    nl = fk.acopf_model.nl
    assert len(fk.nlp.device[2]) == 8 * nl and np.array_equal(fk.nlp.device[2], fe.nlp.device[2][:8 * nl]) and fe.nlp.n_params == 8 * nl
    for rep, x, lam, dc in points(fk, 11):
        de = np.concatenate([dc, np.zeros(len(fe.nlp.device[2]) - 8 * nl)])          # (the tape's literal constants follow the parameters)
        gk, ge = block_gradient(fk, x, lam), block_gradient(fe, x, lam)[:8 * nl]
        uk, wk = block_cross(fk, x, lam, dc)
        ue, we = block_cross(fe, x, lam, de)
        eg, eu, ew = rel_err(gk, ge), rel_err(uk, ue), rel_err(wk, we)
        print("%s point %d: rel err gradient %.3e, u %.3e, w %.3e (bar %.1e)" % (name, rep, eg, eu, ew, LIBM_BAR))
        assert gk.shape == (8 * nl,) and uk.shape == (fk.n,) and wk.shape == (fk.m,)
        assert np.any(uk != 0.0) and np.any(wk != 0.0) and np.any(gk != 0.0)
        assert eg <= LIBM_BAR and eu <= LIBM_BAR and ew <= LIBM_BAR, (name, rep, eg, eu, ew)


# ------------------------------------------------------------------------------------------------ 2. independent of both twins
def _moved(fm, rebuild, x, lam, dc):
    """w = g(dpar + dc) - g(dpar) and u = -(J(dpar + dc) - J(dpar))' lam of the block, from eval_g / eval_jac_g of the models built on
    dpar and on dpar + dc (`rebuild` makes the second)."""
    f2 = rebuild(dc)
    assert np.array_equal(f2.nlp.device[2], fm.nlp.device[2] + dc)
    w = f2.eval_g(x, np.zeros(fm.m)) - fm.eval_g(x, np.zeros(fm.m))
    J = sensitivity.dense_jacobian(f2, x) - sensitivity.dense_jacobian(fm, x)
    return -(J.T @ lam), w


def _assert_linear(tag, fm, rebuild, seed):
    for rep, x, lam, dc in points(fm, seed):
        u, w = block_cross(fm, x, lam, dc)
        ru, rw = _moved(fm, rebuild, x, lam, dc)
        bu, bw = PARITY * max(1.0, float(np.abs(ru).max())), PARITY * max(1.0, float(np.abs(rw).max()))
        g = block_gradient(fm, x, lam)
        lhs, rhs = float(g @ dc), float(-(lam @ rw))
        bg = PARITY * max(1.0, abs(rhs), float(np.abs(g * dc).max()))
        print("%s point %d: max |u - ref| %.3e (bar %.3e), max |w - ref| %.3e (bar %.3e), gradient . dc %.12e against -lam' w %.12e"
              % (tag, rep, float(np.abs(u - ru).max()), bu, float(np.abs(w - rw).max()), bw, lhs, rhs))
        assert np.any(u != 0.0) and (np.any(w != 0.0) or not np.any(x))      # (the dense rows start at x = 0, where w is 0)
        assert np.all(np.abs(u - ru) <= bu) and np.all(np.abs(w - rw) <= bw), (tag, rep)
        assert abs(lhs - rhs) <= bg, (tag, rep, lhs, rhs)


class _OhmMoved:
    """The kernel form on the coefficients dpar + dc: the model's eight coefficient arrays replaced before the block reads them."""

    def __init__(self, case):
        self.case = case

    def __call__(self, dc):
        fm = acopf.function_model(self.case, hessian=True)
        mdl, nl = fm.acopf_model, fm.acopf_model.nl
        for q, key in enumerate(("k_ff_p", "k_ff_q", "k_tt_p", "k_tt_q", "a_f", "b_f", "a_t", "b_t")):
            setattr(mdl, key, getattr(mdl, key) + dc[q * nl:(q + 1) * nl])
        fm.nlp.device = (fm.nlp.device[0], fm.nlp.device[1], fm.nlp.device[2] + dc)
        return fm


@pytest.mark.parametrize("name", ("grid3", "grid14"))
def test_ohm_twins_by_linearity(name):
    case = grid(name)
    _assert_linear(name, acopf.function_model(case, hessian=True), _OhmMoved(case), 21)


@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=lambda s: "n%d_m%d" % s)
def test_dense_twins_by_linearity(shape):
    n, m = shape
    fm = problems.synthetic_dense_function_model(n, m, hessian=True)

    def rebuild(dc):
        pr = problems.synthetic_dense_nlp(n, m)
        pr.data["A"] += dc[:m * n].reshape(m, n)               # in place: the problem's callbacks hold these arrays
        pr.data["Q"] += dc[m * n:].reshape(m, n)
        f2 = problems.synthetic_dense_function_model(n, m, hessian=True)
        f2.nlp.eval_g, f2.nlp.eval_jac_g = pr.eval_g, pr.eval_jac_g
        f2.nlp.device = (f2.nlp.device[0], f2.nlp.device[1], f2.nlp.device[2] + dc)
        return f2
    _assert_linear("dense %r" % (shape,), fm, rebuild, 31)


def test_dense_twin_formulas_entry_by_entry():
    """out[A_ij] = (-lam_i) x_j, out[Q_ij] = (-lam_i) (x_j^2 / 2); a unit direction in A_ij gives w = x_j e_i, u = -lam_i e_j."""
    n, m = 7, 3
    fm = problems.synthetic_dense_function_model(n, m, hessian=True)
    rng = np.random.default_rng(2)
    x, lam = rng.standard_normal(n), rng.standard_normal(m)
    g = fm.nlp.data_gradient(x, lam)
    assert np.array_equal(g[:m * n].reshape(m, n), np.outer(-lam, x)) and np.array_equal(g[m * n:].reshape(m, n), np.outer(-lam, 0.5 * (x * x)))
    dc = np.zeros(2 * m * n)
    dc[1 * n + 4] = 1.0
    u, w = fm.nlp.data_cross(x, lam, dc)
    assert w.tolist() == [0.0, x[4], 0.0] and u[4] == -lam[1] and np.count_nonzero(u) == 1
    with pytest.raises(ValueError):
        fm.nlp.data_cross(x, lam, dc[:-1])


# ------------------------------------------------------------------------------------------------ 3. defaults unchanged
def test_the_defaults_carry_no_twin():
    case = grid("grid3")
    plain, hess = acopf.function_model(case), acopf.function_model(case, hessian=True)
    assert plain.nlp.data_cross is None and plain.nlp.data_gradient is None and plain.nlp.eval_hess is None
    assert plain.nlp.device[0] == "acopf_ohm" and hess.nlp.device[0] == "acopf_ohm_hess"
    assert callable(hess.nlp.data_cross) and callable(hess.nlp.data_gradient)
    assert all(np.array_equal(p, h) for p, h in zip(plain.nlp.device[1:], hess.nlp.device[1:]))
    dp, dh = problems.synthetic_dense_function_model(12, 5), problems.synthetic_dense_function_model(12, 5, hessian=True)
    assert dp.nlp.data_cross is None and dp.nlp.data_gradient is None and dp.nlp.eval_hess is None and dp.nlp.device[0] == "dense_quadratic"
    assert dh.nlp.device[0] == "dense_quadratic_hess" and callable(dh.nlp.data_cross) and callable(dh.nlp.data_gradient)
    assert all(np.array_equal(p, h) for p, h in zip(dp.nlp.device[1:], dh.nlp.device[1:]))
    for a, b in ((plain, hess), (dp, dh)):
        assert set(vars(b.nlp)) - set(vars(a.nlp)) == {"data_cross", "data_gradient"} and set(vars(a.nlp)) <= set(vars(b.nlp))
        x = a.start_point() + 0.01
        assert np.array_equal(a.eval_g(x, np.zeros(a.m)), b.eval_g(x, np.zeros(b.m)))
        assert np.array_equal(a.nlp.rows, b.nlp.rows) and np.array_equal(a.nlp.cols, b.nlp.cols)
    blk = A.moi_evaluator.NlpBlock(np.zeros(1), np.zeros(1), [1], [1], None, None)
    assert blk.data_cross is None and blk.data_gradient is None


# ------------------------------------------------------------------------------------------------ 4. through the KKT solve
def test_kkt_reference_with_either_twin_at_a_host_slp_point(ohm_pairs):
    fk, fe = ohm_pairs["grid14"]
    nl = fk.acopf_model.nl
    fx = acopf.function_model(grid("grid14"), nlp="expr")
    mdl, res = host_run(fx, "Trust Region", max_iter=12)                  # (its first iterations restore feasibility with zero multipliers)
    x, lam = np.asarray(res.x, float), np.asarray(res.lam, float)
    rs, bs = sensitivity.working_set(fk.to_problem(), x, lam, res.mult_x_U, res.mult_x_L, tol=1e-6)
    assert rs.sum() <= (bs == 0).sum() and np.any(lam[fk.nlp_constraint_offset:] != 0.0)
    dc = np.random.default_rng(9).standard_normal(8 * nl)
    uk, wk = block_cross(fk, x, lam, dc)
    ue, we = block_cross(fe, x, lam, np.concatenate([dc, np.zeros(len(fe.nlp.device[2]) - 8 * nl)]))
    got, ref = sensitivity.kkt_reference(fk, x, lam, rs, bs, uk, wk), sensitivity.kkt_reference(fe, x, lam, rs, bs, ue, we)
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    print("grid14 after %d iterations: |W| %d, |F| %d, rel diff dx %.3e dlam %.3e dz %.3e (bar %.3e)" % (res.iter, rs.sum(), (bs == 0).sum(), *errs, KKT_BAR))
    assert np.any(ref[0] != 0.0) and max(errs) <= KKT_BAR, errs
