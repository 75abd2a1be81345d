"""Adjoint solution sensitivities on the host (include/asm_hip.h, "Adjoint solution sensitivities"): the host twins of the transposed
cross derivative (ExprBlock.data_cross_t, the Ohm's-law and dense blocks' data_cross_t) against the forward twins by the identity
dc' out = vx' u + vl' w, the dense adjoint reference against forward solves of the same dense system - data and bounds - and against
the closed forms of the parametric model.  Signs and conventions, no GPU."""
import numpy as np
import pytest

from activesetmethods_amd import acopf, problems, sensitivity
from tests.test_block_data_cpu import LIBM_BAR, block_cross
from tests.test_nlexpr_cpu import HS071_ORACLE_X
from tests.test_ohm_hess_cpu import grid
from tests.test_sensitivity_cpu import KKT_BAR, KKT_SHAPES, PARAMETRIC_VALUES, kkt_instance
from tests.test_sensitivity_gpu import _branch_case, _exact_cross_models, hs071_param_model

assert LIBM_BAR == 1e-12


def twin_models():
    out = list(_exact_cross_models()) + [("hs071 rhs parameters (again)", hs071_param_model()), ("acopf case118 branch parameters", _branch_case()),
                                          ("ohm kernel form, grid14", acopf.function_model(grid("grid14"), hessian=True)),
                                          ("dense block 23 x 7", problems.synthetic_dense_function_model(23, 7, hessian=True))]
    return out


def hs071_point():
    """(fm, x, lam, row_state, bound_state) at the hs071 solution: x the oracle's, lam the least-squares multipliers of the stationarity
    of the free variables on the working set {both rows}, x1 at its lower bound."""
    fm = hs071_param_model()
    x = np.array(HS071_ORACLE_X, float)
    rs, bs = np.array([1, 1], np.int32), np.array([-1, 0, 0, 0], np.int32)
    J = sensitivity.dense_jacobian(fm, x)
    df = fm.to_problem().eval_grad_f(x, np.zeros(4))
    lam = np.linalg.lstsq(J[:, 1:].T, df[1:], rcond=None)[0]
    return fm, x, lam, rs, bs


# ------------------------------------------------------------------------------------------------ 1. the twins: dc' out = vx' u + vl' w
@pytest.mark.parametrize("case", twin_models(), ids=lambda c: c[0])
def test_transposed_twin_identity(case):
    name, fm = case
    rng = np.random.default_rng(len(name))
    nd = len(fm.nlp.device[2])
    for rep in range(2):
        x = fm.start_point() + (0.3 if fm.n < 10 else 0.01) * rng.uniform(-1, 1, fm.n)
        lam, vx, vl, dc = rng.standard_normal(fm.m), rng.standard_normal(fm.n), rng.standard_normal(fm.m), rng.standard_normal(nd)
        out = sensitivity.model_cross_t(fm, x, lam, vx, vl)
        u, w = block_cross(fm, x, lam, dc)
        assert out.shape == (nd,) and np.any(out != 0.0)
        lhs, rhs = float(dc @ out), float(vx @ u + vl @ w)
        size = float(np.abs(dc * out).sum() + np.abs(vx * u).sum() + np.abs(vl * w).sum())
        print("%s point %d: dc'out %.15e, vx'u + vl'w %.15e, difference %.3e (bar %.3e)" % (name, rep, lhs, rhs, abs(lhs - rhs), LIBM_BAR * size))
        assert abs(lhs - rhs) <= LIBM_BAR * size, (name, rep, lhs, rhs)
        # each weight alone: the u part and the w part have their own signs
        for a, b in ((vx, np.zeros(fm.m)), (np.zeros(fm.n), vl)):
            o1 = sensitivity.model_cross_t(fm, x, lam, a, b)
            s1 = float(np.abs(dc * o1).sum() + np.abs(a * u).sum() + np.abs(b * w).sum())
            assert abs(float(dc @ o1) - float(a @ u + b @ w)) <= LIBM_BAR * max(s1, 1e-300), name


def test_transposed_twin_summation_order_and_the_const_exponent():
    """Rows before terms from 0.0 for a shared parameter; the CONST exponent of a POW yields its occurrence (closed form); no CONST node:
    empty."""
    from activesetmethods_amd import nlexpr
    from activesetmethods_amd.nlexpr import ExprBlock, parameters, variables
    x = variables(2)
    p = parameters([3.0])
    blk = ExprBlock([(p[0] * x[0] * x[1], 0.0, 0.0), (x[0] * x[1], 0.0, 0.0)], objective=p[0] * x[0] * x[0] + x[1], n=2, parameters=p)
    xv, lam, vx, vl = np.array([0.3, -0.7]), np.array([0.25, 5.0]), np.array([1.5, -2.0]), np.array([0.5, 7.0])
    out = blk.data_cross_t(xv, lam, vx, vl, -1.0)
    # row 0: g = p x0 x1 - d/dp (D_vx g) = vx0 x1 + x0 vx1, d/dp g = x0 x1; the term p x0^2: d/dp (D_vx f) = 2 x0 vx0
    row = (-lam[0]) * (vx[0] * xv[1] + xv[0] * vx[1]) + vl[0] * (xv[0] * xv[1])
    term = -1.0 * (vx[0] * xv[0] + xv[0] * vx[0])
    assert out.shape == (1,) and abs(out[0] - ((0.0 + row) + term)) <= 4 * np.finfo(float).eps * (abs(row) + abs(term))
    q = parameters([2.5])
    pw = ExprBlock([(nlexpr.pow(x[0], q[0]) + q[0] * x[1], 0.0, 0.0)], n=2, parameters=q)
    got = pw.data_cross_t(np.array([1.3, 0.4]), np.array([1.0]), np.array([1.0, 1.0]), np.array([2.0]))
    # g = x0^q + q x1:  out = vx' (-lam d/dq grad g) + vl dg/dq = -(x0^(q-1) (1 + q log x0)) - 1 + 2 (x0^q log x0 + x1)
    lx = float(np.log(1.3))
    want = -(1.3 ** 1.5 * (1.0 + 2.5 * lx)) - 1.0 + 2.0 * (1.3 ** 2.5 * lx + 0.4)
    size = 1.3 ** 1.5 * (1.0 + 2.5 * lx) + 1.0 + 2.0 * (1.3 ** 2.5 * lx + 0.4)
    assert got.shape == (1,) and abs(got[0] - want) <= 8 * np.finfo(float).eps * size
    # the entries that are not the exponent's stay finite at a base below 0; the exponent's own is NaN, as data_gradient's
    pz = ExprBlock([(nlexpr.pow(x[0], 2.0) + q[0] * x[1], 0.0, 0.0)], n=2, parameters=q)
    got = pz.data_cross_t(np.array([-1.3, 0.4]), np.array([1.0]), np.array([1.0, 1.0]), np.array([2.0]))
    assert got[0] == (-1.0) * 1.0 + 2.0 * 0.4 and np.isnan(got[1]) and np.isnan(pz.data_gradient(np.array([-1.3, 0.4]), np.array([1.0]))[1])
    nc = ExprBlock([(x[0] * x[1], 0.0, 0.0)], objective=x[0] * x[0], n=2)
    assert nc.data_cross_t(xv, np.array([1.0]), vx, np.array([1.0])).shape == (0,)


# ------------------------------------------------------------------------------------------------ 2. adjoint_reference against forward solves
def _forward_sum(gx, gl, dx, dlam):
    return float(gx @ dx + gl @ dlam), float(np.abs(gx * dx).sum() + np.abs(gl * dlam).sum())


def _check_bounds(tag, fm, x, lam, rs, bs, gx, gl, dbound):
    W, out = np.nonzero(rs == 1)[0], np.nonzero(rs == 0)[0]
    worst = 0.0
    if len(W):
        RW = np.zeros((len(W), fm.m))
        RW[np.arange(len(W)), W] = -1.0
        DX, DLAM, _ = sensitivity.kkt_reference_multi(fm, x, lam, rs, bs, np.zeros((len(W), fm.n)), RW)
        for q, i in enumerate(W):
            want, size = _forward_sum(gx, gl, DX[q], DLAM[q])
            err, bar = abs(dbound[i] - want), KKT_BAR * (abs(dbound[i]) + size)
            worst = max(worst, err / max(bar, 1e-300))
            assert err <= bar, (tag, int(i), dbound[i], want)
    print("%s: %d working rows, largest |dbound - forward| / bar = %.3f" % (tag, len(W), worst))
    if len(out):
        assert dbound[out[0]] == 0.0 and not dbound[out].any()


@pytest.mark.parametrize("shape", KKT_SHAPES, ids=lambda s: "n%d_B%d_W%d" % s)
def test_adjoint_reference_on_the_constructed_qps(shape):
    """The function store alone: no data (out is empty), the bound gradient against one forward solve per working row."""
    fm, x, lam, rs, bs, _, _ = kkt_instance(*shape)
    rng = np.random.default_rng(sum(shape))
    gx, gl = rng.standard_normal(fm.n), rng.standard_normal(fm.m)
    out, dbound, ax, al = sensitivity.adjoint_reference(fm, x, lam, rs, bs, gx, gl)
    assert out.shape == (0,) and dbound.shape == (fm.m,) and not ax[bs != 0].any() and not al[rs == 0].any()
    _check_bounds("shape %r" % (shape,), fm, x, lam, rs, bs, gx, gl, dbound)


def test_adjoint_reference_on_hs071():
    fm, x, lam, rs, bs = hs071_point()
    rng = np.random.default_rng(71)
    for rep in range(3):
        gx, gl, dc = rng.standard_normal(4), rng.standard_normal(2), rng.standard_normal(2)
        out, dbound, ax, al = sensitivity.adjoint_reference(fm, x, lam, rs, bs, gx, gl)
        u, w = block_cross(fm, x, lam, dc)
        dx, dlam, _ = sensitivity.kkt_reference(fm, x, lam, rs, bs, u, w)
        want, size = _forward_sum(gx, gl, dx, dlam)
        got = float(out @ dc)
        print("hs071 %d: adjoint . dc %.15e, forward %.15e, difference %.3e" % (rep, got, want, abs(got - want)))
        assert np.any(out != 0.0) and abs(got - want) <= KKT_BAR * (float(np.abs(out * dc).sum()) + size), (rep, got, want)
        _check_bounds("hs071 %d" % rep, fm, x, lam, rs, bs, gx, gl, dbound)
    # a row outside the working set: exactly 0, and the adjoint state leaves it alone
    rs1 = np.array([0, 1], np.int32)
    out, dbound, ax, al = sensitivity.adjoint_reference(fm, x, lam, rs1, bs, gx, gl)
    assert dbound[0] == 0.0 and al[0] == 0.0 and dbound[1] == -al[1] != 0.0
    _check_bounds("hs071 without row 0", fm, x, lam, rs1, bs, gx, gl, dbound)


# ------------------------------------------------------------------------------------------------ 3. closed forms
@pytest.mark.parametrize("a,p", PARAMETRIC_VALUES)
def test_adjoint_reference_reproduces_the_closed_forms(a, p):
    """out[k] = gx' (dx/dc_k) + gl' (dlam/dc_k) with the closed-form derivatives of problems.parametric_function_model (the values of
    test_solution_sensitivity_reproduces_the_closed_forms), for two weight vectors."""
    fm = problems.parametric_function_model(a, p)
    s = float(np.sqrt(p))
    x, lam = np.array([s, s]), np.array([a + 1.0 + 0.5 / s, s * (1.0 - a) - 0.5])
    rs, bs = np.ones(2, np.int32), np.zeros(2, np.int32)
    want = {0: (np.zeros(2), np.array([1.0, -s])), 1: (np.full(2, 0.5 / s), np.array([-0.25 / p ** 1.5, (1.0 - a) / (2.0 * s)]))}
    for gx, gl in ((np.array([1.0, -2.0]), np.array([0.5, 3.0])), (np.array([0.0, 1.0]), np.array([-1.25, 0.0]))):
        out, dbound, ax, al = sensitivity.adjoint_reference(fm, x, lam, rs, bs, gx, gl)
        for k in range(2):
            w = float(gx @ want[k][0] + gl @ want[k][1])
            assert abs(out[k] - w) <= KKT_BAR * max(1.0, abs(w)), (k, out[k], w)
        assert np.array_equal(dbound, -al)


def test_the_header_declares_the_adjoint_entries():
    import os
    from activesetmethods_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "asm_hip.h")).read()
    for name in ("asm_eval_data_cross_t", "asm_solution_adjoint", "asm_solution_adjoint_multi", "asm_batch_solution_adjoint"):
        assert "int %s(" % name in text and name in _lib.PROTOTYPES
