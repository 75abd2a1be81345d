"""Solution sensitivities on the host (include/asm_hip.h, "Cross derivatives of an expression block", "The KKT solve on a working
set"): the host twin of asm_eval_data_cross against torch's autograd on the same expression graphs, the dense KKT reference against
the closed forms of the parametric model, the NumPy twin of the device's projected conjugate gradients against that reference on
constructed QPs, and the working set of known solutions.  No GPU."""
import struct

import numpy as np
import pytest

from activesetmethods_amd import nlexpr, problems, sensitivity
from activesetmethods_amd.moi_evaluator import FunctionModel, ScalarFunction
from activesetmethods_amd.nlexpr import ExprBlock, parameters, variables
from tests.test_nlexpr_cpu import HS071_ORACLE_X
from tests.test_nlhess_cpu import PARITY, all_ops_model
from tests.test_nlparams_cpu import random_param_block

INF = float("inf")
PARAMETRIC_VALUES = ((0.5, 4.0), (0.7, 5.0), (0.5, 5.0))     # the (a, p) of the parameter tests

# kkt_pcg against kkt_reference on KKT_SHAPES: the largest relative error test_kkt_pcg_against_the_reference measures (it prints every
# figure; the worst is dx of shape (33, 1, 1)).  The device bar of tests/test_sensitivity_gpu.py is 10 x this, not below 1e-12.
TWIN_ERR_MEASURED = 1.51e-13
KKT_BAR = max(10.0 * TWIN_ERR_MEASURED, 1e-12)
# (n, |B|, |W|): no rows (plain CG) | a vertex (no CG) | the ldn pitch boundary | either side of the 64-wide Cholesky step | three panel
# steps and a null space of 50
KKT_SHAPES = ((8, 0, 0), (8, 3, 5), (33, 1, 1), (96, 10, 63), (96, 10, 65), (200, 20, 130))


# ------------------------------------------------------------------------------------------------ data_cross against torch autograd
def _dpar_index(blk):
    """node -> dpar slot of every CONST node of the block's graphs: a parameter by identity, a constant by its value."""
    P = blk.n_params
    by_value = {struct.pack("<d", float(v)): P + k for k, v in enumerate(blk.tape.consts[P:])}
    by_id = {id(p): k for k, p in enumerate(blk.params)}
    return lambda e: by_id[id(e)] if id(e) in by_id else by_value[struct.pack("<d", float(e.arg))]


def _torch_value(root, z, c, slot):
    """The value of the graph `root` with variable j read from z[j] and every CONST node from c[its dpar slot], the CONST exponent
    of a POW included."""
    import torch
    un = {nlexpr.NEG: torch.neg, nlexpr.SQRT: torch.sqrt, nlexpr.EXP: torch.exp, nlexpr.LOG: torch.log, nlexpr.SIN: torch.sin,
          nlexpr.COS: torch.cos, nlexpr.ABS: torch.abs, nlexpr.TAN: torch.tan, nlexpr.ASIN: torch.asin, nlexpr.ACOS: torch.acos,
          nlexpr.ATAN: torch.atan, nlexpr.SINH: torch.sinh, nlexpr.COSH: torch.cosh, nlexpr.TANH: torch.tanh, nlexpr.LOG10: torch.log10,
          nlexpr.LOG2: torch.log2, nlexpr.LOG1P: torch.log1p, nlexpr.EXPM1: torch.expm1,
          nlexpr.CBRT: lambda u: torch.sign(u) * torch.abs(u) ** (1.0 / 3.0)}
    bi = {nlexpr.ADD: torch.add, nlexpr.SUB: torch.sub, nlexpr.MUL: torch.mul, nlexpr.DIV: torch.div, nlexpr.POW: torch.pow,
          nlexpr.ATAN2: torch.atan2, nlexpr.MIN: lambda u, y: torch.where(y < u, y, u), nlexpr.MAX: lambda u, y: torch.where(y > u, y, u)}
    memo, stack = {}, [(root, False)]
    while stack:
        e, done = stack.pop()
        if id(e) in memo:
            continue
        if not done:
            stack.append((e, True))
            stack += [(a, False) for a in e.args if id(a) not in memo]
            continue
        a = [memo[id(q)] for q in e.args]
        if e.op == nlexpr.CONST:
            v = c[slot(e)]
        elif e.op == nlexpr.VAR:
            v = z[e.arg]
        elif e.op == nlexpr.POWI:
            v = a[0] ** int(e.arg)
        elif e.op in bi:
            v = bi[e.op](a[0], a[1])
        else:
            v = un[e.op](a[0])
        memo[id(e)] = v
    return memo[id(root)]


def torch_data_cross(blk, x, lam, dc, scale):
    """(u, w): d/dc (grad_x (scale * f - lam' g)) . dc and (dg/dc) . dc by torch.autograd, float64 on the CPU."""
    import torch
    from torch.autograd.functional import jacobian
    slot, R = _dpar_index(blk), blk.tape.R
    z = torch.tensor(np.asarray(x, float), requires_grad=True)
    c0 = torch.tensor(np.asarray(blk.device[2], float))
    wt = [-float(v) for v in lam[:R]] + [float(scale)] * blk.tape.T

    def grad_x(c):
        L = sum((w * _torch_value(e, z, c, slot) for w, e in zip(wt, blk.exprs)), torch.zeros((), dtype=torch.float64))
        return torch.autograd.grad(L, z, create_graph=True, allow_unused=True)[0]

    def rows(c):
        return torch.stack([_torch_value(e, z, c, slot) + 0.0 * c.sum() for e in blk.exprs[:R]]) if R else torch.zeros(0, dtype=torch.float64)
    u = jacobian(grad_x, c0).detach().numpy() @ dc
    w = jacobian(rows, c0).detach().numpy() @ dc if R else np.zeros(0)
    return u, w


def cross_cases():
    rng = np.random.default_rng(77)
    out = [("all ops %s" % s, all_ops_model(s).nlp, rng.uniform(0.4, 1.1, 4), -1.0 if s == "MAX_SENSE" else 1.0) for s in ("MIN_SENSE", "MAX_SENSE")]
    for a, p in PARAMETRIC_VALUES:
        out.append(("parametric %g %g" % (a, p), problems.parametric_function_model(a, p).nlp, np.array([2.1, 1.9]), 1.0))
    for seed in range(4):
        v = np.random.default_rng(seed + 3).uniform(-1.5, 1.5, 3)
        blk, n = random_param_block(seed, v, exact=seed % 2 == 1)
        out.append(("random %d" % seed, blk, rng.uniform(-1, 1, n), 1.0))
    x = variables(2)
    q = parameters([2.5, 1.7])                                   # parameters as exponents: of a variable, of a product with a parameter, in a term
    pw = ExprBlock([(nlexpr.pow(x[0], q[0]) + q[0] * x[1], 0.0, 0.0), (nlexpr.pow(x[1] * q[1], q[0]) - x[0], 0.0, 0.0)],
                   objective=nlexpr.pow(x[0] + x[1], q[1]) * q[0] + nlexpr.pow(x[1], 1.5), n=2, parameters=q)
    for s in (1.0, -1.0):
        out.append(("parameter exponent %g" % s, pw, np.array([1.3, 0.4]), s))
    return out


@pytest.mark.parametrize("case", cross_cases(), ids=lambda c: c[0])
def test_data_cross_against_torch_autograd(case):
    name, blk, x, scale = case
    rng = np.random.default_rng(len(name))
    lam, dc = rng.standard_normal(blk.m), rng.standard_normal(len(blk.device[2]))
    u, w = blk.data_cross(x, lam, dc, scale)
    ur, wr = torch_data_cross(blk, x, lam, dc, scale)
    assert u.shape == (blk.n_var,) and w.shape == (blk.m,)
    eu, ew = float(np.abs(u - ur).max()), float(np.abs(w - wr).max()) if blk.m else 0.0
    print("%s: |u - u_torch| = %.3e (max |u| %.3e), |w - w_torch| = %.3e" % (name, eu, np.abs(ur).max(), ew))
    assert eu <= PARITY * max(1.0, float(np.abs(ur).max())), (name, eu)
    assert ew <= PARITY * max(1.0, float(np.abs(wr).max()) if blk.m else 1.0), (name, ew)
    assert np.any(ur != 0.0)


def test_data_cross_summation_order_and_the_const_exponent():
    """A parameter shared by two rows and a term; a row without constants; u[j] sums rows before terms from 0.0; the CONST exponent of
    a POW takes its tangent like any other constant (closed form); a tape without CONST node gives zeros."""
    x = variables(2)
    p = parameters([3.0])
    blk = ExprBlock([(p[0] * x[0] * x[1], 0.0, 0.0), (x[0] * x[1], 0.0, 0.0), (x[0] * (p[0] * x[0]), 0.0, 0.0)],
                    objective=p[0] * x[0] * x[0] + x[1], n=2, parameters=p)
    xv, lam, dc = np.array([0.3, -0.7]), np.array([0.25, 5.0, -2.0]), np.array([1.5])
    u, w = blk.data_cross(xv, lam, dc, -1.0)
    assert w.tolist() == [1.5 * xv[0] * xv[1], 0.0, xv[0] * (1.5 * xv[0])]
    want0 = 0.0 + (-lam[0]) * (1.5 * xv[1])                              # row 0, then row 2, then the term
    want0 = want0 + (-lam[2]) * (1.5 * xv[0] + 1.5 * xv[0])
    want0 = want0 + -1.0 * (1.5 * xv[0] + 1.5 * xv[0])
    assert u[0] == want0 and u[1] == (-lam[0]) * (1.5 * xv[0])
    q = parameters([2.5])
    pw = ExprBlock([(nlexpr.pow(x[0], q[0]) + q[0] * x[1], 0.0, 0.0)], n=2, parameters=q)
    u, w = pw.data_cross(np.array([1.3, 0.4]), np.array([1.0]), np.array([1.0]))
    # g = x0^q + q x1:  w = dg/dq = x0^q log x0 + x1,  u = -lam d/dq grad g = -(x0^(q-1) (1 + q log x0), 1)
    lx, eps = float(np.log(1.3)), np.finfo(float).eps
    want_w, want_u0 = 1.3 ** 2.5 * lx + 0.4, -(1.3 ** 1.5 * (1.0 + 2.5 * lx))
    assert abs(w[0] - want_w) <= 8 * eps * abs(want_w) and abs(u[0] - want_u0) <= 8 * eps * abs(want_u0) and u[1] == -1.0
    # a direction that leaves the exponent alone: today's bits, finite at a base below 0
    pz = ExprBlock([(nlexpr.pow(x[0], 2.0) + q[0] * x[1], 0.0, 0.0)], n=2, parameters=q)
    u, w = pz.data_cross(np.array([-1.3, 0.4]), np.array([1.0]), np.array([1.0, 0.0]))
    assert w.tolist() == [0.4] and u.tolist() == [-0.0, -1.0]
    nc = ExprBlock([(x[0] * x[1], 0.0, 0.0)], objective=x[0] * x[0], n=2)
    u, w = nc.data_cross(xv, np.array([1.0]), np.zeros(0))
    assert not u.any() and not w.any()
    with pytest.raises(ValueError):
        blk.data_cross(xv, lam, np.zeros(3))


# ------------------------------------------------------------------------------------------------ kkt_reference: closed forms
@pytest.mark.parametrize("a,p", PARAMETRIC_VALUES)
def test_kkt_reference_on_the_parametric_model(a, p):
    """d(x*, lam*) / d(a, p) of problems.parametric_function_model with both rows active: x* = (s, s), s = sqrt(p),
    lam* = (a + 1 + 1 / (2 s), s (1 - a) - 1 / 2) (parametric_function_model's docstring), differentiated by hand."""
    fm = problems.parametric_function_model(a, p)
    s = float(np.sqrt(p))
    x, lam = np.array([s, s]), np.array([a + 1.0 + 0.5 / s, s * (1.0 - a) - 0.5])
    rs, bs = np.ones(2, np.int32), np.zeros(2, np.int32)
    want = {0: (np.zeros(2), np.array([1.0, -s])), 1: (np.full(2, 0.5 / s), np.array([-0.25 / p ** 1.5, (1.0 - a) / (2.0 * s)]))}
    for k in range(2):
        dc = np.zeros(2)
        dc[k] = 1.0
        u, w = fm.nlp.data_cross(x, lam, dc, fm.objective_scale)
        dx, dlam, dz = sensitivity.kkt_reference(fm, x, lam, rs, bs, u, w)
        wx, wl = want[k]
        assert np.all(np.abs(dx - wx) <= 1e-12 * max(1.0, np.abs(wx).max())), (k, dx, wx)
        assert np.all(np.abs(dlam - wl) <= 1e-12 * max(1.0, np.abs(wl).max())), (k, dlam, wl)
        assert not dz.any()
        px, pl, pz, info = sensitivity.kkt_pcg(fm, x, lam, rs, bs, u, w)           # a vertex: no CG iteration
        assert info["status"] == 0 and info["cg_iters"] == 0 and np.allclose(px, wx, rtol=0, atol=1e-12) and np.allclose(pl, wl, rtol=0, atol=1e-12)
    assert np.array_equal(sensitivity.predict(x, np.full(2, 0.5 / s), 0.1), x + 0.1 * (0.5 / s))


# ------------------------------------------------------------------------------------------------ constructed QPs
def kkt_instance(n, nB, nW, seed=1, diag=None, duplicate_row=False):
    """A FunctionModel of the function store alone (nlp_kind 0) whose KKT system on a working set is a well-conditioned QP:
    objective 1/2 sum d_j x_j^2 + a few off-diagonal products, d_j in [2, 9] and at most two products of size <= 0.4 per variable
    (Gershgorin: eigenvalues in [1, 10]); nW + 3 dense affine rows with normal01 coefficients (the last three outside the working
    set); B = nB variables spread over the range, at alternating bounds.  Returns (fm, x, lam, row_state, bound_state, ru, rw);
    checks that the reduced Hessian is positive definite (unless `diag` is given) and cond(A A') <= 1e4."""
    m = nW + 3
    d = 2.0 + 7.0 * problems.uniform01(100 + seed, n) if diag is None else np.asarray(diag, float)
    off = 0.8 * problems.uniform01(200 + seed, n) - 0.4
    quad = [(float(d[j]), j + 1, j + 1) for j in range(n)] + [(float(off[j]), j + 1, j + 2) for j in range(0, n - 1, 3)]
    fm = FunctionModel(n, -10.0 * np.ones(n), 10.0 * np.ones(n))
    fm.objective = ScalarFunction(0.0, [(1.0, 1)], quad)
    G = problems.normal01(300 + seed, m * n).reshape(m, n)
    if duplicate_row:
        G[1] = G[0]
    for i in range(m):
        fm.add_constraint(ScalarFunction(0.0, [(float(G[i, j]), j + 1) for j in range(n)]), "le", 1.0)
    bound_state = np.zeros(n, np.int32)
    if nB:
        where = np.linspace(0, n - 1, nB).astype(int)
        bound_state[where] = np.where(np.arange(nB) % 2 == 0, -1, 1)
    row_state = np.zeros(m, np.int32)
    row_state[:nW] = 1
    x = problems.uniform01(400 + seed, n) - 0.5
    lam = problems.normal01(500 + seed, m)
    ru, rw = problems.normal01(600 + seed, n), problems.normal01(700 + seed, m)
    F = np.nonzero(bound_state == 0)[0]
    A = G[:nW][:, F]
    if nW and not duplicate_row:
        assert np.linalg.cond(A @ A.T) <= 1e4, (n, nB, nW, np.linalg.cond(A @ A.T))
    if diag is None:
        H = sensitivity.lagrangian_hessian(fm, x, lam)
        ev = np.linalg.eigvalsh(H)
        assert ev[0] >= 1.0 and ev[-1] <= 10.0, (ev[0], ev[-1])
    return fm, x, lam, row_state, bound_state, ru, rw


def rel_err(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(1.0, np.abs(want).max())) if len(want) else 0.0


@pytest.fixture(scope="module")
def kkt_references():
    """shape -> (instance, kkt_reference's answer), computed once for the module."""
    out = {}
    for shape in KKT_SHAPES:
        inst = kkt_instance(*shape)
        out[shape] = (inst, sensitivity.kkt_reference(*inst))
    return out


def test_kkt_pcg_against_the_reference(kkt_references):
    worst = 0.0
    for shape, (inst, ref) in kkt_references.items():
        dx, dlam, dz, info = sensitivity.kkt_pcg(*inst)
        errs = [rel_err(g, w) for g, w in zip((dx, dlam, dz), ref)]
        print("shape %r: status %d, %d CG iterations, rel err dx %.3e dlam %.3e dz %.3e, res %.3e / %.3e" % ((shape, info["status"], info["cg_iters"]) + tuple(errs)
                                                                                                           + (info["res_stat"], info["res_feas"])))
        n, nB, nW = shape
        assert info["status"] == 0 and info["n_free"] == n - nB and info["n_rows"] == nW and info["dropped_pivots"] == 0
        assert (info["cg_iters"] == 0) == (n - nB == nW) and info["cg_iters"] <= 2 * (n - nB - nW) + 20
        fm, x, lam, rs, bs, ru, rw = inst
        assert not dx[bs != 0].any() and not dlam[rs == 0].any() and not dz[bs == 0].any()
        worst = max(worst, *errs)
    # the bound of the twin itself: rtol 1e-12 times the condition of the reduced Hessian (<= 10), plus the normal-equation solves at
    # cond(A A') <= 1e4 times the unit roundoff times sqrt(n): below 1e-10.  TWIN_ERR_MEASURED records what this loop printed.
    assert worst <= 1e-10, "largest relative error of kkt_pcg against kkt_reference: %.3e" % worst


def test_kkt_pcg_result_statuses():
    neg = np.full(8, 4.0)
    neg[2] = -50.0
    inst = kkt_instance(8, 0, 2, seed=3, diag=neg)
    dx, dlam, dz, info = sensitivity.kkt_pcg(*inst)
    assert info["status"] == 2 and np.all(np.isfinite(dx)) and np.all(np.isfinite(dlam))
    inst = kkt_instance(12, 2, 4, seed=4, duplicate_row=True)
    dx, dlam, dz, info = sensitivity.kkt_pcg(*inst)
    assert info["status"] == 3 and info["dropped_pivots"] == 1 and np.all(np.isfinite(dx))
    inst = kkt_instance(200, 20, 130)
    assert sensitivity.kkt_pcg(*inst, max_iter=1)[3]["status"] == 1
    fm, x, lam, rs, bs, ru, rw = kkt_instance(8, 3, 5)
    with pytest.raises(ValueError):
        sensitivity.kkt_reference(fm, x, lam, np.ones(8, np.int32), bs, ru, rw)      # |W| > |F|
    with pytest.raises(ValueError):
        sensitivity.kkt_pcg(fm, x, lam, rs, 2 * np.ones(8, np.int32), ru, rw)


# ------------------------------------------------------------------------------------------------ working sets
def test_working_set_of_known_solutions():
    pr = problems.toy_problem()
    rs, bs = sensitivity.working_set(pr, np.array([-1.0, -1.0]), np.zeros(4), np.zeros(2), np.zeros(2))
    assert rs.tolist() == [0, 1, 1, 0] and bs.tolist() == [0, 0] and rs.dtype == np.int32 and bs.dtype == np.int32
    hs = problems.hs071_problem()
    rs, bs = sensitivity.working_set(hs, np.array(HS071_ORACLE_X), np.zeros(2), np.zeros(4), np.zeros(4), tol=1e-6)
    assert rs.tolist() == [1, 1] and bs.tolist() == [-1, 0, 0, 0]
    rs, bs = sensitivity.working_set(hs, np.array([1.0, 5.0, 5.0, 1.0]), np.zeros(2), np.zeros(4), np.zeros(4))
    assert rs.tolist() == [1, 1] and bs.tolist() == [-1, 1, 1, -1]                 # the start point: 25 at its lower bound, the equality
    for a, p in PARAMETRIC_VALUES:
        pp = problems.parametric_function_model(a, p).to_problem()
        xs = problems.parametric_solution(a, p)[0]
        rs, bs = sensitivity.working_set(pp, xs, np.zeros(2), np.zeros(2), np.zeros(2))
        assert rs.tolist() == [1, 1] and bs.tolist() == [0, 0]
        assert sensitivity.working_set(pp, xs + np.array([0.0, 0.5]), np.zeros(2), np.zeros(2), np.zeros(2))[0].tolist() == [0, 0]
    with pytest.raises(ValueError):
        sensitivity.working_set(pr, np.zeros(3), np.zeros(4), np.zeros(2), np.zeros(2))
