"""The Hessian of the Lagrangian on the host (include/asm_hip.h, "Hessian of the Lagrangian"): the pattern rule, the function-store part
of the reference (MOI_wrapper.jl:748-774, 946-978), the host twin of the device kernels (nlexpr.py: ExprBlock.hessian_values) against
closed forms and against torch's autograd Hessian of the same expression graphs, and the product.  No GPU."""
import numpy as np
import pytest

from activesetmethods_amd import acopf, nlexpr, problems
from activesetmethods_amd.moi_evaluator import FunctionModel, NlpBlock, ScalarFunction, hessian_matrix, hessian_product, lagrangian_hessian
from activesetmethods_amd.nlexpr import (ExprBlock, variables, sin, cos, exp, log, sqrt, tan, asin, acos, atan, sinh, cosh, tanh,
                                         log10, log2, log1p, expm1, cbrt, minimum, maximum)
from tests.test_nlexpr_cpu import HS071_ORACLE_X

INF = float("inf")
PARITY = 1e-10                 # the project's parity bar (BASELINE.json north star)


def _pairs(e, n=3):
    r, c = ExprBlock([(e, 0.0, 0.0)], n=n).hessian_structure()
    return list(zip((r - 1).tolist(), (c - 1).tolist()))


def test_pattern_rule_on_hand_cases():
    x = variables(3)
    assert _pairs(x[0] + x[1] * x[2]) == [(2, 1)]
    assert _pairs(2.0 * x[0] - x[1] + 3.0) == []
    assert _pairs(sin(x[0]) * x[1]) == [(0, 0), (1, 0)]
    assert _pairs(x[0] / x[1]) == [(1, 0), (1, 1)]
    assert _pairs(x[0] ** 1) == []
    assert _pairs(x[0] ** 2) == [(0, 0)] and _pairs(abs(x[0] + x[1])) == [(0, 0), (1, 0), (1, 1)]
    assert _pairs(nlexpr.pow(x[0], x[2])) == [(0, 0), (2, 0), (2, 2)] and _pairs(nlexpr.pow(x[0], 2.5)) == [(0, 0)]
    assert _pairs(minimum(x[0] * x[1], x[2])) == [(1, 0)] and _pairs(3.0 * (x[0] * x[1])) == [(1, 0)]
    blk = ExprBlock([(x[0] * x[1], 0.0, 0.0), (x[1] * x[0] + x[2] * x[2], 0.0, 0.0)], objective=x[0] * x[1] + x[2], n=3)
    r, c = blk.hessian_structure()
    assert list(zip(r.tolist(), c.tolist())) == [(2, 1), (3, 3)]              # two rows and a term share (2, 1): one entry
    # the shared entry sums its rows, then the term
    v = blk.hessian_values(np.array([0.3, 0.7, 1.1]), 0.5, np.array([2.0, -3.0]))
    assert v.tolist() == [(0.0 + 2.0 * 1.0) + -3.0 * 1.0 + 0.5 * 1.0, -3.0 * 2.0]


def store_model(nlp=None, sense="MAX_SENSE"):
    """Quadratic objective and quadratic <=, >=, == rows behind one linear row: a repeated term, an (i, j) with i < j."""
    fm = FunctionModel(3, -2 * np.ones(3), 2 * np.ones(3))
    fm.sense = sense
    fm.objective = ScalarFunction(1.0, [(1.0, 2)], [(2.0, 1, 1), (1.5, 1, 3), (1.5, 1, 3), (-1.0, 3, 2)])
    fm.add_constraint(ScalarFunction(0.0, [(1.0, 1), (1.0, 3)]), "le", 4.0)
    fm.add_constraint(ScalarFunction(0.0, [(1.0, 1)], [(1.0, 2, 2), (0.5, 1, 2)]), "le", 3.0)
    fm.add_constraint(ScalarFunction(0.0, [], [(3.0, 3, 1)]), "ge", -5.0)
    fm.add_constraint(ScalarFunction(0.5, [(2.0, 3)], [(-2.0, 2, 3), (-2.0, 2, 3)]), "eq", 0.5)
    fm.nlp = nlp
    return fm


def test_function_store_part_is_the_reference_rule():
    fm = store_model()
    assert fm.hessian_lagrangian_structure() == [(1, 1), (1, 3), (1, 3), (3, 2), (2, 2), (1, 2), (3, 1), (2, 3), (2, 3)]
    lam = np.array([7.0, 0.25, -1.5, 3.0])                # lam[0] belongs to the linear row
    x = np.array([0.1, 0.2, 0.3])
    for sigma in (1.0, 0.0, 0.5):
        s = sigma * -1.0                                   # obj_factor *= objective_scale (MAX_SENSE)
        want = [s * 2.0, s * 1.5, s * 1.5, s * -1.0, 0.25 * 1.0, 0.25 * 0.5, -1.5 * 3.0, 3.0 * -2.0, 3.0 * -2.0]
        assert fm.eval_hessian_lagrangian(x, sigma, lam, np.zeros(9)).tolist() == want
    # an NLP objective overrides the store's: its terms contribute nothing; the block's entries follow the rows'
    X = variables(3)
    fn = store_model(ExprBlock([(X[0] * X[2], 0.0, 1.0)], objective=X[1] * X[1] * X[0], n=3))
    assert fn.hessian_lagrangian_structure() == [(2, 2), (1, 2), (3, 1), (2, 3), (2, 3), (2, 1), (2, 2), (3, 1)]
    lam5 = np.append(lam, 0.75)
    got = fn.eval_hessian_lagrangian(x, 1.0, lam5, np.zeros(8))
    assert got.tolist() == [0.25, 0.125, -4.5, -6.0, -6.0, -1.0 * (2 * 0.2), -1.0 * (2 * 0.1), 0.75]
    # a block without second derivatives announces none
    blk = NlpBlock([0.0], [1.0], [1], [1], lambda x, g: g, lambda x, v: v)
    with pytest.raises(ValueError, match="announces no Hessian"):
        store_model(blk).hessian_lagrangian_structure()
    with pytest.raises(ValueError, match="announces no Hessian"):
        store_model(blk).eval_hessian_lagrangian(x, 1.0, lam5, np.zeros(9))


def dense_hessian(fm, x, sigma, lam):
    h = fm.hessian_lagrangian_structure()
    v = fm.eval_hessian_lagrangian(np.asarray(x, float), sigma, np.asarray(lam, float), np.zeros(len(h)))
    H = hessian_matrix([r for r, _ in h], [c for _, c in h], v, fm.n)
    assert np.array_equal(H, H.T)                          # symmetric by construction of the storage
    return H


def test_hs071_against_the_closed_form():
    fm = problems.hs071_function_model()
    for x in (fm.start_point(), np.array(HS071_ORACLE_X)):
        for sigma, lam in ((1.0, np.array([0.3, -0.7])), (0.0, np.array([1.0, 0.0])), (2.5, np.zeros(2))):
            x1, x2, x3, x4 = x
            Hf = np.zeros((4, 4))
            Hf[0, 0] = 2 * x4
            Hf[0, 1] = Hf[1, 0] = Hf[0, 2] = Hf[2, 0] = x4
            Hf[0, 3] = Hf[3, 0] = 2 * x1 + x2 + x3
            Hf[1, 3] = Hf[3, 1] = Hf[2, 3] = Hf[3, 2] = x1
            Hg = np.array([[0, x3 * x4, x2 * x4, x2 * x3], [x3 * x4, 0, x1 * x4, x1 * x3], [x2 * x4, x1 * x4, 0, x1 * x2], [x2 * x3, x1 * x3, x1 * x2, 0]])
            want = sigma * Hf + lam[0] * Hg + lam[1] * 2.0 * np.eye(4)
            got = dense_hessian(fm, x, sigma, lam)
            assert np.all(np.abs(got - want) <= 1e-14 * np.maximum(1.0, np.abs(want))), (x, sigma, got - want)
    # the SLP sign convention: f - lam' g
    x, lam = fm.start_point(), np.array([0.3, -0.7])
    assert np.array_equal(lagrangian_hessian(fm, x, lam), dense_hessian(fm, x, 1.0, -lam))


# ---------------------------------------------------------------- an independent second derivative: torch autograd on the same graphs
def _torch_value(root, z):
    """The value of the expression graph `root` with variable j read from z[j] (a dict of torch scalars), float64 on the CPU."""
    import torch
    t = lambda c: torch.tensor(float(c), dtype=torch.float64)
    un = {nlexpr.NEG: torch.neg, nlexpr.SQRT: torch.sqrt, nlexpr.EXP: torch.exp, nlexpr.LOG: torch.log, nlexpr.SIN: torch.sin,
          nlexpr.COS: torch.cos, nlexpr.ABS: torch.abs, nlexpr.TAN: torch.tan, nlexpr.ASIN: torch.asin, nlexpr.ACOS: torch.acos,
          nlexpr.ATAN: torch.atan, nlexpr.SINH: torch.sinh, nlexpr.COSH: torch.cosh, nlexpr.TANH: torch.tanh, nlexpr.LOG10: torch.log10,
          nlexpr.LOG2: torch.log2, nlexpr.LOG1P: torch.log1p, nlexpr.EXPM1: torch.expm1,
          nlexpr.CBRT: lambda u: torch.sign(u) * torch.abs(u) ** (1.0 / 3.0)}
    bi = {nlexpr.ADD: torch.add, nlexpr.SUB: torch.sub, nlexpr.MUL: torch.mul, nlexpr.DIV: torch.div, nlexpr.POW: torch.pow,
          nlexpr.ATAN2: torch.atan2, nlexpr.MIN: lambda u, y: torch.where(y < u, y, u), nlexpr.MAX: lambda u, y: torch.where(y > u, y, u)}
    memo, stack = {}, [(root, False)]
    while stack:                                           # post-order without recursion
        e, done = stack.pop()
        if id(e) in memo:
            continue
        if not done:
            stack.append((e, True))
            stack += [(c, False) for c in e.args if id(c) not in memo]
            continue
        a = [memo[id(c)] for c in e.args]
        if e.op == nlexpr.CONST:
            v = t(e.arg)
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


def _variables_of(root):
    seen, out, stack = set(), set(), [root]
    while stack:
        e = stack.pop()
        if id(e) in seen:
            continue
        seen.add(id(e))
        if e.op == nlexpr.VAR:
            out.add(e.arg)
        stack += list(e.args)
    return sorted(out)


def torch_hessian(fm, x, sigma, lam, whole, rows=None):
    """hess of sigma * f + lam' g by torch.autograd.functional.hessian, float64 on the CPU.  whole: one call on the Lagrangian as a function
    of all of x.  Otherwise one call per row and term, each as a function of its own variables, weighted and summed (the Hessian is
    linear in the rows; a case118-sized Lagrangian in one graph would need n passes over all of its nodes); `rows`, a dict, keeps
    those unweighted Hessians at x for the next call."""
    import torch
    from torch.autograd.functional import hessian
    blk, n = fm.nlp, fm.n
    R = blk.tape.R
    w = [float(lam[fm.nlp_constraint_offset + r]) for r in range(R)] + [sigma * fm.objective_scale] * blk.tape.T
    H = np.zeros((n, n))
    # the function store: quadratic terms of the objective (unless overridden) and of the rows, from their definition
    for f, row in fm._hessian_functions():
        wf = sigma * fm.objective_scale if row is None else float(lam[row])

        def q(z, f=f):
            return sum(((0.5 * c if a == b else c) * z[a - 1] * z[b - 1] for c, a, b in f.quadratic), torch.zeros((), dtype=torch.float64))
        if f.quadratic:
            H += wf * hessian(q, torch.tensor(np.asarray(x, float))).numpy()
    xt = torch.tensor(np.asarray(x, float))
    if whole:
        def lagr(z):
            zz = {j: z[j] for j in range(n)}
            return sum((wi * _torch_value(e, zz) for wi, e in zip(w, blk.exprs)), torch.zeros((), dtype=torch.float64))
        return H + hessian(lagr, xt).numpy()
    for wi, e in zip(w, blk.exprs):
        vs = _variables_of(e)
        if not vs:
            continue
        key = id(e)
        if rows is None or key not in rows:
            He = hessian(lambda z: _torch_value(e, {j: z[i] for i, j in enumerate(vs)}), xt[vs]).numpy()
            if rows is not None:
                rows[key] = He
        else:
            He = rows[key]
        H[np.ix_(vs, vs)] += wi * He
    return H


def all_ops_model(sense="MIN_SENSE"):
    """Every op of the tape at least once, arguments away from ties of min / max, the kink of abs and domain edges for x in [0.4, 1.1]^4."""
    x = variables(4)
    fm = FunctionModel(4, 0.4 * np.ones(4), 1.1 * np.ones(4))
    fm.sense = sense
    fm.add_constraint(ScalarFunction(0.0, [(1.0, 1)], [(2.0, 1, 1), (-1.0, 2, 4)]), "le", 5.0)
    fm.nlp = ExprBlock([
        (sin(x[0]) * cos(x[1]) + exp(0.3 * x[2]) - log(2 + x[3] * x[3]), -INF, 9.0),
        (sqrt(1 + x[0] ** 2) / (1.5 + x[1] * x[1]) + x[2] ** 3 - (-x[3]) ** -2, -INF, 9.0),
        (abs(x[0] * x[1] - 3) * x[2] - (-(x[0] * x[3])), -INF, 9.0),
        (tan(0.5 * x[0] * x[1]) + asin(0.5 * x[2] * x[3]) + acos(0.4 * x[0] * x[3]), -INF, 9.0),
        (atan(x[0] * x[1]) + sinh(x[1] * x[2]) + cosh(x[2] - x[3]) + tanh(x[0] * x[3]), -INF, 9.0),
        (log10(1 + x[0] * x[1]) + log2(2 + x[2] * x[3]) + log1p(x[0] * x[0]) * expm1(0.5 * x[1]) + cbrt(1.5 + x[2] * x[0]), -INF, 9.0),
        (nlexpr.pow(1 + x[0] * x[0], x[1]) + nlexpr.pow(2 + x[2], 1.5) + atan(x[0] * x[1], 2 + x[3]), -INF, 9.0),
        (minimum(x[0] * x[1], x[2] * x[3] + 5) * maximum(x[1] * x[1], x[3] - 5), -INF, 9.0),
    ], objective=x[0] * x[1] * x[2] + exp(x[3]) * x[0] + nlexpr.pow(x[1], 3.0), n=4)
    assert set(fm.nlp.tape.op.tolist()) == set(range(nlexpr.OP_COUNT))
    return fm


def arithmetic_model(sense="MIN_SENSE"):
    """ADD..POWI, ABS, MIN and MAX only (device and twin agree bit for bit), behind one quadratic row of the store."""
    x = variables(4)
    fm = FunctionModel(4, 0.4 * np.ones(4), 1.1 * np.ones(4))
    fm.sense = sense
    fm.add_constraint(ScalarFunction(0.0, [(1.0, 1)], [(2.0, 1, 1), (-1.0, 2, 4), (0.3, 4, 2)]), "ge", -5.0)
    fm.nlp = ExprBlock([
        (x[0] * x[1] * x[2] / (1.5 + x[3] * x[3]) - x[0] ** 3, -INF, 9.0),
        (abs(x[0] * x[1] - 3) * x[2] - (-(x[0] * x[3])) + x[1] ** -2, -INF, 9.0),
        (minimum(x[0] * x[1], x[2] * x[3] + 5) * maximum(x[1] * x[1], x[3] - 5) + x[2] ** 5 / x[0], -INF, 9.0),
        ((x[0] + x[1]) ** 2 * (x[2] - x[3]) ** -1, -INF, 9.0),
    ], objective=x[0] * x[1] * x[2] + x[3] ** 4 * x[0] + abs(x[1] * x[1] - x[2]) / x[3], n=4)
    return fm


def parity_cases():
    """(name, function model, x, whole-Lagrangian autograd): the models of the parity tests, seeded points."""
    rng = np.random.default_rng(2024)
    out = [("all ops %d" % k, all_ops_model(s), rng.uniform(0.4, 1.1, 4), True) for k, s in enumerate(("MIN_SENSE", "MAX_SENSE", "MIN_SENSE"))]
    te = problems.toy_expr_function_model()
    out += [("toy", te, np.array([-1.3, 0.8]), True), ("toy start", te, te.start_point() + 0.5, True)]
    pf = problems.parametric_function_model(0.5, 4.0)
    out += [("parametric", pf, pf.start_point(), True), ("parametric 2", pf, np.array([2.1, 1.9]), True)]
    fe = acopf.function_model(acopf.synthetic_case("case118", 1, 0.5), nlp="expr")
    out.append(("acopf case118 expr", fe, fe.start_point(), False))
    return out


@pytest.mark.parametrize("case", parity_cases(), ids=lambda c: c[0])
def test_host_twin_against_torch_autograd(case):
    name, fm, x, whole = case
    rng = np.random.default_rng(len(name))
    rows = {}
    for sigma in (1.0, 0.0):
        lam = rng.standard_normal(fm.m)
        got = dense_hessian(fm, x, sigma, lam)
        want = torch_hessian(fm, x, sigma, lam, whole, rows)
        bar = PARITY * max(1.0, float(np.abs(want).max()))
        err = float(np.abs(got - want).max())
        print("%s sigma %g: max |H_twin - H_torch| = %.3e, bar %.3e, max |H| = %.3e" % (name, sigma, err, bar, np.abs(want).max()))
        assert np.all(np.abs(got - want) <= bar), (name, sigma, err, bar)            # every entry of the n x n matrix
        assert np.any(want != 0.0)


@pytest.mark.parametrize("case", parity_cases(), ids=lambda c: c[0])
def test_product_equals_the_dense_matrix_times_v(case):
    name, fm, x, _ = case
    rng = np.random.default_rng(len(name) + 5)
    lam, v = rng.standard_normal(fm.m), rng.standard_normal(fm.n)
    want = dense_hessian(fm, x, 1.0, lam) @ v
    got = fm.hessian_lagrangian_product(x, 1.0, lam, v)
    assert np.all(np.abs(got - want) <= PARITY * max(1.0, float(np.abs(want).max())))
    h = fm.hessian_lagrangian_structure()
    vals = fm.eval_hessian_lagrangian(x, 1.0, lam, np.zeros(len(h)))
    assert np.array_equal(got, hessian_product([r for r, _ in h], [c for _, c in h], vals, v))
    # by hand on a tiny pattern with a duplicate, an upper-triangle entry and a diagonal one: entry order per variable
    got = hessian_product([1, 1, 2, 1], [2, 2, 2, 3], [0.5, 0.25, 3.0, -1.0], [1.0, 2.0, 4.0])
    assert got.tolist() == [(0.0 + 0.5 * 2.0) + 0.25 * 2.0 + -1.0 * 4.0, (0.0 + 0.5 * 1.0) + 0.25 * 1.0 + 3.0 * 2.0, 0.0 + -1.0 * 1.0]
