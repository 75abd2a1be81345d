"""The expression ops after COS (include/asm_hip.h, "Expression block": abs, tan, asin, acos, atan, sinh, cosh, tanh, log10, log2,
log1p, expm1, cbrt, pow, atan(y, x), min, max) on the host: builders and encoding of activesetmethods_amd/nlexpr.py, the host twin
against closed forms and central differences, and a known-answer model through the CPU oracle.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

from activesetmethods_amd import nlexpr
from activesetmethods_amd.nlexpr import (ExprBlock, variables, sin, cos, exp, log, sqrt, tan, asin, acos, atan, sinh, cosh, tanh,
                                         log10, log2, log1p, expm1, cbrt, minimum, maximum)

INF = float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (builder, value, derivative, points inside the domain)
UNARY = [
    (abs, abs, lambda u: math.copysign(1.0, u), [-1.7, -0.3, 0.4, 2.5]),
    (tan, math.tan, lambda u: 1.0 / math.cos(u) ** 2, [-1.2, -0.1, 0.3, 1.4]),
    (asin, math.asin, lambda u: 1.0 / math.sqrt(1.0 - u * u), [-0.9, -0.2, 0.5, 0.95]),
    (acos, math.acos, lambda u: -1.0 / math.sqrt(1.0 - u * u), [-0.9, -0.2, 0.5, 0.95]),
    (atan, math.atan, lambda u: 1.0 / (1.0 + u * u), [-3.0, -0.2, 0.5, 7.0]),
    (sinh, math.sinh, math.cosh, [-2.0, -0.1, 0.6, 3.0]),
    (cosh, math.cosh, math.sinh, [-2.0, -0.1, 0.6, 3.0]),
    (tanh, math.tanh, lambda u: 1.0 / math.cosh(u) ** 2, [-2.0, -0.1, 0.6, 3.0]),
    (log10, math.log10, lambda u: 1.0 / (u * math.log(10.0)), [0.01, 0.5, 3.0, 1e4]),
    (log2, math.log2, lambda u: 1.0 / (u * math.log(2.0)), [0.01, 0.5, 3.0, 1e4]),
    (log1p, math.log1p, lambda u: 1.0 / (1.0 + u), [-0.9, -1e-9, 0.5, 30.0]),
    (expm1, math.expm1, math.exp, [-3.0, -1e-9, 0.5, 4.0]),
    (cbrt, np.cbrt, lambda u: 1.0 / (3.0 * np.cbrt(u) ** 2), [-8.0, -0.3, 0.2, 27.0]),
]
# (builder, value, gradient, points)
BINARY = [
    (nlexpr.pow, lambda u, y: u ** y, lambda u, y: (y * u ** (y - 1.0), u ** y * math.log(u)), [(0.5, 1.5), (2.0, -0.7), (3.0, 2.2)]),
    (atan, math.atan2, lambda u, y: (y / (u * u + y * y), -u / (u * u + y * y)), [(0.5, 1.5), (-2.0, -0.7), (3.0, -2.2)]),
    (minimum, min, lambda u, y: (0.0, 1.0) if y < u else (1.0, 0.0), [(0.5, 1.5), (-2.0, -0.7), (3.0, -2.2)]),
    (maximum, max, lambda u, y: (0.0, 1.0) if y > u else (1.0, 0.0), [(0.5, 1.5), (-2.0, -0.7), (3.0, -2.2)]),
]


def _row(e, n):
    """One free row e(x) over n variables: (value, dense gradient) callables of the host twin."""
    blk = ExprBlock([(e, -INF, INF)], n=n)

    def val(x):
        return float(blk.eval_g(np.asarray(x, float), np.zeros(1))[0])

    def grad(x):
        g = np.zeros(n)
        g[blk.cols - 1] = blk.eval_jac_g(np.asarray(x, float), np.zeros(len(blk.cols)))
        return g
    return val, grad


def _central(f, x, j, h=1e-6):
    xp, xm = np.array(x, float), np.array(x, float)
    s = h * max(1.0, abs(x[j]))
    xp[j] += s
    xm[j] -= s
    return (f(xp) - f(xm)) / (2 * s)


@pytest.mark.parametrize("op", UNARY, ids=["abs", "tan", "asin", "acos", "atan", "sinh", "cosh", "tanh", "log10", "log2", "log1p",
                                             "expm1", "cbrt"])
def test_unary_ops_match_closed_forms_and_central_differences(op):
    build, value, deriv, points = op
    x = variables(1)
    val, grad = _row(build(x[0]), 1)
    for u in points:
        assert abs(val([u]) - value(u)) <= 5e-16 * max(1.0, abs(value(u))), (u, val([u]), value(u))     # NumPy against libm
        d = grad([u])[0]
        assert abs(d - deriv(u)) <= 1e-14 * max(1.0, abs(deriv(u))), (u, d, deriv(u))
        fd = _central(val, [u], 0, 1e-7 if abs(u) < 0.1 else 1e-6)
        assert abs(d - fd) <= 1e-6 * max(1.0, abs(fd)), (u, d, fd)


@pytest.mark.parametrize("op", BINARY, ids=["pow", "atan2", "minimum", "maximum"])
def test_binary_ops_match_closed_forms_and_central_differences(op):
    build, value, grad_of, points = op
    x = variables(2)
    val, grad = _row(build(x[0], x[1]), 2)
    for u, y in points:
        assert abs(val([u, y]) - value(u, y)) <= 5e-16 * max(1.0, abs(value(u, y)))
        g = grad([u, y])
        assert np.allclose(g, grad_of(u, y), rtol=1e-14, atol=1e-15), (u, y, g, grad_of(u, y))
        for j in range(2):
            fd = _central(val, [u, y], j)
            assert abs(g[j] - fd) <= 1e-6 * max(1.0, abs(fd)), (u, y, j, g[j], fd)


def test_edge_rules():
    x = variables(2)
    val, grad = _row(abs(x[0]), 1)
    assert grad([0.0])[0] == 1.0 and grad([-0.0])[0] == -1.0 and val([-0.0]) == 0.0
    for build, pick in ((minimum, min), (maximum, max)):
        val, grad = _row(build(x[0], x[1]), 2)
        assert val([0.7, 0.7]) == 0.7 and np.array_equal(grad([0.7, 0.7]), [1.0, 0.0])        # a tie goes to a
        val, grad = _row(build(x[0], nlexpr.const(np.nan)), 1)
        assert val([0.7]) == 0.7 and grad([0.7])[0] == 1.0                                    # NaN on the right: a
        val, grad = _row(build(nlexpr.const(np.nan), x[0]), 1)
        assert np.isnan(val([0.7])) and grad([0.7])[0] == 0.0                                 # NaN on the left: a (the constant)
        val, grad = _row(build(x[0], x[0] * 2, x[0] - 1), 1)                                  # n-ary
        assert val([1.5]) == pick(1.5, 3.0, 0.5) and grad([1.5])[0] == (1.0 if build is minimum else 2.0)
    # a constant exponent: its adjoint (v * log(u), NaN for u < 0) lands on the CONST node and is dropped
    val, grad = _row(nlexpr.pow(x[0], 3.0), 1)
    assert val([-2.0]) == -8.0 and grad([-2.0])[0] == 12.0
    val, grad = _row(nlexpr.pow(x[0], x[1]), 2)
    g = grad([-2.0, 3.0])
    assert g[0] == 12.0 and np.isnan(g[1])
    # domain errors: NaN / inf as the math library gives them
    assert np.isnan(_row(asin(x[0]), 1)[0]([1.5])) and _row(log10(x[0]), 1)[0]([0.0]) == -INF
    assert np.isnan(_row(log1p(x[0]), 1)[0]([-2.0])) and np.isnan(_row(acos(x[0]), 1)[0]([-1.5]))


def test_encoding():
    hdr = open(os.path.join(ROOT, "include", "asm_hip.h")).read()
    codes = dict(re.findall(r"ASM_OP_(\w+) = (\d+)", hdr))
    assert int(codes.pop("COUNT")) == nlexpr.OP_COUNT == len(codes)
    for name, v in codes.items():
        assert getattr(nlexpr, name) == int(v), name
    x = variables(3)

    def ops(e):
        R, T, L, ptr, op, a, b = nlexpr.parse_ipar(ExprBlock([(e, 0.0, 0.0)], n=3).device[1])
        return op.tolist(), a.tolist(), b.tolist()
    blk = ExprBlock([(nlexpr.pow(x[0], 2.5), 0.0, 0.0)], n=3)
    assert ops(nlexpr.pow(x[0], 2.5)) == ([nlexpr.VAR, nlexpr.CONST, nlexpr.POW], [0, 0, 0], [0, 0, 1])
    assert blk.device[2].tolist() == [2.5]
    assert ops(nlexpr.pow(x[0], 3))[0][-1] == nlexpr.POW                   # pow is never rewritten to POWI
    assert ops(x[0] ** 3) == ([nlexpr.VAR, nlexpr.POWI], [0, 0], [0, 3])
    assert ops(nlexpr.pow(2, x[1])) == ([nlexpr.CONST, nlexpr.VAR, nlexpr.POW], [0, 1, 0], [0, 0, 1])
    assert ops(atan(x[1], x[2])) == ([nlexpr.VAR, nlexpr.VAR, nlexpr.ATAN2], [1, 2, 0], [0, 0, 1])
    assert ops(atan(x[1]))[0] == [nlexpr.VAR, nlexpr.ATAN]
    assert ops(minimum(x[0], x[1], x[2])) == ([nlexpr.VAR, nlexpr.VAR, nlexpr.MIN, nlexpr.VAR, nlexpr.MIN], [0, 1, 0, 2, 2], [0, 0, 1, 0, 3])
    assert ops(maximum(x[2], 1.0, x[2])) == ([nlexpr.VAR, nlexpr.CONST, nlexpr.MAX, nlexpr.MAX], [2, 0, 0, 2], [0, 0, 1, 0])
    assert ops(abs(x[0] - x[1]))[0] == [nlexpr.VAR, nlexpr.VAR, nlexpr.SUB, nlexpr.ABS]
    for build, code in ((tan, "TAN"), (asin, "ASIN"), (acos, "ACOS"), (sinh, "SINH"), (cosh, "COSH"), (tanh, "TANH"), (log10, "LOG10"),
                        (log2, "LOG2"), (log1p, "LOG1P"), (expm1, "EXPM1"), (cbrt, "CBRT")):
        assert ops(build(x[1])) == ([nlexpr.VAR, getattr(nlexpr, code)], [1, 0], [0, 0])
    with pytest.raises(TypeError):
        x[0] ** 1.5
    with pytest.raises(ValueError):
        x[0] ** 65
    with pytest.raises(TypeError):
        minimum()
    with pytest.raises(TypeError):
        nlexpr.pow(x[0], "2")


def random_ops_block(seed, n=5, rows=6, objective=True, exact=False):
    """Seeded random rows mixing the ops up to COS with the ops after it.  Arguments are wrapped away from poles and domain edges
    (asin(0.9 tanh(u)), tan(0.5 tanh(u)), pow(1 + u^2, tanh(v)), ...) so that last-bit differences of the math library stay small.
    exact=True keeps to + - * / and abs, min, max (bit-exact on the device)."""
    rng = np.random.default_rng(seed)
    x = variables(n)

    def leaf():
        return x[int(rng.integers(n))] if rng.random() < 0.75 else nlexpr.const(float(rng.uniform(-2, 2)))

    def build(depth):
        if depth == 0:
            return leaf()
        k = int(rng.choice([0, 1, 2, 5, 17, 18])) if exact else int(rng.integers(20))
        u, v = build(depth - 1), build(depth - 1)
        return [
            lambda: u + v, lambda: u * v - u, lambda: u / (1.5 + v * v), lambda: sin(u) * exp(0.3 * tanh(v)),
            lambda: sqrt(1 + u ** 2) - log(2 + cos(v)),
            lambda: abs(u) - v, lambda: tan(0.5 * tanh(u)) + v, lambda: asin(0.9 * tanh(u)) * v, lambda: acos(0.9 * tanh(u)) - v,
            lambda: atan(u) + sinh(tanh(v)), lambda: cosh(sin(u)) * v, lambda: log10(1 + u * u) - log2(2 + sin(v)),
            lambda: log1p(u * u) * expm1(0.5 * tanh(v)), lambda: cbrt(1.5 + cos(u)) + v,
            lambda: nlexpr.pow(1 + u * u, tanh(v)), lambda: nlexpr.pow(2 + cos(u), 1.5) - v, lambda: atan(u, 2 + cos(v)),
            lambda: minimum(u, v), lambda: maximum(u, v, 0.5 * u), lambda: minimum(tanh(u), 0.3) * maximum(v, -1.0),
        ][k]()
    cons = []
    for r in range(rows):
        e = build(3)
        cons.append((e, -1.0, 1.0) if r % 2 else (e, 0.5, 0.5))
    obj = None
    if objective:
        obj = build(2) * build(1) + abs(x[0]) + build(2) + (x[n - 1] if exact else nlexpr.pow(1 + x[n - 1] ** 2, 0.75))
    return ExprBlock(cons, obj, n=n), n


@pytest.mark.parametrize("seed", range(6))
def test_random_blocks_match_central_differences(seed):
    from tests.test_nlexpr_cpu import _model
    block, n = random_ops_block(seed)
    used = set(block.tape.op.tolist())
    assert len(used & set(range(nlexpr.ABS, nlexpr.OP_COUNT))) >= 5, used
    pr = _model(block, n).to_problem()
    rng = np.random.default_rng(seed + 200)
    for _ in range(2):
        x = rng.uniform(-1, 1, n)
        J = pr.eval_jac_g(x, np.zeros(pr.nnz))
        g = pr.eval_grad_f(x, np.zeros(n))
        Jd = np.zeros((pr.m, n))
        np.add.at(Jd, (pr.j_row - 1, pr.j_col - 1), J)
        for j in range(n):
            fd_g = np.array([_central(lambda z: pr.eval_g(z, np.zeros(pr.m))[i], x, j) for i in range(pr.m)])
            fd_f = _central(pr.eval_f, x, j)
            assert np.allclose(Jd[:, j], fd_g, rtol=1e-6, atol=1e-6 * max(1.0, np.abs(fd_g).max())), (j, Jd[:, j], fd_g)
            assert abs(g[j] - fd_f) <= 1e-6 * max(1.0, abs(fd_f)), (j, g[j], fd_f)


def ops_function_model(x_L=(0.25, 0.25), x_U=(3.0, 3.0), start=(2.0, 0.5)):
    """min x0^1.5 + x1^1.5 + cosh(x0 - x1)  s.t.  atan(x0) + atan(x1) == pi/2 (x0 x1 = 1), x in [0.25, 3]^2: every term is least at
    x0 = x1 = 1 along x1 = 1 / x0, so the optimum is (1, 1) with value 3.  atan(x1, x0) >= pi/4 (x1 >= x0) keeps that optimum and
    makes it a vertex, which an SLP reaches in a few steps (without it Line Search creeps along x0 x1 = 1); the other rows are
    inactive and carry every other op after COS."""
    from activesetmethods_amd.moi_evaluator import FunctionModel
    x0, x1 = variables(2)
    fm = FunctionModel(2, np.asarray(x_L, float), np.asarray(x_U, float))
    fm.start = {1: start[0], 2: start[1]}
    fm.nlp = ExprBlock([
        (atan(x0) + atan(x1), math.pi / 2, math.pi / 2),
        (abs(x0 - x1), -INF, 1.0),
        (log10(x0) + log2(x1), -3.0, INF),
        (tanh(x0) + tanh(x1), -INF, 1.99),
        (asin(x0 / 4) + acos(x1 / 4), -INF, 3.0),
        (tan(x0 / 4) + cbrt(x1), -INF, 3.0),
        (log1p(x0) + expm1(x1), -INF, 25.0),
        (sinh(x0) - x1, -INF, 12.0),
        (atan(x1, x0), math.pi / 4, 1.5),
        (minimum(x0, x1, 2.0), 0.1, INF),
        (maximum(x0, x1), -INF, 3.5),
    ], objective=nlexpr.pow(x0, 1.5) + nlexpr.pow(x1, 1.5) + cosh(x0 - x1), n=2)
    return fm


def test_known_answer_model_through_the_cpu_oracle():
    from tests.test_nlexpr_cpu import _oracle
    pr = ops_function_model().to_problem("ops")
    assert set(pr.function_model.nlp.tape.op.tolist()) >= set(range(nlexpr.ABS, nlexpr.OP_COUNT))
    for alg in ("Line Search", "Trust Region"):
        mo = _oracle(pr, alg)
        assert mo.status == 0 and np.allclose(mo.x, [1.0, 1.0], rtol=1e-4), (alg, mo.status, mo.x)
        assert abs(pr.eval_f(mo.x) - 3.0) < 1e-4
