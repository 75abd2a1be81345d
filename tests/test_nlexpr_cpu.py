"""Expression NLP blocks (activesetmethods_amd/nlexpr.py, nlp_kind 3 of include/asm_hip.h) on the host: the tape, its pattern and
the host twin of the device kernels against closed forms, finite differences, the hand-written ACOPF evaluator and the CPU
oracle.  No GPU."""
import numpy as np
import pytest

from activesetmethods_amd import acopf, nlexpr, problems
from activesetmethods_amd.nlexpr import ExprBlock, variables, sin, cos, exp, log, sqrt

# the CPU oracle's run of HS071 (oracle/slp.py, Trust Region, default parameters): the pin of tests/test_nlexpr_gpu.py
HS071_ORACLE_STATUS = 0
HS071_ORACLE_X = [1.0, 4.742998387062792, 3.8211516176177085, 1.3794080671070619]


def _oracle(pr, alg):
    from oracle import slp as O
    mo = O.Model(pr.n, pr.m, pr.x_L, pr.x_U, pr.g_L, pr.g_U, pr.j_str, pr.eval_f, pr.eval_g, pr.eval_grad_f, pr.eval_jac_g,
                 O.Parameters(algorithm=alg))
    mo.x[:] = pr.x0
    O.optimize(mo)
    return mo


def random_expr_block(seed, n=6, rows=5, smooth=True, objective=True):
    """Seeded random rows over n variables; smooth=False keeps to + - * / unary - and integer powers (bit-exact on the device)."""
    rng = np.random.default_rng(seed)
    x = variables(n)

    def leaf():
        return x[int(rng.integers(n))] if rng.random() < 0.75 else nlexpr.const(float(rng.uniform(-2, 2)))

    def build(depth):
        if depth == 0:
            return leaf()
        k = int(rng.integers(10 if smooth else 6))
        u, v = build(depth - 1), build(depth - 1)
        if k == 0:
            return u + v
        if k == 1:
            return u - v
        if k == 2:
            return u * v
        if k == 3:
            return u / (1.5 + v * v)
        if k == 4:
            return -u + v ** 3
        if k == 5:
            return u ** -2 if rng.random() < 0.2 else u ** 2 * v
        if k == 6:
            return log(1 + u ** 2) * v
        if k == 7:
            return sqrt(1 + u ** 2) - v
        if k == 8:
            return sin(u) * exp(0.3 * v)
        return cos(u) + exp(-(v ** 2))
    cons = []
    for r in range(rows):
        e = build(3)
        shared = x[r % n] * x[(r + 1) % n]
        cons.append((e + shared * shared - shared, -1.0, 1.0) if r % 2 else (e, 0.5, 0.5))
    obj = None
    if objective:
        obj = build(2) * build(1) + x[0] ** 2 + build(2) + x[n - 1]
    return ExprBlock(cons, obj, n=n), n


def _model(block, n, sense="MIN_SENSE"):
    from activesetmethods_amd.moi_evaluator import FunctionModel, ScalarFunction
    fm = FunctionModel(n, -2 * np.ones(n), 2 * np.ones(n))
    fm.add_constraint(ScalarFunction(0.5, [(1.0, 1), (-2.0, n)]), "le", 1.0)
    fm.objective = ScalarFunction(3.0, [(1.0, 1)])          # overridden by the block's objective when it has one
    fm.sense = sense
    fm.nlp = block
    return fm


def test_toy_as_expressions_equals_the_toy_callbacks_bit_for_bit():
    t, e = problems.toy_problem(), problems.toy_expr_problem()
    assert e.j_str == t.j_str and np.array_equal(e.g_L, t.g_L) and np.array_equal(e.g_U, t.g_U)
    rng = np.random.default_rng(3)
    for x in [np.zeros(2), np.array([-1.0, -1.0])] + [rng.standard_normal(2) * 3 for _ in range(20)]:
        assert e.eval_f(x) == t.eval_f(x)
        assert np.array_equal(e.eval_grad_f(x, np.zeros(2)), t.eval_grad_f(x, np.zeros(2)))
        assert np.array_equal(e.eval_g(x, np.zeros(4)), t.eval_g(x, np.zeros(4)))
        assert np.array_equal(e.eval_jac_g(x, np.zeros(6)), t.eval_jac_g(x, np.zeros(6)))


def test_hs071_equals_closed_forms():
    pr = problems.hs071_problem()
    assert pr.n == 4 and pr.m == 2 and np.array_equal(pr.x0, [1, 5, 5, 1])
    assert np.array_equal(pr.x_L, np.ones(4)) and np.array_equal(pr.x_U, np.full(4, 5.0))
    assert np.array_equal(pr.g_L, [25.0, 40.0]) and np.array_equal(pr.g_U, [np.inf, 40.0])
    assert pr.j_str == [(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (2, 3), (2, 4)]
    rng = np.random.default_rng(5)
    for x in [pr.x0] + [rng.uniform(1, 5, 4) for _ in range(10)]:
        x1, x2, x3, x4 = x
        assert np.isclose(pr.eval_f(x), x1 * x4 * (x1 + x2 + x3) + x3, rtol=1e-15)
        want = [x4 * (x1 + x2 + x3) + x1 * x4, x1 * x4, x1 * x4 + 1.0, x1 * (x1 + x2 + x3)]
        assert np.allclose(pr.eval_grad_f(x, np.zeros(4)), want, rtol=1e-15)
        assert np.allclose(pr.eval_g(x, np.zeros(2)), [x1 * x2 * x3 * x4, x @ x], rtol=1e-15)
        assert np.allclose(pr.eval_jac_g(x, np.zeros(8)), [x2 * x3 * x4, x1 * x3 * x4, x1 * x2 * x4, x1 * x2 * x3, *(2 * x)], rtol=1e-15)


@pytest.mark.parametrize("seed", range(6))
def test_gradients_match_central_differences(seed):
    block, n = random_expr_block(seed)
    fm = _model(block, n)
    pr = fm.to_problem()
    rng = np.random.default_rng(seed + 100)
    x = rng.uniform(-1, 1, n)
    J = pr.eval_jac_g(x, np.zeros(pr.nnz))
    g = pr.eval_grad_f(x, np.zeros(n))
    Jd = np.zeros((pr.m, n))
    np.add.at(Jd, (pr.j_row - 1, pr.j_col - 1), J)
    for j in range(n):
        h = 1e-6 * max(1.0, abs(x[j]))
        xp, xm = x.copy(), x.copy()
        xp[j] += h
        xm[j] -= h
        fd_g = (pr.eval_g(xp, np.zeros(pr.m)) - pr.eval_g(xm, np.zeros(pr.m))) / (2 * h)
        fd_f = (pr.eval_f(xp) - pr.eval_f(xm)) / (2 * h)
        assert np.allclose(Jd[:, j], fd_g, rtol=1e-6, atol=1e-6 * max(1.0, np.abs(fd_g).max())), (j, Jd[:, j], fd_g)
        assert abs(g[j] - fd_f) <= 1e-6 * max(1.0, abs(fd_f)), (j, g[j], fd_f)


def test_expression_objective_overrides_and_is_scaled():
    block, n = random_expr_block(7)
    x = np.linspace(-0.5, 0.7, n)
    base = block.eval_f(x)
    gb = block.eval_grad_f(x, np.zeros(n))
    for sense, s in (("MIN_SENSE", 1.0), ("MAX_SENSE", -1.0), ("FEASIBILITY_SENSE", 0.0)):
        fm = _model(block, n, sense)
        assert fm.eval_f(x) == s * base
        assert np.array_equal(fm.eval_grad_f(x, np.zeros(n)), gb * s)


def test_pattern_is_ascending_and_distinct_per_row():
    for seed in range(8):
        block, n = random_expr_block(seed)
        for r in np.unique(block.rows):
            cols = block.cols[block.rows == r]
            assert np.all(np.diff(cols) > 0)
        R, T, L, ptr, op, a, b = nlexpr.parse_ipar(block.device[1])
        assert R == block.m and L == len(op) and ptr[-1] == L
        for r in range(R):
            k = np.arange(ptr[r], ptr[r + 1])
            assert np.array_equal(np.unique(a[k[op[k] == nlexpr.VAR]]) + 1, block.cols[block.rows == r + 1])
            nodes = k[(op[k] != nlexpr.CONST) & (op[k] != nlexpr.VAR)]
            assert np.all(a[nodes] < nodes - ptr[r])         # references go to earlier nodes of the same row


def test_malformed_expressions_are_rejected():
    x = variables(3)
    with pytest.raises(TypeError):
        x[0] ** 1.5
    with pytest.raises(TypeError):
        x[0] + "1"
    with pytest.raises(ValueError):
        x[0] ** 65
    with pytest.raises(ValueError):
        ExprBlock([(x[0] * x[2], 0.0, 1.0)], n=2)             # variable out of range
    from activesetmethods_amd.moi_evaluator import NlpBlock, nlp_kind
    with pytest.raises(ValueError):
        NlpBlock([0.0], [0.0], [1], [1], None, None, has_objective=True)
    with pytest.raises(ValueError):
        nlp_kind(("no_such_kernel", None, None))
    assert nlp_kind(("acopf_ohm",)) == 1 and nlp_kind(("dense_quadratic",)) == 2 and nlp_kind(("expr",)) == 3


def test_acopf_expression_rows_match_the_hand_written_evaluator():
    case = acopf.synthetic_case("case118", 1)
    pe = acopf.function_model(case, nlp="expr").to_problem()
    po = acopf.function_model(case).to_problem()
    assert pe.m == po.m and pe.nnz == po.nnz and np.array_equal(pe.g_L, po.g_L) and np.array_equal(pe.g_U, po.g_U)
    rng = np.random.default_rng(2)
    for x in (pe.x0, pe.x0 + 0.02 * rng.standard_normal(pe.n)):
        ge, go = pe.eval_g(x, np.zeros(pe.m)), po.eval_g(x, np.zeros(po.m))
        assert np.all(np.abs(ge - go) <= 1e-13 * np.maximum(1.0, np.abs(go)))
        assert pe.eval_f(x) == po.eval_f(x) and np.array_equal(pe.eval_grad_f(x, np.zeros(pe.n)), po.eval_grad_f(x, np.zeros(po.n)))
        Je, Jo = pe.eval_jac_g(x, np.zeros(pe.nnz)), po.eval_jac_g(x, np.zeros(po.nnz))
        de = dict(zip(zip(pe.j_row.tolist(), pe.j_col.tolist()), Je))
        do = dict(zip(zip(po.j_row.tolist(), po.j_col.tolist()), Jo))
        assert len(de) == pe.nnz and de.keys() == do.keys()
        assert all(abs(de[k] - do[k]) <= 1e-13 * max(1.0, abs(do[k])) for k in do)
    with pytest.raises(ValueError):
        acopf.function_model(case, nlp="quadratic")


def test_cpu_oracle_solves_the_expression_models():
    mo = _oracle(problems.toy_expr_problem(), "Line Search")
    assert mo.status == 0 and np.allclose(mo.x, [-1.0, -1.0], atol=1e-8)
    mo = _oracle(problems.hs071_problem(), "Trust Region")
    assert mo.status == HS071_ORACLE_STATUS
    assert np.allclose(mo.x, HS071_ORACLE_X, rtol=0, atol=1e-12)
    assert abs(problems.hs071_problem().eval_f(mo.x) - 17.0140173) < 1e-6      # the problem's known optimum
