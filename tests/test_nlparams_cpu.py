"""Parameters of expression NLP blocks on the host (activesetmethods_amd/nlexpr.py: parameters, ExprBlock(..., parameters=...),
set_parameter_values, data_gradient): their dpar layout, the unchanged encoding of tapes without them, the host twin of the data
gradient against central differences, and the envelope theorem at an oracle SLP solution."""
import os

import numpy as np
import pytest

from activesetmethods_amd import acopf, nlexpr, problems
from activesetmethods_amd.nlexpr import ExprBlock, parameters, variables
from oracle import slp as O
from tests.test_nlexpr_cpu import _model
from tests.test_nlexpr_ops_cpu import ops_function_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = dict(tol_direction=1e-12, tol_residual=1e-10, tol_infeas=1e-12)


def test_parameters_occupy_the_first_dpar_slots_and_are_never_merged():
    x = variables(2)
    p = parameters([2.0, 2.0, 0.5])
    blk = ExprBlock([(p[0] * x[0] + 2.0 * x[1] + p[1], 0.0, 0.0), (p[2] * x[0] - 0.5 + p[0], -1.0, 1.0)],
                    objective=p[1] * x[1] ** 2 + 2.0, n=2, parameters=p)
    assert blk.n_params == 3
    dpar = blk.device[2]
    assert dpar.tolist() == [2.0, 2.0, 0.5, 2.0, 0.5]         # the parameters in declaration order, then the distinct constants
    R, T, L, ptr, op, a, b = nlexpr.parse_ipar(blk.device[1])
    used = a[op == nlexpr.CONST].tolist()
    assert set(used) == {0, 1, 2, 3, 4}                      # equal values: five separate slots
    # a parameter used twice in a row is one node; declared, unused parameters keep their slot
    q = parameters([1.0, 3.0])
    blk2 = ExprBlock([(q[0] * x[0] + q[0] * x[1], 0.0, 0.0)], n=2, parameters=q)
    _, _, _, _, op2, a2, _ = nlexpr.parse_ipar(blk2.device[1])
    assert (op2 == nlexpr.CONST).sum() == 1 and blk2.device[2].tolist() == [1.0, 3.0]
    with pytest.raises(ValueError):
        ExprBlock([(q[1] * x[0], 0.0, 0.0)], n=2, parameters=q[:1])            # undeclared parameter
    with pytest.raises(TypeError):
        ExprBlock([(x[0], 0.0, 0.0)], n=2, parameters=[nlexpr.const(1.0)])
    with pytest.raises(ValueError):
        blk2.set_parameter_values([1.0])


def test_tapes_without_parameters_keep_their_encoding():
    """hs071 and the ops model encode byte for byte as before parameters existed (tests/golden/nlexpr_encoding.npz)."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "nlexpr_encoding.npz"))
    for name, fm in (("hs071", problems.hs071_function_model()), ("ops", ops_function_model())):
        _, ipar, dpar = fm.nlp.device
        assert fm.nlp.n_params == 0
        assert np.asarray(ipar, np.int64).tobytes() == gold[name + "_ipar"].tobytes(), name
        assert np.asarray(dpar, np.float64).tobytes() == gold[name + "_dpar"].tobytes(), name


def random_param_block(seed, values, n=4, rows=5, exact=False):
    """Seeded random rows and objective whose leaves are variables, parameters (each used in several rows and terms) and constants;
    exact=True keeps to + - * / and abs, min, max.  `values`: the parameter values, so that the same seed gives the same tape."""
    rng = np.random.default_rng(seed)
    x = variables(n)
    p = parameters(values)

    def leaf():
        u = rng.random()
        if u < 0.5:
            return x[int(rng.integers(n))]
        if u < 0.85:
            return p[int(rng.integers(len(p)))]
        return nlexpr.const(float(rng.uniform(-2, 2)))

    def build(depth):
        if depth == 0:
            return leaf()
        k = int(rng.choice([0, 1, 2, 5, 9, 10])) if exact else int(rng.integers(11))
        u, v = build(depth - 1), build(depth - 1)
        return [lambda: u + v, lambda: u * v - u, lambda: u / (1.5 + v * v), lambda: nlexpr.sin(u) * nlexpr.exp(0.3 * nlexpr.tanh(v)),
                lambda: nlexpr.sqrt(1 + u ** 2) - nlexpr.log(2 + nlexpr.cos(v)), lambda: abs(u) - v,
                lambda: nlexpr.pow(1 + u * u, nlexpr.tanh(v)), lambda: nlexpr.atan(u, 2 + nlexpr.cos(v)),
                lambda: nlexpr.cbrt(1.5 + nlexpr.cos(u)) + v, lambda: nlexpr.minimum(u, v), lambda: nlexpr.maximum(u, v, 0.5 * u)][k]()
    cons = [(build(3), 0.5, 0.5) if r % 2 == 0 else (build(3), -1.0, 1.0) for r in range(rows)]
    obj = build(2) * build(1) + build(2) + p[0] * x[n - 1]
    return ExprBlock(cons, obj, n=n, parameters=p), n


@pytest.mark.parametrize("seed", range(4))
def test_set_parameter_values_equals_a_rebuilt_block(seed):
    v0 = np.random.default_rng(seed).uniform(-1.5, 1.5, 3)
    v1 = v0 + np.random.default_rng(seed + 9).uniform(-0.5, 0.5, 3)
    blk, n = random_param_block(seed, v0)
    ipar0 = blk.device[1].copy()
    dpar0 = blk.device[2].copy()
    blk.set_parameter_values(v1)
    ref, _ = random_param_block(seed, v1)
    assert np.array_equal(blk.device[1], ipar0) and np.array_equal(blk.device[1], ref.device[1])
    assert np.array_equal(blk.device[2], ref.device[2]) and np.array_equal(blk.device[2][3:], dpar0[3:])
    pa, pb = _model(blk, n).to_problem(), _model(ref, n).to_problem()
    rng = np.random.default_rng(seed + 70)
    for _ in range(3):
        x = rng.uniform(-1, 1, n)
        assert pa.eval_f(x) == pb.eval_f(x)
        assert np.array_equal(pa.eval_grad_f(x, np.zeros(n)), pb.eval_grad_f(x, np.zeros(n)))
        assert np.array_equal(pa.eval_g(x, np.zeros(pa.m)), pb.eval_g(x, np.zeros(pb.m)))
        assert np.array_equal(pa.eval_jac_g(x, np.zeros(pa.nnz)), pb.eval_jac_g(x, np.zeros(pb.nnz)))
        lam = rng.standard_normal(blk.m)
        assert np.array_equal(blk.data_gradient(x, lam), ref.data_gradient(x, lam))


def _lagrangian(blk, x, lam, scale):
    g = blk.eval_g(x, np.zeros(blk.m))
    return scale * blk.eval_f(x) - float(np.dot(lam, g))


@pytest.mark.parametrize("seed", range(6))
def test_data_gradient_matches_central_differences(seed):
    """d(scale f - lam' g) / d parameter against central differences of the host evaluations (parameters shared by rows and terms)."""
    v = np.random.default_rng(seed + 3).uniform(-1.5, 1.5, 3)
    blk, n = random_param_block(seed, v, exact=seed % 2 == 1)
    rng = np.random.default_rng(seed + 300)
    for scale in (1.0, -1.0):
        x = rng.uniform(-1, 1, n)
        lam = rng.standard_normal(blk.m)
        dg = blk.data_gradient(x, lam, scale)
        assert dg.shape == (len(blk.device[2]),)
        for k in range(3):
            h = 1e-6
            vals = []
            for sg in (1, -1):
                w = v.copy()
                w[k] += sg * h
                blk.set_parameter_values(w)
                vals.append(_lagrangian(blk, x, lam, scale))
            blk.set_parameter_values(v)
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(dg[k] - fd) <= 1e-6 * max(1.0, abs(fd)), (seed, scale, k, dg[k], fd)


def test_data_gradient_of_constants_and_the_summation_order():
    """The constants get their derivative too; a parameter's occurrences are summed in (row, then term; node) order from 0.0."""
    x = variables(2)
    p = parameters([3.0])
    blk = ExprBlock([(p[0] * x[0], 0.0, 0.0), (x[1] - p[0] * 2.0, 0.0, 0.0)], objective=p[0] * x[0] * x[1] + 1.5 * x[1], n=2, parameters=p)
    xv, lam = np.array([0.3, -0.7]), np.array([0.25, -2.0])
    dg = blk.data_gradient(xv, lam, -1.0)
    want = 0.0 + (-lam[0]) * xv[0]
    want = want + (-lam[1]) * -2.0
    want = want + -1.0 * (xv[0] * xv[1])
    assert dg[0] == want
    assert blk.device[2].tolist() == [3.0, 2.0, 1.5]
    assert dg[1] == (-lam[1]) * -3.0 and dg[2] == -1.0 * xv[1]


def _oracle(pr, alg):
    mo = O.Model(pr.n, pr.m, pr.x_L, pr.x_U, pr.g_L, pr.g_U, pr.j_str, pr.eval_f, pr.eval_g, pr.eval_grad_f, pr.eval_jac_g,
                 O.Parameters(algorithm=alg, **TIGHT))
    mo.x[:] = pr.x0
    O.optimize(mo)
    return mo


@pytest.mark.parametrize("alg", ["Line Search", "Trust Region"])
def test_envelope_theorem_at_the_oracle_solution(alg):
    """dV/d(a, p) of problems.parametric_function_model: the data gradient at the oracle's SLP solution equals the closed form and the
    central difference of the oracle's optimal values V(p +- h)."""
    a, p = 0.5, 4.0
    fm = problems.parametric_function_model(a, p)
    pr = fm.to_problem("parametric")
    mo = _oracle(pr, alg)
    xs, V, dV = problems.parametric_solution(a, p)
    assert mo.status == 0 and np.allclose(mo.x, xs, rtol=1e-9, atol=0.0), mo.x
    assert abs(pr.eval_f(mo.x) - V) <= 1e-9 * V
    dg = fm.nlp.data_gradient(mo.x, mo.mult_g, fm.objective_scale)
    assert dg.shape == (2,) and np.allclose(dg, dV, rtol=1e-8)
    h = 1e-3
    for k in range(2):
        vals = []
        for sg in (1, -1):
            v = np.array([a, p])
            v[k] += sg * h
            f2 = problems.parametric_function_model(*v).to_problem()
            m2 = _oracle(f2, alg)
            assert m2.status == 0
            vals.append(f2.eval_f(m2.x))
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - dg[k]) <= 1e-4 * abs(dg[k]), (k, fd, dg[k])


def test_line_scenarios_share_one_parameterised_tape():
    """line_scenario_case scales each branch admittance by 1 / U(0.95, 1.05); with branch_params the Ohm's-law coefficients are the
    parameters, in the kernel's dpar layout, and every scenario has the tape of the base case; host evaluations equal the block without
    parameters bit for bit."""
    base = acopf.synthetic_case("case118", 1, 0.5)
    c1, c1b = acopf.line_scenario_case(base, 1), acopf.line_scenario_case(base, 1)
    k = base["g"] / c1["g"]
    assert np.all((k >= 0.95) & (k <= 1.05)) and np.array_equal(c1["g"], c1b["g"]) and np.array_equal(c1["pd"], base["pd"])
    assert np.allclose(base["b"] / c1["b"], k, rtol=1e-12)
    f0 = acopf.function_model(base, nlp="expr", branch_params=True)
    f1 = acopf.function_model(c1, nlp="expr", branch_params=True)
    k1 = acopf.function_model(c1)
    nl = len(base["f_bus"])
    assert f1.nlp.n_params == 8 * nl
    assert np.array_equal(f0.nlp.device[1], f1.nlp.device[1])
    assert np.array_equal(f1.nlp.device[2][:8 * nl], k1.nlp.device[2])
    plain = acopf.function_model(c1, nlp="expr")
    pa, pb = f1.to_problem(), plain.to_problem()
    assert pa.j_str == pb.j_str
    x = pa.x0 + 0.01 * np.random.default_rng(5).standard_normal(pa.n)
    assert np.array_equal(pa.eval_g(x, np.zeros(pa.m)), pb.eval_g(x, np.zeros(pb.m)))
    assert np.array_equal(pa.eval_jac_g(x, np.zeros(pa.nnz)), pb.eval_jac_g(x, np.zeros(pb.nnz)))
    with pytest.raises(ValueError):
        acopf.function_model(base, branch_params=True)
