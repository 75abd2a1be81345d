"""Second derivatives of the Ohm's-law block and of the dense quadratic block on the host (acopf.function_model(..., hessian=True),
problems.synthetic_dense_function_model(..., hessian=True)): the closed-form twin of k_nlp_ohm_hess / k_nlp_dense_hess against the
expression twin of the same rows (nlp="expr"), against finite differences of its own Jacobian, and under SLP-EQP."""
import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import acopf, problems, sensitivity
from activesetmethods_amd.moi_evaluator import NLP_KINDS, hessian_matrix, hessian_product
from tests.test_nlhess_cpu import PARITY
from tests.test_slp_eqp_cpu import run as eqp_run

GRIDS = {"grid3": (3, 2, 3, 1, 0.5), "grid14": (14, 5, 20, 1, 0.5)}
BRANCH_KEYS = ("f_bus", "t_bus", "g", "b", "b_fr", "b_to", "g_fr", "g_to", "tr", "ti", "tm", "rate_a", "angmin", "angmax")


def grid(name):
    return acopf.synthetic_case(name, 1, 0.5) if name.startswith("case") else acopf.synthetic_grid(*GRIDS[name])


def with_branches(case, idx, reverse=()):
    """`case` with the branch rows `idx` (repeats allowed); the rows at the positions in `reverse` run the other way."""
    c = dict(case)
    for k in BRANCH_KEYS:
        c[k] = np.asarray(case[k])[list(idx)].copy()
    for p in reverse:
        c["f_bus"][p], c["t_bus"][p] = c["t_bus"][p], c["f_bus"][p]
    return c


def twins(case):
    return acopf.function_model(case, hessian=True), acopf.function_model(case, nlp="expr")


def values(fm, x, sigma, lam):
    return fm.eval_hessian_lagrangian(np.asarray(x, float), sigma, np.asarray(lam, float), np.zeros(len(fm.hessian_lagrangian_structure())))


def dense(fm, x, sigma, lam):
    h = fm.hessian_lagrangian_structure()
    return hessian_matrix([r for r, _ in h], [c for _, c in h], values(fm, x, sigma, lam), fm.n)


def assert_matrices_agree(fk, fe, tag, seed=5):
    """Start point and two seeded perturbed points, random multipliers, obj_factor 1 and 0."""
    rng = np.random.default_rng(seed)
    x0 = fk.start_point()
    for rep in range(3):
        x = x0 if rep == 0 else x0 + 0.05 * rng.standard_normal(fk.n)
        lam = rng.standard_normal(fk.m)
        for sigma in (1.0, 0.0):
            Hk, He = dense(fk, x, sigma, lam), dense(fe, x, sigma, lam)
            bar = PARITY * max(1.0, float(np.abs(He).max()))
            print("%s point %d sigma %g: max |H_ohm - H_expr| = %.3e, bar %.3e" % (tag, rep, sigma, float(np.abs(Hk - He).max()), bar))
            assert np.all(np.abs(Hk - He) <= bar), (tag, rep, sigma)


def test_the_kinds_are_announced():
    assert NLP_KINDS["acopf_ohm_hess"] == 4 and NLP_KINDS["dense_quadratic_hess"] == 5
    case = grid("grid3")
    plain, hess = acopf.function_model(case), acopf.function_model(case, hessian=True)
    assert plain.nlp.device[0] == "acopf_ohm" and plain.nlp.eval_hess is None            # the default builds today's object
    assert hess.nlp.device[0] == "acopf_ohm_hess"
    assert np.array_equal(plain.nlp.device[1], hess.nlp.device[1]) and np.array_equal(plain.nlp.device[2], hess.nlp.device[2])
    with pytest.raises(ValueError):
        plain.hessian_lagrangian_structure()
    with pytest.raises(ValueError):
        acopf.function_model(case, nlp="expr", hessian=True)
    dp, dh = problems.synthetic_dense_function_model(12, 5), problems.synthetic_dense_function_model(12, 5, hessian=True)
    assert dp.nlp.device[0] == "dense_quadratic" and dp.nlp.eval_hess is None and dh.nlp.device[0] == "dense_quadratic_hess"
    assert np.array_equal(dp.nlp.device[2], dh.nlp.device[2])


@pytest.mark.parametrize("name,block,store", [("grid3", 21, 14), ("grid14", 122, 85)])
def test_pattern_is_the_expression_twins(name, block, store):
    fk, fe = twins(grid(name))
    sk, se = fk.hessian_lagrangian_structure(), fe.hessian_lagrangian_structure()
    assert sk == se
    assert len(fk.nlp.hess_rows) == block and len(sk) == store + block
    assert fk.nlp_constraint_offset == fe.nlp_constraint_offset
    pairs = list(zip(fk.nlp.hess_rows.tolist(), fk.nlp.hess_cols.tolist()))
    assert pairs == sorted(set(pairs)) and all(r >= c for r, c in pairs)                  # distinct, lower triangle, sorted by (row, column)


@pytest.mark.parametrize("name", ["grid3", "grid14", "case300"])
def test_values_agree_with_the_expression_twin(name):
    fk, fe = twins(grid(name))
    assert fk.hessian_lagrangian_structure() == fe.hessian_lagrangian_structure()
    assert_matrices_agree(fk, fe, name)


def test_parallel_and_reversed_branches_add():
    """Branch 0 twice (a parallel pair) and branch 1 once in each direction (a reversed pair): the occurrences of a pair of buses add into one
    entry.  A branch from a bus to itself is refused."""
    base = grid("grid3")
    case = with_branches(base, [0, 1, 2, 0, 1], reverse=[4])
    assert case["f_bus"][3] == case["f_bus"][0] and case["t_bus"][3] == case["t_bus"][0]
    assert case["f_bus"][4] == case["t_bus"][1] and case["t_bus"][4] == case["f_bus"][1]
    fk, fe = twins(case)
    assert fk.hessian_lagrangian_structure() == fe.hessian_lagrangian_structure()
    assert len(fk.nlp.hess_rows) == len(acopf.function_model(base, hessian=True).nlp.hess_rows)       # no new pair of variables
    assert_matrices_agree(fk, fe, "grid3 + parallel + reversed")
    loop = with_branches(base, [0, 1, 2])
    loop["t_bus"][1] = loop["f_bus"][1]
    with pytest.raises(ValueError, match="itself"):
        acopf.function_model(loop, hessian=True)
    assert acopf.function_model(loop).nlp.eval_hess is None                                            # without second derivatives it still builds


def _fd_error(fm, x, lam, v, h):
    """Relative distance between the central difference of J' lam along v and H v (obj_factor 0: the constraints' part alone)."""
    jtl = lambda z: sensitivity.dense_jacobian(fm, z).T @ lam
    fd = (jtl(x + h * v) - jtl(x - h * v)) / (2.0 * h)
    hv = fm.hessian_lagrangian_product(x, 0.0, lam, v)
    return float(np.abs(fd - hv).max() / max(1.0, np.abs(hv).max()))


def test_finite_differences_of_the_jacobian():
    """The bar is twice the error of the same check on the expression twin at the same point, step and direction.  h = 1e-4 puts the
    truncation error of the central difference (h^2 f''' / 6 ~ 1e-8 of the entries, the same for both models: they are one function) three
    orders above its rounding noise (u |J' lam| / h ~ 1e-12), so the two errors differ by noise only and a wrong entry shows at O(1)."""
    fk, fe = twins(grid("grid14"))
    rng = np.random.default_rng(9)
    x = fk.start_point() + 0.05 * rng.standard_normal(fk.n)
    lam, v = rng.standard_normal(fk.m), rng.standard_normal(fk.n)
    v /= np.abs(v).max()
    ek, ee = _fd_error(fk, x, lam, v, 1e-4), _fd_error(fe, x, lam, v, 1e-4)
    print("central difference of J' lam against H v: Ohm's-law twin %.3e, expression twin %.3e, bar %.3e" % (ek, ee, 2.0 * ee))
    assert ee < 1e-5                # the reference check itself works
    assert ek <= 2.0 * ee


def test_dense_block_values_and_products():
    n, m = 23, 7
    fm = problems.synthetic_dense_function_model(n, m, hessian=True)
    Q = np.asarray(fm.nlp.device[2], float)[m * n:].reshape(m, n)
    off = fm.nlp_constraint_offset
    struct = fm.hessian_lagrangian_structure()
    assert struct[-n:] == [(j, j) for j in range(1, n + 1)] and len(struct) == n + n       # objective diagonal, then the block's
    rng = np.random.default_rng(2)
    x, lam, v = rng.standard_normal(n), rng.standard_normal(fm.m), rng.standard_normal(n)
    for sigma in (1.0, 0.0):
        vals = values(fm, x, sigma, lam)
        want = []
        for j in range(n):
            g = 0.0
            for i in range(m):
                g = g + float(lam[off + i]) * float(Q[i, j])
            want.append(g)
        assert np.array_equal(vals[-n:], np.array(want)), sigma
        rows, cols = [r for r, _ in struct], [c for _, c in struct]
        hv = fm.hessian_lagrangian_product(x, sigma, lam, v)
        assert np.array_equal(hv, hessian_product(rows, cols, vals, v))
        ref = hessian_matrix(rows, cols, vals, n) @ v
        assert np.all(np.abs(hv - ref) <= 1e-13 * max(1.0, np.abs(ref).max()))


def test_slp_eqp_on_the_host_converges_with_the_exact_hessian():
    """The 14-bus grid with the Ohm's-law block: status 0 within max_iter = 60 (the limited-memory run of tests/test_lmhess_cpu.py stops at
    the limit there); the iteration count beside the expression model's is printed, not asserted equal."""
    fk, fe = twins(grid("grid14"))
    mk, sk = eqp_run(fk, "SLP-EQP", "grid14 ohm hess", max_iter=60)
    me, se = eqp_run(fe, "SLP-EQP", "grid14 expr", max_iter=60)
    print("grid14 SLP-EQP: Ohm's-law block status %d iter %d lp %d %r | expression block status %d iter %d lp %d" %
          (mk.status, sk.iter, sk.lp_solves, sk.eqp_counts, me.status, se.iter, se.lp_solves))
    assert mk.status == 0 and sk.iter < 60
    assert sk.eqp_counts["accepted"] >= 1
