"""Sensitivities to variable bounds and to the bound multipliers z on the host (include/asm_hip.h, "Variable-bound sensitivities" under
"Many right-hand sides on one factor" and asm_solution_adjoint_z under "Adjoint solution sensitivities"): the recipe ru = H delta,
rw = J delta, dx += delta against the dense system with dx_B = delta imposed directly; both against the exact change of a QP's solution
when a fixed variable moves; the adjoint reference with weights on z against forward columns; the declared symbols.  No GPU."""
import os

import numpy as np
import pytest

from activesetmethods_amd import sensitivity
from tests.test_adjoint_cpu import hs071_point
from tests.test_block_data_cpu import block_cross
from tests.test_sensitivity_cpu import KKT_BAR, kkt_instance, rel_err

NEW_SYMBOLS = ("asm_var_bound_sensitivity_multi", "asm_batch_var_bound_sensitivity", "asm_solution_adjoint_z", "asm_solution_adjoint_z_multi",
               "asm_batch_solution_adjoint_z")


def _matrices(fm, x, lam):
    return sensitivity.lagrangian_hessian(fm, x, lam), sensitivity.dense_jacobian(fm, x)


# ------------------------------------------------------------------------------------------------ 1. recipe and reference
@pytest.mark.parametrize("shape", ((8, 3, 5), (33, 1, 1), (96, 10, 65)), ids=lambda s: "n%d_B%d_W%d" % s)
def test_the_recipe_equals_the_direct_solve(shape):
    """var_bound_reference (dx_B = delta imposed on the dense system) against kkt_reference_multi on var_bound_rhs plus delta: every
    variable of B, one free variable (the zero column) and a repeated variable, with moves of both signs."""
    fm, x, lam, rs, bs = kkt_instance(*shape)[:5]
    B, free = np.nonzero(bs != 0)[0], int(np.nonzero(bs == 0)[0][0])
    vars = list(map(int, B)) + [free, int(B[0])]
    delta = 0.25 + np.random.default_rng(sum(shape)).uniform(-2.0, 2.0, len(vars))
    H, J = _matrices(fm, x, lam)
    for d in (delta, None):
        RU, RW, D = sensitivity.var_bound_rhs(H, J, fm.n, fm.m, bs, vars, d)
        assert RU.shape == (len(vars), fm.n) and RW.shape == (len(vars), fm.m) and D.shape == (len(vars), fm.n)
        DX, DLAM, DZ = sensitivity.kkt_reference_multi(fm, x, lam, rs, bs, RU, RW)
        DX = DX + D
        RX, RL, RZ = sensitivity.var_bound_reference(fm, x, lam, rs, bs, vars, d)
        errs = [rel_err(g, w) for g, w in zip((DX, DLAM, DZ), (RX, RL, RZ))]
        print("shape %r, delta %s: rel err of dx, dlam, dz %r (bar %.3e)" % (shape, "given" if d is not None else "None", errs, KKT_BAR))
        assert max(errs) <= KKT_BAR, (shape, errs)
        k = len(B)
        assert not RX[k].any() and not RL[k].any() and not RZ[k].any() and not RU[k].any() and not RW[k].any() and not D[k].any()
        for c, j in enumerate(vars):
            if c != k:
                assert RX[c, j] == (1.0 if d is None else d[c]) and np.any(RZ[c] != 0.0) and not RZ[c, bs == 0].any()
        if d is None:
            assert np.array_equal(RX[k + 1], RX[0]) and np.array_equal(RZ[k + 1], RZ[0])


def test_no_bound_variable_gives_zero_columns():
    fm, x, lam, rs, bs = kkt_instance(8, 0, 0)[:5]
    H, J = _matrices(fm, x, lam)
    vars = [0, 3, 7]
    RU, RW, D = sensitivity.var_bound_rhs(H, J, fm.n, fm.m, bs, vars)
    got = sensitivity.var_bound_reference(fm, x, lam, rs, bs, vars, [1.0, -2.0, 0.5])
    assert not RU.any() and not RW.any() and not D.any() and not any(a.any() for a in got)
    with pytest.raises(ValueError):
        sensitivity.var_bound_rhs(H, J, fm.n, fm.m, bs, [8])
    with pytest.raises(ValueError):
        sensitivity.var_bound_reference(fm, x, lam, rs, bs, [-1])


# ------------------------------------------------------------------------------------------------ 2. exactness on a QP
def _qp_solution(fm, H, J, c, rs, bs, xB, b):
    """(x, lam, z) of min 1/2 x'Hx + c'x over J[W] x = b, x_B = xB (z = (H x + c - J_W' lam) on B): one dense solve."""
    F, B, W = np.nonzero(bs == 0)[0], np.nonzero(bs != 0)[0], np.nonzero(rs == 1)[0]
    nF, nW = len(F), len(W)
    A = J[np.ix_(W, F)]
    K = np.zeros((nF + nW, nF + nW))
    K[:nF, :nF], K[:nF, nF:], K[nF:, :nF] = H[np.ix_(F, F)], -A.T, A
    sol = np.linalg.solve(K, np.concatenate([-c[F] - H[np.ix_(F, B)] @ xB, b - J[np.ix_(W, B)] @ xB]))
    x, lam, z = np.zeros(fm.n), np.zeros(fm.m), np.zeros(fm.n)
    x[F], x[B], lam[W] = sol[:nF], xB, sol[nF:]
    z[B] = (H @ x + c - J[W].T @ lam[W])[B]
    return x, lam, z


@pytest.mark.parametrize("shape", ((8, 3, 5), (96, 10, 65)), ids=lambda s: "n%d_B%d_W%d" % s)
def test_the_columns_are_the_exact_change_of_a_qp_solution(shape):
    """kkt_instance is a quadratic objective with affine rows: the solution of the equality-constrained problem with x_B fixed is affine
    in x_B, so (x, lam, z)(x_B + t e_j) - (x, lam, z)(x_B) = t * column, for t = 0.5 and every j of B.  Signs and the dz convention
    against something other than the recipe."""
    fm, x0, lam0, rs, bs = kkt_instance(*shape)[:5]
    H, J = _matrices(fm, x0, lam0)
    pr = fm.to_problem()
    c = np.asarray(pr.eval_grad_f(np.zeros(fm.n), np.zeros(fm.n)), float)
    assert np.allclose(np.asarray(pr.eval_grad_f(x0, np.zeros(fm.n)), float), H @ x0 + c, rtol=0, atol=1e-12)      # f is that quadratic
    B = np.nonzero(bs != 0)[0]
    xB, b, t = x0[B].copy(), np.ones(int(rs.sum())), 0.5
    base = _qp_solution(fm, H, J, c, rs, bs, xB, b)
    cols = sensitivity.var_bound_reference(fm, base[0], base[1], rs, bs, B)
    H2, J2 = _matrices(fm, *base[:2])
    RU, RW, D = sensitivity.var_bound_rhs(H2, J2, fm.n, fm.m, bs, B)
    rec = sensitivity.kkt_reference_multi(fm, base[0], base[1], rs, bs, RU, RW)
    worst = 0.0
    for q, j in enumerate(B):
        moved = xB.copy()
        moved[q] += t
        after = _qp_solution(fm, H, J, c, rs, bs, moved, b)
        for name, a0, a1, col, rcol in zip(("x", "lam", "z"), base, after, cols, (rec[0] + D, rec[1], rec[2])):
            for which, cc in (("reference", col[q]), ("recipe", rcol[q])):
                err = rel_err(a1 - a0, t * cc)
                worst = max(worst, err)
                assert err <= KKT_BAR, (shape, int(j), name, which, err)
        assert np.any(after[2] != base[2]) and np.any(after[1] != base[1])
    print("shape %r: largest rel err of a finite move against t * column %.3e (bar %.3e)" % (shape, worst, KKT_BAR))


# ------------------------------------------------------------------------------------------------ 3. adjoint against forward
def _weighted(gx, gl, gz, dx, dlam, dz):
    return float(gx @ dx + gl @ dlam + gz @ dz), float(np.abs(gx * dx).sum() + np.abs(gl * dlam).sum() + np.abs(gz * dz).sum())


def _adjoint_against_forward(tag, fm, x, lam, rs, bs, rng, with_data):
    B, W = np.nonzero(bs != 0)[0], np.nonzero(rs == 1)[0]
    gx, gl, gz = rng.standard_normal(fm.n), rng.standard_normal(fm.m), rng.standard_normal(fm.n)
    out, dbound, dxbound, ax, al = sensitivity.adjoint_reference_z(fm, x, lam, rs, bs, gx, gl, gz)
    gzb = np.where(bs != 0, gz, 0.0)
    # entries of gz on F are ignored
    again = sensitivity.adjoint_reference_z(fm, x, lam, rs, bs, gx, gl, gzb)
    assert all(np.array_equal(a, b) for a, b in zip(again, (out, dbound, dxbound, ax, al)))
    assert not dxbound[bs == 0].any() and not dbound[rs == 0].any() and not ax[bs != 0].any() and np.any(dxbound[B] != 0.0)
    DX, DLAM, DZ = sensitivity.var_bound_reference(fm, x, lam, rs, bs, B)
    worst = 0.0
    for q, j in enumerate(B):
        want, size = _weighted(gx, gl, gzb, DX[q], DLAM[q], DZ[q])
        err, bar = abs(dxbound[j] - want), KKT_BAR * (abs(dxbound[j]) + size)
        worst = max(worst, err / bar)
        assert err <= bar, (tag, "dxbound", int(j), dxbound[j], want)
    RW = np.zeros((len(W), fm.m))
    RW[np.arange(len(W)), W] = -1.0
    FX, FL, FZ = sensitivity.kkt_reference_multi(fm, x, lam, rs, bs, np.zeros((len(W), fm.n)), RW)
    for q, i in enumerate(W):
        want, size = _weighted(gx, gl, gzb, FX[q], FL[q], FZ[q])
        err, bar = abs(dbound[i] - want), KKT_BAR * (abs(dbound[i]) + size)
        worst = max(worst, err / bar)
        assert err <= bar, (tag, "dbound", int(i), dbound[i], want)
    if with_data:
        nd = len(fm.nlp.device[2])
        for rep in range(3):
            dc = rng.standard_normal(nd)
            u, w = block_cross(fm, x, lam, dc)
            want, size = _weighted(gx, gl, gzb, *sensitivity.kkt_reference(fm, x, lam, rs, bs, u, w))
            got = float(out @ dc)
            err, bar = abs(got - want), KKT_BAR * (float(np.abs(out * dc).sum()) + size)
            worst = max(worst, err / bar)
            assert np.any(out != 0.0) and err <= bar, (tag, "out . dc", rep, got, want)
    else:
        assert out.shape == (0,)
    # without weights on z: adjoint_reference itself
    plain = sensitivity.adjoint_reference(fm, x, lam, rs, bs, gx, gl)
    zero = sensitivity.adjoint_reference_z(fm, x, lam, rs, bs, gx, gl, np.zeros(fm.n))
    for a, b in zip(plain, (zero[0], zero[1], zero[3], zero[4])):
        assert rel_err(b, a) <= KKT_BAR
    print("%s: |B| = %d, |W| = %d, largest error / bar %.3f" % (tag, len(B), len(W), worst))


def test_adjoint_reference_z_against_forward_columns_on_hs071():
    fm, x, lam, rs, bs = hs071_point()
    _adjoint_against_forward("hs071", fm, x, lam, rs, bs, np.random.default_rng(73), True)


def test_adjoint_reference_z_against_forward_columns_on_a_constructed_qp():
    fm, x, lam, rs, bs = kkt_instance(33, 4, 7)[:5]
    _adjoint_against_forward("constructed QP (33, 4, 7)", fm, x, lam, rs, bs, np.random.default_rng(79), False)


# ------------------------------------------------------------------------------------------------ 4. the symbols
def test_the_header_declares_and_the_library_exports_the_new_entries():
    from activesetmethods_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "asm_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in text and name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    assert "are not part of these entries" not in text
