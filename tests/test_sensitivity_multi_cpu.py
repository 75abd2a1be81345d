"""Sensitivity matrices on the host (include/asm_hip.h, "Many right-hand sides on one factor"): the dense reference with a matrix
right-hand side against the single reference, the column-by-column twin of the lockstep iteration against it on the constructed QPs,
the Jacobian helpers against the closed forms of the parametric model through a host stand-in for the device handle, the shape checks
of the Python wrappers and the header's declarations.  No GPU."""
import os
import re

import numpy as np
import pytest

from activesetmethods_amd import problems, sensitivity
from tests.test_sensitivity_cpu import KKT_SHAPES, PARAMETRIC_VALUES, kkt_instance, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kkt_pcg_multi against kkt_reference_multi on KKT_SHAPES with multi_columns(inst, 5): the largest relative error
# test_kkt_pcg_multi_against_the_reference measures on the host (it prints every figure; the worst is dx of shape (96, 10, 63), the
# first random column).  The device bar of tests/test_sensitivity_multi_gpu.py is 10 x this, not below 1e-12 - the factor the project
# grants for the device's summation order and Cholesky.
TWIN_MULTI_ERR_MEASURED = 2.21e-13
KKT_MULTI_BAR = max(10.0 * TWIN_MULTI_ERR_MEASURED, 1e-12)


def multi_columns(inst, nrhs, seed=11):
    """(RU [nrhs x n], RW [nrhs x m]) for an instance of kkt_instance: row 0 the instance's own (ru, rw), row 1 all zero, the others
    seeded standard_normal."""
    fm, x, lam, rs, bs, ru, rw = inst
    rng = np.random.default_rng(seed)
    RU, RW = rng.standard_normal((nrhs, fm.n)), rng.standard_normal((nrhs, fm.m))
    RU[0], RW[0] = ru, rw
    if nrhs > 1:
        RU[1], RW[1] = 0.0, 0.0
    return RU, RW


@pytest.fixture(scope="module")
def multi_references():
    """shape -> (instance, RU, RW, kkt_reference_multi's answer) for five columns, once for the module."""
    out = {}
    for shape in KKT_SHAPES:
        inst = kkt_instance(*shape)
        RU, RW = multi_columns(inst, 5)
        out[shape] = (inst, RU, RW, sensitivity.kkt_reference_multi(*inst[:5], RU, RW))
    return out


def test_kkt_reference_multi_equals_the_reference_column_by_column(multi_references):
    for shape, (inst, RU, RW, (DX, DLAM, DZ)) in multi_references.items():
        fm = inst[0]
        assert DX.shape == (5, fm.n) and DLAM.shape == (5, fm.m) and DZ.shape == (5, fm.n)
        for c in range(5):
            dx, dlam, dz = sensitivity.kkt_reference(*inst[:5], RU[c], RW[c])
            # one LU factorisation with five columns against five factorisations of the same matrix: LAPACK's blocked substitution may
            # round differently from the one-column one - a few units of the last place of the solution's size times cond(K) <= 1e4
            e = max(rel_err(DX[c], dx), rel_err(DLAM[c], dlam), rel_err(DZ[c], dz))
            assert e <= 1e-13, (shape, c, e)
        assert not DX[1].any() and not DLAM[1].any() and not DZ[1].any()
    with pytest.raises(ValueError):
        sensitivity.kkt_reference_multi(*inst[:5], RU[:, :-1], RW)
    with pytest.raises(ValueError):
        sensitivity.kkt_reference_multi(*inst[:5], RU, RW[:-1])


def test_kkt_pcg_multi_against_the_reference(multi_references):
    worst = 0.0
    for shape, (inst, RU, RW, ref) in multi_references.items():
        DX, DLAM, DZ, infos = sensitivity.kkt_pcg_multi(*inst[:5], RU, RW)
        n, nB, nW = shape
        for c in range(5):
            errs = [rel_err(g[c], w[c]) for g, w in zip((DX, DLAM, DZ), ref)]
            print("shape %r column %d: status %d, %d CG iterations, rel err dx %.3e dlam %.3e dz %.3e" % ((shape, c, infos[c]["status"], infos[c]["cg_iters"]) + tuple(errs)))
            assert infos[c]["status"] == 0 and infos[c]["n_free"] == n - nB and infos[c]["n_rows"] == nW and infos[c]["dropped_pivots"] == 0
            assert infos[c]["cg_iters"] <= 2 * (n - nB - nW) + 20 and (infos[c]["cg_iters"] == 0) == (n - nB == nW or c == 1)
            worst = max(worst, *errs)
        assert not DX[1].any() and not DLAM[1].any() and not DZ[1].any()
        one = sensitivity.kkt_pcg(*inst)                                   # column 0 is the instance's own: the single twin's bits
        assert np.array_equal(DX[0], one[0]) and np.array_equal(DLAM[0], one[1]) and np.array_equal(DZ[0], one[2])
    print("largest relative error of kkt_pcg_multi against kkt_reference_multi: %.3e (TWIN_MULTI_ERR_MEASURED %.3e)" % (worst, TWIN_MULTI_ERR_MEASURED))
    # the twin's own bound, as in tests/test_sensitivity_cpu.py; TWIN_MULTI_ERR_MEASURED records what this loop printed
    assert worst <= 1e-10
    assert KKT_MULTI_BAR == max(10.0 * TWIN_MULTI_ERR_MEASURED, 1e-12)


def test_kkt_pcg_multi_statuses_are_per_column():
    neg = np.full(8, 4.0)
    neg[2] = -50.0
    inst = kkt_instance(8, 0, 2, seed=3, diag=neg)
    RU, RW = multi_columns(inst, 2)
    DX, DLAM, DZ, infos = sensitivity.kkt_pcg_multi(*inst[:5], RU, RW)
    assert [i["status"] for i in infos] == [2, 0] and infos[1]["cg_iters"] == 0 and np.all(np.isfinite(DX)) and np.all(np.isfinite(DLAM))
    inst = kkt_instance(200, 20, 130)
    RU, RW = multi_columns(inst, 3)
    infos = sensitivity.kkt_pcg_multi(*inst[:5], RU, RW, max_iter=1)[3]
    assert [(i["status"], i["cg_iters"]) for i in infos] == [(1, 1), (0, 0), (1, 1)]


class TwinHandle:
    """A host stand-in for HipSubOptimizer built on the twins: the two multi calls with the device's signatures and return values."""

    def __init__(self, fm):
        self.fm = fm

    def kkt_solve_multi(self, x, lam, row_state, bound_state, RU, RW, max_iter=None, rtol=None):
        return sensitivity.kkt_pcg_multi(self.fm, x, lam, row_state, bound_state, RU, RW, max_iter, 1e-12 if rtol is None else rtol)

    def solution_sensitivity_multi(self, x, lam, row_state, bound_state, DC, max_iter=None, rtol=None):
        fm = self.fm
        off = fm.nlp_constraint_offset
        RU, RW = np.zeros((len(DC), fm.n)), np.zeros((len(DC), fm.m))
        for c, dc in enumerate(np.asarray(DC, float)):
            u, w = fm.nlp.data_cross(x, np.asarray(lam, float)[off:], dc, fm.objective_scale)
            RU[c, :len(u)], RW[c, off:] = u, w
        return self.kkt_solve_multi(x, lam, row_state, bound_state, RU, RW, max_iter, rtol)


@pytest.mark.parametrize("a,p", PARAMETRIC_VALUES)
def test_jacobians_reproduce_the_closed_forms(a, p):
    """d(x*, lam*) / d(a, p) as in test_kkt_reference_on_the_parametric_model, as matrix columns; a bound of row 0 (x1 x2 - p >= b0)
    moves as p does; along the bound of row 1 (x2 - x1 >= b1): x = (s - b1 / 2, s + b1 / 2) to first order, and the stationarity
    equations (2 a x1 + 1, 2 x2) = lam0 (x2, x1) + lam1 (-1, 1) give dlam0 = (1 - a) / (2 s), dlam1 = 1 + a + 1 / (4 s)."""
    fm = problems.parametric_function_model(a, p)
    s = float(np.sqrt(p))
    x, lam = np.array([s, s]), np.array([a + 1.0 + 0.5 / s, s * (1.0 - a) - 0.5])
    rs, bs = np.ones(2, np.int32), np.zeros(2, np.int32)
    opt = TwinHandle(fm)
    d_a = (np.zeros(2), np.array([1.0, -s]))
    d_p = (np.full(2, 0.5 / s), np.array([-0.25 / p ** 1.5, (1.0 - a) / (2.0 * s)]))
    d_b1 = (np.array([-0.5, 0.5]), np.array([(1.0 - a) / (2.0 * s), 1.0 + a + 0.25 / s]))
    close = lambda got, want: np.all(np.abs(got - want) <= 1e-12 * max(1.0, np.abs(want).max()))
    Jx, Jl = sensitivity.solution_jacobian(opt, fm, x, lam, rs, bs)
    assert Jx.shape == (2, 2) and Jl.shape == (2, 2)
    assert close(Jx[:, 0], d_a[0]) and close(Jl[:, 0], d_a[1]) and close(Jx[:, 1], d_p[0]) and close(Jl[:, 1], d_p[1]), (Jx, Jl)
    Jx1, Jl1 = sensitivity.solution_jacobian(opt, fm, x, lam, rs, bs, indices=[1])
    assert Jx1.shape == (2, 1) and np.array_equal(Jx1[:, 0], Jx[:, 1]) and np.array_equal(Jl1[:, 0], Jl[:, 1])
    Bx, Bl = sensitivity.bound_jacobian(opt, fm, x, lam, rs, bs, [0, 1])
    assert Bx.shape == (2, 2) and Bl.shape == (2, 2)
    assert close(Bx[:, 0], d_p[0]) and close(Bl[:, 0], d_p[1]) and close(Bx[:, 1], d_b1[0]) and close(Bl[:, 1], d_b1[1]), (Bx, Bl)
    with pytest.raises(ValueError):
        sensitivity.solution_jacobian(opt, fm, x, lam, rs, bs, indices=[2])
    with pytest.raises(ValueError):
        sensitivity.bound_jacobian(opt, fm, x, lam, np.array([1, 0], np.int32), bs, [1])       # not a working row
    assert sensitivity.solution_jacobian(opt, fm, x, lam, rs, bs, indices=[])[0].shape == (2, 0)


def test_the_python_wrappers_check_shapes_before_the_call():
    """The wrappers raise ValueError before they reach the C call: a stand-in object with the handle's sizes and no library."""
    import activesetmethods_amd as A

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("the C call %s was reached" % name)
    opt = object.__new__(A.HipSubOptimizer)
    opt.n, opt.m, opt._lib, opt._h, opt._ev_keep = 4, 2, NoLibrary(), None, (None, None, np.zeros(3))
    x, lam, rs, bs = np.zeros(4), np.zeros(2), np.zeros(2, np.int32), np.zeros(4, np.int32)
    good_u, good_w, good_c = np.zeros((3, 4)), np.zeros((3, 2)), np.zeros((3, 3))
    for RU, RW in ((np.zeros((3, 5)), good_w), (good_u, np.zeros((3, 3))), (good_u, np.zeros((2, 2))), (np.zeros(4), np.zeros(2)), (np.zeros((0, 4)), np.zeros((0, 2)))):
        with pytest.raises(ValueError):
            opt.kkt_solve_multi(x, lam, rs, bs, RU, RW)
    for DC in (np.zeros((3, 2)), np.zeros(3), np.zeros((0, 3))):
        with pytest.raises(ValueError):
            opt.solution_sensitivity_multi(x, lam, rs, bs, DC)
    with pytest.raises(ValueError):
        opt.kkt_solve_multi(x[:-1], lam, rs, bs, good_u, good_w)
    with pytest.raises(ValueError):
        opt.solution_sensitivity_multi(x, lam, rs[:-1], bs, good_c)
    with pytest.raises(ValueError):
        opt.kkt_solve_multi(x, lam, rs, bs, good_u, good_w, max_iter=3)
    with pytest.raises(AssertionError, match="asm_kkt_solve_multi"):                        # good shapes do reach the call
        opt.kkt_solve_multi(x, lam, rs, bs, good_u, good_w)
    with pytest.raises(AssertionError, match="asm_solution_sensitivity_multi"):
        opt.solution_sensitivity_multi(x, lam, rs, bs, good_c)


def test_the_header_declares_the_two_entries():
    from activesetmethods_amd import _lib
    text = open(os.path.join(ROOT, "include", "asm_hip.h")).read()
    for name in ("asm_kkt_solve_multi", "asm_solution_sensitivity_multi"):
        assert re.search(r"^int %s\(asm_handle\* h," % name, text, re.M), name
        assert name in _lib.PROTOTYPES
    m = re.search(r"^#define ASM_KKT_CHUNK (\d+)$", text, re.M)
    assert m and int(m.group(1)) % 32 == 0
    assert len(_lib.PROTOTYPES["asm_kkt_solve_multi"][1]) == 13 and len(_lib.PROTOTYPES["asm_solution_sensitivity_multi"][1]) == 12
