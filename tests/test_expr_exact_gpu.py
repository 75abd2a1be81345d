"""The expression kernels' derivatives against exact math through the handle API: the table, the bars and the checks of
tests/test_expr_exact_cpu.py (read its docstring first) with the device behind them - asm_eval_functions, asm_eval_jacobian_values,
asm_eval_hessian_lagrangian, asm_eval_hessian_product, asm_eval_data_gradient, asm_eval_data_cross, asm_eval_data_cross_t.  One set-up and
one call (or a few, one per unit weight) per entry cover the 2 x 446 rows and terms: two workgroups of k_nlp_expr_rows, _terms,
_const_adj, _hess, _cross, _cross_t and their gathers, the second one partly past R, T and S.  The objective's value is a sum over terms of
every size and is not compared; the terms' derivatives are.

DEVICE_L is the device math library's error per function, measured on the MI355X by test_device_library_errors_are_as_recorded the way
NUMPY_L is on the host ("Expression derivatives against exact math", has the figures)."""
import numpy as np
import pytest

from activesetmethods_amd import batch
from tests.test_expr_exact_cpu import (EXPONENT_SCENARIOS, KKT_BAR, NUMPY_L, POSITION_X, assert_sweeps, check_asin_acos, check_positions, check_table,
                                       exponent_model, exponent_solution, measure_library, position_model, position_reference, table_model)
from tests.test_nlparams_gpu import _handle_for

pytestmark = pytest.mark.gpu

# largest error in eps |exact| over the table -> doubled, rounded up, at least 1 (the figures: DESIGN.md)
DEVICE_L = {"sqrt": 1, "exp": 1, "log": 1, "sin": 1, "cos": 1, "tan": 1, "asin": 1, "acos": 1, "atan": 1, "sinh": 1, "cosh": 1, "tanh": 1,
            "log10": 1, "log2": 1, "log1p": 1, "expm1": 1, "cbrt": 1, "pow": 2, "atan2": 1}


class Device:
    """The handle behind the calls of check_table / check_positions (the Twin of tests/test_expr_exact_cpu.py on the device)."""

    def __init__(self, fm):
        self.fm, self.pr = fm, fm.to_problem("expr exact")
        assert fm.nlp_constraint_offset == 0
        self.opt = _handle_for(self.pr, fm)

    def close(self):
        self.opt.close()

    def row_values(self, x):
        return self.opt.eval_functions(x)[2]

    def jacobian(self, x):
        self.opt.eval_functions(x)
        return np.asarray(self.pr.j_row) - 1, np.asarray(self.pr.j_col) - 1, self.opt.jacobian_values()

    def gradient(self, x):
        return self.opt.eval_functions(x)[1]

    def hessian(self, x, obj_factor, lam):
        r, c = self.opt.hessian_structure()
        return r - 1, c - 1, self.opt.eval_hessian_lagrangian(x, obj_factor, lam)

    def hessian_product(self, x, obj_factor, lam, v):
        return self.opt.hessian_product(x, obj_factor, lam, v)

    def data_gradient(self, x, lam):
        return self.opt.eval_data_gradient(x, lam)

    def data_cross(self, x, lam, dc):
        return self.opt.data_cross(x, lam, dc)

    def data_cross_t(self, x, lam, vx, vl):
        return self.opt.data_cross_t(x, lam, vx, vl)


def test_device_library_errors_are_as_recorded():
    def values(fm, xv):
        dev = Device(fm)
        try:
            return dev.row_values(xv)
        finally:
            dev.close()
    worst = measure_library(values)
    for f in sorted(worst):
        print("%-6s largest error %.3f eps |exact|   L = %d" % (f, worst[f], DEVICE_L[f]))
    assert set(worst) == set(DEVICE_L) == set(NUMPY_L)
    assert {f: max(1, int(np.ceil(2.0 * q))) for f, q in worst.items()} == DEVICE_L


@pytest.mark.parametrize("sense", ["MIN_SENSE", "MAX_SENSE"])
def test_every_sweep_of_the_device_against_exact_math(sense):
    fm, recs, xv = table_model(sense)
    dev = Device(fm)
    try:
        sweeps = check_table(dev, fm, recs, xv, DEVICE_L, seed=len(sense))
    finally:
        dev.close()
    assert_sweeps(sweeps)


def test_asin_and_acos_lose_nothing_to_cancellation_on_the_device():
    fm, recs, xv = table_model()
    dev = Device(fm)
    try:
        worst = check_asin_acos(dev, fm, recs, xv, DEVICE_L)
    finally:
        dev.close()
    assert max(worst) <= 1.0


@pytest.mark.parametrize("sense", ["MIN_SENSE", "MAX_SENSE"])
def test_data_derivatives_in_every_position_on_the_device(sense):
    fm = position_model(sense)
    exact = position_reference(fm, POSITION_X)
    dev = Device(fm)
    try:
        check_positions(dev, fm, POSITION_X, *exact, seed=len(sense))
    finally:
        dev.close()


def test_solution_sensitivity_to_an_exponent_parameter_single_handle():
    """asm_solution_sensitivity and asm_solution_adjoint along the exponent q against the closed forms (a vertex: no CG iteration)."""
    for q, a in EXPONENT_SCENARIOS:
        fm = exponent_model(q, a)
        x, lam, wx, wl = exponent_solution(q, a)
        rs, bs = np.ones(2, np.int32), np.zeros(2, np.int32)
        dc = np.zeros(len(fm.nlp.device[2]))
        dc[0] = 1.0
        opt = _handle_for(fm.to_problem("exponent"), fm)
        dx, dlam, dz, info = opt.solution_sensitivity(x, lam, rs, bs, dc)
        gx, gl = np.array([1.0, -2.0]), np.array([0.5, 3.0])
        out, dbound, ax, al, ainfo = opt.solution_adjoint(x, lam, rs, bs, gx, gl)
        opt.close()
        print("q %g a %g: dx %r (exact %r), dlam %r (exact %r), adjoint %r" % (q, a, dx, wx, dlam, wl, out[0]))
        assert info.status == 0 and ainfo.status == 0 and not dz.any()
        assert np.abs(dx - wx).max() <= KKT_BAR * max(1.0, np.abs(wx).max()) and np.abs(dlam - wl).max() <= KKT_BAR * max(1.0, np.abs(wl).max())
        want = float(gx @ wx + gl @ wl)
        assert abs(out[0] - want) <= KKT_BAR * max(1.0, abs(want)), (out[0], want)
        assert wx[1] != 0.0 and wl[1] != 0.0


def test_solution_sensitivity_to_an_exponent_parameter_scenario_batch():
    """The same through asm_batch_solution_sensitivity and asm_batch_solution_adjoint: one batch of 3 slots, a scenario per (q, a)."""
    S = len(EXPONENT_SCENARIOS)
    fms = [exponent_model(q, a) for q, a in EXPONENT_SCENARIOS]
    prs = [fm.to_problem("exponent %d" % s) for s, fm in enumerate(fms)]
    sol = [exponent_solution(q, a) for q, a in EXPONENT_SCENARIOS]
    X, LAM = np.stack([s[0] for s in sol]), np.stack([s[1] for s in sol])
    rs, bs = np.ones((S, 2), np.int32), np.zeros((S, 2), np.int32)
    nd = len(fms[0].nlp.device[2])
    hb = batch.HipBatch(prs[0], 3)
    data = hb.scenario_data(prs)
    assert data is not None and data.shape == (S, nd)
    hb.set_scenario_data(data)
    DC = np.zeros((1, nd))
    DC[0, 0] = 1.0
    DX, DLAM, DZ, infos = hb.solution_sensitivity_multi(X, LAM, rs, bs, DC)
    GX, GL = np.tile(np.array([1.0, -2.0]), (S, 1, 1)), np.tile(np.array([0.5, 3.0]), (S, 1, 1))
    OUT, DBOUND, AX, AL, ainfos = hb.solution_adjoint(X, LAM, rs, bs, GX, GL)
    hb.close()
    for s, (x, lam, wx, wl) in enumerate(sol):
        assert infos[s][0].status == 0 and ainfos[s][0].status == 0
        assert np.abs(DX[s, 0] - wx).max() <= KKT_BAR * max(1.0, np.abs(wx).max()), (s, DX[s, 0], wx)
        assert np.abs(DLAM[s, 0] - wl).max() <= KKT_BAR * max(1.0, np.abs(wl).max()), (s, DLAM[s, 0], wl)
        want = float(GX[s, 0] @ wx + GL[s, 0] @ wl)
        assert abs(OUT[s, 0, 0] - want) <= KKT_BAR * max(1.0, abs(want)), (s, OUT[s, 0, 0], want)
    assert not np.array_equal(DX[0], DX[1])
