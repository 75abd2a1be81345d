"""The static row order of the sparse KKT form on the device, through the C ABI (include/asm_hip.h, "The row order of the sparse form":
asm_kkt_set_order, asm_kkt_order_info, asm_kkt_row_order): the KKT entries in sparse form and static order against the dense NumPy
references and against the working-set order on the constructed sparse QPs of tests/test_kkt_sparse_cpu.py, the row order, band and
pairs against the host's, the cache, column independence, switching order and form on one handle, degenerate faces, the fallback and
the SLP-EQP drivers."""
import ctypes as C

import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import _lib, eqp, sensitivity
from tests.test_kkt_sparse_cpu import SPARSE_KKT_BAR, SPARSE_LARGE, SPARSE_SHAPES, SPARSE_TWIN_ERR_MEASURED, sparse_instance_of, sparse_kkt_instance
from tests.test_kkt_sparse_gpu import _two_bands
from tests.test_kkt_static_cpu import band_and_pairs, restricted, row_columns, static_order
from tests.test_kkt_step_cpu import step_errors
from tests.test_nlparams_gpu import _handle_for
from tests.test_sensitivity_cpu import kkt_instance, rel_err
from tests.test_sensitivity_multi_cpu import multi_columns
from tests.test_slp_eqp_cpu import grid14_function_model

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
BAR = SPARSE_KKT_BAR
assert BAR == max(10.0 * SPARSE_TWIN_ERR_MEASURED, 1e-12)
INFO = ("status", "cg_iters", "n_free", "n_rows", "dropped_pivots", "res_stat", "res_feas")
STEP_ONLY = ("boundary", "theta", "norm_normal", "norm_step", "model")
SMALL = (160, 6, 33)
MID = (200, 20, 130)
WS, STATIC = "working-set", "static"


def _open(fm, form, order=WS):
    opt = _handle_for(fm.to_problem(), fm)
    opt.set_kkt_form(form)
    opt.set_kkt_order(order)
    return opt


def _bits(out, c=None, fields=INFO):
    dx, dlam, dz, info = out if c is None else (out[0][c], out[1][c], out[2][c], out[3][c])
    return (dx.tobytes(), dlam.tobytes(), dz.tobytes()) + tuple(getattr(info, k) for k in fields)


def _errs(got, ref):
    return [rel_err(g, w) for g, w in zip(got[:3], ref[:3])]


@pytest.fixture(scope="module")
def cases():
    """shape -> (instance, kkt_reference's answer), once for the module."""
    out = {}
    for shape in SPARSE_SHAPES:
        inst = sparse_instance_of(shape)
        out[shape] = (inst, sensitivity.kkt_reference(*inst))
    return out


@pytest.mark.parametrize("shape", SPARSE_SHAPES, ids=lambda s: "n%d_B%d_W%d" % s)
def test_static_solve_against_the_reference_the_other_order_and_the_host_s_order(cases, shape):
    inst, ref = cases[shape]
    fm, x, lam, rs, bs, ru, rw = inst
    n, nB, nW = shape
    cols = row_columns(fm.to_problem())
    order, all_band = static_order(cols)
    want_rows = restricted(order, rs)
    want_band, want_pairs = band_and_pairs(want_rows, cols)
    opt = _open(fm, "sparse", STATIC)
    oi = opt.kkt_order_info()
    assert (oi.order_requested, oi.order_used, oi.all_band, oi.all_pairs) == (1, 0, 0, 0)
    got = opt.kkt_solve(x, lam, rs, bs, ru, rw)
    fi, oi = opt.kkt_form_info(), opt.kkt_order_info()
    errs = _errs(got, ref)
    print("shape %r static: status %d, %d CG iterations, band %d (host %d, all rows %d), pairs %d (host %d, all rows %d), rel err dx %.3e dlam %.3e dz %.3e (bar %.3e), order %.3f ms"
          % (shape, got[3].status, got[3].cg_iters, fi.band, want_band, oi.all_band, fi.n_pairs, want_pairs, oi.all_pairs, errs[0], errs[1], errs[2], BAR, fi.order_ms))
    assert (fi.form_requested, fi.form_used, fi.order_reused) == (1, 1, 0) and fi.dense_bytes == 0 and fi.sparse_bytes > 0
    assert (oi.order_requested, oi.order_used, oi.all_band) == (1, 1, all_band) and oi.all_pairs == band_and_pairs(order, cols)[1]
    assert np.array_equal(opt.kkt_row_order(), np.array(want_rows, np.int32))
    # (the band of a non-empty working set is reported as at least 1, as in the working-set order)
    assert fi.band == (max(want_band, 1) if nW else 0) and fi.n_pairs == want_pairs and fi.band <= max(all_band, 1)
    if shape == SPARSE_LARGE:
        assert 0 < 2 * fi.band < nW                                    # the banded panel launches
    assert got[3].status == 0 and got[3].n_free == n - nB and got[3].n_rows == nW and got[3].dropped_pivots == 0
    assert max(errs) <= BAR, (shape, errs)
    dx, dlam, dz, _ = got
    assert np.all(dx[bs != 0] == 0.0) and np.all(dlam[rs == 0] == 0.0) and np.all(dz[bs == 0] == 0.0)
    again = opt.kkt_solve(x, lam, rs, bs, ru, rw)
    f2 = opt.kkt_form_info()
    assert _bits(again) == _bits(got) and f2.order_reused == 1 and f2.order_ms == 0.0 and f2.dense_bytes == 0 and (f2.band, f2.n_pairs) == (fi.band, fi.n_pairs)
    opt.close()
    other = _open(fm, "sparse", WS)
    want = other.kkt_solve(x, lam, rs, bs, ru, rw)
    wi, wo = other.kkt_form_info(), other.kkt_order_info()
    assert sorted(other.kkt_row_order()) == sorted(want_rows) and (wo.order_requested, wo.order_used) == (0, 0) and wi.n_pairs == fi.n_pairs
    other.close()
    cross = _errs(got, want)
    print("shape %r static against working-set order (band %d): rel diff dx %.3e dlam %.3e dz %.3e" % (shape, wi.band, cross[0], cross[1], cross[2]))
    assert all(getattr(want[3], k) == getattr(got[3], k) for k in ("status", "n_free", "n_rows", "dropped_pivots"))
    assert max(cross) <= BAR, (shape, cross)


def test_static_multi_columns_and_column_independence(cases):
    inst, _ = cases[(96, 10, 65)]
    fm, x, lam, rs, bs, ru, rw = inst
    RU, RW = multi_columns(inst, 5)
    opt = _open(fm, "sparse", STATIC)
    out = opt.kkt_solve_multi(x, lam, rs, bs, RU, RW)
    assert opt.kkt_form_info().form_used == 1 and opt.kkt_order_info().order_used == 1 and opt.kkt_form_info().dense_bytes == 0
    opt.close()
    for c in range(5):
        ref = sensitivity.kkt_reference(fm, x, lam, rs, bs, RU[c], RW[c])
        errs = _errs((out[0][c], out[1][c], out[2][c]), ref)
        print("column %d: rel err %r (bar %.3e)" % (c, errs, BAR))
        assert out[3][c].status == 0 and max(errs) <= BAR
        one = _open(fm, "sparse", STATIC)
        single = one.kkt_solve_multi(x, lam, rs, bs, RU[c:c + 1], RW[c:c + 1])
        one.close()
        assert _bits(single, 0) == _bits(out, c), c


def test_static_step(cases):
    inst, ref = cases[MID]
    fm, x, lam, rs, bs, ru, rw = inst
    want = eqp.kkt_step_reference(fm, x, lam, rs, bs, ru, rw, 0.5)
    opt = _open(fm, "sparse", STATIC)
    one = opt.kkt_step(x, lam, rs, bs, ru, rw, 0.5)
    ladder = opt.kkt_step_multi(x, lam, rs, bs, np.tile(ru, (3, 1)), np.tile(rw, (3, 1)), np.array([0.5, 0.25, 0.5]))
    assert opt.kkt_form_info().form_used == 1 and opt.kkt_order_info().order_used == 1 and opt.kkt_form_info().order_reused == 1
    opt.close()
    e1 = step_errors(one, want)
    e2 = step_errors((ladder[0][0], ladder[1][0], ladder[2][0], ladder[3][0]), want)
    print("step radius 0.5: boundary %d (reference %d), %d iterations, errors single %.2e block %.2e (bar %.2e)"
          % (one[3].boundary, want[3]["boundary"], one[3].cg_iters, max(e1), max(e2), BAR))
    assert one[3].boundary == want[3]["boundary"] == ladder[3][0].boundary and one[3].status == want[3]["status"] == ladder[3][0].status
    assert max(e1) <= BAR and max(e2) <= BAR
    assert float(np.linalg.norm(one[0])) <= 0.5 * (1.0 + 1e-12)
    assert _bits(ladder, 0, INFO + STEP_ONLY) == _bits(ladder, 2, INFO + STEP_ONLY)          # wherever the column stands
    fresh = _open(fm, "sparse", STATIC)
    single = fresh.kkt_step_multi(x, lam, rs, bs, ru[None], rw[None], np.array([0.25]))
    fresh.close()
    assert _bits(single, 0, INFO + STEP_ONLY) == _bits(ladder, 1, INFO + STEP_ONLY)


def test_switching_order_and_form_on_one_handle():
    """working-set order -> static -> static on a narrower working set -> dense -> static: each answer, one column and a block, is that of a
    fresh handle in that mode bit for bit - the factor the modes share holds nothing of the call before, and the cache of one order is not
    taken for the other's."""
    inst, rs2 = _two_bands()
    fm, x, lam, rs, bs, ru, rw = inst
    RU, RW = multi_columns(inst, 5)
    plan = (("sparse", WS, rs), ("sparse", STATIC, rs), ("sparse", STATIC, rs2), ("dense", STATIC, rs2), ("sparse", STATIC, rs))

    def call(opt, rows):
        return _bits(opt.kkt_solve(x, lam, rows, bs, ru, rw)), [_bits(opt.kkt_solve_multi(x, lam, rows, bs, RU, RW), c) for c in range(5)]
    want, bands = [], []
    for form, order, rows in plan:
        opt = _open(fm, form, order)
        want.append(call(opt, rows))
        bands.append(opt.kkt_form_info().band)
        opt.close()
    opt = _open(fm, "sparse")
    for k, (form, order, rows) in enumerate(plan):
        opt.set_kkt_form(form)
        opt.set_kkt_order(order)
        assert call(opt, rows) == want[k], (k, form, order)
        fi, oi = opt.kkt_form_info(), opt.kkt_order_info()
        assert fi.form_used == (form == "sparse") and fi.band == bands[k] and oi.order_used == (form == "sparse" and order == STATIC)
        assert fi.order_reused == (form == "sparse")                    # (the block call after the one-column call; the dense form has no order)
    opt.close()
    print("bands of the plan: %r" % bands)
    assert 0 < bands[2] < bands[1] and bands[3] == 0


@pytest.mark.parametrize("kind", ["bound_row", "duplicate_row"])
def test_static_dependent_rows_as_the_dense_form(kind):
    inst = sparse_kkt_instance(*SMALL, bound_rows=(5,)) if kind == "bound_row" else sparse_kkt_instance(*SMALL, duplicate_row=True)
    fm, x, lam, rs, bs, ru, rw = inst
    if kind == "duplicate_row":                                          # one right-hand side for the two copies
        J = sensitivity.dense_jacobian(fm, x)
        twins = [(a, b) for a in np.nonzero(rs)[0] for b in np.nonzero(rs)[0] if a < b and np.array_equal(J[a], J[b])]
        assert len(twins) == 1
        rw = rw.copy()
        rw[twins[0][1]] = rw[twins[0][0]]
    outs = {}
    for form in ("sparse", "dense"):
        opt = _open(fm, form, STATIC)
        outs[form] = opt.kkt_solve(x, lam, rs, bs, ru, rw)
        assert opt.kkt_form_info().form_used == (form == "sparse") and opt.kkt_order_info().order_used == (form == "sparse")
        opt.close()
    s, d = outs["sparse"][3], outs["dense"][3]
    print("%s: static status %d dropped %d, dense status %d dropped %d" % (kind, s.status, s.dropped_pivots, d.status, d.dropped_pivots))
    assert (s.status, s.dropped_pivots, s.n_rows, s.n_free) == (d.status, d.dropped_pivots, d.n_rows, d.n_free) and s.status == 3 and s.dropped_pivots == 1
    assert all(np.all(np.isfinite(v)) for v in outs["sparse"][:3])
    assert rel_err(outs["sparse"][0], outs["dense"][0]) <= BAR


def test_static_two_components_and_no_rows(cases):
    inst = sparse_kkt_instance(*SMALL, split=True)
    fm, x, lam, rs, bs, ru, rw = inst
    ref = sensitivity.kkt_reference(*inst)
    opt = _open(fm, "sparse", STATIC)
    got = opt.kkt_solve(x, lam, rs, bs, ru, rw)
    fi = opt.kkt_form_info()
    assert fi.form_used == 1 and got[3].status == 0 and got[3].dropped_pivots == 0 and max(_errs(got, ref)) <= BAR
    none = np.zeros_like(rs)                                            # the same handle without working rows
    got0, ref0 = opt.kkt_solve(x, lam, none, bs, ru, rw), sensitivity.kkt_reference(fm, x, lam, none, bs, ru, rw)
    f0 = opt.kkt_form_info()
    assert (f0.form_used, f0.band, f0.n_pairs) == (1, 0, 0) and len(opt.kkt_row_order()) == 0
    assert got0[3].status == 0 and got0[3].n_rows == 0 and max(_errs(got0, ref0)) <= BAR
    assert _bits(opt.kkt_solve(x, lam, rs, bs, ru, rw)) == _bits(got)
    opt.close()
    inst0, ref00 = cases[(128, 0, 0)]
    multi = _open(inst0[0], "sparse", STATIC)
    RU, RW = multi_columns(inst0, 3)
    out = multi.kkt_solve_multi(*inst0[1:5], RU, RW)
    assert multi.kkt_form_info().form_used == 1 and max(_errs((out[0][0], out[1][0], out[2][0]), ref00)) <= BAR
    multi.close()


def test_fallback_to_the_dense_form_and_errors():
    fm, x, lam, rs, bs, ru, rw = kkt_instance(96, 10, 63)                # dense rows: the library keeps no sparse pattern
    outs = {}
    for form in ("sparse", "dense"):
        opt = _open(fm, form, STATIC)
        outs[form] = _bits(opt.kkt_solve(x, lam, rs, bs, ru, rw)), _bits(opt.kkt_step(x, lam, rs, bs, ru, rw, 0.5), fields=INFO + STEP_ONLY), \
            _bits(opt.kkt_solve_multi(x, lam, rs, bs, np.stack([ru, 2 * ru]), np.stack([rw, -rw])), 1)
        fi, oi = opt.kkt_form_info(), opt.kkt_order_info()
        assert (fi.form_requested, fi.form_used, fi.band, fi.n_pairs, fi.sparse_bytes) == (int(form == "sparse"), 0, 0, 0, 0) and fi.dense_bytes > 0
        assert (oi.order_requested, oi.order_used, oi.all_band, oi.all_pairs) == (1, 0, 0, 0)
        assert np.array_equal(opt.kkt_row_order(), np.nonzero(rs)[0])   # ascending in the dense form
        opt.close()
    assert outs["sparse"] == outs["dense"]
    fm = sparse_kkt_instance(*SMALL)[0]
    opt = _handle_for(fm.to_problem(), fm)
    lib, info, nW = opt._lib, _lib.KktOrderInfo(), C.c_int64(7)
    for bad in (2, -1, 7):
        assert lib.asm_kkt_set_order(opt._h, bad) == ERR_ARG
    assert lib.asm_kkt_order_info(opt._h, None) == ERR_ARG and lib.asm_kkt_set_order(None, 1) == ERR_ARG and lib.asm_kkt_order_info(None, C.byref(info)) == ERR_ARG
    assert lib.asm_kkt_row_order(opt._h, None, None) == ERR_ARG and lib.asm_kkt_row_order(None, None, C.byref(nW)) == ERR_ARG
    assert lib.asm_kkt_row_order(opt._h, None, C.byref(nW)) == 0 and nW.value == 0          # no KKT call yet
    for bad in ("rcm", "Static", None, 1):
        with pytest.raises(ValueError):
            opt.set_kkt_order(bad)
    assert opt.kkt_order_info().order_requested == 0                    # the refused values changed nothing
    opt.set_kkt_order(STATIC)
    assert opt.kkt_order_info().order_requested == 1 and opt.kkt_form_info().form_requested == 0
    opt.eval_setup(fm)                                                    # a new evaluator starts from the working-set order
    assert opt.kkt_order_info().order_requested == 0
    opt.close()
    pr = fm.to_problem()
    bare = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    assert bare._lib.asm_kkt_set_order(bare._h, 1) == ERR_STATE and bare._lib.asm_kkt_order_info(bare._h, C.byref(info)) == ERR_STATE
    assert bare._lib.asm_kkt_row_order(bare._h, None, C.byref(nW)) == ERR_STATE
    bare.close()


def test_slp_eqp_drivers_in_static_order():
    runs = {}
    for form in ("sparse", "dense"):
        par = dict(algorithm="SLP-EQP", device_eval=True, max_iter=60, kkt_form=form, kkt_order=STATIC)
        mdl = A.Model.from_problem(grid14_function_model().to_problem("grid14"), A.Parameters(**par))
        slp = A.optimize(mdl)
        fi, oi = slp.optimizer.kkt_form_info(), slp.optimizer.kkt_order_info()
        slp.optimizer.close()
        native = A.Model.from_problem(grid14_function_model().to_problem("grid14"), A.Parameters(**par))
        run = A.optimize(native, native=True)
        print("grid14 %s static: host status %d iter %d %r | native status %d iter %d %r; form used %d order requested %d used %d band %d"
              % (form, slp.ret, slp.iter, slp.eqp_counts, run.ret, run.iter, run.eqp_counts, fi.form_used, oi.order_requested, oi.order_used, fi.band))
        assert (fi.form_requested, oi.order_requested) == (int(form == "sparse"), 1)
        assert (run.ret, run.iter, run.lp_solves) == (slp.ret, slp.iter, slp.lp_solves) and run.ret == 0
        assert run.eqp_counts == slp.eqp_counts and run.eqp_counts["accepted"] > 0 and run.Delta_E == slp.Delta_E
        assert np.array_equal(run.x, slp.x) and np.array_equal(run.lam, slp.lam) and np.array_equal(run.E, slp.E)
        assert np.array_equal(run.mult_x_U, slp.mult_x_U) and np.array_equal(run.mult_x_L, slp.mult_x_L)
        runs[form] = run
    # converges as the dense form does: the same status (the objective values are printed, a record)
    s, d = runs["sparse"], runs["dense"]
    print("objective sparse-static %.12g, dense %.12g, iterations %d / %d" % (s.obj_val, d.obj_val, s.iter, d.iter))
    assert s.ret == d.ret == 0
    with pytest.raises(ValueError):
        A.Parameters(kkt_order="other")
