"""The sparse form of the KKT solve on the device, through the C ABI (include/asm_hip.h, "The form of the KKT solve": asm_kkt_set_form,
asm_kkt_form_info): every KKT entry in sparse form against the dense NumPy references on the constructed sparse QPs of
tests/test_kkt_sparse_cpu.py, against the dense form on a second handle, column independence of the multi entries, degenerate faces,
the order cache, switching forms on one handle, the fallback to the dense form, a case118-sized ACOPF and the SLP-EQP drivers."""
import ctypes as C

import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import _lib, acopf, eqp, problems, sensitivity
from tests.test_kkt_sparse_cpu import SPARSE_KKT_BAR, SPARSE_LARGE, SPARSE_SHAPES, SPARSE_TWIN_ERR_MEASURED, sparse_instance_of, sparse_kkt_instance
from tests.test_kkt_step_cpu import step_errors
from tests.test_nlparams_gpu import _handle_for
from tests.test_sensitivity_cpu import kkt_instance, rel_err
from tests.test_sensitivity_multi_cpu import multi_columns
from tests.test_slp_eqp_cpu import grid14_function_model

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
INF = float("inf")
BAR = SPARSE_KKT_BAR
# 10 x the error of the NumPy twin against the dense solve on these instances (tests/test_kkt_sparse_cpu.py), never below 1e-12
assert BAR == max(10.0 * SPARSE_TWIN_ERR_MEASURED, 1e-12) and 1.8e-11 < BAR < 2e-11
INFO = ("status", "cg_iters", "n_free", "n_rows", "dropped_pivots", "res_stat", "res_feas")
STEP_ONLY = ("boundary", "theta", "norm_normal", "norm_step", "model")
SMALL = (160, 6, 33)
MID = (200, 20, 130)


def _open(fm, form):
    opt = _handle_for(fm.to_problem(), fm)
    opt.set_kkt_form(form)
    return opt


def _bits(out, c=None, fields=INFO):
    dx, dlam, dz, info = out if c is None else (out[0][c], out[1][c], out[2][c], out[3][c])
    return (dx.tobytes(), dlam.tobytes(), dz.tobytes()) + tuple(getattr(info, k) for k in fields)


def _errs(got, ref):
    return [rel_err(g, w) for g, w in zip(got[:3], ref[:3])]


def _residuals(inst, dx, dlam):
    fm, x, lam, rs, bs, ru, rw = inst
    H, J = sensitivity.lagrangian_hessian(fm, x, lam), sensitivity.dense_jacobian(fm, x)
    F, W = bs == 0, rs == 1
    stat = (H @ dx - J[W].T @ dlam[W] + ru)[F]
    feas = J[W] @ dx + rw[W]
    return (float(np.abs(stat).max()) if F.any() else 0.0), (float(np.abs(feas).max()) if W.any() else 0.0)


@pytest.fixture(scope="module")
def cases():
    """shape -> (instance, kkt_reference's answer), once for the module."""
    out = {}
    for shape in SPARSE_SHAPES:
        inst = sparse_instance_of(shape)
        out[shape] = (inst, sensitivity.kkt_reference(*inst))
    return out


# ------------------------------------------------------------------------------------------------ 1., 2. the solve, and the dense form beside it
@pytest.mark.parametrize("shape", SPARSE_SHAPES, ids=lambda s: "n%d_B%d_W%d" % s)
def test_sparse_solve_against_the_reference_and_the_dense_form(cases, shape):
    inst, ref = cases[shape]
    fm, x, lam, rs, bs, ru, rw = inst
    n, nB, nW = shape
    opt = _open(fm, "sparse")
    fresh = opt.kkt_form_info()
    assert (fresh.form_requested, fresh.form_used, fresh.band, fresh.n_pairs, fresh.dense_bytes, fresh.sparse_bytes) == (1, 0, 0, 0, 0, 0)
    got = opt.kkt_solve(x, lam, rs, bs, ru, rw)
    dx, dlam, dz, info = got
    fi = opt.kkt_form_info()
    errs = _errs(got, ref)
    print("shape %r sparse: status %d, %d CG iterations, band %d, pairs %d, rel err dx %.3e dlam %.3e dz %.3e (bar %.3e), res %.3e / %.3e, bytes %d / %d, order %.3f ms"
          % (shape, info.status, info.cg_iters, fi.band, fi.n_pairs, errs[0], errs[1], errs[2], BAR, info.res_stat, info.res_feas, fi.dense_bytes, fi.sparse_bytes, fi.order_ms))
    assert (fi.form_requested, fi.form_used, fi.order_reused) == (1, 1, 0) and fi.dense_bytes == 0 and fi.sparse_bytes > 0
    assert (fi.band > 0) == (nW > 0) and nW <= fi.n_pairs <= 7 * max(nW, 1) and fi.band < max(nW, 1)
    if shape == SPARSE_LARGE:
        assert fi.band < nW / 4
    assert info.status == 0 and info.n_free == n - nB and info.n_rows == nW and info.dropped_pivots == 0
    assert (info.cg_iters == 0) == (n - nB == nW) and info.cg_iters <= 2 * (n - nB - nW) + 20
    assert max(errs) <= BAR, (shape, errs)
    assert np.all(dx[bs != 0] == 0.0) and np.all(dlam[rs == 0] == 0.0) and np.all(dz[bs == 0] == 0.0)
    ws, wf = _residuals(inst, dx, dlam)
    scale = max(1.0, float(np.abs(ru).max()), float(np.abs(rw).max()))
    assert abs(info.res_stat - ws) <= BAR * scale and abs(info.res_feas - wf) <= BAR * scale, (info.res_stat, ws, info.res_feas, wf)
    again = opt.kkt_solve(x, lam, rs, bs, ru, rw)                       # the answer repeats bit for bit (from the cached order)
    assert _bits(again) == _bits(got) and opt.kkt_form_info().order_reused == 1 and opt.kkt_form_info().dense_bytes == 0
    opt.close()
    dense = _open(fm, "dense")
    want = dense.kkt_solve(x, lam, rs, bs, ru, rw)
    di = dense.kkt_form_info()
    dense.close()
    assert (di.form_requested, di.form_used, di.band, di.n_pairs, di.sparse_bytes) == (0, 0, 0, 0, 0) and di.dense_bytes > 0
    assert all(getattr(want[3], k) == getattr(info, k) for k in ("status", "n_free", "n_rows", "dropped_pivots"))
    cross = _errs(got, want)
    print("shape %r sparse against dense: rel diff dx %.3e dlam %.3e dz %.3e, dense against the reference %r" % (shape, cross[0], cross[1], cross[2], _errs(want, ref)))
    assert max(cross) <= BAR, (shape, cross)


# ------------------------------------------------------------------------------------------------ 3. many columns
@pytest.mark.parametrize("shape", [SMALL, (96, 10, 65), MID], ids=lambda s: "n%d_B%d_W%d" % s)
def test_sparse_multi_columns(cases, shape):
    inst, _ = cases[shape]
    fm, x, lam, rs, bs, ru, rw = inst
    RU, RW = multi_columns(inst, 69)
    refs = [sensitivity.kkt_reference(fm, x, lam, rs, bs, RU[c], RW[c]) for c in range(69)]
    opt = _open(fm, "sparse")
    outs = {k: opt.kkt_solve_multi(x, lam, rs, bs, RU[:k], RW[:k]) for k in (1, 8, 33, 69)}
    assert opt.kkt_form_info().form_used == 1 and opt.kkt_form_info().dense_bytes == 0
    worst = 0.0
    for k, out in outs.items():
        for c in range(k):
            worst = max(worst, *_errs((out[0][c], out[1][c], out[2][c]), refs[c]))
            assert out[3][c].status == 0 and out[3][c].dropped_pivots == 0
            assert _bits(out, c) == _bits(outs[69], c), (k, c)                    # whatever nrhs
    print("shape %r: 69 columns, largest relative error %.3e (bar %.3e)" % (shape, worst, BAR))
    assert worst <= BAR
    assert not outs[69][0][1].any() and outs[69][3][1].cg_iters == 0             # the zero column
    order = np.arange(69)[::-1].copy()
    back = opt.kkt_solve_multi(x, lam, rs, bs, RU[order], RW[order])             # ... and wherever it stands
    assert all(_bits(back, k) == _bits(outs[69], int(c)) for k, c in enumerate(order))
    part = opt.kkt_solve_multi(x, lam, rs, bs, RU[60:], RW[60:])
    assert all(_bits(part, c) == _bits(outs[69], 60 + c) for c in range(9))
    one = opt.kkt_solve(x, lam, rs, bs, RU[0], RW[0])                              # the one-column entry: to tolerance
    assert max(_errs(one, (outs[69][0][0], outs[69][1][0], outs[69][2][0]))) <= BAR
    opt.close()


# ------------------------------------------------------------------------------------------------ 4. the trust-region step
@pytest.mark.parametrize("shape", [(128, 0, 0), SMALL, MID], ids=lambda s: "n%d_B%d_W%d" % s)
def test_sparse_step(cases, shape):
    inst, ref = cases[shape]
    fm, x, lam, rs, bs, ru, rw = inst
    opt = _open(fm, "sparse")
    solve, step = opt.kkt_solve(x, lam, rs, bs, ru, rw), opt.kkt_step(x, lam, rs, bs, ru, rw, INF)
    assert _bits(solve) == _bits(step) and step[3].boundary == 0 and step[3].theta == 1.0
    RU, RW = multi_columns(inst, 3)
    ms, mt = opt.kkt_solve_multi(x, lam, rs, bs, RU, RW), opt.kkt_step_multi(x, lam, rs, bs, RU, RW, np.full(3, INF))
    assert all(_bits(ms, c) == _bits(mt, c) for c in range(3))
    full = float(np.linalg.norm(ref[0]))
    radii = full * np.array([0.05, 0.3, 0.6, 0.9, 1.5])
    ladder = opt.kkt_step_multi(x, lam, rs, bs, np.tile(ru, (5, 1)), np.tile(rw, (5, 1)), radii)
    for c, rad in enumerate(radii):
        want = eqp.kkt_step_reference(fm, x, lam, rs, bs, ru, rw, rad)
        one = opt.kkt_step(x, lam, rs, bs, ru, rw, rad)
        e1 = step_errors(one, want)
        e2 = step_errors((ladder[0][c], ladder[1][c], ladder[2][c], ladder[3][c]), want)
        e3 = step_errors((ladder[0][c], ladder[1][c], ladder[2][c], ladder[3][c]), one[:3] + ({k: getattr(one[3], k) for k in STEP_ONLY},))
        print("shape %r radius %.3g: boundary %d / %d (reference %d), %d iterations, errors single %.2e ladder %.2e ladder against single %.2e"
              % (shape, rad, one[3].boundary, ladder[3][c].boundary, want[3]["boundary"], one[3].cg_iters, max(e1), max(e2), max(e3)))
        assert one[3].boundary == want[3]["boundary"] == ladder[3][c].boundary and one[3].status == want[3]["status"] == ladder[3][c].status
        assert max(e1) <= BAR and max(e2) <= BAR and max(e3) <= BAR, (shape, rad, e1, e2, e3)
        norm = float(np.linalg.norm(one[0]))
        assert norm <= rad * (1.0 + 1e-12) and abs(one[3].norm_step - norm) <= 1e-14 * max(1.0, norm)
    assert opt.kkt_form_info().form_used == 1 and opt.kkt_form_info().dense_bytes == 0
    opt.close()


# ------------------------------------------------------------------------------------------------ 5. degenerate faces
@pytest.mark.parametrize("kind", ["bound_row", "duplicate_row"])
def test_sparse_dependent_rows_as_the_dense_form(kind):
    inst = sparse_kkt_instance(*SMALL, bound_rows=(5,)) if kind == "bound_row" else sparse_kkt_instance(*SMALL, duplicate_row=True)
    fm, x, lam, rs, bs, ru, rw = inst
    if kind == "duplicate_row":                                          # one right-hand side for the two copies: whichever the factor keeps, dx is the same
        J = sensitivity.dense_jacobian(fm, x)
        twins = [(a, b) for a in np.nonzero(rs)[0] for b in np.nonzero(rs)[0] if a < b and np.array_equal(J[a], J[b])]
        assert len(twins) == 1
        rw = rw.copy()
        rw[twins[0][1]] = rw[twins[0][0]]
    outs = {}
    for form in ("sparse", "dense"):
        opt = _open(fm, form)
        outs[form] = opt.kkt_solve(x, lam, rs, bs, ru, rw)
        assert opt.kkt_form_info().form_used == (form == "sparse")
        opt.close()
    s, d = outs["sparse"][3], outs["dense"][3]
    print("%s: sparse status %d dropped %d, dense status %d dropped %d" % (kind, s.status, s.dropped_pivots, d.status, d.dropped_pivots))
    assert (s.status, s.dropped_pivots, s.n_rows, s.n_free) == (d.status, d.dropped_pivots, d.n_rows, d.n_free) and s.status == 3 and s.dropped_pivots == 1
    assert all(np.all(np.isfinite(v)) for v in outs["sparse"][:3])
    # (the rows that stay determine dx: the least-squares answer of both forms)
    assert rel_err(outs["sparse"][0], outs["dense"][0]) <= BAR


def test_sparse_two_components_and_no_rows(cases):
    inst = sparse_kkt_instance(*SMALL, split=True)
    fm, x, lam, rs, bs, ru, rw = inst
    ref = sensitivity.kkt_reference(*inst)
    opt = _open(fm, "sparse")
    got = opt.kkt_solve(x, lam, rs, bs, ru, rw)
    fi = opt.kkt_form_info()
    print("two components: band %d pairs %d errors %r" % (fi.band, fi.n_pairs, _errs(got, ref)))
    assert fi.form_used == 1 and got[3].status == 0 and got[3].dropped_pivots == 0 and max(_errs(got, ref)) <= BAR
    none = np.zeros_like(rs)                                            # the same handle without working rows
    got0, ref0 = opt.kkt_solve(x, lam, none, bs, ru, rw), sensitivity.kkt_reference(fm, x, lam, none, bs, ru, rw)
    f0 = opt.kkt_form_info()
    assert (f0.form_used, f0.band, f0.n_pairs) == (1, 0, 0) and got0[3].status == 0 and got0[3].n_rows == 0 and max(_errs(got0, ref0)) <= BAR
    assert _bits(opt.kkt_solve(x, lam, rs, bs, ru, rw)) == _bits(got)
    opt.close()
    inst0, ref00 = cases[(128, 0, 0)]
    multi = _open(inst0[0], "sparse")
    RU, RW = multi_columns(inst0, 3)
    out = multi.kkt_solve_multi(*inst0[1:5], RU, RW)
    assert multi.kkt_form_info().form_used == 1 and max(_errs((out[0][0], out[1][0], out[2][0]), ref00)) <= BAR
    multi.close()


# ------------------------------------------------------------------------------------------------ 6. the order cache
def test_order_cache(cases):
    inst, ref = cases[MID]
    fm, x, lam, rs, bs, ru, rw = inst
    opt = _open(fm, "sparse")
    first = opt.kkt_solve(x, lam, rs, bs, ru, rw)
    f1 = opt.kkt_form_info()
    second = opt.kkt_solve(x, lam, rs, bs, ru, rw)
    f2 = opt.kkt_form_info()
    assert (f1.order_reused, f2.order_reused) == (0, 1) and _bits(first) == _bits(second) and (f1.band, f1.n_pairs) == (f2.band, f2.n_pairs)
    assert f1.order_ms > 0.0 and f2.order_ms == 0.0
    bs2 = bs.copy()
    bs2[np.nonzero(bs == 0)[0][:2]] = 1                                  # another F, the same W: the structure of S is the same
    got, want = opt.kkt_solve(x, lam, rs, bs2, ru, rw), sensitivity.kkt_reference(fm, x, lam, rs, bs2, ru, rw)
    assert opt.kkt_form_info().order_reused == 1 and got[3].status == 0 and max(_errs(got, want)) <= BAR
    multi = opt.kkt_solve_multi(x, lam, rs, bs, ru[None], rw[None])      # the block entry shares the cache
    assert opt.kkt_form_info().order_reused == 1 and max(_errs((multi[0][0], multi[1][0], multi[2][0]), ref)) <= BAR
    rs2 = rs.copy()
    rs2[np.nonzero(rs)[0][::7]] = 0                                      # another W
    got, want = opt.kkt_solve(x, lam, rs2, bs, ru, rw), sensitivity.kkt_reference(fm, x, lam, rs2, bs, ru, rw)
    f3 = opt.kkt_form_info()
    assert f3.order_reused == 0 and f3.n_pairs < f1.n_pairs and got[3].status == 0 and got[3].n_rows == int(rs2.sum()) and max(_errs(got, want)) <= BAR
    back = opt.kkt_solve(x, lam, rs, bs, ru, rw)
    assert opt.kkt_form_info().order_reused == 0 and _bits(back) == _bits(first)
    opt.close()


# ------------------------------------------------------------------------------------------------ 7. switching forms on one handle
def test_switching_forms_on_one_handle(cases):
    """sparse (wide working set) -> dense -> sparse with fewer rows and a narrower band, one column and a block: each answer is that
    of a fresh handle in that form, bit for bit - the factor the forms share holds nothing of the call before."""
    inst, rs2 = _two_bands()
    fm, x, lam, rs, bs, ru, rw = inst
    RU, RW = multi_columns(inst, 5)
    plan = (("sparse", rs), ("dense", rs), ("sparse", rs2), ("dense", rs2), ("sparse", rs))

    def call(opt, rows):
        return _bits(opt.kkt_solve(x, lam, rows, bs, ru, rw)), [_bits(opt.kkt_solve_multi(x, lam, rows, bs, RU, RW), c) for c in range(5)]
    want, bands = [], []
    for form, rows in plan:
        opt = _open(fm, form)
        want.append(call(opt, rows))
        bands.append(opt.kkt_form_info().band)
        opt.close()
    opt = _open(fm, "sparse")
    for k, (form, rows) in enumerate(plan):
        opt.set_kkt_form(form)
        assert call(opt, rows) == want[k], (k, form)
        fi = opt.kkt_form_info()
        assert fi.form_used == (form == "sparse") and fi.band == bands[k]
    assert fi.dense_bytes > 0 and fi.sparse_bytes > 0
    opt.close()
    print("bands of the plan: %r" % bands)
    assert 0 < bands[2] < bands[0] and bands[1] == 0


def _two_bands():
    """An instance and a second working set of it with a narrower band: every second row of the banded order, half the coupling."""
    inst = sparse_kkt_instance(256, 8, 150)
    fm, x, lam, rs, bs, ru, rw = inst
    W = np.nonzero(rs)[0]
    J = sensitivity.dense_jacobian(fm, x)
    first = np.array([np.nonzero(J[r])[0][0] for r in W])
    narrow = rs.copy()
    narrow[W[np.argsort(first, kind="stable")[1::2]]] = 0
    return inst, narrow


def test_a_narrower_band_after_a_wider_one():
    """Two working sets of one model whose bands differ: the second call must not read what the first left outside its band."""
    inst, narrow = _two_bands()
    fm, x, lam, rs, bs, ru, rw = inst
    fresh = _open(fm, "sparse")
    want = fresh.kkt_solve(x, lam, narrow, bs, ru, rw)
    band_n = fresh.kkt_form_info().band
    fresh.close()
    opt = _open(fm, "sparse")
    opt.kkt_solve(x, lam, rs, bs, ru, rw)
    band_w = opt.kkt_form_info().band
    got = opt.kkt_solve(x, lam, narrow, bs, ru, rw)
    opt.close()
    print("bands %d then %d" % (band_w, band_n))
    assert band_n < band_w and _bits(got) == _bits(want) and got[3].status == 0
    assert max(_errs(got, sensitivity.kkt_reference(fm, x, lam, narrow, bs, ru, rw))) <= BAR


# ------------------------------------------------------------------------------------------------ 8. fallback and errors
def test_fallback_to_the_dense_form_and_errors():
    for name, inst in (("dense rows", kkt_instance(96, 10, 63)), ("hs071", None)):
        if inst is None:
            fm = problems.hs071_function_model()
            x, lam = np.array([1.1, 4.6, 3.9, 1.3]), np.array([0.4, -0.2])
            rs, bs = np.array([1, 1], np.int32), np.array([-1, 0, 0, 0], np.int32)
            ru, rw = np.array([0.3, -1.0, 0.5, 2.0]), np.array([0.1, -0.4])
        else:
            fm, x, lam, rs, bs, ru, rw = inst
        outs = {}
        for form in ("sparse", "dense"):
            opt = _open(fm, form)
            outs[form] = _bits(opt.kkt_solve(x, lam, rs, bs, ru, rw)), _bits(opt.kkt_step(x, lam, rs, bs, ru, rw, 0.5), fields=INFO + STEP_ONLY), \
                _bits(opt.kkt_solve_multi(x, lam, rs, bs, np.stack([ru, 2 * ru]), np.stack([rw, -rw])), 1)
            fi = opt.kkt_form_info()
            assert (fi.form_requested, fi.form_used, fi.band, fi.n_pairs, fi.sparse_bytes) == (int(form == "sparse"), 0, 0, 0, 0) and fi.dense_bytes > 0, name
            opt.close()
        assert outs["sparse"] == outs["dense"], name
    fm = sparse_kkt_instance(*SMALL)[0]
    opt = _handle_for(fm.to_problem(), fm)
    lib, info = opt._lib, _lib.KktFormInfo()
    for bad in (2, -1, 7):
        assert lib.asm_kkt_set_form(opt._h, bad) == ERR_ARG
    assert lib.asm_kkt_form_info(opt._h, None) == ERR_ARG and lib.asm_kkt_set_form(None, 1) == ERR_ARG and lib.asm_kkt_form_info(None, C.byref(info)) == ERR_ARG
    with pytest.raises(ValueError):
        opt.set_kkt_form("banded")
    assert opt.kkt_form_info().form_requested == 0                      # the refused values changed nothing
    opt.set_kkt_form("sparse")
    opt.eval_setup(fm)                                                    # a new evaluator starts from the dense form
    assert opt.kkt_form_info().form_requested == 0
    opt.close()
    pr = fm.to_problem()
    bare = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    assert bare._lib.asm_kkt_set_form(bare._h, 1) == ERR_STATE and bare._lib.asm_kkt_form_info(bare._h, C.byref(info)) == ERR_STATE
    bare.close()


# ------------------------------------------------------------------------------------------------ 9. a case118-sized ACOPF
def _size(H, J, dx, dlam, *rhs):
    return max(1.0, float(np.abs(H).max() * np.abs(dx).max()), float(np.abs(J).max() * np.abs(dlam).max()), *[float(np.abs(v).max()) for v in rhs if len(v)])


def test_case118_trial_and_sensitivity_in_both_forms():
    fm = acopf.function_model(acopf.synthetic_case("case118", 1, 0.5), nlp="expr")
    pr = fm.to_problem("case118-sized")
    opt = _handle_for(pr, fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm="Line Search", max_iter=60, device_eval=True), 6)
    x, lam = run.x, run.lam
    S = opt.active_set()
    f, df, E = opt.eval_functions(x)
    H, J = sensitivity.lagrangian_hessian(fm, x, lam), sensitivity.dense_jacobian(fm, x)
    nu = np.ones(pr.m)
    trials = {}
    for form in ("dense", "sparse"):
        opt.set_kkt_form(form)
        trials[form] = opt.eqp_trial(x, lam, S[0], S[1], 0.4, nu)
        fi = opt.kkt_form_info()
        assert trials[form][6].skipped == 1 or fi.form_used == (form == "sparse")
    (d0, l0, _, _, rs0, bs0, i0), (d1, l1, _, _, rs1, bs1, i1) = trials["dense"], trials["sparse"]
    size = _size(H, J, d0, l0, df, E)
    print("case118 trial: n %d m %d |W| %d |F| %d skipped %d / %d status %d / %d boundary %d / %d cg %d / %d, |d - d'| %.3e |lam - lam'| %.3e (bar %.3e x size %.3e), band %d pairs %d"
          % (pr.n, pr.m, i0.n_rows, i0.n_free, i0.skipped, i1.skipped, i0.status, i1.status, i0.boundary, i1.boundary, i0.cg_iters, i1.cg_iters,
             np.abs(d0 - d1).max(), np.abs(l0 - l1).max(), BAR, size, fi.band, fi.n_pairs))
    assert np.array_equal(rs0, rs1) and np.array_equal(bs0, bs1) and (i0.skipped, i0.status, i0.boundary, i0.n_rows, i0.n_free) == (i1.skipped, i1.status, i1.boundary, i1.n_rows, i1.n_free)
    assert np.abs(d0 - d1).max() <= BAR * size and np.abs(l0 - l1).max() <= BAR * size
    # the step on the working set of the multipliers (full row rank at this seed and load: tests/test_sensitivity_gpu.py), both forms
    rs, bs = sensitivity.working_set(pr, x, lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    F, W = np.nonzero(bs == 0)[0], np.nonzero(rs == 1)[0]
    assert 0 < len(W) <= len(F)
    rw = np.where(rs == 1, E - np.where(np.isfinite(pr.g_L), pr.g_L, pr.g_U), 0.0)
    steps = {}
    for form in ("dense", "sparse"):
        opt.set_kkt_form(form)
        steps[form] = opt.kkt_step(x, lam, rs, bs, df, rw, 0.4)
        assert opt.kkt_form_info().form_used == (form == "sparse")
    fi = opt.kkt_form_info()
    (dx0, dl0, dz0, s0), (dx1, dl1, dz1, s1) = steps["dense"], steps["sparse"]
    size = _size(H, J, dx0, dl0, df, rw)
    print("case118 step: |W| %d |F| %d band %d pairs %d, status %d / %d boundary %d / %d cg %d / %d, |dx - dx'| %.3e |dlam - dlam'| %.3e (bar x size %.3e)"
          % (len(W), len(F), fi.band, fi.n_pairs, s0.status, s1.status, s0.boundary, s1.boundary, s0.cg_iters, s1.cg_iters, np.abs(dx0 - dx1).max(), np.abs(dl0 - dl1).max(), BAR * size))
    assert (s0.status, s0.boundary, s0.dropped_pivots) == (s1.status, s1.boundary, s1.dropped_pivots) and 0 < fi.band < len(W)
    assert np.abs(dx0 - dx1).max() <= BAR * size and np.abs(dl0 - dl1).max() <= BAR * size
    # asm_solution_sensitivity in sparse form: the dense KKT residual of its answer, recomputed in NumPy from the twin's right-hand sides
    dc = np.random.default_rng(9).standard_normal(len(fm.nlp.device[2]))
    off = fm.nlp_constraint_offset
    ub, wb = fm.nlp.data_cross(x, lam[off:], dc, fm.objective_scale)
    u, w = np.zeros(pr.n), np.zeros(pr.m)
    u[:len(ub)] = ub
    w[off:] = wb
    dx, dlam, dz, info = opt.solution_sensitivity(x, lam, rs, bs, dc)
    # (the dense KKT matrix of this face is singular to numpy.linalg.solve - kkt_reference raises on it - so the check is the one
    # tests/test_sensitivity_gpu.py makes on its case118-sized model: the residual of the device's answer against the size of its terms)
    r1, r2 = H @ dx - J[W].T @ dlam[W] + u, J[W] @ dx + w[W]
    size = _size(H, J, dx, dlam, u, w)
    e1, e2 = float(np.abs(r1[F]).max()) / size, float(np.abs(r2).max()) / size
    print("case118 sensitivity, sparse: status %d, %d CG iterations, relative residuals %.3e / %.3e (bar %.3e, size %.3e)" % (info.status, info.cg_iters, e1, e2, BAR, size))
    assert info.status == 0 and opt.kkt_form_info().form_used == 1 and opt.kkt_form_info().order_reused == 1
    assert np.all(dx[bs != 0] == 0.0) and np.all(dlam[rs == 0] == 0.0) and np.all(dz[F] == 0.0)
    assert e1 <= BAR and e2 <= BAR, (e1, e2)
    assert np.any(dx != 0.0)
    opt.close()


# ------------------------------------------------------------------------------------------------ 10. the SLP-EQP drivers
def test_slp_eqp_drivers_in_sparse_form():
    par = dict(algorithm="SLP-EQP", device_eval=True, max_iter=60, kkt_form="sparse")
    mdl = A.Model.from_problem(grid14_function_model().to_problem("grid14"), A.Parameters(**par))
    slp = A.optimize(mdl)
    host_form = slp.optimizer.kkt_form_info()
    slp.optimizer.close()
    native = A.Model.from_problem(grid14_function_model().to_problem("grid14"), A.Parameters(**par))
    run = A.optimize(native, native=True)
    print("grid14 sparse: host status %d iter %d %r | native status %d iter %d %r; form requested %d used %d band %d"
          % (slp.ret, slp.iter, slp.eqp_counts, run.ret, run.iter, run.eqp_counts, host_form.form_requested, host_form.form_used, host_form.band))
    assert host_form.form_requested == 1
    assert (run.ret, run.iter, run.lp_solves) == (slp.ret, slp.iter, slp.lp_solves) and run.ret == 0
    assert run.eqp_counts == slp.eqp_counts and run.eqp_counts["accepted"] > 0 and run.Delta_E == slp.Delta_E
    assert np.array_equal(run.x, slp.x) and np.array_equal(run.lam, slp.lam) and np.array_equal(run.E, slp.E)
    assert np.array_equal(run.mult_x_U, slp.mult_x_U) and np.array_equal(run.mult_x_L, slp.mult_x_L)
    with pytest.raises(ValueError):
        A.Parameters(kkt_form="other")
