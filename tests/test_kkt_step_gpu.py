"""The trust-region step on the device through the C ABI (include/asm_hip.h: asm_kkt_step, asm_kkt_step_multi): an infinite radius is
asm_kkt_solve bit for bit; every shape and finite radius against the independent dense reference of activesetmethods_amd/eqp.py with the
same boundary code and iteration count; a radius ladder and a call across the column chunk, the independence of the columns, different
outcomes in one call, the read-back path, no interference with asm_kkt_solve, one step on hs071, argument and state errors.  The
instances, radii and the bar are those of tests/test_kkt_step_cpu.py, where the reference's decisions on all of them are shown to be
clear of rounding."""
import ctypes as C

import numpy as np
import pytest

from activesetmethods_amd import _lib, eqp, sensitivity
from tests.test_kkt_step_cpu import (FACTORS, HS071_GAIN, HS071_RADIUS, HS071_TOL, KKT_STEP_BAR, ReferenceStepper, hs071_start, kkt_residual, ladder_case,
                                     mixed_case, step_cases, step_errors, vertex_case, wide_case)
from tests.test_nlparams_gpu import _handle_for
from tests.test_sensitivity_cpu import kkt_instance
from tests.test_sensitivity_gpu import hs071_param_model
from tests.test_sensitivity_multi_cpu import multi_columns

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
INF = float("inf")
BAR = KKT_STEP_BAR
assert BAR == 1e-12
D, I = _lib.dptr, _lib.i32ptr
SHARED = ("status", "cg_iters", "n_free", "n_rows", "dropped_pivots", "res_stat", "res_feas")          # the fields asm_kkt_info has
STEP_ONLY = ("boundary", "theta", "norm_normal", "norm_step", "model")
CASE_NAMES = sorted({name.rsplit(" f=", 1)[0] for name, _, _ in step_cases()})


def _column(out, c):
    return out[0][c], out[1][c], out[2][c], out[3][c]


def _bits(out, c=None):
    """Everything a call returned for one column (of a multi call: column c), as comparable bits."""
    dx, dlam, dz, info = out if c is None else _column(out, c)
    return (dx.tobytes(), dlam.tobytes(), dz.tobytes()) + tuple(getattr(info, k) for k in SHARED + STEP_ONLY)


def _agrees(got, ref, what):
    """got = (dx, dlam, dz, asm_kkt_step_info) against kkt_step_reference's answer: the errors at the bar, the same decisions."""
    errs = step_errors(got, ref)
    gi, ri = got[3], ref[3]
    print("%s: theta %.4f boundary %d status %d, %d iterations, rel err dx %.2e dlam %.2e dz %.2e model %.2e theta %.2e norms %.2e %.2e, res %.2e / %.2e" %
          ((what, gi.theta, gi.boundary, gi.status, gi.cg_iters) + tuple(errs) + (gi.res_stat, gi.res_feas)))
    assert (gi.boundary, gi.cg_iters, gi.status) == (ri["boundary"], ri["cg_iters"], ri["status"]), what
    assert (gi.theta < 1.0) == (ri["theta"] < 1.0) and (gi.n_free, gi.n_rows, gi.dropped_pivots) == (ri["n_free"], ri["n_rows"], 0), what
    assert max(errs) <= BAR, (what, errs)


@pytest.fixture(scope="module")
def references():
    """name -> (instance, radius, kkt_step_reference's answer) for the finite radii of step_cases(), once for the module."""
    return {name: (inst, rad, eqp.kkt_step_reference(*inst, rad)) for name, inst, rad in step_cases() if np.isfinite(rad)}


# ------------------------------------------------------------------------------------------------ 1. an infinite radius
@pytest.mark.parametrize("shape", [(8, 0, 0), (8, 3, 5), (96, 10, 65), (200, 20, 130)], ids=lambda s: "n%d_B%d_W%d" % s)
def test_an_infinite_radius_is_the_kkt_solve_bit_for_bit(shape):
    inst = kkt_instance(*shape)
    fm, x, lam, rs, bs, ru, rw = inst
    RU, RW = multi_columns(inst, 3)
    opt = _handle_for(fm.to_problem(), fm)
    pairs = [(opt.kkt_solve(x, lam, rs, bs, ru, rw), opt.kkt_step(x, lam, rs, bs, ru, rw, INF))]
    solve, step = opt.kkt_solve_multi(x, lam, rs, bs, RU, RW), opt.kkt_step_multi(x, lam, rs, bs, RU, RW, np.full(3, INF))
    pairs += [(_column(solve, c), _column(step, c)) for c in range(3)]
    par = dict(max_iter=1, rtol=1e-12)                                     # the iteration limit too
    pairs.append((opt.kkt_solve(x, lam, rs, bs, ru, rw, **par), opt.kkt_step(x, lam, rs, bs, ru, rw, INF, normal_share=0.8, **par)))
    opt.close()
    for want, got in pairs:
        assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3]))
        assert all(getattr(got[3], k) == getattr(want[3], k) for k in SHARED)
        norm = float(np.linalg.norm(got[0]))
        assert got[3].boundary == 0 and got[3].theta == 1.0 and abs(got[3].norm_step - norm) <= 1e-14 * max(1.0, norm)
    assert pairs[-1][1][3].status == (1 if shape[0] - shape[1] > shape[2] else 0)


# ------------------------------------------------------------------------------------------------ 2. against the reference
@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_finite_radius_against_the_reference(references, name):
    opt = None
    for f in FACTORS[:3]:
        inst, rad, ref = references["%s f=%g" % (name, f)]
        fm, x, lam, rs, bs, ru, rw = inst
        opt = opt or _handle_for(fm.to_problem(), fm)
        got = opt.kkt_step(x, lam, rs, bs, ru, rw, rad)
        _agrees(got, ref, "%s f=%g" % (name, f))
        info = got[3]
        norm = float(np.linalg.norm(got[0]))
        assert norm <= rad * (1.0 + 1e-12) and (info.boundary == 0 or abs(norm - rad) <= 1e-12 * rad), (name, f, norm / rad)
        assert abs(info.norm_step - norm) <= 1e-14 * max(1.0, norm)
    opt.close()


# ------------------------------------------------------------------------------------------------ 3. the multi entry
def test_a_radius_ladder_in_one_call():
    inst, RU, RW, radii = ladder_case()
    fm, x, lam, rs, bs = inst[:5]
    opt = _handle_for(fm.to_problem(), fm)
    got = opt.kkt_step_multi(x, lam, rs, bs, RU, RW, radii)
    alone = [opt.kkt_step_multi(x, lam, rs, bs, RU[c:c + 1], RW[c:c + 1], radii[c:c + 1]) for c in range(len(radii))]
    single = [opt.kkt_step(x, lam, rs, bs, RU[c], RW[c], radii[c]) for c in range(len(radii))]
    wide = opt.kkt_step_multi(x, lam, rs, bs, np.tile(RU, (9, 1))[:66], np.tile(RW, (9, 1))[:66], np.tile(radii, 9)[:66])      # the rungs again and again, two chunks
    opt.close()
    for c, rad in enumerate(radii):
        ref = eqp.kkt_step_reference(*inst[:5], RU[c], RW[c], rad)
        _agrees(_column(got, c), ref, "ladder column %d" % c)
        _agrees(single[c], ref, "ladder column %d, single entry" % c)
        assert _bits(got, c) == _bits(alone[c], 0), c                      # a column alone and in the ladder: the same bits
    assert all(_bits(wide, c) == _bits(got, c % len(radii)) for c in range(66))      # ... and in a call of 66 columns, wherever it stands
    assert [i.boundary != 0 for i in got[3]] == [True] * 5 + [False] * 3 and len({i.cg_iters for i in got[3]}) >= 3


def test_a_call_across_the_column_chunk():
    inst, RU, RW, radii = wide_case()
    fm, x, lam, rs, bs = inst[:5]
    opt = _handle_for(fm.to_problem(), fm)
    got = opt.kkt_step_multi(x, lam, rs, bs, RU, RW, radii)
    for c in range(len(radii)):
        _agrees(_column(got, c), eqp.kkt_step_reference(*inst[:5], RU[c], RW[c], radii[c]), "wide column %d" % c)
    for c in (0, 1, 2, 63, 64, 65):
        assert _bits(opt.kkt_step_multi(x, lam, rs, bs, RU[c:c + 1], RW[c:c + 1], radii[c:c + 1]), 0) == _bits(got, c), c
        one = opt.kkt_step(x, lam, rs, bs, RU[c], RW[c], radii[c])
        assert one[3].boundary == got[3][c].boundary and one[3].cg_iters == got[3][c].cg_iters
        assert max(step_errors(one, (got[0][c], got[1][c], got[2][c], {k: getattr(got[3][c], k) for k in STEP_ONLY}))) <= BAR, c
    part = opt.kkt_step_multi(x, lam, rs, bs, RU[60:], RW[60:], radii[60:])
    opt.close()
    assert all(_bits(part, c) == _bits(got, 60 + c) for c in range(6))
    assert got[3][1].cg_iters == 0 and not got[0][1].any() and {i.boundary for i in got[3]} == {0, 1}


# ------------------------------------------------------------------------------------------------ 4. mixed outcomes in one call
def test_mixed_outcomes_in_one_call():
    """Converged inside | the boundary on positive curvature | the boundary along p'Hp <= 0 | g0 = 0, in one call; a vertex shape, where
    no iteration runs, in a call of its own (the shape is the call's).  A frozen column does not depend on its neighbours: every column
    alone, and the columns in the opposite order, return the same bits."""
    inst, RU, RW, radii, want = mixed_case()
    fm, x, lam, rs, bs = inst[:5]
    opt = _handle_for(fm.to_problem(), fm)
    got = opt.kkt_step_multi(x, lam, rs, bs, RU, RW, radii)
    for c in range(4):
        _agrees(_column(got, c), eqp.kkt_step_reference(*inst[:5], RU[c], RW[c], radii[c]), "mixed column %d" % c)
        assert (got[3][c].boundary, got[3][c].status) == want[c]
        assert _bits(opt.kkt_step_multi(x, lam, rs, bs, RU[c:c + 1], RW[c:c + 1], radii[c:c + 1]), 0) == _bits(got, c), c
    back = opt.kkt_step_multi(x, lam, rs, bs, RU[::-1].copy(), RW[::-1].copy(), radii[::-1].copy())
    assert all(_bits(back, 3 - c) == _bits(got, c) for c in range(4))
    assert [i.cg_iters for i in got[3]] == [1, 1, 2, 0] and not got[0][3].any() and got[3][3].model == 0.0
    same_rhs = opt.kkt_step_multi(x, lam, rs, bs, RU[[2, 2]], RW[[2, 2]], np.array([radii[2], INF]))      # a finite and an infinite radius side by side
    assert _bits(same_rhs, 0) == _bits(got, 2) and (same_rhs[3][1].status, same_rhs[3][1].boundary) == (2, 0)
    opt.close()
    inst, RU, RW, radii = vertex_case()
    fm, x, lam, rs, bs = inst[:5]
    opt = _handle_for(fm.to_problem(), fm)
    got = opt.kkt_step_multi(x, lam, rs, bs, RU, RW, radii)
    for c in range(2):
        _agrees(_column(got, c), eqp.kkt_step_reference(*inst[:5], RU[c], RW[c], radii[c]), "vertex column %d" % c)
        _agrees(opt.kkt_step(x, lam, rs, bs, RU[c], RW[c], radii[c]), eqp.kkt_step_reference(*inst[:5], RU[c], RW[c], radii[c]), "vertex column %d, single" % c)
    opt.close()
    assert [i.theta < 1.0 for i in got[3]] == [True, False] and [i.cg_iters for i in got[3]] == [0, 0]
    assert abs(got[3][0].norm_step - 0.8 * radii[0]) <= 1e-12 * radii[0]


# ------------------------------------------------------------------------------------------------ 5. the read-back path
def test_the_active_count_by_copy_and_synchronise_gives_the_same_bits(monkeypatch):
    inst, RU, RW, radii = ladder_case()
    fm, x, lam, rs, bs = inst[:5]
    outs = []
    for spin in ("1", "0"):
        monkeypatch.setenv("ASM_HIP_SPIN", spin)                 # read at asm_create
        opt = _handle_for(fm.to_problem(), fm)
        got = opt.kkt_step_multi(x, lam, rs, bs, RU, RW, radii)
        outs.append([_bits(got, c) for c in range(len(radii))])
        opt.close()
    assert outs[0] == outs[1] and outs[0][0][4] > 0


# ------------------------------------------------------------------------------------------------ 6. no interference
def test_a_step_leaves_the_kkt_solve_alone():
    inst, RU, RW, radii = ladder_case()
    fm, x, lam, rs, bs, ru, rw = inst
    opt = _handle_for(fm.to_problem(), fm)
    bits = lambda o: (o[0].tobytes(), o[1].tobytes(), o[2].tobytes()) + tuple(getattr(o[3], k) for k in SHARED)
    s0, m0 = opt.kkt_solve(x, lam, rs, bs, ru, rw), opt.kkt_solve_multi(x, lam, rs, bs, RU[:2], RW[:2])
    opt.kkt_step(x, lam, rs, bs, ru, rw, radii[1])
    s1 = opt.kkt_solve(x, lam, rs, bs, ru, rw)
    opt.kkt_step_multi(x, lam, rs, bs, RU, RW, radii)
    s2, m1 = opt.kkt_solve(x, lam, rs, bs, ru, rw), opt.kkt_solve_multi(x, lam, rs, bs, RU[:2], RW[:2])
    opt.close()
    assert bits(s0) == bits(s1) == bits(s2) and all(bits(_column(m0, c)) == bits(_column(m1, c)) for c in range(2))


# ------------------------------------------------------------------------------------------------ 7. one step on hs071
def test_eqp_step_on_hs071():
    fm, pr, x, lam = hs071_start()
    zero = np.zeros(4)
    rs, bs = sensitivity.working_set(pr, x, lam, zero, zero, HS071_TOL)
    xr, lr, ir = eqp.eqp_step(ReferenceStepper(fm), fm, pr, x, lam, zero, zero, HS071_RADIUS, tol=HS071_TOL)
    opt = _handle_for(pr, fm)
    x1, lam1, info = eqp.eqp_step(opt, fm, pr, x, lam, zero, zero, HS071_RADIUS, tol=HS071_TOL)
    opt.close()
    before, after = kkt_residual(fm, pr, x, lam, rs, bs), kkt_residual(fm, pr, x1, lam1, rs, bs)
    scale = max(1.0, float(np.abs(xr - x).max()))
    print("hs071: KKT residual %.3e -> %.3e, step error %.3e, multiplier error %.3e" % (before, after, np.abs(x1 - xr).max() / scale, np.abs(lam1 - lr).max()))
    assert np.abs((x1 - x) - (xr - x)).max() <= BAR * scale and np.abs(lam1 - lr).max() <= BAR * max(1.0, float(np.abs(lr).max()))
    assert (info.status, info.boundary, info.cg_iters) == (ir["status"], ir["boundary"], ir["cg_iters"]) and info.theta == 1.0
    assert after * HS071_GAIN <= before and np.all(x1 >= pr.x_L) and np.all(x1 <= pr.x_U)


# ------------------------------------------------------------------------------------------------ 8. errors
def test_argument_and_state_errors_and_the_exports():
    import activesetmethods_amd as A
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "asm_kkt_step") and hasattr(raw, "asm_kkt_step_multi")
    fm = hs071_param_model()
    pr = fm.to_problem()
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    K = 2
    x, lam = pr.x0.copy(), np.array([0.5, -0.3])
    RU, RW, RAD = np.ones((K, 4)), np.ones((K, 2)), np.array([0.5, INF])
    DX, DLAM, DZ = np.zeros((K, 4)), np.zeros((K, 2)), np.zeros((K, 4))
    rs, bs = np.array([1, 1], np.int32), np.array([-1, 0, 0, 0], np.int32)
    info = (_lib.KktStepInfo * K)()
    one = lambda a: lib.asm_kkt_step(opt._h, *a)
    multi = lambda a: lib.asm_kkt_step_multi(opt._h, *a)
    oa = [D(x), D(lam), I(rs), I(bs), D(RU), D(RW), 0.5, None, D(DX), D(DLAM), D(DZ), info]
    ma = [D(x), D(lam), I(rs), I(bs), K, D(RU), D(RW), D(RAD), None, D(DX), D(DLAM), D(DZ), info]
    assert one(oa) == ERR_STATE and multi(ma) == ERR_STATE                                                # before asm_eval_setup
    opt.eval_setup(fm)
    assert one(oa) == 0 and multi(ma) == 0
    for bad in (0, 1, 2, 3, 4, 5, 8, 9, 11):                                                              # par and dz may be NULL
        a = list(oa)
        a[bad] = None
        assert one(a) == ERR_ARG, bad
    for bad in (0, 1, 2, 3, 5, 6, 7, 9, 10, 12):
        a = list(ma)
        a[bad] = None
        assert multi(a) == ERR_ARG, bad
    for a in (oa[:10] + [None, info], ma[:11] + [None, info]):
        assert (one if len(a) == 12 else multi)(a) == 0
    for radius in (0.0, -1.0, float("nan"), -INF):
        a, b = list(oa), list(ma)
        a[6], b[7] = radius, D(np.array([1.0, radius]))
        assert one(a) == ERR_ARG and multi(b) == ERR_ARG, radius
    for share in (0.0, -0.5, 1.0 + 1e-9, float("nan")):
        par = _lib.KktStepParams(10, 1e-12, share)
        a, b = list(oa), list(ma)
        a[7], b[8] = C.byref(par), C.byref(par)
        assert one(a) == ERR_ARG and multi(b) == ERR_ARG, share
    for par in (_lib.KktStepParams(-1, 1e-12, 0.8), _lib.KktStepParams(10, float("nan"), 0.8)):
        a = list(oa)
        a[7] = C.byref(par)
        assert one(a) == ERR_ARG
    par = _lib.KktStepParams(10, 1e-12, 1.0)                                                              # the whole radius to the normal step is allowed
    a = list(oa)
    a[7] = C.byref(par)
    assert one(a) == 0
    for nrhs in (0, -1):
        b = list(ma)
        b[4] = nrhs
        assert multi(b) == ERR_ARG
    assert lib.asm_kkt_step(None, *oa) == ERR_ARG and lib.asm_kkt_step_multi(None, *ma) == ERR_ARG
    for brs, bbs in ((np.array([2, 1], np.int32), bs), (rs, np.array([2, 0, 0, 0], np.int32)), (rs, np.array([-1, 1, 1, 0], np.int32))):   # a state of 2; |W| > |F|
        a, b = list(oa), list(ma)
        a[2], a[3], b[2], b[3] = I(brs), I(bbs), I(brs), I(bbs)
        assert one(a) == ERR_ARG and multi(b) == ERR_ARG
    first = DX.copy()
    assert multi(ma) == 0 and np.array_equal(DX, first)                                                   # the handle works afterwards
    with pytest.raises(ValueError):
        opt.kkt_step_multi(x, lam, rs, bs, RU, RW, RAD[:1])
    with pytest.raises(ValueError):
        opt.kkt_step(x, lam, rs, bs, RU[0], RW[0], 1.0, max_iter=5)
    with pytest.raises(A.AsmHipError):
        opt.kkt_step(x, lam, rs, bs, RU[0], RW[0], 0.0)
    opt.close()
