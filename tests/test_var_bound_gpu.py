"""Sensitivities to variable bounds and to the bound multipliers z on the device (include/asm_hip.h: asm_var_bound_sensitivity_multi under
"Many right-hand sides on one factor", asm_solution_adjoint_z(_multi) under "Adjoint solution sensitivities"): the right-hand sides made
on the device against asm_kkt_solve_multi on their host statement, bit for bit, in the dense form and - on the sparse instances - in the
sparse form in both row orders; against the dense system with dx_B = delta imposed; free variables, refusals, column independence across
the chunk boundary; the adjoint entries with and without weights on z against the dense reference; a Line-Search run before and after."""
import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import _lib, acopf, problems, sensitivity
from tests.test_kkt_sparse_cpu import SPARSE_KKT_BAR, sparse_instance_of
from tests.test_nlparams_gpu import _handle_for, _same_run
from tests.test_ohm_hess_cpu import grid
from tests.test_sensitivity_cpu import KKT_BAR, kkt_instance, rel_err
from tests.test_sensitivity_gpu import LIBM_BAR, hs071_param_model

pytestmark = pytest.mark.gpu
ERR_ARG = -1
D, I = _lib.dptr, _lib.i32ptr
LS, TR = "Line Search", "Trust Region"
CHUNK = 64
SHAPES = ((8, 3, 5), (33, 1, 1), (96, 10, 63), (96, 10, 65))


def _info(i):
    return tuple(getattr(i, k) for k, _ in i._fields_)


def _bits(out, c):
    return (out[0][c].tobytes(), out[1][c].tobytes(), out[2][c].tobytes()) + _info(out[3][c])


def _device_rhs(opt, fm, x, lam, vars, delta):
    """(RU, RW) of the columns as the entry states them, from the device's own numbers: RU[c] = delta[c] * (H e_j) by the handle's Hessian
    product, RW[c] = delta[c] * J[:, j] from the device evaluator's Jacobian values (no duplicate pattern entries here)."""
    opt.eval_functions(x)
    vals = opt.jacobian_values()
    r, c = np.asarray(opt.j_row) - 1, np.asarray(opt.j_col) - 1
    assert len(set(zip(r.tolist(), c.tolist()))) == len(r)
    J = np.zeros((fm.m, fm.n))
    J[r, c] = vals
    RU, RW = np.zeros((len(vars), fm.n)), np.zeros((len(vars), fm.m))
    for k, j in enumerate(vars):
        e = np.zeros(fm.n)
        e[j] = 1.0
        RU[k], RW[k] = delta[k] * opt.hessian_product(x, 1.0, -lam, e), delta[k] * J[:, j]
    return RU, RW


def _columns(bs, count, seed):
    """`count` variables of B (each at least once where count allows, then repeats) with seeded moves of both signs."""
    B = np.nonzero(bs != 0)[0]
    vars = np.array([int(B[k % len(B)]) for k in range(count)], np.int32)
    delta = 0.25 + np.random.default_rng(seed).uniform(-2.0, 2.0, count)
    return vars, delta


def _equal_but_the_moved_entry(tag, got, want, vars, delta):
    for c, j in enumerate(vars):
        assert got[0][c, j] == delta[c] and want[0][c, j] == 0.0, (tag, c)
        gx = got[0][c].copy()
        gx[j] = want[0][c, j]
        assert gx.tobytes() == want[0][c].tobytes(), (tag, c, "DX")
        assert _bits(got, c)[1:] == _bits(want, c)[1:], (tag, c)


def _against_the_reference(tag, got, fm, x, lam, rs, bs, vars, delta, bar):
    ref = sensitivity.var_bound_reference(fm, x, lam, rs, bs, vars, delta)
    errs = [rel_err(g, r) for g, r in zip(got[:3], ref)]
    print("%s: statuses %r, CG iterations %r, rel err dx %.3e dlam %.3e dz %.3e (bar %.3e)"
          % ((tag, sorted({i.status for i in got[3]}), sorted({i.cg_iters for i in got[3]})) + tuple(errs) + (bar,)))
    assert all(i.status == 0 for i in got[3]) and max(errs) <= bar, (tag, errs)
    assert np.any(got[2] != 0.0) and np.any(got[1] != 0.0) and not got[2][:, bs == 0].any()


# ------------------------------------------------------------------------------------------------ 1. bit identity, the independent answer
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_B%d_W%d" % s)
def test_columns_equal_the_multi_solve_on_their_right_hand_sides(shape):
    """Fails without the entry.  The dense instances have no sparse pattern: the dense form (the sparse one is the next test's)."""
    fm, x, lam, rs, bs = kkt_instance(*shape)[:5]
    opt = _handle_for(fm.to_problem(), fm)
    for count in (1, shape[1] + 2):
        vars, delta = _columns(bs, count, sum(shape))
        RU, RW = _device_rhs(opt, fm, x, lam, vars, delta)
        got = opt.var_bound_sensitivity_multi(x, lam, rs, bs, vars, delta)
        assert opt.kkt_form_info().form_used == 0
        want = opt.kkt_solve_multi(x, lam, rs, bs, RU, RW)
        _equal_but_the_moved_entry((shape, count), got, want, vars, delta)
        _against_the_reference("shape %r, %d columns" % (shape, count), got, fm, x, lam, rs, bs, vars, delta, KKT_BAR)
    Jx, Jl, Jz = sensitivity.var_bound_jacobian(opt, fm, x, lam, rs, bs, vars[:shape[1]])
    ones = opt.var_bound_sensitivity_multi(x, lam, rs, bs, vars[:shape[1]])
    assert Jx.shape == (fm.n, shape[1]) and Jl.shape == (fm.m, shape[1]) and Jz.shape == (fm.n, shape[1])
    assert np.array_equal(Jx, ones[0].T) and np.array_equal(Jl, ones[1].T) and np.array_equal(Jz, ones[2].T)
    opt.close()


@pytest.mark.parametrize("order", ("working-set", "static"))
@pytest.mark.parametrize("shape", ((96, 10, 63), (96, 10, 65)), ids=lambda s: "n%d_B%d_W%d" % s)
def test_sparse_form_columns_equal_the_multi_solve(shape, order):
    """The sparse instances of tests/test_kkt_sparse_cpu.py: J[:, j] through the CSC column and the position list, in both row orders, a
    row outside W skipped.  The bar against the dense system is that file's (the sparse twin's own error on these instances)."""
    fm, x, lam, rs, bs = sparse_instance_of(shape)[:5]
    opt = _handle_for(fm.to_problem(), fm)
    opt.set_kkt_form("sparse")
    opt.set_kkt_order(order)
    vars, delta = _columns(bs, shape[1] + 2, sum(shape))
    RU, RW = _device_rhs(opt, fm, x, lam, vars, delta)
    J = sensitivity.dense_jacobian(fm, x)
    assert np.any(J[np.ix_(rs == 0, vars)] != 0.0) and np.any(J[np.ix_(rs == 1, vars)] != 0.0)       # entries to skip and entries to take
    got = opt.var_bound_sensitivity_multi(x, lam, rs, bs, vars, delta)
    fi = opt.kkt_form_info()
    assert fi.form_used == 1 and fi.dense_bytes == 0
    want = opt.kkt_solve_multi(x, lam, rs, bs, RU, RW)
    _equal_but_the_moved_entry((shape, order), got, want, vars, delta)
    _against_the_reference("sparse %r, %s order" % (shape, order), got, fm, x, lam, rs, bs, vars, delta, SPARSE_KKT_BAR)
    opt.close()


# ------------------------------------------------------------------------------------------------ 2. a free variable, the refusals
def test_a_free_variable_gives_the_zero_column_and_bad_arguments_are_refused():
    shape = (8, 3, 5)
    fm, x, lam, rs, bs = kkt_instance(*shape)[:5]
    n, m = fm.n, fm.m
    opt = _handle_for(fm.to_problem(), fm)
    B, free = np.nonzero(bs != 0)[0], int(np.nonzero(bs == 0)[0][1])
    vars = [int(B[0]), free, int(B[1])]
    for delta in (np.array([0.5, -2.0, 1.5]), None):
        got = opt.var_bound_sensitivity_multi(x, lam, rs, bs, vars, delta)
        assert not got[0][1].any() and not got[1][1].any() and not got[2][1].any() and got[3][1].status == 0 and got[3][1].cg_iters == 0
        assert np.any(got[0][0] != 0.0) and np.any(got[0][2] != 0.0) and got[3][0].status == 0
    first = opt.var_bound_sensitivity_multi(x, lam, rs, bs, vars)
    lib, info = opt._lib, (_lib.KktInfo * 2)()
    X, L, Z = np.empty((2, n)), np.empty((2, m)), np.empty((2, n))
    rs32, bs32 = np.ascontiguousarray(rs, np.int32), np.ascontiguousarray(bs, np.int32)
    call = lambda nrhs, v: lib.asm_var_bound_sensitivity_multi(opt._h, D(x), D(lam), I(rs32), I(bs32), nrhs, v, None, None, D(X), D(L), D(Z), info)
    for bad in ([0, n], [-1, 0]):                                 # a variable index outside [0, n)
        assert call(2, I(np.array(bad, np.int32))) == ERR_ARG
    assert call(2, None) == ERR_ARG
    assert call(0, I(np.zeros(2, np.int32))) == ERR_ARG and call(-1, I(np.zeros(2, np.int32))) == ERR_ARG
    with pytest.raises(A.AsmHipError):
        opt.var_bound_sensitivity_multi(x, lam, rs, bs, None)
    with pytest.raises(ValueError):
        sensitivity.var_bound_jacobian(opt, fm, x, lam, rs, bs, [free])
    again = opt.var_bound_sensitivity_multi(x, lam, rs, bs, vars)
    assert all(_bits(again, c) == _bits(first, c) for c in range(3))                  # the handle stays usable
    opt.close()
    for fk in (acopf.function_model(grid("grid14")), problems.synthetic_dense_function_model(5, 3)):          # kinds 1 and 2: no exact Hessian
        pk = fk.to_problem()
        ok = _handle_for(pk, fk)
        with pytest.raises(A.AsmHipError):
            ok.var_bound_sensitivity_multi(pk.x0, np.zeros(pk.m), np.zeros(pk.m, np.int32), -np.ones(pk.n, np.int32), [0])
        ok.close()


# ------------------------------------------------------------------------------------------------ 3. column independence, the chunk boundary
def test_a_column_depends_on_its_own_variable_and_move_only():
    shape = (96, 10, 65)
    fm, x, lam, rs, bs = kkt_instance(*shape)[:5]
    opt = _handle_for(fm.to_problem(), fm)
    vars, delta = _columns(bs, CHUNK + 1, 5)
    assert len(set(vars.tolist())) == 10 and len(set(delta.tolist())) == CHUNK + 1
    all65 = opt.var_bound_sensitivity_multi(x, lam, rs, bs, vars, delta)
    assert all(i.status == 0 for i in all65[3])
    for c in (0, 9, 10, CHUNK - 1, CHUNK):                                            # (column CHUNK is alone in the second chunk)
        alone = opt.var_bound_sensitivity_multi(x, lam, rs, bs, vars[c:c + 1], delta[c:c + 1])
        assert _bits(alone, 0) == _bits(all65, c), c
        perm = [3, c, 0]
        moved = opt.var_bound_sensitivity_multi(x, lam, rs, bs, vars[perm], delta[perm])
        assert _bits(moved, 1) == _bits(all65, c), c
    assert _bits(all65, 0)[:3] != _bits(all65, 10)[:3]                                # the same variable, another move
    none, ones = opt.var_bound_sensitivity_multi(x, lam, rs, bs, vars), opt.var_bound_sensitivity_multi(x, lam, rs, bs, vars, np.ones(CHUNK + 1))
    assert all(_bits(none, c) == _bits(ones, c) for c in range(CHUNK + 1))
    assert _bits(none, 0) == _bits(none, 10) and none[0][0, vars[0]] == 1.0
    opt.close()


# ------------------------------------------------------------------------------------------------ 4. the adjoint entries with gz
def _adj_bits(res, c=None):
    arrays, infos = res[:-1], res[-1]
    if c is None:
        return tuple(a.tobytes() for a in arrays) + _info(infos)
    return tuple(a[c].tobytes() for a in arrays) + _info(infos[c])


def _adjoint_z_checks(tag, opt, fm, x, lam, rs, bs, bar, seed, **kw):
    """kw: max_iter and rtol of every call (none: the defaults)."""
    rng = np.random.default_rng(seed)
    n, m = fm.n, fm.m
    on_b = bs != 0
    assert on_b.any() and rs.sum() <= (~on_b).sum()
    GX, GL, GZ = rng.standard_normal((3, n)), rng.standard_normal((3, m)), rng.standard_normal((3, n))
    # without weights: the existing entries' bits, and the new output
    plain, z0 = opt.solution_adjoint(x, lam, rs, bs, GX[0], GL[0], **kw), opt.solution_adjoint_z(x, lam, rs, bs, GX[0], GL[0], **kw)
    assert _adj_bits(plain) == _adj_bits((z0[0], z0[1], z0[3], z0[4], z0[5])), tag
    mplain, mz0 = opt.solution_adjoint_multi(x, lam, rs, bs, GX, GL, **kw), opt.solution_adjoint_z_multi(x, lam, rs, bs, GX, GL, **kw)
    for c in range(3):
        assert _adj_bits(mplain, c) == _adj_bits((mz0[0], mz0[1], mz0[3], mz0[4], mz0[5]), c), (tag, c)
    ref0 = sensitivity.adjoint_reference_z(fm, x, lam, rs, bs, GX[0], GL[0], np.zeros(n))
    assert rel_err(z0[2], ref0[2]) <= bar and rel_err(mz0[2][0], ref0[2]) <= bar and not z0[2][~on_b].any()
    # with weights: the dense reference; entries of gz on F change nothing
    multi = opt.solution_adjoint_z_multi(x, lam, rs, bs, GX, GL, GZ, **kw)
    other = GZ + np.where(on_b, 0.0, 7.0 + rng.standard_normal((3, n)))
    assert all(_adj_bits(opt.solution_adjoint_z_multi(x, lam, rs, bs, GX, GL, other, **kw), c) == _adj_bits(multi, c) for c in range(3)), tag
    worst = 0.0
    for c in range(3):
        ref = sensitivity.adjoint_reference_z(fm, x, lam, rs, bs, GX[c], GL[c], GZ[c])
        one = opt.solution_adjoint_z(x, lam, rs, bs, GX[c], GL[c], GZ[c], **kw)
        assert _adj_bits(opt.solution_adjoint_z(x, lam, rs, bs, GX[c], GL[c], other[c], **kw)) == _adj_bits(one), (tag, c)
        alone = opt.solution_adjoint_z_multi(x, lam, rs, bs, GX[c:c + 1], GL[c:c + 1], GZ[c:c + 1], **kw)
        assert _adj_bits(alone, 0) == _adj_bits(multi, c), (tag, c)
        for name, res, info in (("single", one[:3], one[5]), ("multi", (multi[0][c], multi[1][c], multi[2][c]), multi[5][c])):
            errs = [rel_err(g, r) for g, r in zip(res, ref[:3])]
            worst = max(worst, *errs)
            print("%s function %d, %s: status %d, %d CG iterations, rel err out %.3e dbound %.3e dxbound %.3e (bar %.3e)"
                  % ((tag, c, name, info.status, info.cg_iters) + tuple(errs) + (bar,)))
            assert info.status == 0 and max(errs) <= bar, (tag, c, name, errs)
            assert res[0].shape == ref[0].shape and not res[2][~on_b].any() and np.any(res[2][on_b] != 0.0) and not res[1][rs == 0].any()
        assert not np.array_equal(one[2], z0[2]) and (len(one[0]) == 0 or not np.array_equal(one[0], opt.solution_adjoint_z(x, lam, rs, bs, GX[c], GL[c], **kw)[0]))
    return worst


def _with_a_bound(fm, rs, bs, want=2):
    """bs with at least `want` variables at a bound: the point's own, else the first free variables no working row count forbids."""
    bs = bs.copy()
    for j in np.nonzero(bs == 0)[0]:
        if (bs != 0).sum() >= want or (bs == 0).sum() - 1 < rs.sum():
            break
        bs[j] = -1
    return bs


def test_adjoint_z_on_hs071_at_its_solution():
    fm = hs071_param_model()
    pr = fm.to_problem("hs071 rhs parameters")
    opt = _handle_for(pr, fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm=TR, max_iter=60, device_eval=True), 0)
    rs, bs = sensitivity.working_set(pr, run.x, run.lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    assert run.ret == 0 and rs.tolist() == [1, 1] and bs.tolist() == [-1, 0, 0, 0]       # x1 at its lower bound
    _adjoint_z_checks("hs071", opt, fm, run.x, run.lam, rs, bs, KKT_BAR, 71)
    opt.close()


@pytest.mark.parametrize("form", ("dense", "sparse"))
def test_adjoint_z_on_the_function_store_alone(form):
    fm, x, lam, rs, bs = (kkt_instance(33, 4, 7) if form == "dense" else sparse_instance_of((96, 10, 63)))[:5]
    opt = _handle_for(fm.to_problem(), fm)
    opt.set_kkt_form(form)
    worst = _adjoint_z_checks("function store, %s form" % form, opt, fm, x, lam, rs, bs, KKT_BAR if form == "dense" else SPARSE_KKT_BAR, 5)
    assert opt.kkt_form_info().form_used == (form == "sparse") and worst > 0.0
    assert opt.solution_adjoint_z(x, lam, rs, bs, np.ones(fm.n), np.ones(fm.m), np.ones(fm.n))[0].shape == (0,)          # kind 0: no data
    opt.close()


def test_adjoint_z_on_the_dense_block():
    fm = problems.synthetic_dense_function_model(5, 3, hessian=True)
    pr = fm.to_problem()
    rng = np.random.default_rng(53)
    x, lam = fm.start_point() + 0.3 * rng.uniform(-1, 1, fm.n), 0.05 * rng.standard_normal(fm.m)
    rs, bs = np.array([1, 1, 0], np.int32), np.array([-1, 0, 0, 0, 1], np.int32)
    opt = _handle_for(pr, fm)
    _adjoint_z_checks("dense block (5, 3)", opt, fm, x, lam, rs, bs, KKT_BAR, 53)
    opt.close()


def test_adjoint_z_on_the_ohm_block():
    fm = acopf.function_model(grid("grid14"), hessian=True)
    pr = fm.to_problem("grid14")
    opt = _handle_for(pr, fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm=LS, max_iter=60, device_eval=True), 12)
    rs, bs = sensitivity.working_set(pr, run.x, run.lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    bs = _with_a_bound(fm, rs, bs)
    print("grid14: %d LPs, |W| %d, |B| %d" % (run.lp_solves, rs.sum(), (bs != 0).sum()))
    # The default rtol of the solve is 1e-12 - the bar itself - and it bounds the projected residual, not the error: at this point the
    # lockstep iteration stops one round before the single-column one and its dxbound is 2.1e-12 off the dense solve (dbound 1.2e-12),
    # the single-column answer 1.3e-14.  The bar is about the entries, not about where the iteration is told to stop: rtol = 1e-13 here.
    nF, nW = int((bs == 0).sum()), int(rs.sum())
    _adjoint_z_checks("grid14 ohm block", opt, fm, run.x, run.lam, rs, bs, LIBM_BAR, 14, max_iter=2 * (nF - nW) + 20, rtol=1e-13)
    vars = np.nonzero(bs != 0)[0]
    got = opt.var_bound_sensitivity_multi(run.x, run.lam, rs, bs, vars, None, 2 * (nF - nW) + 20, 1e-13)      # (3.3e-12 in dz at the default rtol)
    _against_the_reference("grid14 ohm block, variable bounds", got, fm, run.x, run.lam, rs, bs, vars, None, KKT_BAR)
    opt.close()


# ------------------------------------------------------------------------------------------------ 5. state
def test_a_line_search_run_returns_its_bits_after_the_calls():
    fm = hs071_param_model()
    pr = fm.to_problem()
    par = A.Parameters(algorithm=LS, max_iter=60, device_eval=True)
    rng = np.random.default_rng(3)
    lam, GX, GL, GZ = rng.standard_normal(pr.m), rng.standard_normal((3, pr.n)), rng.standard_normal((3, pr.m)), rng.standard_normal((3, pr.n))
    outs = []
    for calls in (False, True):
        opt = _handle_for(pr, fm)

        def new_calls(x, lm):
            rs, bs = np.array([1, 1], np.int32), np.array([-1, 0, 0, 0], np.int32)
            opt.var_bound_sensitivity_multi(x, lm, rs, bs, [0, 1, 0], [1.0, 2.0, -0.5])
            opt.solution_adjoint_z(x, lm, rs, bs, GX[0], GL[0], GZ[0])
            opt.solution_adjoint_z_multi(x, lm, rs, bs, GX, GL, GZ)
            opt.solution_adjoint_z_multi(x, lm, rs, bs, GX, GL)
        f0 = opt.eval_functions(pr.x0)
        if calls:
            new_calls(pr.x0 + 0.01, lam)
        run = opt.slp_run(pr.x0, par, 3)
        state = (opt.active_set(), opt.ns_basis(), opt.jacobian_values())
        if calls:
            new_calls(run.x, run.lam)
            after = (opt.active_set(), opt.ns_basis(), opt.jacobian_values())
            assert all(np.array_equal(p, q) for p, q in zip(state[0], after[0])) and np.array_equal(state[1], after[1]) and np.array_equal(state[2], after[2])
        run2 = opt.slp_run(pr.x0, par, 3)
        outs.append((f0, run, run2))
        opt.close()
    (fa, ra, ra2), (fb, rb, rb2) = outs
    assert 1 <= ra.lp_solves <= 3
    _same_run(ra, rb)
    _same_run(ra2, rb2)
    assert fa[0] == fb[0] and np.array_equal(fa[1], fb[1]) and np.array_equal(fa[2], fb[2])
