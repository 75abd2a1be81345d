"""Adjoint solution sensitivities on the device through the C ABI (include/asm_hip.h, "Adjoint solution sensitivities":
asm_eval_data_cross_t, asm_solution_adjoint, asm_solution_adjoint_multi): the transposed sweep of the three block kinds against the host
twins - bit for bit where no math-library value enters - the composed call half by half, forward against reverse on hs071 and on the
case118-sized ACOPF in the sparse form, column independence of the multi entry, no interference with the SLP state, errors."""
import ctypes as C

import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import _lib, acopf, nlexpr, problems, sensitivity
from activesetmethods_amd.nlexpr import ExprBlock, parameters, variables
from tests.test_nlexpr_cpu import _model
from tests.test_nlhess_cpu import all_ops_model
from tests.test_nlparams_gpu import _handle_for, _same_run
from tests.test_ohm_hess_cpu import grid
from tests.test_sensitivity_cpu import KKT_BAR, KKT_SHAPES, kkt_instance, rel_err
from tests.test_sensitivity_gpu import LIBM_BAR, _branch_case, _exact_cross_models, hs071_param_model

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
LS, TR = "Line Search", "Trust Region"
CHUNK = 64
D, I = _lib.dptr, _lib.i32ptr


def _weights(fm, rng):
    return rng.standard_normal(fm.m), rng.standard_normal(fm.n), rng.standard_normal(fm.m)


# ------------------------------------------------------------------------------------------------ 4. the primitive, expression blocks
def test_cross_t_is_bit_identical_on_arithmetic_tapes():
    for name, fm in _exact_cross_models():
        opt = _handle_for(fm.to_problem(name), fm)
        rng = np.random.default_rng(len(name))
        for rep in range(2):
            x = fm.start_point() + 0.3 * rng.uniform(-1, 1, fm.n)
            lam, vx, vl = _weights(fm, rng)
            out, twin = opt.data_cross_t(x, lam, vx, vl), sensitivity.model_cross_t(fm, x, lam, vx, vl)
            assert out.shape == twin.shape == (len(fm.nlp.device[2]),) and np.any(twin != 0.0), name
            assert np.array_equal(out, twin), (name, rep, np.abs(out - twin).max())
            assert np.array_equal(opt.data_cross_t(x, lam, vx, vl), out)                 # a second call: equal bits
        opt.close()


def test_cross_t_without_constants_and_with_a_const_exponent():
    x = variables(2)
    nc = _model(ExprBlock([(x[0] * x[1], 0.0, 0.0)], objective=x[0] * x[0], n=2), 2)
    opt = _handle_for(nc.to_problem(), nc)
    out = opt.data_cross_t(np.array([0.3, 0.7]), np.ones(2), np.ones(2), np.ones(2))
    assert out.shape == (0,) and np.array_equal(out, sensitivity.model_cross_t(nc, np.array([0.3, 0.7]), np.ones(2), np.ones(2), np.ones(2)))
    opt.close()
    q = parameters([2.5])
    pw = _model(ExprBlock([(nlexpr.pow(x[0], q[0]) + q[0] * x[1], 0.0, 0.0)], n=2, parameters=q), 2)
    opt = _handle_for(pw.to_problem(), pw)
    xv, lam, vx, vl = np.array([1.3, 0.4]), np.array([0.5, 1.0]), np.array([1.0, -3.0]), np.array([0.25, 2.0])
    out, twin = opt.data_cross_t(xv, lam, vx, vl), sensitivity.model_cross_t(pw, xv, lam, vx, vl)
    # g = x0^q + q x1 with lam 1, vl 2:  out = vx' (-(x0^(q-1) (1 + q log x0), 1)) + 2 (x0^q log x0 + x1); pow and log are the libraries':
    # the closed form and the twin at LIBM_BAR
    lx = float(np.log(1.3))
    want = -(1.3 ** 1.5 * (1.0 + 2.5 * lx)) + 3.0 + 2.0 * (1.3 ** 2.5 * lx + 0.4)
    size = 1.3 ** 1.5 * (1.0 + 2.5 * lx) + 3.0 + 2.0 * (1.3 ** 2.5 * lx + 0.4)
    assert out.shape == (1,) and abs(out[0] - want) <= LIBM_BAR * size and abs(out[0] - twin[0]) <= LIBM_BAR * size
    opt.close()


def test_cross_t_with_math_library_ops():
    rng = np.random.default_rng(5)
    fa, fb = all_ops_model(), _branch_case()
    for name, fm, x in (("all ops", fa, rng.uniform(0.4, 1.1, 4)), ("acopf case118 branch parameters", fb, fb.start_point() + 0.01 * rng.standard_normal(fb.n))):
        opt = _handle_for(fm.to_problem(name), fm)
        lam, vx, vl = _weights(fm, rng)
        out, twin = opt.data_cross_t(x, lam, vx, vl), sensitivity.model_cross_t(fm, x, lam, vx, vl)
        err = rel_err(out, twin)
        print("%s: rel |out - twin| = %.3e (max |out| %.3e, bar %.1e)" % (name, err, np.abs(twin).max(), LIBM_BAR))
        assert err <= LIBM_BAR and np.any(twin != 0.0), (name, err)
        opt.close()


# ------------------------------------------------------------------------------------------------ 5. kinds 4 and 5
def _block_rows_set(fm):
    """The working set {the block's rows}, every variable free: rows with a unit (Ohm's law) or dense random (dense block) Jacobian."""
    rs = np.zeros(fm.m, np.int32)
    rs[fm.nlp_constraint_offset:] = 1
    return rs, np.zeros(fm.n, np.int32)


def _block_columns(name, fm, exact):
    """One column through the primitive and three through the multi entry (the column in blockIdx.y) against the twin."""
    opt = _handle_for(fm.to_problem(name), fm)
    rng = np.random.default_rng(len(name))
    x = fm.start_point() + 0.05 * rng.standard_normal(fm.n)
    lam, vx, vl = _weights(fm, rng)
    out, twin = opt.data_cross_t(x, lam, vx, vl), sensitivity.model_cross_t(fm, x, lam, vx, vl)
    err = rel_err(out, twin)
    print("%s, one column: rel |out - twin| = %.3e, equal bits %s" % (name, err, np.array_equal(out, twin)))
    assert out.shape == (len(fm.nlp.device[2]),) and np.any(twin != 0.0)
    assert np.array_equal(out, twin) if exact else err <= LIBM_BAR, (name, err)
    rs, bs = _block_rows_set(fm)
    GX, GL = rng.standard_normal((3, fm.n)), rng.standard_normal((3, fm.m))
    OUT, DBOUND, AX, AL, infos = opt.solution_adjoint_multi(x, lam, rs, bs, GX, GL, max_iter=30, rtol=1e-12)      # (any status: a result)
    assert OUT.shape == (3, len(twin)) and np.all(np.isfinite(OUT))
    for c in range(3):
        tw = sensitivity.model_cross_t(fm, x, lam, -AX[c], AL[c])
        err = rel_err(OUT[c], tw)
        print("%s, column %d of 3: status %d, rel |out - twin| = %.3e" % (name, c, infos[c].status, err))
        assert np.any(tw != 0.0) and np.any(AL[c] != 0.0) and np.any(AX[c] != 0.0), (name, c)
        assert np.array_equal(OUT[c], tw) if exact else err <= LIBM_BAR, (name, c, err)
        assert np.array_equal(OUT[c], opt.data_cross_t(x, lam, -AX[c], AL[c])), (name, c)       # the chunk launch against one column alone
    assert not np.array_equal(OUT[0], OUT[1])
    opt.close()


@pytest.mark.parametrize("name", ["grid14", "case300"])
def test_ohm_block_cross_t_against_the_twin(name):
    case = grid("grid14") if name == "grid14" else acopf.synthetic_case("case300", 1, 0.5)
    fm = acopf.function_model(case, hessian=True)
    assert name == "grid14" or fm.acopf_model.nl > 256                      # a second workgroup
    _block_columns(name, fm, False)


@pytest.mark.parametrize("n,m", [(5, 3), (40, 20)])
def test_dense_block_cross_t_against_the_twin(n, m):
    _block_columns("dense %d x %d" % (n, m), problems.synthetic_dense_function_model(n, m, hessian=True), True)


def test_kinds_without_derivative_entries_raise():
    for fk in (acopf.function_model(grid("grid14")), problems.synthetic_dense_function_model(5, 3)):          # kinds 1 and 2
        pk = fk.to_problem()
        ok = _handle_for(pk, fk)
        with pytest.raises(A.AsmHipError):
            ok.data_cross(pk.x0, np.zeros(pk.m), np.zeros(len(fk.nlp.device[2])))
        with pytest.raises(A.AsmHipError):
            ok.data_cross_t(pk.x0, np.zeros(pk.m), np.zeros(pk.n), np.zeros(pk.m))
        with pytest.raises(A.AsmHipError):
            ok.solution_adjoint(pk.x0, np.zeros(pk.m), np.zeros(pk.m, np.int32), np.zeros(pk.n, np.int32), np.ones(pk.n), np.zeros(pk.m))
        ok.close()


# ------------------------------------------------------------------------------------------------ 6. the composed call, half by half
@pytest.mark.parametrize("shape", KKT_SHAPES, ids=lambda s: "n%d_B%d_W%d" % s)
def test_adjoint_state_against_the_dense_solve(shape):
    fm, x, lam, rs, bs, _, _ = kkt_instance(*shape)
    rng = np.random.default_rng(sum(shape))
    gx, gl = rng.standard_normal(fm.n), rng.standard_normal(fm.m)
    rx, rl, _ = sensitivity.kkt_reference(fm, x, lam, rs, bs, -gx, gl)
    opt = _handle_for(fm.to_problem(), fm)
    out, dbound, ax, al, info = opt.solution_adjoint(x, lam, rs, bs, gx, gl)
    ex, el = rel_err(ax, rx), rel_err(al, rl)
    print("shape %r: status %d, %d CG iterations, rel err ax %.3e al %.3e (bar %.3e)" % (shape, info.status, info.cg_iters, ex, el, KKT_BAR))
    assert info.status == 0 and info.n_free == shape[0] - shape[1] and info.n_rows == shape[2]
    assert ex <= KKT_BAR and el <= KKT_BAR, (shape, ex, el)
    assert out.shape == (0,)                                               # the function store alone has no data
    W = rs == 1
    assert np.array_equal(dbound[W], -al[W]) and np.all(dbound[~W] == 0.0) and np.all(al[~W] == 0.0) and np.all(ax[bs != 0] == 0.0)
    ref = sensitivity.adjoint_reference(fm, x, lam, rs, bs, gx, gl)
    assert rel_err(dbound, ref[1]) <= KKT_BAR
    kx, kl, _, kinfo = opt.kkt_solve(x, lam, rs, bs, -gx, gl)               # the solve it is
    assert np.array_equal(kx, ax) and np.array_equal(kl, al) and kinfo.cg_iters == info.cg_iters
    opt.close()


@pytest.fixture(scope="module")
def hs071_run():
    fm = hs071_param_model()
    pr = fm.to_problem("hs071 rhs parameters")
    opt = _handle_for(pr, fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm=TR, max_iter=60, device_eval=True), 0)
    opt.close()
    rs, bs = sensitivity.working_set(pr, run.x, run.lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    assert run.ret == 0 and rs.tolist() == [1, 1] and bs.tolist() == [-1, 0, 0, 0]
    return fm, pr, run.x, run.lam, rs, bs


def _forward_reverse(tag, opt, x, lam, rs, bs, gx, gl, ks):
    """Test 7's check: out[k] of the adjoint call against gx' dx_k + gl' dlam_k of the forward call along the unit direction of constant k."""
    out, dbound, ax, al, info = opt.solution_adjoint(x, lam, rs, bs, gx, gl)
    assert info.status == 0 and np.array_equal(out, opt.data_cross_t(x, lam, -ax, al))
    W = rs == 1
    assert np.array_equal(dbound[W], -al[W]) and np.all(dbound[~W] == 0.0)
    for k in ks:
        dc = np.zeros(len(out))
        dc[k] = 1.0
        dx, dlam, _, finfo = opt.solution_sensitivity(x, lam, rs, bs, dc)
        u, w = opt.data_cross(x, lam, dc)
        want = float(gx @ dx + gl @ dlam)
        bar = KKT_BAR * (np.abs(gx).sum() * np.abs(dx).max() + np.abs(gl).sum() * np.abs(dlam).max() + np.abs(u).sum() * np.abs(ax).max() + np.abs(w).sum() * np.abs(al).max())
        print("%s constant %d: reverse %.15e, forward %.15e, difference %.3e (bar %.3e)" % (tag, k, out[k], want, abs(out[k] - want), bar))
        assert finfo.status == 0 and want != 0.0 and abs(out[k] - want) <= bar, (tag, k, out[k], want, bar)
    return out, dbound, ax, al


def test_forward_and_reverse_agree_on_hs071(hs071_run):
    fm, pr, x, lam, rs, bs = hs071_run
    opt = _handle_for(pr, fm)
    rng = np.random.default_rng(71)
    for rep in range(2):
        gx, gl = rng.standard_normal(4), rng.standard_normal(2)
        out, dbound, ax, al = _forward_reverse("hs071 %d" % rep, opt, x, lam, rs, bs, gx, gl, (0, 1))
        ref = sensitivity.adjoint_reference(fm, x, lam, rs, bs, gx, gl)
        assert all(rel_err(g, r) <= KKT_BAR for g, r in zip((out, dbound, ax, al), ref))
        got = sensitivity.solution_adjoint(opt, fm, x, lam, rs, bs, gx, gl)
        assert all(np.array_equal(g, r) for g, r in zip(got[:4], (out, dbound, ax, al)))
    opt.close()


# ------------------------------------------------------------------------------------------------ 8. the multi entry
def _adj_bits(res, c):
    OUT, DBOUND, AX, AL, infos = res
    return OUT[c].tobytes(), DBOUND[c].tobytes(), AX[c].tobytes(), AL[c].tobytes(), infos[c].status, infos[c].cg_iters


def acopf_functionals(fm, rs, bs, count, seed):
    """(GX [count x n], GL [count x m]): `count` functions of the solution of an ACOPF model with unit gradients - in turn a line flow (a
    free p-flow variable), a voltage magnitude (a free one) and a price (the multiplier of a working row), drawn with `seed`.  Seeded
    dense gradients are not used at these points: a 6-LP run is not at a solution, and along a random direction in all variables the
    KKT system of its working set is singular to working precision - both entries end at the iteration limit with norms of 1e16, which
    no derivative of a function of the solution is.  Flows, voltages and prices are the functions the entries are for."""
    mdl = fm.acopf_model
    rng = np.random.default_rng(seed)
    pools = [np.array([j for j in idx if bs[j] == 0]) for idx in (mdl.pf, mdl.vm)]
    W = np.nonzero(rs == 1)[0]
    GX, GL = np.zeros((count, fm.n)), np.zeros((count, fm.m))
    for c in range(count):
        if c % 3 == 2:
            GL[c, rng.choice(W)] = 1.0
        else:
            GX[c, rng.choice(pools[c % 3])] = 1.0
    return GX, GL


def _multi_checks(tag, opt, x, lam, rs, bs, GX, GL):
    """Column c of nrhs = 3 and of nrhs = CHUNK + 1 against the same weights alone and at another place, bit for bit; each column against
    the single entry to the KKT bar."""
    assert len(GX) == CHUNK + 1
    all65, first3 = opt.solution_adjoint_multi(x, lam, rs, bs, GX, GL), opt.solution_adjoint_multi(x, lam, rs, bs, GX[:3], GL[:3])
    print("%s: statuses %r, CG iterations %r" % (tag, sorted({i.status for i in all65[4]}), sorted({i.cg_iters for i in all65[4]})))
    assert np.all(np.isfinite(all65[0])) and np.all(np.isfinite(all65[2]))
    for c in range(3):
        assert _adj_bits(all65, c) == _adj_bits(first3, c), (tag, c)
    for c in (0, 2, CHUNK):                                                  # alone, and moved to another place
        alone = opt.solution_adjoint_multi(x, lam, rs, bs, GX[c:c + 1], GL[c:c + 1])
        assert _adj_bits(alone, 0) == _adj_bits(all65, c), (tag, c)
        perm = [1, c, 0]
        moved = opt.solution_adjoint_multi(x, lam, rs, bs, GX[perm], GL[perm])
        assert _adj_bits(moved, 1) == _adj_bits(all65, c), (tag, c)
        out, dbound, ax, al, info = opt.solution_adjoint(x, lam, rs, bs, GX[c], GL[c])
        errs = [rel_err(all65[k][c], one) for k, one in enumerate((out, dbound, ax, al))]
        print("%s column %d: CG iterations multi %d single %d, rel diff out %.3e dbound %.3e ax %.3e al %.3e (bar %.3e)" % ((tag, c, all65[4][c].cg_iters, info.cg_iters)
                                                                                                                   + tuple(errs) + (KKT_BAR,)))
        assert info.status == all65[4][c].status == 0 and max(errs) <= KKT_BAR, (tag, c, errs)
        assert np.any(out != 0.0) or len(out) == 0
        W = rs == 1
        assert np.array_equal(all65[1][c][W], -all65[3][c][W]) and np.all(all65[1][c][~W] == 0.0)
    assert np.any(all65[2][CHUNK] != 0.0) and not np.array_equal(all65[2][0], all65[2][1])


def test_multi_columns_on_the_constructed_qp():
    fm, x, lam, rs, bs, _, _ = kkt_instance(200, 20, 130)
    rng = np.random.default_rng(8)
    opt = _handle_for(fm.to_problem(), fm)
    _multi_checks("(200, 20, 130)", opt, x, lam, rs, bs, rng.standard_normal((CHUNK + 1, fm.n)), rng.standard_normal((CHUNK + 1, fm.m)))
    opt.close()


def test_multi_columns_on_the_case118_sized_ohm_block():
    """The point of test_block_data_gpu.test_solution_sensitivity_on_the_case118_sized_ohm_block (seed 1, load 0.5, a 6-LP run), 65
    flow / voltage / price functions.  Measured on one MI355X: all columns status 0 after 88 to 99 CG iterations; multi against single
    1.0e-14 (a flow), 1.5e-12 (a price: al, 94 against 95 iterations) and 3.9e-14 (a voltage), against the bar of 1.51e-12."""
    fm = acopf.function_model(acopf.synthetic_case("case118", 1, 0.5), hessian=True)
    pr = fm.to_problem("acopf ohm block")
    opt = _handle_for(pr, fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm=LS, max_iter=60, device_eval=True), 6)
    rs, bs = sensitivity.working_set(pr, run.x, run.lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    GX, GL = acopf_functionals(fm, rs, bs, CHUNK + 1, 18)
    _multi_checks("case118 ohm", opt, run.x, run.lam, rs, bs, GX, GL)
    OUT = opt.solution_adjoint_multi(run.x, run.lam, rs, bs, GX[:2], GL[:2])[0]
    assert OUT.shape == (2, len(fm.nlp.device[2])) and np.any(OUT[0] != 0.0)
    opt.close()


# ------------------------------------------------------------------------------------------------ 9. the sparse form
def test_forward_and_reverse_agree_in_the_sparse_form_on_the_acopf():
    fm = _branch_case()
    pr = fm.to_problem("acopf branch parameters")
    opt = _handle_for(pr, fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm=LS, max_iter=60, device_eval=True), 6)
    rs, bs = sensitivity.working_set(pr, run.x, run.lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    opt.set_kkt_form("sparse")
    opt.set_kkt_order("static")
    GX, GL = acopf_functionals(fm, rs, bs, 3, 9)
    nl = fm.acopf_model.nl
    for c, (gx, gl) in enumerate(((GX[0], GL[0]), (GX[0] + GX[1], GL[2]))):          # a line flow; flow + voltage with a price
        _forward_reverse("acopf sparse, function %d" % c, opt, run.x, run.lam, rs, bs, gx, gl, (0, 4 * nl + 1))
    assert opt.kkt_form_info().form_used == 1
    opt.close()


# ------------------------------------------------------------------------------------------------ 10. isolation, errors
def test_the_adjoint_calls_do_not_interfere():
    fm = hs071_param_model()
    pr = fm.to_problem()
    par = A.Parameters(algorithm=TR, max_iter=60, device_eval=True)
    rng = np.random.default_rng(3)
    lam, GX, GL = rng.standard_normal(pr.m), rng.standard_normal((3, pr.n)), rng.standard_normal((3, pr.m))
    outs = []
    for calls in (False, True):
        opt = _handle_for(pr, fm)

        def new_calls(x, lm):
            rs, bs = sensitivity.working_set(pr, x, lm, np.zeros(pr.n), np.zeros(pr.n), tol=1e-6)
            if rs.sum() > (bs == 0).sum():
                rs[:] = 0
            opt.data_cross_t(x, lm, GX[0], GL[0])
            opt.solution_adjoint(x, lm, rs, bs, GX[0], GL[0])
            opt.solution_adjoint_multi(x, lm, rs, bs, GX, GL)
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


def test_argument_and_state_errors():
    """Null pointers, nrhs < 1, wrong kinds and a call before the set-up: the codes of asm_solution_sensitivity_multi."""
    lib = _lib.load()
    fm = hs071_param_model()
    pr = fm.to_problem()
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    K = 2
    x, lam = pr.x0.copy(), np.array([0.5, -0.3])
    DC, GX, GL = np.ones((K, 2)), np.ones((K, 4)), np.ones((K, 2))
    DX, DLAM, DZ = np.zeros((K, 4)), np.zeros((K, 2)), np.zeros((K, 4))
    OUT, DB, AX, AL = np.zeros((K, 2)), np.zeros((K, 2)), np.zeros((K, 4)), np.zeros((K, 2))
    rs, bs = np.array([1, 1], np.int32), np.array([-1, 0, 0, 0], np.int32)
    info = (_lib.KktInfo * K)()
    sens = lambda a: lib.asm_solution_sensitivity_multi(opt._h, *a)
    multi = lambda a: lib.asm_solution_adjoint_multi(opt._h, *a)
    single = lambda a: lib.asm_solution_adjoint(opt._h, *a)
    prim = lambda a: lib.asm_eval_data_cross_t(opt._h, *a)
    sa = [D(x), D(lam), I(rs), I(bs), K, D(DC), None, D(DX), D(DLAM), D(DZ), info]
    ma = [D(x), D(lam), I(rs), I(bs), K, D(GX), D(GL), None, D(OUT), D(DB), D(AX), D(AL), info]
    ga = [D(x), D(lam), I(rs), I(bs), D(GX), D(GL), None, D(OUT), D(DB), D(AX), D(AL), info]
    pa = [D(x), D(lam), D(GX), D(GL), D(OUT)]
    assert sens(sa) == multi(ma) == single(ga) == prim(pa) == ERR_STATE                                   # before asm_eval_setup
    opt.eval_setup(fm)
    assert sens(sa) == multi(ma) == single(ga) == prim(pa) == 0
    assert multi(ma) == 0                                                  # (the single entry and the primitive wrote the first rows)
    first = (OUT.copy(), DB.copy(), AX.copy(), AL.copy())
    for bad, want in ((0, ERR_ARG), (1, ERR_ARG), (2, ERR_ARG), (3, ERR_ARG), (5, ERR_ARG), (6, ERR_ARG), (8, ERR_ARG), (12, ERR_ARG), (7, 0), (9, 0), (10, 0), (11, 0)):
        a = list(ma)                                                       # par, DBOUND, AX and AL may be NULL
        a[bad] = None
        assert multi(a) == want, bad
    for bad, want in ((0, ERR_ARG), (1, ERR_ARG), (2, ERR_ARG), (3, ERR_ARG), (4, ERR_ARG), (5, ERR_ARG), (7, ERR_ARG), (11, ERR_ARG), (6, 0), (8, 0), (9, 0), (10, 0)):
        a = list(ga)
        a[bad] = None
        assert single(a) == want, bad
    for bad in range(5):
        a = list(pa)
        a[bad] = None
        assert prim(a) == ERR_ARG, bad
    for nrhs in (0, -1):
        a, b = list(ma), list(sa)
        a[4], b[4] = nrhs, nrhs
        assert multi(a) == sens(b) == ERR_ARG
    assert lib.asm_solution_adjoint_multi(None, *ma) == lib.asm_solution_sensitivity_multi(None, *sa) == ERR_ARG
    for brs, bbs in ((np.array([2, 1], np.int32), bs), (rs, np.array([2, 0, 0, 0], np.int32)), (rs, np.array([-1, 1, 1, 0], np.int32))):   # a state of 2; |W| > |F|
        a, b, g = list(ma), list(sa), list(ga)
        a[2], a[3], b[2], b[3], g[2], g[3] = I(brs), I(bbs), I(brs), I(bbs), I(brs), I(bbs)
        assert multi(a) == sens(b) == single(g) == ERR_ARG
    assert multi(ma) == 0 and all(np.array_equal(p, q) for p, q in zip((OUT, DB, AX, AL), first))        # the handle works afterwards
    with pytest.raises(ValueError):
        opt.solution_adjoint_multi(x, lam, rs, bs, GX[:, :-1], GL)
    with pytest.raises(ValueError):
        opt.data_cross_t(x, lam, GX[0], GL[0][:-1])
    opt.close()
    for fk in (acopf.function_model(acopf.synthetic_case("case118", 1, 0.5)), problems.synthetic_dense_function_model(40, 10)):      # kinds 1 and 2
        pk = fk.to_problem()
        ok = _handle_for(pk, fk)
        z = lambda *s: np.zeros([max(k, 1) for k in s])
        rs0, bs0 = np.zeros(pk.m, np.int32), np.zeros(pk.n, np.int32)
        nd = len(fk.nlp.device[2])
        one = (_lib.KktInfo * 1)()
        want = lib.asm_solution_sensitivity_multi(ok._h, D(pk.x0), D(z(pk.m)), I(rs0), I(bs0), 1, D(z(1, nd)), None, D(z(1, pk.n)), D(z(1, pk.m)), None, one)
        assert want == ERR_ARG
        assert lib.asm_solution_adjoint_multi(ok._h, D(pk.x0), D(z(pk.m)), I(rs0), I(bs0), 1, D(z(1, pk.n)), D(z(1, pk.m)), None, D(z(1, nd)), None, None, None, one) == want
        assert lib.asm_solution_adjoint(ok._h, D(pk.x0), D(z(pk.m)), I(rs0), I(bs0), D(z(pk.n)), D(z(pk.m)), None, D(z(nd)), None, None, None, one) == want
        assert lib.asm_eval_data_cross_t(ok._h, D(pk.x0), D(z(pk.m)), D(z(pk.n)), D(z(pk.m)), D(z(nd))) == want
        f, df, E = ok.eval_functions(pk.x0)
        assert np.isfinite(f) and np.all(np.isfinite(E))
        ok.close()
