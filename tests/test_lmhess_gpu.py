"""The limited-memory Hessian on the device through the C ABI (include/asm_hip.h, "Limited-memory Hessian"): asm_lm_product against the
NumPy twin (activesetmethods_amd/lmhess.py) on the explicit pairs of tests/test_lmhess_cpu.py, the independence of the columns;
asm_lm_begin / asm_lm_end on the three kinds of NLP block; asm_kkt_step(_multi) in both forms of the KKT solve on models without second
derivatives; switching the type on one handle; SLP-EQP end to end on the Ohm's-law ACOPF, host driver and native driver bit for bit."""
import ctypes as C

import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import _lib, acopf, eqp, sensitivity
from activesetmethods_amd.lmhess import LMHessian
from tests.test_kkt_step_cpu import KKT_STEP_BAR, hs071_start, step_errors
from tests.test_lmhess_cpu import STORES, rel, spd_pairs
from tests.test_nlparams_gpu import _handle_for

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
INF = float("inf")
PRODUCT_BAR = 1e-11
PAIR_BAR = 1e-11
COLUMNS = (1, 8, 9, 64)
SHARED = ("status", "cg_iters", "n_free", "n_rows", "dropped_pivots", "boundary")


def ohm14():
    return acopf.function_model(acopf.synthetic_grid(14, 5, 20, 1, 0.5))


MODELS = {"hs071": A.problems.hs071_function_model,                              # n = 4, m = 2, expressions (nlp_kind 3)
          "ohm14": ohm14,                                                          # the 14-bus grid, the Ohm's-law kernel (nlp_kind 1)
          "dense": lambda: A.problems.synthetic_dense_function_model(40, 10),      # the dense quadratic block (nlp_kind 2)
          "ohm118": lambda: acopf.function_model(acopf.synthetic_case("case118", 1, 1.0))}      # n = 1 088: reductions over two workgroups


@pytest.fixture(scope="module")
def models():
    """name -> (fm, problem), built where first asked for and once for the module."""
    made = {}

    def get(name):
        if name not in made:
            fm = MODELS[name]()
            made[name] = (fm, fm.to_problem(name))
        return made[name]
    return get


def _open(models, name, memory=None):
    fm, pr = models(name)
    opt = _handle_for(pr, fm)
    if memory is not None:
        opt.set_hessian_type("limited-memory", memory)
    return opt


def _bits(out, c=None):
    dx, dlam, dz, info = out if c is None else (out[0][c], out[1][c], out[2][c], out[3][c])
    return (dx.tobytes(), dlam.tobytes(), dz.tobytes()) + tuple(getattr(info, k) for k in SHARED + ("res_stat", "res_feas", "theta", "norm_normal", "norm_step", "model"))


# ------------------------------------------------------------------------------------------------ 1. the product
@pytest.mark.parametrize("n,memory,pushes", STORES)
def test_product_against_the_twin(models, n, memory, pushes):
    name = {4: "hs071", 1088: "ohm118"}[n]
    assert models(name)[0].n == n
    opt = _open(models, name, memory)
    twin = LMHessian(n, memory)
    S, Y = spd_pairs(n, pushes)
    V = np.random.default_rng(11).standard_normal((64, n))
    assert np.array_equal(opt.lm_product(V[:3]), V[:3]) and opt.lm_info().pairs == 0           # no pairs: the identity
    for s, y in zip(S, Y):
        opt.lm_push_pair(s, y)
        assert twin.push_pair(s, y)
    info = opt.lm_info()
    assert (info.type, info.memory, info.pairs, info.pushed, info.skipped_zero, info.skipped_curvature) == (1, memory, min(memory, pushes), pushes, 0, 0)
    assert abs(info.sigma - twin.sigma) <= PRODUCT_BAR * twin.sigma and info.bytes > 0
    want = twin.product(V)
    single = [opt.lm_product(V[c]) for c in range(64)]
    for cols in COLUMNS:
        got = opt.lm_product(V[:cols])
        err = rel(got, want[:cols])
        print("n %d memory %d pushes %d, %d columns: against the twin %.2e" % (n, memory, pushes, cols, err))
        assert err <= PRODUCT_BAR
        assert all(np.array_equal(got[c], single[c]) for c in range(cols))                     # a column's bits are its own
    back = opt.lm_product(V[::-1].copy())                                                      # ... wherever it stands
    wide = opt.lm_product(np.vstack([V, V[:2]]))                                               # ... and across the 64-column chunk
    assert all(np.array_equal(back[63 - c], single[c]) for c in range(64)) and np.array_equal(wide[64:], np.array(single[:2]))
    # the skip rule on the device: nothing changes, the counters say why
    opt.lm_push_pair(np.zeros(n), Y[0])
    opt.lm_push_pair(S[0], -Y[0])
    info = opt.lm_info()
    assert (info.pairs, info.pushed, info.skipped_zero, info.skipped_curvature) == (min(memory, pushes), pushes + 2, 1, 1)
    assert np.array_equal(opt.lm_product(V[0]), single[0])
    opt.lm_reset()
    assert np.array_equal(opt.lm_product(V[:3]), V[:3]) and opt.lm_info().pairs == 0 and opt.lm_info().sigma == 1.0
    opt.close()


# ------------------------------------------------------------------------------------------------ 2. begin / end
def _grad_lag(fm, x, lam):
    return np.asarray(fm.eval_grad_f(x, np.zeros(fm.n)), float) - sensitivity.dense_jacobian(fm, x).T @ lam


def begin_end_points(fm, pr, name):
    """Points inside the bounds and the multipliers of the steps between them.  The steps are a twentieth of the box (or 0.05) wide, so
    y = the difference of two gradients keeps twelve digits of them.  hs071 starts next to its solution with its multipliers there; its
    second step runs along negative curvature of the Lagrangian (s'y = -0.11 ||s|| ||y||): the device has to refuse it as the twin does.
    Elsewhere the multipliers are small against the objective's curvature.  Every other pair passes the skip rule by a wide margin."""
    rng = np.random.default_rng(5)
    if name == "hs071":
        _, _, x0, lam = hs071_start()
        steps = [np.array([0.0, 0.04, -0.03, 0.02]), np.array([0.0, -0.02, 0.05, 0.03]), np.array([0.0, 0.05, -0.04, 0.01])]
    else:
        x0 = np.clip(pr.x0, pr.x_L, pr.x_U)
        width = np.where(np.isfinite(pr.x_U - pr.x_L), pr.x_U - pr.x_L, 1.0)
        lam = 1e-3 * rng.standard_normal(pr.m)
        steps = [0.05 * np.minimum(width, 1.0) * rng.uniform(0.2, 1.0, pr.n) * np.where(x0 + 0.1 * width <= pr.x_U, 1.0, -1.0) for _ in range(2)]
        steps[1] = 0.5 * steps[1]
    pts = [x0 + sum(steps[:k], np.zeros(pr.n)) for k in range(len(steps) + 1)]
    assert all(np.all(p >= pr.x_L) and np.all(p <= pr.x_U) for p in pts)
    return pts, lam


@pytest.mark.parametrize("name", ["ohm14", "dense", "hs071"])
def test_begin_end_against_the_twin(models, name):
    fm, pr = models(name)
    pts, lam = begin_end_points(fm, pr, name)
    opt, twin = _open(models, name, 5), LMHessian(fm.n, 5)
    probes = np.random.default_rng(3).standard_normal((6, fm.n))
    probes /= np.linalg.norm(probes, axis=1)[:, None]
    opt.lm_end(lam)                                                   # no pending begin: nothing
    assert opt.lm_info().pushed == 0
    opt.eval_functions(pts[0])
    for k in range(1, len(pts)):
        opt.lm_begin(lam)
        twin.begin(pts[k - 1], _grad_lag(fm, pts[k - 1], lam))
        assert opt.lm_info().pending == 1
        opt.eval_functions(pts[k])
        opt.lm_end(lam)
        stored = twin.end(pts[k], _grad_lag(fm, pts[k], lam))
        assert stored is (not (name == "hs071" and k == 2)), "the test's own pairs: all stored but the second of hs071"
        info = opt.lm_info()
        err, serr = rel(opt.lm_product(probes), twin.product(probes)), abs(info.sigma - twin.sigma) / twin.sigma
        print("%s pair %d: sigma %.6g, B on unit probes against the twin %.2e, sigma %.2e" % (name, k, info.sigma, err, serr))
        assert (info.pairs, info.pushed, info.skipped_zero, info.skipped_curvature, info.pending) == (twin.pairs, k, 0, twin.skipped_curvature, 0)
        assert err <= PAIR_BAR and serr <= PAIR_BAR
    before = opt.lm_product(probes)
    opt.lm_end(lam)                                                   # a second end without a begin changes nothing
    info = opt.lm_info()
    assert (info.pairs, info.pushed) == (2, len(pts) - 1) and np.array_equal(opt.lm_product(probes), before)
    opt.close()


# ------------------------------------------------------------------------------------------------ 3. the trust-region step
def step_instance(fm, pr, name):
    """(x, lam, row_state, bound_state, ru, rw, radii): the equality rows as the working set (the first five rows of the dense block),
    every variable free, ru = grad f, a small rw, and a ladder of radii around the length of the unrestricted step."""
    rng = np.random.default_rng(9)
    x = np.clip(pr.x0, pr.x_L, pr.x_U)
    lam = 1e-2 * rng.standard_normal(pr.m)
    rs = (pr.g_L == pr.g_U).astype(np.int32) if name == "ohm14" else (np.arange(pr.m) < 5).astype(np.int32)
    bs = np.zeros(pr.n, np.int32)
    ru = np.asarray(fm.eval_grad_f(x, np.zeros(pr.n)), float)
    rw = np.where(rs == 1, 1e-2 * rng.standard_normal(pr.m), 0.0)
    return x, lam, rs, bs, ru, rw


def _agrees(got, ref, what):
    errs = step_errors(got, ref)
    gi, ri = got[3], ref[3]
    print("%s: theta %.4f boundary %d status %d, %d iterations, errors %s" % (what, gi.theta, gi.boundary, gi.status, gi.cg_iters, " ".join("%.1e" % e for e in errs)))
    assert (gi.boundary, gi.cg_iters, gi.status, gi.n_free, gi.n_rows, gi.dropped_pivots) == (ri["boundary"], ri["cg_iters"], ri["status"], ri["n_free"], ri["n_rows"], 0), what
    assert max(errs) <= KKT_STEP_BAR, (what, errs)


@pytest.mark.parametrize("name", ["ohm14", "dense"])
def test_kkt_step_on_models_without_second_derivatives(models, name):
    fm, pr = models(name)
    x, lam, rs, bs, ru, rw = step_instance(fm, pr, name)
    opt = _open(models, name)
    for call in (lambda: opt.kkt_step(x, lam, rs, bs, ru, rw, 1.0), lambda: opt.kkt_step_multi(x, lam, rs, bs, ru[None], rw[None], [1.0]),
                 lambda: opt.kkt_solve(x, lam, rs, bs, ru, rw)):
        with pytest.raises(A.AsmHipError, match="second derivatives"):              # the exact type: the present refusal
            call()
    opt.set_hessian_type("limited-memory", 5)
    twin = LMHessian(pr.n, 5)
    # three pairs from a matrix of condition 10, as the instances of the bar (tests/test_kkt_step_cpu.py: cond(H) <= 10)
    for s, y in zip(*spd_pairs(pr.n, 3, seed=4, cond=10.0)):
        opt.lm_push_pair(s, y)
        twin.push_pair(s, y)
    full = eqp.kkt_step_pcg(fm, x, lam, rs, bs, ru, rw, INF, hess=twin.product)
    assert full[3]["status"] == 0, "the test's own instance is not solvable"
    radii = np.array([f * full[3]["norm_step"] for f in (0.25, 0.6, 1.5)] + [INF])
    refs = [eqp.kkt_step_pcg(fm, x, lam, rs, bs, ru, rw, r, hess=twin.product) for r in radii]
    RU, RW = np.tile(ru, (len(radii), 1)), np.tile(rw, (len(radii), 1))
    outs = {}
    for form in ("dense", "sparse"):
        opt.set_kkt_form(form)
        single = [opt.kkt_step(x, lam, rs, bs, ru, rw, r) for r in radii]
        ladder = opt.kkt_step_multi(x, lam, rs, bs, RU, RW, radii)
        assert opt.kkt_form_info().form_requested == _lib.KKT_FORMS[form]
        for c, r in enumerate(radii):
            col = (ladder[0][c], ladder[1][c], ladder[2][c], ladder[3][c])
            _agrees(single[c], refs[c], "%s %s radius %.3g" % (name, form, r))
            _agrees(col, refs[c], "%s %s radius %.3g, column %d of the ladder" % (name, form, r, c))
            assert max(step_errors(col, (single[c][0], single[c][1], single[c][2], refs[c][3]))[:3]) <= KKT_STEP_BAR
            alone = opt.kkt_step_multi(x, lam, rs, bs, RU[c:c + 1], RW[c:c + 1], radii[c:c + 1])
            assert _bits(ladder, c) == _bits(alone, 0)                                  # a column alone and in the ladder: the same bits
        solve = opt.kkt_solve(x, lam, rs, bs, ru, rw)                                   # radius = +inf stays asm_kkt_solve bit for bit
        assert all(np.array_equal(a, b) for a, b in zip(solve[:3], single[-1][:3])) and solve[3].cg_iters == single[-1][3].cg_iters
        outs[form] = single
    for c in range(len(radii)):                                                         # the two forms agree at the bar
        d, s = outs["dense"][c], outs["sparse"][c]
        assert max(step_errors(s, (d[0], d[1], d[2], refs[c][3]))[:3]) <= KKT_STEP_BAR
    assert any(r[3]["boundary"] for r in refs) and not refs[-1][3]["boundary"]
    opt.close()


# ------------------------------------------------------------------------------------------------ 4. switching the type
def test_switching_the_type_on_one_handle(models):
    fm, pr = models("hs071")
    _, _, x, lam = hs071_start()
    rs, bs = np.array([1, 1], np.int32), np.array([-1, 0, 0, 0], np.int32)
    ru, rw = np.array([1.0, -2.0, 0.5, 0.25]), np.array([0.1, -0.2])

    def exact(opt):
        return _bits(opt.kkt_step(x, lam, rs, bs, ru, rw, 0.5)) + _bits(opt.kkt_solve(x, lam, rs, bs, ru, rw)[:3] + (opt.kkt_step(x, lam, rs, bs, ru, rw, INF)[3],))

    fresh = _open(models, "hs071")
    want = exact(fresh)
    hess = fresh.eval_hessian_lagrangian(x, 1.0, -lam)
    fresh.close()
    opt = _open(models, "hs071")
    first = exact(opt)
    opt.set_hessian_type("limited-memory", 3)
    for s, y in zip(*spd_pairs(4, 2)):
        opt.lm_push_pair(s, y)
    approx = _bits(opt.kkt_step(x, lam, rs, bs, ru, rw, 0.5))
    # the derivative entries stay exact in this mode
    assert np.array_equal(opt.eval_hessian_lagrangian(x, 1.0, -lam), hess)
    opt.set_hessian_type("exact")
    assert opt.lm_info().pairs == 0 and opt.lm_info().type == 0                      # switching clears the store
    assert first == want and exact(opt) == want and approx != want
    lib = _lib.load()
    for memory in (0, 33):
        assert lib.asm_hessian_set_type(opt._h, 1, memory) == ERR_ARG
    assert lib.asm_hessian_set_type(opt._h, 2, 10) == ERR_ARG and exact(opt) == want
    opt.close()
    # before asm_eval_setup
    bare = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    lam2 = np.zeros(2)
    assert lib.asm_lm_begin(bare._h, _lib.dptr(lam2)) == ERR_STATE and lib.asm_lm_end(bare._h, _lib.dptr(lam2)) == ERR_STATE
    bare.eval_setup(fm)
    assert lib.asm_lm_begin(bare._h, _lib.dptr(lam2)) == ERR_STATE                   # ... and before the first asm_eval_functions
    bare.close()
    # a slot of a batch
    b = C.c_void_p()
    assert lib.asm_batch_create(0, 2, C.byref(b)) == 0
    assert lib.asm_hessian_set_type(lib.asm_batch_handle(b, 0), 1, 10) == ERR_ARG
    assert lib.asm_batch_destroy(b) == 0


# ------------------------------------------------------------------------------------------------ 5. SLP-EQP end to end
def test_slp_eqp_on_the_ohms_law_acopf(models):
    fm, pr = models("ohm14")
    kw = dict(device_eval=True, max_iter=60)
    par = A.Parameters(algorithm="SLP-EQP", hessian_type="limited-memory", **kw)
    tr_par = A.Parameters(algorithm="Trust Region", **kw)
    mdl = A.Model.from_problem(MODELS["ohm14"]().to_problem("ohm14"), par)
    slp = A.optimize(mdl)
    host_info = slp.optimizer.lm_info()
    slp.optimizer.close()
    mdl2 = A.Model.from_problem(MODELS["ohm14"]().to_problem("ohm14"), par)
    run = A.optimize(mdl2, native=True)
    c = run.eqp_counts
    print("ohm14: status %d iter %d lp %d %r radius %.6g, store: pairs %d pushed %d skipped %d + %d sigma %.6g" %
          (run.ret, run.iter, run.lp_solves, c, run.Delta_E, host_info.pairs, host_info.pushed, host_info.skipped_zero, host_info.skipped_curvature, host_info.sigma))
    assert (run.ret, run.iter, run.lp_solves) == (slp.ret, slp.iter, slp.lp_solves) and mdl2.status == mdl.status
    assert run.eqp_counts == slp.eqp_counts and run.Delta_E == slp.Delta_E and run.delta == slp.Delta
    assert np.array_equal(run.x, slp.x) and np.array_equal(run.lam, slp.lam)
    assert np.array_equal(run.mult_x_U, slp.mult_x_U) and np.array_equal(run.mult_x_L, slp.mult_x_L) and np.array_equal(run.E, slp.E)
    assert c["attempts"] > 0 and c["attempts"] == c["accepted"] + c["rejected"] + c["skipped_rows"] + c["skipped_dependent"] + c["skipped_zero"]
    assert host_info.pairs > 0 and host_info.type == 1
    # one handle: Trust Region, SLP-EQP in this mode, Trust Region again (asm_sublp_reset_warm between the runs, as every second run on a
    # handle needs it - tests/test_slp_eqp_gpu.py): the mode leaves the LP's state alone
    opt = _handle_for(pr, fm)

    def bits(r):
        return (r.ret, r.iter, r.lp_solves, r.restoration_solves, r.obj_val, r.delta) + tuple(getattr(r, k).tobytes() for k in ("x", "lam", "mult_x_U", "mult_x_L", "E"))

    before = opt.slp_run(pr.x0, tr_par)
    opt.reset_warm()
    opt.set_hessian_type("limited-memory", par.lm_memory)
    mid = opt.slp_run(pr.x0, par)
    info = opt.lm_info()
    opt.reset_warm()
    after = opt.slp_run(pr.x0, tr_par)
    opt.close()
    assert bits(before) == bits(after) and bits(mid) == bits(run) and mid.eqp_counts == run.eqp_counts
    assert (info.pairs, info.pushed, info.sigma) == (host_info.pairs, host_info.pushed, host_info.sigma)
