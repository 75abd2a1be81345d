"""KKT solves and solution sensitivities of a scenario batch through the C ABI (include/asm_hip.h, "Scenario batches: KKT solves and
sensitivities": asm_batch_kkt_solve, asm_batch_solution_sensitivity, asm_batch_bound_sensitivity, and per handle
asm_bound_sensitivity_multi): the bound right-hand sides made on the device against asm_kkt_solve_multi on their NumPy statement, and
every scenario of every batch entry against the per-handle entry on a fresh handle - byte for byte, whatever the slots, groups and
refills - on the function store, the hs071 family with a data table and the 14-bus line scenarios in both KKT forms; a Line-Search
batch run before and after; argument, state and model errors."""
import ctypes as C

import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import _lib, acopf, batch, sensitivity
from tests.test_batch_eqp_gpu import _line_problems, _par, _same_run, _stack
from tests.test_batch_sens_cpu import hs071_scenario_models
from tests.test_nlparams_gpu import _handle_for
from tests.test_sensitivity_cpu import kkt_instance, rel_err
from tests.test_sensitivity_gpu import _twin_cross
from tests.test_sensitivity_multi_gpu import BAR, CHUNK

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
D, I = _lib.dptr, _lib.i32ptr
S = 4


def _col_bits(out, c):
    DX, DLAM, DZ, infos = out
    return DX[c].tobytes(), DLAM[c].tobytes(), DZ[c].tobytes(), infos[c].status, infos[c].cg_iters


def _same_columns(got, want, what):
    """(DX, DLAM, DZ, infos) of one scenario twice: bytes, status and iteration count of every column."""
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape and len(got[3]) == len(want[3]), what
    for c in range(len(want[3])):
        assert _col_bits(got, c) == _col_bits(want, c), (what, c)


def _scenario(out, s):
    return out[0][s], out[1][s], out[2][s], out[3][s]


# ------------------------------------------------------------------------------------------------ 1. the new kernel, per handle
@pytest.mark.parametrize("shape", ((8, 3, 5), (33, 1, 1), (96, 10, 65)), ids=lambda s: "n%d_B%d_W%d" % s)
def test_bound_columns_equal_the_multi_solve_on_their_right_hand_sides(shape):
    """asm_bound_sensitivity_multi against asm_kkt_solve_multi on bound_rhs(...): working rows (65 of them: one past the 64-row tile), a
    row outside the working set and a duplicate; 1, 3 and one more column than a chunk holds; delta given and NULL."""
    n, nB, nW = shape
    fm, x, lam, rs, bs = kkt_instance(*shape)[:5]
    opt = _handle_for(fm.to_problem(), fm)
    work, outside = np.nonzero(rs == 1)[0], int(np.nonzero(rs == 0)[0][0])
    pattern = [int(work[0]), outside, int(work[0])] + [int(work[(3 * k + 1) % nW]) for k in range(CHUNK + 1 - 3)]       # (column 2 repeats column 0)
    deltas = 0.25 + np.random.default_rng(5).uniform(-2.0, 2.0, CHUNK + 1)
    for nrhs in (1, 3, CHUNK + 1):
        rows = pattern[:nrhs]
        for delta in (deltas[:nrhs], None):
            got = opt.bound_sensitivity_multi(x, lam, rs, bs, rows, delta)
            want = opt.kkt_solve_multi(x, lam, rs, bs, *sensitivity.bound_rhs(fm.m, n, rows, delta))
            _same_columns(got, want, (shape, nrhs, delta is None))
            assert all(i.status == 0 for i in got[3]) and np.any(got[0][0] != 0.0)
            if nrhs > 1:                                          # the row outside the working set: the zero column, no iteration
                assert not got[0][1].any() and not got[1][1].any() and not got[2][1].any() and got[3][1].cg_iters == 0 and got[3][1].status == 0
            if nrhs > 2 and delta is None:                        # the duplicate repeats its column
                assert _col_bits(got, 2) == _col_bits(got, 0)
    lib, info = opt._lib, (_lib.KktInfo * 2)()
    X, L, Z = np.empty((2, n)), np.empty((2, fm.m)), np.empty((2, n))
    rs32, bs32 = np.ascontiguousarray(rs, np.int32), np.ascontiguousarray(bs, np.int32)
    for bad in ([0, fm.m], [-1, 0]):                              # a row index outside [0, m)
        assert lib.asm_bound_sensitivity_multi(opt._h, D(x), D(lam), I(rs32), I(bs32), 2, I(np.array(bad, np.int32)), None, None, D(X), D(L), D(Z), info) == ERR_ARG
    assert lib.asm_bound_sensitivity_multi(opt._h, D(x), D(lam), I(rs32), I(bs32), 2, None, None, None, D(X), D(L), D(Z), info) == ERR_ARG
    assert lib.asm_bound_sensitivity_multi(opt._h, D(x), D(lam), I(rs32), I(bs32), 0, I(np.zeros(2, np.int32)), None, None, D(X), D(L), D(Z), info) == ERR_ARG
    again = opt.bound_sensitivity_multi(x, lam, rs, bs, pattern[:3])
    _same_columns(again, opt.kkt_solve_multi(x, lam, rs, bs, *sensitivity.bound_rhs(fm.m, n, pattern[:3])), "after the refusals")
    opt.close()


# ------------------------------------------------------------------------------------------------ 2. the batch KKT solve on the function store
@pytest.fixture(scope="module")
def store_case():
    """One (96, 10, 65) model and three scenarios - seeded perturbations of (x, lam); the instance's working set, one working row dropped,
    one bound freed - with CHUNK + 1 right-hand sides each, the fresh-handle answers and the dense reference, once for the module."""
    fm, x, lam, rs, bs = kkt_instance(96, 10, 65)[:5]
    rng = np.random.default_rng(17)
    X = np.stack([x + 0.05 * rng.standard_normal(fm.n) * (s > 0) for s in range(3)])
    L = np.stack([lam + 0.05 * rng.standard_normal(fm.m) * (s > 0) for s in range(3)])
    RS, BS = np.stack([rs] * 3).astype(np.int32), np.stack([bs] * 3).astype(np.int32)
    RS[1, np.nonzero(rs == 1)[0][7]] = 0
    BS[2, np.nonzero(bs != 0)[0][3]] = 0
    RU, RW = rng.standard_normal((3, CHUNK + 1, fm.n)), rng.standard_normal((3, CHUNK + 1, fm.m))
    pr = fm.to_problem("constructed QP")
    fresh, ref = [], []
    for s in range(3):
        opt = _handle_for(pr, fm)
        fresh.append({k: opt.kkt_solve_multi(X[s], L[s], RS[s], BS[s], RU[s, :k], RW[s, :k]) for k in (3, CHUNK + 1)})
        opt.close()
        ref.append(sensitivity.kkt_reference_multi(fm, X[s], L[s], RS[s], BS[s], RU[s], RW[s]))
    return fm, pr, X, L, RS, BS, RU, RW, fresh, ref


@pytest.mark.parametrize("slots,groups", ((3, 2), (2, None)), ids=("3 slots in 2 groups", "2 slots, one refill"))
def test_batch_kkt_solve_equals_fresh_handles(store_case, slots, groups):
    fm, pr, X, L, RS, BS, RU, RW, fresh, ref = store_case
    hb = batch.HipBatch(pr, slots, groups=groups)
    assert groups is None or hb.groups == groups
    for k in (3, CHUNK + 1):
        out = hb.kkt_solve_multi(X, L, RS, BS, RU[:, :k], RW[:, :k])
        assert out[0].shape == (3, k, fm.n) and out[1].shape == (3, k, fm.m) and out[2].shape == (3, k, fm.n)
        worst = 0.0
        for s in range(3):
            got = _scenario(out, s)
            _same_columns(got, fresh[s][k], (slots, k, s))
            assert all(i.status == 0 for i in got[3]), (slots, k, s)
            assert got[3][0].n_rows == RS[s].sum() and got[3][0].n_free == (BS[s] == 0).sum()
            for c in range(k):
                errs = [rel_err(g[c], r[c]) for g, r in zip(got[:3], ref[s])]
                worst = max(worst, *errs)
                assert max(errs) <= BAR, (slots, k, s, c, errs)
        print("%d slots, %d columns: largest rel err against the dense solve %.3e (bar %.3e)" % (slots, k, worst, BAR))
    st = hb.stats()
    assert st["ops"] > st["launches"], st
    hb.close()


# ------------------------------------------------------------------------------------------------ 3. the hs071 family with a data table
def test_hs071_scenarios_with_a_data_table():
    """(p0, p1) = (25 + s, 40 + 0.5 s): the points from the batch's own SLP-EQP runs, the working sets from batch.working_sets, the two
    unit data directions shared and per scenario, through 4 slots and 2: byte-equal to fresh handles whose data asm_eval_set_data set,
    and to the bar of the per-handle hs071 test against the dense solve fed with the host twin's cross derivatives."""
    fms = hs071_scenario_models(S)
    prs = [fm.to_problem("hs071 scenario %d" % s) for s, fm in enumerate(fms)]
    hb = batch.HipBatch(prs[0], S)
    data = hb.scenario_data(prs)
    assert data is not None and data.shape == (S, 2)
    runs = hb.slp_run(*_stack(prs), _par(), data=data)
    rs, bs = batch.working_sets(prs, runs)
    print("hs071 scenarios: ret %r, iterations %r, row_state %r, bound_state %r" % ([r.ret for r in runs], [r.iter for r in runs], rs.tolist(), bs.tolist()))
    assert rs.tolist() == [[1, 1]] * S and bs.tolist() == [[-1, 0, 0, 0]] * S          # (the condition of tests/test_batch_sens_cpu.py)
    X, L = np.stack([r.x for r in runs]), np.stack([r.lam for r in runs])
    DC = np.eye(2)
    fresh = []
    for s in range(S):
        opt = _handle_for(prs[0], fms[0])
        opt.set_eval_data(data[s])
        fresh.append(opt.solution_sensitivity_multi(X[s], L[s], rs[s], bs[s], DC))
        opt.close()
    shared4 = hb.solution_sensitivity_multi(X, L, rs, bs, DC)
    per4 = hb.solution_sensitivity_multi(X, L, rs, bs, np.stack([DC] * S))
    Jx, Jl, status = batch.solution_jacobians(hb, prs, runs)
    hb.close()
    hb2 = batch.HipBatch(prs[0], 2)
    hb2.set_scenario_data(data)
    shared2 = hb2.solution_sensitivity_multi(X, L, rs, bs, DC)
    per2 = hb2.solution_sensitivity_multi(X, L, rs, bs, np.stack([DC] * S))
    hb2.close()
    assert Jx.shape == (S, 4, 2) and Jl.shape == (S, 2, 2) and status.shape == (S, 2) and not status.any()
    worst = 0.0
    for s in range(S):
        for name, out in (("4 slots, shared", shared4), ("4 slots, per scenario", per4), ("2 slots, shared", shared2), ("2 slots, per scenario", per2)):
            _same_columns(_scenario(out, s), fresh[s], (name, s))
        DX, DLAM, DZ, infos = _scenario(shared4, s)
        assert np.array_equal(Jx[s], DX.T) and np.array_equal(Jl[s], DLAM.T)
        RU, RW = np.zeros((2, 4)), np.zeros((2, 2))
        for c in range(2):
            RU[c], RW[c] = _twin_cross(fms[s], X[s], L[s], DC[c])
        ref = sensitivity.kkt_reference_multi(fms[s], X[s], L[s], rs[s], bs[s], RU, RW)
        for c in range(2):
            assert infos[c].status == 0 and infos[c].cg_iters >= 1 and infos[c].n_free == 3 and infos[c].n_rows == 2, (s, c, infos[c].status, infos[c].cg_iters)
            errs = [rel_err(g[c], r[c]) for g, r in zip((DX, DLAM, DZ), ref)]
            worst = max(worst, *errs)
            assert max(errs) <= BAR and np.any(DX[c] != 0.0), (s, c, errs)
    assert any(not np.array_equal(fresh[0][0], fresh[s][0]) for s in range(1, S))        # the scenarios' data reached their slots
    print("hs071 scenarios: largest rel err against the dense solve with the twin's cross derivatives %.3e (bar %.3e)" % (worst, BAR))


# ------------------------------------------------------------------------------------------------ 4. the 14-bus line scenarios
def _p_balance_rows(pr, count=3):
    """The first `count` nodal P-balance rows of an ACOPF function model: equalities of the function store over p flows and no q variable."""
    fm = pr.function_model
    mdl = fm.acopf_model
    J = sensitivity.dense_jacobian(fm, pr.x0)
    p_cols, q_cols = set(map(int, list(mdl.pf) + list(mdl.pt))), set(map(int, list(mdl.qf) + list(mdl.qt) + list(mdl.qg)))
    rows = []
    for i in range(fm.nlp_constraint_offset):
        nz = set(np.nonzero(J[i])[0].tolist())
        if pr.g_L[i] == pr.g_U[i] and nz & p_cols and not nz & q_cols:
            rows.append(i)
    assert len(rows) == mdl.nb
    return rows[:count]


def _fresh_answers(prs, form, X, L, rs, bs, DC, rows):
    out = []
    for s, pr in enumerate(prs):
        opt = _handle_for(pr)
        if form == "sparse":
            opt.set_kkt_form("sparse")
            opt.set_kkt_order("static")
        sens = opt.solution_sensitivity_multi(X[s], L[s], rs[s], bs[s], DC)
        assert opt.kkt_form_info().form_used == (1 if form == "sparse" else 0)
        out.append((sens, opt.bound_sensitivity_multi(X[s], L[s], rs[s], bs[s], rows)))
        opt.close()
    return out


def _line_sensitivities(prs, n_slots, forms):
    """The scenarios `prs` through solve_batch_lockstep (SLP-EQP; it fills the data table), then five seeded data directions and the bound
    sensitivities of the first three nodal P-balance rows in every form of `forms`, each against fresh handles in that form."""
    nd = len(prs[0].function_model.nlp.device[2])
    hb = batch.HipBatch(prs[0], n_slots)
    runs, _, _ = batch.solve_batch_lockstep(prs, _par(), n_slots, batch=hb)
    rs, bs = batch.working_sets(prs, runs)
    X, L = np.stack([r.x for r in runs]), np.stack([r.lam for r in runs])
    DC = np.random.default_rng(23).standard_normal((5, nd))
    rows = _p_balance_rows(prs[0])
    assert all(rs[s, rows].all() and pr.g_L[rows[0]] == pr.g_U[rows[0]] for s, pr in enumerate(prs))
    seen = set()
    for form in forms:
        hb.set_kkt_form(form, "static" if form == "sparse" else "working-set")
        before = hb.stats()
        sens = hb.solution_sensitivity_multi(X, L, rs, bs, DC)
        bnd = hb.bound_sensitivity(X, L, rs, bs, rows)
        after = hb.stats()
        assert after["ops"] - before["ops"] > after["launches"] - before["launches"] > 0, (form, before, after)
        fresh = _fresh_answers(prs, form, X, L, rs, bs, DC, rows)
        live = 0
        for s in range(len(prs)):
            _same_columns(_scenario(sens, s), fresh[s][0], (form, "data directions", s))
            _same_columns(_scenario(bnd, s), fresh[s][1], (form, "bound rows", s))
            for i in sens[3][s] + bnd[3][s]:
                seen.add(i.status)
                live += i.status == 0 and i.cg_iters >= 1
        print("%s form, %d scenarios: statuses %r, CG iterations %r, ops %d in %d launches" % (form, len(prs), sorted({i.status for row in sens[3] + bnd[3] for i in row}),
              sorted({i.cg_iters for row in sens[3] + bnd[3] for i in row}), after["ops"] - before["ops"], after["launches"] - before["launches"]))
        assert live >= 1, form                                    # the comparison is not of zeros
        Bx, Bl, status = batch.bound_jacobians(hb, prs, runs, rows)
        assert Bx.shape == (len(prs), prs[0].n, 3) and Bl.shape == (len(prs), prs[0].m, 3) and status.shape == (len(prs), 3)
        assert np.array_equal(Bx, np.transpose(bnd[0], (0, 2, 1))) and np.array_equal(Bl, np.transpose(bnd[1], (0, 2, 1)))
    print("statuses over all forms: %r" % sorted(seen))
    hb.close()


def test_line_scenarios_in_both_forms_equal_fresh_handles():
    prs = _line_problems()
    assert prs[0].n == 118 and prs[0].m == 189 and len(prs) == S
    _line_sensitivities(prs, S, ("dense", "sparse"))


def test_line_scenarios_on_the_ohm_kernel_with_derivatives():
    base = acopf.synthetic_grid(14, 5, 20, 1, 0.5)
    prs = [acopf.function_model(acopf.line_scenario_case(base, s), hessian=True).to_problem("grid14 ohm line scenario %d" % s) for s in range(2)]
    assert prs[0].function_model.nlp.device[0] == "acopf_ohm_hess"
    _line_sensitivities(prs, 2, ("dense",))


# ------------------------------------------------------------------------------------------------ 5. no interference
def test_a_line_search_run_returns_its_bits_after_the_sensitivity_calls():
    prs = _line_problems()
    hb = batch.HipBatch(prs[0], S)
    data = hb.scenario_data(prs)
    ls = _par(algorithm="Line Search")
    first = hb.slp_run(*_stack(prs), ls, data=data)
    X, L = np.stack([r.x for r in first]), np.stack([r.lam for r in first])
    # (the equality rows and no bound: a valid working set at any point - the calls are what matters here)
    rs, bs = np.stack([(p.g_L == p.g_U).astype(np.int32) for p in prs]), np.zeros((S, hb.n), np.int32)
    assert rs[0].sum() <= hb.n
    rng = np.random.default_rng(29)
    hb.solution_sensitivity_multi(X, L, rs, bs, rng.standard_normal((3, hb.n_dpar)))
    hb.bound_sensitivity(X, L, rs, bs, _p_balance_rows(prs[0]))
    hb.kkt_solve_multi(X, L, rs, bs, rng.standard_normal((S, 2, hb.n)), rng.standard_normal((S, 2, hb.m)))
    third = hb.slp_run(*_stack(prs), ls, data=data)
    hb.close()
    for a, b in zip(first, third):
        _same_run(a, b)
        assert a.ls_trials == b.ls_trials


# ------------------------------------------------------------------------------------------------ 6. errors
def test_state_argument_and_model_errors_leave_the_batch_usable():
    lib = _lib.load()
    fms = hs071_scenario_models(2)
    prs = [fm.to_problem("hs071 scenario %d" % s) for s, fm in enumerate(fms)]
    n, m, K, NS = 4, 2, 2, 2
    rng = np.random.default_rng(31)
    x, lam = np.stack([p.x0 + 0.1 for p in prs]), rng.standard_normal((NS, m))
    rs, bs = np.ones((NS, m), np.int32), np.ascontiguousarray(np.stack([[-1, 0, 0, 0]] * NS), np.int32)
    RU, RW, DC = rng.standard_normal((NS, K, n)), rng.standard_normal((NS, K, m)), np.eye(2)
    rows, delta = np.array([1, 0], np.int32), np.array([0.5, 2.0])
    DX, DLAM, DZ, info = np.zeros((NS, K, n)), np.zeros((NS, K, m)), np.zeros((NS, K, n)), (_lib.KktInfo * (NS * K))()
    head, tail = [NS, D(x), D(lam), I(rs), I(bs), K], [None, D(DX), D(DLAM), D(DZ), info]
    entries = {"kkt": (lib.asm_batch_kkt_solve, head + [D(RU), D(RW)] + tail), "sens": (lib.asm_batch_solution_sensitivity, head + [D(DC), 0] + tail),
               "bound": (lib.asm_batch_bound_sensitivity, head + [I(rows), D(delta)] + tail)}
    required = {"kkt": (1, 2, 3, 4, 6, 7, 9, 10, 12), "sens": (1, 2, 3, 4, 6, 9, 10, 12), "bound": (1, 2, 3, 4, 6, 9, 10, 12)}    # (par, delta and DZ may be NULL)
    call = lambda b, k, a=None: entries[k][0](b, *(entries[k][1] if a is None else a))
    raw = C.c_void_p()
    assert lib.asm_batch_create(0, 2, C.byref(raw)) == 0
    assert [call(raw, k) for k in entries] == [ERR_STATE] * 3                               # before asm_batch_setup
    assert lib.asm_batch_destroy(raw) == 0
    assert [call(None, k) for k in entries] == [ERR_ARG] * 3

    hb = batch.HipBatch(prs[0], 2)
    hb.set_scenario_data(hb.scenario_data(prs))
    right = {}
    for k in entries:
        assert call(hb._b, k) == 0, (k, lib.asm_batch_last_error(hb._b))
        right[k] = (DX.copy(), DLAM.copy(), DZ.copy(), [(i.status, i.cg_iters) for i in info])
        assert np.any(DX != 0.0)

    def still_right(k):
        for a in (DX, DLAM, DZ):
            a[:] = 0.0
        assert call(hb._b, k) == 0
        assert np.array_equal(DX, right[k][0]) and np.array_equal(DLAM, right[k][1]) and np.array_equal(DZ, right[k][2])
        assert [(i.status, i.cg_iters) for i in info] == right[k][3]
    for k in entries:
        for pos, bad in ((0, 0), (0, -1), (5, 0), (5, -2)):                                  # n_scen < 1, nrhs < 1
            a = list(entries[k][1])
            a[pos] = bad
            assert call(hb._b, k, a) == ERR_ARG, (k, pos, bad)
        for pos in required[k]:
            a = list(entries[k][1])
            a[pos] = None
            assert call(hb._b, k, a) == ERR_ARG, (k, pos)
        a = list(entries[k][1])
        a[0] = 3                                                                            # beyond the scenario table: check_scen's code
        grad = np.zeros((3, 2))
        want = lib.asm_batch_data_gradient(hb._b, 3, D(np.zeros((3, n))), D(np.zeros((3, m))), D(grad))
        assert call(hb._b, k, a) == want == ERR_ARG, k
        still_right(k)
    for bad in ([0, m], [-1, 1]):                                                           # a row index outside [0, m)
        a = list(entries["bound"][1])
        a[6] = I(np.array(bad, np.int32))
        assert call(hb._b, "bound", a) == ERR_ARG, bad
    a = list(entries["sens"][1])
    a[7] = 2                                                                                # dc_per_scenario outside {0, 1}
    assert call(hb._b, "sens", a) == ERR_ARG
    brs = np.ascontiguousarray(np.stack([[1, 1], [2, 1]]), np.int32)                        # a scenario's own refusal: the per-handle code
    a = list(entries["kkt"][1])
    a[3] = I(brs)
    assert call(hb._b, "kkt", a) == ERR_ARG
    for k in entries:
        still_right(k)

    # a model without second derivatives: the code of asm_batch_hessian_lagrangian, before any fiber starts
    base = acopf.synthetic_grid(14, 5, 20, 1, 0.5)
    ohm = acopf.function_model(base).to_problem("grid14 ohm")
    hb.setup(ohm)
    on, om = ohm.n, ohm.m
    ox, ol = np.stack([ohm.x0] * NS), np.zeros((NS, om))
    ors, obs = np.zeros((NS, om), np.int32), np.zeros((NS, on), np.int32)
    OX, OL, OZ = np.zeros((NS, K, on)), np.zeros((NS, K, om)), np.zeros((NS, K, on))
    want = lib.asm_batch_hessian_lagrangian(hb._b, NS, D(ox), None, D(ol), D(np.zeros((NS, 8))))
    ohead, otail = [NS, D(ox), D(ol), I(ors), I(obs), K], [None, D(OX), D(OL), D(OZ), info]
    ops0 = hb.stats()["ops"]
    assert want == ERR_ARG
    assert lib.asm_batch_kkt_solve(hb._b, *(ohead + [D(np.zeros((NS, K, on))), D(np.zeros((NS, K, om)))] + otail)) == want
    assert lib.asm_batch_solution_sensitivity(hb._b, *(ohead + [D(np.zeros((K, len(ohm.function_model.nlp.device[2])))), 0] + otail)) == want
    assert lib.asm_batch_bound_sensitivity(hb._b, *(ohead + [I(rows), None] + otail)) == want
    assert hb.stats()["ops"] == ops0
    hb.setup(prs[0])
    hb.set_scenario_data(hb.scenario_data(prs))
    for k in entries:
        still_right(k)
    hb.close()
