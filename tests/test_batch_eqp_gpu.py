"""SLP-EQP over a scenario batch (include/asm_hip.h: asm_batch_slp_run_eqp) against asm_slp_run_eqp on a fresh handle per scenario,
through the C ABI, bit for bit: load scenarios (bounds) and line-parameter scenarios (the scenario data table) of the 14-bus expression
ACOPF (n = 118, m = 189), with as many slots as scenarios and with slots that refill; enabled = 0 against asm_batch_slp_run_tr; a
Line-Search batch run before and after; argument and state errors."""
import ctypes as C

import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import _lib, acopf, batch

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
EQP, TR, LS = "SLP-EQP", "Trust Region", "Line Search"
S = 4


def _par(**kw):
    return A.Parameters(algorithm=kw.pop("algorithm", EQP), max_iter=60, device_eval=True, **kw)


def _base():
    return acopf.synthetic_grid(14, 5, 20, 1, 0.5)


def _load_problems():
    base = _base()
    return [acopf.function_model(acopf.scenario_case(base, s), nlp="expr").to_problem("grid14 load scenario %d" % s) for s in range(S)]


def _line_problems():
    base = _base()
    return [acopf.function_model(acopf.line_scenario_case(base, s), nlp="expr", branch_params=True).to_problem("grid14 line scenario %d" % s)
            for s in range(S)]


def _stack(prs):
    return tuple(np.stack([getattr(p, k) for p in prs]) for k in ("g_L", "g_U", "x_L", "x_U", "x0"))


def _fresh_handle_run(pr, par, J):
    """asm_slp_run_eqp (by par.algorithm) on a new handle set up from the scenario's own model, from the basis columns J."""
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(pr.function_model)
    Jc = np.ascontiguousarray(J, np.int32)
    assert _lib.load().asm_sublp_set_ns_basis(opt._h, _lib.i32ptr(Jc), len(Jc)) == 0
    run = opt.slp_run(pr.x0, par)
    opt.close()
    return run


def _same_run(r, one):
    assert (r.ret, r.iter, r.lp_solves, r.restoration_solves, r.paths) == (one.ret, one.iter, one.lp_solves, one.restoration_solves, one.paths)
    for k in ("x", "lam", "mult_x_U", "mult_x_L", "E"):
        assert np.array_equal(getattr(r, k), getattr(one, k)), k
    assert r.obj_val == one.obj_val
    assert (r.delta, r.accepted, r.rejected, r.shrunk, r.expanded) == (one.delta, one.accepted, one.rejected, one.shrunk, one.expanded)
    assert r.eqp_counts == one.eqp_counts and r.Delta_E == one.Delta_E


@pytest.fixture(scope="module")
def load_reference():
    """The four load scenarios once: (problems, the 4-slot batch's runs, its statistics, its basis columns, the per-handle runs)."""
    prs = _load_problems()
    hb = batch.HipBatch(prs[0], S, groups=2)
    assert hb.groups == 2
    runs4 = hb.slp_run(*_stack(prs), _par())
    bst, J = hb.stats(), hb.ns_basis()
    hb.close()
    ones = [_fresh_handle_run(pr, _par(), J) for pr in prs]
    return prs, runs4, bst, J, ones


def test_load_scenarios_equal_fresh_handles_bit_for_bit(load_reference):
    """scenario_case(base, 0..3) through four slots in two groups, through two slots that refill (the first batch's basis columns) and one
    by one on fresh handles: every field of every run equal.  The scenarios are in different phases most of the time: each makes trials,
    the batch sees accepted and rejected ones, the iteration counts differ, and launches are shared."""
    prs, runs4, bst, J, ones = load_reference
    hb2 = batch.HipBatch(prs[0], 2)
    hb2.set_ns_basis(J)
    runs2 = hb2.slp_run(*_stack(prs), _par())
    hb2.close()
    print("iter", [r.iter for r in ones], "ret", [r.ret for r in ones], "eqp", [r.eqp_counts for r in ones], "batch", {k: bst[k] for k in ("ops", "launches", "rounds")})
    assert len(J) > 0
    for s in range(S):
        _same_run(runs4[s], ones[s])
        _same_run(runs2[s], ones[s])
    assert sorted(r.slot for r in runs4) == list(range(S)) and {r.slot for r in runs2} == {0, 1}
    assert all(r.eqp_counts["attempts"] >= 1 for r in ones)
    assert sum(r.eqp_counts["accepted"] for r in ones) >= 1 and sum(r.eqp_counts["rejected"] for r in ones) >= 1
    assert len({r.iter for r in ones}) > 1
    assert bst["ops"] > bst["launches"], bst


def test_line_scenarios_with_a_data_table_equal_fresh_handles():
    """line_scenario_case(base, 0..3) with the branch data as parameters through solve_batch_lockstep (it fills the scenario data table)
    against fresh handles built from each scenario's own model: a slot whose Hessian or KKT Jacobian values came from the set-up data
    and not from its scenario's would differ."""
    prs = _line_problems()
    dpars = [np.asarray(p.function_model.nlp.device[2], np.float64) for p in prs]
    assert all(not np.array_equal(dpars[0], d) for d in dpars[1:])
    hb = batch.HipBatch(prs[0], S)
    runs, stats, bst = batch.solve_batch_lockstep(prs, _par(), S, batch=hb)
    J = hb.ns_basis()
    hb.close()
    assert stats["scenarios"] == S and stats["iterations"] == sum(r.iter for r in runs) and bst["ops"] > bst["launches"]
    for s, pr in enumerate(prs):
        one = _fresh_handle_run(pr, _par(), J)
        _same_run(runs[s], one)
        assert one.eqp_counts["attempts"] >= 1
    assert sum(r.eqp_counts["accepted"] for r in runs) >= 1


def test_disabled_equals_the_trust_region_batch():
    """enabled = 0 through asm_batch_slp_run_eqp against asm_batch_slp_run_tr on a fresh batch: the same bits, every count zero."""
    prs = _load_problems()
    out = []
    for par in (_par(eqp=False), _par(algorithm=TR)):
        hb = batch.HipBatch(prs[0], S)
        out.append(hb.slp_run(*_stack(prs), par))
        hb.close()
    for off, tr in zip(*out):
        assert off.eqp_counts is not None and not any(off.eqp_counts.values()) and off.Delta_E == _par().tr_size
        assert tr.eqp_counts is None
        off.eqp_counts, off.Delta_E = None, None
        _same_run(off, tr)


def test_a_line_search_run_returns_its_bits_after_an_eqp_run(load_reference):
    """Line Search, SLP-EQP, Line Search on one batch: the third run equals the first (LP inputs, bases and hints of the slots are as they
    were), and the SLP-EQP run between them equals the reference."""
    prs, _, _, _, ones = load_reference
    hb = batch.HipBatch(prs[0], S)
    first = hb.slp_run(*_stack(prs), _par(algorithm=LS))
    J = hb.ns_basis()
    mid = hb.slp_run(*_stack(prs), _par())
    third = hb.slp_run(*_stack(prs), _par(algorithm=LS))
    hb.close()
    for a, b in zip(first, third):
        _same_run(a, b)
        assert a.ls_trials == b.ls_trials
    # (the batch chose its columns in its Line-Search run: the same first LP of scenario 0, the same columns as the reference batch)
    assert np.array_equal(J, load_reference[3])
    for r, one in zip(mid, ones):
        _same_run(r, one)


def _raw_call(lib, b, prs, sp, tr_size, ep, n_scen=S):
    gl, gu, xl, xu, x0 = (np.ascontiguousarray(a, np.float64) for a in _stack(prs))
    n, m = prs[0].n, prs[0].m
    X, L, U, W, G = np.empty((n_scen, n)), np.empty((n_scen, m)), np.empty((n_scen, n)), np.empty((n_scen, n)), np.empty((n_scen, m))
    R = (_lib.SlpResult * n_scen)()
    D = _lib.dptr
    return lib.asm_batch_slp_run_eqp(b, n_scen, D(gl), D(gu), D(xl), D(xu), D(x0), C.byref(sp), tr_size, C.byref(ep) if ep is not None else None,
                                     D(X), D(L), D(U), D(W), D(G), R, None, None)


@pytest.mark.parametrize("what", ["radius0", "radius_max", "tol_active", "null and tr_size"])
def test_argument_errors_leave_the_batch_usable(load_reference, what):
    """radius0 of 0, negative or NaN, radius_max 0, tol_active -1, a null parameter record and tr_size 0: ASM_ERR_ARG; the batch then runs
    and gives the reference's bits."""
    prs, _, _, J, ones = load_reference
    lib = _lib.load()
    sp = batch.slp_params(_par())
    bad = {"radius0": [(0.0, 1e3, 1e-8), (-1.0, 1e3, 1e-8), (float("nan"), 1e3, 1e-8)], "radius_max": [(0.4, 0.0, 1e-8)], "tol_active": [(0.4, 1e3, -1.0)],
           "null and tr_size": []}[what]
    hb = batch.HipBatch(prs[0], S)
    hb.set_ns_basis(J)
    for ep in bad:
        assert _raw_call(lib, hb._b, prs, sp, 0.4, _lib.SlpEqpParams(*ep, 1)) == ERR_ARG, ep
    if what == "null and tr_size":
        assert _raw_call(lib, hb._b, prs, sp, 0.4, None) == ERR_ARG
        assert _raw_call(lib, hb._b, prs, sp, 0.0, _lib.SlpEqpParams(0.4, 1e3, 1e-8, 1)) == ERR_ARG
        assert _raw_call(lib, None, prs, sp, 0.4, _lib.SlpEqpParams(0.4, 1e3, 1e-8, 1)) == ERR_ARG
    runs = hb.slp_run(*_stack(prs), _par())
    hb.close()
    for r, one in zip(runs, ones):
        _same_run(r, one)


def test_state_and_model_errors_are_the_per_handle_entry_s(load_reference):
    """Before the two set-ups: ASM_ERR_STATE.  The Ohm's-law kernel block has no second derivatives: the code asm_slp_run_eqp returns on a
    handle, before any fiber starts (the batch has recorded nothing).  The same batch, set up with the expression model, then gives the
    reference's bits."""
    prs, _, _, J, ones = load_reference
    lib = _lib.load()
    sp, ok = batch.slp_params(_par()), _lib.SlpEqpParams(0.4, 1e3, 1e-8, 1)
    raw = C.c_void_p()
    assert lib.asm_batch_create(0, 2, C.byref(raw)) == 0
    assert _raw_call(lib, raw, prs, sp, 0.4, ok) == ERR_STATE
    assert lib.asm_batch_destroy(raw) == 0
    base = _base()
    ohms = [acopf.function_model(acopf.scenario_case(base, s)).to_problem("grid14 ohm %d" % s) for s in range(S)]
    opt = A.HipSubOptimizer(A.QpData(np.zeros(ohms[0].n), 0.0, np.zeros(ohms[0].nnz), np.zeros(ohms[0].m), ohms[0].g_L, ohms[0].g_U, ohms[0].x_L, ohms[0].x_U),
                            ohms[0].j_row, ohms[0].j_col)
    opt.eval_setup(ohms[0].function_model)
    x0 = np.ascontiguousarray(ohms[0].x0, np.float64)
    res = _lib.SlpResult()
    want = lib.asm_slp_run_eqp(opt._h, C.byref(sp), 0.4, C.byref(ok), _lib.dptr(x0), None, None, None, None, None, C.byref(res), None, None)
    opt.close()
    hb = batch.HipBatch(ohms[0], S)
    ops0 = hb.stats()["ops"]
    assert _raw_call(lib, hb._b, ohms, sp, 0.4, ok) == want == ERR_ARG
    assert hb.stats()["ops"] == ops0
    with pytest.raises(A.AsmHipError):
        hb.slp_run(*_stack(ohms), _par())
    assert all(r.lp_solves >= 1 for r in hb.slp_run(*_stack(ohms), A.Parameters(algorithm=TR, max_iter=3, device_eval=True)))
    hb.setup(prs[0])
    hb.set_ns_basis(J)
    runs = hb.slp_run(*_stack(prs), _par())
    hb.close()
    for r, one in zip(runs, ones):
        _same_run(r, one)
