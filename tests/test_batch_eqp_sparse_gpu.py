"""SLP-EQP over a scenario batch in the sparse form of the KKT solve on the static row order (include/asm_hip.h: asm_batch_kkt_set_form)
against asm_slp_run_eqp on a fresh handle per scenario in the same form and order, through the C ABI, bit for bit: the load and
line-parameter scenarios of tests/test_batch_eqp_gpu.py (the 14-bus expression ACOPF, n = 118, m = 189), what the slots hold, switching
the form on one batch, the refusals, the dense fallback, and two case118-sized scenarios beyond 640 working rows."""
import ctypes as C

import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import _lib, acopf, batch, problems
from tests.test_batch_eqp_gpu import S, _line_problems, _load_problems, _same_run, _stack

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
EQP, LS = "SLP-EQP", "Line Search"
# the case118-sized test: the smallest max_iter at which each of its two scenarios makes at least one trial, found on an MI355X - at 12
# the scenarios make 0 and 1 trials, at 13 they make 1 and 2
BIG_MAX_ITER = 13


def _par(form="sparse", order="static", **kw):
    return A.Parameters(algorithm=kw.pop("algorithm", EQP), max_iter=kw.pop("max_iter", 60), device_eval=True, kkt_form=form, kkt_order=order, **kw)


def _fresh_handle_run(pr, par, J):
    """asm_slp_run_eqp on a new handle set up from the scenario's own model, in par's form and order, from the basis columns J."""
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(pr.function_model)
    opt.set_kkt_form(par.kkt_form)
    opt.set_kkt_order(par.kkt_order)
    Jc = np.ascontiguousarray(J, np.int32)
    assert _lib.load().asm_sublp_set_ns_basis(opt._h, _lib.i32ptr(Jc), len(Jc)) == 0
    run = opt.slp_run(pr.x0, par)
    fi, oi = opt.kkt_form_info(), opt.kkt_order_info()
    opt.close()
    return run, fi, oi


def _slot_infos(hb):
    lib, out = _lib.load(), []
    for s in range(hb.n_slots):
        fi, oi = _lib.KktFormInfo(), _lib.KktOrderInfo()
        h = lib.asm_batch_handle(hb._b, s)
        assert lib.asm_kkt_form_info(h, C.byref(fi)) == 0 and lib.asm_kkt_order_info(h, C.byref(oi)) == 0
        out.append((fi, oi))
    return out


def _all_sparse_static(hb):
    for fi, oi in _slot_infos(hb):
        assert (fi.form_requested, fi.form_used, oi.order_requested, oi.order_used) == (1, 1, 1, 1)
        assert fi.dense_bytes == 0 and fi.sparse_bytes > 0 and oi.all_pairs > 0


@pytest.fixture(scope="module")
def load_reference():
    """The four load scenarios once, sparse form and static order: (problems, the 4-slot batch's runs, its statistics, its basis columns,
    the per-handle runs)."""
    prs = _load_problems()
    hb = batch.HipBatch(prs[0], S, groups=2)
    assert hb.groups == 2
    runs4 = hb.slp_run(*_stack(prs), _par())
    _all_sparse_static(hb)
    bst, J = hb.stats(), hb.ns_basis()
    hb.close()
    ones = []
    for pr in prs:
        run, fi, oi = _fresh_handle_run(pr, _par(), J)
        assert (fi.form_used, oi.order_used) == (1, 1) and fi.dense_bytes == 0
        ones.append(run)
    return prs, runs4, bst, J, ones


def test_load_scenarios_equal_fresh_handles_bit_for_bit(load_reference):
    prs, runs4, bst, J, ones = load_reference
    hb2 = batch.HipBatch(prs[0], 2)
    hb2.set_ns_basis(J)
    runs2 = hb2.slp_run(*_stack(prs), _par())
    _all_sparse_static(hb2)
    bst2 = hb2.stats()
    hb2.close()
    print("iter", [r.iter for r in ones], "ret", [r.ret for r in ones], "eqp", [r.eqp_counts for r in ones], "batch", {k: bst[k] for k in ("ops", "launches", "rounds")})
    assert len(J) > 0
    for s in range(S):
        _same_run(runs4[s], ones[s])
        _same_run(runs2[s], ones[s])
    assert sorted(r.slot for r in runs4) == list(range(S)) and {r.slot for r in runs2} == {0, 1}
    assert all(r.eqp_counts["attempts"] >= 1 for r in ones)
    assert sum(r.eqp_counts["accepted"] for r in ones) >= 1 and sum(r.eqp_counts["rejected"] for r in ones) >= 1
    assert bst["ops"] > bst["launches"] and bst2["ops"] > bst2["launches"], (bst, bst2)


def test_line_scenarios_with_a_data_table_equal_fresh_handles():
    """A slot whose CSR values of the KKT Jacobian came from the set-up data and not from its scenario's would differ."""
    prs = _line_problems()
    dpars = [np.asarray(p.function_model.nlp.device[2], np.float64) for p in prs]
    assert all(not np.array_equal(dpars[0], d) for d in dpars[1:])
    hb = batch.HipBatch(prs[0], S)
    runs, stats, bst = batch.solve_batch_lockstep(prs, _par(), S, batch=hb)
    _all_sparse_static(hb)
    J = hb.ns_basis()
    hb.close()
    assert stats["scenarios"] == S and bst["ops"] > bst["launches"]
    for s, pr in enumerate(prs):
        one, fi, oi = _fresh_handle_run(pr, _par(), J)
        _same_run(runs[s], one)
        assert one.eqp_counts["attempts"] >= 1 and (fi.form_used, oi.order_used) == (1, 1)
    assert sum(r.eqp_counts["accepted"] for r in runs) >= 1


def test_switching_the_form_on_one_batch(load_reference):
    """dense, sparse-static, dense on one batch: the first and the third equal bit for bit, the second equals the reference; a Line-Search
    run afterwards returns the bits of one made before."""
    prs, _, _, J, ones = load_reference
    hb = batch.HipBatch(prs[0], S)
    ls0 = hb.slp_run(*_stack(prs), _par(algorithm=LS))
    assert np.array_equal(hb.ns_basis(), J)
    first = hb.slp_run(*_stack(prs), _par("dense", "working-set"))
    assert all(fi.form_used == 0 and fi.sparse_bytes == 0 and fi.dense_bytes > 0 for fi, _ in _slot_infos(hb))
    mid = hb.slp_run(*_stack(prs), _par())
    assert all((fi.form_used, oi.order_used) == (1, 1) and fi.sparse_bytes > 0 for fi, oi in _slot_infos(hb))
    third = hb.slp_run(*_stack(prs), _par("dense", "static"))
    assert all(fi.form_used == 0 and oi.order_used == 0 for fi, oi in _slot_infos(hb))
    ls1 = hb.slp_run(*_stack(prs), _par(algorithm=LS))
    hb.close()
    for a, b in zip(first, third):
        _same_run(a, b)
    for r, one in zip(mid, ones):
        _same_run(r, one)
    for a, b in zip(ls0, ls1):
        _same_run(a, b)
        assert a.ls_trials == b.ls_trials


def test_refusals_leave_the_batch_usable(load_reference):
    prs, _, _, J, ones = load_reference
    lib = _lib.load()
    raw = C.c_void_p()
    assert lib.asm_batch_create(0, 2, C.byref(raw)) == 0
    assert lib.asm_batch_kkt_set_form(raw, 1, 1) == ERR_STATE
    assert lib.asm_batch_destroy(raw) == 0
    assert lib.asm_batch_kkt_set_form(None, 1, 1) == ERR_ARG
    hb = batch.HipBatch(prs[0], S)
    hb.set_ns_basis(J)
    assert lib.asm_batch_kkt_set_form(hb._b, 1, 0) == ERR_ARG
    msg = lib.asm_batch_last_error(hb._b).decode()
    assert "per handle" in msg and "ASM_KKT_ORDER_STATIC" in msg, msg
    for form, order in ((2, 1), (-1, 0), (1, 2), (0, -1), (0, 7)):
        assert lib.asm_batch_kkt_set_form(hb._b, form, order) == ERR_ARG, (form, order)
    for form, order in ((0, 0), (0, 1), (1, 1)):
        assert lib.asm_batch_kkt_set_form(hb._b, form, order) == 0, (form, order)
    with pytest.raises(A.AsmHipError, match="per handle"):
        hb.set_kkt_form("sparse", "working-set")
    with pytest.raises(ValueError):
        hb.set_kkt_form("banded", "static")
    runs = hb.slp_run(*_stack(prs), _par())
    _all_sparse_static(hb)
    hb.setup(prs[0])                                                      # the set-up starts from the dense form again
    hb.set_ns_basis(J)
    ep, sp = batch.slp_eqp_params(_par()), batch.slp_params(_par())
    gl, gu, xl, xu, x0 = (np.ascontiguousarray(a, np.float64) for a in _stack(prs))
    R, D = (_lib.SlpResult * S)(), _lib.dptr
    assert lib.asm_batch_slp_run_eqp(hb._b, S, D(gl), D(gu), D(xl), D(xu), D(x0), C.byref(sp), 0.4, C.byref(ep), None, None, None, None, None, R, None, None) == 0
    assert all(fi.form_requested == 0 and fi.form_used == 0 and fi.sparse_bytes == 0 for fi, _ in _slot_infos(hb))
    hb.close()
    for r, one in zip(runs, ones):
        _same_run(r, one)


def test_a_model_without_a_sparse_pattern_runs_the_dense_form_on_every_slot():
    fm = problems.synthetic_dense_function_model(24, 12, hessian=True)
    pr = fm.to_problem("dense24")
    rng = np.random.RandomState(5)
    gl, gu, xl, xu = (np.tile(getattr(pr, k), (S, 1)) for k in ("g_L", "g_U", "x_L", "x_U"))
    x0 = np.clip(np.tile(pr.x0, (S, 1)) + 0.05 * rng.standard_normal((S, pr.n)), xl, xu)
    out = {}
    for form, order in (("sparse", "static"), ("dense", "working-set")):
        hb = batch.HipBatch(pr, S)
        out[form] = hb.slp_run(gl, gu, xl, xu, x0, _par(form, order))
        for fi, oi in _slot_infos(hb):
            assert (fi.form_requested, fi.form_used, oi.order_used) == (int(form == "sparse"), 0, 0) and fi.sparse_bytes == 0 and fi.dense_bytes > 0
        hb.close()
    print("dense24: iter", [r.iter for r in out["dense"]], "eqp", [r.eqp_counts for r in out["dense"]])
    for a, b in zip(out["sparse"], out["dense"]):
        _same_run(a, b)
    assert sum(r.eqp_counts["attempts"] for r in out["dense"]) >= 1


def test_case118_sized_scenarios_beyond_640_working_rows():
    """Two case118-sized load scenarios (n = 1 180, m = 1 725, 981 equality rows: more working rows than one banded panel launch takes)
    in two slots against fresh handles.  max_iter = BIG_MAX_ITER is the smallest value at which each scenario makes a trial."""
    base = acopf.synthetic_case("case118", 1, 0.5)
    prs = [acopf.function_model(acopf.scenario_case(base, s), nlp="expr").to_problem("case118-sized load scenario %d" % s) for s in range(2)]
    par = _par(max_iter=BIG_MAX_ITER)
    hb = batch.HipBatch(prs[0], 2)
    runs = hb.slp_run(*_stack(prs), par)
    infos, bst, J = _slot_infos(hb), hb.stats(), hb.ns_basis()
    lib, nW = _lib.load(), C.c_int64(0)
    for s, (fi, oi) in enumerate(infos):
        assert (fi.form_used, oi.order_used) == (1, 1) and fi.dense_bytes == 0
        assert lib.asm_kkt_row_order(lib.asm_batch_handle(hb._b, s), None, C.byref(nW)) == 0
        assert nW.value > 640 and 0 < 2 * fi.band < nW.value, (s, nW.value, fi.band)      # the last trial's factor was banded, beyond one panel launch
    hb.close()
    print("case118-sized: iter", [r.iter for r in runs], "eqp", [r.eqp_counts for r in runs], "last band / pairs", [(fi.band, fi.n_pairs) for fi, _ in infos],
          "batch", {k: bst[k] for k in ("ops", "launches", "rounds", "panel_launches", "panel_ops")})
    for s, pr in enumerate(prs):
        one, fi, _ = _fresh_handle_run(pr, par, J)
        _same_run(runs[s], one)
        assert one.eqp_counts["attempts"] >= 1
    assert bst["ops"] > bst["launches"]
