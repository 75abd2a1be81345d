"""Variable-bound sensitivities and the adjoint entries with weights on z of a scenario batch through the C ABI (include/asm_hip.h:
asm_batch_var_bound_sensitivity, asm_batch_solution_adjoint_z): every scenario against the per-handle entry on a fresh handle with that
scenario's data, byte for byte, info included - three hs071 scenarios with a data table on two slots (one refill), and two line
scenarios of the 14-bus grid on the Ohm's-law kernel with derivatives in the dense form and in the sparse form on the static row order;
batch.var_bound_jacobians; a Line-Search batch run before and after the calls."""
import numpy as np
import pytest

from activesetmethods_amd import acopf, batch
from tests.test_batch_eqp_gpu import _line_problems, _par, _same_run, _stack
from tests.test_batch_sens_cpu import hs071_scenario_models
from tests.test_nlparams_gpu import _handle_for

pytestmark = pytest.mark.gpu


def _info(i):
    return tuple(getattr(i, k) for k, _ in i._fields_)


def _kkt_bits(out, c):
    return (out[0][c].tobytes(), out[1][c].tobytes(), out[2][c].tobytes()) + _info(out[3][c])


def _adj_bits(res, c):
    return tuple(a[c].tobytes() for a in res[:5]) + _info(res[5][c])


def _scenario(out, s):
    return tuple(a[s] for a in out)


def _compare(tag, hb, fresh_handle, X, L, rs, bs, vars, delta, GX, GL, GZ):
    """Every scenario of the two batch entries (the adjoint with and without weights) against fresh_handle(s)'s answers."""
    S, k = len(X), len(vars)
    before = hb.stats()
    fwd = hb.var_bound_sensitivity(X, L, rs, bs, vars, delta)
    adj = hb.solution_adjoint_z(X, L, rs, bs, GX, GL, GZ)
    adj0 = hb.solution_adjoint_z(X, L, rs, bs, GX, GL)
    after = hb.stats()
    n, m = hb.n, hb.m
    assert fwd[0].shape == (S, k, n) and fwd[1].shape == (S, k, m) and fwd[2].shape == (S, k, n)
    assert adj[1].shape == (S, GX.shape[1], m) and adj[2].shape == (S, GX.shape[1], n) and adj[0].shape == (S, GX.shape[1], hb.n_dpar)
    assert after["ops"] - before["ops"] > after["launches"] - before["launches"] > 0, (tag, before, after)          # the slots' launches merged
    live = 0
    for s in range(S):
        opt = fresh_handle(s)
        want = opt.var_bound_sensitivity_multi(X[s], L[s], rs[s], bs[s], vars, delta)
        wadj = opt.solution_adjoint_z_multi(X[s], L[s], rs[s], bs[s], GX[s], GL[s], GZ[s])
        wadj0 = opt.solution_adjoint_z_multi(X[s], L[s], rs[s], bs[s], GX[s], GL[s])
        opt.close()
        got = _scenario(fwd, s)
        for c in range(k):
            assert _kkt_bits(got, c) == _kkt_bits(want, c), (tag, "var bound", s, c)
            if bs[s][vars[c]] == 0:
                assert not got[0][c].any() and not got[2][c].any() and got[3][c].cg_iters == 0
            else:
                assert got[0][c, vars[c]] == (1.0 if delta is None else delta[c])
                live += got[3][c].status == 0 and bool(np.any(got[2][c] != 0.0))
        for name, g, w in (("adjoint z", _scenario(adj, s), wadj), ("adjoint, no weights", _scenario(adj0, s), wadj0)):
            for c in range(GX.shape[1]):
                assert _adj_bits(g, c) == _adj_bits(w, c), (tag, name, s, c)
                assert not g[2][c][bs[s] == 0].any()
        assert not np.array_equal(adj[2][s], adj0[2][s])
        print("%s scenario %d: var-bound statuses %r CG %r, adjoint statuses %r CG %r" % (tag, s, [i.status for i in got[3]], [i.cg_iters for i in got[3]],
              [i.status for i in adj[5][s]], [i.cg_iters for i in adj[5][s]]))
    assert live >= 1, tag                                         # the comparison is not of zeros
    return fwd


def test_hs071_scenarios_with_a_data_table_on_two_slots():
    S = 3
    fms = hs071_scenario_models(S)
    prs = [fm.to_problem("hs071 scenario %d" % s) for s, fm in enumerate(fms)]
    hb = batch.HipBatch(prs[0], 2)
    data = hb.scenario_data(prs)
    assert data is not None and data.shape == (S, 2)
    runs = hb.slp_run(*_stack(prs), _par(), data=data)
    rs, bs = batch.working_sets(prs, runs)
    assert rs.tolist() == [[1, 1]] * S and bs.tolist() == [[-1, 0, 0, 0]] * S
    X, L = np.stack([r.x for r in runs]), np.stack([r.lam for r in runs])
    rng = np.random.default_rng(37)
    GX, GL, GZ = rng.standard_normal((S, 2, 4)), rng.standard_normal((S, 2, 2)), rng.standard_normal((S, 2, 4))
    vars, delta = np.array([0, 2, 0], np.int32), np.array([1.5, 1.0, -0.25])

    def fresh(s):
        opt = _handle_for(prs[0], fms[0])
        opt.set_eval_data(data[s])
        return opt
    fwd = _compare("hs071", hb, fresh, X, L, rs, bs, vars, delta, GX, GL, GZ)
    assert not np.array_equal(fwd[0][0], fwd[0][1])                                   # the scenarios' data reached their slots
    Jx, Jl, Jz, status = batch.var_bound_jacobians(hb, prs, runs, vars)
    ones = hb.var_bound_sensitivity(X, L, rs, bs, vars)
    hb.close()
    assert Jx.shape == (S, 4, 3) and Jl.shape == (S, 2, 3) and Jz.shape == (S, 4, 3) and status.shape == (S, 3) and not status.any()
    assert np.array_equal(Jx, np.transpose(ones[0], (0, 2, 1))) and np.array_equal(Jl, np.transpose(ones[1], (0, 2, 1)))
    assert np.array_equal(Jz, np.transpose(ones[2], (0, 2, 1)))
    with pytest.raises(ValueError):
        batch.var_bound_jacobians(hb, prs, runs, [4])


def test_line_scenarios_on_the_ohm_kernel_in_both_forms():
    base = acopf.synthetic_grid(14, 5, 20, 1, 0.5)
    prs = [acopf.function_model(acopf.line_scenario_case(base, s), hessian=True).to_problem("grid14 ohm line scenario %d" % s) for s in range(2)]
    assert prs[0].function_model.nlp.device[0] == "acopf_ohm_hess"
    S, n, m = 2, prs[0].n, prs[0].m
    hb = batch.HipBatch(prs[0], 2)
    runs, _, _ = batch.solve_batch_lockstep(prs, _par(), 2, batch=hb)
    rs, bs = batch.working_sets(prs, runs)
    X, L = np.stack([r.x for r in runs]), np.stack([r.lam for r in runs])
    # two variables that are free in both scenarios join B there (a working set is a statement about the linear algebra; the calls are what
    # is compared), beside whatever the runs left at a bound; one variable stays free: its column is zero
    free = [int(j) for j in range(n) if not bs[:, j].any()]
    assert len(free) - 2 >= rs.sum(axis=1).max() + 1
    bs[:, free[:2]] = -1
    bound0 = [int(j) for j in np.nonzero(bs[0])[0]]
    vars = np.array(free[:2] + [free[2], bound0[-1]], np.int32)
    delta = np.array([1.0, -0.5, 2.0, 0.75])
    mdl = prs[0].function_model.acopf_model
    GX, GL, GZ = np.zeros((S, 2, n)), np.zeros((S, 2, m)), np.zeros((S, 2, n))
    for s in range(S):
        GX[s, 0, [j for j in mdl.pf if bs[s, j] == 0][0]] = 1.0                       # a line flow ...
        GZ[s, 0, free[0]] = 1.0                                                       # ... with the price of a variable bound
        GL[s, 1, np.nonzero(rs[s])[0][0]] = 1.0                                       # a row price ...
        GZ[s, 1, free[1]] = -2.0
        GZ[s, 1, free[2]] = 9.0                                                       # (on F: ignored)
    for form in ("dense", "sparse"):
        hb.set_kkt_form(form, "static" if form == "sparse" else "working-set")

        def fresh(s):
            opt = _handle_for(prs[s])
            if form == "sparse":
                opt.set_kkt_form("sparse")
                opt.set_kkt_order("static")
            return opt
        _compare("grid14 ohm, %s form" % form, hb, fresh, X, L, rs, bs, vars, delta, GX, GL, GZ)
        chk = fresh(0)
        chk.var_bound_sensitivity_multi(X[0], L[0], rs[0], bs[0], vars)
        assert chk.kkt_form_info().form_used == (1 if form == "sparse" else 0)
        chk.close()
    hb.close()


def test_a_line_search_run_returns_its_bits_after_the_calls():
    prs = _line_problems()
    S = len(prs)
    hb = batch.HipBatch(prs[0], S)
    data = hb.scenario_data(prs)
    ls = _par(algorithm="Line Search")
    first = hb.slp_run(*_stack(prs), ls, data=data)
    X, L = np.stack([r.x for r in first]), np.stack([r.lam for r in first])
    # (the equality rows and two variables at a bound: a valid working set at any point - the calls are what matters here)
    rs, bs = np.stack([(p.g_L == p.g_U).astype(np.int32) for p in prs]), np.zeros((S, hb.n), np.int32)
    bs[:, :2] = -1
    assert rs[0].sum() <= hb.n - 2
    rng = np.random.default_rng(29)
    hb.var_bound_sensitivity(X, L, rs, bs, [0, 1, 5], [1.0, -1.0, 2.0])
    hb.solution_adjoint_z(X, L, rs, bs, rng.standard_normal((S, 2, hb.n)), rng.standard_normal((S, 2, hb.m)), rng.standard_normal((S, 2, hb.n)))
    hb.solution_adjoint_z(X, L, rs, bs, rng.standard_normal((S, 2, hb.n)), rng.standard_normal((S, 2, hb.m)))
    third = hb.slp_run(*_stack(prs), ls, data=data)
    hb.close()
    for a, b in zip(first, third):
        _same_run(a, b)
        assert a.ls_trials == b.ls_trials
