"""Adjoint solution sensitivities of a scenario batch through the C ABI (include/asm_hip.h: asm_batch_solution_adjoint): three
line-parameter scenarios of the case118-sized ACOPF on the Ohm's-law kernel with derivatives, on two slots (one refill), two functions
each - every scenario's OUT, DBOUND, AX, AL and infos against asm_solution_adjoint_multi on a fresh handle with that scenario's data,
byte for byte, in the dense form and in the sparse form on the static row order."""
import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import acopf, batch, sensitivity
from tests.test_adjoint_gpu import acopf_functionals
from tests.test_nlparams_gpu import _handle_for

pytestmark = pytest.mark.gpu
S, NRHS = 3, 2


@pytest.fixture(scope="module")
def line_points():
    """(problems, runs) of the three scenarios: each the point of a 6-LP Line-Search run on a handle of its own."""
    base = acopf.synthetic_case("case118", 1, 0.5)
    prs = [acopf.function_model(acopf.line_scenario_case(base, s), hessian=True).to_problem("case118 ohm line scenario %d" % s) for s in range(S)]
    assert prs[0].function_model.nlp.device[0] == "acopf_ohm_hess"
    runs = []
    for pr in prs:
        opt = _handle_for(pr)
        runs.append(opt.slp_run(pr.x0, A.Parameters(algorithm="Line Search", max_iter=60, device_eval=True), 6))
        opt.close()
    return prs, runs


def _bits(res, c):
    OUT, DBOUND, AX, AL, infos = res
    return (OUT[c].tobytes(), DBOUND[c].tobytes(), AX[c].tobytes(), AL[c].tobytes()) + tuple(getattr(infos[c], k) for k, _ in infos[c]._fields_)


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_line_scenarios_equal_fresh_handles(line_points, form):
    prs, runs = line_points
    n, m, nd = prs[0].n, prs[0].m, len(prs[0].function_model.nlp.device[2])
    rs, bs = batch.working_sets(prs, runs)
    X, L = np.stack([r.x for r in runs]), np.stack([r.lam for r in runs])
    # per scenario a voltage magnitude and a price of its own working set (columns 1 and 2 of acopf_functionals)
    GX, GL = (np.stack(v) for v in zip(*[[a[1:] for a in acopf_functionals(pr.function_model, rs[s], bs[s], 3, 31 + s)] for s, pr in enumerate(prs)]))
    assert GX.shape == (S, NRHS, n) and GL.shape == (S, NRHS, m)
    hb = batch.HipBatch(prs[0], 2)
    data = hb.scenario_data(prs)
    assert data is not None and data.shape == (S, nd)
    hb.set_scenario_data(data)
    if form == "sparse":
        hb.set_kkt_form("sparse", "static")
    before = hb.stats()
    out = hb.solution_adjoint(X, L, rs, bs, GX, GL)
    after = hb.stats()
    assert out[0].shape == (S, NRHS, nd) and out[1].shape == (S, NRHS, m) and out[2].shape == (S, NRHS, n) and out[3].shape == (S, NRHS, m)
    assert after["ops"] - before["ops"] > after["launches"] - before["launches"] > 0, (before, after)          # the slots' launches merged
    OUT2, DB2, status = batch.solution_adjoints(hb, prs, runs, GX, GL)
    hb.close()
    assert np.array_equal(OUT2, out[0]) and np.array_equal(DB2, out[1]) and status.shape == (S, NRHS)
    live = 0
    for s, pr in enumerate(prs):
        opt = _handle_for(pr)
        if form == "sparse":
            opt.set_kkt_form("sparse")
            opt.set_kkt_order("static")
        fresh = opt.solution_adjoint_multi(X[s], L[s], rs[s], bs[s], GX[s], GL[s])
        assert opt.kkt_form_info().form_used == (1 if form == "sparse" else 0)
        opt.close()
        got = (out[0][s], out[1][s], out[2][s], out[3][s], out[4][s])
        for c in range(NRHS):
            assert _bits(got, c) == _bits(fresh, c), (form, s, c)
            live += got[4][c].status == 0 and got[4][c].cg_iters >= 1 and bool(np.any(got[0][c] != 0.0))
            W = rs[s] == 1
            assert np.array_equal(got[1][c][W], -got[3][c][W]) and np.all(got[1][c][~W] == 0.0)
        print("%s form, scenario %d: statuses %r, CG iterations %r" % (form, s, [i.status for i in got[4]], [i.cg_iters for i in got[4]]))
    assert live >= 1                                                        # the comparison is not of zeros
    assert not np.array_equal(out[0][0], out[0][1])                         # the scenarios differ
