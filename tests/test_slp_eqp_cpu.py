"""CPU checks of SLP-EQP (include/asm_hip.h, "SLP-EQP"; activesetmethods_amd/slp.py: SlpEQP; eqp.py: lp_working_set, eqp_trial_host): the
working set an LP's active set names on hand-made cases, the driver on the oracle-backed LP of tests/test_host_cpu.py with the NumPy
trial step - hs071, a 14-bus ACOPF and the parametric model against the Trust-Region driver on the same set-up - the switch that
leaves the Trust-Region driver, a run that never leaves restoration, skipped trials, and the bindings against the header."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import acopf, eqp
from tests.test_host_cpu import _OracleBackedSubOptimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
HS071_X = np.array([1.0, 4.74299964, 3.82114998, 1.37940829])


def grid14_function_model():
    return acopf.function_model(acopf.synthetic_grid(14, 5, 20, 1, 0.5), nlp="expr")


def host_factory(fm, pr, trial=None):
    """The oracle-backed LP with eqp_trial: eqp.eqp_trial_host, or `trial` (a stub) with the same arguments after (fm, pr)."""
    class Opt(_OracleBackedSubOptimizer):
        calls = []

        def eqp_trial(self, x, lam, lp_rows, lp_bnd, radius, nu, tol):
            Opt.calls.append((np.array(x), float(radius)))
            return (trial or eqp.eqp_trial_host)(fm, pr, x, lam, lp_rows, lp_bnd, radius, nu, tol)
    return Opt


def run(fm, algorithm, name="model", trial=None, **kw):
    pr = fm.to_problem(name)
    mdl = A.Model.from_problem(pr, A.Parameters(algorithm=algorithm, external_optimizer=host_factory(fm, pr, trial), **kw))
    return mdl, A.optimize(mdl)


def same_run(a, b):
    """Trace, iterates, multipliers and counts of two runs, exactly."""
    assert (a.ret, a.iter, a.lp_solves, a.Delta) == (b.ret, b.iter, b.lp_solves, b.Delta)
    assert np.array_equal(a.x, b.x) and np.array_equal(a.lam, b.lam) and np.array_equal(a.mult_x_U, b.mult_x_U) and np.array_equal(a.mult_x_L, b.mult_x_L)
    assert len(a.trace) == len(b.trace)
    for ra, rb in zip(a.trace, b.trace):
        assert (ra["iter"], ra["fr"], ra["status"], ra["delta"]) == (rb["iter"], rb["fr"], rb["status"], rb["delta"])
        assert all(np.array_equal(ra[k], rb[k]) for k in ("x", "p", "lam", "mult_x_U", "mult_x_L"))


@pytest.fixture(scope="module")
def tr_runs():
    """The Trust-Region driver on the three models, once for the module."""
    return {"hs071": run(A.problems.hs071_function_model(), "Trust Region"),
            "grid14": run(grid14_function_model(), "Trust Region", max_iter=60),
            "parametric": run(A.problems.parametric_function_model(), "Trust Region")}


# ------------------------------------------------------------------------------------------------ 1. the working set
def _rows_problem():
    """Four rows over three variables: an equality, a range row, a one-sided upper row, a one-sided lower row; adj = [1]."""
    return SimpleNamespace(n=3, m=4, g_L=np.array([2.0, -1.0, -INF, 0.5]), g_U=np.array([2.0, 3.0, 4.0, INF]),
                           x_L=np.array([0.0, -INF, -5.0]), x_U=np.array([10.0, 1.0, INF]))


def test_working_set_rows():
    pr = _rows_problem()
    x = np.array([1.0, 0.0, 0.0])
    none = (np.zeros(5, np.int32), np.zeros(3, np.int32))
    rs, bs, at = eqp.lp_working_set(pr, x, none)
    assert rs.tolist() == [1, 0, 0, 0] and bs.tolist() == [0, 0, 0] and at.tolist() == [2.0, 0.0, 0.0, 0.0]      # an equality the LP calls inactive is in W
    rs, _, at = eqp.lp_working_set(pr, x, (np.array([0, 0, 0, 0, 1]), none[1]))
    assert rs.tolist() == [1, 1, 0, 0] and at[1] == 3.0                                                           # the range row's twin: at g_U
    rs, _, at = eqp.lp_working_set(pr, x, (np.array([0, 1, 0, 0, 0]), none[1]))
    assert rs.tolist() == [1, 1, 0, 0] and at[1] == -1.0                                                          # the range row itself: at g_L
    rs, _, at = eqp.lp_working_set(pr, x, (np.array([0, 0, 1, 1, 0]), none[1]))
    assert rs.tolist() == [1, 0, 1, 1] and at[2] == 4.0 and at[3] == 0.5                                          # one-sided rows: at their finite bound
    assert rs.dtype == np.int32 and bs.dtype == np.int32


def test_working_set_variables():
    pr = _rows_problem()
    rows = np.zeros(5, np.int32)
    lp = np.array([-1, 1, -1])
    # variable 0 at its real lower bound, variable 1 stopped by the trust region below its bound 1.0, variable 2 stopped by the region
    _, bs, _ = eqp.lp_working_set(pr, np.array([0.0, 0.4, -3.0]), (rows, lp))
    assert bs.tolist() == [-1, 0, 0]
    # at the real bound on the side the LP reports; on the other side it is free
    _, bs, _ = eqp.lp_working_set(pr, np.array([10.0, 1.0, -5.0]), (rows, np.array([1, 1, -1])))
    assert bs.tolist() == [1, 1, -1]
    _, bs, _ = eqp.lp_working_set(pr, np.array([10.0, 1.0, -5.0]), (rows, np.array([-1, -1, 1])))
    assert bs.tolist() == [0, 0, 0]                                   # (variable 1 has no lower bound, variable 2 no upper one)
    # the tolerance is relative to 1 + |bound|
    _, bs, _ = eqp.lp_working_set(pr, np.array([10.0 - 5e-8, 1.0, 0.0]), (rows, np.array([1, 0, 0])), tol=1e-8)
    assert bs.tolist() == [1, 0, 0]
    _, bs, _ = eqp.lp_working_set(pr, np.array([10.0 - 2e-7, 1.0, 0.0]), (rows, np.array([1, 0, 0])), tol=1e-8)
    assert bs.tolist() == [0, 0, 0]


@pytest.mark.parametrize("rows,bnd,x", [(4, 3, 3), (5, 2, 3), (5, 3, 2), (6, 3, 3)])
def test_working_set_refuses_wrong_lengths(rows, bnd, x):
    with pytest.raises(ValueError):
        eqp.lp_working_set(_rows_problem(), np.zeros(x), (np.zeros(rows, np.int32), np.zeros(bnd, np.int32)))


def test_trial_host_refuses_a_negative_tolerance():
    fm = A.problems.hs071_function_model()
    pr = fm.to_problem("hs071")
    for tol in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            eqp.eqp_trial_host(fm, pr, pr.x0, np.zeros(2), np.zeros(2, np.int32), np.zeros(4, np.int32), 1.0, np.ones(2), tol)


# ------------------------------------------------------------------------------------------------ 2. the driver against Trust Region
def test_hs071(tr_runs):
    """Trust Region: 31 iterations, final radius 8e-7; SLP-EQP: 10 iterations, 4 trials, all accepted."""
    mdl, s = run(A.problems.hs071_function_model(), "SLP-EQP")
    tr = tr_runs["hs071"][1]
    print("hs071: SLP-EQP status %d iter %d lp %d %r radius %g dual %.2e | Trust Region status %d iter %d lp %d" %
          (mdl.status, s.iter, s.lp_solves, s.eqp_counts, s.Delta_E, s.dual_infeas, tr.ret, tr.iter, tr.lp_solves))
    assert mdl.status == 0 and np.abs(mdl.x - HS071_X).max() <= 1e-5
    assert 2 * s.iter <= tr.iter
    c = s.eqp_counts
    assert c["attempts"] == c["accepted"] + c["rejected"] + c["skipped_rows"] + c["skipped_dependent"] + c["skipped_zero"] and c["accepted"] >= 1
    assert mdl.statistics["eqp"]["radius"] == s.Delta_E and mdl.statistics["eqp"]["accepted"] == c["accepted"]
    assert s.lp_solves == len(s.trace)                                       # the trials solve no LP


def test_grid14(tr_runs):
    """The 14-bus ACOPF (n = 118, m = 189) with max_iter = 60: Trust Region stops at the limit with status 6, SLP-EQP converges (25)."""
    mdl, s = run(grid14_function_model(), "SLP-EQP", max_iter=60)
    mt, tr = tr_runs["grid14"]
    print("grid14: SLP-EQP status %d iter %d lp %d %r radius %g | Trust Region status %d iter %d" %
          (mdl.status, s.iter, s.lp_solves, s.eqp_counts, s.Delta_E, mt.status, tr.iter))
    assert (mt.status, tr.iter) == (6, 60)
    assert mdl.status == 0 and s.iter < 60


def test_parametric_model(tr_runs):
    mdl, s = run(A.problems.parametric_function_model(), "SLP-EQP")
    tr = tr_runs["parametric"][1]
    print("parametric: SLP-EQP status %d iter %d %r | Trust Region iter %d" % (mdl.status, s.iter, s.eqp_counts, tr.iter))
    assert mdl.status == 0 and s.iter <= tr.iter


def test_disabled_is_the_trust_region_driver(tr_runs):
    for name, fm, kw in (("hs071", A.problems.hs071_function_model(), {}), ("parametric", A.problems.parametric_function_model(), {})):
        mdl, s = run(fm, "SLP-EQP", eqp=False, **kw)
        assert isinstance(s, A.SlpEQP) and s.eqp_counts["attempts"] == 0
        same_run(s, tr_runs[name][1])
        assert mdl.status == tr_runs[name][0].status


def test_a_run_in_restoration_attempts_nothing():
    """toy_expr_problem: the first LP is infeasible, the run then stays in restoration up to its last LP, the only normal-phase OPTIMAL
    one, which ends it - so no trial is made and the run is Trust Region's."""
    fm = A.problems.toy_expr_function_model()
    _, tr = run(fm, "Trust Region")
    _, s = run(fm, "SLP-EQP")
    assert all(r["fr"] for r in tr.trace[1:-1]) and tr.lp_solves > 3 and tr.trace[0]["status"] == 2 and not tr.trace[-1]["fr"]
    assert s.eqp_counts["attempts"] == 0
    same_run(s, tr)


@pytest.mark.parametrize("code,key", [(1, "skipped_rows"), (2, "skipped_dependent")])
def test_skipped_trials_leave_the_trust_region_run(tr_runs, code, key):
    def stub(fm, pr, x, lam, lp_rows, lp_bnd, radius, nu, tol):
        z = np.zeros(pr.n)
        return z, np.zeros(pr.m), z, z, np.zeros(pr.m, np.int32), np.zeros(pr.n, np.int32), SimpleNamespace(skipped=code, cg_iters=3)
    _, s = run(A.problems.hs071_function_model(), "SLP-EQP", trial=stub)
    tr = tr_runs["hs071"][1]
    same_run(s, tr)
    c = s.eqp_counts
    assert c[key] == c["attempts"] > 0 and c["accepted"] == c["rejected"] == 0 and s.Delta_E == A.Parameters().tr_size
    assert c["cg_iters"] == (0 if code == 1 else 3 * c["attempts"])
    # a trial after every normal-phase OPTIMAL LP but the last
    normal = [r for r in tr.trace if not r["fr"] and r["status"] == 1]
    assert c["attempts"] == len(normal) - 1


def test_a_rejected_trial_halves_the_radius_to_the_step():
    """A stub whose step never lowers the merit function: nothing moves, and the radius of the trial follows ||d|| / 2."""
    seen = []

    def stub(fm, pr, x, lam, lp_rows, lp_bnd, radius, nu, tol):
        seen.append(radius)
        z = np.zeros(pr.n)
        info = SimpleNamespace(skipped=0, cg_iters=1, boundary=1, t=1.0, norm_d=radius, phi0=1.0, phi1=1.0)
        return np.ones(pr.n), np.zeros(pr.m), z, z, np.zeros(pr.m, np.int32), np.zeros(pr.n, np.int32), info
    _, s = run(A.problems.parametric_function_model(), "SLP-EQP", trial=stub, eqp_radius=0.75)
    _, tr = run(A.problems.parametric_function_model(), "Trust Region")
    same_run(s, tr)
    assert seen == [0.75 * 0.5 ** k for k in range(len(seen))] and len(seen) == s.eqp_counts["rejected"] > 0


# ------------------------------------------------------------------------------------------------ 3. parameters and bindings
def test_parameters_keep_the_reference_defaults():
    p = A.Parameters()
    assert (p.tol_direction, p.tol_residual, p.tol_infeas, p.max_iter) == (1e-6, 0.01, 0.01, 1000)
    assert (p.eta, p.tau, p.min_alpha, p.tr_size) == (0.4, 0.9, 1e-6, 0.4) and p.algorithm == "Line Search" and p.method == "SLP" and p.device_eval is False
    assert (p.eqp_radius, p.eqp_radius_max, p.eqp_tol_active, p.eqp) == (None, 1e3, 1e-8, True)
    mdl = A.Model.from_problem(A.problems.hs071_problem(), A.Parameters(algorithm="SLP-EQP", tr_size=0.3, device_eval=True))
    assert A.SlpEQP(mdl).Delta_E == 0.3
    mdl.parameters.eqp_radius = 2.5
    assert A.SlpEQP(mdl).Delta_E == 2.5
    for bad in (dict(eqp_radius=0.0), dict(eqp_radius=INF), dict(eqp_radius_max=0.0), dict(eqp_tol_active=-1.0)):
        with pytest.raises(ValueError):
            A.SlpEQP(A.Model.from_problem(A.problems.hs071_problem(), A.Parameters(algorithm="SLP-EQP", device_eval=True, **bad)))
    # on the HIP sub-optimizer the trial reads what the device evaluator left in HBM: host callbacks are refused before any handle is made
    with pytest.raises(ValueError):
        A.optimize(A.Model.from_problem(A.problems.hs071_problem(), A.Parameters(algorithm="SLP-EQP")))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asm_hip.h")).read(), flags=re.S)


def _c_layout(name):
    """[(field, offset)] and the size of a typedef'd struct of int32_t and double fields in the header, by the C rules."""
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, _header()).group(1)
    sizes = {"int32_t": 4, "double": 8}
    fields, off = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            for n in names.split(","):
                off = -(-off // sizes[ctype]) * sizes[ctype]
                fields.append((n.strip(), off))
                off += sizes[ctype]
    return fields, -(-off // 8) * 8


@pytest.mark.parametrize("cname,pyname", [("asm_eqp_info", "EqpInfo"), ("asm_slp_eqp_params", "SlpEqpParams"), ("asm_slp_eqp_info", "SlpEqpInfo")])
def test_structures_match_the_header(cname, pyname):
    from activesetmethods_amd import _lib
    fields, size = _c_layout(cname)
    T = getattr(_lib, pyname)
    assert [(f[0], getattr(T, f[0]).offset) for f in T._fields_] == fields and ctypes.sizeof(T) == size
    if cname == "asm_eqp_info":          # it begins with the fields of asm_kkt_step_info, at their offsets
        step, _ = _c_layout("asm_kkt_step_info")
        assert fields[:len(step)] == step


def test_prototypes_match_the_header():
    from activesetmethods_amd import _lib
    txt = _header()
    for name in ("asm_eqp_trial", "asm_slp_run_eqp"):
        args = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, txt).group(1).split(",")
        res, types = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(types) == len(args)
        for a, t in zip(args, types):
            a = a.strip()
            if "*" not in a:
                assert t is (ctypes.c_double if a.startswith("double") else ctypes.c_int), (name, a)
            elif a.startswith("const double*") or a.startswith("double*"):
                assert t == ctypes.POINTER(ctypes.c_double), (name, a)
            elif "int32_t*" in a:
                assert t == ctypes.POINTER(ctypes.c_int32), (name, a)
    assert _lib.PROTOTYPES["asm_eqp_trial"][1][-1] == ctypes.POINTER(_lib.EqpInfo)
    assert _lib.PROTOTYPES["asm_slp_run_eqp"][1][3] == ctypes.POINTER(_lib.SlpEqpParams)
    assert _lib.PROTOTYPES["asm_slp_run_eqp"][1][-1] == ctypes.POINTER(_lib.SlpEqpInfo)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "asm_eqp_trial") and hasattr(lib, "asm_slp_run_eqp")


def test_dispatch():
    """optimize() selects SlpEQP by name; the scenario batch keeps refusing it; the native record carries the counters."""
    from activesetmethods_amd import _lib, batch
    hb = batch.HipBatch.__new__(batch.HipBatch)
    hb.n, hb.m, hb._b = 2, 1, None
    z = lambda k: np.zeros((1, k))
    with pytest.raises(ValueError):
        hb.slp_run(z(1), z(1), z(2), z(2), z(2), A.Parameters(algorithm="SLP-EQP"))
    with pytest.raises(ValueError):
        A.optimize(A.Model.from_problem(A.problems.hs071_problem(), A.Parameters(algorithm="SLP-EQP")), native=True)      # no device_eval
    res = _lib.SlpResult()
    eq = _lib.SlpEqpInfo(0.8, 5, 3, 1, 0, 1, 0, 17, 2)
    v = np.zeros(2)
    r = batch.NativeRun(res, v, v, v, v, v, _lib.SlpTrInfo(0.05, 5, 2, 3, 1), eq)
    assert r.Delta_E == 0.8 and r.eqp_counts == dict(attempts=5, accepted=3, rejected=1, skipped_rows=0, skipped_dependent=1, skipped_zero=0, cg_iters=17, boundary=2)
    assert batch.NativeRun(res, v, v, v, v, v).eqp_counts is None
