"""The long-double twins of the null-space iteration kernels (tests/util.py) chained into whole iterations against the oracle's IPM in null-space
form, and the properties of the generator tests/test_ns_stages_gpu.py relies on.  No GPU."""
import sys

import numpy as np
import pytest

from oracle import lp_solver as O
from tests import util
from tests.test_ipm_stages_cpu import permuted, rel

ITERS = 4
ITERATE = ("p", "g", "y", "tL", "tU", "muL", "muU", "pi")
PLACE = {"p": "c", "tL": "c", "tU": "c", "muL": "c", "muU": "c", "g": "r", "y": "r", "pi": "r"}


def ns_lp(seed):
    """The normal-phase LP of an equality-rich sparse sub-problem (n = 120, 100 equality and 60 inequality rows), scaled as the solver scales it."""
    from oracle.subproblem import QpData, QpModel, compute_jacobian_matrix
    sp = util.equality_rich_subproblem(seed, n=120, neq=100, nineq=60)
    A, stored = compute_jacobian_matrix(sp["m"], sp["n"], sp["j_row"] - 1, sp["j_col"] - 1, sp["dE"])
    qp = QpModel(QpData(sp["df"], sp["f"], A, sp["E"], sp["c_lb"], sp["c_ub"], sp["v_lb"], sp["v_ub"], stored), sp["j_row"], sp["j_col"])
    lp = qp.build_lp(sp["x_k"], sp["delta"], False)
    lp.ub[[0, lp.n - 1]] = lp.lb[[0, lp.n - 1]]      # two fixed columns
    return lp


def oracle_ns_trace(lp, nsp, iters):
    """IPM.run in null-space form for `iters` iterations: the final iterate, e, and per iteration (pinf, dinf, mu, ap, ad).  The step lengths are
    read by a trace function from the locals `ap`, `ad`, `b` of run (see tests/test_ipm_stages_cpu.py: oracle_trace)."""
    ipm = O.IPM(lp, nsp=nsp)
    steps = {}

    def tracer(frame, event, arg):
        if frame.f_code.co_name != "run" or not frame.f_code.co_filename.endswith("lp_solver.py"):
            return None

        def local(fr, ev, a):
            if ev == "line" and "b" in fr.f_locals and "ap" in fr.f_locals:
                steps[fr.f_locals["self"].iters] = (fr.f_locals["ap"], fr.f_locals["ad"])
            return local
        return local
    old = sys.gettrace()
    sys.settrace(tracer)
    try:
        ipm.run(1e-300, iters)
    finally:
        sys.settrace(old)
    assert ipm.iters == iters and ipm.ns_iters == iters and not ipm.ns_off, "the oracle left the null-space form"
    assert sorted(steps) == list(range(1, iters + 1)), "IPM.run no longer has the locals ap, ad and b this trace reads"
    rows = [(lg[1], lg[2], lg[3] * ipm.scale_q) + steps[k + 1] for k, lg in enumerate(ipm.log[:iters])]
    return ipm, np.array(rows)


def twin_state(lp, nsp):
    st = util.ipm_twin_start(lp)
    st["A"] = lp.A
    st["ptr"] = np.concatenate([[0], np.cumsum((lp.A != 0).sum(1))]).astype(np.int32)
    st["Zt"], st["GI"], st["k"] = nsp.Zt, nsp.GI.T.copy(), nsp.k
    st["E"], st["I"] = nsp.E, nsp.I
    for nm in ("dpb", "kdpb", "ht", "v", "e"):
        st[nm] = np.zeros(lp.n)
    for nm in ("yM", "bI"):
        st[nm] = np.zeros(lp.M)
    for nm in ("ru", "du"):
        st[nm] = np.zeros(nsp.k)
    return st


def finish_y(lp, st, nsp):
    """The end of the oracle's run (IPM.ns_finish_y) as Solver::ns_finish_y states it: the measures of the final iterate, then
    y_E += S0^-1 (A rdp)_E in long double on the oracle's factor of S0."""
    LD = util.LD
    st["act"], st["aty"] = lp.A @ st["p"], lp.A.T @ st["y"]
    util._f(util.tw_measures(st), st, ["rdp"])
    rE = (lp.A.astype(LD) @ st["rdp"].astype(LD))[nsp.E]
    L0 = np.tril(nsp.L0).astype(LD)
    st["y"][nsp.E] = np.asarray(st["y"][nsp.E].astype(LD) + util._ld_trsv(L0.T, util._ld_trsv(L0, rE, True), False), np.float64)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_chained_twin_reproduces_the_oracle(seed):
    lp = ns_lp(seed)
    assert O.ns_applicable(lp)
    nsp = O.NullSpace(lp)
    assert nsp.valid
    ipm, rows = oracle_ns_trace(lp, nsp, ITERS)
    # the agreement level: what two float64 evaluation orders of the oracle itself (rows and columns permuted: another order of the equality
    # rows, another basis) differ by after ITERS iterations
    l2, pr, pc, _ = permuted(lp, 10 + seed)
    n2 = O.NullSpace(l2)
    assert n2.valid and n2.k == nsp.k
    ipm2, rows2 = oracle_ns_trace(l2, n2, ITERS)
    back = {"c": np.argsort(pc), "r": np.argsort(pr)}
    # (dinf = max|Zt rdp| depends on the basis, which the reordered LP does not share: it is compared for the twin, which uses the oracle's basis)
    level = max([rel(getattr(ipm, nm), getattr(ipm2, nm)[back[PLACE[nm]]]) for nm in ITERATE] + [rel(rows[:, c], rows2[:, c]) for c in (0, 2, 3, 4)])
    # measured on these five LPs: oracle against its reordering 8.8e-14 .. 1.1e-11, twin against oracle 5.7e-14 .. 1.1e-11 (the assertion uses
    # the level of its own LP, x 10)
    st = twin_state(lp, nsp)
    e, got = None, []
    for _ in range(ITERS):
        row, e = util.ns_twin_iteration(lp, st, nsp, e)
        assert row[5] <= O.NS_RERR
        got.append(row[:5])
    got = np.array(got)
    finish_y(lp, st, nsp)
    worst = max([rel(getattr(ipm, nm), st[nm]) for nm in ITERATE] + [rel(rows[:, c], got[:, c]) for c in range(5)] + [rel(ipm.ns_e, e)])
    print("twin vs oracle %.2e, oracle vs reordered oracle %.2e" % (worst, level))
    assert level > 0.0 and worst <= 10.0 * level


@pytest.mark.parametrize("n,M,k,nI", [(45, 40, 1, 0), (256, 255, 64, 1), (257, 257, 137, 60), (300, 330, 257, 70), (300, 40, 65, 39)])
def test_generator_has_the_shapes_the_kernels_branch_on(n, M, k, nI):
    st = util.ns_state(7, n, M, k, nI)
    cnt = (st["A"] != 0).sum(0)
    assert set(cnt) >= {0, 1, 7, 8, 9, 17} and cnt[n - 2] == 7 and cnt[n - 1] > 0 and cnt[5] == 0 and ((st["A"] != 0).sum(1) == 0).any()
    fx = st["ub"] == st["lb"]
    assert fx[0] and fx[n - 1] and not fx[n - 2] and 0.05 * n <= fx.sum() <= 0.25 * n + 2
    assert not st["Zt"][:, fx].any() and np.all(st["th"][fx] == 0) and np.all(st["th"][~fx] > 0)
    assert len(st["I"]) == nI and len(st["thI"]) == nI and np.all(st["rtype"][st["E"]] == 0)
    if k <= (~fx).sum():
        assert np.abs(st["Zt"] @ st["Zt"].T - np.eye(k)).max() < 1e-13
        assert np.linalg.eigvalsh(st["N0"]).min() > 0
    d = np.arange(k)
    assert np.array_equal(st["N"][d, d], st["N0"][d, d] + (1e-13 * st["N0"][d, d] + 1e-30))
    # no zero magnitude under a non-zero twin value on the state the GPU file evaluates
    for tw in (util.tw_ns_wm_neg(st), util.tw_ns_kx(st), util.tw_ns_ht(st, 1.0, st), util.tw_ns_rows(st, "A", st), util.tw_ns_dp(st, "A", 1.0, st)):
        for nm, t in tw.items():
            if isinstance(t, tuple):
                assert np.all((np.atleast_1d(t[1]) > 0) | (np.atleast_1d(t[0]) == 0)), nm
