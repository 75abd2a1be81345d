"""The null-space interior-point iteration with its factor-independent head on a side stream (ASM_NS_SIDE) and with k_ns_add / k_ns_dp folded
into the kernels in front of them (ASM_NS_FOLD): no value may change.

Reduced solve and direction: the solver's members (k_wtrsv_bwd_diag_add, k_gemv_t_stage2_dp) against the stage lists of the separate kernels on
the same state through asm_test_ns_stages, bit for bit, everything else back as loaded.  End to end: one LP on handles made with the knobs on and
off - answer and statistics bit for bit - at k = 137 (case300-sized grid: the one-workgroup solves, only the side stream differs) and at k = 519
(acopf.synthetic_case has no instance between 256 and 1024 besides the case1354pegase-sized one: the first normal-phase LP of
test_c4_size_three_consecutive_normal_phase_lps, once per knob setting).  Determinism: the same LP three times on one handle - a missing join
between the streams shows as a run that differs."""
import numpy as np
import pytest

from activesetmethods_amd import acopf
from tests import util
from tests.test_ns_stages_gpu import Run, same, stage

pytestmark = pytest.mark.gpu
SC = util.SC
# (n, M, k, nI): 257 = first order beyond the one-workgroup path, one row past a 4-row workgroup; 519 = 8 * 64 + 7, the flagship's k
CASES = [(300, 330, 257, 70), (300, 330, 300, 70), (600, 560, 519, 40)]
IDS = ["n%d-M%d-k%d-nI%d" % c for c in CASES]
KNOBS = [{}, {"ASM_NS_SIDE": "0"}, {"ASM_NS_SIDE": "0", "ASM_NS_FOLD": "0"}]

_STATES = {}


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = util.abi_create(hip_lib)
    yield h
    hip_lib.asm_destroy(h)


def state(case):
    if case not in _STATES:
        _STATES[case] = util.ns_state(70 + CASES.index(case), *case)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _STATES[case].items()}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reduced_solve_with_the_add_folded_in(hip_lib, handle, case):
    st = state(case)
    k = st["k"]
    st["scal"][SC["NSERR"]] = 0.0
    o = Run(hip_lib, handle, st, []).nsv      # work vectors of the solver's sequence: ru 10, du 11, rr 12, dd 13
    ru, du, rr, dd = o[10], o[11], o[12], o[13]
    old = Run(hip_lib, handle, st, [stage("factor"), stage("chol_solve", x=[ru, du]), stage("symv_res", x=[du, ru, rr]), stage("chol_solve", x=[rr, dd]),
                                    stage("add", x=[du, dd, du], len=k), stage("symv_res", x=[du, ru, rr]), stage("relres", x=[rr, ru])])
    new = Run(hip_lib, handle, st, [stage("factor"), stage("reduced_solve")])
    for nm in ("du", "dd", "rr"):
        assert same(new.v(nm), old.v(nm)), nm
        assert not same(new.v(nm), st[nm]), nm      # (written, not left as loaded)
    assert same(new.sc("NSERR"), old.sc("NSERR")) and new.sc("NSERR") > 0.0
    assert same(new.factor(), old.factor())
    for r in (old, new):
        r.only(vecs=["du", "rr", "dd"], scal=["NSERR"], regions=[(r.S, r.fld ** 2 + r.linv_len)])
    assert new.grid[1] == -(-k // 4)      # the grid of the first k_ns_symv_res, as before


@pytest.mark.parametrize("D", ["A", "C"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_direction_with_dp_folded_in(hip_lib, handle, case, D):
    st = state(case)
    n = st["n"]
    fx = st["ub"] == st["lb"]
    assert fx.sum() >= 2 and np.all(st["th"][fx] == 0) and n % 32 != 0      # zeros in theta (fixed columns) and ldn padding
    o = Run(hip_lib, handle, st, []).nsv
    old = Run(hip_lib, handle, st, [stage("gemv_t", x=[o[11], o[3]]), stage("dp", D=D, res=1.0, x=[o[3]])])
    new = Run(hip_lib, handle, st, [stage("direction", D=D, res=1.0)])
    for nm, full in (("v", True), (D + ".dp", True), (D + ".dmuL", False), (D + ".dmuU", False)):
        assert same(new.v(nm, full), old.v(nm, full)), nm
    assert np.all(new.v(D + ".dp", True)[:n][fx] == 0) and np.all(new.v(D + ".dp", True)[n:] == 0) and np.any(new.v(D + ".dp") != 0)
    for r in (old, new):
        r.only(full=[D + ".dp", "v"], vecs=[D + ".dmuL", D + ".dmuU"])
    assert new.grid == [-(-new.ldn // 256)] and old.grid[1] == new.grid[0]      # launch_ns_dp's grid


def _solve(hip_lib, monkeypatch, knobs, sp, repeats=1):
    """`repeats` set-ups and solves of the LP on ONE handle made with `knobs` in the environment (read at asm_create)."""
    for nm in ("ASM_NS_SIDE", "ASM_NS_FOLD"):
        monkeypatch.delenv(nm, raising=False)
    for nm, v in knobs.items():
        monkeypatch.setenv(nm, v)
    h = util.abi_create(hip_lib)
    try:
        outs = []
        for _ in range(repeats):
            assert util.abi_setup(hip_lib, h, sp) == 0, hip_lib.asm_last_error(h)
            out, stt = util.abi_solve(hip_lib, h, sp)
            assert out[0] == 1
            outs.append((out, {nm: stt[nm] for nm in ("ipm_iters", "ns_iters", "path", "nfact", "ns_dim")}))
        return outs
    finally:
        hip_lib.asm_destroy(h)


def _acopf_lp(name):
    pr = acopf.acopf_problem(acopf.synthetic_case(name, 1, 0.5), name)
    x = np.asarray(pr.x0, float).copy()
    return dict(n=pr.n, m=pr.m, j_row=pr.j_row, j_col=pr.j_col, dE=pr.eval_jac_g(x, np.zeros(pr.nnz)), df=pr.eval_grad_f(x, np.zeros(pr.n)),
                f=pr.eval_f(x), E=pr.eval_g(x, np.zeros(pr.m)), x_k=x.copy(), c_lb=pr.g_L, c_ub=pr.g_U, v_lb=pr.x_L, v_ub=pr.x_U, delta=1000.0)


@pytest.fixture(scope="module")
def lp300():
    return _acopf_lp("case300")


@pytest.mark.parametrize("name,k", [("case300", 137), ("case1354pegase", 519)])
def test_knobs_do_not_change_an_lp(hip_lib, monkeypatch, lp300, name, k):
    sp = lp300 if name == "case300" else _acopf_lp(name)
    runs = [_solve(hip_lib, monkeypatch, knobs, sp)[0] for knobs in KNOBS]
    assert runs[0][1]["ns_dim"] == k and runs[0][1]["ns_iters"] > 0, runs[0][1]
    for out, stt in runs[1:]:
        assert stt == runs[0][1], (stt, runs[0][1])
        assert out == runs[0][0]


def test_three_solves_on_one_handle_are_identical(hip_lib, monkeypatch, lp300):
    runs = _solve(hip_lib, monkeypatch, {}, lp300, repeats=3)
    assert runs[0][1]["ns_iters"] > 0
    for out, stt in runs[1:]:
        assert stt == runs[0][1] and out == runs[0][0]
