"""The twins of the basis set-up of the null-space form (tests/util.py: tw_nss_*, nss_chain) chained into whole set-ups against the oracle's
NullSpace on the same LP: same path, same columns J, and a basis Zt that agrees to ten times what the same chain in plain float64 NumPy differs
from the long-double chain by - the reference of tests/test_ns_setup_gpu.py checked on a machine without a GPU.  Also the properties of the
cases that file relies on.  No GPU."""
import numpy as np
import pytest

from oracle import lp_solver as O
from tests import util

LD = np.longdouble
SMALL = ["small", "small-fixed", "small-dep", "k1", "one-ineq", "dense"]
_LPS = {}


def case_lp(name):
    """The normal-phase LP of a case, scaled as the oracle scales it, with the case's fixed columns; the operand of the twins."""
    if name not in _LPS:
        from oracle.subproblem import QpData, QpModel, compute_jacobian_matrix
        sp, fm, kres = util.nss_case(name)
        A, stored = compute_jacobian_matrix(sp["m"], sp["n"], sp["j_row"] - 1, sp["j_col"] - 1, sp["dE"])
        qp = QpModel(QpData(sp["df"], sp["f"], A, sp["E"], sp["c_lb"], sp["c_ub"], sp["v_lb"], sp["v_ub"], stored), sp["j_row"], sp["j_col"])
        lp = qp.build_lp(sp["x_k"], sp["delta"], False)
        lp.ub = np.where(fm > 0, lp.ub, lp.lb)
        assert np.all(lp.ub[fm > 0] > lp.lb[fm > 0])
        cold = O.NullSpace(lp)
        _LPS[name] = (lp, cold, util.NssOp(lp.A, cold.E, cold.I, fm))
    return _LPS[name]


def agree(nsp, tw, tw64, what):
    """Same path and columns; Zt and GI to ten times the float64 chain's distance from the long-double chain."""
    assert nsp.valid and tw["path"] == nsp.how == tw64["path"], what
    assert tw["k"] == nsp.k and np.array_equal(tw["J"], nsp.J) and np.array_equal(tw64["J"], nsp.J), what
    level = float(np.abs(tw64["Zt"] - tw["Zt"]).max())
    worst = float(np.abs(nsp.Zt - tw["Zt"]).max())
    print("%s: oracle vs twin chain %.2e, float64 NumPy vs twin chain %.2e" % (what, worst, level))
    assert level > 0 and worst <= 10.0 * level, what
    gl = float(np.abs(tw64["GI"] - tw["GI"]).max())
    assert float(np.abs(nsp.GI.T - tw["GI"]).max()) <= 10.0 * max(gl, level), what


@pytest.mark.parametrize("name", SMALL)
def test_three_paths_against_the_oracle(name):
    lp, cold, op = case_lp(name)
    M = lp.M
    agree(cold, util.nss_chain(op, LD, M=M), util.nss_chain(op, np.float64, M=M), name + " cold")
    assert cold.how == "cold"
    J = cold.J
    cols = O.NullSpace(lp, warm_J=J)
    assert cols.how == "columns"
    agree(cols, util.nss_chain(op, LD, hint_J=J, M=M), util.nss_chain(op, np.float64, hint_J=J, M=M), name + " columns")
    rng = np.random.default_rng(3)
    Zw = cold.Zt * (1.0 + 1e-3 * rng.standard_normal(cold.Zt.shape))      # the basis of a neighbouring LP
    bas = O.NullSpace(lp, warm_J=J, warm_Z=Zw)
    assert bas.how == "basis"
    agree(bas, util.nss_chain(op, LD, hint_J=J, warm_Z=Zw, M=M), util.nss_chain(op, np.float64, hint_J=J, warm_Z=Zw, M=M), name + " basis")
    # the condition the active-set solves state, on the twin chain's own basis
    for tw in (util.nss_chain(op, LD, M=M), util.nss_chain(op, LD, hint_J=J, warm_Z=Zw, M=M)):
        a, b, c = util.nss_quality(op, tw["Zt"], tw["GI"])
        print("%s: |A_EF Zt'| %.1e  |Zt Zt' - I| %.1e  |GI - A_I Zt'| %.1e" % (name, a, b, c))
        assert a <= 1e-13


@pytest.mark.parametrize("name", ["banded", "wide", "wide-fixed"])
def test_large_cases_against_the_oracle(name):
    """The cases that reach a banded S0, k_ns_ortho (k = 836) and the product branch inside a factor of pitch 1152: the cold selection and
    the retained columns by the rule of the small cases (the long-double products of order 900 take seconds each)."""
    lp, cold, op = case_lp(name)
    M = lp.M
    tw = util.nss_chain(op, LD, M=M)
    agree(cold, tw, util.nss_chain(op, np.float64, M=M), name + " cold")
    assert cold.how == "cold"
    J = cold.J
    cols = O.NullSpace(lp, warm_J=J)
    assert cols.how == "columns"
    agree(cols, util.nss_chain(op, LD, hint_J=J, M=M), util.nss_chain(op, np.float64, hint_J=J, M=M), name + " columns")
    a, b, c = util.nss_quality(op, tw["Zt"], tw["GI"])
    print("%s: k %d  |A_EF Zt'| %.1e  |Zt Zt' - I| %.1e  |GI - A_I Zt'| %.1e" % (name, tw["k"], a, b, c))
    assert a <= 1e-13


@pytest.mark.parametrize("name", ["small", "wide"])
def test_ortho_rows_twin(name):
    """util.tw_nss_ortho_rows, the statement bound (a) holds k_ns_ortho to (k = 836 on the wide case): a float64 forward substitution of the
    oracle's own second-pass system - each row from the rows before it, the sum in BLAS's order - is within the bound with constant
    1; one entry moved by 1e-13 relative is not."""
    from scipy.linalg import solve_triangular
    lp, cold, op = case_lp(name)
    k = cold.k
    rng = np.random.default_rng(8)
    G = cold.Zt * (1.0 + 1e-3 * rng.standard_normal(cold.Zt.shape))
    S = np.tril(G @ G.T)
    L = np.asarray(util.nss_chol_guard(S, np.ones(k), util.NS_WARM_THR, np.float64))
    dev = np.zeros(G.shape)
    for r in range(k):      # (LAPACK's trsm multiplies by reciprocals of the pivots: a rounding more than the statement has)
        dev[r] = (G[r] - L[r, :r] @ dev[:r]) / L[r, r]
    assert np.abs(dev - solve_triangular(L, G, lower=True)).max() <= 1e-12
    val, mag, K = util.tw_nss_ortho_rows(L, G, dev)
    ratio = util.bound_ratio(dev, val, mag, K)
    print("%s k %d: float64 substitution against the twin, ratio %.3e" % (name, k, ratio))
    assert 0 < ratio <= 1.0
    bad = dev.copy()
    c, j = k - 1, int(np.argmax(np.abs(dev[k - 1])))
    bad[c, j] *= 1.0 + 1e-13
    val, mag, K = util.tw_nss_ortho_rows(L, G, bad)
    assert util.bound_ratio(bad, val, mag, K) > 1.0
    # ... and it is the long-double substitution itself when the rows before are exact
    ref = util.nss_ortho(L, G)
    val, _, _ = util.tw_nss_ortho_rows(L, G, np.asarray(ref, np.float64))
    assert float(np.abs(val - ref).max()) <= 1e-14 * float(np.abs(ref).max())


def test_refusals():
    """A column list with a repeated column is no basis (a dropped pivot of P[J, J]): the chain goes cold and finds the oracle's J; two equal
    rows in the carried basis are refused by the Gram factor at NS_ZWARM_THR."""
    lp, cold, op = case_lp("small")
    J = cold.J.copy()
    J[3] = J[2]
    nsp = O.NullSpace(lp, warm_J=J)
    tw = util.nss_chain(op, LD, hint_J=J, M=lp.M)
    assert nsp.how == "cold" == tw["path"] and np.array_equal(tw["J"], cold.J) and np.array_equal(nsp.J, cold.J)
    Zw = cold.Zt.copy()
    Zw[4] = Zw[9]
    nsp = O.NullSpace(lp, warm_Z=Zw)
    tw = util.nss_chain(op, LD, warm_Z=Zw, M=lp.M)
    assert nsp.how == "cold" == tw["path"]


def test_blocked_factor_is_a_factor():
    """util.nss_chol_blocked, the float64 restatement of the device's factorisation that measures the allowance of convention (c): on a
    matrix of two 64-wide steps and a remainder, with one dependent row, it drops the same pivot as the column loop and agrees with the
    long-double factor to the conditioning of the matrix; its block inverse is the inverse of its diagonal block."""
    rng = np.random.default_rng(5)
    B = rng.standard_normal((150, 170))
    B[70] = B[3] - 2.0 * B[40]
    S, one = np.tril(B @ B.T), np.ones(150)
    ref = util.nss_chol_guard(S, np.diag(S), 1e-10)
    Lb = util.nss_chol_blocked(S, np.diag(S), 1e-10)
    big = np.diag(Lb) >= util.NS_BIG
    assert big.sum() == 1 and big[70] and np.array_equal(big, np.asarray(np.diag(ref), np.float64) >= util.NS_BIG)
    keep = ~big
    err = float(np.abs(Lb.astype(LD) - ref)[np.ix_(keep, keep)].max() / np.abs(ref[np.ix_(keep, keep)]).max())
    print("blocked factor against long double: %.2e" % err)
    assert 0 < err <= 1e-11
    assert not np.triu(Lb, 1).any()
    L, W = util._nss_potrf64(S[:64, :64], np.diag(S)[:64], 1e-10)
    assert np.abs(W @ L - np.eye(64)).max() <= 1e-12 and np.array_equal(L, Lb[:64, :64])


def test_case_properties():
    """What tests/test_ns_setup_gpu.py assumes of its cases: the dimensions, the dropped pivot, both branches of ns_ortho."""
    want = {"small": (30, 0), "small-fixed": (24, 0), "small-dep": (31, 1), "k1": (1, 0), "one-ineq": (1, 0), "dense": (35, 0)}
    for name, (k, dropped) in want.items():
        lp, cold, op = case_lp(name)
        assert (cold.k, int((np.diag(cold.L0) >= util.NS_BIG).sum())) == (k, dropped), name
        assert len(cold.E) >= 64 and op.n - len(cold.E) <= 0.3 * lp.M and op.n <= (lp.M + 15) // 16 * 16, name
    assert case_lp("one-ineq")[2].nI == 1
    lp, cold, op = case_lp("wide")
    assert cold.k == 836 and util.nss_kcap(836) == 1152 and util.nss_wb(1152) == 512
    lp, cold, op = case_lp("wide-fixed")
    assert 1 <= cold.k <= 512
    lp, cold, op = case_lp("banded")
    assert cold.k == 100 and 0 < cold.band * 2 < len(cold.E) and op.n - len(cold.E) <= 0.3 * lp.M
