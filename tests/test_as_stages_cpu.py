"""The NumPy twins of the active-set and optimal-face kernels (tests/util.py) against the oracle (oracle/lp_solver.py), the classes of their
decisions and the census of their branches - everything the GPU file (tests/test_as_stages_gpu.py) relies on, checked without a GPU.

The oracle works on a dense matrix; the kernels take the products with the matrix as inputs.  The oracle therefore gets a stand-in matrix whose
products are the state's own t and tN, so both sides decide on the same numbers.  Parts of the oracle that solve inside the function
(face_dual, _face_primal_anchored) cannot be fed that way: their rules - the sign repair, the tie order rows < slacks < lower < upper, lowest
index - are asserted directly on planted states."""
import numpy as np
import pytest

from oracle import lp_solver as O
from tests import util

AC, AS = util.AC, util.AS
CASES = [(c, rp) for c in util.AS_CASES for rp in (0, 1)]
CASE_IDS = ["n%d-M%d-ns%d-%s" % (c + (("natural", "rperm")[rp],)) for c, rp in CASES]
SQ = 8.0


class _Products:
    """Stand-in for lp.A: A @ p is the state's t, A.T @ y its tN."""

    def __init__(self, fwd, bwd):
        self.fwd, self.bwd = fwd, bwd

    def __matmul__(self, x):
        return self.fwd.copy()

    @property
    def T(self):
        return _Products(self.bwd, self.fwd)


def state(case, rp):
    n, M, ns = case
    st = util.as_state(100 + n % 97 + rp, n, M, ns, SQ)
    st["q"][0] = SQ                                    # the oracle's scale: max(1, |q|, |w|)
    st["s"] = st["slo"].copy()                         # as k_as_setup (and eqp) leave the slacks before the tail computes the basic ones
    assert max(np.abs(st["q"]).max(), np.abs(st["w"]).max(initial=0.0)) == SQ
    return st


def oracle_lp(st, t=None, tN=None, rp=0):
    lp = O.LP.__new__(O.LP)
    lp.n, lp.M, lp.ns = st["n"], st["M"], st["ns"]
    lp.A = _Products(st["t"] if t is None else t, st["tN"] if tN is None else tN)
    for nm in "q r lb ub w slo scoef".split():
        setattr(lp, nm, st[nm])
    lp.rtype, lp.srow = st["rtype"].astype(np.int64), st["srow"].astype(np.int64)
    lp.row_pos = None
    if rp:
        lp.row_pos = np.empty(lp.M, np.int64)
        lp.row_pos[st["rperm"]] = np.arange(lp.M)
    return lp


def all_twins(st, rp, bk):
    """Every twin once, as the GPU file runs them; returns the results by name."""
    n, M, ns = st["n"], st["M"], st["ns"]
    out = {}
    out["identify"] = util.tw_as_identify(st, 3, bk)
    util.tw_as_clip0(st, None, "zero", bk); util.tw_as_clip0(st, "ip.p", "pref", bk)
    out["setup"] = util.tw_as_setup(st, 0, None, rp, bk)
    util.tw_as_setup(st, 4, "pref", rp, bk)
    util.tw_as_rhs(st, None, bk); util.tw_as_rhs(st, "ip.y", bk)
    util.tw_as_scatter_h(st, "u", 1, bk); util.tw_as_scatter_h(st, "yH", 0, bk)
    util.tw_as_merge(st, 0, bk); util.tw_as_merge(st, 1, bk)
    out["finish"] = util.tw_as_finish(st, 0, 1, 2, 1, util.TOL_P, util.TOL_D, bk)
    util.tw_as_finish(st, 0, 1, 2, 0, util.TOL_P, util.TOL_D, bk)
    util.tw_face_primal_finish(st, 4, 3, util.TOL_P, util.FACE_TOL_M, 0, bk)
    util.tw_face_primal_finish(st, 4, 3, util.TOL_P, util.FACE_TOL_M, 1, bk)
    sf = dict(st)
    sf["p"] = np.clip(st["p"], st["lb"], st["ub"])
    sf["t"] = st["r"] + st["rtype"] * 0.5 - st["sl"]
    sf["S4.sst"] = np.zeros(ns, np.int32)
    sf["ksoft"] = np.full(M, -1, np.int32)
    util.tw_face_primal_finish(sf, 4, 3, util.TOL_P, util.FACE_TOL_M, 0, bk)
    util.tw_face_primal_finish(sf, 4, 3, util.TOL_P, 1e9, 0, bk)                   # nothing to release: unchanged
    out["dual_finish"] = util.tw_face_dual_finish(st, 5, util.FACE_TOL_M, bk)
    util.tw_face_dual_finish(st, 5, 1e9, bk)
    out["kkt"] = util.tw_face_kkt(st, 5, bk)
    util.tw_face_ns_step(st, 4, util.TOL_P, bk); util.tw_face_ns_step(sf, 4, util.TOL_P, bk)
    for fam, e in ((0, M - 1), (1, ns - 1), (2, n - 1), (3, 0)):
        if e >= 0:
            util.tw_face_ns_unmark(st, 4, fam, e, bk)
            if M:
                util.tw_face_ns_col(st, np.ones(n), fam, e, "pf", "actf", bk)
    return out


@pytest.mark.parametrize("case,rp", CASES, ids=CASE_IDS)
def test_twins_match_oracle(case, rp):
    st = state(case, rp)
    n, M, ns = case
    bk = util.AsBook()
    tw = all_twins(st, rp, bk)
    assert bk.cls["between"] == 0, bk.cls
    lp = oracle_lp(st, rp=rp)
    # identify
    ip = {k[3:]: v for k, v in st.items() if k.startswith("ip.")}
    rowst, bst, sst = O.identify(lp, ip)
    ex = tw["identify"][0]
    assert np.array_equal(rowst, ex["S3.rowst"]) and np.array_equal(bst, ex["S3.bst"]) and np.array_equal(sst, ex["S3.sst"])
    # soft rows, ordered hard rows and free columns of eqp
    ex = tw["setup"][0]
    s0 = tuple(a.astype(np.int64) for a in util._sets(st, 0))
    soft, ysoft, ksoft = O._soft_rows(lp, s0[2])
    assert np.array_equal(ksoft, ex["ksoft"]) and np.array_equal(ysoft, ex["y"])
    H = O.ordered_rows(lp, np.nonzero((s0[0] == 1) & ~soft)[0])
    assert ex["cnt.NH"] == len(H) and np.array_equal(ex["Hidx"][:len(H)], H)
    F = np.nonzero(s0[1] == 0)[0]
    assert ex["cnt.NF"] == len(F) and np.array_equal(ex["Fidx"][:len(F)], F) and ex["cnt.ANYSOFT"] == int(soft.any())
    inv = np.full(M, -1); inv[H] = np.arange(len(H))
    assert np.array_equal(ex["hpos"], inv)
    # kkt_measures + correct against the k_as_finish twin (the slack values are the twin's: the oracle computes them in eqp)
    ex, bnd = tw["finish"]
    s = bnd["s"][0].astype(np.float64) if ns else np.zeros(0)
    pr, du = O.kkt_measures(lp, st["p"], s, st["y"], s0)
    (nrow, nb, nss), nchg = O.correct(lp, st["p"], s, st["y"], s0)
    assert np.array_equal(nrow, ex["S1.rowst"]) and np.array_equal(nb, ex["S1.bst"]) and np.array_equal(nss, ex["S1.sst"]) and nchg == ex["cnt.NCHG"]
    rp_, rd_ = util.bound_ratio(pr, *bnd["scal.PR"]), util.bound_ratio(du, *bnd["scal.DU"])
    assert rp_ <= 1.0 and rd_ <= 1.0, (rp_, rd_)
    # dual measure of face_polish's tail, on a state whose z is q - tN as the oracle forms it (one subtraction: exact on both sides)
    sz = dict(st, z=st["q"] - st["tN"])
    ex, bnd = util.tw_face_kkt(sz, 5, util.AsBook())
    s5 = tuple(a.astype(np.int64) for a in util._sets(st, 5))
    _, du = O.kkt_measures(lp, st["p"], st["s"], st["y"], s5)
    rk_ = util.bound_ratio(du, *bnd["scal.DU"])
    assert rk_ <= 1.0, rk_
    print("%s: twin vs oracle in units of the bound: PR %.3f DU %.3f face DU %.3f; classes %s" % (case, rp_, rd_, rk_, bk.cls))


def test_census_and_classes():
    """Every branch of every kernel's decision tree is taken somewhere over the cases, the planted ties and the equal-ratio states; no decision
    falls between the classes clear and tie."""
    bk = util.AsBook()
    for case, rp in CASES:
        all_twins(state(case, rp), rp, bk)
    for fams in ([0, 1], [2, 3], [1], [3, 2, 1, 0]):
        st, _ = util.as_ratio_tie_state(fams, (63, 64))
        util.tw_face_ns_step(st, 4, util.TIE_TOL_P, bk)
    zero = [(k, b) for k, v in bk.census.items() for b, c in v.items() if c == 0]
    assert not zero, zero
    assert bk.cls["between"] == 0 and bk.cls["clear"] > 0, bk.cls


TIES = [(k, w) for k, ws in util.AS_TIES.items() for w in ws]
# what the operator of each comparison dictates exactly on the threshold: every strict one is not taken; the slack test of identify is >=
TAKEN = {("identify", "slack"): True, ("identify", "forced"): True}


@pytest.mark.parametrize("kernel,which", TIES, ids=["%s-%s" % t for t in TIES])
def test_planted_ties_decide_by_operator(kernel, which):
    st, I = util.as_tie_state(kernel, which)
    bk = util.AsBook()
    tp, td, tm = util.TIE_TOL_P, util.TIE_TOL_D, util.TIE_TOL_M
    taken = TAKEN.get((kernel, which), False)
    I = np.asarray(I)
    if kernel == "identify":
        ex, _ = util.tw_as_identify(st, 3, bk)
        nm, val = {"lower": ("bst", -1), "upper": ("bst", 1), "slack": ("sst", 1), "row": ("rowst", 1), "forced": ("rowst", 1)}[which]
        got = ex["S3." + nm][I] == val
    elif kernel == "finish":
        ex, _ = util.tw_as_finish(st, 0, 1, 2, 1, tp, td, bk)
        old = {"row": st["S0.rowst"], "rel": st["S0.bst"], "fix": st["S0.bst"], "sla": st["S0.sst"]}[which[:3]][I]
        new = {"row": ex["S1.rowst"], "rel": ex["S1.bst"], "fix": ex["S1.bst"], "sla": ex["S1.sst"]}[which[:3]][I]
        got = new != old
    elif kernel == "dual_finish":
        ex, _ = util.tw_face_dual_finish(st, 5, tm, bk)
        nm = {"col": "bst", "row": "rowst", "sla": "sst"}[which[:3]]
        got = ex["S5." + nm][I] != st["S5." + nm][I]
    elif kernel == "primal_finish":
        if which.startswith("rel"):
            st["p"] = np.where(st["S4.bst"] == 0, np.clip(st["p"], st["lb"], st["ub"]), st["p"])
            st["t"] = st["r"] + st["rtype"] * 0.5 - st["sl"]
            st["S4.sst"][:] = 0
            st["ksoft"][:] = -1
        before = {nm: st["S4." + nm].copy() for nm in ("rowst", "bst", "sst")}
        ex, _ = util.tw_face_primal_finish(st, 4, 3, tp, tm, 0, bk)
        if which.startswith("rel"):
            assert ex["cnt.NVIOL"] == 0
        nm = "rowst" if which.endswith("row") else "bst"
        got = ex["S4." + nm][I] != before[nm][I]
    else:
        ex, _, info = util.tw_face_ns_step(st, 4, tp, bk)
        fam = {"thr_row": 0, "thr_slack": 1, "thr_lower": 2, "thr_upper": 3}[which]
        got = np.isin(I, info["cand"][fam][0]) if info["nviol"] else np.zeros(len(I), bool)
    # (the ratio test of k_face_ns_step is a float64-exact statement of its twin: it files no classes)
    assert len(I) > 0 and (kernel == "ns_step" or bk.cls["tie"] >= len(I)) and bk.cls["between"] == 0, bk.cls
    assert np.all(got == taken), (kernel, which, got)


@pytest.mark.parametrize("fams", [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3], [3, 2, 1, 0]])
def test_equal_ratios_tie_order(fams):
    """Equal minimal ratios: family order rows < slacks < lower < upper (the order of _face_primal_anchored's `best` tuple), then lowest index;
    ineligible decoys with a smaller ratio do not count."""
    for spots in ((0, 2099), (63, 64), (1023, 1024)):
        st, planted = util.as_ratio_tie_state(fams, spots)
        ex, bnd, info = util.tw_face_ns_step(st, 4, util.TIE_TOL_P, util.AsBook())
        assert info["nviol"] == len(planted) and info["alpha"] == 0.25
        assert (info["fam"], info["e"]) == min(planted)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("seed", [3, 4, 5, 6])
def test_chained_round(mode, seed):
    """setup -> rhs -> sweeps -> merge -> finish through the twins, with the products and the H-system solve in long double, against
    oracle.eqp + kkt_measures + correct on the same working set (modes 0, 1, 2 of Solver::as_solve)."""
    st0, A = util.as_chain_lp(seed)
    bk = util.AsBook()
    p_ref, y_ref = ("pref", "ip.y") if mode == 0 else (None, None)
    fin = util.as_chain(st0, A, 0, mode, p_ref, y_ref, util.as_twin_do(bk))
    err, lp, sets = util.as_chain_errors(st0, A, fin, mode, p_ref, y_ref)
    print("chained round mode %d seed %d: " % (mode, seed) + ", ".join("%s error %.2e, oracle against itself %.2e" % (k, e[0], e[1]) for k, e in err.items()))
    assert all(e[2] <= 1.0 for e in err.values()), err
    if mode != 1:
        ex, bnd = util.tw_as_finish(fin, 0, 1, 2, 0, util.TOL_P, util.TOL_D, bk)
        out = util.as_apply(fin, (ex, bnd))
        (nrow, nb, nss), nchg = O.correct(lp, fin["p"], out["s"], fin["y"], sets)
        assert np.array_equal(nrow, ex["S1.rowst"]) and np.array_equal(nb, ex["S1.bst"]) and np.array_equal(nss, ex["S1.sst"]) and nchg == ex["cnt.NCHG"]
        pr, du = O.kkt_measures(lp, fin["p"], out["s"], fin["y"], sets)
        # the oracle forms A p and A'y itself, in float64: its own products carry gamma_n |A||p| on top of the kernel's statement
        v, m, k = bnd["scal.PR"]
        extra = (np.abs(A) @ np.abs(fin["p"])).max()
        assert util.bound_ratio(pr, v, m + extra, k + st0["n"]) <= 1.0
        v, m, k = bnd["scal.DU"]
        extra = (np.abs(A.T) @ np.abs(fin["y"])).max() / st0["scale_q"]
        assert util.bound_ratio(du, v, m + extra, k + st0["M"]) <= 1.0
    assert bk.cls["between"] == 0


FACE_SEEDS = {3: 0, 4: 0, 5: 0, 6: 2, 28: 2, 55: 3, 90: 3, 210: 1}      # seed: the family of the oracle's blocking inequality (all four occur)


@pytest.mark.parametrize("seed", sorted(FACE_SEEDS))
def test_face_rounds_match_oracle(seed, monkeypatch):
    """One round of face_dual (sign repair), one bulk round of face_primal (grow / release) and one step of _face_primal_anchored (blocking
    choice, anchor move) on a real dense LP: the oracle is cut to a single round and the twins are fed the oracle's own solve."""
    st, A = util.as_chain_lp(seed)
    n, M, ns = st["n"], st["M"], st["ns"]
    lp = util.as_oracle_lp(st, A)
    part = tuple(a.astype(np.int64) for a in util._sets(st, 0))
    bk = util.AsBook()
    stats = {"nfact": 0, "eqp": 0}
    ex0, _ = util.tw_as_setup(st, 0, None, 0, bk)
    base = dict(util.as_apply(st, (ex0, {})), **{"S3.%s" % k: st["S0.%s" % k] for k in ("rowst", "bst", "sst")})
    # ---- face_dual: one round
    monkeypatch.setattr(O, "FACE_BULK", 1)
    ok, y, D = O.face_dual(lp, part, dict(stats))
    sd = dict(base, y=y, tN=A.T @ y, **{"S5.%s" % k: st["S0.%s" % k] for k in ("rowst", "bst", "sst")})
    ex, _ = util.tw_face_dual_finish(sd, 5, util.FACE_TOL_M, bk)
    assert np.array_equal(ex["S5.rowst"], D[0]) and np.array_equal(ex["S5.bst"], D[1]) and np.array_equal(ex["S5.sst"], D[2])
    assert (ex["cnt.NVIOL"] == 0) == ok
    # ---- face_primal: the working set the oracle hands to its second solve is the one its first round left
    seen = []
    real = O._face_primal_solve

    def spy(lp_, W, sl, stats_):
        seen.append(tuple(a.copy() for a in W))
        out = real(lp_, W, sl, stats_)
        seen.append(out)
        return out
    monkeypatch.setattr(O, "_face_primal_solve", spy)
    monkeypatch.setattr(O, "FACE_BULK", 2)
    monkeypatch.setattr(O, "FACE_STEPS", 0)
    anchor = (np.clip(st["p"], st["lb"], st["ub"]), st["slo"] + 1.0)
    O.face_primal(lp, part, anchor, dict(stats))
    p, s, act, u, nu, hard, hres = seen[1]
    done = []
    if len(seen) >= 4 and not hres > util.TOL_P:
        done.append("primal")
        W1 = seen[2]
        sp = dict(base, p=p, t=A @ p, tN=A.T @ u, uacc=u[ex0["Hidx"][:ex0["cnt.NH"]]].tolist() + [0.0] * (M - ex0["cnt.NH"]),
                  **{"S4.%s" % k: st["S0.%s" % k] for k in ("rowst", "bst", "sst")})
        sp["uacc"] = np.asarray(sp["uacc"])
        ex, _ = util.tw_face_primal_finish(sp, 4, 3, util.TOL_P, util.FACE_TOL_M, 0, bk)
        assert np.array_equal(ex["S4.rowst"], W1[0]) and np.array_equal(ex["S4.bst"], W1[1]) and np.array_equal(ex["S4.sst"], W1[2]), seed
    # ---- _face_primal_anchored: one step
    monkeypatch.setattr(O, "_face_primal_solve", real)
    monkeypatch.setattr(O, "FACE_STEPS", 1)
    sl = st["sl"]
    okk, pa, sa, W = O._face_primal_anchored(lp, part, anchor, sl, dict(stats))
    p0, *_ = real(lp, part, sl, dict(stats))
    acta = A @ anchor[0]
    np.add.at(acta, st["srow"], st["scoef"] * anchor[1])
    sa_ = dict(base, p=p0, t=A @ p0, pa=anchor[0], sa=anchor[1], acta=acta, **{"S4.%s" % k: st["S0.%s" % k] for k in ("rowst", "bst", "sst")})
    ex, bnd, info = util.tw_face_ns_step(sa_, 4, util.TOL_P, bk)
    if info["nviol"] and ex["scal.HARDRES"] <= util.TOL_P:
        done.append("anchored fam %d" % info["fam"])
        assert np.array_equal(ex["S4.rowst"], W[0]) and np.array_equal(ex["S4.bst"], W[1]) and np.array_equal(ex["S4.sst"], W[2]), (seed, info["fam"], info["e"])
        assert util.bound_ratio(pa, *bnd["pa"]) <= 1.0 and util.bound_ratio(sa, *bnd["sa"]) <= 1.0
        # the constraint as the oracle states it: c, g = b - c'(p0 - pfix), c'c
        fam, e = info["fam"], info["e"]
        row = util.as_col_row(sa_, fam, e)
        pfix = np.where(part[1] < 0, st["lb"], np.where(part[1] > 0, st["ub"], 0.0))
        Fm = (part[1] == 0).astype(float)
        c = Fm * A[row] if row >= 0 else np.eye(n)[e]
        bc = (st["r"][row] - sl[row] - A[row] @ pfix) if row >= 0 else (st["lb"][e] if fam == 2 else st["ub"][e])
        sc_ = dict(sa_, pf=p0, actf=A @ p0)
        exc, bc_ = util.tw_face_ns_col(sc_, A[max(row, 0)], fam, e, "pf", "actf", bk)
        assert np.array_equal(exc["rd"], c)
        g = bc - c @ (p0 - pfix)
        v, m, k = bc_["scal.EQRES"]
        assert util.bound_ratio(g, v, m + np.abs(A[max(row, 0)]) @ (np.abs(p0) + np.abs(pfix)), k + 2 * n) <= 1.0
        assert util.bound_ratio(c @ c, *bc_["scal.PR"]) <= 1.0
    print("seed %d compared with the oracle: dual, %s" % (seed, ", ".join(done)))
    assert "anchored fam %d" % FACE_SEEDS[seed] in done, done          # every seed reaches the anchored comparison, in the family listed
    assert seed >= 10 or len(done) == 2, done
    assert bk.cls["between"] == 0
