"""The stage twins of tests/kkt_twins.py without a GPU: chained into steps 3 to 6 they reproduce the host twins and the dense reference of
the KKT solve and of the trust-region step; the face and trial twins reproduce eqp.lp_working_set and eqp.fraction_to_box; and every random
case of tests/test_kkt_stages_gpu.py (made here, with fixed seeds and sizes) keeps each decision further from its threshold than the decision's
own rounding bound - a condition on the inputs, asserted for all of them: nothing is skipped or filtered."""
import numpy as np
import pytest

from activesetmethods_amd import eqp, sensitivity
from tests import kkt_twins as T
from tests import util
from tests.test_kkt_step_cpu import FACTORS, KKT_STEP_BAR, full_norm, ladder_case, negative_curvature_instance, step_errors
from tests.test_sensitivity_cpu import kkt_instance, rel_err

INF = float("inf")
KK = T.KK
VBLOCKS = "b_ru dx0 d r p hraw hp tt dx hdx q jtl dz g".split()
RBLOCKS = "rww tw spare dlw adx".split()
# (n, cols): ldn -> 1, 1, 1, 2, 9 workgroups per column and 65 clamped to 64 with a partly filled second stride; 1, 3 and 64 columns
SHAPES = [(1, 1), (33, 3), (255, 64), (257, 1), (257, 3), (257, 64), (2049, 3), (16417, 1), (16417, 3), (16417, 64)]
SHAPE_IDS = ["n%d-c%d" % s for s in SHAPES]
ROWS = (0, 1, 31, 33, 64, 65)          # working rows; capW = nW + 2 puts nW < nWp < ldT (but at 0: no rows at all) and nW < nWg


def base_state(n, M, nW, capW, cols, seed):
    """A state with every output buffer at the sentinel: the mask (about one variable in five on a bound, zero beyond n), the working rows
    (distinct, not ascending), their positions, radii, a scalar block of plain numbers, counters at 0."""
    rng = np.random.default_rng(seed)
    d = T.dims(n, M, nW, capW, cols)
    st = dict(dims=d, seed=seed)
    for nm in VBLOCKS:
        st[nm] = np.full(T.KKM_CW * d["ldn"], util.SENTINEL)
    for nm in RBLOCKS:
        st[nm] = np.full(T.KKM_CW * d["ldT"], util.SENTINEL)
    st["dlf"] = np.full(T.KKM_CW * d["Mp"], util.SENTINEL)
    mask = np.zeros(d["ldn"])
    mask[:n] = rng.random(n) > 0.2
    if n > 2:
        mask[0], mask[n - 1] = 1.0, 0.0
    st["mask"] = mask
    st["rad"] = 1.0 + rng.random(T.KKM_CW)
    st["scal"] = np.concatenate([1.0 + rng.random(T.WORD), [util.SENTINEL], np.full(15, util.SENTINEL)])
    st["part"] = np.full(T.KKM_CW * T.KK_MAXWG * T.KK_SLOTS, util.SENTINEL)
    st["cnt"] = np.zeros(T.KKM_CW + 1, np.uint32)
    st["act"] = rng.integers(0, 2, T.KKM_CW).astype(np.uint32)
    st["hscal"], st["hseq"] = np.array([util.SENTINEL]), np.array([777], np.uint32)
    wrow = np.full(d["Mp"], util.ISENT, np.int32)
    wrow[:nW] = rng.permutation(M)[:nW]
    wpos = np.full(d["Mp"], util.ISENT, np.int32)
    wpos[:M] = -1
    wpos[wrow[:nW]] = np.arange(nW)
    st["wrow"], st["wpos"] = wrow, wpos
    st["rows"] = rng.integers(0, max(M, 1), T.KKM_CW).astype(np.int32)
    st["counts"] = np.full(4, util.ISENT, np.int32)
    S = T.scal2d(st)
    S[:, KK["STOP"]] = 0.0
    S[:, KK["BND"]] = 0.0
    S[:, KK["ITERS"]] = rng.integers(0, 9, T.KKM_CW)
    return st, rng


def fill(st, rng, names, scale=1.0):
    """Random numbers in the first `cols` rows of the named blocks (zero beyond n in blocks over the variables, as the solver keeps them)."""
    d = st["dims"]
    for nm in names:
        ld = d["ldn"] if nm in VBLOCKS else d["ldT"]
        live = d["n"] if nm in VBLOCKS else d["nW"]
        b = st[nm].reshape(T.KKM_CW, ld)
        b[:d["cols"], :] = 0.0
        b[:d["cols"], :live] = scale * rng.standard_normal((d["cols"], live))


def freeze(st, rng):
    """With more than one column: column 1 frozen by convergence, and with more than 3 every seventh column by the curvature stop."""
    S, cols = T.scal2d(st), st["dims"]["cols"]
    if cols > 1:
        S[1, KK["STOP"]] = 1.0
        st["act"][1] = 0
    if cols > 3:
        S[6:cols:7, KK["STOP"]] = 2.0
        st["act"][6:cols:7] = 0
    return [c for c in range(cols) if S[c, KK["STOP"]] != 0.0]


# ---- the random cases of the kernels that decide: made here, run on the device by tests/test_kkt_stages_gpu.py
def normal_case(n, cols, seed=11):
    """Columns in turn: a radius that cuts the normal step to 0.3 of its length, one three times as long as needed, an infinite one."""
    st, rng = base_state(n, 4, 0, 1, cols, seed)
    fill(st, rng, ["dx0"])
    share = 0.8
    for c in range(cols):
        nn = float(np.linalg.norm(st["dx0"].reshape(T.KKM_CW, -1)[c]))
        st["rad"][c] = (0.3 * nn / share if nn > 0 else 1.0, 3.0 * max(nn, 1.0) / share, INF)[c % 3]
    return st, share


def curv_case(n, cols, trust, seed=12):
    """hp_raw = D p + noise with D in [2, 9] (p'Hp > 0 by a wide margin) but -D p in every fifth column (p'Hp < 0); Dt^2 in turn far outside
    the trial point, between d'd and the trial norm (boundary on positive curvature), and infinite.  Frozen columns as freeze() sets them."""
    st, rng = base_state(n, 4, 0, 1, cols, seed + int(trust))
    fill(st, rng, ["p", "hraw", "d"])
    d = st["dims"]
    P, HR, D = (st[nm].reshape(T.KKM_CW, -1) for nm in ("p", "hraw", "d"))
    S = T.scal2d(st)
    D[:cols] *= 0.25
    for c in range(cols):
        diag = 2.0 + 7.0 * rng.random(d["ldn"])
        HR[c] = (-1.0 if c % 5 == 4 else 1.0) * diag * P[c] + 0.01 * HR[c]
        HR[c, d["n"]:] = 0.0
        free = st["mask"] != 0.0
        php = float(P[c, free] @ HR[c, free])
        S[c, KK["RG"]] = abs(php) * (0.5 + rng.random())
        dd, dp, pp = float(D[c] @ D[c]), float(D[c] @ P[c]), float(P[c] @ P[c])
        alpha = S[c, KK["RG"]] / php if php > 0 else 1.0
        trial = dd + 2 * alpha * dp + alpha * alpha * pp
        S[c, KK["DT2"]] = (4.0 * max(trial, dd) + 1.0, 0.5 * (dd + max(trial, 1.5 * dd + 1e-3)), INF)[c % 3]
    freeze(st, rng)
    return st


def dir_case(n, cols, init, tr, seed=13):
    """||g|| against rtol ||g0|| at 10 (go on) and at 0.1 (converged) in alternate columns; tr: a boundary code in every third column."""
    st, rng = base_state(n, 4, 0, 1, cols, seed + 2 * int(init) + int(tr))
    fill(st, rng, ["r"])
    S, R = T.scal2d(st), st["r"].reshape(T.KKM_CW, -1)
    rtol = 1e-3
    for c in range(cols):
        g = float(np.linalg.norm(R[c]))
        S[c, KK["R0"]] = (g if g > 0 else 1.0) / rtol * (0.1 if c % 2 == 0 else 10.0)
        if tr and c % 3 == 2:
            S[c, KK["BND"]] = 1.0 + (c % 2)
    if init:
        if cols > 2:
            R[2] = 0.0           # g0 = 0: stops at once
    else:
        freeze(st, rng)
    return st, rtol


def decisions_of_every_random_case():
    for n, cols in SHAPES:
        st, share = normal_case(n, cols)
        yield "normal n%d c%d" % (n, cols), T.tw_normal(st, "dx0", share)[1]
        for trust in (False, True):
            yield "cg_curv n%d c%d tr%d" % (n, cols, trust), T.tw_cg_curv(curv_case(n, cols, trust), "p", "hraw", "d", "hp", trust)[1]
        for init, tr in ((1, 0), (0, 0), (0, 1)):
            st, rtol = dir_case(n, cols, init, tr)
            yield "cg_dir n%d c%d init%d tr%d" % (n, cols, init, tr), T.tw_cg_dir(st, "r", init, rtol, 5, tr)[1]


def test_every_random_case_is_clear_of_its_thresholds():
    """No skip, no filter: every decision of every random case is further from its threshold than its rounding bound."""
    count, tightest = 0, INF
    for name, dec in decisions_of_every_random_case():
        for what, dist, bound in dec:
            count += 1
            assert np.isfinite(dist) and abs(dist) > bound, (name, what, dist, bound)
            tightest = min(tightest, abs(dist) / bound if bound > 0 else INF)
    print("%d decisions, the tightest at %.3g times its rounding bound" % (count, tightest))
    assert count > 900


def test_the_random_cases_cover_every_branch():
    seen = set()
    for n, cols in SHAPES:
        st = curv_case(n, cols, True)
        outs, _ = T.tw_cg_curv(st, "p", "hraw", "d", "hp", True)
        for o in outs:
            if o.buf == "scal" and o.err is None:
                seen.add(("bnd" if o.idx[0] % T.KKM_SCAL == KK["BND"] else "stop", float(o.val[0])))
        st = curv_case(n, cols, False)
        seen |= {("stop-plain", float(o.val[0])) for o in T.tw_cg_curv(st, "p", "hraw", "d", "hp", False)[0] if o.buf == "scal" and o.err is None}
    assert seen >= {("bnd", 1.0), ("bnd", 2.0), ("stop", 2.0), ("stop-plain", 2.0)}, seen


# ---- the chained twins against the host twins and the dense reference
def _hj(inst):
    fm, x, lam = inst[:3]
    return sensitivity.lagrangian_hessian(fm, x, lam), sensitivity.dense_jacobian(fm, x)


def _check_decisions(dec, name):
    for what, dist, bound in dec:
        if "||g||" in what and abs(dist) <= 1e3 * bound:
            continue          # (a residual that vanishes outright against rtol ||g0||: checked by the iteration counts below)
        assert abs(dist) > bound, (name, what, dist, bound)


@pytest.mark.parametrize("which", ["n96_B10_W65", "curvature"])
def test_chained_twins_reproduce_the_kkt_solve(which):
    inst = kkt_instance(96, 10, 65) if which == "n96_B10_W65" else negative_curvature_instance()
    H, J = _hj(inst)
    (dx, dlam, dz, info), = T.chain_columns(H, J, inst[3], inst[4], inst[5][None, :], inst[6][None, :])[0]
    px, pl, pz, pinfo = sensitivity.kkt_pcg(*inst)
    assert (info["status"], info["cg_iters"]) == (pinfo["status"], pinfo["cg_iters"]) and info["stop"] == {0: 1, 2: 2}[pinfo["status"]]
    errs = [rel_err(dx, px), rel_err(dlam, pl), rel_err(dz, pz)]
    print(which, "chained twins against kkt_pcg:", errs)
    assert max(errs) <= KKT_STEP_BAR
    if pinfo["status"] == 0:
        rx, rl, rz = sensitivity.kkt_reference(*inst)
        assert max(rel_err(dx, rx), rel_err(dlam, rl), rel_err(dz, rz)) <= KKT_STEP_BAR


def _step_columns(inst, RU, RW, radii, name):
    H, J = _hj(inst)
    res, dec = T.chain_columns(H, J, inst[3], inst[4], RU, RW, radii=radii)
    _check_decisions(dec, name)
    worst = 0.0
    for c, got in enumerate(res):
        tw = eqp.kkt_step_pcg(*inst[:5], RU[c], RW[c], radii[c])
        ref = eqp.kkt_step_reference(*inst[:5], RU[c], RW[c], radii[c])
        gi = got[3]
        for other in (tw[3], ref[3]):
            assert (gi["boundary"], gi["cg_iters"], gi["status"]) == (other["boundary"], other["cg_iters"], other["status"]), (name, c, gi, other)
        assert gi["stop"] == (2 if gi["status"] == 2 else 1)
        worst = max([worst] + step_errors(got, tw) + step_errors(got, ref))
    print(name, "chained twins against kkt_step_pcg and kkt_step_reference: %.3e" % worst)
    assert worst <= KKT_STEP_BAR


def test_chained_twins_reproduce_the_trust_region_step():
    for name, inst in (("n96_B10_W65", kkt_instance(96, 10, 65)), ("curvature", negative_curvature_instance())):
        full = full_norm(inst)
        k = len(FACTORS)
        _step_columns(inst, np.tile(inst[5], (k, 1)), np.tile(inst[6], (k, 1)), np.array([f * full for f in FACTORS]), name)


def test_chained_twins_reproduce_the_ladder():
    inst, RU, RW, radii = ladder_case()
    _step_columns(inst, RU, RW, radii, "ladder")


# ---- the face and the trial step
class _Problem:
    pass


def face_problem(n, m, seed=5):
    """Rows in turn: an equality, a range row (twin), a row with g_L = -inf, a lower-only row; variables with infinite bounds on either side
    and a nonzero LP state, at a bound, near it and away from it."""
    rng = np.random.default_rng(seed)
    P = _Problem()
    P.n, P.m = n, m
    kind = np.arange(m) % 4
    lo = rng.integers(-4, 4, m).astype(float)
    P.g_L = np.where(kind == 2, -INF, lo)
    P.g_U = np.where(kind == 0, lo, np.where(kind == 3, INF, lo + 1.0 + rng.integers(0, 3, m)))
    P.x_L = np.where(np.arange(n) % 5 == 3, -INF, -1.0 - (np.arange(n) % 3))
    P.x_U = np.where(np.arange(n) % 7 == 2, INF, 2.0 + (np.arange(n) % 2))
    adj = np.flatnonzero(np.isfinite(P.g_L) & np.isfinite(P.g_U) & (P.g_L != P.g_U))
    lp_rows = rng.integers(0, 2, m + len(adj)).astype(np.int32)
    lp_bnd = rng.integers(-1, 2, n).astype(np.int32)
    tol = 2.0 ** -20
    where = np.arange(n) % 4
    off = np.where(where == 0, 0.0, np.where(where == 1, 0.5 * tol, np.where(where == 2, 3.0 * tol, 0.25)))
    x = np.where(lp_bnd == -1, np.where(np.isfinite(P.x_L), P.x_L, -3.0) + off, np.where(lp_bnd == 1, np.where(np.isfinite(P.x_U), P.x_U, 5.0) - off, 0.125))
    E = rng.standard_normal(m)
    twin = np.full(m, -1, np.int32)
    twin[adj] = np.arange(len(adj))
    return P, x, E, lp_rows, lp_bnd, twin, tol


def face_state(n, m, seed=5):
    P, x, E, lp_rows, lp_bnd, twin, tol = face_problem(n, m, seed)
    st, _ = base_state(8, 4, 0, 1, 1, seed)
    st.update(E=E, g_L=P.g_L.copy(), g_U=P.g_U.copy(), x=x, x_L=P.x_L.copy(), x_U=P.x_U.copy(), rw=np.full(m, util.SENTINEL), lp_rows=lp_rows, lp_bnd=lp_bnd, twin=twin,
              f_rows=np.full(m, util.ISENT, np.int32), f_bnd=np.full(n, util.ISENT, np.int32), f_side=np.full(m, util.ISENT, np.int32),
              f_counts=np.full(2, util.ISENT, np.int32))
    return st, P, tol


FACE_NAMES = "E g_L g_U x x_L x_U rw lp_rows lp_bnd twin f_rows f_bnd f_side f_counts".split()
FACE_SIZES = [(5, 12), (12, 5), (7, 0), (300, 257), (16417, 40), (40, 16417)]


@pytest.mark.parametrize("n,m", FACE_SIZES)
def test_face_twin_reproduces_lp_working_set(n, m):
    st, P, tol = face_state(n, m)
    res = {o.buf: o for o in T.tw_eqp_face(st, FACE_NAMES, n, m, tol) if o.buf != "part"}
    rs, bs, at = eqp.lp_working_set(P, st["x"], (st["lp_rows"], st["lp_bnd"]), tol)
    assert np.array_equal(res["f_rows"].val, rs) and np.array_equal(res["f_bnd"].val, bs)
    assert np.array_equal(res["rw"].val, np.where(rs == 1, st["E"] - at, 0.0))
    assert list(res["f_counts"].val) == [rs.sum(), (bs == 0).sum()]
    assert set(bs) == {-1, 0, 1} or n < 12


def trial_state(n, kind, seed=6):
    """kind: free (no component limits the step, t = 1) | on_bound (a component on its bound, the step pointing outwards: t = 0) | outside (a
    point outside the box: t clipped to 0) | zero (dx = 0) | cut (0 < t < 1, infinite bounds among the others)."""
    rng = np.random.default_rng(seed + n)
    st, _ = base_state(8, 4, 0, 1, 1, seed)
    x = rng.integers(-3, 4, n) / 4.0
    x_L, x_U = np.full(n, -2.0), np.full(n, 2.0)
    x_L[::3], x_U[1::3] = -INF, INF
    dx = rng.integers(-8, 9, n) / 16.0
    if kind == "free":
        dx = dx / 16.0
    if kind == "on_bound":
        x[n - 1], dx[n - 1] = 2.0, 0.5
        x_U[n - 1] = 2.0
    if kind == "outside":
        x[n // 2], dx[n // 2], x_U[n // 2] = 3.0, 0.25, 2.0
    if kind == "zero":
        dx[:] = 0.0
    if kind == "cut":
        dx[n // 2], x[n // 2], x_L[n // 2] = -4.0, 0.0, -1.0
    st.update(t_dx=dx, t_x=x, t_xL=x_L, t_xU=x_U, t_d=np.full(n, util.SENTINEL), t_out=np.full(4, util.SENTINEL))
    return st


TRIAL_NAMES = "t_dx t_x t_xL t_xU t_d t_out".split()
TRIAL_KINDS = {"free": 1.0, "on_bound": 0.0, "outside": 0.0, "zero": 1.0, "cut": 0.25}


@pytest.mark.parametrize("kind", sorted(TRIAL_KINDS))
@pytest.mark.parametrize("n", [1, 257, 16417])
def test_trial_twin_reproduces_fraction_to_box(n, kind):
    st = trial_state(n, kind)
    outs, t = T.tw_eqp_trial(st, TRIAL_NAMES, n)
    assert t == eqp.fraction_to_box(st["t_dx"], st["t_xL"] - st["t_x"], st["t_xU"] - st["t_x"])
    if n > 1:
        assert t == TRIAL_KINDS[kind]
    res = {(o.buf, int(o.idx[0])): o for o in outs if o.buf == "t_out"}
    d = t * st["t_dx"]
    assert float(res[("t_out", 3)].val[0]) == np.count_nonzero(d) and float(res[("t_out", 2)].val[0]) == (np.abs(d).max())
    assert abs(float(res[("t_out", 1)].val[0]) - np.linalg.norm(d)) <= 1e-14 * max(1.0, np.linalg.norm(d))
    if kind in ("on_bound", "outside", "zero"):
        assert np.count_nonzero(d) == 0
