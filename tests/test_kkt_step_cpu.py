"""The trust-region step on the host (include/asm_hip.h, "Trust-region step on the working set"): the NumPy twin of asm_kkt_step against
the independent dense reference of activesetmethods_amd/eqp.py on every instance and radius that this file and tests/test_kkt_step_gpu.py
use, the decision margins of the reference on all of them, the properties of a trust-region step on both, and fraction_to_box.  No GPU."""
import numpy as np
import pytest

from activesetmethods_amd import eqp, sensitivity
from tests.test_sensitivity_cpu import KKT_SHAPES, kkt_instance, rel_err
from tests.test_sensitivity_gpu import hs071_param_model
from tests.test_sensitivity_multi_cpu import multi_columns

INF = float("inf")
# kkt_step_pcg against kkt_step_reference over step_cases(), the ladder, the 66 columns and the mixed columns: the largest relative error
# that test_twin_against_the_reference measures on the host (it prints every figure; the worst is shape (200, 20, 130) at
# f = 0.6).  The device bar is 10 x this - the project's margin for the device's summation order (KKT_BAR) - and not below 1e-12.
TWIN_STEP_ERR_MEASURED = 5.1e-15
KKT_STEP_BAR = max(10.0 * TWIN_STEP_ERR_MEASURED, 1e-12)
DECISION_MARGIN = 1e-6         # every boundary and curvature decision of the reference is clear by this much, relative
# the convergence decision ||g|| <= rtol ||g0||: the residual recurrence carries a relative error of about the unit roundoff times
# cond(H) <= 10 against ||g0||, that is 1e-16 * 10 / rtol = 1e-3 of the threshold; nearer than that an iteration count could differ
CONVERGENCE_MARGIN = 1e-3
FACTORS = (0.25, 0.6, 1.5, INF)                       # radius = f * ||dx_full||_2, dx_full from kkt_reference
LADDER_SHAPE, LADDER = (96, 10, 65), (0.1, 0.25, 0.4, 0.6, 0.9, 1.2, 1.5, INF)
WIDE_SHAPE, WIDE_COLUMNS = (33, 1, 1), 66             # crosses the 64-column chunk
HS071_RADIUS, HS071_TOL, HS071_GAIN = 1.0, 1e-3, 100.0


def negative_curvature_instance():
    """The instance of test_kkt_pcg_result_statuses: one eigenvalue of about -50 on null(A)."""
    neg = np.full(8, 4.0)
    neg[2] = -50.0
    return kkt_instance(8, 0, 2, seed=3, diag=neg)


def long_normal_instance():
    """(96, 10, 65) with rw twenty times as large: the normal step alone is longer than 0.8 of the two smaller radii."""
    fm, x, lam, rs, bs, ru, rw = kkt_instance(96, 10, 65)
    return fm, x, lam, rs, bs, ru, 20.0 * rw


def full_norm(inst):
    return float(np.linalg.norm(sensitivity.kkt_reference(*inst)[0]))


def step_cases():
    """[(name, instance, radius)]: every shape of KKT_SHAPES, the negative-curvature instance and the long normal step, each at
    f * ||dx_full|| for f in FACTORS."""
    insts = [("n%d_B%d_W%d" % s, kkt_instance(*s)) for s in KKT_SHAPES]
    insts += [("curvature", negative_curvature_instance()), ("long_normal", long_normal_instance())]
    out = []
    for name, inst in insts:
        full = full_norm(inst)
        out += [("%s f=%g" % (name, f), inst, f * full) for f in FACTORS]
    return out


def ladder_case():
    """(instance, RU, RW, radii): one right-hand side of LADDER_SHAPE at the radii of LADDER."""
    inst = kkt_instance(*LADDER_SHAPE)
    full = full_norm(inst)
    k = len(LADDER)
    return inst, np.tile(inst[5], (k, 1)), np.tile(inst[6], (k, 1)), np.array([f * full for f in LADDER])


def tangent_case():
    """(instance, RU, RW, radii): LADDER_SHAPE with rw = 0 - no normal step, theta = 1 on every rung - at the radii of LADDER."""
    fm, x, lam, rs, bs, ru, rw = kkt_instance(*LADDER_SHAPE)
    inst = (fm, x, lam, rs, bs, ru, np.zeros_like(rw))
    full = full_norm(inst)
    k = len(LADDER)
    return inst, np.tile(ru, (k, 1)), np.zeros((k, fm.m)), np.array([f * full for f in LADDER])


def wide_case():
    """(instance, RU, RW, radii): WIDE_COLUMNS columns of multi_columns on WIDE_SHAPE (column 1 is all zero: g0 = 0), column c at the
    finite factor FACTORS[c % 3] of its own full step (of 1 where that is 0)."""
    inst = kkt_instance(*WIDE_SHAPE)
    RU, RW = multi_columns(inst, WIDE_COLUMNS)
    DX = sensitivity.kkt_reference_multi(*inst[:5], RU, RW)[0]
    norms = np.linalg.norm(DX, axis=1)
    radii = np.array([FACTORS[c % 3] * (norms[c] if norms[c] > 0.0 else 1.0) for c in range(WIDE_COLUMNS)])
    return inst, RU, RW, radii


def mixed_case():
    """(instance, RU, RW, radii, want): four columns on the negative-curvature instance whose outcomes differ.
    0: ru a positive eigenvector of the reduced Hessian, rw = 0 - one iteration, converged inside;  1: the instance's right-hand side at
    a quarter of its full step - the boundary on positive curvature;  2: the same at 1.5 times - the boundary along p'Hp <= 0;
    3: all zero - g0 = 0.  want: per column (boundary, status)."""
    inst = negative_curvature_instance()
    fm, x, lam, rs, bs, ru, rw = inst
    H, J = sensitivity.lagrangian_hessian(fm, x, lam), sensitivity.dense_jacobian(fm, x)
    A = J[rs == 1]
    Z = np.linalg.svd(A)[2][len(A):].T
    ev, V = np.linalg.eigh(Z.T @ H @ Z)
    assert ev[0] < 0.0 < ev[-1]
    full = full_norm(inst)
    RU = np.array([Z @ V[:, -1], ru, ru, np.zeros(fm.n)])
    RW = np.array([np.zeros(fm.m), rw, rw, np.zeros(fm.m)])
    return inst, RU, RW, np.array([10.0, 0.25 * full, 1.5 * full, 1.0]), [(0, 0), (1, 0), (2, 0), (0, 0)]


def vertex_case():
    """(instance, RU, RW, radii): the vertex shape (8, 3, 5) - no iteration - with a radius that cuts the normal step and one that does not."""
    inst = kkt_instance(8, 3, 5)
    full = full_norm(inst)
    return inst, np.tile(inst[5], (2, 1)), np.tile(inst[6], (2, 1)), np.array([0.25 * full, 1.5 * full])


def all_columns():
    """[(name, instance, ru, rw, radius)]: every column that either file solves on constructed QPs."""
    out = [(name, inst, inst[5], inst[6], rad) for name, inst, rad in step_cases()]
    for tag, (inst, RU, RW, radii) in (("ladder", ladder_case()), ("tangent", tangent_case()), ("wide", wide_case()), ("mixed", mixed_case()[:4]), ("vertex", vertex_case())):
        out += [("%s column %d" % (tag, c), inst, RU[c], RW[c], radii[c]) for c in range(len(RU))]
    return out


@pytest.fixture(scope="module")
def solved():
    """name -> (instance, ru, rw, radius, the twin's answer, the reference's answer), computed once for the module."""
    out = {}
    for name, inst, ru, rw, rad in all_columns():
        out[name] = (inst, ru, rw, rad, eqp.kkt_step_pcg(*inst[:5], ru, rw, rad), eqp.kkt_step_reference(*inst[:5], ru, rw, rad))
    return out


def step_errors(got, ref):
    """The relative errors of (dx, dlam, dz, model, theta) of an answer (dx, dlam, dz, info) against the reference's; info a dict or the
    asm_kkt_step_info structure."""
    gi, ri = got[3], ref[3]
    get = (lambda k: gi[k]) if isinstance(gi, dict) else (lambda k: getattr(gi, k))
    return [rel_err(got[0], ref[0]), rel_err(got[1], ref[1]), rel_err(got[2], ref[2]),
            abs(get("model") - ri["model"]) / max(1.0, abs(ri["model"])), abs(get("theta") - ri["theta"]),
            abs(get("norm_step") - ri["norm_step"]) / max(1.0, ri["norm_step"]), abs(get("norm_normal") - ri["norm_normal"]) / max(1.0, ri["norm_normal"])]


def decision_margin(name, trace, radius):
    """The tightest relative margin of the decisions in a trace of kkt_step_reference: nn against normal_share * radius, the sign of every
    p'Hp (against ||p||^2 ||Z'HZ||_2), every trial norm against the tangential radius.  Asserts DECISION_MARGIN on them and
    CONVERGENCE_MARGIN on every convergence test."""
    margins = []
    if np.isfinite(radius) and trace["nn"] > 0.0:
        margins.append(abs(trace["nn"] - trace["cap"]) / trace["cap"])
    for it in trace["iterations"]:
        margins.append(abs(it["php"]) / (it["pp"] * trace["hnorm"]))
        if it["trial"] is not None and np.isfinite(trace["dt"]):
            margins.append(abs(it["trial"] ** 2 - trace["dt"] ** 2) / trace["dt"] ** 2)
        if it["gnorm"] is not None and it["gnorm"] > 1e-3 * 1e-12 * trace["g0"]:          # (a residual that vanishes outright is no close call)
            assert abs(it["gnorm"] / (1e-12 * trace["g0"]) - 1.0) >= CONVERGENCE_MARGIN, (name, it)
    assert not margins or min(margins) >= DECISION_MARGIN, (name, min(margins))
    return min(margins) if margins else INF


# ------------------------------------------------------------------------------------------------ twin against reference
def test_twin_against_the_reference(solved):
    worst = 0.0
    for name, (inst, ru, rw, rad, twin, ref) in solved.items():
        errs = step_errors(twin, ref)
        ti, ri = twin[3], ref[3]
        print("%s: radius %.4g theta %.4f boundary %d status %d, %d iterations, rel err dx %.2e dlam %.2e dz %.2e model %.2e theta %.2e" %
              ((name, rad, ti["theta"], ti["boundary"], ti["status"], ti["cg_iters"]) + tuple(errs[:5])))
        assert (ti["boundary"], ti["cg_iters"], ti["status"]) == (ri["boundary"], ri["cg_iters"], ri["status"]), name
        assert (ti["theta"] < 1.0) == (ri["theta"] < 1.0) and ti["n_free"] == ri["n_free"] and ti["n_rows"] == ri["n_rows"]
        worst = max(worst, *errs)
    print("largest relative error of kkt_step_pcg against kkt_step_reference: %.3e" % worst)
    assert worst <= KKT_STEP_BAR, worst


def test_the_cases_cover_every_outcome(solved):
    infos = {name: s[4][3] for name, s in solved.items()}
    assert {i["boundary"] for i in infos.values()} == {0, 1, 2} and {i["status"] for i in infos.values()} == {0, 2}
    assert any(i["theta"] < 1.0 and i["boundary"] == 1 for i in infos.values()) and any(i["theta"] < 1.0 and i["boundary"] == 0 for i in infos.values())
    assert any(i["boundary"] == 1 and i["cg_iters"] > 1 for i in infos.values())          # the boundary after interior iterations
    assert all(infos["long_normal f=%g" % f]["theta"] < 1.0 for f in (0.25, 0.6))
    assert infos["curvature f=inf"]["status"] == 2 and infos["curvature f=1.5"]["boundary"] == 2
    want = mixed_case()[4]
    assert [(infos["mixed column %d" % c]["boundary"], infos["mixed column %d" % c]["status"]) for c in range(4)] == want
    assert infos["mixed column 0"]["cg_iters"] == 1 and infos["mixed column 3"]["cg_iters"] == 0 and infos["wide column 1"]["cg_iters"] == 0
    assert [infos["vertex column %d" % c]["theta"] < 1.0 for c in range(2)] == [True, False]


def test_decision_margins_of_the_reference(solved):
    """A condition on the cases, not a measurement: the reference decides every boundary test, every curvature sign and nn against
    normal_share * radius by at least DECISION_MARGIN relative (and convergence by CONVERGENCE_MARGIN), so a decision that the device
    takes differently is a bug, not rounding."""
    tightest = INF
    for name, (inst, ru, rw, rad, twin, ref) in solved.items():
        tightest = min(tightest, decision_margin(name, ref[4], rad))
    print("the tightest decision of the reference over all cases: %.3e relative" % tightest)


# ------------------------------------------------------------------------------------------------ properties
def _cauchy_model(inst, ru, rw, rad, theta):
    """The model value at the Cauchy point of the tangential problem: from theta dx0 along -g, g the projected gradient there, to the
    minimiser on that ray inside ||d|| <= dt.  None where the ray is unbounded below."""
    fm, x, lam, rs, bs = inst[:5]
    F, W = np.flatnonzero(bs == 0), np.flatnonzero(rs == 1)
    H, J = sensitivity.lagrangian_hessian(fm, x, lam), sensitivity.dense_jacobian(fm, x)
    HF, A = H[np.ix_(F, F)], J[np.ix_(W, F)]
    dx0 = theta * np.linalg.lstsq(A, -rw[W], rcond=None)[0] if len(W) else np.zeros(len(F))
    P = np.eye(len(F)) - (np.linalg.pinv(A) @ A if len(W) else 0.0)
    g = P @ (ru[F] + HF @ dx0)
    gn, curv = float(np.linalg.norm(g)), float(g @ HF @ g)
    dt = np.sqrt(max(rad ** 2 - float(dx0 @ dx0), 0.0))
    m0 = float(ru[F] @ dx0 + 0.5 * dx0 @ HF @ dx0)
    if gn <= 1e-14 * max(1.0, float(np.linalg.norm(ru))):
        return m0
    if curv <= 0.0 and not np.isfinite(dt):
        return None
    t = dt / gn if curv <= 0.0 else min(gn * gn / curv, dt / gn)
    return m0 - t * gn * gn + 0.5 * t * t * curv


@pytest.mark.parametrize("which", ["twin", "reference"])
def test_properties_of_the_step(solved, which):
    for name, (inst, ru, rw, rad, twin, ref) in solved.items():
        dx, dlam, dz, info = (twin if which == "twin" else ref)[:4]
        fm, x, lam, rs, bs = inst[:5]
        F, W = np.flatnonzero(bs == 0), np.flatnonzero(rs == 1)
        norm = float(np.linalg.norm(dx))
        assert not dx[bs != 0].any() and not dlam[rs == 0].any() and not dz[bs == 0].any()
        assert abs(info["norm_step"] - norm) <= 1e-14 * max(1.0, norm)
        if np.isfinite(rad):
            assert norm <= rad * (1.0 + 1e-12), (name, norm / rad)
            if info["boundary"] != 0:
                assert abs(norm - rad) <= 1e-12 * rad, (name, norm / rad - 1.0)
        else:
            assert info["boundary"] == 0 and info["theta"] == 1.0
        A = sensitivity.dense_jacobian(fm, x)[np.ix_(W, F)]
        if len(W):
            feas = float(np.abs(A @ dx[F] + info["theta"] * rw[W]).max())
            assert feas <= 1e-11 * max(1.0, float(np.abs(rw[W]).max())), (name, feas)      # cond(A A') <= 1e4 times the unit roundoff, with room
        H = sensitivity.lagrangian_hessian(fm, x, lam)
        model = float(ru @ dx + 0.5 * dx @ H @ dx)
        assert abs(info["model"] - model) <= 1e-13 * max(1.0, abs(model))
        cauchy = _cauchy_model(inst, ru, rw, rad, info["theta"])
        if cauchy is not None and info["status"] == 0:
            assert model <= cauchy + 1e-12 * max(1.0, abs(cauchy)), (name, model, cauchy)


@pytest.mark.parametrize("which", ["twin", "reference"])
def test_the_model_does_not_increase_along_the_ladder(solved, which):
    """One right-hand side at growing radii.  With theta = 1 on every rung the constraint A dx = -rw is the same on all of them, the
    iterates of the conjugate gradients are the same and grow in norm, and a larger radius stops further along them: the model value
    cannot rise.  (Where theta < 1 the constraint itself moves with the radius and the model values are not comparable; the ladder of
    LADDER_SHAPE with its own rw is such a ladder below f = 1.2, and only its rungs with theta = 1 are compared.)"""
    k = 4 if which == "twin" else 5
    falls = lambda v: all(b <= a + 1e-12 * max(1.0, abs(a)) for a, b in zip(v, v[1:]))
    rungs = [solved["tangent column %d" % c][k][3] for c in range(len(LADDER))]
    assert all(r["theta"] == 1.0 for r in rungs) and [r["boundary"] != 0 for r in rungs] == [f < 1.0 for f in LADDER]
    models = [r["model"] for r in rungs]
    assert falls(models) and models[0] > models[4] > models[-1], models
    rungs = [solved["ladder column %d" % c][k][3] for c in range(len(LADDER))]
    assert falls([r["model"] for r in rungs if r["theta"] == 1.0]) and sum(r["theta"] == 1.0 for r in rungs) >= 3
    for shape in KKT_SHAPES[:1] + KKT_SHAPES[2:3]:          # no rows, and one row with a short normal step: theta = 1 at every factor
        name = "n%d_B%d_W%d" % shape
        rungs = [solved["%s f=%g" % (name, f)][k][3] for f in FACTORS]
        assert all(r["theta"] == 1.0 for r in rungs) and falls([r["model"] for r in rungs]), name


def test_the_twin_at_an_infinite_radius_is_kkt_pcg(solved):
    for name, (inst, ru, rw, rad, twin, ref) in solved.items():
        if np.isfinite(rad):
            continue
        dx, dlam, dz, info = sensitivity.kkt_pcg(*inst[:5], ru, rw)
        assert np.array_equal(twin[0], dx) and np.array_equal(twin[1], dlam) and np.array_equal(twin[2], dz), name
        assert all(twin[3][key] == info[key] for key in info), name
    inst = kkt_instance(200, 20, 130)
    assert eqp.kkt_step_pcg(*inst, INF, max_iter=1)[3]["status"] == 1 and eqp.kkt_step_reference(*inst, INF, max_iter=1)[3]["status"] == 1


def test_multi_forms_and_argument_errors():
    inst, RU, RW, radii = vertex_case()
    DX, DLAM, DZ, infos = eqp.kkt_step_pcg_multi(*inst[:5], RU, RW, radii)
    RX, RLAM, RZ, rinfos, traces = eqp.kkt_step_reference_multi(*inst[:5], RU, RW, radii)
    assert DX.shape == RX.shape == (2, 8) and DLAM.shape == RLAM.shape == (2, inst[0].m) and len(infos) == len(rinfos) == len(traces) == 2
    for c in range(2):
        one = eqp.kkt_step_pcg(*inst[:5], RU[c], RW[c], radii[c])
        assert np.array_equal(DX[c], one[0]) and np.array_equal(DLAM[c], one[1]) and infos[c] == one[3]
    for bad in (0.0, -1.0, float("nan")):
        for fn in (eqp.kkt_step_pcg, eqp.kkt_step_reference):
            with pytest.raises(ValueError):
                fn(*inst[:5], RU[0], RW[0], bad)
    for share in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            eqp.kkt_step_pcg(*inst[:5], RU[0], RW[0], 1.0, normal_share=share)
    with pytest.raises(ValueError):
        eqp.kkt_step_pcg_multi(*inst[:5], RU, RW, radii[:1])
    assert eqp.kkt_step_pcg(*inst[:5], RU[0], RW[0], radii[0], normal_share=1.0)[3]["theta"] > infos[0]["theta"]


# ------------------------------------------------------------------------------------------------ fraction_to_box
def test_fraction_to_box_edge_cases():
    f = eqp.fraction_to_box
    assert f(np.zeros(3), -np.ones(3), np.ones(3)) == 1.0                                  # a zero step
    assert f(np.zeros(2), np.zeros(2), np.zeros(2)) == 1.0                                 # ... also on active bounds
    assert f(np.array([1.0, -1.0]), np.array([-2.0, 0.0]), np.array([2.0, 5.0])) == 0.0    # an active lower bound, the step pointing outwards
    assert f(np.array([1.0, 1.0]), np.array([-2.0, -1.0]), np.array([0.0, 5.0])) == 0.0    # an active upper bound likewise
    assert f(np.array([-1.0, 1.0]), np.array([0.0, -1.0]), np.array([5.0, 0.5])) == 0.0
    assert f(np.array([1.0, -1.0]), np.array([0.0, -4.0]), np.array([4.0, 0.0])) == 1.0    # active bounds, the step pointing inwards
    assert f(np.array([3.0, -1e9]), np.full(2, -INF), np.full(2, INF)) == 1.0              # infinite bounds
    assert f(np.array([2.0, -8.0]), np.array([-INF, -2.0]), np.array([1.0, INF])) == 0.25
    assert f(np.array([2.0, -1.0]), np.array([-1.0, -1.0]), np.array([1.0, 1.0])) == 0.5
    with pytest.raises(ValueError):
        f(np.zeros(2), np.zeros(3), np.zeros(3))


# ------------------------------------------------------------------------------------------------ eqp_step on hs071, on the host
class ReferenceStepper:
    """kkt_step_reference behind the one method of HipSubOptimizer that eqp_step calls."""
    def __init__(self, fm):
        self.fm = fm

    def kkt_step(self, x, lam, row_state, bound_state, ru, rw, radius):
        out = eqp.kkt_step_reference(self.fm, x, lam, row_state, bound_state, ru, rw, radius)
        self.trace = out[4]
        return out[:4]


def hs071_start():
    """(fm, problem, x, lam): the fixed point of tests/test_kkt_bits_gpu.py::_hs071 near hs071's solution."""
    fm = hs071_param_model()
    pr = fm.to_problem("hs071 rhs parameters")
    return fm, pr, pr.x0 + np.array([0.0, -0.257, -1.1789, 0.3794]), np.array([0.55229, -0.16147])


def kkt_residual(fm, pr, x, lam, row_state, bound_state):
    """max(|| (grad f - J' lam)_F ||_inf, || (g - bound)_W ||_inf) on a working set: the first-order residual the step reduces."""
    grad = fm.eval_grad_f(x, np.zeros(fm.n)) - sensitivity.dense_jacobian(fm, x).T @ lam
    g = np.asarray(pr.eval_g(x, np.zeros(pr.m)), float)
    bound = np.where(np.isfinite(pr.g_L), pr.g_L, pr.g_U)
    return max(float(np.abs(grad[bound_state == 0]).max()), float(np.abs((g - bound)[row_state == 1]).max()))


def test_eqp_step_on_hs071_with_the_reference():
    fm, pr, x, lam = hs071_start()
    rs, bs = sensitivity.working_set(pr, x, lam, np.zeros(4), np.zeros(4), HS071_TOL)
    assert rs.tolist() == [1, 1] and bs.tolist() == [-1, 0, 0, 0]
    ref = ReferenceStepper(fm)
    x1, lam1, info = eqp.eqp_step(ref, fm, pr, x, lam, np.zeros(4), np.zeros(4), HS071_RADIUS, tol=HS071_TOL)
    before, after = kkt_residual(fm, pr, x, lam, rs, bs), kkt_residual(fm, pr, x1, lam1, rs, bs)
    print("hs071: KKT residual %.3e -> %.3e (factor %.1f), boundary %d, ||dx|| %.3e" % (before, after, before / after, info["boundary"], info["norm_step"]))
    assert info["status"] == 0 and info["boundary"] == 0 and after * HS071_GAIN <= before
    assert np.all(x1 >= pr.x_L) and np.all(x1 <= pr.x_U) and x1[0] == 1.0
    decision_margin("hs071", ref.trace, HS071_RADIUS)
