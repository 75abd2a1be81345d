"""Validity ranges of solution sensitivities on the host (include/asm_hip.h, "Validity ranges"): sensitivity.validity_range_host, the
specification of the rule, on constructed QPs at a strict KKT point.  Every finite range it returns is checked against the KKT conditions
of the perturbed QP just inside it and against the condition it names just outside; then the order on equal ratios, the clamping, the
twin in extended precision beside float64 (the device's bar), and the header against the bindings.  No GPU."""
import ctypes
import re

import numpy as np
import pytest

from activesetmethods_amd import _lib, problems, sensitivity
from activesetmethods_amd.moi_evaluator import FunctionModel, ScalarFunction
from tests.test_slp_eqp_cpu import _c_layout, _header

INF = float("inf")
# (n, |B|, |W|): one wavefront | the pitch boundary, a single working row | either side of a 64-row tile
RANGE_SHAPES = ((8, 3, 4), (33, 1, 1), (96, 10, 63), (96, 10, 65), (200, 20, 130))
# the seed of each shape's instance, chosen on the CPU so that over RANGE_SHAPES every kind 1..6 blocks somewhere (asserted below) and
# no (column, side) of the twin is a near-tie (tests/test_range_gpu.py)
RANGE_SEEDS = {(8, 3, 4): 1, (33, 1, 1): 1, (96, 10, 63): 1, (96, 10, 65): 1, (200, 20, 130): 1}
# float64 twin against the np.longdouble twin on RANGE_SHAPES: the largest relative difference of a finite t that
# test_the_twin_in_extended_precision measures (it prints every figure).  The device bar is 10 x this - the factor this project grants
# the device's summation order - and not below 1e-12.
RANGE_TWIN_ERR_MEASURED = 9.77e-16
RANGE_BAR = max(10.0 * RANGE_TWIN_ERR_MEASURED, 1e-12)
INSIDE, OUTSIDE, KKT_TOL = 1.0 - 1e-5, 1.0 + 1e-5, 1e-9


class RangeInstance:
    """What range_instance returns: the function model, the problem with its bounds, the strict KKT point and its working set, the dense
    H, G and linear term c of the QP  min c'x + x'Hx/2  s.t.  g_L <= G x <= g_U, x_L <= x <= x_U."""
    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def point(self):
        return self.x, self.lam, self.mU, self.mL, self.rs, self.bs


def range_instance(n, nB, nW, seed=1):
    """A function-store QP (nlp_kind 0) built like tests/test_sensitivity_cpu.kkt_instance - diagonal in [2, 9], a few products, dense
    normal01 rows - but AT a strict KKT point: x_B on its bounds at alternating sides; the nW working rows on a bound, of four sorts in
    turn (`<=` at g_U, `>=` at g_L, two-sided at g_L, equality); multipliers and z of the right sign and away from zero; three inactive
    rows (`<=`, `>=`, two-sided) and the free variables with slack; the linear term chosen so that df - J' lam - z = 0.  The function
    store orders its rows `<=`, `>=`, `==`: the working rows are spread over the row range.  A two-sided row is a `>=` row of the store
    whose upper bound the problem adds."""
    m = nW + 3
    u01, n01 = problems.uniform01, problems.normal01
    d = 2.0 + 7.0 * u01(100 + seed, n)
    off = 0.8 * u01(200 + seed, n) - 0.4
    quad = [(float(d[j]), j + 1, j + 1) for j in range(n)] + [(float(off[j]), j + 1, j + 2) for j in range(0, n - 1, 3)]
    # logical rows: the working rows in turn, then the three inactive ones; the store's order is by kind, stable
    sort = [r % 4 for r in range(nW)] + [0, 1, 2]                     # 0 `<=`, 1 `>=`, 2 two-sided, 3 equality
    active = np.array([True] * nW + [False] * 3)
    group = np.array([{0: 0, 1: 1, 2: 1, 3: 2}[s] for s in sort])
    order = np.argsort(group, kind="stable")
    sort, active = np.array(sort)[order], active[order]
    G = n01(300 + seed, m * n).reshape(m, n)
    bs = np.zeros(n, np.int32)
    if nB:
        bs[np.linspace(0, n - 1, nB).astype(int)] = np.where(np.arange(nB) % 2 == 0, -1, 1)
    x_L, x_U = -1.0 - u01(400 + seed, n), 1.0 + u01(410 + seed, n)
    x = u01(420 + seed, n) - 0.5
    x = np.where(bs < 0, x_L, np.where(bs > 0, x_U, x))
    E = G @ x
    # the scales: a column of a QP does not depend on the multipliers or the slacks, so a few columns of the bare system say how fast rows,
    # multipliers and z move against the free variables (whose slack is about 1); every kind's ratios are put on that footing, times its
    # share of the candidates - the smallest of N like ratios falls as 1 / N
    W, F = active, bs == 0
    ineq = W & (sort != 3)
    bare = FunctionModel(n, x_L, x_U)
    bare.objective = ScalarFunction(0.0, [], quad)
    for i in range(m):
        bare.add_constraint(ScalarFunction(0.0, [(float(G[i, j]), j + 1) for j in range(n)]), {0: "le", 1: "ge", 2: "ge", 3: "eq"}[sort[i]], 0.0)
    RU, RW = n01(480 + seed, 8 * n).reshape(8, n), np.zeros((8, m))
    RU[4:] = 0.0
    RW[np.arange(4, 8), np.nonzero(W)[0][np.arange(4) % nW]] = -1.0
    dX, dL, dZ = sensitivity.kkt_reference_multi(bare, x, np.zeros(m), active.astype(np.int32), bs, RU, RW)
    med = lambda a: float(np.median(np.abs(a))) if a.size and np.median(np.abs(a)) > 0.0 else 1.0
    per_x = med(dX[:, F]) * F.sum()
    # (the factors 6, 1.4, 6 are hand-tuned: on the equal footing alone the variables hardly ever block on the larger shapes)
    s_row, s_lam, s_z = 6 * med((dX @ G.T)[:, ~W]) * 3 / per_x, 1.4 * med(dL[:, ineq]) * max(ineq.sum(), 1) / per_x, 6 * med(dZ[:, ~F]) * max(nB, 1) / per_x
    slack, width = s_row * (0.5 + u01(430 + seed, m)), s_row * (2.0 + u01(440 + seed, m))
    mag = s_lam * (0.5 + u01(450 + seed, m))
    g_L, g_U, lam = np.full(m, -INF), np.full(m, INF), np.zeros(m)
    for i in range(m):
        s = sort[i]
        if active[i]:
            if s == 0: g_U[i], lam[i] = E[i], -mag[i]
            elif s == 1: g_L[i], lam[i] = E[i], mag[i]
            elif s == 2: g_L[i], g_U[i], lam[i] = E[i], E[i] + width[i], mag[i]
            else: g_L[i], g_U[i], lam[i] = E[i], E[i], mag[i] * (1.0 if i % 2 else -1.0)
        else:
            if s == 0: g_U[i] = E[i] + slack[i]
            elif s == 1: g_L[i] = E[i] - slack[i]
            else: g_L[i], g_U[i] = E[i] - slack[i], E[i] + width[i]
    z = s_z * np.where(bs < 0, 0.5 + u01(460 + seed, n), np.where(bs > 0, -0.5 - u01(470 + seed, n), 0.0))
    fm = FunctionModel(n, x_L, x_U)
    fm.objective = ScalarFunction(0.0, [], quad)
    for i in range(m):
        kind = {0: "le", 1: "ge", 2: "ge", 3: "eq"}[sort[i]]
        fm.add_constraint(ScalarFunction(0.0, [(float(G[i, j]), j + 1) for j in range(n)]), kind, float(g_U[i] if kind == "le" else g_L[i]))
    Hx = fm.eval_grad_f(x, np.zeros(n)).copy()                        # (no linear term yet: H x)
    c = G.T @ lam + z - Hx
    fm.objective = ScalarFunction(0.0, [(float(c[j]), j + 1) for j in range(n)], quad)
    pr = fm.to_problem("range_instance")
    pr.g_L, pr.g_U = g_L.copy(), g_U.copy()
    H = sensitivity.lagrangian_hessian(fm, x, lam)
    rs = active.astype(np.int32)
    assert np.array_equal(sensitivity.dense_jacobian(fm, x), G)
    assert np.abs(fm.eval_grad_f(x, np.zeros(n)) - G.T @ lam - z).max() <= 1e-12
    return RangeInstance(fm=fm, pr=pr, x=x, lam=lam, mU=np.minimum(z, 0.0), mL=np.maximum(z, 0.0), z=z, rs=rs, bs=bs, H=H, G=G, c=c, sort=sort,
                         g_L=g_L, g_U=g_U, x_L=x_L, x_U=x_U, n=n, m=m)


def range_columns(inst, count, seed=0):
    """`count` sensitivity columns of the instance through the dense kkt_reference: first the moves of the bounds of its one-sided and
    equality working rows (ru = 0, rw_i = -1), in row order, then objective tilts (ru = a seeded direction, rw = 0); more columns than
    that repeat the list with other tilts.  Returns (DX, DLAM, DZ, what) with what[c] = ("bound", row) or ("tilt", direction)."""
    rows = [i for i in range(inst.m) if inst.rs[i] and inst.sort[i] != 2]
    RU, RW, what = np.zeros((count, inst.n)), np.zeros((count, inst.m)), []
    per = len(rows) + 3
    for c in range(count):
        k, again = c % per, c // per
        if k < len(rows):
            move = 1.0 if again % 2 == 0 else -0.5
            RW[c, rows[k]] = -move
            what.append(("bound", rows[k], move))
        else:
            RU[c] = problems.normal01(900 + 7 * seed + c, inst.n)
            what.append(("tilt", RU[c].copy(), 1.0))
    DX, DLAM, DZ = sensitivity.kkt_reference_multi(inst.fm, inst.x, inst.lam, inst.rs, inst.bs, RU, RW)
    return DX, DLAM, DZ, what


def _upper(inst):
    E = inst.G @ inst.x
    return ~(inst.g_L > -INF) | ((inst.g_U < INF) & (np.abs(E - inst.g_U) < np.abs(E - inst.g_L)))


def kkt_violations(inst, what, t, dx, dlam, dz):
    """The violations of the KKT conditions of the perturbed QP at the point t of the path: (stationarity, working set held, primal
    feasibility of what is outside the working set, signs of the multipliers) - each a largest violation, 0.0 when it holds - and the
    signed violation of every condition a range can name: viol[kind](position)."""
    x, lam, z = inst.x + t * dx, inst.lam + t * dlam, inst.z + t * dz
    g_L, g_U, c = inst.g_L.copy(), inst.g_U.copy(), inst.c.copy()
    if what[0] == "bound":
        i, sg = what[1], what[2]
        if _upper(inst)[i] or inst.sort[i] == 3: g_U[i] += sg * t
        if not _upper(inst)[i] or inst.sort[i] == 3: g_L[i] += sg * t
    else:
        c = c + t * what[1]
    E = inst.G @ x
    up = _upper(inst)
    W, F = inst.rs == 1, inst.bs == 0
    stat = np.abs(inst.H @ x + c - inst.G.T @ lam - z).max()
    held = max([0.0] + [abs(E[i] - (g_U[i] if up[i] else g_L[i])) for i in np.nonzero(W)[0]]
               + [abs(x[j] - (inst.x_U[j] if inst.bs[j] > 0 else inst.x_L[j])) for j in np.nonzero(~F)[0]]
               + list(np.abs(lam[~W])) + list(np.abs(z[F])))
    row_lo, row_up = g_L - E, E - g_U                      # > 0: violated
    var_lo, var_up = inst.x_L - x, x - inst.x_U
    eq = inst.g_L == inst.g_U
    lam_bad = np.where(W & ~eq, np.where(up, lam, -lam), -INF)       # a row at g_U wants lam <= 0, at g_L lam >= 0
    z_bad = np.where(~F, np.where(inst.bs > 0, z, -z), -INF)
    primal = max(0.0, row_lo[~W].max(), row_up[~W].max(), var_lo[F].max(), var_up[F].max())
    signs = max(0.0, lam_bad.max(), z_bad.max())
    m = inst.m
    viol = {1: lambda p: row_lo[p], 2: lambda p: row_up[p], 3: lambda p: var_lo[p - m], 4: lambda p: var_up[p - m], 5: lambda p: lam_bad[p],
            6: lambda p: z_bad[p - m]}
    return (stat, held, primal, signs), viol


@pytest.fixture(scope="module")
def range_cases():
    """shape -> (instance, columns, the twin's ranges with its runner-up ratios), computed once for the module."""
    out = {}
    for shape in RANGE_SHAPES:
        inst = range_instance(*shape, seed=RANGE_SEEDS[shape])
        cols = range_columns(inst, 40)
        out[shape] = (inst, cols, sensitivity.validity_range_host(inst.pr, *inst.point, *cols[:3], runner_up=True))
    return out


def test_every_range_is_the_edge_of_the_kkt_conditions(range_cases):
    """The perturbed QP's KKT conditions hold at (1 - 1e-5) t to 1e-9, and the reported (kind, position) is violated at (1 + 1e-5) t."""
    kinds = set()
    for shape, (inst, (DX, DLAM, DZ, what), (rg, _)) in range_cases.items():
        finite = 0
        for c in range(len(DX)):
            for side in ("lo", "hi"):
                t, pos, kind = float(rg[c]["t_" + side]), int(rg[c]["pos_" + side]), int(rg[c]["kind_" + side])
                assert (t <= 0.0) if side == "lo" else (t >= 0.0)
                if not np.isfinite(t):
                    assert (pos, kind) == (-1, 0)
                    continue
                finite += 1
                kinds.add(kind)
                assert 1 <= kind <= 6 and 0 <= pos < inst.m + inst.n and (pos < inst.m) == (kind in (1, 2, 5)) and abs(t) > 1e-6
                inside, _ = kkt_violations(inst, what[c], INSIDE * t, DX[c], DLAM[c], DZ[c])
                assert max(inside) <= KKT_TOL, (shape, c, side, t, sensitivity.RANGE_KINDS[kind], inside)
                _, viol = kkt_violations(inst, what[c], OUTSIDE * t, DX[c], DLAM[c], DZ[c])
                assert viol[kind](pos) > 0.0, (shape, c, side, t, sensitivity.RANGE_KINDS[kind], viol[kind](pos))
        print("shape %r: %d finite ranges of %d" % (shape, finite, 2 * len(DX)))
        assert finite > len(DX)
    assert kinds == {1, 2, 3, 4, 5, 6}, kinds


def test_each_kind_blocks_on_the_shapes_of_the_device_tests(range_cases):
    """The four shapes tests/test_range_gpu.py runs, with the columns it runs: every kind 1..6 is the blocker of at least one
    (column, side), and the twin has no near-tie there (runner-up within 1e-9 relative of the best)."""
    kinds, near, total = set(), 0, 0
    for shape in RANGE_SHAPES[:4]:
        inst = range_cases[shape][0]
        cols = range_columns(inst, 65)
        rg, second = sensitivity.validity_range_host(inst.pr, *inst.point, *cols[:3], runner_up=True)
        kinds |= set(rg["kind_lo"].tolist()) | set(rg["kind_hi"].tolist())
        best = np.stack([-rg["t_lo"], rg["t_hi"]], axis=1)
        with np.errstate(invalid="ignore"):
            near += int(np.sum(np.isfinite(best) & (second - best <= 1e-9 * np.abs(best))))
        total += best.size
    print("near-ties: %d of %d (column, side) pairs" % (near, total))
    assert kinds >= {1, 2, 3, 4, 5, 6}, kinds
    assert near <= 0.05 * total


# ------------------------------------------------------------------------------------------------ order on equal ratios, clamping
def _tie_problem():
    """n = 3, two identical inactive `<=` rows x0 - x1 <= 1 and variables 0 and 1 with the same value and bounds."""
    fm = FunctionModel(3, [-4.0, -4.0, -1.0], [4.0, 4.0, 1.0])
    fm.objective = ScalarFunction(0.0, [], [(1.0, 1, 1), (1.0, 2, 2), (1.0, 3, 3)])
    for _ in range(2):
        fm.add_constraint(ScalarFunction(0.0, [(1.0, 1), (-1.0, 2)]), "le", 1.0)
    return fm.to_problem("ties")


def test_equal_ratios_report_the_smallest_position_and_a_zero_column_reports_nothing():
    pr = _tie_problem()
    x, zero = np.zeros(3), np.zeros(3)
    rs, bs = np.zeros(2, np.int32), np.zeros(3, np.int32)
    DX = np.array([[0.5, 0.0, 0.0], [0.25, 0.25, 0.0], [0.0, 0.0, 0.0]])
    rg = sensitivity.validity_range_host(pr, x, np.zeros(2), zero, zero, rs, bs, DX, np.zeros((3, 2)), np.zeros((3, 3)))
    # column 0: both rows reach g_U at t = 2, variable 0 its bound at 8 - the duplicated row, the first one wins; downwards variable 0 alone
    assert (rg[0]["t_hi"], rg[0]["pos_hi"], rg[0]["kind_hi"]) == (2.0, 0, 2) and (rg[0]["t_lo"], rg[0]["pos_lo"], rg[0]["kind_lo"]) == (-8.0, 2, 3)
    # column 1: the rows do not move, variables 0 and 1 reach their bounds together - the duplicated bound, the first one wins
    assert (rg[1]["t_hi"], rg[1]["pos_hi"], rg[1]["kind_hi"]) == (16.0, 2, 4) and (rg[1]["t_lo"], rg[1]["pos_lo"], rg[1]["kind_lo"]) == (-16.0, 2, 3)
    assert (rg[2]["t_lo"], rg[2]["t_hi"]) == (-INF, INF) and tuple(rg[2][k] for k in ("pos_lo", "kind_lo", "pos_hi", "kind_hi")) == (-1, 0, -1, 0)


def test_a_violated_row_and_a_multiplier_of_the_wrong_sign_give_zero_on_their_side():
    pr = _tie_problem()
    zero = np.zeros(3)
    bs = np.zeros(3, np.int32)
    # row 0 inactive and violated (E = 1.5 > 1), moving further up along +dx: 0 upwards; downwards it is variable 0 at (-4 - 1.5) / -1
    x = np.array([1.5, 0.0, 0.0])
    DX = np.array([[1.0, 0.0, 0.0]])
    rg = sensitivity.validity_range_host(pr, x, np.zeros(2), zero, zero, np.zeros(2, np.int32), bs, DX, np.zeros((1, 2)), np.zeros((1, 3)))
    assert (rg[0]["t_hi"], rg[0]["pos_hi"], rg[0]["kind_hi"]) == (0.0, 0, 2) and (rg[0]["t_lo"], rg[0]["pos_lo"], rg[0]["kind_lo"]) == (-5.5, 2, 3)
    # row 1 in the working set at g_U with lam = +0.5 (it wants lam <= 0) and dlam = +1: -lam / dlam < 0, clamped to 0 upwards; downwards
    # dlam < 0 is no candidate for a row at its upper bound
    x = np.array([1.0, 0.0, 0.0])
    rg = sensitivity.validity_range_host(pr, x, np.array([0.0, 0.5]), zero, zero, np.array([0, 1], np.int32), bs, np.zeros((1, 3)),
                                         np.array([[0.0, 1.0]]), np.zeros((1, 3)))
    assert (rg[0]["t_hi"], rg[0]["pos_hi"], rg[0]["kind_hi"]) == (0.0, 1, 5) and (rg[0]["t_lo"], rg[0]["pos_lo"], rg[0]["kind_lo"]) == (-INF, -1, 0)
    # a bound multiplier of the wrong sign: variable 2 at its upper bound with z = +0.25 and dz = +1
    x = np.array([0.0, 0.0, 1.0])
    rg = sensitivity.validity_range_host(pr, x, np.zeros(2), zero, np.array([0.0, 0.0, 0.25]), np.zeros(2, np.int32), np.array([0, 0, 1], np.int32),
                                         np.zeros((1, 3)), np.zeros((1, 2)), np.array([[0.0, 0.0, 1.0]]))
    assert (rg[0]["t_hi"], rg[0]["pos_hi"], rg[0]["kind_hi"]) == (0.0, 4, 6) and rg[0]["kind_lo"] == 0


# ------------------------------------------------------------------------------------------------ the device's bar
def test_the_twin_in_extended_precision(range_cases):
    worst = 0.0
    for shape, (inst, (DX, DLAM, DZ, _), (rg, _)) in range_cases.items():
        ld = sensitivity.validity_range_host(inst.pr, *inst.point, DX, DLAM, DZ, dtype=np.longdouble)
        for k in ("pos_lo", "kind_lo", "pos_hi", "kind_hi"):
            assert np.array_equal(rg[k], ld[k]), (shape, k)
        for k in ("t_lo", "t_hi"):
            fin = np.isfinite(ld[k])
            assert np.array_equal(fin, np.isfinite(rg[k]))
            err = float(np.max(np.abs(rg[k][fin] - ld[k][fin]) / np.abs(ld[k][fin]))) if fin.any() else 0.0
            print("shape %r, %s: float64 against longdouble, largest relative difference %.3e" % (shape, k, err))
            worst = max(worst, err)
    print("RANGE_TWIN_ERR_MEASURED should be %.3e (is %.3e); RANGE_BAR %.3e" % (worst, RANGE_TWIN_ERR_MEASURED, RANGE_BAR))
    assert worst <= 1.05 * RANGE_TWIN_ERR_MEASURED or 10.0 * worst <= 1e-12


# ------------------------------------------------------------------------------------------------ header against bindings
def test_the_structure_matches_the_header():
    fields, size = _c_layout("asm_range_info")
    T = _lib.RangeInfo
    assert [(f[0], getattr(T, f[0]).offset) for f in T._fields_] == fields and ctypes.sizeof(T) == size == 32
    assert sensitivity.RANGE_DTYPE == np.dtype(T) and len(sensitivity.RANGE_KINDS) == 7
    txt = _header()
    for k, name in enumerate(("NONE", "ROW_LOWER", "ROW_UPPER", "VAR_LOWER", "VAR_UPPER", "ROW_MULT", "VAR_MULT")):
        assert int(re.search(r"#define\s+ASM_RANGE_%s\s+(\d+)" % name, txt).group(1)) == k


def test_the_prototypes_match_the_header_and_the_library_exports_them():
    txt = _header()
    for name in ("asm_sensitivity_range_multi", "asm_batch_sensitivity_range"):
        args = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, txt).group(1).split(",")
        res, types = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(types) == len(args)
        for a, t in zip(args, types):
            a = a.strip()
            if "asm_range_info*" in a:
                assert t == ctypes.POINTER(_lib.RangeInfo), (name, a)
            elif a.startswith("asm_handle*") or a.startswith("asm_batch*"):
                assert t is ctypes.c_void_p, (name, a)
            elif "*" not in a:
                assert t is (ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_int32), (name, a)
            elif a.startswith("const double*"):
                assert t == ctypes.POINTER(ctypes.c_double), (name, a)
            else:
                assert a.startswith("const int32_t*") and t == ctypes.POINTER(ctypes.c_int32), (name, a)
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
