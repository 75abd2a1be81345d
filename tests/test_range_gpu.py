"""Validity ranges of solution sensitivities on the device (include/asm_hip.h, "Validity ranges": asm_sensitivity_range_multi and
asm_batch_sensitivity_range) against sensitivity.validity_range_host on the constructed QPs of tests/test_range_cpu.py - one wavefront, the
pitch boundary, either side of a 64-row tile, with 1, 5, 64 and 65 columns; column independence in both KKT forms of the handle; hs071
at its solution and the 14-bus grid on the Ohm's-law kernel with and without second derivatives; the refusals; a Line-Search run before
and after; three scenarios with their own bounds and data on two slots against fresh handles, byte for byte."""
import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import _lib, acopf, batch, sensitivity
from tests.test_batch_eqp_gpu import _par, _stack
from tests.test_batch_sens_cpu import hs071_scenario_models
from tests.test_kkt_sparse_cpu import SPARSE_LARGE, sparse_instance_of
from tests.test_nlparams_gpu import _handle_for, _same_run
from tests.test_ohm_hess_cpu import grid
from tests.test_range_cpu import RANGE_BAR, RANGE_SEEDS, range_columns, range_instance
from tests.test_sensitivity_gpu import hs071_param_model

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
D, I = _lib.dptr, _lib.i32ptr
LS = "Line Search"
CHUNK = 64
SHAPES = ((8, 3, 4), (33, 1, 1), (96, 10, 63), (96, 10, 65))
NRHS = (1, 5, CHUNK, CHUNK + 1)
TIE = 1e-9                    # a runner-up within this (relative) of the best ratio: the blocker may be either
assert RANGE_BAR == 1e-12


@pytest.fixture(scope="module")
def cases():
    """shape -> (instance, its 65 columns, the twin's ranges, the twin's runner-up ratios), computed once for the module."""
    out = {}
    for shape in SHAPES:
        inst = range_instance(*shape, seed=RANGE_SEEDS[shape])
        DX, DLAM, DZ, _ = range_columns(inst, CHUNK + 1)
        out[shape] = (inst, (DX, DLAM, DZ)) + sensitivity.validity_range_host(inst.pr, *inst.point, DX, DLAM, DZ, runner_up=True)
    return out


def agree(tag, got, want, second):
    """The device's ranges against the twin's: finite t within RANGE_BAR relative, infinities exactly, (position, kind) exactly unless the
    twin's runner-up is within TIE of its best.  Returns (worst relative difference, excused pairs, pairs)."""
    worst, excused = 0.0, 0
    assert got.shape == want.shape
    for c in range(len(want)):
        for s, side in enumerate(("lo", "hi")):
            tg, tw = float(got[c]["t_" + side]), float(want[c]["t_" + side])
            if not np.isfinite(tw):
                assert tg == tw and (got[c]["pos_" + side], got[c]["kind_" + side]) == (-1, 0), (tag, c, side, tg, tw)
                continue
            err = abs(tg - tw) / abs(tw) if tw != 0.0 else abs(tg)
            worst = max(worst, err)
            assert err <= RANGE_BAR, (tag, c, side, tg, tw, err)
            if second[c, s] - abs(tw) > TIE * abs(tw):
                assert (got[c]["pos_" + side], got[c]["kind_" + side]) == (want[c]["pos_" + side], want[c]["kind_" + side]), (tag, c, side, got[c], want[c])
            else:
                excused += 1
    print("%s: %d columns, worst relative difference of t %.3e (bar %.3e), %d near-ties excused" % (tag, len(want), worst, RANGE_BAR, excused))
    return worst, excused, 2 * len(want)


def _range(opt, inst, cols):
    return opt.sensitivity_range(*inst.point, *cols)


# ------------------------------------------------------------------------------------------------ 1. against the twin
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_B%d_W%d" % s)
def test_the_device_agrees_with_the_twin(cases, shape):
    """Fails without the entry."""
    inst, cols, want, second = cases[shape]
    opt = _handle_for(inst.pr, inst.fm)
    excused = total = 0
    for nrhs in NRHS:
        got = _range(opt, inst, [a[:nrhs] for a in cols])
        _, e, t = agree("shape %r, nrhs %d" % (shape, nrhs), got, want[:nrhs], second[:nrhs])
        excused, total = excused + e, total + t
        assert np.all(got["t_lo"] <= 0.0) and np.all(got["t_hi"] >= 0.0)
    assert excused <= 0.05 * total
    assert sensitivity.validity_range(opt, *inst.point, *cols).tobytes() == got.tobytes()
    opt.close()


def test_every_kind_blocks_somewhere_on_the_device(cases):
    kinds = set()
    for shape in SHAPES:
        inst, cols, want, _ = cases[shape]
        opt = _handle_for(inst.pr, inst.fm)
        got = _range(opt, inst, cols)
        opt.close()
        kinds |= set(got["kind_lo"].tolist()) | set(got["kind_hi"].tolist())
    assert kinds >= {1, 2, 3, 4, 5, 6}, kinds


@pytest.mark.parametrize("shape", ((96, 10, 63), (96, 10, 65), SPARSE_LARGE), ids=lambda s: "n%d_B%d_W%d" % s)
def test_rows_of_a_sparse_pattern_against_the_twin(shape):
    """The CSR rows part: the sparse instances of tests/test_kkt_sparse_cpu.py (four entries per row, all `<=` rows) with every third row
    in the working set, so that inactive rows of every 64-row tile compete, and seeded columns; the large shape has 22 workgroups of rows
    and 32 of variables for the last arrival to combine.  The point is made consistent with that working set - the working rows on
    g_U with lam < 0, the others with slack, z of the bound's sign - and is no KKT point: the rule does not ask for one."""
    fm, x = sparse_instance_of(shape)[:2]
    pr = fm.to_problem()
    n, m = fm.n, fm.m
    rng = np.random.default_rng(sum(shape))
    rs, bs = (np.arange(m) % 3 == 0).astype(np.int32), np.zeros(n, np.int32)
    bs[::7] = np.where(np.arange(len(bs[::7])) % 2 == 0, -1, 1)
    size = m / 66.0                                               # (the smallest of N like ratios falls as 1 / N)
    pr.g_U = pr.eval_g(x, np.zeros(m)) + np.where(rs != 0, 0.0, 6.0 * size * rng.uniform(0.5, 1.5, m))
    lam = -2.0 * size * rng.uniform(0.5, 1.5, m) * (rs != 0)
    z = -bs * size * rng.uniform(0.5, 1.5, n)
    pr.x_L, pr.x_U = x - size * rng.uniform(1.0, 3.0, n), x + size * rng.uniform(1.0, 3.0, n)
    k = CHUNK + 1
    cols = (rng.standard_normal((k, n)), rng.standard_normal((k, m)) * (rs != 0), rng.standard_normal((k, n)) * (bs != 0))
    point = (x, lam, np.minimum(z, 0.0), np.maximum(z, 0.0), rs, bs)
    want, second = sensitivity.validity_range_host(pr, *point, *cols, runner_up=True)
    opt = _handle_for(pr, fm)
    got = opt.sensitivity_range(*point, *cols)
    opt.set_kkt_form("sparse")
    assert opt.sensitivity_range(*point, *cols).tobytes() == got.tobytes()
    opt.close()
    _, excused, total = agree("sparse %r" % (shape,), got, want, second)
    kinds = np.concatenate([got["kind_lo"], got["kind_hi"]])
    print("sparse %r: blocking kinds %r" % (shape, np.bincount(kinds, minlength=7).tolist()))
    assert excused <= 0.05 * total and (kinds == 2).sum() >= k // 4 and len(set(kinds.tolist())) >= 2 and not (kinds == 1).any()


# ------------------------------------------------------------------------------------------------ 2. column independence
def test_a_column_depends_on_itself_alone_in_both_kkt_forms_of_the_handle(cases):
    inst, cols, _, _ = cases[(96, 10, 65)]
    opt = _handle_for(inst.pr, inst.fm)
    all65 = _range(opt, inst, cols)
    assert len({all65[c].tobytes() for c in range(CHUNK + 1)}) > CHUNK // 2
    for form in ("dense", "sparse"):
        opt.set_kkt_form(form)
        assert _range(opt, inst, cols).tobytes() == all65.tobytes(), form
        for c in (0, 7, 8, 31, 32, CHUNK - 1, CHUNK):                              # (column CHUNK is alone in the second chunk)
            alone = _range(opt, inst, [a[c:c + 1] for a in cols])
            assert alone[0].tobytes() == all65[c].tobytes(), (form, c)
            perm = [3, 40, c, 0]
            moved = _range(opt, inst, [a[perm] for a in cols])
            assert moved[2].tobytes() == all65[c].tobytes() and moved[0].tobytes() == all65[3].tobytes(), (form, c)
    opt.close()


# ------------------------------------------------------------------------------------------------ 3. other models
def _model_check(tag, opt, fm, pr, run, rs, bs, cols):
    point = (run.x, run.lam, run.mult_x_U, run.mult_x_L, rs, bs)
    want, second = sensitivity.validity_range_host(pr, *point, *cols, runner_up=True)
    got = opt.sensitivity_range(*point, *cols)
    worst, excused, total = agree(tag, got, want, second)
    kinds = sorted(set(got["kind_lo"].tolist()) | set(got["kind_hi"].tolist()))
    print("%s: |W| %d, |B| %d, blocking kinds %r" % (tag, rs.sum(), (bs != 0).sum(), kinds))
    assert excused <= 0.05 * total and np.isfinite(got["t_lo"]).any() and np.isfinite(got["t_hi"]).any() and max(kinds) > 0
    assert np.array_equal(sensitivity.validity_range_host(fm, *point, *cols), want)          # (the function model carries the same bounds)
    return got


def test_hs071_at_its_solution():
    """The expression block: columns from the bound sensitivities of its two working rows and of the variable at its bound."""
    fm = hs071_param_model()
    pr = fm.to_problem("hs071 rhs parameters")
    opt = _handle_for(pr, fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm="Trust Region", max_iter=60, device_eval=True), 0)
    rs, bs = sensitivity.working_set(pr, run.x, run.lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    assert run.ret == 0 and rs.tolist() == [1, 1] and bs.tolist() == [-1, 0, 0, 0]
    rows = opt.bound_sensitivity_multi(run.x, run.lam, rs, bs, [0, 1, 0], [1.0, 1.0, -2.0])
    var = opt.var_bound_sensitivity_multi(run.x, run.lam, rs, bs, [0])
    assert all(i.status == 0 for i in rows[3] + var[3])
    cols = [np.vstack([rows[k], var[k]]) for k in range(3)]
    got = _model_check("hs071", opt, fm, pr, run, rs, bs, cols)
    assert np.all(np.isfinite(got["t_hi"]) | np.isfinite(got["t_lo"])) and len(set(got["kind_lo"].tolist()) | set(got["kind_hi"].tolist())) >= 2
    opt.close()


@pytest.mark.parametrize("hessian", (False, True), ids=("kind1", "kind4"))
def test_the_grid_on_the_ohm_kernel(hessian):
    """A sparse skeleton; kind 1 has no Hessian - the entry needs first derivatives only - and takes seeded columns."""
    fm = acopf.function_model(grid("grid14"), hessian=hessian)
    pr = fm.to_problem("grid14")
    assert fm.nlp.device[0] == ("acopf_ohm_hess" if hessian else "acopf_ohm")
    opt = _handle_for(pr, fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm=LS, max_iter=60, device_eval=True), 12)
    rs, bs = sensitivity.working_set(pr, run.x, run.lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    if hessian:
        W = np.nonzero(rs)[0][:12]
        out = opt.bound_sensitivity_multi(run.x, run.lam, rs, bs, W)
        assert all(i.status == 0 for i in out[3])
        cols = list(out[:3])
    else:
        # (the working rows of this point are equalities and nothing sits at a bound: its variables block every column)
        rng = np.random.default_rng(14)
        cols = [rng.standard_normal((12, pr.n)), rng.standard_normal((12, pr.m)) * (rs != 0), rng.standard_normal((12, pr.n)) * (bs != 0)]
    _model_check("grid14 ohm block, %s" % ("kind 4" if hessian else "kind 1"), opt, fm, pr, run, rs, bs, cols)
    opt.close()


# ------------------------------------------------------------------------------------------------ 4. refusals, state
def test_refusals_leave_the_handle_usable(cases):
    inst, cols, _, _ = cases[(8, 3, 4)]
    n, m, k = inst.n, inst.m, 3
    DX, DLAM, DZ = (np.ascontiguousarray(a[:k]) for a in cols)
    lib = _lib.load()
    out = (_lib.RangeInfo * k)()
    x, lam, z = inst.x.copy(), inst.lam.copy(), inst.z.copy()
    rs, bs = inst.rs.copy(), inst.bs.copy()
    args = lambda: [D(x), D(lam), D(z), I(rs), I(bs), k, D(DX), D(DLAM), D(DZ), out]
    bare = A.HipSubOptimizer(A.QpData(np.zeros(n), 0.0, np.zeros(inst.pr.nnz), np.zeros(m), inst.pr.g_L, inst.pr.g_U, inst.pr.x_L, inst.pr.x_U), inst.pr.j_row, inst.pr.j_col)
    assert lib.asm_sensitivity_range_multi(bare._h, *args()) == ERR_STATE                    # no evaluator yet
    bare.close()
    opt = _handle_for(inst.pr, inst.fm)
    first = _range(opt, inst, (DX, DLAM, DZ))
    for at in (0, 1, 2, 3, 4, 6, 7, 8, 9):
        a = args()
        a[at] = None
        assert lib.asm_sensitivity_range_multi(opt._h, *a) == ERR_ARG, at
    for nrhs in (0, -1):
        a = args()
        a[5] = nrhs
        assert lib.asm_sensitivity_range_multi(opt._h, *a) == ERR_ARG
    for arr, bad in ((rs, 2), (rs, -1), (bs, 2), (bs, -2)):
        keep = arr[1]
        arr[1] = bad
        assert lib.asm_sensitivity_range_multi(opt._h, *args()) == ERR_ARG, (bad,)
        arr[1] = keep
    with pytest.raises(ValueError):
        opt.sensitivity_range(*inst.point, DX, DLAM[:2], DZ)
    with pytest.raises(ValueError):
        opt.sensitivity_range(*inst.point, DX[:, :n - 1], DLAM, DZ)
    assert lib.asm_sensitivity_range_multi(opt._h, *args()) == 0
    assert bytes(out) == first.tobytes() == _range(opt, inst, (DX, DLAM, DZ)).tobytes()
    opt.close()


def test_a_line_search_run_returns_its_bits_after_the_call():
    fm = hs071_param_model()
    pr = fm.to_problem()
    par = A.Parameters(algorithm=LS, max_iter=60, device_eval=True)
    rng = np.random.default_rng(3)
    lam, cols = rng.standard_normal(pr.m), (rng.standard_normal((5, pr.n)), rng.standard_normal((5, pr.m)), rng.standard_normal((5, pr.n)))
    rs, bs = np.array([1, 1], np.int32), np.array([-1, 0, 0, 0], np.int32)
    outs = []
    for calls in (False, True):
        opt = _handle_for(pr, fm)
        f0 = opt.eval_functions(pr.x0)
        if calls:
            opt.sensitivity_range(pr.x0 + 0.01, lam, np.zeros(pr.n), np.ones(pr.n), rs, bs, *cols)
        run = opt.slp_run(pr.x0, par, 3)
        state = (opt.active_set(), opt.ns_basis(), opt.jacobian_values())
        if calls:
            opt.sensitivity_range(run.x, run.lam, run.mult_x_U, run.mult_x_L, rs, bs, *cols)
            after = (opt.active_set(), opt.ns_basis(), opt.jacobian_values())
            assert all(np.array_equal(p, q) for p, q in zip(state[0], after[0])) and np.array_equal(state[1], after[1]) and np.array_equal(state[2], after[2])
        run2 = opt.slp_run(pr.x0, par, 3)
        outs.append((f0, run, run2))
        opt.close()
    (fa, ra, ra2), (fb, rb, rb2) = outs
    assert 1 <= ra.lp_solves <= 3
    _same_run(ra, rb)
    _same_run(ra2, rb2)
    assert fa[0] == fb[0] and np.array_equal(fa[1], fb[1]) and np.array_equal(fa[2], fb[2])


# ------------------------------------------------------------------------------------------------ 5. the scenario batch
def test_three_scenarios_on_two_slots_equal_fresh_handles():
    """Different data (the table) and different bounds per scenario, 64 columns; the refusals come before any fiber starts."""
    S, k = 3, CHUNK
    fms = hs071_scenario_models(S)
    prs = [fm.to_problem("hs071 scenario %d" % s) for s, fm in enumerate(fms)]
    hb = batch.HipBatch(prs[0], 2)
    data = hb.scenario_data(prs)
    runs = hb.slp_run(*_stack(prs), _par(), data=data)
    n, m = hb.n, hb.m
    for s, p in enumerate(prs):                                   # (the kinds of the rows stay; every other bound moves with the scenario)
        p.x_U = p.x_U + 0.25 * s
        p.x_L = p.x_L - 0.125 * s
        p.g_L = p.g_L - np.array([0.5 * s, 0.0])
    rs, bs = batch.working_sets(prs, runs)                        # (with the moved bounds: scenario 0 keeps its working set, the others lose a part)
    assert rs[0].tolist() == [1, 1] and bs[0].tolist() == [-1, 0, 0, 0] and rs[1].tolist() == [0, 1]
    g_L, g_U, x_L, x_U, _ = _stack(prs)
    X, L = np.stack([r.x for r in runs]), np.stack([r.lam for r in runs])
    mU, mL = np.stack([r.mult_x_U for r in runs]), np.stack([r.mult_x_L for r in runs])
    rng = np.random.default_rng(41)
    DX, DLAM, DZ = rng.standard_normal((S, k, n)), rng.standard_normal((S, k, m)), rng.standard_normal((S, k, n))
    before = hb.stats()
    got = hb.sensitivity_range(g_L, g_U, x_L, x_U, X, L, mU, mL, rs, bs, DX, DLAM, DZ)
    after = hb.stats()
    assert got.shape == (S, k) and after["ops"] - before["ops"] > after["launches"] - before["launches"] > 0          # the slots' launches merged
    for s in range(S):
        opt = _handle_for(prs[s], fms[0])
        opt.set_eval_data(data[s])
        want = opt.sensitivity_range(X[s], L[s], mU[s], mL[s], rs[s], bs[s], DX[s], DLAM[s], DZ[s])
        opt.close()
        assert got[s].tobytes() == want.tobytes(), s
        assert np.isfinite(want["t_hi"]).all() and len(set(want["kind_hi"].tolist())) >= 2
    assert got[0].tobytes() != got[1].tobytes()
    via = batch.validity_ranges(hb, prs, runs, DX, DLAM, DZ)
    assert via.tobytes() == got.tobytes()
    # refusals: on the calling thread, no round of the batch runs
    z = np.ascontiguousarray(mU + mL)
    out = (_lib.RangeInfo * (S * k))()
    lib = _lib.load()
    rs32, bs32 = np.array(rs, np.int32), np.array(bs, np.int32)                # (copies: one of them is written below)
    args = lambda: [hb._b, S, D(g_L), D(g_U), D(x_L), D(x_U), D(X), D(L), D(z), I(rs32), I(bs32), k, D(DX), D(DLAM), D(DZ), out]
    rounds = hb.stats()["rounds"]
    for at in (2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15):
        a = args()
        a[at] = None
        assert lib.asm_batch_sensitivity_range(*a) == ERR_ARG, at
    for at, bad in ((1, 0), (11, 0)):
        a = args()
        a[at] = bad
        assert lib.asm_batch_sensitivity_range(*a) == ERR_ARG, at
    bs32[S - 1, 2] = 3                                            # a state outside its value set, in the last scenario
    assert lib.asm_batch_sensitivity_range(*args()) == ERR_ARG
    bs32[S - 1, 2] = bs[S - 1, 2]
    assert hb.stats()["rounds"] == rounds
    assert lib.asm_batch_sensitivity_range(*args()) == 0 and bytes(out) == got.tobytes()
    hb.close()
