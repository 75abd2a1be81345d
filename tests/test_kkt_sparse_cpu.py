"""The sparse form of the KKT solve on the host (include/asm_hip.h, "The form of the KKT solve"): constructed QPs whose working-set
Jacobian is sparse and banded only after a reordering of the rows, the NumPy twin of the device's method against the dense reference on
them (its error sets the device bar of tests/test_kkt_sparse_gpu.py), and the `kkt_form` parameter.  No GPU."""
import numpy as np
import pytest

from activesetmethods_amd import problems, sensitivity
from activesetmethods_amd.batch import HipBatch, check_batch_kkt_form, solve_batch_dynamic, solve_batch_lockstep
from activesetmethods_amd.moi_evaluator import FunctionModel, ScalarFunction
from activesetmethods_amd.parameters import Parameters
from tests.test_sensitivity_cpu import rel_err

# (n, |B|, |W|): no rows | a narrow working set | either side of a 64-tile | three panel steps | a vertex (|W| = |F|) | more than one
# wide block of the factor and |W| > CHOL_NBI + 2 ASM_NB with a band far below |W|: the banded panel launches, band-limited substitutions
SPARSE_LARGE = (2048, 40, 1400)
SPARSE_VERTEX = (96, 10, 86)
SPARSE_SHAPES = ((128, 0, 0), (160, 6, 33), (96, 10, 63), (96, 10, 65), (200, 20, 130), SPARSE_VERTEX, SPARSE_LARGE)
# kkt_pcg against kkt_reference on SPARSE_SHAPES: the largest relative error test_sparse_twin_against_the_reference measures (it prints
# every figure).  The device bar is 10 x this, not below 1e-12 - the rule KKT_BAR of tests/test_sensitivity_cpu.py follows.
SPARSE_TWIN_ERR_MEASURED = 1.89e-12      # dx of the large shape; every other figure is below 6e-13
SPARSE_KKT_BAR = max(10.0 * SPARSE_TWIN_ERR_MEASURED, 1e-12)
DOMINANCE = 3.0
VERTEX_TAIL = 4         # the last variables of the vertex shape: no working row reaches them


def sparse_kkt_instance(n, nB, nW, seed=1, tail=0, bound_rows=(), duplicate_row=False, split=False):
    """kkt_instance's QP (tests/test_sensitivity_cpu.py: function store only, the same objective) with SPARSE affine rows: m = nW + 3
    rows, row i with 4 normal01 entries on consecutive variables from (i (n - 4)) // (m - 1), one of them made dominant (+-3 added; a
    free variable where the row has one, and no variable twice while free ones are left), the rows then permuted so that the ascending
    order of the working set is not the banded one.  The working rows are rows 0 .. nW - 1 of the unpermuted list; B = nB variables at
    alternating bounds: the last `tail` variables (a vertex binds the variables that only the three rows outside W reach) and the others
    spread over the rest of the range.  bound_rows: working rows (unpermuted index) whose four variables all join B.  duplicate_row:
    unpermuted row 1 repeats row 0.  split: the first half of the rows ends left of variable n // 2 and the second half starts at it - the
    row graph of W has two components.  Returns (fm, x, lam, row_state, bound_state, ru, rw); asserts the library's sparse-pattern rule and - without
    the degenerate options - full row rank of A, cond(A A') <= 1e4 and a positive definite reduced Hessian."""
    m = nW + 3
    d = 2.0 + 7.0 * problems.uniform01(100 + seed, n)
    off = 0.8 * problems.uniform01(200 + seed, n) - 0.4
    quad = [(float(d[j]), j + 1, j + 1) for j in range(n)] + [(float(off[j]), j + 1, j + 2) for j in range(0, n - 1, 3)]
    fm = FunctionModel(n, -10.0 * np.ones(n), 10.0 * np.ones(n))
    fm.objective = ScalarFunction(0.0, [(1.0, 1)], quad)
    start = [(i * (n - 4)) // (m - 1) for i in range(m)]
    if split:                       # the rows left of the middle end before it, the others start at it
        half = n // 2
        start = [min(s, half - 4) if i < m // 2 else max(s, half) for i, s in enumerate(start)]
    bound_state = np.zeros(n, np.int32)
    if nB:
        where = np.concatenate([np.linspace(0, n - 1 - tail, nB - tail).astype(int), np.arange(n - tail, n)])
        bound_state[where] = np.where(np.arange(nB) % 2 == 0, -1, 1)
        assert int((bound_state != 0).sum()) == nB
    for i in bound_rows:
        bound_state[start[i]:start[i] + 4] = 1
    vals = problems.normal01(300 + seed, 4 * m).reshape(m, 4)
    used = set()
    for i in range(m):
        free = [k for k in range(4) if bound_state[start[i] + k] == 0]
        fresh = [k for k in free if start[i] + k not in used]
        k = (fresh or free or [i % 4])[0]
        used.add(start[i] + k)
        vals[i, k] += DOMINANCE if vals[i, k] >= 0.0 else -DOMINANCE
    if duplicate_row:
        start[1], vals[1] = start[0], vals[0]
    perm = np.argsort(problems.uniform01(800 + seed, m), kind="stable")        # model row r holds unpermuted row perm[r]
    G = np.zeros((m, n))
    for r in range(m):
        i = int(perm[r])
        G[r, start[i]:start[i] + 4] = vals[i]
        fm.add_constraint(ScalarFunction(0.0, [(float(vals[i, k]), start[i] + k + 1) for k in range(4)]), "le", 1.0)
    row_state = (perm < nW).astype(np.int32)
    x = problems.uniform01(400 + seed, n) - 0.5
    lam = problems.normal01(500 + seed, m)
    ru, rw = problems.normal01(600 + seed, n), problems.normal01(700 + seed, m)
    assert 16 * 4 * m <= m * n, "fill above 1/16: the library keeps no sparse pattern"
    W = np.nonzero(row_state)[0]
    assert nW < 8 or not np.array_equal(np.argsort([start[int(perm[r])] for r in W], kind="stable"), np.arange(nW)), "the ascending order of W is the banded one"
    if not (bound_rows or duplicate_row):
        A = G[W][:, bound_state == 0]
        if nW:
            assert np.linalg.matrix_rank(A) == nW
            assert np.linalg.cond(A @ A.T) <= 1e4, (n, nB, nW, np.linalg.cond(A @ A.T))
        ev = np.linalg.eigvalsh(sensitivity.lagrangian_hessian(fm, x, lam))
        assert ev[0] >= 1.0 and ev[-1] <= 10.0, (ev[0], ev[-1])
    return fm, x, lam, row_state, bound_state, ru, rw


def sparse_instance_of(shape):
    return sparse_kkt_instance(*shape, tail=VERTEX_TAIL if shape == SPARSE_VERTEX else 0)


@pytest.fixture(scope="module")
def sparse_references():
    """shape -> (instance, kkt_reference's answer), computed once for the module."""
    out = {}
    for shape in SPARSE_SHAPES:
        inst = sparse_instance_of(shape)
        out[shape] = (inst, sensitivity.kkt_reference(*inst))
    return out


def test_sparse_twin_against_the_reference(sparse_references):
    worst = 0.0
    for shape, (inst, ref) in sparse_references.items():
        dx, dlam, dz, info = sensitivity.kkt_pcg(*inst)
        errs = [rel_err(g, w) for g, w in zip((dx, dlam, dz), ref)]
        print("shape %r: status %d, %d CG iterations, rel err dx %.3e dlam %.3e dz %.3e" % ((shape, info["status"], info["cg_iters"]) + tuple(errs)))
        n, nB, nW = shape
        assert info["status"] == 0 and info["n_free"] == n - nB and info["n_rows"] == nW and info["dropped_pivots"] == 0
        assert (info["cg_iters"] == 0) == (n - nB == nW)
        worst = max(worst, *errs)
    print("largest relative error of kkt_pcg against kkt_reference on the sparse instances: %.3e" % worst)
    # what the twin itself can reach (tests/test_sensitivity_cpu.py gives the argument): below 1e-10; the constant above records the figure
    assert worst <= 1e-10
    assert SPARSE_KKT_BAR == max(10.0 * SPARSE_TWIN_ERR_MEASURED, 1e-12)


def test_sparse_instances_are_what_the_device_tests_need():
    """The large shape: more than one wide block of the factor (512 or 1024 wide) and more rows than one banded panel launch takes; the
    degenerate builders keep the pattern rule."""
    n, nB, nW = SPARSE_LARGE
    assert n == 2048 and 1300 <= nW <= 1500 and nW > 512 + 2 * 64
    assert SPARSE_VERTEX[0] - SPARSE_VERTEX[1] == SPARSE_VERTEX[2]
    fm, x, lam, rs, bs, ru, rw = sparse_kkt_instance(160, 6, 33, bound_rows=(5,))
    J = sensitivity.dense_jacobian(fm, x)
    dead = [r for r in np.nonzero(rs)[0] if not J[r][bs == 0].any()]
    assert len(dead) == 1
    fm, x, lam, rs, bs, ru, rw = sparse_kkt_instance(160, 6, 33, duplicate_row=True)
    J = sensitivity.dense_jacobian(fm, x)[rs == 1]
    assert np.linalg.matrix_rank(J) == 32
    fm, x, lam, rs, bs, ru, rw = sparse_kkt_instance(160, 6, 33, split=True)
    J = sensitivity.dense_jacobian(fm, x)[rs == 1]
    left, right = (J[:, :80] != 0).any(axis=1), (J[:, 80:] != 0).any(axis=1)
    assert left.any() and right.any() and not (left & right).any()


def test_kkt_form_parameter_is_validated():
    assert Parameters().kkt_form == "dense" and Parameters(kkt_form="sparse").kkt_form == "sparse"
    for bad in ("banded", "Sparse", "", None, 1):
        with pytest.raises(ValueError):
            Parameters(kkt_form=bad)


def test_batch_entries_refuse_the_sparse_form():
    par = Parameters(algorithm="SLP-EQP", device_eval=True, kkt_form="sparse")
    check_batch_kkt_form(Parameters(algorithm="SLP-EQP", device_eval=True))
    with pytest.raises(ValueError, match="per handle"):
        check_batch_kkt_form(par)
    # refused before a batch is built or touched: no GPU is needed to be told
    with pytest.raises(ValueError, match="per handle"):
        solve_batch_lockstep([], par, 4)
    with pytest.raises(ValueError, match="per handle"):
        solve_batch_dynamic(lambda s: None, 4, par, 4, batch=None)
    with pytest.raises(ValueError, match="per handle"):
        HipBatch.slp_run(None, np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1)), par)
