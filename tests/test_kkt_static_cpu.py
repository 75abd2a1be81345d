"""The static row order of the sparse KKT form on the host (include/asm_hip.h, "The row order of the sparse form"): the `kkt_order`
parameter, what the scenario batches accept of form and order, the new symbols of the built library, and the property the order rests
on - the reverse Cuthill-McKee order of ALL rows, restricted to a working set, is a banded order of that set no wider than the all-rows
band.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from activesetmethods_amd import _lib, acopf
from activesetmethods_amd.batch import HipBatch, check_batch_kkt_form, solve_batch_dynamic, solve_batch_lockstep
from activesetmethods_amd.parameters import Parameters
from oracle.lp_solver import rcm_order
from tests.test_kkt_sparse_cpu import SPARSE_SHAPES, sparse_instance_of

NEW_SYMBOLS = ("asm_kkt_set_order", "asm_kkt_order_info", "asm_kkt_row_order", "asm_batch_kkt_set_form", "asm_kkt_set_form")


def row_columns(pr):
    """The column set of every row of the problem's Jacobian pattern (j_row, j_col are 1-based)."""
    cols = [set() for _ in range(pr.m)]
    for r, c in zip(pr.j_row, pr.j_col):
        cols[int(r) - 1].add(int(c) - 1)
    return cols


def band_and_pairs(rows, cols):
    """Of the rows `rows` taken in that order: the largest distance between two that share a column (0 without such a pair) and the number
    of structural entries of the lower triangle of their Gram matrix, diagonal included - what asm_kkt_form_info reports as n_pairs."""
    by_col = {}
    for q, r in enumerate(rows):
        for c in cols[int(r)]:
            by_col.setdefault(c, []).append(q)
    pairs = {(q, q) for q in range(len(rows))}
    for qs in by_col.values():
        pairs.update((a, b) for a in qs for b in qs if b < a)
    return max((a - b for a, b in pairs), default=0), len(pairs)


def static_order(cols):
    """(the reverse Cuthill-McKee order of all rows, its band): what the library keeps at its first sparse call."""
    order, bw = rcm_order(cols)
    return [int(r) for r in order], int(bw)


def restricted(order, row_state):
    """The all-rows order filtered by row_state: the working rows as the static order takes them."""
    return [r for r in order if row_state[r]]


def fresh_order(cols, row_state):
    """(the working rows in the reverse Cuthill-McKee order of their own coupling graph, its band): the working-set order."""
    W = [int(r) for r in np.nonzero(row_state)[0]]
    order, bw = rcm_order([cols[r] for r in W])
    return [W[int(q)] for q in order], int(bw)


def test_kkt_order_parameter_is_validated():
    assert Parameters().kkt_order == "working-set" and Parameters(kkt_order="static").kkt_order == "static"
    assert Parameters(kkt_order="working-set").kkt_order == "working-set"
    for bad in ("rcm", "Static", "", None, 1):
        with pytest.raises(ValueError):
            Parameters(kkt_order=bad)


def test_batch_entries_accept_sparse_static_and_refuse_sparse_working_set():
    ok = Parameters(algorithm="SLP-EQP", device_eval=True, kkt_form="sparse", kkt_order="static")
    check_batch_kkt_form(ok)
    check_batch_kkt_form(Parameters(algorithm="SLP-EQP", device_eval=True, kkt_order="static"))
    for par in (Parameters(algorithm="SLP-EQP", device_eval=True, kkt_form="sparse"),
                Parameters(algorithm="SLP-EQP", device_eval=True, kkt_form="sparse", kkt_order="working-set")):
        with pytest.raises(ValueError, match="per handle") as e:
            check_batch_kkt_form(par)
        assert 'kkt_order="static"' in str(e.value)
        # refused before a batch is built or touched: no GPU is needed to be told
        with pytest.raises(ValueError, match="per handle"):
            solve_batch_lockstep([], par, 4)
        with pytest.raises(ValueError, match="per handle"):
            solve_batch_dynamic(lambda s: None, 4, par, 4, batch=None)
        with pytest.raises(ValueError, match="per handle"):
            HipBatch.slp_run(None, np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1)), par)
    with pytest.raises(ValueError, match="limited-memory"):
        check_batch_kkt_form(Parameters(algorithm="SLP-EQP", device_eval=True, kkt_form="sparse", kkt_order="static", hessian_type="limited-memory"))


def test_the_built_library_exports_the_new_symbols():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    assert _lib.KKT_ORDERS == {"working-set": 0, "static": 1}
    assert C.sizeof(_lib.KktOrderInfo) == 24


def _report(name, cols, row_state, all_band):
    rows_s, (rows_f, band_f) = restricted(static_order(cols)[0], row_state), fresh_order(cols, row_state)
    band_s, pairs_s = band_and_pairs(rows_s, cols)
    assert band_and_pairs(rows_f, cols) == (band_f, pairs_s)        # the helper measures what rcm_order measures; the pairs do not depend on the order
    nW = int(np.sum(row_state))
    ratio = band_s / band_f if band_f else 1.0
    print("%s: |W| %d, band of the fresh order %d, of the restricted all-rows order %d (all rows: %d), ratio %.3f" % (name, nW, band_f, band_s, all_band, ratio))
    assert sorted(rows_s) == sorted(rows_f) and len(rows_s) == nW
    assert band_s <= all_band, name
    if 2 * band_f < nW:
        assert 2 * band_s < nW, name
    return ratio


def test_the_restricted_order_on_the_constructed_instances():
    worst = 0.0
    for shape in SPARSE_SHAPES:
        fm, _, _, rs, _, _, _ = sparse_instance_of(shape)
        cols = row_columns(fm.to_problem())
        worst = max(worst, _report("shape %r" % (shape,), cols, rs, static_order(cols)[1]))
    print("largest ratio restricted / fresh on the constructed instances: %.3f" % worst)


def case118_families():
    """The case118-sized expression ACOPF with the four working-set families of DESIGN.md ("KKT solve: the sparse form", the static order):
    (row column sets, [(name, row_state)])."""
    pr = acopf.function_model(acopf.synthetic_case("case118", 1, 0.5), nlp="expr").to_problem("case118-sized")
    eq = np.asarray(pr.g_L) == np.asarray(pr.g_U)
    E, I = np.nonzero(eq)[0], np.nonzero(~eq)[0]
    rng = np.random.RandomState(3)

    def state(e_share, i_share):
        rs = np.zeros(pr.m, np.int32)
        rs[E if e_share == 1.0 else rng.choice(E, int(round(e_share * len(E))), replace=False)] = 1
        if i_share:
            rs[rng.choice(I, int(round(i_share * len(I))), replace=False)] = 1
        return rs
    fams = [("all equalities", state(1.0, 0.0)), ("equalities + 1 % of the inequalities", state(1.0, 0.01)),
            ("equalities + 10 % of the inequalities", state(1.0, 0.10)), ("90 % of the equalities + 5 % of the inequalities", state(0.9, 0.05))]
    return row_columns(pr), fams


def test_the_restricted_order_on_the_case118_sized_acopf():
    cols, fams = case118_families()
    all_band = static_order(cols)[1]
    assert len(cols) == 1725
    worst = max(_report("case118-sized, " + name, cols, rs, all_band) for name, rs in fams)
    print("largest ratio restricted / fresh on the case118-sized ACOPF: %.3f (a record, not a gate)" % worst)
