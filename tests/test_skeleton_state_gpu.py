"""Lifetime of the LP skeleton on a handle, through the C ABI: everything asm_sublp_setup makes - dimensions, buffers, factors, validity
flags, band data, uploaded inputs, retained working sets - belongs to one skeleton that the next set-up replaces as a whole.  A handle
that has been through any sequence of set-ups, test hooks and failed set-ups solves like a fresh one, bit for bit: every solve's raw
outputs and its asm_solve_stats (wall time aside) are compared with the same solve on a new handle.

Skeletons: B(seed) = banded_subproblem(seed, 260, 400, 80, 20): M = 420 >= 256 with 20 range rows, sparse (16 nnz <= M n), row band 43 / 23
and column band 25 / 24 for seeds 3 / 4 (CPU oracle), column form available (n <= 0.8 M) - sparse copy, both orders, range-row copies and
the column form are all live; D = random_subproblem(7, 96, 48) is dense and row-major (the fast assembly, no sparse copy, no order, no
column form); R is D with 5 range rows (dense, sorted assembly plan); the shapes of edge_case_subproblems() have M = 0, n = 1, rows
without entries.  The CPU oracle solves the normal and the restoration LP of B, D and R OPTIMAL, B's restoration LP in 9 to 10
column-form iterations."""
import ctypes as C

import numpy as np
import pytest

from tests.util import random_subproblem, banded_subproblem, edge_case_subproblems, equality_rich_subproblem, NSS_KINDS
from tests.util import abi_create as _create, abi_setup as _setup, abi_set_bounds as _set_bounds, abi_solve as _solve

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -11


def _sp(key):
    if key == 'D':
        return random_subproblem(7, 96, 48)
    if key == 'R':
        return random_subproblem(7, 96, 48, n_range=5)
    if key[0] == 'B':
        return banded_subproblem(key[1], n=260, m=400, neq=80, nrange=20)
    if key == 'Q':
        return equality_rich_subproblem(62, 300, 260, 160)
    return edge_case_subproblems()[key]


def _one(lib, h, sp, feasibility=0):
    out, st = _solve(lib, h, sp, feasibility)
    st.pop('wall_ms')
    return out, st


def _stretch(lib, h, key):
    """The solves that follow a set-up: one normal LP, one restoration LP (the edge shapes: the normal LP only)."""
    sp = _sp(key)
    res = [_one(lib, h, sp)]
    if key == 'D' or key == 'R' or key[0] == 'B':
        assert res[0][0][0] == 1, (key, res[0])
        res.append(_one(lib, h, sp, 1))
        assert res[1][0][0] == 1, (key, res[1])
        if key[0] == 'B':
            assert res[1][1]['col_iters'] > 0, res[1][1]       # the column form of the restoration phase is in use
    if key == 'Q':
        assert res[0][0][0] == 1 and res[0][1]['ns_dim'] > 0, (key, res[0])      # the null-space form is in use
    return res


def _row_order(lib, h, M=0):
    """(band of the row order, number of equality rows of the null-space form, the order itself when M > 0 and there is one)"""
    from activesetmethods_amd import _lib
    band, n_e, e_band = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert lib.asm_sublp_row_order(h, None, C.byref(band), None, C.byref(n_e), C.byref(e_band)) == 0
    perm = np.full(max(M, 1), -1, np.int32)
    if M > 0 and band.value > 0:
        assert lib.asm_sublp_row_order(h, _lib.i32ptr(perm), C.byref(band), None, C.byref(n_e), C.byref(e_band)) == 0
    return band.value, n_e.value, perm.tobytes()


_FRESH = {}


def _fresh(lib, key, again=False):
    """The stretch of a fresh handle on skeleton `key` (again: its second stretch on the same skeleton) and its row order: once per session."""
    if (key, again) not in _FRESH:
        sp = _sp(key)
        g = _create(lib)
        try:
            assert _setup(lib, g, sp) == 0
            order = _row_order(lib, g, sp['m'] + 20 if key[0] == 'B' else 0)
            _FRESH[(key, False)] = (_stretch(lib, g, key), order)
            if again:
                _FRESH[(key, True)] = (_stretch(lib, g, key), order)
        finally:
            lib.asm_destroy(g)
    return _FRESH[(key, again)]


def _setup_and_compare(lib, h, key, what):
    sp = _sp(key)
    assert _setup(lib, h, sp) == 0, what
    fresh, order = _fresh(lib, key)
    if key[0] == 'B':
        assert order[0] > 0, order[:2]                          # the rows have a banded order: band data and row-order buffers are live
        assert _row_order(lib, h, sp['m'] + 20) == order, what
    elif key in ('D', 'R'):
        assert _row_order(lib, h)[0] == 0, what
    assert _stretch(lib, h, key) == fresh, what


def test_banded_dense_and_range_row_skeletons_in_turn(hip_lib):
    """B(3), D, B(4), R, B(3) on one handle: every stretch equals a fresh handle's, the row order is reported for B alone and is the
    fresh handle's."""
    h = _create(hip_lib)
    try:
        for step, key in enumerate((('B', 3), 'D', ('B', 4), 'R', ('B', 3))):
            _setup_and_compare(hip_lib, h, key, step)
    finally:
        assert hip_lib.asm_destroy(h) == 0


def test_edge_shapes_then_a_banded_skeleton(hip_lib):
    """Every edge shape in turn on one handle (no rows, one variable, rows without entries, ...), then B(3)."""
    h = _create(hip_lib)
    try:
        for key in list(edge_case_subproblems()) + [('B', 3)]:
            _setup_and_compare(hip_lib, h, key, key)
    finally:
        assert hip_lib.asm_destroy(h) == 0


def test_kernel_hooks_share_the_skeleton(hip_lib):
    """The kernel hooks make a skeleton of their own and, with asm_test_set_factor(layout 1), a factor buffer in its pool; the band of
    asm_test_set_band goes to the factor they load.  With both settings back at their defaults the next set-up solves like a fresh handle."""
    from activesetmethods_amd import _lib
    lib = hip_lib
    N = 64
    rng = np.random.default_rng(11)
    A = rng.standard_normal((N, N))
    S = np.ascontiguousarray(A @ A.T + 4 * N * np.eye(N))
    Sb = np.ascontiguousarray(np.where(np.abs(np.subtract.outer(np.arange(N), np.arange(N))) <= 8, S, 0.0))       # banded and still SPD (diagonally dominant)
    L = np.zeros((N, N))
    h = _create(lib)
    try:
        _setup_and_compare(lib, h, ('B', 3), 'before')
        assert lib.asm_test_set_factor(h, 1, 0, 0, 0.0, 0.0, 1e-14) == 0
        assert lib.asm_test_cholesky(h, _lib.dptr(S), N, _lib.dptr(L)) == 0
        assert np.abs(L @ L.T - S).max() <= 1e-10 * np.abs(S).max()
        assert lib.asm_test_set_band(h, 8) == 0
        assert lib.asm_test_cholesky(h, _lib.dptr(Sb), N, _lib.dptr(L)) == 0
        assert np.abs(L @ L.T - Sb).max() <= 1e-10 * np.abs(Sb).max()
        assert lib.asm_test_set_factor(h, 0, 0, 0, 0.0, 0.0, 1e-14) == 0 and lib.asm_test_set_band(h, 0) == 0
        _setup_and_compare(lib, h, ('B', 3), 'after')
    finally:
        assert lib.asm_destroy(h) == 0


def test_ns_setup_hook_shares_the_skeleton(hip_lib):
    """asm_test_ns_setup_stages works on the skeleton's own null-space form: it re-scales the Jacobian with unit column scale, makes the k-sized
    buffers for the reservation it is given and leaves basis rows, factors and the cold selection's blocks behind.  Q =
    equality_rich_subproblem(62, 300, 260, 160) has the form (k = 40 with every column free).  The next set-up solves like a fresh handle."""
    from activesetmethods_amd import _lib
    lib = hip_lib
    sp = _sp('Q')
    n, k = sp['n'], 40
    h = _create(lib)
    try:
        _setup_and_compare(lib, h, 'Q', 'before')
        dE, fm = np.ascontiguousarray(sp['dE'], dtype=np.float64), np.ones(n)
        lay, grid, res, out = np.zeros(16, np.int64), np.zeros(1, np.uint32), np.zeros(1, np.int32), np.full(4 + n, -1, np.int32)
        st = (_lib.NssStage * 1)(_lib.NssStage(NSS_KINDS.index("setup"), 0, 0.0))      # ASM_NSS_SETUP
        assert lib.asm_test_ns_setup_stages(h, _lib.dptr(dE), _lib.dptr(fm), k, k + 17, None, _lib.i64ptr(lay), None, None, None, None, None, None, None, None, None, None,
                                            0, None, 0, st, 1, grid.ctypes.data_as(C.POINTER(C.c_uint32)), _lib.i32ptr(res), _lib.i32ptr(out)) == 0, lib.asm_last_error(h)
        assert res[0] == 1 and tuple(out[:4]) == (3, k, 0, k)      # a cold set-up with k basis columns
        _setup_and_compare(lib, h, 'Q', 'after')
        _setup_and_compare(lib, h, ('B', 3), 'another skeleton')
    finally:
        assert lib.asm_destroy(h) == 0


def test_failed_setups(hip_lib):
    """A set-up rejected for its arguments leaves the skeleton in use; one rejected later (a free row) leaves the handle without a
    skeleton: every entry that needs one answers ASM_ERR_STATE, the reading entries answer as on a new handle - the previous problem's
    active set and basis columns are gone with it (new with the skeleton as one owner) -, and the next good set-up solves like a fresh handle."""
    from activesetmethods_amd import _lib
    lib = hip_lib
    sp = _sp(('B', 3))
    n, m = sp['n'], sp['m']
    h = _create(lib)
    try:
        _setup_and_compare(lib, h, ('B', 3), 'first')
        bad = dict(sp); bad['n'] = 0
        assert _setup(lib, h, bad) == ERR_ARG
        assert _stretch(lib, h, ('B', 3)) == _fresh(lib, ('B', 3), again=True)[0]
        free = dict(sp); free['c_lb'] = sp['c_lb'].copy(); free['c_ub'] = sp['c_ub'].copy()
        free['c_lb'][0], free['c_ub'][0] = -np.inf, np.inf
        assert _setup(lib, h, free) == ERR_UNSUPPORTED
        x = np.zeros(2 * (n + m + 20) + len(sp['dE']))
        xi = np.zeros(n + m + 20, np.int32)
        zi = np.zeros(8, np.int64)
        d, st = _lib.dptr(x), C.byref(C.c_int32(0))
        assert lib.asm_sublp_solve(h, d, d, 0.0, d, d, 0.4, 0, d, d, d, d, d, st) == ERR_STATE
        assert _set_bounds(lib, h, sp) == ERR_STATE
        assert lib.asm_lp_solve(h, d, d, d, d, d, 0, d, d, d, d, d, d, _lib.i32ptr(xi), st) == ERR_STATE
        i = _lib.i64ptr(zi)
        assert lib.asm_eval_setup(h, 0, i, i, d, i, i, i, d, d, i, i, i, d, i, 1.0, 0, 0, 0, i, 0, d, 0) == ERR_STATE
        assert _row_order(lib, h)[:2] == (0, 0)
        assert lib.asm_sublp_active_set(h, None, None, None, C.byref(C.c_int64(0)), C.byref(C.c_int64(0))) == ERR_STATE       # (new)
        k = C.c_int64(-1)
        assert lib.asm_sublp_ns_basis(h, _lib.i32ptr(xi), C.byref(k)) == 0 and k.value == 0                                  # (new)
        _setup_and_compare(lib, h, 'D', 'after the failure')
    finally:
        assert lib.asm_destroy(h) == 0


def test_set_bounds_between_two_solves(hip_lib):
    """asm_sublp_set_bounds with unchanged row kinds between two LPs of B(3), on a handle that held D before: both solves equal those of
    a fresh handle given the same calls."""
    lib = hip_lib
    sp = _sp(('B', 3))
    runs = []
    for history in (True, False):
        h = _create(lib)
        try:
            if history:
                _setup_and_compare(lib, h, 'D', 'history')
            assert _setup(lib, h, sp) == 0
            first = _one(lib, h, sp)
            assert _set_bounds(lib, h, sp) == 0
            runs.append([first, _one(lib, h, sp)])
        finally:
            assert lib.asm_destroy(h) == 0
    assert runs[0] == runs[1]
    assert runs[0][0][0][0] == 1 and runs[0][1][0][0] == 1
