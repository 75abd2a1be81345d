"""Lifetime of the null-space form's state on a handle, through the C ABI: the form exists exactly while the handle holds a skeleton that
qualifies for it, its k-sized buffers are made by the first LP that uses it and re-made when the null space outgrows them, and a handle
that has been through any such sequence solves like a fresh one, bit for bit.

Skeletons: equality_rich_subproblem(seed, 96, 80, 48) qualifies (80 hard equality rows >= 64, n - nE = 16 <= 0.3 * 128, 4 entries per
row, n <= Mp = 128; the CPU oracle solves seeds 3, 4, 5 OPTIMAL in the null-space form with 11, 11, 9 null-space iterations, the basis
columns selected from scratch in the first LP and re-used in the second); random_subproblem(7, 96, 48) is dense and does not."""
import ctypes as C

import numpy as np
import pytest

from tests.util import random_subproblem, equality_rich_subproblem
from tests.util import abi_create as _create, abi_setup as _setup, abi_set_bounds as _set_bounds, abi_solve as _solve

pytestmark = pytest.mark.gpu

N_E, K_SMALL = 80, 16


def _small(seed):
    return equality_rich_subproblem(seed, 96, N_E, 48)


def _dense():
    return random_subproblem(7, 96, 48)


def _stretch(lib, h, sp, capable):
    """The solves that follow a set-up: two normal-phase LPs when the skeleton qualifies (the second re-uses the basis of the first), one
    when it does not, then a restoration LP.  Returns the outputs; checks what the statistics say about the form."""
    outs = []
    for q in range(2 if capable else 1):
        out, st = _solve(lib, h, sp)
        assert out[0] == 1, (q, out[0])
        if capable:
            assert st['ns_dim'] == sp['n'] - N_E and st['ns_cold'] == (1 if q == 0 else 0), (q, st)
            assert q > 0 or st['ns_iters'] > 0, st
        else:
            assert st['ns_dim'] == 0 and st['ns_iters'] == 0 and st['ns_cold'] == 0, st
        outs.append(out)
    out, st = _solve(lib, h, sp, 1)
    assert st['ns_dim'] == 0 and st['ns_iters'] == 0, st        # a restoration LP has slack columns: the form is not used
    outs.append(out)
    return outs


_FRESH = {}


def _fresh(lib, key):
    """The stretch of a fresh handle on skeleton `key` (a seed of the small capable skeleton, or 'dense'): computed once per session."""
    if key not in _FRESH:
        sp = _dense() if key == 'dense' else _small(key)
        g = _create(lib)
        try:
            assert _setup(lib, g, sp) == 0
            _FRESH[key] = _stretch(lib, g, sp, key != 'dense')
        finally:
            lib.asm_destroy(g)
    return _FRESH[key]


def _row_order(lib, h):
    band, n_e, e_band = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert lib.asm_sublp_row_order(h, None, C.byref(band), None, C.byref(n_e), C.byref(e_band)) == 0
    return n_e.value, e_band.value


def test_form_exists_only_with_a_capable_skeleton(hip_lib):
    """asm_sublp_row_order reports no equality rows before any set-up, the 80 of the capable skeleton after its set-up (in an order that is a
    permutation of them), and none again after a rejected set-up, which leaves the handle without a skeleton."""
    from activesetmethods_amd import _lib
    lib = hip_lib
    sp, dn = _small(3), _dense()
    free = dict(dn); free['c_lb'] = dn['c_lb'].copy(); free['c_ub'] = dn['c_ub'].copy()
    free['c_lb'][0], free['c_ub'][0] = -np.inf, np.inf
    bad_row = dict(dn); bad_row['j_row'] = dn['j_row'].copy(); bad_row['j_row'][0] = dn['m'] + 1
    x = np.zeros(2 * (sp['n'] + sp['m']))
    st = C.c_int32(0)
    h = _create(lib)
    try:
        assert _row_order(lib, h) == (0, 0)
        for rejected, rc in ((free, -11), (bad_row, -1)):      # ASM_ERR_UNSUPPORTED (free row), ASM_ERR_ARG (j_row out of range)
            assert _setup(lib, h, sp) == 0
            n_e, e_band = _row_order(lib, h)
            assert n_e == N_E and 0 <= e_band < N_E
            e_rows, band = np.full(N_E, -1, np.int32), C.c_int64(0)
            assert lib.asm_sublp_row_order(h, None, C.byref(band), _lib.i32ptr(e_rows), C.byref(C.c_int64(0)), C.byref(C.c_int64(0))) == 0
            assert np.array_equal(np.sort(e_rows), np.arange(N_E))      # (the first 80 rows are the equality rows)
            assert _setup(lib, h, rejected) == rc
            assert _row_order(lib, h) == (0, 0)
            assert lib.asm_sublp_solve_resident(h, 0.4, 0, *[_lib.dptr(x)] * 5, C.byref(st)) == -3     # ASM_ERR_STATE
        assert _setup(lib, h, dn) == 0
        assert _row_order(lib, h) == (0, 0)
    finally:
        lib.asm_destroy(h)


def test_form_comes_and_goes_with_the_skeleton(hip_lib):
    """Capable, not capable, capable again on one handle: after every set-up the solves equal a fresh handle's bit for bit, and within each
    capable stretch the basis columns are selected from scratch in the first LP only."""
    lib = hip_lib
    h = _create(lib)
    try:
        for step, key in enumerate((3, 'dense', 3, 4)):
            sp = _dense() if key == 'dense' else _small(key)
            assert _setup(lib, h, sp) == 0
            assert _row_order(lib, h)[0] == (0 if key == 'dense' else N_E), step
            assert _stretch(lib, h, sp, key != 'dense') == _fresh(lib, key), step
    finally:
        lib.asm_destroy(h)


def test_k_sized_buffers_across_a_regrow_and_a_new_skeleton(hip_lib):
    """The null space outgrows its first reservation (130 of 560 columns fixed: k = 30 or 31; then free: k = 160), the k-sized buffers are
    re-made; the next set-up on the handle replaces the form with the small skeleton's, whose solves equal a fresh handle's bit for bit;
    destroying the handle releases both."""
    lib = hip_lib
    sp3 = equality_rich_subproblem(90, 560, 400, 200)
    fix = np.random.default_rng(90).choice(sp3['n'], 130, replace=False)
    a3 = dict(sp3); a3['v_lb'] = sp3['v_lb'].copy(); a3['v_ub'] = sp3['v_ub'].copy()
    a3['v_lb'][fix] = a3['v_ub'][fix] = (sp3['x_k'] + sp3['p_star'])[fix]          # fixed where the generator's feasible step puts them
    h = _create(lib)
    try:
        assert _setup(lib, h, a3) == 0
        out, st = _solve(lib, h, a3)
        assert out[0] == 1 and st['ns_dim'] in (30, 31) and st['ns_iters'] > 0 and st['ns_cold'] == 1, st
        assert _set_bounds(lib, h, sp3) == 0
        out, st = _solve(lib, h, sp3)
        assert out[0] == 1 and st['ns_dim'] == 160 and st['ns_iters'] > 0 and st['ns_cold'] == 1, st      # (30 retained columns are no basis of 160)
        sp = _small(4)
        assert _setup(lib, h, sp) == 0
        assert _stretch(lib, h, sp, True) == _fresh(lib, 4)
    finally:
        assert lib.asm_destroy(h) == 0


def test_set_bounds_and_set_ns_basis_keep_the_form(hip_lib):
    """asm_sublp_set_bounds and asm_sublp_set_ns_basis between two LPs of the small skeleton: the resident basis is forgotten, the form and
    its basis columns stay in use.  On a handle whose skeleton does not qualify both calls succeed and change nothing: the next solves
    equal a fresh handle's bit for bit."""
    from activesetmethods_amd import _lib
    lib = hip_lib
    sp = _small(5)
    h = _create(lib)
    try:
        assert _setup(lib, h, sp) == 0
        out1, st = _solve(lib, h, sp)
        assert out1[0] == 1 and st['ns_dim'] == K_SMALL and st['ns_iters'] > 0 and st['ns_cold'] == 1, st
        k = C.c_int64(0)
        J = np.full(sp['n'], -1, np.int32)
        assert lib.asm_sublp_ns_basis(h, _lib.i32ptr(J), C.byref(k)) == 0 and k.value == K_SMALL
        assert _set_bounds(lib, h, sp) == 0
        assert _row_order(lib, h)[0] == N_E
        out2, st = _solve(lib, h, sp)
        assert out2[0] == 1 and st['ns_dim'] == K_SMALL and st['ns_iters'] > 0 and st['ns_cold'] == 0, st
        assert lib.asm_sublp_set_ns_basis(h, _lib.i32ptr(J), K_SMALL) == 0
        assert _set_bounds(lib, h, sp) == 0
        out3, st = _solve(lib, h, sp)
        assert out3[0] == 1 and st['ns_dim'] == K_SMALL and st['ns_iters'] > 0 and st['ns_cold'] == 0, st
        assert out3 == out2                       # the same columns, the same LP, no retained working set either time
        assert lib.asm_sublp_set_ns_basis(h, _lib.i32ptr(J), K_SMALL) == 0      # alone: the retained working set stays, so does the form
        out4, st = _solve(lib, h, sp)
        assert out4[0] == 1 and st['ns_dim'] == K_SMALL and st['ns_cold'] == 0, st
    finally:
        lib.asm_destroy(h)
    dn = _dense()
    h = _create(lib)
    try:
        assert _setup(lib, h, dn) == 0
        before = _stretch(lib, h, dn, False)
        J3 = np.arange(3, dtype=np.int32)
        assert _set_bounds(lib, h, dn) == 0 and lib.asm_sublp_set_ns_basis(h, _lib.i32ptr(J3), 3) == 0
        assert _row_order(lib, h) == (0, 0)
        assert _stretch(lib, h, dn, False) == before == _fresh(lib, 'dense')
    finally:
        lib.asm_destroy(h)
