"""CPU checks of the batch Hessian entries (include/asm_hip.h: asm_batch_hessian_structure, asm_batch_hessian_lagrangian,
asm_batch_hessian_product): the header declares them, the built library exports them, the ctypes binding covers them, and the Python
side (HipBatch methods, batch.lagrangian_hessians) is there and checks shapes before any device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("asm_batch_hessian_structure", "asm_batch_hessian_lagrangian", "asm_batch_hessian_product")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asm_hip.h")).read(), flags=re.S)


def test_header_declares_the_entries_the_library_exports_them_and_the_binding_covers_them():
    from activesetmethods_amd import _lib
    txt = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*asm_batch\s*\*" % name, txt), name
        assert hasattr(lib, name), "libasmhip.so does not export %s" % name
        assert name in _lib.PROTOTYPES, name
    i64, dbl = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    assert _lib.PROTOTYPES[NEW[0]] == (ctypes.c_int, [ctypes.c_void_p, i64, i64, i64])
    assert _lib.PROTOTYPES[NEW[1]] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, dbl, dbl, dbl, dbl])              # obj_factor is an array
    assert _lib.PROTOTYPES[NEW[2]] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, dbl, dbl, dbl, dbl, dbl])


def test_python_side_is_there():
    from activesetmethods_amd import batch
    for name in ("hessian_structure", "eval_hessian_lagrangian", "hessian_product"):
        assert callable(getattr(batch.HipBatch, name, None)), name
    assert callable(getattr(batch, "lagrangian_hessians", None))


def test_shapes_are_checked_before_the_c_call():
    """_hessian_args on an object that has only the sizes: a bad shape raises ValueError, a good one gives contiguous float64 arrays and
    one obj_factor per scenario."""
    from activesetmethods_amd import batch
    hb = batch.HipBatch.__new__(batch.HipBatch)          # no device: only n and m are read
    hb.n, hb.m, hb._b = 3, 2, None
    x, lam, v = np.ones((4, 3)), np.ones((4, 2)), np.ones((4, 3))
    S, xa, of, la, va = hb._hessian_args(x[:, ::1], 0.5, lam, v)
    assert S == 4 and of.shape == (4,) and np.all(of == 0.5) and all(a.flags["C_CONTIGUOUS"] and a.dtype == np.float64 for a in (xa, of, la, va))
    assert np.array_equal(hb._hessian_args(x, [1.0, 0.0, 1.0, 0.0], lam)[2], [1.0, 0.0, 1.0, 0.0])
    for bad in (dict(x=np.ones(3)), dict(x=np.ones((4, 2))), dict(x=np.ones((0, 3)), lam=np.ones((0, 2))), dict(lam=np.ones((3, 2))), dict(lam=np.ones(2)),
                dict(obj_factor=np.ones(3)), dict(obj_factor=np.ones((4, 1))), dict(v=np.ones((4, 2))), dict(v=np.ones(3))):
        a = dict(x=x, obj_factor=1.0, lam=lam, v=v)
        a.update(bad)
        with pytest.raises(ValueError):
            hb._hessian_args(a["x"], a["obj_factor"], a["lam"], a["v"])
    for call in (lambda: hb.eval_hessian_lagrangian(np.ones((4, 2)), 1.0, lam), lambda: hb.hessian_product(x, 1.0, lam, np.ones((4, 2)))):
        with pytest.raises(ValueError):
            call()
