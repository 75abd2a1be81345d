"""CPU checks of the native Trust-Region SLP caller's bindings (include/asm_hip.h: asm_slp_step_quality, asm_slp_run_tr,
asm_batch_slp_run_tr): the header declares them, the ctypes binding covers them with the C layout of asm_slp_tr_info, and the
Python entry points refuse what they cannot run before any device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("asm_slp_step_quality", "asm_slp_run_tr", "asm_batch_slp_run_tr")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asm_hip.h")).read(), flags=re.S)


def test_header_declares_the_trust_region_entries_and_the_binding_covers_them():
    txt = _header()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    from activesetmethods_amd import _lib
    assert set(NEW) <= set(_lib.PROTOTYPES)
    assert _lib.PROTOTYPES["asm_slp_run_tr"][1][2] is ctypes.c_double                       # tr_size after the parameters
    assert _lib.PROTOTYPES["asm_slp_run_tr"][1][-1] == ctypes.POINTER(_lib.SlpTrInfo)
    assert _lib.PROTOTYPES["asm_batch_slp_run_tr"][1][8] is ctypes.c_double
    assert _lib.PROTOTYPES["asm_batch_slp_run_tr"][1][-1] == ctypes.POINTER(_lib.SlpTrInfo)
    assert len(_lib.PROTOTYPES["asm_slp_step_quality"][1]) == 7


def test_tr_info_struct_matches_the_c_layout():
    """asm_slp_tr_info = { double delta; int32_t accepted, rejected, shrunk, expanded; }: 24 bytes, no padding."""
    from activesetmethods_amd import _lib
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*asm_slp_tr_info\s*;", _header()).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert fields == [("delta", "double"), ("accepted", "int32_t"), ("rejected", "int32_t"), ("shrunk", "int32_t"), ("expanded", "int32_t")]
    assert [f[0] for f in _lib.SlpTrInfo._fields_] == [f[0] for f in fields]
    assert ctypes.sizeof(_lib.SlpTrInfo) == 24
    assert [getattr(_lib.SlpTrInfo, f[0]).offset for f in fields] == [0, 8, 12, 16, 20]


def _toy_model(device_eval, with_function_model=True):
    import activesetmethods_amd as A
    from activesetmethods_amd.moi_evaluator import FunctionModel, ScalarFunction
    fm = FunctionModel(2)
    fm.objective = ScalarFunction(0.0, [(1.0, 1)], [(2.0, 1, 1)])
    fm.add_constraint(ScalarFunction(0.0, [(1.0, 1)]), "ge", -2.0)
    fm.add_constraint(ScalarFunction(0.0, [], [(1.0, 1, 2)]), "eq", 1.0)
    pr = fm.to_problem("toy") if with_function_model else A.problems.toy_problem()
    return A.Model.from_problem(pr, A.Parameters(algorithm="Trust Region", device_eval=device_eval))


@pytest.mark.parametrize("device_eval,with_fm", [(False, True), (True, False), (False, False)])
def test_native_optimize_refuses_without_device_evaluation(monkeypatch, device_eval, with_fm):
    """optimize(model, native=True) needs device_eval=True and a FunctionModel: ValueError before any handle is created."""
    from activesetmethods_amd import slp

    def _no_device(*a, **k):
        raise AssertionError("a device handle was requested")
    monkeypatch.setattr(slp, "HipSubOptimizer", _no_device)
    mdl = _toy_model(device_eval, with_fm)
    x0 = mdl.x.copy()
    with pytest.raises(ValueError):
        slp.optimize(mdl, native=True)
    assert mdl.status == -5 and np.array_equal(mdl.x, x0)          # the model is left as it was


def test_batch_dispatch_refuses_an_unknown_algorithm():
    """HipBatch.slp_run takes Line Search and Trust Region; any other name is a ValueError (checked before the library is called)."""
    import activesetmethods_amd as A
    from activesetmethods_amd import batch
    hb = batch.HipBatch.__new__(batch.HipBatch)
    hb.n, hb.m, hb._b = 2, 1, None
    z = lambda k: np.zeros((1, k))
    with pytest.raises(ValueError):
        hb.slp_run(z(1), z(1), z(2), z(2), z(2), A.Parameters(algorithm="Filter"))


def test_native_run_carries_the_trust_region_record():
    from activesetmethods_amd import _lib, batch
    res = _lib.SlpResult()
    res.status, res.iter, res.lp_solves = 0, 7, 8
    tr = _lib.SlpTrInfo(0.05, 5, 2, 3, 1)
    z = np.zeros(2)
    r = batch.NativeRun(res, z, z, z, z, z, tr)
    assert (r.delta, r.accepted, r.rejected, r.shrunk, r.expanded) == (0.05, 5, 2, 3, 1)
    ls = batch.NativeRun(res, z, z, z, z, z)
    assert (ls.delta, ls.accepted, ls.rejected, ls.shrunk, ls.expanded) == (None, None, None, None, None)
