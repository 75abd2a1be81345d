"""asm_batch_slp_run_eqp without a device: the prototype of include/asm_hip.h against its ctypes binding, and the argument handling of
HipBatch.slp_run on a stub library - the asm_slp_eqp_params it builds from Parameters, the records it hands out, the algorithms it
refuses."""
import ctypes
import os
import re

import numpy as np
import pytest

import activesetmethods_amd as A
from activesetmethods_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "asm_batch_slp_run_eqp"


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asm_hip.h")).read(), flags=re.S)


def test_prototype_matches_the_header():
    args = [a.strip() for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, _header()).group(1).split(",")]
    res, types = _lib.PROTOTYPES[NAME]
    assert res is ctypes.c_int and len(types) == len(args) == 18
    structs = {"asm_slp_params": _lib.SlpParams, "asm_slp_eqp_params": _lib.SlpEqpParams, "asm_slp_result": _lib.SlpResult,
               "asm_slp_tr_info": _lib.SlpTrInfo, "asm_slp_eqp_info": _lib.SlpEqpInfo}
    for a, t in zip(args, types):
        if "*" not in a:
            assert t is {"double": ctypes.c_double, "int64_t": ctypes.c_int64}[a.split()[0]], a
        elif a.startswith("asm_batch*"):
            assert t is ctypes.c_void_p, a
        elif a.startswith("const double*") or a.startswith("double*"):
            assert t == ctypes.POINTER(ctypes.c_double), a
        else:
            assert t == ctypes.POINTER(structs[a.replace("const ", "").split("*")[0].strip()]), a
    # the per-scenario entry's arguments in its order, behind the batch's leading ones; asm_batch_slp_run_tr's with the parameter record inserted
    tr = _lib.PROTOTYPES["asm_batch_slp_run_tr"][1]
    assert types[:9] == tr[:9] and types[9] == ctypes.POINTER(_lib.SlpEqpParams) and types[10:17] == tr[9:] and types[17] == ctypes.POINTER(_lib.SlpEqpInfo)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)


class _StubLib:
    """Records the batch SLP calls; fills every result record with its scenario index."""

    def __init__(self):
        self.calls = []

    def asm_batch_set_scenario_data(self, *a):
        return 0

    def _fill(self, name, S, args, res, tr=None, eq=None):
        self.calls.append((name, S, args))
        for s in range(S):
            res[s].status, res[s].iter, res[s].lp_solves, res[s].slot = 0, 10 + s, 20 + s, s
            if tr is not None:
                tr[s].delta, tr[s].accepted = 0.5 + s, s
            if eq is not None:
                eq[s].radius, eq[s].attempts, eq[s].accepted = 2.0 + s, 3 + s, 1 + s
        return 0

    def asm_batch_slp_run(self, b, S, *a):
        return self._fill("ls", S, a, a[-1])

    def asm_batch_slp_run_tr(self, b, S, *a):
        return self._fill("tr", S, a, a[-2], a[-1])

    def asm_batch_slp_run_eqp(self, b, S, *a):
        return self._fill("eqp", S, a, a[-3], a[-2], a[-1])


def _stub_batch():
    hb = batch.HipBatch.__new__(batch.HipBatch)
    hb.n, hb.m, hb._b, hb.nlp_kind = 2, 1, None, 0
    hb._lib, hb._C, hb._err = _StubLib(), ctypes, A.AsmHipError
    return hb


def _run(hb, par, S=3):
    z = lambda k: np.zeros((S, k))
    return hb.slp_run(z(1), z(1), z(2), z(2), z(2), par)


def _eqp_record(call):
    name, S, a = call
    assert name == "eqp"
    return a[6], a[7]._obj        # tr_size, the asm_slp_eqp_params behind byref


def test_slp_run_builds_the_eqp_parameters_from_parameters():
    hb = _stub_batch()
    runs = _run(hb, A.Parameters(algorithm="SLP-EQP", tr_size=0.3, max_iter=77, device_eval=True))
    tr_size, ep = _eqp_record(hb._lib.calls[-1])
    assert isinstance(ep, _lib.SlpEqpParams) and tr_size == 0.3
    assert (ep.radius0, ep.radius_max, ep.tol_active, ep.enabled) == (0.3, 1e3, 1e-8, 1)          # eqp_radius None: tr_size
    assert hb._lib.calls[-1][2][5]._obj.max_iter == 77
    assert [r.iter for r in runs] == [10, 11, 12] and [r.slot for r in runs] == [0, 1, 2]
    assert [r.delta for r in runs] == [0.5, 1.5, 2.5] and [r.Delta_E for r in runs] == [2.0, 3.0, 4.0]
    assert [r.eqp_counts["attempts"] for r in runs] == [3, 4, 5] and set(runs[0].eqp_counts) == {k for k, _ in _lib.SlpEqpInfo._fields_ if k != "radius"}
    assert batch.local_stats(runs, 1.0)["iterations"] == 33
    _run(hb, A.Parameters(algorithm="SLP-EQP", eqp_radius=2.5, eqp_radius_max=50.0, eqp_tol_active=1e-6, eqp=False, device_eval=True))
    tr_size, ep = _eqp_record(hb._lib.calls[-1])
    assert tr_size == 0.4 and (ep.radius0, ep.radius_max, ep.tol_active, ep.enabled) == (2.5, 50.0, 1e-6, 0)
    # one mapping for the handle and the batch
    p = A.Parameters(algorithm="SLP-EQP", eqp_radius=0.7)
    one = batch.slp_eqp_params(p)
    assert (one.radius0, one.radius_max, one.tol_active, one.enabled) == (0.7, 1e3, 1e-8, 1)


def test_the_other_drivers_keep_their_entries_and_records():
    hb = _stub_batch()
    ls = _run(hb, A.Parameters(algorithm="Line Search"), S=2)
    tr = _run(hb, A.Parameters(algorithm="Trust Region"), S=2)
    assert [c[0] for c in hb._lib.calls] == ["ls", "tr"]
    assert all(r.delta is None and r.eqp_counts is None and r.Delta_E is None for r in ls)
    assert [r.delta for r in tr] == [0.5, 1.5] and all(r.eqp_counts is None for r in tr)


def test_an_unknown_algorithm_is_refused():
    hb = _stub_batch()
    for name in ("Newton", "SQP", "slp-eqp", ""):
        with pytest.raises(ValueError):
            _run(hb, A.Parameters(algorithm=name))
    # SLP-EQP without device_eval: refused as SlpEQP and optimize(native=True) refuse it; the other two drivers do not ask for it
    with pytest.raises(ValueError, match="device_eval"):
        _run(hb, A.Parameters(algorithm="SLP-EQP"))
    assert hb._lib.calls == []
    assert "SLP-EQP" in batch.NATIVE_ALGORITHMS and len(batch.NATIVE_ALGORITHMS) == 3
