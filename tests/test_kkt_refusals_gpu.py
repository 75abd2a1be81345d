"""What the KKT column family refuses, entry by entry through the C ABI (include/asm_hip.h): asm_kkt_solve(_multi), asm_kkt_step(_multi),
asm_solution_sensitivity(_multi), asm_bound_sensitivity_multi, asm_solution_adjoint(_multi) on a handle and asm_batch_kkt_solve,
asm_batch_solution_sensitivity, asm_batch_bound_sensitivity, asm_batch_solution_adjoint on a batch of two slots.  The instance is hs071
with two data parameters (n = 4, m = 2), working set [1, 1] / [-1, 0, 0, 0].  Every case is one bad argument, or two to pin which
refusal wins, and asserts the return code and the whole last-error text.  The per-handle and the batch entries share their argument
checks: what only one of them says (the batch's "n_scen < 1 or nrhs < 1", its check of par before any fiber starts) and the order of
the refusals are part of the table.  No case passes a pointer that is read before it is checked, and almost none launches anything."""
import ctypes as C

import numpy as np
import pytest

from activesetmethods_amd import _lib, batch
from tests.test_batch_sens_cpu import hs071_scenario_models
from tests.test_nlparams_gpu import _handle_for

pytestmark = pytest.mark.gpu
ERR_ARG = -1
D, I = _lib.dptr, _lib.i32ptr
N, M, ND, K, NS = 4, 2, 2, 2, 2
NULL_PTR, NRHS, ROW = "null pointer", "nrhs < 1", "a row index outside [0, m)"
RADIUS, SHARE, PAR, SCEN = "a radius is not > 0", "normal_share outside (0, 1]", "max_iter < 0 or rtol not >= 0", "n_scen < 1 or nrhs < 1"


class _Arrays:
    """The valid arguments of every entry: `lead` leading scenarios (0: per handle), K columns.  The arrays live as long as this object."""

    def __init__(self, x0, lead):
        rng = np.random.default_rng(41)
        s = (lead,) if lead else ()
        f8 = lambda *shape: np.ascontiguousarray(rng.standard_normal(s + shape))
        self.x = np.ascontiguousarray(np.stack(x0[:lead]) if lead else x0[0]) + 0.1
        self.lam = f8(M)
        self.rs = np.ones(s + (M,), np.int32)
        self.bs = np.ascontiguousarray(np.broadcast_to(np.array([-1, 0, 0, 0], np.int32), s + (N,)))
        self.ru, self.rw, self.dc = f8(N), f8(M), np.array([1.0, 0.0])
        self.RU, self.RW, self.DC = f8(K, N), f8(K, M), np.eye(ND)
        self.rows, self.delta, self.radius = np.array([1, 0], np.int32), np.array([0.5, 2.0]), np.array([0.7, 1.5])
        self.DX, self.DLAM, self.DZ, self.OUT = f8(K, N), f8(K, M), f8(K, N), f8(K, ND)
        count = K * max(lead, 1)
        self.info, self.sinfo = (_lib.KktInfo * count)(), (_lib.KktStepInfo * count)()

    def point(self):
        return [("x", D(self.x)), ("lambda", D(self.lam)), ("row_state", I(self.rs)), ("bound_state", I(self.bs))]

    def out(self, info=None):
        return [("par", None), ("DX", D(self.DX)), ("DLAM", D(self.DLAM)), ("DZ", D(self.DZ)), ("info", self.info if info is None else info)]

    def adjoint_out(self):
        return [("par", None), ("OUT", D(self.OUT)), ("DBOUND", None), ("AX", None), ("AL", None), ("info", self.info)]


def _handle_entries(a):
    """name -> ordered (argument name, valid value) pairs after the handle."""
    p, nrhs = a.point(), [("nrhs", K)]
    given1, given = [("RU", D(a.ru)), ("RW", D(a.rw))], [("RU", D(a.RU)), ("RW", D(a.RW))]
    return {
        "asm_kkt_solve": p + given1 + a.out(),
        "asm_solution_sensitivity": p + [("DC", D(a.dc))] + a.out(),
        "asm_kkt_solve_multi": p + nrhs + given + a.out(),
        "asm_solution_sensitivity_multi": p + nrhs + [("DC", D(a.DC))] + a.out(),
        "asm_bound_sensitivity_multi": p + nrhs + [("rows", I(a.rows)), ("delta", D(a.delta))] + a.out(),
        "asm_solution_adjoint": p + given1 + a.adjoint_out(),
        "asm_solution_adjoint_multi": p + nrhs + given + a.adjoint_out(),
        "asm_kkt_step": p + given1 + [("radius", C.c_double(0.7))] + a.out(a.sinfo),
        "asm_kkt_step_multi": p + nrhs + given + [("RADIUS", D(a.radius))] + a.out(a.sinfo),
    }


def _batch_entries(a):
    p, given = [("n_scen", NS)] + a.point() + [("nrhs", K)], [("RU", D(a.RU)), ("RW", D(a.RW))]
    return {
        "asm_batch_kkt_solve": p + given + a.out(),
        "asm_batch_solution_sensitivity": p + [("DC", D(a.DC)), ("dc_per_scenario", 0)] + a.out(),
        "asm_batch_bound_sensitivity": p + [("rows", I(a.rows)), ("delta", D(a.delta))] + a.out(),
        "asm_batch_solution_adjoint": p + given + a.adjoint_out(),
    }


class _Kept:
    """A pointer argument with what it points into."""

    def __init__(self, ptr, target):
        self.ptr, self.target = ptr, target


def _rows(*idx):
    keep = np.array(idx, np.int32)
    return _Kept(I(keep), keep)


def _vec(*vals):
    keep = np.array(vals, np.float64)
    return _Kept(D(keep), keep)


def _step_par(share):
    keep = _lib.KktStepParams(50, 1e-10, share)
    return _Kept(C.byref(keep), keep)


def _bad_par():
    keep = _lib.KktParams(-1, 1e-10)
    return _Kept(C.byref(keep), keep)


def _cases(entries, batch_entry):
    """(entry, {argument: bad value}, the name in the message, the message after it).  The same faults for every entry that has the argument."""
    out = []
    for name, args in entries.items():
        names = [k for k, _ in args]
        adjoint, step = "adjoint" in name, "step" in name
        multi = "nrhs" in names
        first = SCEN if batch_entry else NRHS                               # (what nrhs = 0 is called)
        # the single sensitivity and adjoint entries solve through asm_kkt_solve: what the face refuses carries that name
        face = "asm_kkt_solve" if name in ("asm_solution_sensitivity", "asm_solution_adjoint") else name
        for k in ("x", "lambda", "row_state", "bound_state", "info", "RU", "RW", "DC", "rows", "RADIUS") + (("OUT",) if adjoint else ("DX", "DLAM")):
            if k in names:
                out.append((name, {k: None}, NULL_PTR))
        if multi:
            out.append((name, {"nrhs": 0}, first))
            out.append((name, {"nrhs": -3}, first))
            out.append((name, {"nrhs": 0, "x": None}, first))                # two faults: the count before the pointers
        if "rows" in names:
            out.append((name, {"rows": _rows(-1, 0)}, ROW))
            out.append((name, {"rows": _rows(0, M)}, ROW))
            out.append((name, {"rows": _rows(0, M), "x": None}, NULL_PTR))   # the pointers before the indices
            # per handle the entry point refuses a null rows before everything else; the batch counts first
            out.append((name, {"rows": None, "nrhs": 0}, SCEN if batch_entry else NULL_PTR))
        if step:
            rad = "RADIUS" if multi else "radius"
            zero = _vec(0.7, 0.0) if multi else C.c_double(0.0)
            neg = _vec(-1.0, 0.7) if multi else C.c_double(-1.0)
            out.append((name, {rad: zero}, RADIUS))
            out.append((name, {rad: neg}, RADIUS))
            out.append((name, {"par": _step_par(0.0)}, SHARE))
            out.append((name, {"par": _step_par(1.5)}, SHARE))
            out.append((name, {rad: zero, "par": _step_par(0.0)}, RADIUS))   # the radii before the share
            out.append((name, {rad: zero, "x": None}, NULL_PTR))             # the pointers before the radii
            out.append((name, {"par": _step_par(0.0), "DX": None}, NULL_PTR))
        else:
            out.append((name, {"par": _bad_par()}, PAR, face))
            out.append((name, {"par": _bad_par(), "x": None}, NULL_PTR))     # the pointers before par
            if multi:
                out.append((name, {"par": _bad_par(), "nrhs": 0}, first))
        if batch_entry:
            out.append((name, {"n_scen": 0}, SCEN))
            out.append((name, {"n_scen": -1}, SCEN))
            out.append((name, {"n_scen": 0, "x": None}, SCEN))
            out.append((name, {"n_scen": 3}, "3 scenarios, the scenario data table has 2"))
            out.append((name, {"n_scen": 3, "par": _bad_par()}, PAR))        # par before the height of the table
        if "dc_per_scenario" in names:
            for bad in (2, -1):
                out.append((name, {"dc_per_scenario": bad}, "dc_per_scenario is neither 0 nor 1"))
            out.append((name, {"dc_per_scenario": 2, "n_scen": 0}, "dc_per_scenario is neither 0 nor 1"))
    return [c if len(c) == 4 else c + (c[0],) for c in out]


def _call(fn, owner, args, change):
    vals = []
    for k, v in args:
        v = change.get(k, v)
        vals.append(v.ptr if isinstance(v, _Kept) else v)
    return fn(owner, *vals)


def _case_id(case):
    return "%s-%s" % (case[0], "+".join("%s" % k for k in case[1]))


@pytest.fixture(scope="module")
def problems():
    fms = hs071_scenario_models(NS)
    return fms, [fm.to_problem("hs071 scenario %d" % s) for s, fm in enumerate(fms)]


@pytest.fixture(scope="module")
def on_handle(problems):
    fms, prs = problems
    assert (prs[0].n, prs[0].m) == (N, M)
    opt = _handle_for(prs[0], fms[0])
    a = _Arrays([p.x0 for p in prs], 0)
    entries = _handle_entries(a)
    lib = opt._lib
    for name, args in entries.items():                                      # the table's starting point: every entry takes its valid arguments
        assert _call(getattr(lib, name), opt._h, args, {}) == 0, (name, lib.asm_last_error(opt._h))
    yield lib, opt, entries
    for name, args in entries.items():                                      # and still does after every refusal
        assert _call(getattr(lib, name), opt._h, args, {}) == 0, (name, lib.asm_last_error(opt._h))
    opt.close()


@pytest.fixture(scope="module")
def on_batch(problems):
    fms, prs = problems
    hb = batch.HipBatch(prs[0], NS)
    hb.set_scenario_data(hb.scenario_data(prs))
    a = _Arrays([p.x0 for p in prs], NS)
    entries = _batch_entries(a)
    lib = _lib.load()
    for name, args in entries.items():
        assert _call(getattr(lib, name), hb._b, args, {}) == 0, (name, lib.asm_batch_last_error(hb._b))
    yield lib, hb, entries
    for name, args in entries.items():
        assert _call(getattr(lib, name), hb._b, args, {}) == 0, (name, lib.asm_batch_last_error(hb._b))
    hb.close()


def _names_only(make):
    """The entries with arrays of zeros: the case tables are made at collection from the argument names, the arguments in the fixtures."""
    return make(_Arrays([np.zeros(N)] * NS, NS if make is _batch_entries else 0))


HANDLE_CASES = _cases(_names_only(_handle_entries), False)
BATCH_CASES = _cases(_names_only(_batch_entries), True)


@pytest.mark.parametrize("case", HANDLE_CASES, ids=_case_id)
def test_a_handle_entry_refuses(on_handle, case):
    lib, opt, entries = on_handle
    name, change, text, who = case
    rc = _call(getattr(lib, name), opt._h, entries[name], change)
    assert (rc, lib.asm_last_error(opt._h).decode()) == (ERR_ARG, "%s: %s" % (who, text))


@pytest.mark.parametrize("case", BATCH_CASES, ids=_case_id)
def test_a_batch_entry_refuses(on_batch, case):
    lib, hb, entries = on_batch
    name, change, text, who = case
    ops = hb.stats()["ops"]
    rc = _call(getattr(lib, name), hb._b, entries[name], change)
    assert (rc, lib.asm_batch_last_error(hb._b).decode()) == (ERR_ARG, "%s: %s" % (who, text))
    assert hb.stats()["ops"] == ops                                         # refused on the calling thread: no fiber ran


def test_the_tables_cover_the_family():
    assert {c[0] for c in HANDLE_CASES} == set(_names_only(_handle_entries)) and {c[0] for c in BATCH_CASES} == set(_names_only(_batch_entries))
    faults = {k for c in HANDLE_CASES + BATCH_CASES for k in c[1]}
    assert {"x", "DX", "info", "lambda", "nrhs", "RU", "DC", "rows", "radius", "RADIUS", "par", "n_scen", "dc_per_scenario"} <= faults
    assert sum(len(c[1]) == 2 for c in HANDLE_CASES) >= 9 and sum(len(c[1]) == 2 for c in BATCH_CASES) >= 4
