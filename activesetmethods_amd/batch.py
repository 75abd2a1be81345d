"""Scenario batches across GPUs (BASELINE.json configs[4]).

Independent NLP instances are the only data-parallel axis of the path: one SLP run is strictly
sequential.  Scenarios are block-partitioned over ranks (one process per GPU), every rank solves its
own block - `concurrency` scenarios at a time, each on its own handle / HIP stream (stream pool) - with no
data-path collective, and a single all-reduce of a
<= 8-double vector (RCCL over xGMI on the GPU box, gloo in the CPU tests) merges the convergence
statistics at the end: sum{#scenarios, #converged, SLP iterations, LP solves, restoration solves},
max{final inf_pr, final inf_du, wall seconds}."""
import time

import numpy as np

SUM_KEYS = ("scenarios", "converged", "iterations", "lp_solves", "restoration_solves")
MAX_KEYS = ("inf_pr", "inf_du", "wall_s")


def partition(n_items, world, rank):
    """Static block partition: items [lo, hi) of rank `rank` (sizes differ by at most one)."""
    base, rem = divmod(int(n_items), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def local_stats(slps, wall_s):
    s = dict.fromkeys(SUM_KEYS + MAX_KEYS, 0.0)
    for slp in slps:
        s["scenarios"] += 1
        s["converged"] += 1 if slp.ret == 0 else 0
        s["iterations"] += slp.iter
        s["lp_solves"] += slp.lp_solves
        s["restoration_solves"] += sum(1 for r in slp.trace if r["fr"])
        s["inf_pr"] = max(s["inf_pr"], float(slp.prim_infeas) if np.isfinite(slp.prim_infeas) else 0.0)
        s["inf_du"] = max(s["inf_du"], float(slp.dual_infeas) if np.isfinite(slp.dual_infeas) else 0.0)
    s["wall_s"] = float(wall_s)
    return s


def reduce_stats(stats, device=None):
    """All-reduce the statistics over the default process group (no-op without one)."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return dict(stats)
    dev = device if device is not None else "cpu"
    sums = torch.tensor([stats[k] for k in SUM_KEYS], dtype=torch.float64, device=dev)
    maxs = torch.tensor([stats[k] for k in MAX_KEYS], dtype=torch.float64, device=dev)
    dist.all_reduce(sums, op=dist.ReduceOp.SUM)
    dist.all_reduce(maxs, op=dist.ReduceOp.MAX)
    out = {k: float(v) for k, v in zip(SUM_KEYS, sums.tolist())}
    out.update({k: float(v) for k, v in zip(MAX_KEYS, maxs.tolist())})
    return out


def solve_batch(make_model, n_scenarios, rank=0, world=1, run=None, reduce_device=None, concurrency=1):
    """Solve scenarios [lo, hi) of this rank on this rank's GPU; `make_model(s)` returns the Model of scenario s,
    `run(model)` the finished SLP object (default: activesetmethods_amd.optimize).

    `concurrency` > 1 runs that many scenarios at a time, each on its own handle = its own HIP stream, from a pool of
    host threads (the C ABI is re-entrant per handle and releases the GIL): a single case300-sized SLP run is bound by
    the latency of its serial kernel chain and leaves most of the GPU idle, so independent runs overlap almost freely.
    Scenarios are handed to the next free worker in index order (dynamic assignment inside the rank); the results are
    returned in index order and do not depend on the concurrency."""
    if run is None:
        from .slp import optimize as run
    lo, hi = partition(n_scenarios, world, rank)
    t0 = time.perf_counter()
    if concurrency <= 1 or hi - lo <= 1:
        slps = [run(make_model(s)) for s in range(lo, hi)]
    else:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=int(concurrency)) as pool:
            slps = list(pool.map(lambda s: run(make_model(s)), range(lo, hi)))
    st = local_stats(slps, time.perf_counter() - t0)
    return slps, reduce_stats(st, reduce_device)


# ------------------------------------------------------------------------------------------------------------------------------
# Lockstep scenario batch (include/asm_hip.h: asm_batch_*): B scenarios with the same pattern advance through ONE launch sequence
# on one stream, driven by one host thread inside the library (the native SLP driver asm_slp_run per scenario, as fibers).
# ------------------------------------------------------------------------------------------------------------------------------
def slp_params(par, max_lp_solves=0):
    """asm_slp_params from a `Parameters` object (src/parameters.jl:17-28)."""
    from . import _lib
    return _lib.SlpParams(int(par.max_iter), int(max_lp_solves or 0), float(par.tol_direction), float(par.tol_residual), float(par.tol_infeas),
                          float(par.eta), float(par.tau), float(par.min_alpha))


NATIVE_ALGORITHMS = ("Line Search", "Trust Region", "SLP-EQP")      # asm_slp_run, asm_slp_run_tr, asm_slp_run_eqp and their batch forms
KKT_DEFAULT = ("dense", "working-set")                              # what asm_batch_eval_setup starts every batch from (asm_batch_kkt_set_form)


def check_batch_kkt_form(par):
    """The scenario batches run the dense form of the KKT solve, or the sparse form in the static row order (asm_batch_kkt_set_form).  The
    sparse form in the working-set order is per handle only (it orders, uploads and waits at every new working set): a Parameters object
    that asks for it is refused before anything is built or run.  So is the limited-memory Hessian (asm_hessian_set_type)."""
    if getattr(par, "kkt_form", "dense") != "dense" and getattr(par, "kkt_order", "working-set") != "static":
        raise ValueError("Parameters(kkt_form=%r, kkt_order=%r): the scenario batches (asm_batch_*) run the sparse form of the KKT solve in the "
                         "static row order only - the working-set order is per handle (SlpEQP, optimize(native=True), "
                         "HipSubOptimizer.set_kkt_form); give kkt_order=\"static\"" % (par.kkt_form, getattr(par, "kkt_order", "working-set")))
    if getattr(par, "hessian_type", "none") == "limited-memory":
        raise ValueError("Parameters(hessian_type='limited-memory'): the scenario batches (asm_batch_*) use the model's own second derivatives - "
                         "the limited-memory Hessian is per handle (SlpEQP, optimize(native=True), HipSubOptimizer.set_hessian_type)")


def slp_eqp_params(par):
    """asm_slp_eqp_params from a `Parameters` object: `eqp_radius` None is `tr_size` (as SlpEQP)."""
    from . import _lib
    return _lib.SlpEqpParams(float(par.tr_size if par.eqp_radius is None else par.eqp_radius), float(par.eqp_radius_max), float(par.eqp_tol_active),
                             int(bool(par.eqp)))


class NativeRun:
    """Outcome of one native SLP run (asm_slp_result + the final iterate): the attributes `local_stats` and the tests read from an SlpLS.
    Trust Region (`tr`: asm_slp_tr_info) adds the final radius `delta` and the step counts `accepted`, `rejected`, `shrunk`, `expanded`;
    they are None for Line Search.  SLP-EQP (`eqp`: asm_slp_eqp_info) adds `eqp_counts` and the final radius `Delta_E` of its step, as SlpEQP
    names them; None otherwise."""

    def __init__(self, res, x, lam, mult_x_U, mult_x_L, g, tr=None, eqp=None):
        self.ret, self.iter, self.lp_solves = int(res.status), int(res.iter), int(res.lp_solves)
        self.restoration_solves, self.ls_trials, self.slot = int(res.restoration_solves), int(res.ls_trials), int(res.slot)
        self.paths = [int(v) for v in res.paths]
        self.ipm_iters, self.ns_cold = int(res.ipm_iters), int(res.ns_cold)
        self.obj_val, self.prim_infeas, self.dual_infeas, self.compl = float(res.obj_val), float(res.prim_infeas), float(res.dual_infeas), float(res.compl_)
        self.x, self.lam, self.mult_x_U, self.mult_x_L, self.E = x, lam, mult_x_U, mult_x_L, g
        self.trace = [dict(fr=True)] * self.restoration_solves       # (local_stats counts the restoration solves from the trace)
        self.delta = float(tr.delta) if tr is not None else None
        self.accepted, self.rejected, self.shrunk, self.expanded = ((int(tr.accepted), int(tr.rejected), int(tr.shrunk), int(tr.expanded))
                                                                    if tr is not None else (None, None, None, None))
        self.Delta_E = float(eqp.radius) if eqp is not None else None
        self.eqp_counts = ({k: int(getattr(eqp, k)) for k, _ in eqp._fields_ if k != "radius"} if eqp is not None else None)


class HipBatch:
    """`n_slots` sub-problem handles with one LP skeleton and one evaluator on one device, advanced in lockstep (asm_batch_*).
    `problem`: a Problem built from a FunctionModel (its pattern, functions and NLP block are shared by every scenario; scenarios differ in
    bounds and start points, and through a scenario data table in the NLP block's data: slp_run(..., data=...))."""

    def __init__(self, problem, n_slots, device=0, groups=None):
        import ctypes as C
        from . import _lib
        from .subproblem import AsmHipError
        self._lib, self._C, self._err = _lib.load(), C, AsmHipError
        if getattr(problem, "function_model", None) is None:
            raise ValueError("HipBatch needs a problem built from a FunctionModel (the batch evaluates on the device)")
        self.n_slots = int(n_slots)
        self._b = C.c_void_p()
        rc = self._lib.asm_batch_create(int(device), int(n_slots), C.byref(self._b))
        if rc != 0:
            raise AsmHipError("asm_batch_create(device=%d, n_slots=%d) failed with code %d" % (device, n_slots, rc))
        if groups is not None:
            self._check(self._lib.asm_batch_set_groups(self._b, int(groups)))
        self.groups = int(self._lib.asm_batch_groups(self._b))
        self.setup(problem)

    def setup(self, problem):
        """asm_batch_setup + asm_batch_eval_setup with `problem` (built from a FunctionModel) for every slot; on an existing batch: another
        model on the same slots (a scenario data table, the basis columns and the Hessian lists of the earlier model are dropped)."""
        from . import _lib
        from .moi_evaluator import nlp_kind
        fm = getattr(problem, "function_model", None)
        if fm is None:
            raise ValueError("HipBatch needs a problem built from a FunctionModel (the batch evaluates on the device)")
        self.n, self.m = int(problem.n), int(problem.m)
        f64 = lambda a: np.ascontiguousarray(a, np.float64)
        jr, jc = np.ascontiguousarray(problem.j_row, np.int64), np.ascontiguousarray(problem.j_col, np.int64)
        gl, gu, xl, xu = map(f64, (problem.g_L, problem.g_U, problem.x_L, problem.x_U))
        self._check(self._lib.asm_batch_setup(self._b, self.n, self.m, len(jr), _lib.i64ptr(jr), _lib.i64ptr(jc), _lib.dptr(gl), _lib.dptr(gu),
                                              _lib.dptr(xl), _lib.dptr(xu)))
        fl = fm.flatten()
        kind, rows, nnz = 0, 0, 0
        ipar, dpar = np.zeros(1, np.int64), np.zeros(1)
        if fm.nlp is not None:
            kind = nlp_kind(fm.nlp.device)
            _, ipar, dpar = fm.nlp.device
            rows, nnz = fm.nlp.m, len(fm.nlp.rows)
            ipar, dpar = np.ascontiguousarray(ipar, np.int64), np.ascontiguousarray(dpar, np.float64)
        self.nlp_kind, self._ipar, self._dpar = kind, ipar, dpar
        self.n_dpar = len(dpar) if kind else 0
        a = lambda k: fl[k]
        self._check(self._lib.asm_batch_eval_setup(self._b, fl["n_rows"], _lib.i64ptr(a("aff_ptr")), _lib.i64ptr(a("aff_var")), _lib.dptr(a("aff_coef")),
                                                   _lib.i64ptr(a("quad_ptr")), _lib.i64ptr(a("q_v1")), _lib.i64ptr(a("q_v2")), _lib.dptr(a("q_coef")),
                                                   _lib.dptr(a("constant")), _lib.i64ptr(a("jac_off")), _lib.i64ptr(a("g_ptr")), _lib.i64ptr(a("g_kind")),
                                                   _lib.dptr(a("g_coef")), _lib.i64ptr(a("g_other")), float(fl["objective_scale"]), kind, rows, nnz,
                                                   _lib.i64ptr(ipar), len(ipar) if kind else 0, _lib.dptr(dpar), len(dpar) if kind else 0))
        self._kkt = KKT_DEFAULT

    def _check(self, rc):
        if rc != 0:
            raise self._err("libasmhip batch error %d: %s" % (rc, self._lib.asm_batch_last_error(self._b).decode()))

    def close(self):
        if getattr(self, "_b", None):
            self._lib.asm_batch_destroy(self._b)
            self._b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def ns_basis(self):
        from . import _lib
        k = self._C.c_int64(0)
        self._check(self._lib.asm_batch_ns_basis(self._b, None, self._C.byref(k)))
        J = np.zeros(max(int(k.value), 1), np.int32)
        self._check(self._lib.asm_batch_ns_basis(self._b, _lib.i32ptr(J), self._C.byref(k)))
        return J[:int(k.value)]

    def set_ns_basis(self, J):
        from . import _lib
        J = np.ascontiguousarray(J, np.int32)
        self._check(self._lib.asm_batch_set_ns_basis(self._b, _lib.i32ptr(J), len(J)))

    def stats(self):
        from . import _lib
        s = _lib.BatchStats()
        self._check(self._lib.asm_batch_get_stats(self._b, self._C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}

    def set_kkt_form(self, form, order="working-set"):
        """asm_batch_kkt_set_form: the form ("dense" / "sparse") and row order ("working-set" / "static") of the KKT solves of the SLP-EQP
        runs on every slot.  ("sparse", "working-set") is refused: that order is per handle.  setup() starts from dense again."""
        from . import _lib
        if form not in _lib.KKT_FORMS or order not in _lib.KKT_ORDERS:
            raise ValueError("kkt form %r, order %r: expected one of %s and one of %s"
                             % (form, order, ", ".join(map(repr, _lib.KKT_FORMS)), ", ".join(map(repr, _lib.KKT_ORDERS))))
        self._check(self._lib.asm_batch_kkt_set_form(self._b, _lib.KKT_FORMS[form], _lib.KKT_ORDERS[order]))
        self._kkt = (form, order)

    def set_scenario_data(self, data, offset=0):
        """The scenario data table (asm_batch_set_scenario_data): row s of `data` [n_scen x count] is written to dpar[offset, offset + count)
        of the slot that takes scenario s; None clears it (every scenario then starts from the setup data)."""
        from . import _lib
        if data is None:
            self._check(self._lib.asm_batch_set_scenario_data(self._b, 0, 0, 0, None))
            return
        t = np.ascontiguousarray(np.atleast_2d(data), np.float64)
        self._check(self._lib.asm_batch_set_scenario_data(self._b, t.shape[0], int(offset), t.shape[1], _lib.dptr(t)))

    def scenario_data(self, problems):
        """The per-scenario data table of `problems` for this batch: None when every NLP block carries the batch's own data, else their dpar
        stacked (offset 0).  A problem whose NLP block differs in kind or pattern (ipar) cannot share the batch's evaluator: ValueError."""
        if not self.nlp_kind:
            return None
        rows, differ = [], False
        from .moi_evaluator import nlp_kind
        for pr in problems:
            fm = getattr(pr, "function_model", None)
            if fm is None or fm.nlp is None or fm.nlp.device is None:
                raise ValueError("problem %r has no NLP block for the batch's evaluator" % (getattr(pr, "name", pr),))
            _, ipar, dpar = fm.nlp.device
            ipar, dpar = np.asarray(ipar, np.int64), np.asarray(dpar, np.float64)
            if nlp_kind(fm.nlp.device) != self.nlp_kind or not np.array_equal(ipar, self._ipar) or len(dpar) != self.n_dpar:
                raise ValueError("problem %r: its NLP block differs from the batch's in kind or pattern - only its data (dpar) may differ"
                                 % (getattr(pr, "name", pr),))
            differ = differ or not np.array_equal(dpar.view(np.int64), self._dpar.view(np.int64))
            rows.append(dpar)
        return np.stack(rows) if differ else None

    def slp_run(self, g_L, g_U, x_L, x_U, x0, parameters, max_lp_solves=0, data=None, data_offset=0):
        """Complete SLP runs (`parameters.algorithm`: Line Search, Trust Region or SLP-EQP) of `len(g_L)` scenarios (rows of the 2-D arrays):
        list of NativeRun in scenario order.  `data` [n_scen x count]: scenario s solves with dpar[data_offset, data_offset + count) = data[s]
        (the table stays set for data_gradient); None: every scenario with the setup data."""
        from . import _lib
        f64 = lambda a_: np.ascontiguousarray(a_, np.float64)
        g_L, g_U, x_L, x_U, x0 = map(f64, (g_L, g_U, x_L, x_U, x0))
        S = x0.shape[0]
        check_batch_kkt_form(parameters)
        assert g_L.shape == (S, self.m) and g_U.shape == (S, self.m) and x_L.shape == (S, self.n) and x_U.shape == (S, self.n) and x0.shape == (S, self.n)
        if parameters.algorithm not in NATIVE_ALGORITHMS:
            raise ValueError("the native drivers are run!(::SlpLS), run!(::SlpTR) and SLP-EQP, not %r" % parameters.algorithm)
        if parameters.algorithm == "SLP-EQP":
            # what SlpEQP and optimize(native=True) ask of a Parameters object: one that they refuse is refused here too, so the same
            # object selects SLP-EQP on every route or on none (the batch itself always evaluates on the device)
            if not getattr(parameters, "device_eval", False):
                raise ValueError("SLP-EQP needs Parameters(device_eval=True): its trial reads what the device evaluator left in HBM")
        if data is not None and np.atleast_2d(data).shape[0] != S:
            raise ValueError("the data table has %d rows for %d scenarios" % (np.atleast_2d(data).shape[0], S))
        if data is not None or self.nlp_kind:
            self.set_scenario_data(data, data_offset)
        kkt = (getattr(parameters, "kkt_form", "dense"), getattr(parameters, "kkt_order", "working-set"))
        if kkt != getattr(self, "_kkt", KKT_DEFAULT):      # (what the batch has: set_kkt_form, or the set-up's default)
            self.set_kkt_form(*kkt)
        par = slp_params(parameters, max_lp_solves)
        x = np.empty((S, self.n)); lam = np.empty((S, max(self.m, 1))); mU = np.empty((S, self.n)); mL = np.empty((S, self.n)); g = np.empty((S, max(self.m, 1)))
        res = (_lib.SlpResult * S)()
        bounds = (_lib.dptr(g_L), _lib.dptr(g_U), _lib.dptr(x_L), _lib.dptr(x_U), _lib.dptr(x0), self._C.byref(par))
        outs = (_lib.dptr(x), _lib.dptr(lam), _lib.dptr(mU), _lib.dptr(mL), _lib.dptr(g), res)
        tr, eq = [None] * S, [None] * S
        if parameters.algorithm == "SLP-EQP":
            tr, eq = (_lib.SlpTrInfo * S)(), (_lib.SlpEqpInfo * S)()
            ep = slp_eqp_params(parameters)
            self._check(self._lib.asm_batch_slp_run_eqp(self._b, S, *bounds, float(parameters.tr_size), self._C.byref(ep), *outs, tr, eq))
        elif parameters.algorithm == "Trust Region":
            tr = (_lib.SlpTrInfo * S)()
            self._check(self._lib.asm_batch_slp_run_tr(self._b, S, *bounds, float(parameters.tr_size), *outs, tr))
        else:
            self._check(self._lib.asm_batch_slp_run(self._b, S, *bounds, *outs))
        return [NativeRun(res[s], x[s], lam[s, :self.m], mU[s], mL[s], g[s, :self.m], tr[s], eq[s]) for s in range(S)]

    def data_gradient(self, x, lam):
        """asm_batch_data_gradient: d(f - lam' g) / d dpar per scenario (rows of x [n_scen x n], lam [n_scen x m]), each scenario with its
        data (the table of the last slp_run, else the setup data); [n_scen x n_dpar].  For expression blocks and the block kernels with derivatives (for
        the latter the result depends on (x, lam) only: they are linear in their data)."""
        from . import _lib
        x = np.ascontiguousarray(np.atleast_2d(x), np.float64)
        S = x.shape[0]
        lam = np.ascontiguousarray(np.reshape(lam, (S, self.m)) if self.m else np.zeros((S, 1)), np.float64)
        out = np.empty((S, max(self.n_dpar, 1)))
        self._check(self._lib.asm_batch_data_gradient(self._b, S, _lib.dptr(x), _lib.dptr(lam), _lib.dptr(out)))
        return out[:, :self.n_dpar]

    def hessian_structure(self):
        """asm_batch_hessian_structure: the pattern (rows, cols) of the Hessian of the Lagrangian, 1-based int64, the same for every scenario
        (an off-diagonal entry stands for both symmetric positions, duplicates add)."""
        from . import _lib
        nnz = self._C.c_int64(0)
        self._check(self._lib.asm_batch_hessian_structure(self._b, self._C.byref(nnz), None, None))
        rows, cols = np.zeros(max(int(nnz.value), 1), np.int64), np.zeros(max(int(nnz.value), 1), np.int64)
        self._check(self._lib.asm_batch_hessian_structure(self._b, self._C.byref(nnz), _lib.i64ptr(rows), _lib.i64ptr(cols)))
        return rows[:int(nnz.value)], cols[:int(nnz.value)]

    def _hessian_args(self, x, obj_factor, lam, v=None):
        """x [n_scen x n], lam [n_scen x m], obj_factor (scalar or [n_scen]) and v [n_scen x n] as contiguous float64 arrays; ValueError for
        shapes that do not fit the batch."""
        x = np.ascontiguousarray(x, np.float64)
        if x.ndim != 2 or x.shape[1] != self.n or x.shape[0] < 1:
            raise ValueError("x has shape %r, expected [n_scen x %d] with at least one scenario" % (x.shape, self.n))
        S = x.shape[0]
        lam = np.ascontiguousarray(lam, np.float64) if self.m else np.zeros((S, 1))
        if self.m and lam.shape != (S, self.m):
            raise ValueError("lam has shape %r, expected %r" % (lam.shape, (S, self.m)))
        of = np.asarray(obj_factor, np.float64)
        if of.ndim == 0:
            of = np.full(S, float(of))
        if of.shape != (S,):
            raise ValueError("obj_factor has shape %r, expected a scalar or %r" % (of.shape, (S,)))
        of = np.ascontiguousarray(of)
        if v is not None:
            v = np.ascontiguousarray(v, np.float64)
            if v.shape != (S, self.n):
                raise ValueError("v has shape %r, expected %r" % (v.shape, (S, self.n)))
        return S, x, of, lam, v

    def eval_hessian_lagrangian(self, x, obj_factor, lam):
        """asm_batch_hessian_lagrangian: the values [n_scen x nnz] of obj_factor * objective_scale * hess f + sum_i lam_i hess g_i (MOI
        plus-sign convention) per scenario, each with its data (the table of the last slp_run / set_scenario_data, else the setup data);
        `obj_factor`: a scalar or one per scenario."""
        from . import _lib
        S, x, of, lam, _ = self._hessian_args(x, obj_factor, lam)
        nnz = len(self.hessian_structure()[0])
        out = np.empty((S, max(nnz, 1)))
        self._check(self._lib.asm_batch_hessian_lagrangian(self._b, S, _lib.dptr(x), _lib.dptr(of), _lib.dptr(lam), _lib.dptr(out)))
        return out[:, :nnz]

    def hessian_product(self, x, obj_factor, lam, v):
        """asm_batch_hessian_product: H v per scenario, [n_scen x n] (arguments as eval_hessian_lagrangian, v [n_scen x n])."""
        from . import _lib
        S, x, of, lam, v = self._hessian_args(x, obj_factor, lam, v)
        out = np.empty((S, self.n))
        self._check(self._lib.asm_batch_hessian_product(self._b, S, _lib.dptr(x), _lib.dptr(of), _lib.dptr(lam), _lib.dptr(v), _lib.dptr(out)))
        return out

    def _kkt_args(self, x, lam, row_state, bound_state, max_iter, rtol):
        """x [n_scen x n], lam [n_scen x m], row_state [n_scen x m], bound_state [n_scen x n] as contiguous arrays and the asm_kkt_params
        argument; ValueError for shapes that do not fit the batch."""
        from .subproblem import HipSubOptimizer
        x = np.ascontiguousarray(x, np.float64)
        if x.ndim != 2 or x.shape[1] != self.n or x.shape[0] < 1:
            raise ValueError("x has shape %r, expected [n_scen x %d] with at least one scenario" % (x.shape, self.n))
        S = x.shape[0]
        lam = np.ascontiguousarray(lam, np.float64) if self.m else np.zeros((S, 1))
        rs = np.ascontiguousarray(row_state, np.int32) if self.m else np.zeros((S, 1), np.int32)
        bs = np.ascontiguousarray(bound_state, np.int32)
        if self.m and (lam.shape != (S, self.m) or rs.shape != (S, self.m)):
            raise ValueError("lam / row_state have shapes %r / %r, expected %r" % (lam.shape, rs.shape, (S, self.m)))
        if bs.shape != (S, self.n):
            raise ValueError("bound_state has shape %r, expected %r" % (bs.shape, (S, self.n)))
        return S, x, lam, rs, bs, HipSubOptimizer._kkt_params(max_iter, rtol)

    def _kkt_outputs(self, S, nrhs):
        from . import _lib
        return np.empty((S, nrhs, self.n)), np.empty((S, nrhs, max(self.m, 1))), np.empty((S, nrhs, self.n)), (_lib.KktInfo * (S * nrhs))()

    @staticmethod
    def _kkt_result(S, nrhs, m, DX, DLAM, DZ, infos):
        return DX, DLAM[:, :, :m], DZ, [[infos[s * nrhs + c] for c in range(nrhs)] for s in range(S)]

    def kkt_solve_multi(self, x, lam, row_state, bound_state, RU, RW, max_iter=None, rtol=None):
        """(DX [n_scen x nrhs x n], DLAM [n_scen x nrhs x m], DZ [n_scen x nrhs x n], infos[s][c]) of asm_batch_kkt_solve: per scenario
        HipSubOptimizer.kkt_solve_multi - bit for bit what a fresh handle with the scenario's data and the batch's KKT form gives - for
        the rows of x, lam, row_state, bound_state and the right-hand sides RU [n_scen x nrhs x n], RW [n_scen x nrhs x m].  Each
        scenario runs with its data (the table of the last slp_run / set_scenario_data, else the setup data)."""
        from . import _lib
        S, x, lam, rs, bs, par = self._kkt_args(x, lam, row_state, bound_state, max_iter, rtol)
        RU = np.ascontiguousarray(RU, np.float64)
        if RU.ndim != 3 or RU.shape[0] != S or RU.shape[1] < 1 or RU.shape[2] != self.n:
            raise ValueError("RU has shape %r, expected (%d, nrhs, %d) with at least one column" % (RU.shape, S, self.n))
        nrhs = RU.shape[1]
        RW = np.ascontiguousarray(RW, np.float64) if self.m else np.zeros((S, nrhs, 1))
        if self.m and RW.shape != (S, nrhs, self.m):
            raise ValueError("RW has shape %r, expected %r" % (RW.shape, (S, nrhs, self.m)))
        DX, DLAM, DZ, infos = self._kkt_outputs(S, nrhs)
        self._check(self._lib.asm_batch_kkt_solve(self._b, S, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), nrhs, _lib.dptr(RU), _lib.dptr(RW), par,
                                                  _lib.dptr(DX), _lib.dptr(DLAM), _lib.dptr(DZ), infos))
        return self._kkt_result(S, nrhs, self.m, DX, DLAM, DZ, infos)

    def solution_sensitivity_multi(self, x, lam, row_state, bound_state, DC, max_iter=None, rtol=None):
        """asm_batch_solution_sensitivity: per scenario HipSubOptimizer.solution_sensitivity_multi along the directions DC of the NLP block's
        data - [nrhs x n_dpar], the same for every scenario, or [n_scen x nrhs x n_dpar]; the outputs of kkt_solve_multi."""
        from . import _lib
        S, x, lam, rs, bs, par = self._kkt_args(x, lam, row_state, bound_state, max_iter, rtol)
        DC = np.ascontiguousarray(DC, np.float64)
        if DC.ndim not in (2, 3) or DC.shape[-1] != self.n_dpar or DC.shape[-2] < 1 or (DC.ndim == 3 and DC.shape[0] != S):
            raise ValueError("DC has shape %r, expected (nrhs, %d) or (%d, nrhs, %d) with at least one direction" % (DC.shape, self.n_dpar, S, self.n_dpar))
        nrhs, per = DC.shape[-2], int(DC.ndim == 3)
        if not self.n_dpar:
            DC = np.zeros((S, nrhs, 1))
        DX, DLAM, DZ, infos = self._kkt_outputs(S, nrhs)
        self._check(self._lib.asm_batch_solution_sensitivity(self._b, S, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), nrhs, _lib.dptr(DC), per, par,
                                                             _lib.dptr(DX), _lib.dptr(DLAM), _lib.dptr(DZ), infos))
        return self._kkt_result(S, nrhs, self.m, DX, DLAM, DZ, infos)

    def bound_sensitivity(self, x, lam, row_state, bound_state, rows, delta=None, max_iter=None, rtol=None):
        """asm_batch_bound_sensitivity: per scenario HipSubOptimizer.bound_sensitivity_multi for the rows `rows` (0-based, the same for every
        scenario; delta None: unit moves) - column c is the answer to rw[rows[c]] = -delta[c], the zero column where the row is outside the
        scenario's working set; the outputs of kkt_solve_multi."""
        from . import _lib
        S, x, lam, rs, bs, par = self._kkt_args(x, lam, row_state, bound_state, max_iter, rtol)
        rows = np.ascontiguousarray(np.atleast_1d(rows), np.int32)
        if rows.ndim != 1 or len(rows) < 1:
            raise ValueError("rows has shape %r, expected (nrhs,) with at least one row" % (rows.shape,))
        nrhs = len(rows)
        if delta is not None:
            delta = np.ascontiguousarray(np.atleast_1d(delta), np.float64)
            if delta.shape != (nrhs,):
                raise ValueError("delta has shape %r, expected %r" % (delta.shape, (nrhs,)))
        DX, DLAM, DZ, infos = self._kkt_outputs(S, nrhs)
        self._check(self._lib.asm_batch_bound_sensitivity(self._b, S, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), nrhs, _lib.i32ptr(rows),
                                                          None if delta is None else _lib.dptr(delta), par, _lib.dptr(DX), _lib.dptr(DLAM), _lib.dptr(DZ), infos))
        return self._kkt_result(S, nrhs, self.m, DX, DLAM, DZ, infos)

    def solution_adjoint(self, x, lam, row_state, bound_state, GX, GL, max_iter=None, rtol=None):
        """(OUT [n_scen x nrhs x n_dpar], DBOUND [n_scen x nrhs x m], AX [n_scen x nrhs x n], AL [n_scen x nrhs x m], infos[s][c]) of
        asm_batch_solution_adjoint: per scenario HipSubOptimizer.solution_adjoint_multi - bit for bit what a fresh handle with the
        scenario's data and the batch's KKT form gives - for the nrhs functions whose gradients are GX [n_scen x nrhs x n] and
        GL [n_scen x nrhs x m]: the gradient of each with respect to every constant of the block's data and every row bound."""
        from . import _lib
        S, x, lam, rs, bs, par = self._kkt_args(x, lam, row_state, bound_state, max_iter, rtol)
        GX = np.ascontiguousarray(GX, np.float64)
        if GX.ndim != 3 or GX.shape[0] != S or GX.shape[1] < 1 or GX.shape[2] != self.n:
            raise ValueError("GX has shape %r, expected (%d, nrhs, %d) with at least one function" % (GX.shape, S, self.n))
        nrhs = GX.shape[1]
        GL = np.ascontiguousarray(GL, np.float64) if self.m else np.zeros((S, nrhs, 1))
        if self.m and GL.shape != (S, nrhs, self.m):
            raise ValueError("GL has shape %r, expected %r" % (GL.shape, (S, nrhs, self.m)))
        nd = self.n_dpar
        OUT, DBOUND, AL = np.empty((S, nrhs, max(nd, 1))), np.empty((S, nrhs, max(self.m, 1))), np.empty((S, nrhs, max(self.m, 1)))
        AX, infos = np.empty((S, nrhs, self.n)), (_lib.KktInfo * (S * nrhs))()
        self._check(self._lib.asm_batch_solution_adjoint(self._b, S, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), nrhs, _lib.dptr(GX), _lib.dptr(GL), par,
                                                         _lib.dptr(OUT), _lib.dptr(DBOUND), _lib.dptr(AX), _lib.dptr(AL), infos))
        return OUT[:, :, :nd], DBOUND[:, :, :self.m], AX, AL[:, :, :self.m], [[infos[s * nrhs + c] for c in range(nrhs)] for s in range(S)]

    def var_bound_sensitivity(self, x, lam, row_state, bound_state, vars, delta=None, max_iter=None, rtol=None):
        """asm_batch_var_bound_sensitivity: per scenario HipSubOptimizer.var_bound_sensitivity_multi for the variables `vars` (0-based, the
        same for every scenario; delta None: unit moves) - column c answers a move of the bound variable vars[c] sits at, the zero column
        where the variable is free in the scenario; the outputs of kkt_solve_multi."""
        from . import _lib
        S, x, lam, rs, bs, par = self._kkt_args(x, lam, row_state, bound_state, max_iter, rtol)
        vars = np.ascontiguousarray(np.atleast_1d(vars), np.int32)
        if vars.ndim != 1 or len(vars) < 1:
            raise ValueError("vars has shape %r, expected (nrhs,) with at least one variable" % (vars.shape,))
        nrhs = len(vars)
        if delta is not None:
            delta = np.ascontiguousarray(np.atleast_1d(delta), np.float64)
            if delta.shape != (nrhs,):
                raise ValueError("delta has shape %r, expected %r" % (delta.shape, (nrhs,)))
        DX, DLAM, DZ, infos = self._kkt_outputs(S, nrhs)
        self._check(self._lib.asm_batch_var_bound_sensitivity(self._b, S, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), nrhs, _lib.i32ptr(vars),
                                                              None if delta is None else _lib.dptr(delta), par, _lib.dptr(DX), _lib.dptr(DLAM), _lib.dptr(DZ), infos))
        return self._kkt_result(S, nrhs, self.m, DX, DLAM, DZ, infos)

    def solution_adjoint_z(self, x, lam, row_state, bound_state, GX, GL, GZ=None, max_iter=None, rtol=None):
        """(OUT, DBOUND [n_scen x nrhs x m], DXBOUND [n_scen x nrhs x n], AX, AL, infos[s][c]) of asm_batch_solution_adjoint_z: per scenario
        HipSubOptimizer.solution_adjoint_z_multi, bit for bit - solution_adjoint with weights GZ [n_scen x nrhs x n] on the bound
        multipliers (None: 0) and the gradients with respect to the variable bounds."""
        from . import _lib
        S, x, lam, rs, bs, par = self._kkt_args(x, lam, row_state, bound_state, max_iter, rtol)
        GX = np.ascontiguousarray(GX, np.float64)
        if GX.ndim != 3 or GX.shape[0] != S or GX.shape[1] < 1 or GX.shape[2] != self.n:
            raise ValueError("GX has shape %r, expected (%d, nrhs, %d) with at least one function" % (GX.shape, S, self.n))
        nrhs = GX.shape[1]
        GL = np.ascontiguousarray(GL, np.float64) if self.m else np.zeros((S, nrhs, 1))
        if self.m and GL.shape != (S, nrhs, self.m):
            raise ValueError("GL has shape %r, expected %r" % (GL.shape, (S, nrhs, self.m)))
        if GZ is not None:
            GZ = np.ascontiguousarray(GZ, np.float64)
            if GZ.shape != GX.shape:
                raise ValueError("GZ has shape %r, expected %r" % (GZ.shape, GX.shape))
        nd = self.n_dpar
        OUT, DBOUND, AL = np.empty((S, nrhs, max(nd, 1))), np.empty((S, nrhs, max(self.m, 1))), np.empty((S, nrhs, max(self.m, 1)))
        AX, DXBOUND, infos = np.empty((S, nrhs, self.n)), np.empty((S, nrhs, self.n)), (_lib.KktInfo * (S * nrhs))()
        self._check(self._lib.asm_batch_solution_adjoint_z(self._b, S, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), nrhs, _lib.dptr(GX), _lib.dptr(GL),
                                                           None if GZ is None else _lib.dptr(GZ), par, _lib.dptr(OUT), _lib.dptr(DBOUND), _lib.dptr(DXBOUND),
                                                           _lib.dptr(AX), _lib.dptr(AL), infos))
        return (OUT[:, :, :nd], DBOUND[:, :, :self.m], DXBOUND, AX, AL[:, :, :self.m],
                [[infos[s * nrhs + c] for c in range(nrhs)] for s in range(S)])

    def sensitivity_range(self, g_L, g_U, x_L, x_U, x, lam, mult_x_U, mult_x_L, row_state, bound_state, DX, DLAM, DZ):
        """asm_batch_sensitivity_range: per scenario HipSubOptimizer.sensitivity_range, bit for bit what a fresh handle with the scenario's
        bounds (rows of g_L, g_U [n_scen x m], x_L, x_U [n_scen x n], as slp_run takes them) and data gives, for the columns DX, DZ
        [n_scen x nrhs x n] and DLAM [n_scen x nrhs x m].  Returns a structured array [n_scen x nrhs] with the fields of asm_range_info."""
        from . import _lib
        S, x, lam, rs, bs, _ = self._kkt_args(x, lam, row_state, bound_state, None, None)
        f64 = lambda a_: np.ascontiguousarray(a_, np.float64)
        g_L, g_U, x_L, x_U, mU, mL = map(f64, (g_L, g_U, x_L, x_U, mult_x_U, mult_x_L))
        if self.m and (g_L.shape != (S, self.m) or g_U.shape != (S, self.m)):
            raise ValueError("g_L / g_U have shapes %r / %r, expected %r" % (g_L.shape, g_U.shape, (S, self.m)))
        for name, a in (("x_L", x_L), ("x_U", x_U), ("mult_x_U", mU), ("mult_x_L", mL)):
            if a.shape != (S, self.n):
                raise ValueError("%s has shape %r, expected %r" % (name, a.shape, (S, self.n)))
        if not self.m:
            g_L = g_U = np.zeros((S, 1))
        z = mU + mL
        DX = f64(DX)
        if DX.ndim != 3 or DX.shape[0] != S or DX.shape[1] < 1 or DX.shape[2] != self.n:
            raise ValueError("DX has shape %r, expected (%d, nrhs, %d) with at least one column" % (DX.shape, S, self.n))
        nrhs = DX.shape[1]
        DZ = f64(DZ)
        DLAM = f64(DLAM) if self.m else np.zeros((S, nrhs, 1))
        if DZ.shape != DX.shape or (self.m and DLAM.shape != (S, nrhs, self.m)):
            raise ValueError("DZ / DLAM have shapes %r / %r, expected %r / %r" % (DZ.shape, DLAM.shape, DX.shape, (S, nrhs, self.m)))
        out = np.zeros((S, nrhs), dtype=_lib.RangeInfo)
        self._check(self._lib.asm_batch_sensitivity_range(self._b, S, _lib.dptr(g_L), _lib.dptr(g_U), _lib.dptr(x_L), _lib.dptr(x_U), _lib.dptr(x), _lib.dptr(lam),
                                                          _lib.dptr(z), _lib.i32ptr(rs), _lib.i32ptr(bs), nrhs, _lib.dptr(DX), _lib.dptr(DLAM), _lib.dptr(DZ),
                                                          out.ctypes.data_as(self._C.POINTER(_lib.RangeInfo))))
        return out

    def sublp_solve(self, dE, df, f, E, x_k, delta, feasibility, bounds=None):
        """asm_sublp_solve for `count` = len(f) <= n_slots scenarios in lockstep; `bounds` = (g_L, g_U, x_L, x_U) per scenario or None.
        Returns (p, lambda, mult_x_U, mult_x_L, p_slack, status) with a leading scenario dimension."""
        from . import _lib
        f64 = lambda a_: np.ascontiguousarray(a_, np.float64)
        dE, df, f, E, x_k, delta = map(f64, (dE, df, f, E, x_k, delta))
        cnt = len(f)
        fe = np.ascontiguousarray(feasibility, np.int32)
        p = np.empty((cnt, self.n)); lam = np.empty((cnt, max(self.m, 1))); mU = np.empty((cnt, self.n)); mL = np.empty((cnt, self.n))
        ps = np.empty((cnt, 2 * max(self.m, 1))); st = np.zeros(cnt, np.int32)
        if bounds is not None:
            bl = [f64(b_) for b_ in bounds]
            bp = [_lib.dptr(b_) for b_ in bl]
        else:
            bp = [None] * 4
        self._check(self._lib.asm_batch_sublp_solve(self._b, cnt, bp[0], bp[1], bp[2], bp[3], _lib.dptr(dE), _lib.dptr(df), _lib.dptr(f), _lib.dptr(E),
                                                    _lib.dptr(x_k), _lib.dptr(delta), _lib.i32ptr(fe), _lib.dptr(p), _lib.dptr(lam), _lib.dptr(mU), _lib.dptr(mL),
                                                    _lib.dptr(ps), _lib.i32ptr(st)))
        return p, lam[:, :self.m], mU, mL, ps[:, :2 * self.m], st

    def slot_stats(self, slot):
        from . import _lib
        s = _lib.SolveStats()
        h = self._lib.asm_batch_handle(self._b, int(slot))
        rc = self._lib.asm_sublp_last_stats(h, self._C.byref(s))
        if rc != 0:
            raise self._err("asm_sublp_last_stats(slot %d): %d" % (slot, rc))
        return {k: getattr(s, k) for k, _ in s._fields_}


def lagrangian_hessians(hb, runs, sparse=False):
    """The Hessians of the SLP drivers' Lagrangian f - lam' g of the scenarios of a HipBatch at the runs' (x, lam) - e.g. what hb.slp_run
    returned, each scenario with its data: the MOI Hessian at obj_factor 1 and -lam, one symmetric n x n matrix per run (dense, or
    scipy.sparse CSR with sparse=True).  The batch counterpart of moi_evaluator.lagrangian_hessian."""
    from .moi_evaluator import hessian_matrix
    x = np.stack([np.asarray(r.x, float) for r in runs])
    lam = -np.stack([np.asarray(r.lam, float) for r in runs]) if hb.m else np.zeros((len(runs), 0))
    rows, cols = hb.hessian_structure()
    values = hb.eval_hessian_lagrangian(x, 1.0, lam)
    return [hessian_matrix(rows, cols, values[s], hb.n, sparse) for s in range(len(runs))]


def working_sets(problems, runs, tol=1e-6):
    """(row_state [S x m], bound_state [S x n], int32) of the scenarios `problems` at their `runs` (what HipBatch.slp_run or
    solve_batch_lockstep returned): sensitivity.working_set per scenario, stacked."""
    from .sensitivity import working_set
    if len(problems) != len(runs) or not len(runs):
        raise ValueError("%d problems for %d runs (at least one of each)" % (len(problems), len(runs)))
    sets = [working_set(p, r.x, r.lam, r.mult_x_U, r.mult_x_L, tol) for p, r in zip(problems, runs)]
    return np.stack([s[0] for s in sets]).astype(np.int32), np.stack([s[1] for s in sets]).astype(np.int32)


def _run_points(hb, runs):
    x = np.stack([np.asarray(r.x, float) for r in runs])
    lam = np.stack([np.asarray(r.lam, float) for r in runs]) if hb.m else np.zeros((len(runs), 0))
    return x, lam


def _jacobian_stacks(DX, DLAM, infos):
    status = np.array([[i.status for i in row] for row in infos], np.int32)
    return np.transpose(DX, (0, 2, 1)).copy(), np.transpose(DLAM, (0, 2, 1)).copy(), status


def solution_jacobians(hb, problems, runs, indices=None, tol=1e-6):
    """(dx*/dc [S x n x k], dlam*/dc [S x m x k], status [S x k]) of the scenarios of the HipBatch `hb` at their runs, for the constants
    `indices` of the NLP block's data (all of them when None): column q is the solution sensitivity along the unit direction of constant
    indices[q] on the scenario's working set (working_sets with `tol`), every scenario with its data - one
    asm_batch_solution_sensitivity call.  The batch counterpart of sensitivity.solution_jacobian; a column that is not solved is
    reported in `status` (asm_kkt_info.status), not raised."""
    nd = hb.n_dpar
    idx = np.arange(nd) if indices is None else np.atleast_1d(np.asarray(indices, np.int64))
    if idx.ndim != 1 or not len(idx) or np.any(idx < 0) or np.any(idx >= nd):
        raise ValueError("indices must be a non-empty list of constants in [0, %d)" % nd)
    rs, bs = working_sets(problems, runs, tol)
    x, lam = _run_points(hb, runs)
    DC = np.zeros((len(idx), nd))
    DC[np.arange(len(idx)), idx] = 1.0
    DX, DLAM, _, infos = hb.solution_sensitivity_multi(x, lam, rs, bs, DC)
    return _jacobian_stacks(DX, DLAM, infos)


def solution_adjoints(hb, problems, runs, GX, GL, tol=1e-6):
    """(d phi / d dpar [S x k x n_dpar], d phi / d(bound) [S x k x m], status [S x k]) of the scenarios of the HipBatch `hb` at their runs
    for k functions per scenario with gradients GX [S x k x n] and GL [S x k x m] (or [k x n] and [k x m], the same functions for every
    scenario), on each scenario's working set (working_sets with `tol`) and with its data - one asm_batch_solution_adjoint call, one
    KKT solve per function whatever n_dpar.  The reverse-mode counterpart of solution_jacobians; a function whose solve did not
    end with status 0 is reported in `status`, not raised."""
    S = len(runs)
    GX, GL = np.asarray(GX, float), np.asarray(GL, float)
    if GX.ndim == 2:
        GX = np.broadcast_to(GX, (S,) + GX.shape)
    if GL.ndim == 2:
        GL = np.broadcast_to(GL, (S,) + GL.shape)
    rs, bs = working_sets(problems, runs, tol)
    x, lam = _run_points(hb, runs)
    OUT, DBOUND, _, _, infos = hb.solution_adjoint(x, lam, rs, bs, GX, GL)
    return OUT, DBOUND, np.array([[i.status for i in row] for row in infos], np.int32)


def bound_jacobians(hb, problems, runs, rows, tol=1e-6):
    """(dx*/d(bound) [S x n x k], dlam*/d(bound) [S x m x k], status [S x k]) of the scenarios of `hb` at their runs: column q answers a
    unit move of the active bound of row rows[q] (0-based, the same rows for every scenario) - the zero column in a scenario whose
    working set does not hold the row - from one asm_batch_bound_sensitivity call.  The batch counterpart of sensitivity.bound_jacobian;
    it reports the column statuses and does not raise on one that is not 0."""
    rows = np.atleast_1d(np.asarray(rows, np.int64))
    if rows.ndim != 1 or not len(rows) or np.any(rows < 0) or np.any(rows >= hb.m):
        raise ValueError("rows must be a non-empty list of rows in [0, %d)" % hb.m)
    rs, bs = working_sets(problems, runs, tol)
    x, lam = _run_points(hb, runs)
    DX, DLAM, _, infos = hb.bound_sensitivity(x, lam, rs, bs, rows)
    return _jacobian_stacks(DX, DLAM, infos)


def var_bound_jacobians(hb, problems, runs, vars, tol=1e-6):
    """(dx*/d(xbound) [S x n x k], dlam*/d(xbound) [S x m x k], dz*/d(xbound) [S x n x k], status [S x k]) of the scenarios of `hb` at their
    runs: column q answers a unit move of the bound that variable vars[q] sits at (0-based, the same variables for every scenario) - the
    zero column in a scenario where the variable is free - from one asm_batch_var_bound_sensitivity call.  The batch counterpart of
    sensitivity.var_bound_jacobian; it reports the column statuses and does not raise on one that is not 0."""
    vars = np.atleast_1d(np.asarray(vars, np.int64))
    if vars.ndim != 1 or not len(vars) or np.any(vars < 0) or np.any(vars >= hb.n):
        raise ValueError("vars must be a non-empty list of variables in [0, %d)" % hb.n)
    rs, bs = working_sets(problems, runs, tol)
    x, lam = _run_points(hb, runs)
    DX, DLAM, DZ, infos = hb.var_bound_sensitivity(x, lam, rs, bs, vars)
    dx, dlam, status = _jacobian_stacks(DX, DLAM, infos)
    return dx, dlam, np.transpose(DZ, (0, 2, 1)).copy(), status


def validity_ranges(hb, problems, runs, DX, DLAM, DZ, tol=1e-6):
    """The validity ranges (structured array [S x k], the fields of asm_range_info) of the sensitivity columns DX [S x k x n],
    DLAM [S x k x m], DZ [S x k x n] of the scenarios of `hb` at their runs - each on its working set (working_sets with `tol`), with its
    bounds and its data: one asm_batch_sensitivity_range call.  The batch counterpart of sensitivity.validity_range; a scenario whose
    columns all have t_lo <= -1 and t_hi >= 1 for a unit data change keeps the base case's working set to first order."""
    rs, bs = working_sets(problems, runs, tol)
    x, lam = _run_points(hb, runs)
    stack = lambda name: np.stack([np.asarray(getattr(p, name), float) for p in problems]) if name[0] == "x" or hb.m else np.zeros((len(problems), 0))
    mU, mL = np.stack([np.asarray(r.mult_x_U, float) for r in runs]), np.stack([np.asarray(r.mult_x_L, float) for r in runs])
    return hb.sensitivity_range(stack("g_L"), stack("g_U"), stack("x_L"), stack("x_U"), x, lam, mU, mL, rs, bs, DX, DLAM, DZ)


def solve_batch_lockstep(problems, parameters, n_slots, device=0, rank=0, world=1, reduce_device=None, batch=None):
    """The scenarios of this rank (`problems`: list of Problems with one pattern, built from FunctionModels) through a HipBatch of `n_slots`
    slots; returns (runs, reduced statistics, batch statistics) like `solve_batch`.  `batch`: an existing HipBatch to re-use."""
    check_batch_kkt_form(parameters)
    own = batch is None
    if own:
        batch = HipBatch(problems[0], min(int(n_slots), len(problems)), device)
    data = batch.scenario_data(problems)          # NLP blocks with other data (line parameters, ...): per scenario through the table
    t0 = time.perf_counter()
    runs = batch.slp_run(np.stack([p.g_L for p in problems]), np.stack([p.g_U for p in problems]), np.stack([p.x_L for p in problems]),
                         np.stack([p.x_U for p in problems]), np.stack([p.x0 for p in problems]), parameters, data=data)
    st = local_stats(runs, time.perf_counter() - t0)
    bst = batch.stats()
    if own:
        batch.close()
    return runs, reduce_stats(st, reduce_device), bst


# ------------------------------------------------------------------------------------------------------------------------------
# Dynamic assignment across ranks ("consider dynamic work assignment via a host-side counter"): instead of the
# static block partition every rank claims chunks of scenario indices from one counter in the process group's key-value store.  It pays
# when a rank has more scenarios than batch slots AND the iteration counts differ between ranks; with as many slots as scenarios per
# GPU (the default shape: 64 / 64) every scenario of a rank runs concurrently and a rank's time is its slowest scenario - nothing to steal.
# ------------------------------------------------------------------------------------------------------------------------------
def claim_chunks(total, chunk, store=None, key="asm_batch_next"):
    """Yield (lo, hi) ranges of [0, total) claimed from a counter shared by the ranks: `store.add(key, chunk)` is atomic across processes
    (torch.distributed TCPStore / the default group's store).  Without a store: one local counter (single process)."""
    total, chunk = int(total), max(1, int(chunk))
    if store is None:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            from torch.distributed import distributed_c10d
            store = distributed_c10d._get_default_store()
    local = [0]
    while True:
        if store is not None:
            hi = int(store.add(key, chunk))
        else:
            local[0] += chunk
            hi = local[0]
        lo = hi - chunk
        if lo >= total:
            return
        yield lo, min(hi, total)


def solve_batch_dynamic(problem_of, total, parameters, n_slots, batch, chunk=None, store=None, reduce_device=None):
    """Lockstep batch with dynamic assignment: this rank claims chunks of `chunk` scenarios (default: n_slots) until the counter runs out;
    `problem_of(s)` returns the Problem of scenario s.  Returns ({scenario: NativeRun}, reduced statistics)."""
    check_batch_kkt_form(parameters)
    chunk = int(chunk or n_slots)
    t0 = time.perf_counter()
    mine = {}
    for lo, hi in claim_chunks(total, chunk, store):
        prs = [problem_of(s) for s in range(lo, hi)]
        runs = batch.slp_run(np.stack([p.g_L for p in prs]), np.stack([p.g_U for p in prs]), np.stack([p.x_L for p in prs]),
                             np.stack([p.x_U for p in prs]), np.stack([p.x0 for p in prs]), parameters, data=batch.scenario_data(prs))
        mine.update({lo + k: r for k, r in enumerate(runs)})
    st = local_stats(list(mine.values()), time.perf_counter() - t0)
    return mine, reduce_stats(st, reduce_device)
