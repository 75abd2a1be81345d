"""Host-side mirror of the reference's sub-problem interface (src/algorithms/subproblem.jl) on top of
the C ABI of libasmhip (include/asm_hip.h).

    QpData            subproblem.jl:3-14  (same field names; Q is always None on the SLP path, slp.jl:12)
    HipSubOptimizer   the `AbstractSubOptimizer` (subproblem.jl:1) that replaces `QpModel`; it is created
                      once per SLP run (slp.jl:25-36) and called once per outer iteration with
                      `sub_optimize(x_k, Delta, feasibility)` -> the reference's 6-tuple (subproblem.jl:541)

The Jacobian travels as the COO value vector `dE` in `j_str` order (what `eval_jac_g` fills,
slp.jl:186-191); `compute_jacobian_matrix` (common.jl:12-20) runs on the GPU inside the call.
"""
import ctypes as C
from collections.abc import Mapping
import numpy as np
from . import _lib
from .moi_evaluator import nlp_kind


class AsmHipError(RuntimeError):
    pass


class PSlack(Mapping):
    """`p_slack::Dict{Int,Vector{Float64}}` of subproblem.jl:495-505 over the flat array the C ABI returned (`raw`: two entries per
    row, NaN where a row has one slack).  The per-row lists are made when a row is first asked for: the SLP drivers hand `raw`
    straight back to the device-side merit function, and a Python loop over 18 637 rows per LP costs milliseconds."""

    def __init__(self, raw, one_slack):
        self.raw, self._one, self._rows = raw, one_slack, None

    def _dict(self):
        if self._rows is None:
            pl, one = self.raw.tolist(), self._one.tolist()
            self._rows = {i: ([pl[2 * i]] if one[i] else [pl[2 * i], pl[2 * i + 1]]) for i in range(len(one))}
        return self._rows

    def __getitem__(self, i):
        if self._rows is None:
            if not 0 <= i < len(self._one):
                raise KeyError(i)
            return [float(self.raw[2 * i])] if self._one[i] else [float(self.raw[2 * i]), float(self.raw[2 * i + 1])]
        return self._rows[i]

    def __iter__(self):
        return iter(range(len(self._one)))

    def __len__(self):
        return len(self._one)

    def __eq__(self, other):
        return self._dict() == (other._dict() if isinstance(other, PSlack) else other)

    def __repr__(self):
        return "PSlack(%r)" % (self._dict(),)


class QpData:
    """LpData(slp) of slp.jl:8-21: c = df, c0 = f, A = Jacobian (as COO values dE), b = E."""

    def __init__(self, c, c0, dE, b, c_lb, c_ub, v_lb, v_ub, sense="MIN_SENSE", Q=None):
        self.sense, self.Q = sense, Q
        self.c, self.c0, self.dE, self.b = c, c0, dE, b
        self.c_lb, self.c_ub, self.v_lb, self.v_ub = c_lb, c_ub, v_lb, v_ub


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class HipSubOptimizer:
    """One handle <-> one HIP stream <-> one LP skeleton (create_model!, subproblem.jl:51-215)."""

    def __init__(self, data, j_row, j_col, device=0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        rc = self._lib.asm_create(int(device), C.byref(self._h))
        if rc != 0:
            raise AsmHipError("asm_create(device=%d) failed with code %d (no usable HIP device?)" % (device, rc))
        self.data = data
        self.j_row = np.ascontiguousarray(j_row, dtype=np.int64)
        self.j_col = np.ascontiguousarray(j_col, dtype=np.int64)
        self.n = len(data.v_lb)
        self.m = len(data.c_lb)
        assert self.n > 0 and self.m >= 0                       # subproblem.jl:65-72
        assert len(data.c_ub) == self.m and len(data.v_ub) == self.n
        c_lb, c_ub, v_lb, v_ub = map(_f64, (data.c_lb, data.c_ub, data.v_lb, data.v_ub))
        self._check(self._lib.asm_sublp_setup(self._h, self.n, self.m, len(self.j_row), _lib.i64ptr(self.j_row),
                                              _lib.i64ptr(self.j_col), _lib.dptr(c_lb), _lib.dptr(c_ub),
                                              _lib.dptr(v_lb), _lib.dptr(v_ub)))
        self.nslack = np.where((c_lb > -np.inf) & (c_ub < np.inf), 2, 1)

    def set_bounds(self, data):
        """Re-use the handle (all its HBM buffers, the assembly plan, the device evaluator) for another instance with the same
        pattern and new bounds - the next scenario of a batch."""
        c_lb, c_ub, v_lb, v_ub = map(_f64, (data.c_lb, data.c_ub, data.v_lb, data.v_ub))
        assert len(c_lb) == self.m and len(v_lb) == self.n
        self._check(self._lib.asm_sublp_set_bounds(self._h, _lib.dptr(c_lb), _lib.dptr(c_ub), _lib.dptr(v_lb), _lib.dptr(v_ub)))
        self.data = data
        self.nslack = np.where((c_lb > -np.inf) & (c_ub < np.inf), 2, 1)

    def _check(self, rc):
        if rc != 0:
            raise AsmHipError("libasmhip error %d: %s" % (rc, self._lib.asm_last_error(self._h).decode()))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.asm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ the hot call
    def sub_optimize(self, x_k, Delta, feasibility=False):
        """sub_optimize!(qp, x_k, Δ, feasibility) - subproblem.jl:229-542.
        Returns (Xsol, lambda, mult_x_U, mult_x_L, p_slack, status)."""
        d, n, m = self.data, self.n, self.m
        assert len(d.c) == n and len(d.b) == m and len(x_k) == n   # subproblem.jl:239-246
        self.upload(d.dE, d.c, d.c0, d.b, x_k)
        return self.solve_resident(Delta, feasibility)

    def upload(self, dE, df, f, E, x_k):
        dE, df, E, x_k = map(_f64, (dE, df, E, x_k))
        assert len(dE) == len(self.j_row)
        self._check(self._lib.asm_sublp_upload(self._h, _lib.dptr(dE), _lib.dptr(df), float(f), _lib.dptr(E), _lib.dptr(x_k)))

    def solve_resident(self, Delta, feasibility=False):
        n, m = self.n, self.m
        Xsol = np.empty(n); lam = np.empty(m); mU = np.empty(n); mL = np.empty(n)
        ps = np.empty(2 * max(m, 1)); status = C.c_int32(0)
        self._check(self._lib.asm_sublp_solve_resident(self._h, float(Delta), int(bool(feasibility)), _lib.dptr(Xsol),
                                                       _lib.dptr(lam), _lib.dptr(mU), _lib.dptr(mL), _lib.dptr(ps),
                                                       C.byref(status)))
        p_slack = PSlack(ps, self.nslack == 1)            # subproblem.jl:495-505
        return Xsol, lam, mU, mL, p_slack, int(status.value)

    def lp_solve(self, dE, q, r, lb, ub, w=None, slo=None):
        """The LP as an MOI optimizer receives it (include/asm_hip.h: asm_lp_solve): returns (p, s, y, z, bound_state, status)."""
        dE, q, r, lb, ub = map(_f64, (dE, q, r, lb, ub))
        use = w is not None
        ns = int(self.nslack.sum())
        w_, slo_ = (_f64(w), _f64(slo)) if use else (np.zeros(1), np.zeros(1))
        p = np.empty(self.n); s = np.empty(max(ns, 1)); y = np.empty(max(len(r), 1)); z = np.empty(self.n)
        bs = np.empty(self.n, np.int32); status = C.c_int32(0)
        self._check(self._lib.asm_lp_solve(self._h, _lib.dptr(dE), _lib.dptr(q), _lib.dptr(r), _lib.dptr(lb), _lib.dptr(ub), int(use),
                                           _lib.dptr(w_), _lib.dptr(slo_), _lib.dptr(p), _lib.dptr(s), _lib.dptr(y), _lib.dptr(z),
                                           _lib.i32ptr(bs), C.byref(status)))
        return p, s[:ns], y[:len(r)], z, bs, int(status.value)

    # ------------------------------------------------------------------ observability
    def active_set(self):
        nr, nsl = C.c_int64(0), C.c_int64(0)
        rc = self._lib.asm_sublp_active_set(self._h, None, None, None, C.byref(nr), C.byref(nsl))
        if rc != 0:
            return None
        rows = np.empty(nr.value, np.int32); bnd = np.empty(self.n, np.int32); sl = np.empty(max(nsl.value, 1), np.int32)
        self._check(self._lib.asm_sublp_active_set(self._h, _lib.i32ptr(rows), _lib.i32ptr(bnd), _lib.i32ptr(sl), None, None))
        return rows, bnd, sl[:nsl.value]

    def reset_warm(self):
        self._check(self._lib.asm_sublp_reset_warm(self._h))

    def ns_basis(self):
        """Columns (0-based) retained by the null-space form of the normal phase (asm_sublp_ns_basis); empty when the form is not in use."""
        k = C.c_int64(0)
        self._check(self._lib.asm_sublp_ns_basis(self._h, None, C.byref(k)))
        J = np.zeros(max(int(k.value), 1), np.int32)
        self._check(self._lib.asm_sublp_ns_basis(self._h, J.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(k)))
        return J[:int(k.value)].astype(np.int64)

    def row_order(self):
        """(perm, band, e_rows, e_band): the rows by position in the order of the factorisations (None when the natural order is in use), the
        half-bandwidth, the equality rows of the null-space form in their own order and its band (asm_sublp_row_order)."""
        band, n_e, e_band = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(self._lib.asm_sublp_row_order(self._h, None, C.byref(band), None, C.byref(n_e), C.byref(e_band)))
        d = self.data
        M = self.m + int(((d.c_lb > -np.inf) & (d.c_ub < np.inf) & (d.c_lb < d.c_ub)).sum())      # one extra <= row per range constraint
        perm = np.zeros(max(M, 1), np.int32); e = np.zeros(max(int(n_e.value), 1), np.int32)
        self._check(self._lib.asm_sublp_row_order(self._h, perm.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(band),
                                                  e.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n_e), C.byref(e_band)))
        return (perm[:M].astype(np.int64) if band.value > 0 else None), int(band.value), e[:int(n_e.value)].astype(np.int64), int(e_band.value)

    def last_stats(self):
        s = _lib.SolveStats()
        self._check(self._lib.asm_sublp_last_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}

    def kernel_stats(self, reset=False):
        s = _lib.KernelStats()
        self._check(self._lib.asm_kernel_stats_get(self._h, C.byref(s)))
        out = {name: dict(ms=s.ms[i], calls=s.calls[i], flops=s.flops[i], bytes=s.bytes[i]) for i, name in enumerate(_lib.K_NAMES)}
        if reset:
            self._check(self._lib.asm_kernel_stats_reset(self._h))
        return out

    def kernel_timing(self, level):
        """0 off, 1 every launch of the rank-K and panel kernels, 2 every kernel family (asm_kernel_timing)."""
        self._check(self._lib.asm_kernel_timing(self._h, int(level)))

    # ------------------------------------------------------------------ device-side evaluators (include/asm_hip.h: asm_eval_*)
    def eval_setup(self, fm):
        """Hand the flattened function store of a FunctionModel (moi_evaluator.py) and its NLP block kernel to the handle."""
        fl = fm.flatten()
        kind, rows, nnz = 0, 0, 0
        ipar, dpar = np.zeros(1, np.int64), np.zeros(1)
        if fm.nlp is not None:
            if fm.nlp.device is None:
                raise AsmHipError("the model's NLP block has no device kernel")
            kind = nlp_kind(fm.nlp.device)
            _, ipar, dpar = fm.nlp.device
            rows, nnz = fm.nlp.m, len(fm.nlp.rows)
            ipar, dpar = np.ascontiguousarray(ipar, np.int64), np.ascontiguousarray(dpar, np.float64)
        self._ev_keep = (fl, ipar, dpar)
        self._ev_nd = len(dpar) if kind else 0             # n_dpar as the library counts it: none without an NLP block
        a = lambda k: fl[k]
        self._check(self._lib.asm_eval_setup(self._h, fl["n_rows"], _lib.i64ptr(a("aff_ptr")), _lib.i64ptr(a("aff_var")), _lib.dptr(a("aff_coef")),
                                             _lib.i64ptr(a("quad_ptr")), _lib.i64ptr(a("q_v1")), _lib.i64ptr(a("q_v2")), _lib.dptr(a("q_coef")),
                                             _lib.dptr(a("constant")), _lib.i64ptr(a("jac_off")), _lib.i64ptr(a("g_ptr")), _lib.i64ptr(a("g_kind")),
                                             _lib.dptr(a("g_coef")), _lib.i64ptr(a("g_other")), float(fl["objective_scale"]), kind, rows, nnz,
                                             _lib.i64ptr(ipar), len(ipar) if kind else 0, _lib.dptr(dpar), len(dpar) if kind else 0))

    def eval_functions(self, x):
        """eval_functions! (slp.jl:186-191) on the GPU: returns (f, df, E); dE stays in HBM as the next LP's input."""
        x = _f64(x)
        f = C.c_double(0.0); df = np.empty(self.n); E = np.empty(max(self.m, 1))
        self._check(self._lib.asm_eval_functions(self._h, _lib.dptr(x), C.byref(f), _lib.dptr(df), _lib.dptr(E)))
        return f.value, df, E[:self.m]

    def eval_constraints(self, x):
        x = _f64(x)
        f = C.c_double(0.0); E = np.empty(max(self.m, 1))
        self._check(self._lib.asm_eval_constraints(self._h, _lib.dptr(x), C.byref(f), _lib.dptr(E)))
        return f.value, E[:self.m]

    def jacobian_values(self):
        dE = np.empty(max(len(self.j_row), 1))
        self._check(self._lib.asm_eval_jacobian_values(self._h, _lib.dptr(dE)))
        return dE[:len(self.j_row)]

    def set_eval_data(self, values, offset=0):
        """Overwrite dpar[offset, offset + len(values)) of the NLP block on the device (asm_eval_set_data): the next evaluations
        use the new data; pattern, bounds and the retained LP state stay."""
        v = _f64(np.atleast_1d(values))
        self._check(self._lib.asm_eval_set_data(self._h, int(offset), len(v), _lib.dptr(v)))

    def eval_data_gradient(self, x, lam):
        """d(f - lam' g) / d dpar at x (asm_eval_data_gradient; expression blocks and the block kernels with derivatives, device kinds 3, 4 and 5), lam [m] in the sign convention of
        slp_run's multipliers: at an SLP solution, the derivative of the optimal value with respect to each dpar entry."""
        x, lam = _f64(x), _f64(np.atleast_1d(lam) if self.m else np.zeros(1))
        nd = len(self._ev_keep[2]) if getattr(self, "_ev_keep", None) is not None else 0
        out = np.empty(max(nd, 1))
        self._check(self._lib.asm_eval_data_gradient(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.dptr(out)))
        return out[:nd]

    def hessian_structure(self):
        """(rows, cols), 1-based, of the Hessian of the Lagrangian (asm_eval_hessian_structure): the function store's quadratic terms
        as given, then the expression block's sorted lower-triangle pairs; an off-diagonal entry stands for both positions."""
        nnz = C.c_int64(0)
        self._check(self._lib.asm_eval_hessian_structure(self._h, C.byref(nnz), None, None))
        rows, cols = np.zeros(max(nnz.value, 1), np.int64), np.zeros(max(nnz.value, 1), np.int64)
        self._check(self._lib.asm_eval_hessian_structure(self._h, C.byref(nnz), _lib.i64ptr(rows), _lib.i64ptr(cols)))
        return rows[:nnz.value], cols[:nnz.value]

    def eval_hessian_lagrangian(self, x, obj_factor, lam):
        """Values of obj_factor * objective_scale * hess f + sum_i lam[i] hess g_i at x in the pattern's order
        (asm_eval_hessian_lagrangian; MOI sign: pass -lam for slp_run's multipliers)."""
        x, lam = _f64(x), _f64(np.atleast_1d(lam) if self.m else np.zeros(1))
        assert len(x) == self.n and len(lam) >= self.m
        nnz = C.c_int64(0)
        self._check(self._lib.asm_eval_hessian_structure(self._h, C.byref(nnz), None, None))
        values = np.empty(max(nnz.value, 1))
        self._check(self._lib.asm_eval_hessian_lagrangian(self._h, _lib.dptr(x), float(obj_factor), _lib.dptr(lam), _lib.dptr(values)))
        return values[:nnz.value]

    def hessian_product(self, x, obj_factor, lam, v):
        """H v with H the symmetric matrix of eval_hessian_lagrangian(x, obj_factor, lam) (asm_eval_hessian_product)."""
        x, v, lam = _f64(x), _f64(v), _f64(np.atleast_1d(lam) if self.m else np.zeros(1))
        assert len(x) == self.n and len(v) == self.n and len(lam) >= self.m
        out = np.empty(self.n)
        self._check(self._lib.asm_eval_hessian_product(self._h, _lib.dptr(x), float(obj_factor), _lib.dptr(lam), _lib.dptr(v), _lib.dptr(out)))
        return out

    # ------------------------------------------------------------------ solution sensitivities (include/asm_hip.h: asm_eval_data_cross, asm_kkt_solve)
    def _vec(self, a, length, name):
        a = _f64(np.atleast_1d(a))
        if a.shape != (length,):
            raise ValueError("%s has shape %r, expected (%d,)" % (name, a.shape, length))
        return a if length else np.zeros(1)

    def _states(self, row_state, bound_state):
        rs = np.ascontiguousarray(np.atleast_1d(row_state), dtype=np.int32) if self.m else np.zeros(0, np.int32)
        bs = np.ascontiguousarray(np.atleast_1d(bound_state), dtype=np.int32)
        if rs.shape != (self.m,) or bs.shape != (self.n,):
            raise ValueError("row_state / bound_state have shapes %r / %r, expected (%d,) / (%d,)" % (rs.shape, bs.shape, self.m, self.n))
        return (rs if self.m else np.zeros(1, np.int32)), bs

    def data_cross(self, x, lam, dc):
        """(u, w) of asm_eval_data_cross: u [n] = d/d dpar (grad_x (f - lam' g)) . dc and w [m] = (d g / d dpar) . dc for a direction dc in the
        block's data (expression blocks and the block kernels with derivatives), lam [m] in the sign convention of slp_run's multipliers."""
        nd = len(self._ev_keep[2]) if getattr(self, "_ev_keep", None) is not None else 0
        x, lam, dc = self._vec(x, self.n, "x"), self._vec(lam, self.m, "lam"), self._vec(dc, nd, "dc")
        u, w = np.empty(self.n), np.empty(max(self.m, 1))
        self._check(self._lib.asm_eval_data_cross(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.dptr(dc), _lib.dptr(u), _lib.dptr(w)))
        return u, w[:self.m]

    @staticmethod
    def _kkt_params(max_iter, rtol):
        if max_iter is None and rtol is None:
            return None
        if max_iter is None or rtol is None:
            raise ValueError("give max_iter and rtol together (asm_kkt_params), or neither for the defaults")
        return C.byref(_lib.KktParams(int(max_iter), float(rtol)))

    def set_kkt_form(self, form):
        """asm_kkt_set_form: "dense" (the default) or "sparse" for every later KKT entry on this handle - kkt_solve, kkt_step, their multi
        forms, the sensitivities, eqp_trial and the native SLP-EQP driver.  Needs eval_setup, and the next eval_setup starts from "dense"
        again.  Without a sparse pattern the sparse form runs the dense one and says so in kkt_form_info().form_used."""
        if form not in _lib.KKT_FORMS:
            raise ValueError("kkt form %r: expected one of %s" % (form, ", ".join(repr(k) for k in _lib.KKT_FORMS)))
        self._check(self._lib.asm_kkt_set_form(self._h, _lib.KKT_FORMS[form]))

    def kkt_form_info(self):
        """The asm_kkt_form_info structure of the last KKT call on this handle: form_requested, form_used (0 dense, 1 sparse), band, n_pairs,
        order_reused, dense_bytes, sparse_bytes, order_ms."""
        info = _lib.KktFormInfo()
        self._check(self._lib.asm_kkt_form_info(self._h, C.byref(info)))
        return info

    def set_kkt_order(self, order):
        """asm_kkt_set_order: the row order of the sparse form, "working-set" (the default: a new order for every new working set, made on
        the host) or "static" (one order of all rows, made once, restricted to the working set: no ordering, upload or wait per call).
        Needs eval_setup, and the next eval_setup starts from "working-set" again.  No effect in the dense form."""
        if not isinstance(order, str) or order not in _lib.KKT_ORDERS:
            raise ValueError("kkt order %r: expected one of %s" % (order, ", ".join(repr(k) for k in _lib.KKT_ORDERS)))
        self._check(self._lib.asm_kkt_set_order(self._h, _lib.KKT_ORDERS[order]))

    def kkt_order_info(self):
        """The asm_kkt_order_info structure: order_requested, order_used by the last KKT call (0 working-set, 1 static), all_band and
        all_pairs of the order of all rows."""
        info = _lib.KktOrderInfo()
        self._check(self._lib.asm_kkt_order_info(self._h, C.byref(info)))
        return info

    def kkt_row_order(self):
        """asm_kkt_row_order: the working rows (0-based) of the last KKT call on this handle in the order it used."""
        nW = C.c_int64(0)
        self._check(self._lib.asm_kkt_row_order(self._h, None, C.byref(nW)))
        rows = np.zeros(max(int(nW.value), 1), np.int32)
        self._check(self._lib.asm_kkt_row_order(self._h, _lib.i32ptr(rows), C.byref(nW)))
        return rows[:int(nW.value)]

    def kkt_solve(self, x, lam, row_state, bound_state, ru, rw, max_iter=None, rtol=None):
        """(dx, dlam, dz, info) of asm_kkt_solve: the KKT system of the working set (row_state 0 / 1, bound_state -1 / 0 / +1) at (x, lam)
        with the right-hand sides (-ru, -rw); info is the asm_kkt_info structure (status 0 solved, 1 iteration limit, 2 reduced Hessian
        not positive definite, 3 dependent working rows)."""
        x, lam = self._vec(x, self.n, "x"), self._vec(lam, self.m, "lam")
        ru, rw = self._vec(ru, self.n, "ru"), self._vec(rw, self.m, "rw")
        rs, bs = self._states(row_state, bound_state)
        dx, dlam, dz, info = np.empty(self.n), np.empty(max(self.m, 1)), np.empty(self.n), _lib.KktInfo()
        self._check(self._lib.asm_kkt_solve(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), _lib.dptr(ru), _lib.dptr(rw),
                                            self._kkt_params(max_iter, rtol), _lib.dptr(dx), _lib.dptr(dlam), _lib.dptr(dz), C.byref(info)))
        return dx, dlam[:self.m], dz, info

    def solution_sensitivity(self, x, lam, row_state, bound_state, dc, max_iter=None, rtol=None):
        """(dx, dlam, dz, info) of asm_solution_sensitivity: the directional derivative of the solution and its multipliers along the
        direction dc in the block's data (expression blocks and the block kernels with derivatives), on the working set given."""
        nd = len(self._ev_keep[2]) if getattr(self, "_ev_keep", None) is not None else 0
        x, lam, dc = self._vec(x, self.n, "x"), self._vec(lam, self.m, "lam"), self._vec(dc, nd, "dc")
        rs, bs = self._states(row_state, bound_state)
        dx, dlam, dz, info = np.empty(self.n), np.empty(max(self.m, 1)), np.empty(self.n), _lib.KktInfo()
        self._check(self._lib.asm_solution_sensitivity(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), _lib.dptr(dc),
                                                       self._kkt_params(max_iter, rtol), _lib.dptr(dx), _lib.dptr(dlam), _lib.dptr(dz), C.byref(info)))
        return dx, dlam[:self.m], dz, info

    def _mat(self, a, cols, name, nrhs=None):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != cols or a.shape[0] < 1 or (nrhs is not None and a.shape[0] != nrhs):
            raise ValueError("%s has shape %r, expected (%s, %d) with at least one row" % (name, a.shape, "nrhs" if nrhs is None else nrhs, cols))
        return a if cols else np.zeros((a.shape[0], 1))

    def _multi_outputs(self, nrhs):
        return np.empty((nrhs, self.n)), np.empty((nrhs, max(self.m, 1))), np.empty((nrhs, self.n)), (_lib.KktInfo * nrhs)()

    def kkt_solve_multi(self, x, lam, row_state, bound_state, RU, RW, max_iter=None, rtol=None):
        """(DX, DLAM, DZ, infos) of asm_kkt_solve_multi: kkt_solve for the nrhs right-hand sides in the rows of RU [nrhs x n] and
        RW [nrhs x m] on one factor; row c of DX [nrhs x n], DLAM [nrhs x m], DZ [nrhs x n] and infos[c] (asm_kkt_info) answer row c."""
        x, lam = self._vec(x, self.n, "x"), self._vec(lam, self.m, "lam")
        par = self._kkt_params(max_iter, rtol)
        RU = self._mat(RU, self.n, "RU")
        RW = self._mat(RW, self.m, "RW", RU.shape[0])
        rs, bs = self._states(row_state, bound_state)
        nrhs = RU.shape[0]
        DX, DLAM, DZ, infos = self._multi_outputs(nrhs)
        self._check(self._lib.asm_kkt_solve_multi(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), nrhs, _lib.dptr(RU), _lib.dptr(RW),
                                                  par, _lib.dptr(DX), _lib.dptr(DLAM), _lib.dptr(DZ), infos))
        return DX, DLAM[:, :self.m], DZ, list(infos)

    def solution_sensitivity_multi(self, x, lam, row_state, bound_state, DC, max_iter=None, rtol=None):
        """(DX, DLAM, DZ, infos) of asm_solution_sensitivity_multi: solution_sensitivity for the nrhs directions in the rows of
        DC [nrhs x n_dpar] on one factor, one row of the outputs per direction (expression blocks and the block kernels with derivatives)."""
        nd = len(self._ev_keep[2]) if getattr(self, "_ev_keep", None) is not None else 0
        x, lam = self._vec(x, self.n, "x"), self._vec(lam, self.m, "lam")
        par = self._kkt_params(max_iter, rtol)
        DC = self._mat(DC, nd, "DC")
        rs, bs = self._states(row_state, bound_state)
        nrhs = DC.shape[0]
        DX, DLAM, DZ, infos = self._multi_outputs(nrhs)
        self._check(self._lib.asm_solution_sensitivity_multi(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), nrhs, _lib.dptr(DC),
                                                             par, _lib.dptr(DX), _lib.dptr(DLAM), _lib.dptr(DZ), infos))
        return DX, DLAM[:, :self.m], DZ, list(infos)

    def bound_sensitivity_multi(self, x, lam, row_state, bound_state, rows, delta=None, max_iter=None, rtol=None):
        """(DX, DLAM, DZ, infos) of asm_bound_sensitivity_multi: column c is kkt_solve_multi with ru = 0 and rw[rows[c]] = -delta[c]
        (delta None: -1), bit for bit, with the right-hand sides made on the device (sensitivity.bound_rhs states them).  rows: 0-based
        rows, duplicates allowed; a row outside the working set gives the zero column."""
        x, lam = self._vec(x, self.n, "x"), self._vec(lam, self.m, "lam")
        par = self._kkt_params(max_iter, rtol)
        rows = np.ascontiguousarray(np.atleast_1d(rows), dtype=np.int32)
        if rows.ndim != 1 or len(rows) < 1:
            raise ValueError("rows has shape %r, expected (nrhs,) with at least one row" % (rows.shape,))
        nrhs = len(rows)
        if delta is not None:
            delta = self._vec(delta, nrhs, "delta")
        rs, bs = self._states(row_state, bound_state)
        DX, DLAM, DZ, infos = self._multi_outputs(nrhs)
        self._check(self._lib.asm_bound_sensitivity_multi(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), nrhs, _lib.i32ptr(rows),
                                                          None if delta is None else _lib.dptr(delta), par, _lib.dptr(DX), _lib.dptr(DLAM), _lib.dptr(DZ), infos))
        return DX, DLAM[:, :self.m], DZ, list(infos)

    def var_bound_sensitivity_multi(self, x, lam, row_state, bound_state, vars, delta=None, max_iter=None, rtol=None):
        """(DX, DLAM, DZ, infos) of asm_var_bound_sensitivity_multi: column c moves the bound that variable vars[c] sits at by delta[c]
        (delta None: 1) - kkt_solve_multi with ru = delta H[:, j], rw = delta J[:, j], bit for bit, and DX[c, j] = delta[c] - with the
        right-hand sides made on the device (sensitivity.var_bound_rhs states them).  vars: 0-based variables, duplicates allowed; a
        variable outside B gives the zero column.  vars None goes to the library as a null pointer (refused)."""
        x, lam = self._vec(x, self.n, "x"), self._vec(lam, self.m, "lam")
        par = self._kkt_params(max_iter, rtol)
        if vars is not None:
            vars = np.ascontiguousarray(np.atleast_1d(vars), dtype=np.int32)
            if vars.ndim != 1 or len(vars) < 1:
                raise ValueError("vars has shape %r, expected (nrhs,) with at least one variable" % (vars.shape,))
        nrhs = 1 if vars is None else len(vars)
        if delta is not None:
            delta = self._vec(delta, nrhs, "delta")
        rs, bs = self._states(row_state, bound_state)
        DX, DLAM, DZ, infos = self._multi_outputs(nrhs)
        self._check(self._lib.asm_var_bound_sensitivity_multi(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), nrhs,
                                                              None if vars is None else _lib.i32ptr(vars), None if delta is None else _lib.dptr(delta), par,
                                                              _lib.dptr(DX), _lib.dptr(DLAM), _lib.dptr(DZ), infos))
        return DX, DLAM[:, :self.m], DZ, list(infos)

    # ------------------------------------------------------------------ validity ranges (include/asm_hip.h: "Validity ranges")
    def sensitivity_range(self, x, lam, mult_x_U, mult_x_L, row_state, bound_state, DX, DLAM, DZ):
        """asm_sensitivity_range_multi: for every column (row c of DX [nrhs x n], DLAM [nrhs x m], DZ [nrhs x n] - the outputs of the
        sensitivity entries) the range of t on which x + t DX[c], lam + t DLAM[c], z + t DZ[c] keep the working set (row_state,
        bound_state), z = mult_x_U + mult_x_L, with the handle's bounds.  Returns a structured array [nrhs] with the fields of
        asm_range_info: t_lo <= 0 <= t_hi and what blocks at either end, pos_* (row i, or m + variable j; -1 none) and kind_*
        (sensitivity.RANGE_KINDS).  sensitivity.validity_range_host is its NumPy twin."""
        x, lam = self._vec(x, self.n, "x"), self._vec(lam, self.m, "lam")
        z = self._vec(mult_x_U, self.n, "mult_x_U") + self._vec(mult_x_L, self.n, "mult_x_L")
        DX = self._mat(DX, self.n, "DX")
        nrhs = DX.shape[0]
        DLAM, DZ = self._mat(DLAM, self.m, "DLAM", nrhs), self._mat(DZ, self.n, "DZ", nrhs)
        rs, bs = self._states(row_state, bound_state)
        out = np.zeros(nrhs, dtype=_lib.RangeInfo)
        self._check(self._lib.asm_sensitivity_range_multi(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.dptr(z), _lib.i32ptr(rs), _lib.i32ptr(bs), nrhs, _lib.dptr(DX),
                                                          _lib.dptr(DLAM), _lib.dptr(DZ), out.ctypes.data_as(C.POINTER(_lib.RangeInfo))))
        return out

    # ------------------------------------------------------------------ adjoint sensitivities (include/asm_hip.h: "Adjoint solution sensitivities")
    def data_cross_t(self, x, lam, vx, vl):
        """out [n_dpar] of asm_eval_data_cross_t: out[c] = vx' d/d dpar[c] (grad_x (f - lam' g)) + vl' d g / d dpar[c] for weights vx [n],
        vl [m] - for every direction dc, dc' out = vx' u + vl' w with (u, w) = data_cross(x, lam, dc).  Expression blocks and the block
        kernels with derivatives."""
        nd = getattr(self, "_ev_nd", 0)
        x, lam, vx, vl = self._vec(x, self.n, "x"), self._vec(lam, self.m, "lam"), self._vec(vx, self.n, "vx"), self._vec(vl, self.m, "vl")
        out = np.empty(max(nd, 1))
        self._check(self._lib.asm_eval_data_cross_t(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.dptr(vx), _lib.dptr(vl), _lib.dptr(out)))
        return out[:nd]

    def solution_adjoint(self, x, lam, row_state, bound_state, gx, gl, max_iter=None, rtol=None):
        """(out, dbound, ax, al, info) of asm_solution_adjoint for a function phi(x*, lam*) with gradients gx [n], gl [m], on the working
        set given: out [n_dpar] = d phi / d dpar, dbound [m] = d phi / d(bound of row i) (0 outside the working set), (ax, al) the adjoint
        state kkt_solve(ru = -gx, rw = gl), info the solve's asm_kkt_info.  One KKT solve whatever n_dpar."""
        nd = getattr(self, "_ev_nd", 0)
        x, lam, gx, gl = self._vec(x, self.n, "x"), self._vec(lam, self.m, "lam"), self._vec(gx, self.n, "gx"), self._vec(gl, self.m, "gl")
        rs, bs = self._states(row_state, bound_state)
        out, dbound, ax, al, info = np.empty(max(nd, 1)), np.empty(max(self.m, 1)), np.empty(self.n), np.empty(max(self.m, 1)), _lib.KktInfo()
        self._check(self._lib.asm_solution_adjoint(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), _lib.dptr(gx), _lib.dptr(gl),
                                                   self._kkt_params(max_iter, rtol), _lib.dptr(out), _lib.dptr(dbound), _lib.dptr(ax), _lib.dptr(al), C.byref(info)))
        return out[:nd], dbound[:self.m], ax, al[:self.m], info

    def solution_adjoint_multi(self, x, lam, row_state, bound_state, GX, GL, max_iter=None, rtol=None):
        """(OUT, DBOUND, AX, AL, infos) of asm_solution_adjoint_multi: solution_adjoint for the nrhs functions whose gradients are the rows
        of GX [nrhs x n] and GL [nrhs x m], on one factor; row c of OUT [nrhs x n_dpar], DBOUND, AL [nrhs x m], AX [nrhs x n] and infos[c]
        answer row c."""
        nd = getattr(self, "_ev_nd", 0)
        x, lam = self._vec(x, self.n, "x"), self._vec(lam, self.m, "lam")
        par = self._kkt_params(max_iter, rtol)
        GX = self._mat(GX, self.n, "GX")
        GL = self._mat(GL, self.m, "GL", GX.shape[0])
        rs, bs = self._states(row_state, bound_state)
        nrhs = GX.shape[0]
        OUT, DBOUND, AL = np.empty((nrhs, max(nd, 1))), np.empty((nrhs, max(self.m, 1))), np.empty((nrhs, max(self.m, 1)))
        AX, infos = np.empty((nrhs, self.n)), (_lib.KktInfo * nrhs)()
        # (the library's matrices are packed: nrhs x n_dpar and nrhs x m, so a padded column is given only when the true width is 0)
        self._check(self._lib.asm_solution_adjoint_multi(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), nrhs, _lib.dptr(GX), _lib.dptr(GL),
                                                         par, _lib.dptr(OUT), _lib.dptr(DBOUND), _lib.dptr(AX), _lib.dptr(AL), infos))
        return OUT[:, :nd], DBOUND[:, :self.m], AX, AL[:, :self.m], list(infos)

    def solution_adjoint_z(self, x, lam, row_state, bound_state, gx, gl, gz=None, max_iter=None, rtol=None):
        """(out, dbound, dxbound, ax, al, info) of asm_solution_adjoint_z for a function phi(x*, lam*, z*) with gradients gx [n], gl [m] and
        gz [n] (None: 0; entries on free variables are ignored - z exists on B only): solution_adjoint's outputs and
        dxbound [n] = d phi / d(bound variable j sits at), 0 on F.  gz None: solution_adjoint's bits."""
        nd = getattr(self, "_ev_nd", 0)
        x, lam, gx, gl = self._vec(x, self.n, "x"), self._vec(lam, self.m, "lam"), self._vec(gx, self.n, "gx"), self._vec(gl, self.m, "gl")
        if gz is not None:
            gz = self._vec(gz, self.n, "gz")
        rs, bs = self._states(row_state, bound_state)
        out, dbound, ax, al, info = np.empty(max(nd, 1)), np.empty(max(self.m, 1)), np.empty(self.n), np.empty(max(self.m, 1)), _lib.KktInfo()
        dxbound = np.empty(self.n)
        self._check(self._lib.asm_solution_adjoint_z(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), _lib.dptr(gx), _lib.dptr(gl),
                                                     None if gz is None else _lib.dptr(gz), self._kkt_params(max_iter, rtol), _lib.dptr(out), _lib.dptr(dbound),
                                                     _lib.dptr(dxbound), _lib.dptr(ax), _lib.dptr(al), C.byref(info)))
        return out[:nd], dbound[:self.m], dxbound, ax, al[:self.m], info

    def solution_adjoint_z_multi(self, x, lam, row_state, bound_state, GX, GL, GZ=None, max_iter=None, rtol=None):
        """(OUT, DBOUND, DXBOUND, AX, AL, infos) of asm_solution_adjoint_z_multi: solution_adjoint_z for the nrhs functions whose gradients
        are the rows of GX [nrhs x n], GL [nrhs x m] and GZ [nrhs x n] (None: 0), on one factor."""
        nd = getattr(self, "_ev_nd", 0)
        x, lam = self._vec(x, self.n, "x"), self._vec(lam, self.m, "lam")
        par = self._kkt_params(max_iter, rtol)
        GX = self._mat(GX, self.n, "GX")
        GL = self._mat(GL, self.m, "GL", GX.shape[0])
        if GZ is not None:
            GZ = self._mat(GZ, self.n, "GZ", GX.shape[0])
        rs, bs = self._states(row_state, bound_state)
        nrhs = GX.shape[0]
        OUT, DBOUND, AL = np.empty((nrhs, max(nd, 1))), np.empty((nrhs, max(self.m, 1))), np.empty((nrhs, max(self.m, 1)))
        AX, DXBOUND, infos = np.empty((nrhs, self.n)), np.empty((nrhs, self.n)), (_lib.KktInfo * nrhs)()
        self._check(self._lib.asm_solution_adjoint_z_multi(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), nrhs, _lib.dptr(GX), _lib.dptr(GL),
                                                           None if GZ is None else _lib.dptr(GZ), par, _lib.dptr(OUT), _lib.dptr(DBOUND), _lib.dptr(DXBOUND),
                                                           _lib.dptr(AX), _lib.dptr(AL), infos))
        return OUT[:, :nd], DBOUND[:, :self.m], DXBOUND, AX, AL[:, :self.m], list(infos)

    @staticmethod
    def _kkt_step_params(max_iter, rtol, normal_share):
        if max_iter is None and rtol is None and normal_share is None:
            return None
        if max_iter is None or rtol is None or normal_share is None:
            raise ValueError("give max_iter, rtol and normal_share together (asm_kkt_step_params), or none of them for the defaults")
        return C.byref(_lib.KktStepParams(int(max_iter), float(rtol), float(normal_share)))

    def kkt_step(self, x, lam, row_state, bound_state, ru, rw, radius, max_iter=None, rtol=None, normal_share=None):
        """(dx, dlam, dz, info) of asm_kkt_step: the trust-region step on the working set - kkt_solve with an l2 radius (+inf: kkt_solve
        itself); info is the asm_kkt_step_info structure (asm_kkt_info's fields, boundary, theta, norm_normal, norm_step, model)."""
        x, lam = self._vec(x, self.n, "x"), self._vec(lam, self.m, "lam")
        ru, rw = self._vec(ru, self.n, "ru"), self._vec(rw, self.m, "rw")
        rs, bs = self._states(row_state, bound_state)
        dx, dlam, dz, info = np.empty(self.n), np.empty(max(self.m, 1)), np.empty(self.n), _lib.KktStepInfo()
        self._check(self._lib.asm_kkt_step(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), _lib.dptr(ru), _lib.dptr(rw), float(radius),
                                           self._kkt_step_params(max_iter, rtol, normal_share), _lib.dptr(dx), _lib.dptr(dlam), _lib.dptr(dz), C.byref(info)))
        return dx, dlam[:self.m], dz, info

    def kkt_step_multi(self, x, lam, row_state, bound_state, RU, RW, radii, max_iter=None, rtol=None, normal_share=None):
        """(DX, DLAM, DZ, infos) of asm_kkt_step_multi: kkt_step for the nrhs right-hand sides in the rows of RU [nrhs x n] and
        RW [nrhs x m], each with its own radius (radii [nrhs]), on one factor - equal rows answer a ladder of radii."""
        x, lam = self._vec(x, self.n, "x"), self._vec(lam, self.m, "lam")
        par = self._kkt_step_params(max_iter, rtol, normal_share)
        RU = self._mat(RU, self.n, "RU")
        RW = self._mat(RW, self.m, "RW", RU.shape[0])
        nrhs = RU.shape[0]
        radii = self._vec(radii, nrhs, "radii")
        rs, bs = self._states(row_state, bound_state)
        DX, DLAM, DZ = self._multi_outputs(nrhs)[:3]
        infos = (_lib.KktStepInfo * nrhs)()
        self._check(self._lib.asm_kkt_step_multi(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(rs), _lib.i32ptr(bs), nrhs, _lib.dptr(RU), _lib.dptr(RW),
                                                 _lib.dptr(radii), par, _lib.dptr(DX), _lib.dptr(DLAM), _lib.dptr(DZ), infos))
        return DX, DLAM[:, :self.m], DZ, list(infos)

    def eqp_trial(self, x, lam, lp_row_state, lp_bound_state, radius, nu, tol_active=1e-8, max_iter=None, rtol=None, normal_share=None):
        """(d, lam_new, mult_x_U, mult_x_L, row_state, bound_state, info) of asm_eqp_trial: the SLP-EQP trial step at the point of the last
        eval_functions(x) - the working set the LP's active set (lp_row_state [m + n_adj], lp_bound_state [n]: active_set()) names there,
        the trust-region step on it, d = t dx inside the variable bounds and the merit values at x and x + d (info: asm_eqp_info)."""
        x, lam, nu = self._vec(x, self.n, "x"), self._vec(lam, self.m, "lam"), self._vec(nu, self.m, "nu")
        d = self.data
        nadj = int(((d.c_lb > -np.inf) & (d.c_ub < np.inf) & (d.c_lb != d.c_ub)).sum())
        lr = np.ascontiguousarray(np.atleast_1d(lp_row_state), dtype=np.int32)
        lb = np.ascontiguousarray(np.atleast_1d(lp_bound_state), dtype=np.int32)
        if lr.shape != (self.m + nadj,) or lb.shape != (self.n,):
            raise ValueError("the LP's row_state / bound_state have shapes %r / %r, expected (%d,) / (%d,)" % (lr.shape, lb.shape, self.m + nadj, self.n))
        if not len(lr):
            lr = np.zeros(1, np.int32)
        step, lam_new, mU, mL = np.empty(self.n), np.empty(max(self.m, 1)), np.empty(self.n), np.empty(self.n)
        rs, bs, info = np.zeros(max(self.m, 1), np.int32), np.zeros(self.n, np.int32), _lib.EqpInfo()
        self._check(self._lib.asm_eqp_trial(self._h, _lib.dptr(x), _lib.dptr(lam), _lib.i32ptr(lr), _lib.i32ptr(lb), float(radius), _lib.dptr(nu), float(tol_active),
                                            self._kkt_step_params(max_iter, rtol, normal_share), _lib.dptr(step), _lib.dptr(lam_new), _lib.dptr(mU), _lib.dptr(mL),
                                            _lib.i32ptr(rs), _lib.i32ptr(bs), C.byref(info)))
        return step, lam_new[:self.m], mU, mL, rs[:self.m], bs, info

    # ------------------------------------------------------------------ limited-memory Hessian (include/asm_hip.h, "Limited-memory Hessian")
    def set_hessian_type(self, kind, memory=10):
        """asm_hessian_set_type: "exact" (the default) or "limited-memory" with `memory` pairs (1 .. 32) for every later kkt_solve, kkt_step,
        their multi forms, eqp_trial and the native SLP-EQP driver on this handle.  Clears the store.  The derivative entries (Hessians,
        data_cross, the sensitivities) stay exact."""
        if kind not in _lib.HESSIAN_TYPES:
            raise ValueError("hessian type %r: expected one of %s" % (kind, ", ".join(repr(k) for k in _lib.HESSIAN_TYPES)))
        self._check(self._lib.asm_hessian_set_type(self._h, _lib.HESSIAN_TYPES[kind], int(memory)))

    def lm_reset(self):
        """asm_lm_reset: forget every stored pair (B = I)."""
        self._check(self._lib.asm_lm_reset(self._h))

    def lm_push_pair(self, s, y):
        """asm_lm_push_pair: offer the pair (s, y) to the store; the skip rule decides on the device (lm_info() counts)."""
        s, y = self._vec(s, self.n, "s"), self._vec(y, self.n, "y")
        self._check(self._lib.asm_lm_push_pair(self._h, _lib.dptr(s), _lib.dptr(y)))

    def lm_begin(self, lam):
        """asm_lm_begin: before x changes, save x and grad f - J' lam from where the last eval_functions left them."""
        lam = self._vec(lam, self.m, "lam")
        self._check(self._lib.asm_lm_begin(self._h, _lib.dptr(lam)))

    def lm_end(self, lam):
        """asm_lm_end: after the next eval_functions, form the pair with the same lam and push it; nothing without a pending lm_begin."""
        lam = self._vec(lam, self.m, "lam")
        self._check(self._lib.asm_lm_end(self._h, _lib.dptr(lam)))

    def lm_product(self, V):
        """asm_lm_product: B v for a vector [n], or the rows of V [nrhs x n] (a row's bits do not depend on the rows beside it)."""
        V = np.asarray(V, dtype=np.float64)
        if V.ndim == 1:
            return self.lm_product(V[None, :])[0]
        V = self._mat(V, self.n, "V")
        out = np.empty_like(V)
        self._check(self._lib.asm_lm_product(self._h, _lib.dptr(V), V.shape[0], _lib.dptr(out)))
        return out

    def lm_info(self):
        """The asm_lm_info structure: type, memory, pairs, pending, pushed, skipped_zero, skipped_curvature, sigma, bytes."""
        info = _lib.LmInfo()
        self._check(self._lib.asm_lm_info(self._h, C.byref(info)))
        return info

    def slp_norms(self, lam, mult_x_U, mult_x_L):
        """(norm_violations(Inf), norm_violations(1), KT_residuals, norm_complementarity(Inf)) - common.jl:35-98 - on the device."""
        out = np.empty(4)
        lam, mult_x_U, mult_x_L = map(_f64, (lam, mult_x_U, mult_x_L))
        self._check(self._lib.asm_slp_norms(self._h, _lib.dptr(lam), _lib.dptr(mult_x_U), _lib.dptr(mult_x_L), _lib.dptr(out)))
        return tuple(float(v) for v in out)

    def slp_merit(self, mode, alpha, p, nu, p_slack, feasibility, prim_infeas):
        """mode 0: compute_phi(x, alpha, p) (slp.jl:79-115); mode 1: compute_derivative (slp.jl:122-147)."""
        ps = self._flat_slacks(p_slack)
        out = C.c_double(0.0)
        p, nu = _f64(p), _f64(nu)
        self._check(self._lib.asm_slp_merit(self._h, int(mode), float(alpha), _lib.dptr(p), _lib.dptr(nu), _lib.dptr(ps), int(bool(feasibility)),
                                            float(prim_infeas) if np.isfinite(prim_infeas) else 0.0, C.byref(out)))
        return out.value

    def _flat_slacks(self, p_slack):
        ps = getattr(p_slack, "raw", None)
        if ps is None:
            ps = np.full(2 * max(self.m, 1), np.nan)
            for i in range(self.m):
                v = p_slack.get(i, [0.0]) if p_slack else [0.0]
                ps[2 * i] = v[0]
                if len(v) > 1:
                    ps[2 * i + 1] = v[1]
        return ps

    def slp_line_search(self, p, nu, p_slack, feasibility, prim_infeas, phi0, D, eta, tau, min_alpha):
        """compute_alpha (slp_line_search.jl:222-244) with the trial points evaluated on the device (asm_slp_line_search).
        Returns (alpha, phi(alpha), trials, ok)."""
        ps = self._flat_slacks(p_slack)
        p, nu = _f64(p), _f64(nu)
        alpha, phi = C.c_double(0.0), C.c_double(0.0)
        trials, ok = C.c_int(0), C.c_int(0)
        self._check(self._lib.asm_slp_line_search(self._h, _lib.dptr(p), _lib.dptr(nu), _lib.dptr(ps), int(bool(feasibility)),
                                                  float(prim_infeas) if np.isfinite(prim_infeas) else 0.0, float(phi0), float(D), float(eta), float(tau),
                                                  float(min_alpha), C.byref(alpha), C.byref(phi), C.byref(trials), C.byref(ok)))
        return alpha.value, phi.value, trials.value, bool(ok.value)

    def step_quality(self, p, nu, p_slack, feasibility, prim_infeas):
        """step_quality's merit values (slp_trust_region.jl:213-216) with x + p evaluated on the device (asm_slp_step_quality):
        (compute_derivative, compute_phi(x, 0, p), compute_phi(x, 1, p)), each equal to the slp_merit call's value."""
        ps = self._flat_slacks(p_slack)
        p, nu = _f64(p), _f64(nu)
        out = np.empty(3)
        self._check(self._lib.asm_slp_step_quality(self._h, _lib.dptr(p), _lib.dptr(nu), _lib.dptr(ps), int(bool(feasibility)),
                                                   float(prim_infeas) if np.isfinite(prim_infeas) else 0.0, _lib.dptr(out)))
        return tuple(float(v) for v in out)

    def slp_run(self, x0, parameters, max_lp_solves=0):
        """One complete SLP run inside the library (asm_slp_run for Line Search, asm_slp_run_tr for Trust Region, asm_slp_run_eqp for
        SLP-EQP, by `parameters.algorithm`) from x0 on this handle; needs eval_setup.  Returns a batch.NativeRun."""
        from .batch import NATIVE_ALGORITHMS, NativeRun, slp_eqp_params, slp_params
        if parameters.algorithm not in NATIVE_ALGORITHMS:
            raise ValueError("the native drivers are run!(::SlpLS), run!(::SlpTR) and SLP-EQP, not %r" % parameters.algorithm)
        par = slp_params(parameters, max_lp_solves)
        x0 = _f64(x0)
        x = np.empty(self.n); lam = np.empty(max(self.m, 1)); mU = np.empty(self.n); mL = np.empty(self.n); g = np.empty(max(self.m, 1))
        res = _lib.SlpResult()
        outs = (_lib.dptr(x), _lib.dptr(lam), _lib.dptr(mU), _lib.dptr(mL), _lib.dptr(g), C.byref(res))
        tr = None
        if parameters.algorithm == "SLP-EQP":
            tr, eq = _lib.SlpTrInfo(), _lib.SlpEqpInfo()
            ep = slp_eqp_params(parameters)
            self._check(self._lib.asm_slp_run_eqp(self._h, C.byref(par), float(parameters.tr_size), C.byref(ep), _lib.dptr(x0), *outs, C.byref(tr), C.byref(eq)))
            return NativeRun(res, x, lam[:self.m], mU, mL, g[:self.m], tr, eq)
        if parameters.algorithm == "Trust Region":
            tr = _lib.SlpTrInfo()
            self._check(self._lib.asm_slp_run_tr(self._h, C.byref(par), float(parameters.tr_size), _lib.dptr(x0), *outs, C.byref(tr)))
        else:
            self._check(self._lib.asm_slp_run(self._h, C.byref(par), _lib.dptr(x0), *outs))
        return NativeRun(res, x, lam[:self.m], mU, mL, g[:self.m], tr)

    # per-iteration reductions on the resident Jacobian (common.jl:35-44, slp.jl:54-66)
    def kt_residuals(self, df, lam, mult_x_U, mult_x_L):
        out = C.c_double(0.0)
        df, lam, mult_x_U, mult_x_L = map(_f64, (df, lam, mult_x_U, mult_x_L))
        self._check(self._lib.asm_kt_residuals(self._h, _lib.dptr(df), _lib.dptr(lam), _lib.dptr(mult_x_U), _lib.dptr(mult_x_L), C.byref(out)))
        return out.value

    def jac_row_norms(self):
        out = np.empty(max(self.m, 1))
        self._check(self._lib.asm_jac_row_norms(self._h, _lib.dptr(out)))
        return out[:self.m]
