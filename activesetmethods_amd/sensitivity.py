"""Solution sensitivities at an SLP solution: how x* and its multipliers move with the data (include/asm_hip.h, "Cross derivatives of
an expression block" and "The KKT solve on a working set").

On the working set of a solution - the rows W that sit at a bound, the variables B that sit at a bound, F the other variables - the
first-order change of (x*, lam*) along a direction dc of the data solves, with H the Hessian of f - lam' g, J the Jacobian, A = J[W, F],

    H_FF dx_F - A' dlam_W = -u_F ,     A dx_F = -w_W ,     dx_B = 0 ,    dlam_i = 0 (i not in W)

with u = d/dc (grad_x (f - lam' g)) . dc and w = (dg/dc) . dc (asm_eval_data_cross / ExprBlock.data_cross, NlpBlock.data_cross of the
block kernels with derivatives).  A constraint bound that moves by d(bound_i) enters as u = 0, w_i = -d(bound_i).

    working_set          (row_state, bound_state) of a solution
    kkt_reference        the system assembled densely and solved with numpy.linalg.solve: the independent answer
    kkt_pcg              the NumPy twin of the device algorithm (asm_kkt_solve): Cholesky of A A', projected conjugate gradients
    solution_sensitivity the device call on a handle, or on a fresh one for a Model
    kkt_reference_multi  kkt_reference for many right-hand sides: one dense system, one numpy.linalg.solve with a matrix right-hand side
    kkt_pcg_multi        kkt_pcg column by column: what the lockstep iteration of asm_kkt_solve_multi computes
    solution_jacobian    dx*/dc and dlam*/dc for a list of constants, as matrices (asm_solution_sensitivity_multi, unit directions)
    bound_jacobian       dx*/d(bound) and dlam*/d(bound) for a list of working rows (asm_kkt_solve_multi)
    bound_rhs            the right-hand sides of bound sensitivities as matrices: what asm_bound_sensitivity_multi makes on the device
    predict              the first-order prediction x + step * dx

Reverse mode ("Adjoint solution sensitivities"): for one function phi(x*, lam*) with gradients (gx, gl) the KKT matrix of the working
set is symmetric, so d phi / d dpar for ALL constants is one solve - the adjoint state (ax, al) = kkt(ru = -gx, rw = gl) - and one
transposed cross derivative with the weights (-ax, al); d phi / d(bound_i) = -al_i on the working rows.

    model_cross_t        the host twin of asm_eval_data_cross_t for a FunctionModel (the block's data_cross_t on the model's rows)
    adjoint_reference    the dense kkt_reference plus that twin: the independent answer
    solution_adjoint     the device call on a handle (asm_solution_adjoint), or on a fresh one for a Model

Variable bounds and the bound multipliers z: the bounds of variables in B move by delta (supported on B), so dx_B = delta; (dx_F, dlam, dz)
is the solve with ru = H delta, rw = J delta, then dx += delta.  In reverse, phi(x*, lam*, z*) with a gradient gz on B: the adjoint solve
takes gx + H gz and gl - J gz, the transposed sweep vx = gz - ax, and d phi / d(xbound_j) = -dz_j of the adjoint solve on B.

    var_bound_rhs        the right-hand sides of variable-bound sensitivities: what asm_var_bound_sensitivity_multi makes on the device
    var_bound_reference  the dense system with dx_B = delta imposed directly: the independent answer
    var_bound_jacobian   dx*, dlam*, dz* / d(xbound) for a list of variables at a bound (asm_var_bound_sensitivity_multi)
    adjoint_reference_z  adjoint_reference with weights on z and the gradient with respect to the variable bounds

Validity ranges ("Validity ranges"): how far a column (dx, dlam, dz) may be followed before the working set changes - an inactive row
or a free variable reaches a bound, a multiplier of a working row or of a bound reaches zero.

    validity_range_host  the NumPy twin and the specification of the rule, V = J dx from dense_jacobian
    validity_range       the device call on a handle (asm_sensitivity_range_multi)
    RANGE_KINDS          names of the kinds 0..6 of what blocks

For the scenarios of a HipBatch: batch.working_sets, batch.solution_jacobians, batch.bound_jacobians, batch.var_bound_jacobians,
batch.validity_ranges.
"""
import numpy as np

from .moi_evaluator import lagrangian_hessian

PIVOT_THRESHOLD = 1e-10        # a pivot of A A' at or below this share of its diagonal entry is dropped (the library's static guard)
DROPPED = 1e256                # ... by putting this value in its place: the row leaves the solves


def model_hessian(fm, x, lam, hess=None):
    """The n x n matrix that stands for the Hessian of the Lagrangian in the twins: hess None - the model's own (lagrangian_hessian);
    a matrix - that matrix; a callable - an operator on row vectors, V [k x n] -> V B (lmhess.LMHessian.product), applied once to the
    identity."""
    if hess is None:
        return lagrangian_hessian(fm, x, lam)
    H = np.asarray(hess(np.eye(fm.n)), float).T if callable(hess) else np.asarray(hess, float)
    if H.shape != (fm.n, fm.n):
        raise ValueError("hess has shape %r, expected (%d, %d)" % (H.shape, fm.n, fm.n))
    return H


def dense_jacobian(fm, x):
    """The m x n Jacobian of a FunctionModel at x (duplicates of the pattern add)."""
    j_str = fm.jacobian_structure()
    vals = fm.eval_jac_g(np.asarray(x, float), np.zeros(len(j_str)))
    J = np.zeros((fm.m, fm.n))
    if j_str:
        r, c = np.array(j_str, np.int64).T - 1
        np.add.at(J, (r, c), vals)
    return J


def working_set(problem, x, lam, mult_x_U, mult_x_L, tol=1e-8):
    """(row_state [m] in {0, 1}, bound_state [n] in {-1, 0, +1}) at a solution of `problem` (n, m, x_L, x_U, g_L, g_U, eval_g).  A row is
    in the working set when it is an equality or its value sits at a bound within tol * (1 + |bound|); a variable is at its lower
    (-1) or upper (+1) bound likewise.  The multipliers are taken so that a solver's outputs pass through unchanged; only their
    lengths are checked - activity decides, so that a degenerate active row (zero multiplier) stays in the set."""
    x = np.asarray(x, float)
    n, m = int(problem.n), int(problem.m)
    if x.shape != (n,) or np.shape(lam) != (m,) or np.shape(mult_x_U) != (n,) or np.shape(mult_x_L) != (n,):
        raise ValueError("x, lam, mult_x_U, mult_x_L must have shapes (n,), (m,), (n,), (n,)")
    g_L, g_U = np.asarray(problem.g_L, float), np.asarray(problem.g_U, float)
    x_L, x_U = np.asarray(problem.x_L, float), np.asarray(problem.x_U, float)
    g = np.asarray(problem.eval_g(x, np.zeros(m)), float) if m else np.zeros(0)
    with np.errstate(invalid="ignore"):
        at = lambda v, b: np.isfinite(b) & (np.abs(v - b) <= tol * (1.0 + np.abs(b)))
        row_state = ((g_L == g_U) | at(g, g_L) | at(g, g_U)).astype(np.int32)
        lo, up = at(x, x_L), at(x, x_U)
    bound_state = np.where(lo, -1, np.where(up, 1, 0)).astype(np.int32)
    return row_state, bound_state


def _sets(fm, row_state, bound_state, ru, rw):
    rs, bs = np.asarray(row_state), np.asarray(bound_state)
    ru, rw = np.asarray(ru, float), np.asarray(rw, float)
    if rs.shape != (fm.m,) or bs.shape != (fm.n,) or ru.shape != (fm.n,) or rw.shape != (fm.m,):
        raise ValueError("row_state, bound_state, ru, rw must have shapes (m,), (n,), (n,), (m,)")
    if np.any((rs != 0) & (rs != 1)) or np.any(np.abs(bs) > 1):
        raise ValueError("row_state must hold 0 / 1 and bound_state -1 / 0 / +1")
    F, W = np.nonzero(bs == 0)[0], np.nonzero(rs == 1)[0]
    if len(W) > len(F):
        raise ValueError("more working rows (%d) than free variables (%d)" % (len(W), len(F)))
    return F, W, ru, rw


def _finish(H, J, F, W, ru, dxF, dlW, n, m):
    dx, dlam = np.zeros(n), np.zeros(m)
    dx[F], dlam[W] = dxF, dlW
    full = H @ dx + ru - J[W].T @ dlW
    dz = full.copy()
    dz[F] = 0.0
    return dx, dlam, dz


def kkt_reference(fm, x, lam, row_state, bound_state, ru, rw):
    """(dx, dlam, dz): the KKT system of the working set assembled densely, solved with numpy.linalg.solve."""
    F, W, ru, rw = _sets(fm, row_state, bound_state, ru, rw)
    H, J = lagrangian_hessian(fm, x, lam), dense_jacobian(fm, x)
    A = J[np.ix_(W, F)]
    nF, nW = len(F), len(W)
    K = np.zeros((nF + nW, nF + nW))
    K[:nF, :nF] = H[np.ix_(F, F)]
    K[:nF, nF:] = -A.T
    K[nF:, :nF] = A
    sol = np.linalg.solve(K, np.concatenate([-ru[F], -rw[W]])) if nF + nW else np.zeros(0)
    return _finish(H, J, F, W, ru, sol[:nF], sol[nF:], fm.n, fm.m)


def _guarded_cholesky(S):
    """Lower Cholesky factor with the library's static pivot guard: a pivot d <= PIVOT_THRESHOLD * S_ii becomes DROPPED.  Returns
    (L, number of dropped pivots)."""
    N = len(S)
    L = np.zeros((N, N))
    d0 = np.diag(S).copy()
    dropped = 0
    for j in range(N):
        d = S[j, j] - L[j, :j] @ L[j, :j]
        if not d > PIVOT_THRESHOLD * d0[j]:
            d = DROPPED
            dropped += 1
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L, dropped


def _substitute(L, b):
    """S^-1 b from the lower factor L of S: forward, then backward substitution (b itself without rows)."""
    nW = len(L)
    if not nW:
        return b
    y = np.zeros(nW)
    for i in range(nW):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    z = np.zeros(nW)
    for i in range(nW - 1, -1, -1):
        z[i] = (y[i] - L[i + 1:, i] @ z[i + 1:]) / L[i, i]
    return z


def kkt_pcg(fm, x, lam, row_state, bound_state, ru, rw, max_iter=None, rtol=1e-12, hess=None):
    """The NumPy twin of asm_kkt_solve, step by step the method of include/asm_hip.h: S = A A' factored with the pivot guard, the
    particular solution dx0 = -A' S^-1 rw_W, projected conjugate gradients on null(A) with the projection applied twice per
    iteration and the residual kept projected, the multipliers from S^-1 A (H_FF dx_F + ru_F); one refinement step for each of the
    two normal-equation solves outside the iteration.  hess: what stands for the Hessian (model_hessian; None: the model's own).
    Returns (dx, dlam, dz, info), info a dict with the fields of asm_kkt_info."""
    F, W, ru, rw = _sets(fm, row_state, bound_state, ru, rw)
    H, J = model_hessian(fm, x, lam, hess), dense_jacobian(fm, x)
    HF, A = H[np.ix_(F, F)], J[np.ix_(W, F)]
    nF, nW = len(F), len(W)
    if max_iter is None:
        max_iter = 2 * (nF - nW) + 20
    L, dropped = _guarded_cholesky(A @ A.T) if nW else (np.zeros((0, 0)), 0)

    s_solve = lambda b: _substitute(L, b)
    proj = lambda v: v - A.T @ s_solve(A @ v) if nW else v.copy()
    dx0 = -(A.T @ s_solve(rw[W])) if nW else np.zeros(nF)
    if nW:
        dx0 = dx0 - A.T @ s_solve(A @ dx0 + rw[W])         # one refinement step of the normal-equation solve
    d = np.zeros(nF)
    status, iters = 0, 0
    if nF > nW:
        r = ru[F] + HF @ dx0
        r = proj(proj(r))                                  # the residual is kept projected: r = g (no large component in range(A'))
        g = r
        rg, g0 = float(r @ g), float(np.sqrt(g @ g))
        p = -g
        stop = g0 == 0.0
        while not stop:
            if iters >= max_iter:
                status = 1
                break
            hp = HF @ p
            php = float(p @ hp)
            if not php > 0.0:
                status = 2
                break
            alpha = rg / php
            d = d + alpha * p
            r = r + alpha * hp
            r = proj(proj(r))
            g = r
            rg_new = float(r @ g)
            beta = rg_new / rg
            rg = rg_new
            iters += 1
            stop = float(np.sqrt(g @ g)) <= rtol * g0
            p = -g + beta * p
    dxF = dx0 + d
    q = HF @ dxF + ru[F]
    dlW = s_solve(A @ q) if nW else np.zeros(0)
    if nW:
        dlW = dlW + s_solve(A @ (q - A.T @ dlW))           # one refinement step
    if dropped:
        status = 3
    dx, dlam, dz = _finish(H, J, F, W, ru, dxF, dlW, fm.n, fm.m)
    info = dict(status=status, cg_iters=iters, n_free=nF, n_rows=nW, dropped_pivots=dropped,
                res_stat=float(np.abs(HF @ dxF - A.T @ dlW + ru[F]).max()) if nF else 0.0,
                res_feas=float(np.abs(A @ dxF + rw[W]).max()) if nW else 0.0)
    return dx, dlam, dz, info


def _rhs_matrices(fm, RU, RW):
    RU, RW = np.asarray(RU, float), np.asarray(RW, float)
    if RU.ndim != 2 or RW.ndim != 2 or RU.shape[0] < 1 or RU.shape[1] != fm.n or RW.shape != (RU.shape[0], fm.m):
        raise ValueError("RU, RW must have shapes (nrhs, n), (nrhs, m) with nrhs >= 1")
    return RU, RW


def kkt_reference_multi(fm, x, lam, row_state, bound_state, RU, RW):
    """(DX [nrhs x n], DLAM [nrhs x m], DZ [nrhs x n]): kkt_reference for the right-hand sides in the rows of RU, RW - the dense system
    assembled once, numpy.linalg.solve with a matrix right-hand side."""
    RU, RW = _rhs_matrices(fm, RU, RW)
    F, W, _, _ = _sets(fm, row_state, bound_state, RU[0], RW[0])
    H, J = lagrangian_hessian(fm, x, lam), dense_jacobian(fm, x)
    A = J[np.ix_(W, F)]
    nF, nW, K = len(F), len(W), len(RU)
    M = np.zeros((nF + nW, nF + nW))
    M[:nF, :nF] = H[np.ix_(F, F)]
    M[:nF, nF:] = -A.T
    M[nF:, :nF] = A
    sol = np.linalg.solve(M, np.concatenate([-RU[:, F], -RW[:, W]], axis=1).T) if nF + nW else np.zeros((0, K))
    DX, DLAM, DZ = np.zeros((K, fm.n)), np.zeros((K, fm.m)), np.zeros((K, fm.n))
    for c in range(K):
        DX[c], DLAM[c], DZ[c] = _finish(H, J, F, W, RU[c], sol[:nF, c], sol[nF:, c], fm.n, fm.m)
    return DX, DLAM, DZ


def kkt_pcg_multi(fm, x, lam, row_state, bound_state, RU, RW, max_iter=None, rtol=1e-12, hess=None):
    """The NumPy twin of asm_kkt_solve_multi: kkt_pcg column by column.  The device advances the columns together, each with its own
    alpha, beta, reference norm, stop code and iteration count, and freezes a column when it stops - which is this loop.  Returns
    (DX, DLAM, DZ, infos), infos a list of kkt_pcg's dicts."""
    RU, RW = _rhs_matrices(fm, RU, RW)
    if hess is not None:
        hess = model_hessian(fm, x, lam, hess)
    cols = [kkt_pcg(fm, x, lam, row_state, bound_state, RU[c], RW[c], max_iter, rtol, hess) for c in range(len(RU))]
    return np.array([c[0] for c in cols]), np.array([c[1] for c in cols]).reshape(len(RU), fm.m), np.array([c[2] for c in cols]), [c[3] for c in cols]


def _jacobian_columns(DX, DLAM, infos):
    status = lambda i: i["status"] if isinstance(i, dict) else i.status
    bad = [(c, status(i)) for c, i in enumerate(infos) if status(i) != 0]
    if bad:
        raise RuntimeError("columns not solved (column, asm_kkt_info status): %r" % bad)
    return DX.T.copy(), DLAM.T.copy()


def solution_jacobian(opt, fm, x, lam, row_state, bound_state, indices=None, max_iter=None, rtol=None):
    """(dx*/dc [n x k], dlam*/dc [m x k]) for the constants `indices` of fm's NLP block (all of them when None;
    expression blocks and the block kernels with derivatives): column q is
    solution_sensitivity along the unit direction of constant indices[q], all from one asm_solution_sensitivity_multi call on `opt`
    (a HipSubOptimizer whose evaluator holds fm, or any object with its solution_sensitivity_multi).  A column whose status is not 0
    raises RuntimeError.  Below about 8 constants a loop of solution_sensitivity calls is faster ("Sensitivity matrices")."""
    nd = len(fm.nlp.device[2])
    idx = np.arange(nd) if indices is None else np.atleast_1d(np.asarray(indices, np.int64))
    if idx.ndim != 1 or np.any(idx < 0) or np.any(idx >= nd):
        raise ValueError("indices must be a list of constants in [0, %d)" % nd)
    if not len(idx):
        return np.zeros((fm.n, 0)), np.zeros((fm.m, 0))
    DC = np.zeros((len(idx), nd))
    DC[np.arange(len(idx)), idx] = 1.0
    DX, DLAM, _, infos = opt.solution_sensitivity_multi(x, lam, row_state, bound_state, DC, max_iter, rtol)
    return _jacobian_columns(DX, DLAM, infos)


def bound_jacobian(opt, fm, x, lam, row_state, bound_state, rows, max_iter=None, rtol=None):
    """(dx*/d(bound) [n x k], dlam*/d(bound) [m x k]) for the working rows `rows` (0-based): column q answers a unit move of the
    active bound of row rows[q] - ru = 0, rw_i = -1 - all from one asm_kkt_solve_multi call on `opt`.  A column whose status is not 0 raises
    RuntimeError."""
    rows = np.atleast_1d(np.asarray(rows, np.int64))
    rs = np.asarray(row_state)
    if rows.ndim != 1 or np.any(rows < 0) or np.any(rows >= fm.m) or np.any(rs[rows] != 1):
        raise ValueError("rows must be rows of the working set (row_state 1)")
    if not len(rows):
        return np.zeros((fm.n, 0)), np.zeros((fm.m, 0))
    RW = np.zeros((len(rows), fm.m))
    RW[np.arange(len(rows)), rows] = -1.0
    DX, DLAM, _, infos = opt.kkt_solve_multi(x, lam, row_state, bound_state, np.zeros((len(rows), fm.n)), RW, max_iter, rtol)
    return _jacobian_columns(DX, DLAM, infos)


def bound_rhs(m, n, rows, delta=None):
    """(RU [k x n], RW [k x m]) of the bound sensitivities of rows `rows` (0-based, duplicates allowed): RU = 0 and RW[c, rows[c]] =
    -delta[c] (delta None: -1), nothing else - what k_kktm_bound_rhs writes on the device for asm_bound_sensitivity_multi, restricted there
    to the working rows (a row outside the working set leaves its column zero)."""
    rows = np.atleast_1d(np.asarray(rows, np.int64))
    if rows.ndim != 1 or np.any(rows < 0) or np.any(rows >= m):
        raise ValueError("rows must be a list of rows in [0, %d)" % m)
    d = np.ones(len(rows)) if delta is None else np.atleast_1d(np.asarray(delta, float))
    if d.shape != rows.shape:
        raise ValueError("delta has shape %r, expected %r" % (d.shape, rows.shape))
    RU, RW = np.zeros((len(rows), n)), np.zeros((len(rows), m))
    RW[np.arange(len(rows)), rows] = -d
    return RU, RW


def _vars_delta(n, vars, delta):
    vars = np.atleast_1d(np.asarray(vars, np.int64))
    if vars.ndim != 1 or np.any(vars < 0) or np.any(vars >= n):
        raise ValueError("vars must be a list of variables in [0, %d)" % n)
    d = np.ones(len(vars)) if delta is None else np.atleast_1d(np.asarray(delta, float))
    if d.shape != vars.shape:
        raise ValueError("delta has shape %r, expected %r" % (d.shape, vars.shape))
    return vars, d


def var_bound_rhs(H, J, n, m, bound_state, vars, delta=None):
    """(RU [k x n], RW [k x m], D [k x n]) of the variable-bound sensitivities of the variables `vars` (0-based, duplicates allowed) for
    the Hessian H [n x n] and Jacobian J [m x n]: D[c] = delta[c] e_j (delta None: 1), RU[c] = delta[c] H[:, j], RW[c] = delta[c] J[:, j] -
    what asm_var_bound_sensitivity_multi makes on the device (RW restricted there to the working rows).  The column's answer is the
    solve of (RU[c], RW[c]) plus D[c] on dx.  A variable outside B (bound_state[j] == 0) leaves all three rows zero."""
    vars, d = _vars_delta(n, vars, delta)
    H, J, bs = np.asarray(H, float), np.asarray(J, float).reshape(m, n), np.asarray(bound_state)
    RU, RW, D = np.zeros((len(vars), n)), np.zeros((len(vars), m)), np.zeros((len(vars), n))
    for c, j in enumerate(vars):
        if bs[j] == 0:
            continue
        RU[c], RW[c], D[c, j] = d[c] * H[:, j], d[c] * J[:, j], d[c]
    return RU, RW, D


def var_bound_reference(fm, x, lam, row_state, bound_state, vars, delta=None):
    """(DX [k x n], DLAM [k x m], DZ [k x n]): the sensitivities to a move of the bounds the variables `vars` sit at, with dx_B = delta
    imposed directly on the dense system - H_FF dx_F - A' dlam = -H_FB delta_B, A dx_F = -J[W, B] delta_B, then
    dz = H[B, :] dx - J[W, B]' dlam - and numpy.linalg.solve: the independent answer (it does not go through the right-hand sides of
    var_bound_rhs).  A variable outside B gives the zero column."""
    vars, d = _vars_delta(fm.n, vars, delta)
    F, W, _, _ = _sets(fm, row_state, bound_state, np.zeros(fm.n), np.zeros(fm.m))
    B = np.nonzero(np.asarray(bound_state) != 0)[0]
    H, J = lagrangian_hessian(fm, x, lam), dense_jacobian(fm, x)
    A = J[np.ix_(W, F)]
    nF, nW, K = len(F), len(W), len(vars)
    M = np.zeros((nF + nW, nF + nW))
    M[:nF, :nF] = H[np.ix_(F, F)]
    M[:nF, nF:] = -A.T
    M[nF:, :nF] = A
    DX, DLAM, DZ = np.zeros((K, fm.n)), np.zeros((K, fm.m)), np.zeros((K, fm.n))
    for c, j in enumerate(vars):
        if bound_state[j] == 0:
            continue
        dB = np.zeros(fm.n)
        dB[j] = d[c]
        sol = np.linalg.solve(M, np.concatenate([-(H[np.ix_(F, B)] @ dB[B]), -(J[np.ix_(W, B)] @ dB[B])])) if nF + nW else np.zeros(0)
        dx = dB.copy()
        dx[F] = sol[:nF]
        DX[c], DLAM[c, W] = dx, sol[nF:]
        DZ[c, B] = H[B] @ dx - J[np.ix_(W, B)].T @ sol[nF:]
    return DX, DLAM, DZ


def var_bound_jacobian(opt, fm, x, lam, row_state, bound_state, vars, max_iter=None, rtol=None):
    """(dx*/d(xbound) [n x k], dlam*/d(xbound) [m x k], dz*/d(xbound) [n x k]) for the variables `vars` (0-based) at a bound: column q
    answers a unit move of the bound variable vars[q] sits at, all from one asm_var_bound_sensitivity_multi call on `opt`.  A column
    whose status is not 0 raises RuntimeError."""
    vars = np.atleast_1d(np.asarray(vars, np.int64))
    bs = np.asarray(bound_state)
    if vars.ndim != 1 or np.any(vars < 0) or np.any(vars >= fm.n) or np.any(bs[vars] == 0):
        raise ValueError("vars must be variables at a bound (bound_state -1 or +1)")
    if not len(vars):
        return np.zeros((fm.n, 0)), np.zeros((fm.m, 0)), np.zeros((fm.n, 0))
    DX, DLAM, DZ, infos = opt.var_bound_sensitivity_multi(x, lam, row_state, bound_state, vars, None, max_iter, rtol)
    dx, dlam = _jacobian_columns(DX, DLAM, infos)
    return dx, dlam, DZ.T.copy()


def solution_sensitivity(model_or_opt, fm, x, lam, row_state, bound_state, dc, max_iter=None, rtol=None):
    """(dx, dlam, dz, info) of asm_solution_sensitivity for the FunctionModel `fm` (expression blocks and the block kernels with derivatives, with
    its data) at the solution
    (x, lam) with the working set given, along the direction dc of the block's data.  `model_or_opt`: a HipSubOptimizer whose
    evaluator holds fm (eval_setup(fm)), or a Model built from fm - then a fresh handle is made for the call and closed again."""
    from .subproblem import HipSubOptimizer, QpData
    if isinstance(model_or_opt, HipSubOptimizer):
        return model_or_opt.solution_sensitivity(x, lam, row_state, bound_state, dc, max_iter, rtol)
    mdl = model_or_opt
    opt = HipSubOptimizer(QpData(np.zeros(mdl.n), 0.0, np.zeros(len(mdl.j_row)), np.zeros(mdl.m), mdl.g_L, mdl.g_U, mdl.x_L, mdl.x_U), mdl.j_row, mdl.j_col)
    try:
        opt.eval_setup(fm)
        return opt.solution_sensitivity(x, lam, row_state, bound_state, dc, max_iter, rtol)
    finally:
        opt.close()


def model_cross_t(fm, x, lam, vx, vl):
    """out [n_dpar] of the host twin of asm_eval_data_cross_t for the FunctionModel `fm`: the block's data_cross_t with the block's part
    of lam and vl (its rows follow the function store's) and the model's sense scale; empty without an NLP block."""
    if fm.nlp is None:
        return np.zeros(0)
    if getattr(fm.nlp, "data_cross_t", None) is None:
        raise ValueError("the model's NLP block has no data derivatives")
    off = fm.nlp_constraint_offset
    return np.asarray(fm.nlp.data_cross_t(np.asarray(x, float), np.asarray(lam, float)[off:], np.asarray(vx, float), np.asarray(vl, float)[off:],
                                          fm.objective_scale), float)


def adjoint_reference(fm, x, lam, row_state, bound_state, gx, gl):
    """(out [n_dpar], dbound [m], ax [n], al [m]) for a function with gradients gx, gl at the solution (x, lam) with its working set:
    the adjoint state from the dense kkt_reference(ru = -gx, rw = gl), out = model_cross_t(vx = -ax, vl = al), dbound = -al on the
    working rows and 0 elsewhere."""
    gx, gl = np.asarray(gx, float), np.asarray(gl, float)
    ax, al, _ = kkt_reference(fm, x, lam, row_state, bound_state, -gx, gl)
    dbound = np.where(np.asarray(row_state) == 1, -al, 0.0)
    return model_cross_t(fm, x, lam, -ax, al), dbound, ax, al


def adjoint_reference_z(fm, x, lam, row_state, bound_state, gx, gl, gz):
    """(out [n_dpar], dbound [m], dxbound [n], ax [n], al [m]) for a function phi(x*, lam*, z*) with gradients gx, gl, gz (gz counts on B
    only): with gx~ = gx + H gz and gl~ = gl - J gz the adjoint state (ax, al, dz) = kkt_reference(ru = -gx~, rw = gl~),
    out = model_cross_t(vx = gz - ax, vl = al), dbound = -al on the working rows, dxbound = -dz on B; 0 elsewhere."""
    gx, gl = np.asarray(gx, float), np.asarray(gl, float)
    on_b = np.asarray(bound_state) != 0
    gzb = np.where(on_b, np.asarray(gz, float), 0.0)
    H, J = lagrangian_hessian(fm, x, lam), dense_jacobian(fm, x)
    ax, al, dz = kkt_reference(fm, x, lam, row_state, bound_state, -(gx + H @ gzb), gl - J @ gzb)
    dbound = np.where(np.asarray(row_state) == 1, -al, 0.0)
    return model_cross_t(fm, x, lam, gzb - ax, al), dbound, np.where(on_b, -dz, 0.0), ax, al


def solution_adjoint(model_or_opt, fm, x, lam, row_state, bound_state, gx, gl, max_iter=None, rtol=None):
    """(out, dbound, ax, al, info) of asm_solution_adjoint for the FunctionModel `fm` at the solution (x, lam) with the working set
    given: the gradient of a function phi(x*, lam*) with gradients (gx, gl) with respect to every constant of the block's data and
    every row bound, from one KKT solve.  `model_or_opt` as for solution_sensitivity."""
    from .subproblem import HipSubOptimizer, QpData
    if isinstance(model_or_opt, HipSubOptimizer):
        return model_or_opt.solution_adjoint(x, lam, row_state, bound_state, gx, gl, max_iter, rtol)
    mdl = model_or_opt
    opt = HipSubOptimizer(QpData(np.zeros(mdl.n), 0.0, np.zeros(len(mdl.j_row)), np.zeros(mdl.m), mdl.g_L, mdl.g_U, mdl.x_L, mdl.x_U), mdl.j_row, mdl.j_col)
    try:
        opt.eval_setup(fm)
        return opt.solution_adjoint(x, lam, row_state, bound_state, gx, gl, max_iter, rtol)
    finally:
        opt.close()


RANGE_KINDS = ("none", "row reaches g_L", "row reaches g_U", "variable reaches x_L", "variable reaches x_U", "row multiplier reaches 0",
               "bound multiplier reaches 0")        # asm_range_info.kind_*: ASM_RANGE_* 0..6
RANGE_DTYPE = np.dtype([("t_lo", np.float64), ("t_hi", np.float64), ("pos_lo", np.int32), ("kind_lo", np.int32), ("pos_hi", np.int32),
                        ("kind_hi", np.int32)], align=True)


def _range_model(p, x):
    """(g_L, g_U, x_L, x_U, E, J) of a Problem or a FunctionModel at x: the bounds, g(x) and the dense Jacobian (duplicates add)."""
    x = np.asarray(x, float)
    if hasattr(p, "constraint_bounds"):
        g_L, g_U = p.constraint_bounds()
        J = dense_jacobian(p, x)
    else:
        g_L, g_U = np.asarray(p.g_L, float), np.asarray(p.g_U, float)
        J = np.zeros((p.m, p.n))
        if len(p.j_row):
            np.add.at(J, (np.asarray(p.j_row, np.int64) - 1, np.asarray(p.j_col, np.int64) - 1), p.eval_jac_g(x, np.zeros(len(p.j_row))))
    m = int(p.m)
    E = np.asarray(p.eval_g(x, np.zeros(m)), float) if m else np.zeros(0)
    return np.asarray(g_L, float).reshape(m), np.asarray(g_U, float).reshape(m), np.asarray(p.x_L, float), np.asarray(p.x_U, float), E, J


def validity_range_host(problem_or_fm, x, lam, mult_x_U, mult_x_L, row_state, bound_state, DX, DLAM, DZ, dtype=np.float64, runner_up=False):
    """The NumPy twin of asm_sensitivity_range_multi and the specification of the rule (include/asm_hip.h, "Validity ranges"): for every
    column c - row c of DX [k x n], DLAM [k x m], DZ [k x n] - the range [t_lo, t_hi] of t on which x + t dx, lam + t dlam, z + t dz
    (z = mult_x_U + mult_x_L) keep the working set (row_state, bound_state) of `problem_or_fm` (a Problem or a FunctionModel) to first
    order, and what blocks at either end.  With sg = +1 for the upper and -1 for the lower range, V = J dx from dense_jacobian, and the
    candidates in position order (rows 0 .. m - 1, then variable j at m + j):
        row i outside W     sg V_i < 0 and g_L_i > -inf: (g_L_i - E_i) / (sg V_i), kind 1; else sg V_i > 0 and g_U_i < inf: kind 2
        row i in W, g_L_i != g_U_i   at its upper bound (!(g_L_i > -inf) or g_U_i < inf and |E_i - g_U_i| < |E_i - g_L_i|) with
                            sg dlam_i > 0, at its lower bound with sg dlam_i < 0: -lam_i / (sg dlam_i), kind 5
        variable j in F     sg dx_j < 0 and x_L_j > -inf: (x_L_j - x_j) / (sg dx_j), kind 3; else sg dx_j > 0 and x_U_j < inf: kind 4
        variable j in B     at +1 with sg dz_j > 0, at -1 with sg dz_j < 0: -z_j / (sg dz_j), kind 6
    every ratio clamped from below at 0, one that is not below +inf no candidate; the smallest ratio wins, on equal ratios the smallest
    position; +inf, position -1 and kind 0 without a candidate; t_hi = best, t_lo = 0 - best.  Returns a structured array [k] with the
    fields of asm_range_info (RANGE_DTYPE; t in float64 whatever `dtype`, the type of the arithmetic).  runner_up: also (k x 2) the
    smallest ratio at another position than the winner's, columns (lower, upper), +inf without one."""
    T = np.dtype(dtype).type
    g_L, g_U, x_L, x_U, E, J = (np.asarray(a, T) for a in _range_model(problem_or_fm, x))
    m, n = J.shape
    x, lam = np.asarray(x, T).reshape(n), np.asarray(lam, T).reshape(m)
    z = np.asarray(mult_x_U, T).reshape(n) + np.asarray(mult_x_L, T).reshape(n)
    rs, bs = np.asarray(row_state).reshape(m), np.asarray(bound_state).reshape(n)
    DX, DZ = np.atleast_2d(np.asarray(DX, T)), np.atleast_2d(np.asarray(DZ, T))
    k = DX.shape[0]
    DLAM = np.asarray(DLAM, T).reshape(k, m)
    if DX.shape != (k, n) or DZ.shape != (k, n) or k < 1:
        raise ValueError("DX, DLAM, DZ must have shapes (k, n), (k, m), (k, n) with k >= 1")
    if np.any((rs != 0) & (rs != 1)) or np.any(np.abs(bs) > 1):
        raise ValueError("row_state must hold 0 / 1 and bound_state -1 / 0 / +1")
    V = DX @ J.T                                               # k x m
    inf = T(np.inf)
    upper = ~(g_L > -inf) | ((g_U < inf) & (np.abs(E - g_U) < np.abs(E - g_L)))
    out = np.zeros(k, RANGE_DTYPE)
    second = np.full((k, 2), np.inf)
    pos = np.arange(m + n)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for side, sg in enumerate((T(-1.0), T(1.0))):
            v, dl, vx, dv = sg * V, sg * DLAM, sg * DX, sg * DZ
            ratio = np.full((k, m + n), inf, T)
            kind = np.zeros((k, m + n), np.int32)

            def offer(cond, num, den, kd, at):
                r = np.where(cond, num / np.where(cond, den, T(1.0)), inf)
                sl = (slice(None), at)
                ratio[sl] = np.where(cond, r, ratio[sl])
                kind[sl] = np.where(cond, kd, kind[sl])

            rows, vars_ = slice(0, m), slice(m, m + n)
            out_w, in_w = (rs == 0)[None, :], ((rs == 1) & (g_L != g_U))[None, :]
            lo1 = out_w & (v < 0) & (g_L > -inf)[None, :]
            offer(lo1, (g_L - E)[None, :], v, 1, rows)
            offer(out_w & ~lo1 & (v > 0) & (g_U < inf)[None, :], (g_U - E)[None, :], v, 2, rows)
            offer(in_w & np.where(upper[None, :], dl > 0, dl < 0), -lam[None, :], dl, 5, rows)
            free, atb = (bs == 0)[None, :], (bs != 0)[None, :]
            lo3 = free & (vx < 0) & (x_L > -inf)[None, :]
            offer(lo3, (x_L - x)[None, :], vx, 3, vars_)
            offer(free & ~lo3 & (vx > 0) & (x_U < inf)[None, :], (x_U - x)[None, :], vx, 4, vars_)
            offer(atb & np.where((bs > 0)[None, :], dv > 0, dv < 0), -z[None, :], dv, 6, vars_)
            ratio = np.where(ratio < 0, T(0.0), ratio)
            ok = ratio < inf
            ratio = np.where(ok, ratio, inf)
            kind = np.where(ok, kind, 0)
            best = np.argmin(ratio, axis=1)                    # (the first of equal minima: the smallest position)
            for c in range(k):
                b = ratio[c, best[c]]
                if b < inf:
                    p_, kd = int(pos[best[c]]), int(kind[c, best[c]])
                    others = np.delete(ratio[c], best[c])
                    second[c, side] = float(others.min()) if len(others) else np.inf
                else:
                    p_, kd = -1, 0
                t = float(T(0.0) - b) if side == 0 else float(b)
                out[c][("t_lo", "t_hi")[side]] = t
                out[c][("pos_lo", "pos_hi")[side]] = p_
                out[c][("kind_lo", "kind_hi")[side]] = kd
    return (out, second) if runner_up else out


def validity_range(opt, x, lam, mult_x_U, mult_x_L, row_state, bound_state, DX, DLAM, DZ):
    """The validity ranges of the sensitivity columns DX, DLAM, DZ on the device: asm_sensitivity_range_multi on `opt`, a HipSubOptimizer
    whose evaluator holds the model and whose bounds are the problem's (or any object with its sensitivity_range).  A structured array
    with the fields of asm_range_info; validity_range_host is the NumPy twin."""
    return opt.sensitivity_range(x, lam, mult_x_U, mult_x_L, row_state, bound_state, DX, DLAM, DZ)


def predict(x, dx, step):
    """The first-order prediction of the solution after the data moved by step * dc: x + step * dx."""
    return np.asarray(x, float) + float(step) * np.asarray(dx, float)
