"""The trust-region step on a working set (include/asm_hip.h, "Trust-region step on the working set"): Byrd-Omojokun with
Steihaug-Toint truncation - the equality-constrained QP of sensitivity.py with an l2 radius.

    minimise  ru' dx + 1/2 dx' H dx   over   A dx_F = -theta rw_W ,  dx_B = 0 ,  ||dx||_2 <= radius

    kkt_step_pcg             the NumPy twin of the device algorithm (asm_kkt_step), line for line the method of the header
    kkt_step_reference       an independent dense answer: lstsq normal step, SVD null-space basis, textbook Steihaug CG in reduced
                             coordinates, lstsq multipliers; returns its per-iteration trace
    kkt_step_pcg_multi       kkt_step_pcg column by column: what the lockstep iteration of asm_kkt_step_multi computes
    kkt_step_reference_multi kkt_step_reference column by column
    fraction_to_box          the largest t in [0, 1] with lo <= t dx <= hi
    eqp_step                 one step from a point: working set, right-hand sides, kkt_step, fraction to the variable bounds
    lp_working_set           the working set an LP's active set names at a point (include/asm_hip.h, "SLP-EQP")
    eqp_trial_host           the NumPy twin of asm_eqp_trial: lp_working_set, kkt_step_pcg, fraction_to_box, the two merit values

The driver that uses the step is slp.SlpEQP (Parameters(algorithm="SLP-EQP")); its native form is asm_slp_run_eqp.
"""
from types import SimpleNamespace

import numpy as np

from .sensitivity import _finish, _guarded_cholesky, _rhs_matrices, _sets, _substitute, dense_jacobian, model_hessian, working_set

INF = float("inf")


def _check_radius(radius, normal_share):
    radius, normal_share = float(radius), float(normal_share)
    if not radius > 0.0:
        raise ValueError("the radius must be > 0")
    if not 0.0 < normal_share <= 1.0:
        raise ValueError("normal_share must be in (0, 1]")
    return radius, normal_share


def kkt_step_pcg(fm, x, lam, row_state, bound_state, ru, rw, radius, max_iter=None, rtol=1e-12, normal_share=0.8, hess=None):
    """The NumPy twin of asm_kkt_step: sensitivity.kkt_pcg with the radius.  Steps 1 and 2 unchanged; step 3 scales the normal step to
    normal_share * radius where it is longer; step 4 applies the Steihaug-Toint rule from d'd, d'p and p'p summed directly; steps 5
    and 6 add the model value and the norms.  The boundary move counts as a completed iteration (cg_iters).  radius = inf is kkt_pcg,
    bit for bit.  hess: what stands for the Hessian (sensitivity.model_hessian; None: the model's own).  Returns (dx, dlam, dz, info),
    info a dict with the fields of asm_kkt_step_info."""
    F, W, ru, rw = _sets(fm, row_state, bound_state, ru, rw)
    radius, normal_share = _check_radius(radius, normal_share)
    H, J = model_hessian(fm, x, lam, hess), dense_jacobian(fm, x)
    HF, A = H[np.ix_(F, F)], J[np.ix_(W, F)]
    nF, nW = len(F), len(W)
    if max_iter is None:
        max_iter = 2 * (nF - nW) + 20
    L, dropped = _guarded_cholesky(A @ A.T) if nW else (np.zeros((0, 0)), 0)
    s_solve = lambda b: _substitute(L, b)
    proj = lambda v: v - A.T @ s_solve(A @ v) if nW else v.copy()
    # 3. the normal step and the share of it that the radius admits
    dx0 = -(A.T @ s_solve(rw[W])) if nW else np.zeros(nF)
    if nW:
        dx0 = dx0 - A.T @ s_solve(A @ dx0 + rw[W])         # one refinement step of the normal-equation solve
    nn = float(np.sqrt(dx0 @ dx0))
    cap = normal_share * radius
    theta = cap / nn if nn > cap else 1.0
    if theta != 1.0:
        dx0 = theta * dx0
    tn = theta * nn
    dt2 = max(radius * radius - tn * tn, 0.0)              # dx0 in range(A'), d in null(A): ||dx||^2 = ||dx0||^2 + ||d||^2
    # 4. projected conjugate gradients with the Steihaug-Toint truncation
    d = np.zeros(nF)
    status, iters, boundary = 0, 0, 0
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
            php, dd, dp, pp = float(p @ hp), float(d @ d), float(d @ p), float(p @ p)
            gap = dt2 - dd
            tau = gap / (dp + np.sqrt(dp * dp + pp * gap)) if 0.0 < gap < INF else 0.0
            if not php > 0.0:
                if dt2 < INF:
                    alpha, boundary = tau, 2               # along the direction of non-positive curvature to the boundary
                else:
                    status = 2
                    break
            else:
                alpha = rg / php
                if dd + 2.0 * alpha * dp + alpha * alpha * pp >= dt2:
                    alpha, boundary = tau, 1               # the step leaves the region: to the boundary
            d = d + alpha * p
            r = r + alpha * hp
            r = proj(proj(r))
            g = r
            rg_new = float(r @ g)
            beta = rg_new / rg
            rg = rg_new
            iters += 1
            stop = float(np.sqrt(g @ g)) <= rtol * g0 or boundary != 0
            p = -g + beta * p
    # 5., 6. the step, its multipliers, the residuals against theta rw, the model value
    dxF = dx0 + d
    q = HF @ dxF + ru[F]
    dlW = s_solve(A @ q) if nW else np.zeros(0)
    if nW:
        dlW = dlW + s_solve(A @ (q - A.T @ dlW))           # one refinement step
    if dropped:
        status = 3
    dx, dlam, dz = _finish(H, J, F, W, ru, dxF, dlW, fm.n, fm.m)
    info = dict(status=status, cg_iters=iters, n_free=nF, n_rows=nW, dropped_pivots=dropped, boundary=boundary,
                res_stat=float(np.abs(HF @ dxF - A.T @ dlW + ru[F]).max()) if nF else 0.0,
                res_feas=float(np.abs(A @ dxF + theta * rw[W]).max()) if nW else 0.0,
                theta=theta, norm_normal=tn, norm_step=float(np.sqrt(dx @ dx)), model=float(ru @ dx + 0.5 * (dx @ (H @ dx))))
    return dx, dlam, dz, info


def kkt_step_reference(fm, x, lam, row_state, bound_state, ru, rw, radius, max_iter=None, rtol=1e-12, normal_share=0.8, hess=None):
    """An independent dense answer to the trust-region step: the minimum-norm normal step by numpy.linalg.lstsq, an orthonormal basis Z
    of null(A) from the SVD of A, textbook Steihaug conjugate gradients on Z' H_FF Z in reduced coordinates (every pass of the loop that
    moves the iterate counts as an iteration, the boundary move too), multipliers by lstsq.  Returns (dx, dlam, dz, info, trace): info a
    dict with the fields of asm_kkt_step_info except dropped_pivots and the residuals' device forms; trace a dict with nn, cap =
    normal_share * radius, dt (the tangential radius), hnorm = ||Z' H Z||_2, g0 and `iterations`, a list of dicts with php, pp, trial
    (||u + alpha p||_2, None where p'Hp <= 0), gnorm (the residual norm after the move, None on the boundary).  hess as in kkt_step_pcg."""
    rs, bs = np.asarray(row_state), np.asarray(bound_state)
    ru, rw, n, m = np.asarray(ru, float), np.asarray(rw, float), fm.n, fm.m
    radius, normal_share = _check_radius(radius, normal_share)
    free, work = np.flatnonzero(bs == 0), np.flatnonzero(rs == 1)
    if len(work) > len(free):
        raise ValueError("more working rows than free variables")
    H, J = model_hessian(fm, x, lam, hess), dense_jacobian(fm, x)
    Hff, A = H[free][:, free], J[work][:, free]
    k, nf = len(work), len(free)
    normal = np.linalg.lstsq(A, -rw[work], rcond=None)[0] if k else np.zeros(nf)
    nn = float(np.linalg.norm(normal))
    cap = normal_share * radius
    theta = cap / nn if nn > cap else 1.0
    normal = theta * normal
    dt = float(np.sqrt(max(radius ** 2 - float(np.linalg.norm(normal)) ** 2, 0.0)))
    if k:
        _, sv, Vt = np.linalg.svd(A, full_matrices=True)
        rank = int(np.sum(sv > sv[0] * max(A.shape) * np.finfo(float).eps))
        Z = Vt[rank:].T
    else:
        Z = np.eye(nf)
    Hr, c = Z.T @ Hff @ Z, Z.T @ (ru[free] + Hff @ normal)
    nz = Z.shape[1]
    limit = 2 * (nf - k) + 20 if max_iter is None else max_iter
    u, res = np.zeros(nz), c.copy()
    g0 = float(np.linalg.norm(res))
    trace = dict(nn=nn, cap=cap, dt=dt, hnorm=float(np.linalg.norm(Hr, 2)) if nz else 0.0, g0=g0, iterations=[])
    status, iters, boundary = 0, 0, 0
    p = -res
    done = nz == 0 or g0 == 0.0

    def to_boundary(u, p):
        """the positive root of ||u + t p|| = dt"""
        a, b, cc = float(p @ p), float(u @ p), float(u @ u) - dt * dt
        return (-b + np.sqrt(b * b - a * cc)) / a

    while not done:
        if iters >= limit:
            status = 1
            break
        Hp = Hr @ p
        kappa = float(p @ Hp)
        rec = dict(php=kappa, pp=float(p @ p), trial=None, gnorm=None)
        trace["iterations"].append(rec)
        if kappa <= 0.0:
            if not np.isfinite(dt):
                status = 2
                break
            u = u + to_boundary(u, p) * p
            iters, boundary = iters + 1, 2
            break
        alpha = float(res @ res) / kappa
        rec["trial"] = float(np.linalg.norm(u + alpha * p))
        if rec["trial"] >= dt:
            u = u + to_boundary(u, p) * p
            iters, boundary = iters + 1, 1
            break
        u = u + alpha * p
        new = res + alpha * Hp
        iters += 1
        rec["gnorm"] = float(np.linalg.norm(new))
        if rec["gnorm"] <= rtol * g0:
            break
        p = -new + (float(new @ new) / float(res @ res)) * p
        res = new
    step = normal + Z @ u
    mult = np.linalg.lstsq(A.T, Hff @ step + ru[free], rcond=None)[0] if k else np.zeros(0)
    dx, dlam = np.zeros(n), np.zeros(m)
    dx[free], dlam[work] = step, mult
    grad = H @ dx + ru - J[work].T @ mult
    dz = np.where(bs == 0, 0.0, grad)
    info = dict(status=status, cg_iters=iters, n_free=nf, n_rows=k, boundary=boundary, theta=theta,
                res_stat=float(np.abs(grad[free]).max()) if nf else 0.0, res_feas=float(np.abs(A @ step + theta * rw[work]).max()) if k else 0.0,
                norm_normal=float(np.linalg.norm(normal)), norm_step=float(np.linalg.norm(dx)), model=float(ru @ dx + 0.5 * dx @ H @ dx))
    return dx, dlam, dz, info, trace


def _columns(one, fm, x, lam, row_state, bound_state, RU, RW, radii, **kw):
    RU, RW = _rhs_matrices(fm, RU, RW)
    if kw.get("hess") is not None:
        kw["hess"] = model_hessian(fm, x, lam, kw["hess"])
    radii = np.asarray(radii, float)
    if radii.shape != (len(RU),):
        raise ValueError("radii must have shape (nrhs,)")
    cols = [one(fm, x, lam, row_state, bound_state, RU[c], RW[c], radii[c], **kw) for c in range(len(RU))]
    out = (np.array([c[0] for c in cols]), np.array([c[1] for c in cols]).reshape(len(RU), fm.m), np.array([c[2] for c in cols]), [c[3] for c in cols])
    return out + tuple([c[k] for c in cols] for k in range(4, len(cols[0])))


def kkt_step_pcg_multi(fm, x, lam, row_state, bound_state, RU, RW, radii, max_iter=None, rtol=1e-12, normal_share=0.8, hess=None):
    """The NumPy twin of asm_kkt_step_multi: kkt_step_pcg column by column, each with its radius.  The device advances the columns
    together and freezes a column when it stops - on the boundary too - which is this loop.  Returns (DX, DLAM, DZ, infos)."""
    return _columns(kkt_step_pcg, fm, x, lam, row_state, bound_state, RU, RW, radii, max_iter=max_iter, rtol=rtol, normal_share=normal_share, hess=hess)


def kkt_step_reference_multi(fm, x, lam, row_state, bound_state, RU, RW, radii, max_iter=None, rtol=1e-12, normal_share=0.8, hess=None):
    """kkt_step_reference column by column.  Returns (DX, DLAM, DZ, infos, traces)."""
    return _columns(kkt_step_reference, fm, x, lam, row_state, bound_state, RU, RW, radii, max_iter=max_iter, rtol=rtol, normal_share=normal_share, hess=hess)


def fraction_to_box(dx, lo, hi):
    """The largest t in [0, 1] with lo <= t * dx <= hi, component by component (lo <= 0 <= hi is the caller's: lo = x_L - x,
    hi = x_U - x at a point inside its bounds).  A zero component never binds, an infinite bound never binds, and a bound already
    active with the step pointing outwards gives 0."""
    dx, lo, hi = np.asarray(dx, float), np.asarray(lo, float), np.asarray(hi, float)
    if dx.shape != lo.shape or dx.shape != hi.shape:
        raise ValueError("dx, lo, hi must have one shape")
    t = 1.0
    up, down = dx > 0.0, dx < 0.0
    if up.any():
        t = min(t, float((hi[up] / dx[up]).min()))
    if down.any():
        t = min(t, float((lo[down] / dx[down]).min()))
    return max(t, 0.0)


def eqp_step(opt, fm, problem, x, lam, mult_x_U, mult_x_L, radius, tol=1e-8):
    """One trust-region step of the equality-constrained QP at (x, lam): the working set of sensitivity.working_set (activity within
    tol), ru = grad f(x) - with H the Hessian of f - lam' g, the sign convention of asm_eval_hessian_lagrangian(x, 1, -lam), dlam is
    then the new multiplier vector itself - rw = g_W(x) - bound_W (the bound the row sits at), opt.kkt_step (a HipSubOptimizer whose
    evaluator holds fm, or any object with its kkt_step), and the fraction of the step that keeps x_L <= x <= x_U.  Returns
    (x + t dx, the new multipliers, info)."""
    x, lam = np.asarray(x, float), np.asarray(lam, float)
    row_state, bound_state = working_set(problem, x, lam, mult_x_U, mult_x_L, tol)
    ru = np.asarray(fm.eval_grad_f(x, np.zeros(fm.n)), float)
    m = int(problem.m)
    rw = np.zeros(m)
    if m:
        g = np.asarray(problem.eval_g(x, np.zeros(m)), float)
        g_L, g_U = np.asarray(problem.g_L, float), np.asarray(problem.g_U, float)
        with np.errstate(invalid="ignore"):
            lower = np.isfinite(g_L) & ~(np.abs(g - g_U) < np.abs(g - g_L))
        rw = np.where(row_state == 1, g - np.where(lower, g_L, g_U), 0.0)
    dx, lam_new, _, info = opt.kkt_step(x, lam, row_state, bound_state, ru, rw, radius)[:4]
    t = fraction_to_box(dx, np.asarray(problem.x_L, float) - x, np.asarray(problem.x_U, float) - x)
    return x + t * dx, np.asarray(lam_new, float), info


def lp_working_set(problem, x, S, tol=1e-8):
    """The working set the active set S = (row_state [m + n_adj], bound_state [n], ...) of an LP solved at x names (the tuple
    HipSubOptimizer.active_set() returns).  adj, the rows with two distinct finite bounds in index order, have their `<=` twins in rows
    m.. of the LP's row_state.  A row is in W if it is an equality, if the LP holds it active or if its twin is active; it sits at g_L
    (an equality), at g_U (twin active, or g_L infinite), else at g_L.  A variable is in B only where the LP reports it at a bound and
    x is at the matching bound of the problem within tol * (1 + |bound|): a variable the trust region stopped is free.
    Returns (row_state [m] of 0 / 1, bound_state [n] of -1 / 0 / +1, bound [m]: the bound a working row sits at, 0 elsewhere)."""
    x = np.asarray(x, float)
    n, m = int(problem.n), int(problem.m)
    g_L, g_U = np.asarray(problem.g_L, float).reshape(m), np.asarray(problem.g_U, float).reshape(m)
    x_L, x_U = np.asarray(problem.x_L, float), np.asarray(problem.x_U, float)
    adj = np.flatnonzero(np.isfinite(g_L) & np.isfinite(g_U) & (g_L != g_U))
    lp_rows, lp_bnd = np.asarray(S[0]), np.asarray(S[1])
    if lp_rows.shape != (m + len(adj),) or lp_bnd.shape != (n,) or x.shape != (n,):
        raise ValueError("x / the LP's row_state / bound_state have shapes %r / %r / %r, expected (%d,) / (%d,) / (%d,)"
                         % (x.shape, lp_rows.shape, lp_bnd.shape, n, m + len(adj), n))
    twin = np.zeros(m, bool)
    twin[adj] = lp_rows[m:] != 0
    row_state = ((g_L == g_U) | (lp_rows[:m] != 0) | twin).astype(np.int32)
    at = np.where(g_L == g_U, g_L, np.where(twin | ~np.isfinite(g_L), g_U, g_L))
    with np.errstate(invalid="ignore"):
        lower = (lp_bnd == -1) & np.isfinite(x_L) & (np.abs(x - x_L) <= tol * (1.0 + np.abs(x_L)))
        upper = (lp_bnd == 1) & np.isfinite(x_U) & (np.abs(x - x_U) <= tol * (1.0 + np.abs(x_U)))
    bound_state = np.where(lower, -1, np.where(upper, 1, 0)).astype(np.int32)
    return row_state, bound_state, np.where(row_state == 1, at, 0.0)


def _merit(problem, x, nu):
    """compute_phi of the SLP drivers outside restoration: f(x) + nu' viol(g(x))."""
    m = int(problem.m)
    E = np.asarray(problem.eval_g(x, np.zeros(m)), float) if m else np.zeros(0)
    viol = np.maximum(0.0, np.maximum(E - np.asarray(problem.g_U, float), np.asarray(problem.g_L, float) - E))
    return float(problem.eval_f(x) + np.asarray(nu, float) @ viol)


def eqp_trial_host(fm, problem, x, lam, lp_row_state, lp_bound_state, radius, nu, tol_active=1e-8, max_iter=None, rtol=1e-12, normal_share=0.8,
                   kkt_step=None, hess=None):
    """The NumPy twin of asm_eqp_trial: the working set of lp_working_set, ru = grad f(x), rw_W = g_W(x) - bound_W, the trust-region step
    (kkt_step_pcg, or kkt_step(x, lam, row_state, bound_state, ru, rw, radius) -> (dx, dlam, dz, info)), d = t dx with t the fraction of
    fraction_to_box, and the merit values f + nu' viol at x and x + d.  Returns (d, lam_new, mult_x_U, mult_x_L, row_state, bound_state,
    info), info with the fields of asm_eqp_info: those of asm_kkt_step_info, t, norm_d, norm_d_inf, phi0, phi1 and skipped (0 none, 1 more
    working rows than free variables, 2 dependent working rows, 3 zero step).  A skipped trial returns zeros for d and the multipliers.
    hess goes to kkt_step_pcg (a callable is read when the step is taken: the twin of a store that changes between trials)."""
    if not float(tol_active) >= 0.0:
        raise ValueError("tol_active must be >= 0")
    x, lam = np.asarray(x, float), np.asarray(lam, float)
    n, m = int(problem.n), int(problem.m)
    row_state, bound_state, at = lp_working_set(problem, x, (lp_row_state, lp_bound_state), tol_active)
    info = dict(status=0, cg_iters=0, n_free=int((bound_state == 0).sum()), n_rows=int(row_state.sum()), dropped_pivots=0, boundary=0, res_stat=0.0,
                res_feas=0.0, theta=0.0, norm_normal=0.0, norm_step=0.0, model=0.0, t=0.0, norm_d=0.0, norm_d_inf=0.0, phi0=0.0, phi1=0.0, skipped=0)
    zero = (np.zeros(n), np.zeros(m), np.zeros(n), np.zeros(n), row_state, bound_state)
    if info["n_rows"] > info["n_free"]:
        info["skipped"] = 1
        return zero + (SimpleNamespace(**info),)
    ru = np.asarray(fm.eval_grad_f(x, np.zeros(n)), float)
    E = np.asarray(problem.eval_g(x, np.zeros(m)), float) if m else np.zeros(0)
    rw = np.where(row_state == 1, E - at, 0.0)
    if kkt_step is None:
        dx, dlam, dz, step = kkt_step_pcg(fm, x, lam, row_state, bound_state, ru, rw, radius, max_iter=max_iter, rtol=rtol, normal_share=normal_share, hess=hess)
    else:
        dx, dlam, dz, step = kkt_step(x, lam, row_state, bound_state, ru, rw, radius)[:4]
    if not isinstance(step, dict):
        step = {k: getattr(step, k) for k, _ in step._fields_}
    info.update(step)
    if info["status"] == 3:
        info["skipped"] = 2
        return zero + (SimpleNamespace(**info),)
    t = fraction_to_box(dx, np.asarray(problem.x_L, float) - x, np.asarray(problem.x_U, float) - x)
    d = t * dx
    info.update(t=t, norm_d=float(np.sqrt(d @ d)), norm_d_inf=float(np.abs(d).max()) if n else 0.0)
    if not d.any():
        info["skipped"] = 3
        return zero + (SimpleNamespace(**info),)
    info.update(phi0=_merit(problem, x, nu), phi1=_merit(problem, x + d, nu))
    dz = np.asarray(dz, float)
    return (d, np.asarray(dlam, float), np.where(bound_state == 1, dz, 0.0), np.where(bound_state == -1, dz, 0.0), row_state, bound_state,
            SimpleNamespace(**info))
