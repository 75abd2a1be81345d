"""Shared generators for the parity tests (seeded, deterministic)."""
import numpy as np

INF = np.inf


def random_subproblem(seed, n, m, density=1.0, dup_frac=0.0, n_range=0, infeasible=False, delta=0.4):
    """A random instance of the data `sub_optimize!` sees (subproblem.jl:229-246): COO Jacobian with
    optional duplicate entries, mixed EQ / >= / <= / range rows, finite variable bounds, a point x_k."""
    rng = np.random.default_rng(seed)
    mask = rng.random((m, n)) < density
    mask[np.arange(m), rng.integers(0, n, m)] = True
    rows, cols = np.nonzero(mask)
    vals = rng.standard_normal(len(rows)) / np.sqrt(max(1.0, density * n))
    ndup = int(dup_frac * len(rows))
    if ndup:
        pick = rng.integers(0, len(rows), ndup)
        rows = np.concatenate([rows, rows[pick]]); cols = np.concatenate([cols, cols[pick]])
        vals = np.concatenate([vals, 0.25 * rng.standard_normal(ndup)])
        perm = rng.permutation(len(rows))
        rows, cols, vals = rows[perm], cols[perm], vals[perm]
    J = np.zeros((m, n))
    np.add.at(J, (rows, cols), vals)
    x_k = rng.uniform(-0.5, 0.5, n)
    v_lb = -np.ones(n); v_ub = np.ones(n)
    p_star = rng.uniform(-0.3, 0.3, n) * min(1.0, delta / 0.4)
    E = rng.standard_normal(m) * 0.1                       # current constraint values b
    act = E + J @ p_star                                    # linearised value at a feasible step
    c_lb = np.full(m, -INF); c_ub = np.full(m, INF)
    meq = m // 3
    c_lb[:meq] = act[:meq]; c_ub[:meq] = act[:meq]
    k = (m - meq) // 2
    c_ub[meq:meq + k] = act[meq:meq + k] + rng.uniform(0, 0.05, k)
    c_lb[meq + k:] = act[meq + k:] - rng.uniform(0, 0.05, m - meq - k)
    for i in range(n_range):                                # two-sided rows at the end
        r = m - 1 - i
        c_lb[r] = act[r] - 0.02; c_ub[r] = act[r] + 0.03
    if infeasible:
        c_lb[0] = c_ub[0] = act[0] + 50.0
    df = rng.standard_normal(n)
    return dict(n=n, m=m, j_row=rows + 1, j_col=cols + 1, dE=vals, df=df, f=0.3, E=E, x_k=x_k,
                c_lb=c_lb, c_ub=c_ub, v_lb=v_lb, v_ub=v_ub, delta=delta, J=J)


def equality_rich_subproblem(seed, n=300, neq=260, nineq=160, per_row=4, delta=0.6):
    """A sparse sub-problem with the row structure of the ACOPF configurations: many equality rows (their null space is small),
    fewer inequality rows, a few non-zeros per row - the shape on which the solver eliminates the equality rows
    (null-space form of the interior-point Newton system, active-set solves in reduced coordinates)."""
    rng = np.random.default_rng(seed)
    m = neq + nineq
    rows = np.repeat(np.arange(m), per_row)
    cols = np.concatenate([rng.choice(n, per_row, replace=False) for _ in range(m)])
    # every equality row owns one column (a permuted identity keeps the equality block of full row rank)
    own = np.arange(neq) * per_row
    cols[own] = rng.permutation(n)[:neq]
    vals = rng.standard_normal(len(rows)) * 0.5
    vals[own] = 1.0 + rng.random(neq)
    J = np.zeros((m, n))
    np.add.at(J, (rows, cols), vals)
    x_k = rng.uniform(-0.3, 0.3, n)
    v_lb = -np.ones(n); v_ub = np.ones(n)
    p_star = rng.uniform(-0.2, 0.2, n)
    E = rng.standard_normal(m) * 0.05
    act = E + J @ p_star
    c_lb = np.full(m, -INF); c_ub = np.full(m, INF)
    c_lb[:neq] = act[:neq]; c_ub[:neq] = act[:neq]
    k = nineq // 2
    c_ub[neq:neq + k] = act[neq:neq + k] + rng.uniform(0, 0.05, k)
    c_lb[neq + k:] = act[neq + k:] - rng.uniform(0, 0.05, nineq - k)
    df = rng.standard_normal(n)
    return dict(n=n, m=m, j_row=rows + 1, j_col=cols + 1, dE=vals, df=df, f=0.1, E=E, x_k=x_k,
                c_lb=c_lb, c_ub=c_ub, v_lb=v_lb, v_ub=v_ub, delta=delta, J=J, p_star=p_star)


def oracle_solve(sp, feasibility=False, qp=None):
    from oracle.subproblem import QpData, QpModel, compute_jacobian_matrix
    A, stored = compute_jacobian_matrix(sp['m'], sp['n'], sp['j_row'] - 1, sp['j_col'] - 1, sp['dE'])
    data = QpData(sp['df'], sp['f'], A, sp['E'], sp['c_lb'], sp['c_ub'], sp['v_lb'], sp['v_ub'], stored)
    if qp is None:
        qp = QpModel(data, sp['j_row'], sp['j_col'])
    else:
        qp.data = data
    out = qp.sub_optimize(sp['x_k'], sp['delta'], feasibility)
    return qp, out


def hip_solve(sp, feasibility=False, opt=None, device=0):
    from activesetmethods_amd.subproblem import QpData, HipSubOptimizer
    data = QpData(sp['df'], sp['f'], sp['dE'], sp['E'], sp['c_lb'], sp['c_ub'], sp['v_lb'], sp['v_ub'])
    if opt is None:
        opt = HipSubOptimizer(data, sp['j_row'], sp['j_col'], device=device)
    else:
        opt.data = data
    out = opt.sub_optimize(sp['x_k'], sp['delta'], feasibility)
    return opt, out


def rel_err(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    return float(np.abs(a - b).max(initial=0.0) / max(1.0, np.abs(b).max(initial=0.0)))


def edge_case_subproblems():
    """Degenerate shapes of the sub-LP boundary: no rows, one variable (the README problem at x = 0), rows without
    Jacobian entries, all variables fixed, zero trust region, duplicates cancelling to a stored exact zero."""
    e = np.zeros(0); I = np.zeros(0, np.int64)
    one = lambda **kw: dict(f=0.0, **kw)
    return {
        "no_rows": one(n=3, m=0, j_row=I, j_col=I, dE=e, df=np.array([1.0, -2.0, 0.0]), E=e, x_k=np.zeros(3), c_lb=e, c_ub=e,
                       v_lb=-np.ones(3), v_ub=np.ones(3), delta=0.4),
        "one_var": one(n=1, m=1, j_row=np.array([1]), j_col=np.array([1]), dE=np.array([-1.0]), df=np.array([1.0]), E=np.array([0.0]),
                       x_k=np.zeros(1), c_lb=np.array([2.0]), c_ub=np.array([2.0]), v_lb=np.array([-INF]), v_ub=np.array([INF]), delta=1000.0),
        "no_entries": one(n=2, m=2, j_row=I, j_col=I, dE=e, df=np.array([1.0, 1.0]), E=np.array([0.5, -0.5]), x_k=np.zeros(2),
                          c_lb=np.array([0.0, -INF]), c_ub=np.array([INF, 0.0]), v_lb=-np.ones(2), v_ub=np.ones(2), delta=0.4),
        "all_fixed": one(n=2, m=1, j_row=np.array([1, 1]), j_col=np.array([1, 2]), dE=np.array([1.0, 1.0]), df=np.array([1.0, -1.0]),
                         E=np.array([0.0]), x_k=np.array([0.3, 0.7]), c_lb=np.array([-1.0]), c_ub=np.array([1.0]),
                         v_lb=np.array([0.3, 0.7]), v_ub=np.array([0.3, 0.7]), delta=0.4),
        "zero_radius": one(n=2, m=1, j_row=np.array([1, 1]), j_col=np.array([1, 2]), dE=np.array([1.0, 1.0]), df=np.array([1.0, -1.0]),
                           E=np.array([0.0]), x_k=np.array([0.3, 0.7]), c_lb=np.array([-1.0]), c_ub=np.array([1.0]),
                           v_lb=-np.ones(2), v_ub=np.ones(2), delta=0.0),
        "cancelling_duplicates": one(n=2, m=1, j_row=np.array([1, 1, 1]), j_col=np.array([1, 1, 2]), dE=np.array([1.0, -1.0, 2.0]),
                                     df=np.array([1.0, 1.0]), E=np.array([0.1]), x_k=np.zeros(2), c_lb=np.array([0.0]), c_ub=np.array([0.0]),
                                     v_lb=-np.ones(2), v_ub=np.ones(2), delta=0.4),
    }


EDGE_CASE_ANSWERS = {      # worked by hand from the LP each case poses
    "no_rows": ([-0.4, 0.4, 0.0], []),
    "one_var": ([-2.0], [-1.0]),                 # -p = 2 ; df - J'lambda = 1 - (-1)(-1) = 0
    "no_entries": ([-0.4, -0.4], [0.0, 0.0]),
    "all_fixed": ([0.0, 0.0], [0.0]),
    "zero_radius": ([0.0, 0.0], [0.0]),
    "cancelling_duplicates": ([-0.4, -0.05], [0.5]),   # 2 p2 = -0.1 ; 1 - 2 lambda = 0
}


def banded_subproblem(seed, n=400, m=600, neq=120, nrange=30, width=6, per_row=4, delta=0.5, infeasible=False):
    """A sparse sub-problem whose rows couple locally (row i touches columns near i n / m), stored in a random row order: the coupling
    graph has a small bandwidth that only a reordering finds - the shape on which the library factors banded matrices (reverse
    Cuthill-McKee order of the rows / columns).  m >= 256 rows so that the order is used."""
    rng = np.random.default_rng(seed)
    shuffle = rng.permutation(m)                            # row i of the hidden chain is stored as row shuffle[i]
    rows, cols, vals = [], [], []
    for i in range(m):
        c0 = int(i * n / m)
        cand = np.arange(max(0, c0 - width), min(n, c0 + width + 1))
        cs = rng.choice(cand, min(per_row, len(cand)), replace=False)
        for c in cs:
            rows.append(shuffle[i]); cols.append(int(c)); vals.append(rng.standard_normal() * 0.5 + (1.5 if c == c0 else 0.0))
    rows, cols, vals = np.array(rows), np.array(cols), np.array(vals)
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    J = np.zeros((m, n))
    np.add.at(J, (rows, cols), vals)
    x_k = rng.uniform(-0.3, 0.3, n)
    v_lb = -np.ones(n); v_ub = np.ones(n)
    p_star = rng.uniform(-0.2, 0.2, n)
    E = rng.standard_normal(m) * 0.05
    act = E + J @ p_star
    kinds = rng.permutation(m)
    c_lb = np.full(m, -INF); c_ub = np.full(m, INF)
    eq = kinds[:neq]; rg = kinds[neq:neq + nrange]; rest = kinds[neq + nrange:]
    c_lb[eq] = act[eq]; c_ub[eq] = act[eq]
    c_lb[rg] = act[rg] - rng.uniform(0, 0.1, len(rg)); c_ub[rg] = act[rg] + rng.uniform(0, 0.1, len(rg))
    half = len(rest) // 2
    c_ub[rest[:half]] = act[rest[:half]] + rng.uniform(0, 0.05, half)
    c_lb[rest[half:]] = act[rest[half:]] - rng.uniform(0, 0.05, len(rest) - half)
    if infeasible:                                          # contradictory bounds on a few rows: the normal-phase LP is infeasible
        bad = rest[:8]
        c_ub[bad] = act[bad] - 5.0
    df = rng.standard_normal(n)
    return dict(n=n, m=m, j_row=rows + 1, j_col=cols + 1, dE=vals, df=df, f=0.1, E=E, x_k=x_k,
                c_lb=c_lb, c_ub=c_ub, v_lb=v_lb, v_ub=v_ub, delta=delta, J=J, p_star=p_star)


def random_function_model(seed, n=30, sense="MIN_SENSE"):
    """A random model in the MOI wrapper's six lists (affine and quadratic functions, duplicates, diagonal quadratic terms)."""
    from activesetmethods_amd.moi_evaluator import FunctionModel, ScalarFunction
    rng = np.random.default_rng(seed)
    fm = FunctionModel(n, -np.ones(n), np.ones(n))
    fm.sense = sense

    def func(quad):
        aff = [(float(rng.standard_normal()), int(rng.integers(1, n + 1))) for _ in range(int(rng.integers(0, 6)))]
        q = []
        if quad:
            for _ in range(int(rng.integers(1, 5))):
                a, b = int(rng.integers(1, n + 1)), int(rng.integers(1, n + 1))
                if rng.random() < 0.4:
                    b = a
                q.append((float(rng.standard_normal()), a, b))
        return ScalarFunction(float(rng.standard_normal()), aff, q)
    for kind in ("le", "ge", "eq"):
        for _ in range(int(rng.integers(1, 5))):
            fm.add_constraint(func(False), kind, float(rng.standard_normal()))
        for _ in range(int(rng.integers(1, 5))):
            fm.add_constraint(func(True), kind, float(rng.standard_normal()))
    fm.objective = func(True)
    return fm


def oracle_wrapper_model(fm):
    """The plain-dict model of oracle/moi_eval.py from the RAW data of a FunctionModel (constants and term lists as they were given to it -
    nothing of the product's evaluation or flattening code is used): the independent checker of rows a2 / f3."""
    def fn(f):
        return {"constant": float(f.constant), "affine": [(float(c), int(v)) for c, v in f.affine],
                "quadratic": [(float(c), int(a), int(b)) for c, a, b in f.quadratic]}
    m = {"n": fm.n, "sense": fm.sense, "objective": None if fm.objective is None else fn(fm.objective)}
    for name in ("linear_le", "linear_ge", "linear_eq", "quadratic_le", "quadratic_ge", "quadratic_eq"):
        m[name] = [fn(f) for f, _ in getattr(fm, name)]
    m["nlp"] = None
    if fm.nlp is not None:
        blk = fm.nlp
        m["nlp"] = {"m": blk.m, "pattern": list(zip(blk.rows.tolist(), blk.cols.tolist())),
                    "eval_g": lambda x: blk.eval_g(np.asarray(x, float), np.zeros(blk.m)),
                    "eval_jac": lambda x: blk.eval_jac_g(np.asarray(x, float), np.zeros(len(blk.rows)))}
    return m


def oracle_evaluate(om, x):
    """(f, grad f, g, Jacobian values, j_str) of a wrapper model through oracle/moi_eval.py."""
    from oracle import moi_eval as W
    xs = [float(v) for v in x]
    j_str = W.jacobian_structure(om)
    m = W.nlp_constraint_offset(om) + (om["nlp"]["m"] if om["nlp"] is not None else 0)
    g = W.eval_constraint(om, [0.0] * m, xs)
    vals = W.eval_constraint_jacobian(om, [0.0] * len(j_str), xs)
    grad = W.eval_objective_gradient(om, [0.0] * om["n"], xs)
    return W.eval_objective(om, xs), np.array(grad), np.array(g, float), np.array(vals, float), j_str


# ----------------------------------------------------------------------------- guarded Cholesky: matrices with designed pivots
GUARD_SETTINGS = {      # (k_diag_prepare mode, rel, absv, pivot threshold) as the library factors (asm_hip.hip)
    "hook": (0, 0.0, 0.0, 1e-14),        # the kernel hooks' default
    "ipm": (0, 1e-13, 1e-30, 1e-14),     # Schur matrices of the interior-point iterations
    "s0": (1, 0.0, 0.0, 1e-10),          # S0 = A_EF A_EF' of the null-space form, the active-set solves
}
DEP_LEVEL = 1e-12       # designed pivot / diag0 of a dependent row: 100x above 1e-14, 100x below 1e-10


def designed_pivot_spd(seed, N, levels, band=0, K=None):
    """SPD S = B B' + diag(delta) whose pivots are designed: row j of B in `levels` is a combination of two earlier independent rows of B
    (exactly: its Schur complement in B B' is zero up to rounding) and delta_j puts its pivot at levels[j] * S_jj, i.e. the guarded
    factorisation sees pivot / diag0 = levels[j] (a level 0 row is a zero row, S_jj = 0).  The other rows are independent (K >= 2 N
    columns: their pivots are >= ~1/2 of their diagonal) and get no diagonal.  band > 0: B has half-bandwidth band // 2 - 2 and the
    combinations use the two rows just above, so S stays within `band` of the diagonal.  Returns S and the designed levels (1 for the
    independent rows)."""
    rng = np.random.default_rng(seed)
    lv = np.ones(N)
    for j, l in levels.items():
        lv[j] = l
    dep = lv < 1.0
    if band > 0:
        hb = band // 2 - 2
        assert hb >= 1
        B = np.zeros((N, N))
        for d in range(-hb, hb + 1):
            i = np.arange(max(0, -d), min(N, N - d))
            B[i, i + d] = rng.standard_normal(len(i))
        B[np.arange(N), np.arange(N)] += 3.0
    else:
        K = K or 2 * N + 8
        B = rng.standard_normal((N, K))
    for j in np.flatnonzero(dep):
        B[j] = 0.0
        if lv[j] == 0.0:
            continue
        if band > 0:
            src = [i for i in (j - 1, j - 2) if i >= 0 and not dep[i]]
        else:
            src = list(rng.choice([i for i in range(j) if not dep[i]], size=min(2, int((~dep[:j]).sum())), replace=False)) if j else []
        assert src, "row %d: no earlier independent row to depend on" % j
        for i in src:
            B[j] += rng.uniform(0.5, 1.5) * B[i]
    S = B @ B.T
    for j in np.flatnonzero(dep):
        if lv[j] > 0.0:
            S[j, j] += lv[j] / (1.0 - lv[j]) * S[j, j]       # the Schur complement of B B' at j is 0: the pivot is this delta
    S = np.tril(S) + np.tril(S, -1).T
    if band > 0:
        i, k = np.nonzero(S)
        assert np.abs(i - k).max() <= band
    return S, lv


def guard_prepare(S, mode, rel, absv):
    """k_diag_prepare restated: the matrix the guarded factorisation sees and the diag0 its threshold is relative to."""
    S = S.copy()
    d0 = np.diag(S).copy()
    reg = rel * d0 + absv if mode == 0 else np.full(len(d0), rel * max(d0.max(initial=0.0), 1e-300))
    S[np.arange(len(d0)), np.arange(len(d0))] = d0 + reg
    return S, d0


def expected_dropped(levels, setting):
    """Rows the guard drops by design: pivot level below the threshold (a zero row only when the diagonal is not regularised)."""
    mode, rel, absv, thr = GUARD_SETTINGS[setting] if isinstance(setting, str) else setting
    lv = np.asarray(levels)
    drop = lv < thr
    if mode == 0 and absv > 0.0:
        drop &= lv > 0.0           # S_jj = 0 + absv > thr * 0: a zero row is kept (its unknown is b_j / absv)
    return np.flatnonzero(drop)


# --------------------------------------------------------------------------------------------------------------------------------------
# Newton-matrix builds (tests/test_builds_cpu.py, tests/test_builds_gpu.py): operands, the long-double reference and the rounding bound
U = 2.0 ** -53
SENTINEL = -7.25          # finite pre-fill of every output buffer: what a kernel does not own must keep it bit for bit

# (name, Ms, K, tile (0 = the solver's choice), gathered row list, diag given) - what each case is there for:
#   t1-long / t2-long / t4-long: K = 4096, the chunk list of the full tile has 128 entries (second ballot pass of k_syrk)
#   t1-pairs (78 tile pairs), t4-pairs (78), t2-grid (Ms = 2100, 33 tiles = 561 tile pairs: a second dealt run and a second grid block of 512)
#   t1-maxchunks: K = 32768 = ASM_MAXCHUNKS chunks;  pick: tile chosen by the solver's rule (Ms = 800 -> 64 rows)
FLAGGED_CASES = [
    ("t1-long", 100, 4096, 1, False, True),
    ("t1-pairs", 370, 512, 1, True, False),
    ("t1-maxchunks", 125, 32768, 1, False, True),
    ("t2-long", 200, 4096, 2, True, True),
    ("t2-grid", 2100, 256, 2, False, False),
    ("t4-long", 300, 4096, 4, False, True),
    ("t4-pairs", 1420, 256, 4, True, False),
    ("pick", 800, 512, 0, True, True),
]


def pick_tile(Ms):
    """The solver's tile choice (Dev::pick_tile)."""
    return 4 if Ms >= 3072 else (2 if Ms >= 768 else 1)


def flagged_operand(seed, Ms, K, tile, gathered, with_diag):
    """Block-sparse operand of a chunk-skipping build.  With TS = 32 * tile rows per tile and 32 columns per chunk: tile 0 has a non-zero in
    every chunk, tiles 1 and 2 hold the even and the odd chunks only (their lists do not intersect), every other tile a random eighth to
    half of the chunks.  Inside a flagged (tile, chunk) block 30 % of the entries are set, in the top half of the tile's rows only, the
    bottom half only, or all of them (flags computed from part of a tile's rows are wrong).  gathered: the rows sit at a non-monotone
    permutation idx of a subset of a taller matrix whose other rows are dense.  theta is positive over eight decades with exact zeros and
    one negative entry.  Returns A, idx (int32 or None), theta, diag (or None)."""
    rng = np.random.default_rng(seed)
    T = tile if tile > 0 else pick_tile(Ms)
    TS, nch = 32 * T, K // 32
    nt = (Ms + TS - 1) // TS
    assert nt >= 3 and K % 32 == 0
    B = np.zeros((Ms, K))
    for t in range(nt):
        r0, r1 = t * TS, min(Ms, (t + 1) * TS)
        if t == 0:
            on = np.ones(nch, bool)
        elif t in (1, 2):
            on = (np.arange(nch) % 2) == (t - 1)
            on &= rng.random(nch) < 0.6
            on[t - 1] = True
        else:
            on = rng.random(nch) < rng.uniform(0.125, 0.5)
        for c in np.nonzero(on)[0]:
            part = rng.integers(0, 3)
            h = max(1, (r1 - r0) // 2)
            a, b = (r0, r0 + h) if part == 0 else ((r0 + h, r1) if part == 1 and r0 + h < r1 else (r0, r1))
            blk = np.where(rng.random((b - a, 32)) < 0.3, rng.standard_normal((b - a, 32)), 0.0)
            if not blk.any():
                blk[rng.integers(0, b - a), rng.integers(0, 32)] = 1.0 + rng.random()
            B[a:b, 32 * c:32 * c + 32] = blk
    theta = 10.0 ** rng.uniform(-4.0, 4.0, K)
    theta[rng.random(K) < 0.05] = 0.0
    theta[int(rng.integers(0, K))] = -3.5
    diag = rng.uniform(0.5, 2.0, Ms) * 10.0 ** rng.uniform(-2, 2, Ms) if with_diag else None
    if not gathered:
        return B, None, theta, diag
    M = Ms + Ms // 3 + 5
    idx = rng.permutation(M)[:Ms].astype(np.int32)
    assert np.any(np.diff(idx) < 0)
    A = rng.standard_normal((M, K))
    A[idx] = B
    return A, idx, theta, diag


def tile_chunk_flags(A, idx, Ms, TS):
    """flags[t, c] = any(A[rows of tile t, 32 c : 32 c + 32] != 0) for the row list idx (None: the first Ms rows), tiles of TS rows."""
    B = A[idx] if idx is not None else A[:Ms]
    nt, nch = (Ms + TS - 1) // TS, A.shape[1] // 32
    P = np.zeros((nt * TS, A.shape[1]), bool)
    P[:Ms] = B != 0
    return P.reshape(nt, TS, nch, 32).any(axis=(1, 3)).astype(np.uint8)


def executed_fraction(flags):
    """Share of the (tile pair, chunk) products a chunk-skipping build executes (the host formula of Dev::executed_fraction_now)."""
    nt, nch = flags.shape
    act = tot = 0.0
    for a in range(nt):
        for b in range(a + 1):
            act += float(np.count_nonzero(flags[a] & flags[b]))
            tot += float(nch)
    return act / tot if tot > 0 else 1.0


def build_reference(B, theta, diag=None, block=256):
    """Lower triangles (the rest zero) of  ref = B diag(theta) B' + diag  and  mag = |B| diag(|theta|) |B|' + |diag|  in long double, and of
    keff[i, j] = number of k with B_ik theta_k B_jk != 0 (int64)."""
    Ms = B.shape[0]
    Bl = B.astype(np.longdouble)
    Wl = Bl * theta.astype(np.longdouble)
    ind = ((B != 0) & (theta != 0)).astype(np.float64)
    ref = np.zeros((Ms, Ms), np.longdouble)
    mag = np.zeros((Ms, Ms), np.longdouble)
    for i0 in range(0, Ms, block):
        i1 = min(Ms, i0 + block)
        ref[i0:i1, :i1] = Wl[i0:i1] @ Bl[:i1].T
        mag[i0:i1, :i1] = np.abs(Wl[i0:i1]) @ np.abs(Bl[:i1]).T
    keff = np.rint(ind @ ind.T).astype(np.int64)
    if diag is not None:
        ref[np.arange(Ms), np.arange(Ms)] += diag.astype(np.longdouble)
        mag[np.arange(Ms), np.arange(Ms)] += np.abs(diag).astype(np.longdouble)
    return np.tril(ref), np.tril(mag), np.tril(keff)


def rounding_bound_ratio(S, ref, mag, keff, extra=0):
    """Largest |S - ref| / (gamma_n mag) over the lower triangle, n = keff + 2 + extra per entry, gamma_n = n u / (1 - n u): the bound of
    any summation order of keff non-zero products, with or without FMA (one rounding for theta, one per accumulated product, one for the
    diagonal term; `extra` for the additions of split-K slices).  Entries with keff = 0 and no diagonal term must be exactly 0.0 (ratio inf
    otherwise); with mag > 0 only from the diagonal term they must be exactly it, which the bound n = 2 allows for and `exact` reports."""
    Ms = ref.shape[0]
    low = np.tril(np.ones((Ms, Ms), bool))
    n = (keff + 2 + extra).astype(np.longdouble)
    gam = n * np.longdouble(U) / (1 - n * np.longdouble(U))
    err = np.abs(S[:Ms, :Ms].astype(np.longdouble) - ref)
    bound = gam * mag
    ratio = np.zeros((Ms, Ms), np.longdouble)
    pos = low & (bound > 0)
    ratio[pos] = err[pos] / bound[pos]
    ratio[low & (bound == 0) & (err != 0)] = np.inf
    exact = bool(np.all(err[low & (keff == 0)] == 0))          # no product at all: exactly the diagonal term, or 0.0
    return float(ratio.max()), exact


# split-K builds of the k x k matrix of the null-space form: (k, K / 32, slice counts)
SPLIT_KS = [1, 31, 32, 33, 137, 256, 257, 519, 530]
SPLIT_CHUNKS = [1, 7, 8, 9, 16]
SPLIT_COUNTS = [1, 2, 3, 4, 8]
SPLIT_CASES = [(k, c, SPLIT_COUNTS) for k in SPLIT_KS for c in SPLIT_CHUNKS] + [(137, 599, [1, 3, 8]), (519, 599, [8])]      # (519, 599 x 32 = 19168, 8): the C4 shape


def split_operand(seed, k, K):
    """G (k x K, 70 % zeros) and a positive theta spread over eight decades (an interior point near convergence)."""
    rng = np.random.default_rng(seed)
    G = np.where(rng.random((k, K)) < 0.3, rng.standard_normal((k, K)), 0.0)
    theta = 10.0 ** rng.uniform(-4.0, 4.0, K)
    return G, theta


def split_ranges(K, nsplit):
    """Column range [k0, k1) of every slice of a split-K build: per = ceil((K / 32) / nsplit) * 32 columns each, the trailing ones short or empty."""
    nch = K // 32
    per = ((nch + nsplit - 1) // nsplit) * 32
    return [(min(K, s * per), min(K, (s + 1) * per)) for s in range(nsplit)]
