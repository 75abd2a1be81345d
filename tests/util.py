"""Shared generators for the parity tests (seeded, deterministic)."""
import ctypes as C

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


# the sub-LP entries of the raw C ABI (`lib`: the loaded library, `h`: a handle), for the tests that watch a handle's state across calls
def abi_create(lib):
    h = C.c_void_p()
    assert lib.asm_create(0, C.byref(h)) == 0
    return h


def abi_setup(lib, h, sp):
    from activesetmethods_amd import _lib
    jr, jc = (np.ascontiguousarray(sp[k], dtype=np.int64) for k in ('j_row', 'j_col'))
    b = [np.ascontiguousarray(sp[k], dtype=np.float64) for k in ('c_lb', 'c_ub', 'v_lb', 'v_ub')]
    return lib.asm_sublp_setup(h, sp['n'], sp['m'], len(jr), _lib.i64ptr(jr), _lib.i64ptr(jc), *[_lib.dptr(a) for a in b])


def abi_set_bounds(lib, h, sp):
    from activesetmethods_amd import _lib
    b = [np.ascontiguousarray(sp[k], dtype=np.float64) for k in ('c_lb', 'c_ub', 'v_lb', 'v_ub')]
    return lib.asm_sublp_set_bounds(h, *[_lib.dptr(a) for a in b])


def abi_solve(lib, h, sp, feasibility=0):
    """One LP on a set-up handle: (the raw bytes of status, step, multipliers, slacks and active sets - outputs are zero-initialised, so
    entries the library leaves alone compare equal -, the statistics of the solve)."""
    from activesetmethods_amd import _lib
    n, m = sp['n'], sp['m']
    dE, df, E, x_k = (np.ascontiguousarray(sp[k], dtype=np.float64) for k in ('dE', 'df', 'E', 'x_k'))
    p, lam, mU, mL, ps = np.zeros(n), np.zeros(m), np.zeros(n), np.zeros(n), np.zeros(2 * max(m, 1))
    st = C.c_int32(0)
    assert lib.asm_sublp_solve(h, _lib.dptr(dE), _lib.dptr(df), float(sp['f']), _lib.dptr(E), _lib.dptr(x_k), float(sp['delta']), feasibility,
                               _lib.dptr(p), _lib.dptr(lam), _lib.dptr(mU), _lib.dptr(mL), _lib.dptr(ps), C.byref(st)) == 0
    nr, nsl = C.c_int64(0), C.c_int64(0)
    assert lib.asm_sublp_active_set(h, None, None, None, C.byref(nr), C.byref(nsl)) == 0
    rows, bnd, sl = np.zeros(max(nr.value, 1), np.int32), np.zeros(n, np.int32), np.zeros(max(nsl.value, 1), np.int32)
    assert lib.asm_sublp_active_set(h, _lib.i32ptr(rows), _lib.i32ptr(bnd), _lib.i32ptr(sl), None, None) == 0
    s = _lib.SolveStats()
    assert lib.asm_sublp_last_stats(h, C.byref(s)) == 0
    return [st.value] + [a.tobytes() for a in (p, lam, mU, mL, ps, rows, bnd, sl)], {k: getattr(s, k) for k, _ in s._fields_}


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


# --------------------------------------------------------------------------------------------------------------------------------------
# Interior-point stage kernels (tests/test_ipm_stages_cpu.py, tests/test_ipm_stages_gpu.py): states, and a long-double twin of every stage
# written from the statements of oracle/lp_solver.py (class IPM) and the comments of asm_ipm_kernels.hip.h.
#
# A state is a dict: sizes n, M, ns, ncomp, scale_q; the integer arrays rtype, srow, rs0, rs1; `scal` (the 15 scalars, names IPM_SCALARS);
# and one float64 vector per name of IPM_VECTORS.  A twin function returns {output name: (value, magnitude, k)} in np.longdouble: `value`
# is the statement evaluated in long double from the float64 inputs, `magnitude` the same formula with every term replaced by its absolute
# value, k the operation count of the statement plus one, so that  |out - value| <= gamma_k magnitude  holds for float64 arithmetic in any
# association, with or without FMA contraction.  An output that depends on another output of the same kernel (hp on rcL, dmuL on dp, ...)
# is stated from the value the DEVICE wrote for that one (argument `dev`): a bound through a chain would have to carry the cancellation
# of the intermediate, and what the kernel does is exactly the statement applied to its own rounded intermediate.
IPM_SCALARS = "PINF DINF MU YMAX AP AD SM EMAX RMAX RZ RPMAX RZ0 STOP NSERR SPEC".split()
# stage kinds (enum ASM_IPM_* of include/asm_hip.h) and the order in which asm_test_ipm_stages reports the vectors' offsets
IPM_STAGE_KINDS = ("init_p", "init_rest", "measures", "theta", "rhs1", "rhs2", "vec_mul", "res", "pcg_start", "pcg_step1", "pcg_step2", "dir", "steps",
                   "muaff", "diradd", "update", "snapshot", "col_prep", "col_scale", "col_finish", "sdiag_csr", "red_gather", "red_scatter")
IPM_VECTORS = ("q lb ub r w slo scoef p s g y tL tU muL muU ts mus pi act aty rp rdp rds thp_inv ths_inv dS hp hs tmpn t1 rhs res rcL rcU rcs rcg "
               "A.dp A.ds A.dg A.dy A.dmuL A.dmuU A.dmus A.dpi C.dp C.ds C.dg C.dy C.dmuL C.dmuU C.dmus C.dpi sres corr pcg tN").split()
SC = {nm: i for i, nm in enumerate(IPM_SCALARS)}
IPM_N = "q lb ub p tL tU muL muU aty rdp thp_inv hp tmpn rcL rcU A.dp A.dmuL A.dmuU C.dp C.dmuL C.dmuU tN".split()
IPM_M = "r g y pi act rp dS t1 rhs res rcg A.dg A.dy A.dpi C.dg C.dy C.dpi sres corr pcg".split()
IPM_S = "w slo scoef s ts mus rds ths_inv hs rcs A.ds A.dmus C.ds C.dmus".split()
IPM_RHO_P, MCC_BMIN, MCC_BMAX, COL_FIXED = 1e-8, 0.1, 10.0, 1e200
LD = np.longdouble
BIG = 1e300


def gamma(k):
    k = np.asarray(k, LD)
    return k * LD(U) / (1 - k * LD(U))


def bound_ratio(out, val, mag, k):
    """Largest |out - val| / (gamma_k mag); inf where mag == 0 and out != val."""
    out, val, mag = np.atleast_1d(np.asarray(out, LD)), np.atleast_1d(np.asarray(val, LD)), np.atleast_1d(np.asarray(mag, LD))
    if out.size == 0:
        return 0.0
    err = np.abs(out - val)
    b = gamma(k) * mag
    r = np.zeros(out.shape, LD)
    pos = b > 0
    r[pos] = err[pos] / b[pos]
    r[(~pos) & (err != 0)] = np.inf
    r[~np.isfinite(np.asarray(out, LD))] = np.inf
    return float(r.max())


def ipm_vec_len(st, name):
    return st["n"] if name in IPM_N else (st["M"] if name in IPM_M else st["ns"])


def ipm_slack_lists(M, srow):
    """rs0 / rs1 of every row as asm_sublp_setup makes them: the first and the second slack column of the row, -1 for none."""
    rs0 = np.full(M, -1, np.int32)
    rs1 = np.full(M, -1, np.int32)
    for k, r_ in enumerate(srow):
        if rs0[r_] < 0:
            rs0[r_] = k
        else:
            assert rs1[r_] < 0
            rs1[r_] = k
    return rs0, rs1


def ipm_state(seed, n, M, ns, mu=1.0, fixed_frac=0.1):
    """A scrambled interior-point state of sizes (n, M, ns), ns <= 2 M.  Rows: equalities, both inequality signs; slack columns dealt to rows,
    at most two per row (the first with coefficient +1, the second -1, as the solver lays them out: range / equality rows of a restoration
    LP).  About fixed_frac of the columns are fixed (ub == lb) and carry what the solver keeps there (tL = tU = 1, zero multipliers).  The
    complementarity pairs have t over eight decades and multipliers mu / t times a factor over two decades - pairs of opposite extremes at
    every level of mu.  Bounds are finite: the LP container's bounds are the finite trust region (oracle/lp_solver.py, module docstring),
    and scale_lp divides by finite powers of two, so no infinity reaches these kernels.  Everything else - residuals, work vectors,
    directions, products with the matrix - is standard normal, so every stage can be run on its own from this state."""
    rng = np.random.default_rng(seed)
    assert n >= 1 and 0 <= ns <= 2 * M
    st = {"n": n, "M": M, "ns": ns}
    st["rtype"] = rng.integers(-1, 2, M).astype(np.int32)
    npair = max(ns - M, ns // 3) if ns >= 2 else 0                  # rows with two slack columns (rs0 and rs1 both set)
    rows = rng.permutation(M)[:ns - npair]
    srow = np.sort(np.concatenate([rows, rows[:npair]])).astype(np.int32)
    st["srow"] = srow
    st["rs0"], st["rs1"] = ipm_slack_lists(M, srow)
    for nm in IPM_N + IPM_M + IPM_S:
        st[nm] = rng.standard_normal(ipm_vec_len(st, nm))
    sc = np.where(rng.random(ns) < 0.5, 1.0, -1.0)
    for i in range(M):
        if st["rs1"][i] >= 0:
            sc[st["rs0"][i]], sc[st["rs1"][i]] = 1.0, -1.0
    st["scoef"] = sc
    st["lb"] = -10.0 ** rng.uniform(-2, 3, n)
    st["ub"] = 10.0 ** rng.uniform(-2, 3, n)
    fx = rng.random(n) < fixed_frac
    st["ub"][fx] = st["lb"][fx]

    def pair(cnt):
        t = 10.0 ** rng.uniform(-6, 2, cnt)
        return t, mu / t * 10.0 ** rng.uniform(-1, 1, cnt)
    st["tL"], st["muL"] = pair(n)
    st["tU"], st["muU"] = pair(n)
    st["ts"], st["mus"] = pair(ns)
    st["g"], st["pi"] = pair(M)
    st["tL"][fx] = st["tU"][fx] = 1.0
    st["muL"][fx] = st["muU"][fx] = 0.0
    eq = st["rtype"] == 0
    st["g"][eq] = 1.0
    st["pi"][eq] = 0.0
    st["y"] = np.where(eq, st["y"], st["rtype"] * st["pi"])
    st["thp_inv"] = np.where(fx, 0.0, 10.0 ** rng.uniform(-6, 2, n))
    st["ths_inv"] = 10.0 ** rng.uniform(-6, 2, ns)
    st["dS"] = 10.0 ** rng.uniform(-6, 2, M)
    st["scale_q"] = 4.0
    st["ncomp"] = max(2 * int((~fx).sum()) + ns + int((~eq).sum()), 1)
    scal = 10.0 ** rng.uniform(-3, 1, len(IPM_SCALARS))
    scal[SC["MU"]] = mu
    scal[SC["SM"]] = 0.3 * mu
    scal[SC["AP"]], scal[SC["AD"]] = 0.75, 0.5
    scal[SC["STOP"]] = scal[SC["SPEC"]] = 0.0
    st["scal"] = scal
    return st


def _l(st, *names):
    return [st[nm].astype(LD) for nm in names]


def _slack_sum(st, v):
    """(sum, magnitude, term count) per row of  sum_k scoef_k v_k  over the row's slack columns."""
    M = st["M"]
    a, m, c = np.zeros(M, LD), np.zeros(M, LD), np.zeros(M, np.int64)
    if st["ns"]:
        for rs in (st["rs0"], st["rs1"]):
            has = rs >= 0
            t = st["scoef"][rs[has]].astype(LD) * np.asarray(v, LD)[rs[has]]
            a[has] += t
            m[has] += np.abs(t)
            c[has] += 1
    return a, m, c


def _free(st):
    return st["ub"] > st["lb"]


def tw_measures(st):
    """rp, rdp, rds element by element and mu (oracle: IPM.measures).  mu: k = number of products + 3 (a rounding per product, one per
    addition, the division by ncomp).  The maxima are exact statements on the written residuals: ipm_measures_exact."""
    ineq, fr = st["rtype"] != 0, _free(st)
    act, r, g, pi = _l(st, "act", "r", "g", "pi")
    sa, sm_, _ = _slack_sum(st, st["s"])
    gg = np.where(ineq, g, 0)
    out = {"rp": (act + sa - (r + st["rtype"] * gg), np.abs(act) + sm_ + np.abs(r) + np.abs(gg), 7)}
    q, aty, muL, muU, tL, tU = _l(st, "q", "aty", "muL", "muU", "tL", "tU")
    out["rdp"] = (np.where(fr, q - aty - muL + muU, 0), np.where(fr, np.abs(q) + np.abs(aty) + np.abs(muL) + np.abs(muU), 0), 4)
    w, sc, mus, ts = _l(st, "w", "scoef", "mus", "ts")
    ys = st["y"].astype(LD)[st["srow"]]
    out["rds"] = (w - sc * ys - mus, np.abs(w) + np.abs(sc * ys) + np.abs(mus), 4)
    terms = np.concatenate([(g * pi)[ineq], (tL * muL)[fr], (tU * muU)[fr], ts * mus])
    nc = LD(st["ncomp"])
    out["MU"] = (terms.sum() / nc, np.abs(terms).sum() / nc, len(terms) + 3)
    return out


def ipm_measures_exact(st, rp, rdp, rds):
    """PINF, DINF, YMAX, RPMAX in float64 from the residuals as written: divisions and maxima only, every operation correctly rounded."""
    pinf = float((np.abs(rp) / (1.0 + np.abs(st["r"]))).max(initial=0.0))
    dinf = max(float(np.abs(rdp).max(initial=0.0)), float(np.abs(rds).max(initial=0.0))) / st["scale_q"]
    return {"PINF": pinf, "DINF": dinf, "YMAX": float(np.abs(st["y"]).max(initial=0.0)), "RPMAX": float(np.abs(rp).max(initial=0.0))}


def ipm_theta_exact(st, rho_p):
    """thp_inv, ths_inv, dS in float64: divisions and plain additions in the kernel's order (no a*b +/- c shape: nothing to contract)."""
    fr = _free(st)
    with np.errstate(all="ignore"):
        th = np.where(fr, 1.0 / (st["muL"] / st["tL"] + st["muU"] / st["tU"] + rho_p), 0.0)
        ths = st["ts"] / st["mus"]
        d = np.where(st["rtype"] != 0, st["g"] / st["pi"], 0.0)
    if st["ns"]:
        for rs in (st["rs0"], st["rs1"]):
            has = rs >= 0
            d[has] = d[has] + ths[rs[has]]
    return {"thp_inv": th, "ths_inv": ths, "dS": d}


def _mcc(x, dx, z, dz, tp, td, lo, hi):
    """Gondzio's projected complementarity term.  v = (x + tp dx)(z + td dz) has five operations; the result clamp(v) - v (at least -hi) is
    a piecewise linear function of v with slopes in [-1, 0], so an error of v passes through at most unchanged, whatever branch the rounded
    v selects; one more rounding for the subtraction, against lo or hi: k = 7, magnitude |v|-formula + hi."""
    v = (x + tp * dx) * (z + td * dz)
    mv = (np.abs(x) + abs(tp) * np.abs(dx)) * (np.abs(z) + abs(td) * np.abs(dz))
    return np.maximum(np.minimum(np.maximum(v, lo), hi) - v, -hi), mv + abs(hi)


def tw_rhs1(st, base, mode, tp=0.0, td=0.0, dev=None):
    """rcL rcU rcs rcg, then (from the device's own rc*, `dev`) hp, hs and tmpn = thp_inv hp (oracle: IPM.run, solve / corr)."""
    fr, ineq = _free(st), st["rtype"] != 0
    sm = LD(st["scal"][SC["SM"]]) if mode else LD(0)
    lo, hi = LD(MCC_BMIN * float(sm)), LD(MCC_BMAX * float(sm))      # (one correctly rounded product each, as the kernel forms them)
    res = LD(0.0 if mode == 2 else 1.0)
    tL, tU, muL, muU, ts, mus, g, pi = _l(st, "tL", "tU", "muL", "muU", "ts", "mus", "g", "pi")
    dp, dmuL, dmuU, ds, dmus, dg, dpi = _l(st, base + ".dp", base + ".dmuL", base + ".dmuU", base + ".ds", base + ".dmus", base + ".dg", base + ".dpi")
    out = {}
    if mode == 2:
        vL, mL = _mcc(tL, dp, muL, dmuL, tp, td, lo, hi)
        vU, mU = _mcc(tU, -dp, muU, dmuU, tp, td, lo, hi)
        out["rcL"] = (np.where(fr, vL, 0), np.where(fr, mL, 0), 7)
        out["rcU"] = (np.where(fr, vU, 0), np.where(fr, mU, 0), 7)
        out["rcs"] = _mcc(ts, ds, mus, dmus, tp, td, lo, hi) + (7,)
        vg, mg = _mcc(g, dg, pi, dpi, tp, td, lo, hi)
        out["rcg"] = (np.where(ineq, vg, 0), np.where(ineq, mg, 0), 7)
    else:
        c = LD(1 if mode else 0)
        out["rcL"] = (sm - tL * muL - c * dp * dmuL, abs(sm) + np.abs(tL * muL) + c * np.abs(dp * dmuL), 5)
        out["rcU"] = (sm - tU * muU + c * dp * dmuU, abs(sm) + np.abs(tU * muU) + c * np.abs(dp * dmuU), 5)
        out["rcs"] = (sm - ts * mus - c * ds * dmus, abs(sm) + np.abs(ts * mus) + c * np.abs(ds * dmus), 5)
        out["rcg"] = (sm - g * pi - c * dg * dpi, abs(sm) + np.abs(g * pi) + c * np.abs(dg * dpi), 5)
    if dev is not None:
        rcL, rcU, rcs, hpd = dev["rcL"].astype(LD), dev["rcU"].astype(LD), dev["rcs"].astype(LD), dev["hp"].astype(LD)
        rdp, rds, thp = _l(st, "rdp", "rds", "thp_inv")
        out["hp"] = (np.where(fr, -res * rdp + rcL / tL - rcU / tU, 0), np.where(fr, res * np.abs(rdp) + np.abs(rcL / tL) + np.abs(rcU / tU), 0), 6)
        out["tmpn"] = (thp * hpd, np.abs(thp * hpd), 2)
        out["hs"] = (-res * rds + rcs / ts, res * np.abs(rds) + np.abs(rcs / ts), 4)
    return out


def tw_rhs2(st, res):
    """rhs = -res rp - t1 + sg rcg / pi - E (ths_inv hs)   (oracle: IPM.run, solve)."""
    ineq = st["rtype"] != 0
    rp, t1, rcg, pi = _l(st, "rp", "t1", "rcg", "pi")
    with np.errstate(all="ignore"):
        c = np.where(ineq, st["rtype"] * rcg / np.where(ineq, pi, 1), 0)
    sa, sm_, _ = _slack_sum(st, st["ths_inv"].astype(LD) * st["hs"].astype(LD))
    return {"rhs": (-LD(res) * rp - t1 + c - sa, abs(res) * np.abs(rp) + np.abs(t1) + np.abs(c) + sm_, 12)}


def tw_res(st, D):
    """res = rhs - (sres + dS dy); EMAX / RMAX / SPEC are exact statements on the written res (ipm_res_exact)."""
    rhs, sres, dS, dy = _l(st, "rhs", "sres", "dS", D + ".dy")
    return {"res": (rhs - (sres + dS * dy), np.abs(rhs) + np.abs(sres) + np.abs(dS * dy), 4)}


def ipm_res_exact(st, res_written, spec, crel, floor_):
    emax = float(np.abs(res_written).max(initial=0.0))
    rmax = max(1.0, float(np.abs(st["rhs"]).max(initial=0.0)))
    out = {"EMAX": emax, "RMAX": rmax, "SPEC": st["scal"][SC["SPEC"]]}
    if spec:
        bad = 1.0 if emax > max(crel * rmax, floor_) else 0.0
        out["SPEC"] = bad if spec == 1 else max(st["scal"][SC["SPEC"]], bad)
    return out


def _dot(a, b):
    return (a * b).sum(), np.abs(a * b).sum()


def tw_pcg_start(st):
    res, z = _l(st, "res", "corr")
    v, m = _dot(res, z)
    return {"RZ": (v, m, st["M"] + 2)}


def tw_pcg_step1(st, D):
    """acc = p'(sres + dS p) (three operations per term), alpha = rz / acc, x += alpha p, res -= alpha (sres + dS p).  The quotient carries
    the relative error of acc, gamma_(M+4) kappa with kappa = magnitude(acc) / |acc| (the condition number of the sum), so the alpha
    terms of the magnitudes are scaled by kappa; to first order in u, which k + 2 more than covers for kappa u << 1 (asserted by the
    generator: kappa < 1e3)."""
    p, sres, dS, x, res = _l(st, "pcg", "sres", "dS", D + ".dy", "res")
    sp = sres + dS * p
    acc, macc = (p * sp).sum(), (np.abs(p) * (np.abs(sres) + np.abs(dS * p))).sum()
    rz, rz0 = LD(st["scal"][SC["RZ"]]), LD(st["scal"][SC["RZ0"]])
    ok = bool(acc > 0 and rz > LD(1e-30) * rz0 and rz < LD(1e12) * acc)
    if not ok:
        return {"ok": False, "acc": acc, "macc": macc}
    kap = macc / abs(acc)
    al = rz / acc
    M = st["M"]
    return {"ok": True, "acc": acc, "macc": macc, "kappa": float(kap),
            "x": (x + al * p, np.abs(x) + kap * np.abs(al * p), M + 9), "res": (res - al * sp, np.abs(res) + kap * abs(al) * (np.abs(sres) + np.abs(dS * p)), M + 10)}


def tw_pcg_step2(st):
    res, z, p = _l(st, "res", "corr", "pcg")
    acc, macc = _dot(res, z)
    rz = LD(st["scal"][SC["RZ"]])
    kap = macc / abs(acc) if acc != 0 else LD(1)
    be = acc / rz
    M = st["M"]
    return {"RZ": (acc, macc, M + 2), "pcg": (z + be * p, np.abs(z) + kap * np.abs(be * p), M + 6), "kappa": float(kap)}


def tw_dir(st, D, dev):
    """Newton direction from dy and tN = Ah' dy (oracle: IPM.run, solve); dmuL / dmuU / dmus / dg from the device's own dp / ds / dpi."""
    fr, ineq = _free(st), st["rtype"] != 0
    thp, hp, tN, rcL, rcU, muL, muU, tL, tU = _l(st, "thp_inv", "hp", "tN", "rcL", "rcU", "muL", "muU", "tL", "tU")
    out = {D + ".dp": (thp * (hp + tN), np.abs(thp) * (np.abs(hp) + np.abs(tN)), 3)}
    dp = dev[D + ".dp"].astype(LD)
    out[D + ".dmuL"] = (np.where(fr, (rcL - muL * dp) / tL, 0), np.where(fr, (np.abs(rcL) + np.abs(muL * dp)) / np.abs(tL), 0), 4)
    out[D + ".dmuU"] = (np.where(fr, (rcU + muU * dp) / tU, 0), np.where(fr, (np.abs(rcU) + np.abs(muU * dp)) / np.abs(tU), 0), 4)
    ths, hs, sc, rcs, mus, ts = _l(st, "ths_inv", "hs", "scoef", "rcs", "mus", "ts")
    dys = st[D + ".dy"].astype(LD)[st["srow"]]
    out[D + ".ds"] = (ths * (hs + sc * dys), np.abs(ths) * (np.abs(hs) + np.abs(sc * dys)), 4)
    ds = dev[D + ".ds"].astype(LD)
    out[D + ".dmus"] = ((rcs - mus * ds) / ts, (np.abs(rcs) + np.abs(mus * ds)) / np.abs(ts), 4)
    rcg, g, pi = _l(st, "rcg", "g", "pi")
    dpi = dev[D + ".dpi"].astype(LD)
    with np.errstate(all="ignore"):
        out[D + ".dg"] = (np.where(ineq, (rcg - g * dpi) / np.where(ineq, pi, 1), 0), np.where(ineq, (np.abs(rcg) + np.abs(g * dpi)) / np.where(ineq, np.abs(pi), 1), 0), 4)
    return out


def ipm_dir_exact(st, D):
    """dpi = sg dy on inequality rows (exact: sg = +-1), 0 on equality rows."""
    return {D + ".dpi": np.where(st["rtype"] != 0, st["rtype"] * st[D + ".dy"], 0.0)}


def ipm_ratio_candidates(st, D):
    """Every eligible (ratio, where) of the ratio test as float64: -x / dx where dx < 0, one correctly rounded division each."""
    fr, ineq = _free(st), st["rtype"] != 0

    def cand(x, dx, mask):
        sel = mask & (dx < 0)
        with np.errstate(all="ignore"):
            return np.where(sel, -x / np.where(sel, dx, -1.0), BIG)
    dp = st[D + ".dp"]
    allk = np.ones(st["ns"], bool)
    prim = {"tL": cand(st["tL"], dp, fr), "tU": cand(st["tU"], -dp, fr), "ts": cand(st["ts"], st[D + ".ds"], allk), "g": cand(st["g"], st[D + ".dg"], ineq)}
    dual = {"muL": cand(st["muL"], st[D + ".dmuL"], fr), "muU": cand(st["muU"], st[D + ".dmuU"], fr), "mus": cand(st["mus"], st[D + ".dmus"], allk),
            "pi": cand(st["pi"], st[D + ".dpi"], ineq)}
    return prim, dual


def ipm_steps_exact(st, D):
    """AP, AD (oracle: IPM.run, steps / _maxstep): minima of the eligible ratios, capped at 1."""
    prim, dual = ipm_ratio_candidates(st, D)
    return {"AP": min(1.0, min(float(v.min(initial=BIG)) for v in prim.values())), "AD": min(1.0, min(float(v.min(initial=BIG)) for v in dual.values()))}


def tw_muaff(st, D, sexp):
    """The accumulator  sum (t + ap dt)(m + ad dm)  over the complementarity pairs (five operations per product, one per addition; k = number
    of products + 7 with the division by ncomp), and SM = (mu_aff / mu)^sexp mu (0 when mu is 0).  SM takes the accumulator to the power
    sexp:  |(a + e)^p - a^p| <= p max(|a|, |a + e|)^(p-1) |e|, so with the magnitude in place of a and (1 + gamma_k)^p <= 1 + gamma_(p k) the
    bound is gamma_(sexp (k + 3)) magnitude^sexp / mu^(sexp-1)."""
    fr, ineq = _free(st), st["rtype"] != 0
    ap, ad = LD(st["scal"][SC["AP"]]), LD(st["scal"][SC["AD"]])
    tL, tU, muL, muU, ts, mus, g, pi = _l(st, "tL", "tU", "muL", "muU", "ts", "mus", "g", "pi")
    dp, dmuL, dmuU, ds, dmus, dg, dpi = _l(st, D + ".dp", D + ".dmuL", D + ".dmuU", D + ".ds", D + ".dmus", D + ".dg", D + ".dpi")

    def prod(x, dx, z, dz, sel):
        return ((x + ap * dx) * (z + ad * dz))[sel], ((np.abs(x) + ap * np.abs(dx)) * (np.abs(z) + ad * np.abs(dz)))[sel]
    parts = [prod(tL, dp, muL, dmuL, fr), prod(tU, -dp, muU, dmuU, fr), prod(ts, ds, mus, dmus, np.ones(st["ns"], bool)), prod(g, dg, pi, dpi, ineq)]
    acc = sum(p_[0].sum() for p_ in parts)
    macc = sum(p_[1].sum() for p_ in parts)
    cnt = sum(len(p_[0]) for p_ in parts)
    nc, mu = LD(st["ncomp"]), LD(st["scal"][SC["MU"]])
    k = cnt + 7
    if not mu > 0:
        return {"acc": (acc, macc, k), "SM": (LD(0), LD(0), 1)}
    r, mr = acc / nc / mu, macc / nc / mu
    return {"acc": (acc, macc, k), "SM": (r ** sexp * mu, mr ** sexp * mu, sexp * (k + 3))}


def ipm_sm_exact(acc, ncomp, mu, sexp):
    """SM in float64 from the accumulator the device summed (a multi-workgroup launch leaves its partials in rpart)."""
    mu_aff = acc / float(ncomp)
    r = mu_aff / mu if mu > 0.0 else 0.0
    return (r * r if sexp == 2 else (r * r * r * r if sexp == 4 else r * r * r)) * mu


def tw_update(st, C, al, be, dev):
    """iterate += (al, be) direction (oracle: IPM.run, last block); y of an inequality row is sg times the pi the device wrote (exact)."""
    fr, ineq = _free(st), st["rtype"] != 0
    al, be = LD(al), LD(be)
    out = {}

    def axpy(nm, a, d, sign=1):
        x, dx = _l(st, nm, C + "." + d)
        out[nm] = (x + sign * a * dx, np.abs(x) + np.abs(a * dx), 3)
    axpy("p", al, "dp"); axpy("tL", al, "dp"); axpy("tU", al, "dp", -1); axpy("muL", be, "dmuL"); axpy("muU", be, "dmuU")
    axpy("s", al, "ds"); axpy("ts", al, "ds"); axpy("mus", be, "dmus"); axpy("g", al, "dg"); axpy("pi", be, "dpi")
    y, dy = _l(st, "y", C + ".dy")
    out["y"] = (np.where(ineq, st["rtype"] * dev["pi"].astype(LD), y + be * dy), np.where(ineq, np.abs(dev["pi"].astype(LD)), np.abs(y) + np.abs(be * dy)), 3)
    for nm in ("tL", "tU"):
        out[nm] = (np.where(fr, out[nm][0], 1), np.where(fr, out[nm][1], 1), 3)
    out["g"] = (np.where(ineq, out["g"][0], 1), np.where(ineq, out["g"][1], 1), 3)
    return out


def ipm_init_exact(st, origin, mu_factor):
    """k_ipm_init_p then k_ipm_init_rest in float64 (oracle: IPM.__init__).  Single correctly rounded operations throughout: the slack
    coefficients are +-1, so the products of the slack sum are exact and a fused multiply-add rounds as the plain addition does."""
    lb, ub = st["lb"], st["ub"]
    p = 0.5 * (lb + ub)
    if origin:
        w4 = 0.25 * (ub - lb)
        p = np.minimum(np.maximum(0.0, lb + w4), ub - w4)
    s = st["slo"] + 1.0
    return {"p": p, "s": s}


def ipm_init_rest_exact(st, mu_factor):
    fr, ineq, sg = _free(st), st["rtype"] != 0, st["rtype"].astype(float)
    mu0 = mu_factor * st["scale_q"]
    with np.errstate(all="ignore"):
        tl = np.where(fr, st["p"] - st["lb"], 1.0)
        tu = np.where(fr, st["ub"] - st["p"], 1.0)
        out = {"tL": tl, "tU": tu, "muL": np.where(fr, mu0 / tl, 0.0), "muU": np.where(fr, mu0 / tu, 0.0)}
        ts = st["s"] - st["slo"]
        out["ts"], out["mus"] = ts, mu0 / ts
        a = st["act"].copy()
        if st["ns"]:
            sl = np.zeros(st["M"])
            for rs in (st["rs0"], st["rs1"]):
                has = rs >= 0
                sl[has] = sl[has] + st["scoef"][rs[has]] * st["s"][rs[has]]
            a = a + sl
        g = np.where(ineq, np.maximum(sg * (a - st["r"]), 1.0), 1.0)
        pi = np.where(ineq, mu0 / g, 0.0)
    out["g"], out["pi"], out["y"] = g, pi, sg * pi
    return out


def ipm_col_prep_exact(st, rho_p, fixed):
    fr = _free(st)
    with np.errstate(all="ignore"):
        return 1.0 / st["dS"], np.where(fr, st["muL"] / st["tL"] + st["muU"] / st["tU"] + rho_p, fixed)


def tw_col_finish(dinv, u, w):
    dinv, u, w = dinv.astype(LD), u.astype(LD), w.astype(LD)
    return u - dinv * w, np.abs(u) + np.abs(dinv * w), 3


def tw_sdiag_csr(ptr, col, vals, thinv):
    """out_i = sum_k vals_k^2 thinv[col_k] as a running fused sum: each term passes the rounding of its square and at most cnt roundings of
    the sum (the product with thinv is inside the fused operation), so k = terms + 2."""
    R = len(ptr) - 1
    v, cnt = np.zeros(R, LD), np.diff(ptr)
    t = vals.astype(LD) ** 2 * thinv.astype(LD)[col]
    row = np.repeat(np.arange(R), cnt)
    np.add.at(v, row, t)
    m = np.zeros(R, LD)
    np.add.at(m, row, np.abs(t))
    return v, m, cnt + 2


# (n, M, ns): every length of {0 (ns, M), 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 12289, 70001, 262144, 262149}
# appears, each of the three ranges is the longest somewhere; expected workgroups of the reductions = min(64, ceil(max / 4096)).
# M = 0 is a bounds-only LP, which asm_sublp_setup accepts (m >= 0).
IPM_CASES = [
    (1, 1, 0), (256, 0, 0), (64, 63, 65), (255, 257, 256), (1025, 1023, 1024), (4096, 4095, 0), (4095, 4096, 4097), (4097, 1024, 63),
    (8191, 12289, 4096), (70001, 65, 1), (262144, 1025, 255), (1023, 262149, 70001), (4097, 262144, 262149),
]


def ipm_red_grid(n, M, ns):
    return min(64, max(1, (max(n, M, ns) + 4095) // 4096))


def ipm_grid_all(n, M, ns):
    return (max(n, M, ns, 1) + 255) // 256


def ipm_decoys(st, D):
    """Entries the ratio test (and the measures) must ignore, written into the state: a fixed column whose ratios would be the smallest of all
    (1e-30), an equality row with negative dg and dpi and the same tiny ratios, and free columns with dp = 0.0 and dp = -0.0 on tiny
    slacks (neither sign of zero is a negative component)."""
    n, M = st["n"], st["M"]
    if n >= 4:
        j = n // 2
        st["ub"][j] = st["lb"][j]
        st["tL"][j] = st["tU"][j] = st["muL"][j] = st["muU"][j] = 1e-30
        st[D + ".dp"][j] = -1.0
        st[D + ".dmuL"][j] = st[D + ".dmuU"][j] = -1.0
        for jz, z in ((0, 0.0), (n - 1, -0.0)):
            st["ub"][jz] = st["lb"][jz] + 1.0
            st["tL"][jz] = st["tU"][jz] = 1e-30
            st["muL"][jz] = st["muU"][jz] = 1.0
            st[D + ".dp"][jz] = z
    if M >= 2:
        i = M // 2
        st["rtype"][i] = 0
        st["g"][i] = st["pi"][i] = 1e-30
        st[D + ".dg"][i] = st[D + ".dpi"][i] = -1.0
    fr, eq = st["ub"] > st["lb"], st["rtype"] == 0
    st["ncomp"] = max(2 * int(fr.sum()) + st["ns"] + int((~eq).sum()), 1)


def ipm_plant(base, D, rg, pos, ratios=None):
    """A copy of the state with a binding primal and a binding dual ratio at entry `pos` of range rg ('n': tL and muL of a free column, 'M': g
    and pi of an inequality row, 's': ts and mus): half the smallest eligible ratio of the state (or `ratios`), made of x = ratio, dx = -1 so
    that the quotient is exact.  Returns (state, ap, ad); asserts that the planted minimum is below 1 and unique by more than one ulp."""
    st = dict(base)
    for nm in ("ub", "lb", "rtype", "tL", "muL", "g", "pi", "ts", "mus", D + ".dp", D + ".dmuL", D + ".dg", D + ".dpi", D + ".ds", D + ".dmus", "tU", "muU", D + ".dmuU"):
        st[nm] = base[nm].copy()
    prim, dual = ipm_ratio_candidates(base, D)
    if ratios is None:
        ap = 0.5 * min(1.0, min(float(v.min(initial=BIG)) for v in prim.values()))
        ad = 0.5 * min(1.0, min(float(v.min(initial=BIG)) for v in dual.values()))
    else:
        ap, ad = ratios
    if rg == "n":
        if not st["ub"][pos] > st["lb"][pos]:
            st["ub"][pos] = st["lb"][pos] + 1.0
        st["tL"][pos], st[D + ".dp"][pos], st["tU"][pos] = ap, -1.0, 1.0
        st["muL"][pos], st[D + ".dmuL"][pos] = ad, -1.0
        st["muU"][pos], st[D + ".dmuU"][pos] = 1.0, 1.0
    elif rg == "M":
        if st["rtype"][pos] == 0:
            st["rtype"][pos] = 1
        st["g"][pos], st[D + ".dg"][pos], st["pi"][pos], st[D + ".dpi"][pos] = ap, -1.0, ad, -1.0
    else:
        st["ts"][pos], st[D + ".ds"][pos], st["mus"][pos], st[D + ".dmus"][pos] = ap, -1.0, ad, -1.0
    fr, eq = st["ub"] > st["lb"], st["rtype"] == 0
    st["ncomp"] = max(2 * int(fr.sum()) + st["ns"] + int((~eq).sum()), 1)
    if ratios is None:
        for cands, a in (ipm_ratio_candidates(st, D)[0], ap), (ipm_ratio_candidates(st, D)[1], ad):
            allc = np.sort(np.concatenate(list(cands.values())))
            assert allc[0] == a and a < 1.0 and (len(allc) == 1 or allc[1] > np.nextafter(a, np.inf)), "planted minimum is not unique"
    return st, ap, ad


def ipm_planted_positions(st):
    """(range, position) of every planted minimum of a case: first and last entry, the ends of the first wavefront, the last entry of a partial
    wavefront, the first entry of a workgroup's second sweep, the last entry of the last workgroup's share, and - in the longest range - entries
    beyond the end of each shorter range, where the clamped index re-reads that range's last element."""
    L = {"n": st["n"], "M": st["M"], "s": st["ns"]}
    gr = ipm_red_grid(st["n"], st["M"], st["ns"])
    out = []
    for rg, ln in L.items():
        if ln == 0:
            continue
        pos = {0, ln - 1, min(63, ln - 1), min(64, ln - 1), (ln - 1) // 64 * 64, gr * 1024}
        last_wg = [t for t in range(max(0, ln - gr * 1024 - 1024), ln) if (t // 1024) % gr == gr - 1]
        if last_wg:
            pos.add(last_wg[-1])
        for other in L.values():
            pos.update({other, other + 1, other + 70})
        out += [(rg, p) for p in sorted(pos) if 0 <= p < ln]
    return out


def ipm_decoy_state(case, mus):
    """State of the ratio-test cases: the decoys that must be ignored are in place (ipm_plant adds the binding entry)."""
    st = ipm_state(700 + case, *IPM_CASES[case], mu=mus[(case + 3) % len(mus)])
    ipm_decoys(st, "A")
    return st


IPM_MUS = [1e2, 1.0, 1e-2, 1e-4, 1e-6, 1e-8, 1e-10, 1e-12]      # complementarity levels the solver passes through, dealt to the cases


# ---- the twin's stages chained into interior-point iterations (tests/test_ipm_stages_cpu.py): NumPy products with the matrix, the oracle's own
# Cholesky factor as preconditioner, every stage the float64 rounding of the twin's long-double value
def _f(tw, st, names=None):
    for nm in (names or [k for k in tw if isinstance(tw[k], tuple)]):
        if nm in SC:
            st["scal"][SC[nm]] = float(tw[nm][0])
        elif nm in st:
            st[nm] = np.asarray(tw[nm][0], np.float64)


def ipm_twin_start(lp):
    """Start point of oracle IPM.__init__ through ipm_init_exact / ipm_init_rest_exact."""
    from oracle import lp_solver as O
    n, M, ns = lp.n, lp.M, lp.ns
    st = {"n": n, "M": M, "ns": ns, "rtype": lp.rtype.astype(np.int32), "srow": lp.srow.astype(np.int32)}
    st["rs0"], st["rs1"] = ipm_slack_lists(M, st["srow"])
    for nm in IPM_N + IPM_M + IPM_S:
        st[nm] = np.zeros(ipm_vec_len(st, nm))
    for nm in ("q", "lb", "ub", "r", "w", "slo", "scoef"):
        st[nm] = getattr(lp, nm).copy()
    st["scale_q"] = max(1.0, np.abs(lp.q).max(initial=0.0), np.abs(lp.w).max(initial=0.0))
    fr, ineq = lp.ub > lp.lb, lp.rtype != 0
    st["ncomp"] = max(2 * int(fr.sum()) + ns + int(ineq.sum()), 1)
    st["scal"] = np.zeros(len(IPM_SCALARS))
    st.update(ipm_init_exact(st, 1 if ns == 0 else 0, 1.0))
    st["act"] = lp.A @ st["p"]
    st.update(ipm_init_rest_exact(st, O.IPM_MU0_NORMAL if ns == 0 else 1.0))
    return st


def ipm_twin_iteration(lp, st):
    """One iteration of oracle IPM.run in row form from the twin's stages.  Returns (pinf, dinf, mu, ap, ad) of the iteration."""
    from oracle import lp_solver as O
    A, M = lp.A, lp.M
    st["act"], st["aty"] = A @ st["p"], A.T @ st["y"]
    tw = tw_measures(st)
    _f(tw, st, ["rp", "rdp", "rds", "MU"])
    for nm, v in ipm_measures_exact(st, st["rp"], st["rdp"], st["rds"]).items():
        st["scal"][SC[nm]] = v
    pinf, dinf, mu, rpmax = st["scal"][SC["PINF"]], st["scal"][SC["DINF"]], st["scal"][SC["MU"]], st["scal"][SC["RPMAX"]]
    st.update(ipm_theta_exact(st, IPM_RHO_P))
    S = O.dsyrk(1.0, A * np.sqrt(st["thp_inv"]), lower=True)
    idx = np.arange(M)
    S[idx, idx] += st["dS"]
    d0 = S[idx, idx].copy()
    S[idx, idx] += 1e-13 * d0 + 1e-30
    L = O.chol_guard(S, d0)
    applyS = lambda v: A @ (st["thp_inv"] * (A.T @ v))      # (k_vec_mul between the two products)

    def solve(mode, base, D, tp=0.0, td=0.0):
        _f(tw_rhs1(st, base, mode, tp, td), st, ["rcL", "rcU", "rcs", "rcg"])
        t2 = tw_rhs1(st, base, mode, tp, td, dev=dict(st, hp=st["hp"]))
        _f(t2, st, ["hp", "hs"])
        _f(tw_rhs1(st, base, mode, tp, td, dev=st), st, ["tmpn"])
        st["t1"] = A @ st["tmpn"]
        _f(tw_rhs2(st, 0.0 if mode == 2 else 1.0), st)
        st[D + ".dy"] = O.chol_solve(L, st["rhs"])
        st["sres"] = applyS(st[D + ".dy"])
        _f(tw_res(st, D), st)
        ex = ipm_res_exact(st, st["res"], 0, 0.0, 0.0)
        tol = max(O.PCG_FLOOR * ex["RMAX"], O.PCG_KAPPA * rpmax)
        if ex["EMAX"] > tol:
            st["corr"] = O.chol_solve(L, st["res"])
            st["pcg"] = st["corr"].copy()
            st["scal"][SC["RZ"]] = st["scal"][SC["RZ0"]] = float(tw_pcg_start(st)["RZ"][0])
            for _ in range(O.PCG_MAXIT):
                st["sres"] = applyS(st["pcg"])
                t1 = tw_pcg_step1(st, D)
                if not t1["ok"]:
                    break
                st[D + ".dy"], st["res"] = np.asarray(t1["x"][0], np.float64), np.asarray(t1["res"][0], np.float64)
                if np.abs(st["res"]).max(initial=0.0) <= tol:
                    break
                st["corr"] = O.chol_solve(L, st["res"])
                t2_ = tw_pcg_step2(st)
                st["pcg"], st["scal"][SC["RZ"]] = np.asarray(t2_["pcg"][0], np.float64), float(t2_["RZ"][0])
        st["tN"] = A.T @ st[D + ".dy"]
        st.update(ipm_dir_exact(st, D))
        own = [D + "." + c for c in ("dp", "ds")]
        _f(tw_dir(st, D, st), st, own)
        _f(tw_dir(st, D, st), st, [D + "." + c for c in ("dmuL", "dmuU", "dmus", "dg")])

    def steps(D):
        e = ipm_steps_exact(st, D)
        st["scal"][SC["AP"]], st["scal"][SC["AD"]] = e["AP"], e["AD"]
        return e["AP"], e["AD"]
    solve(0, "A", "A")
    steps("A")
    _f(tw_muaff(st, "A", 3), st, ["SM"])
    solve(1, "A", "C")
    ap, ad = steps("C")
    a_, c_ = "A", "C"
    for _ in range(O.IPM_MCC):
        if min(ap, ad) >= 0.9:
            break
        solve(2, c_, a_, min(1.0, ap + O.MCC_DELTA), min(1.0, ad + O.MCC_DELTA))
        for c in ("dp", "ds", "dg", "dy", "dmuL", "dmuU", "dmus", "dpi"):
            st[a_ + "." + c] = st[a_ + "." + c] + st[c_ + "." + c]
        ap2, ad2 = steps(a_)
        if not (ap2 >= ap and ad2 >= ad and ap2 + ad2 >= ap + ad + O.MCC_GAMMA * O.MCC_DELTA):
            break
        a_, c_ = c_, a_
        ap, ad = ap2, ad2
    eta = 0.995 if mu >= 1.0 else min(max(0.995, 1.0 - mu / st["scale_q"]), 0.999999)
    al, be = min(1.0, eta * ap), min(1.0, eta * ad)
    new_pi = np.asarray(tw_update(st, c_, al, be, {"pi": st["pi"]})["pi"][0], np.float64)
    _f(tw_update(st, c_, al, be, {"pi": new_pi}), st)
    return pinf, dinf, mu, ap, ad


def ipm_stage_state(case):
    """The state every stage is run from alone (tests/test_ipm_stages_gpu.py; its twin magnitudes are checked in tests/test_ipm_stages_cpu.py):
    ipm_state with the decoy of k_ipm_measures - a fixed column with a huge dual residual - and a CG state with positive curvature and a
    modest condition number of its dot products (tw_pcg_step1, tw_pcg_step2: kappa)."""
    st = ipm_state(500 + case, *IPM_CASES[case], mu=IPM_MUS[case % len(IPM_MUS)])
    fx = np.flatnonzero(st["ub"] == st["lb"])
    if len(fx):
        st["q"][fx[0]] = 1e250
    rng = np.random.default_rng(900 + case)
    st["sres"] = 0.5 * st["pcg"] + 0.2 * rng.standard_normal(st["M"])
    st["corr"] = 0.5 * st["res"] + 0.2 * rng.standard_normal(st["M"])
    st["scal"][SC["RZ"]], st["scal"][SC["RZ0"]] = 0.7, 2.1
    return st


def ipm_helper_operands(case, st):
    """Operands of the column-form and reduced-row helper stages for a state: r, w (M) of the column form; kept rows E (a non-monotone
    list) and dropped rows I with their diagonal dI, ze (|E|), and CSR rows (ptr, col, vals) with 0 .. 9 entries, row 0 empty."""
    n, M = st["n"], st["M"]
    rng = np.random.default_rng(77 + case)
    op = {"r": rng.standard_normal(M), "w": rng.standard_normal(M)}
    if M > 0:
        perm = rng.permutation(M).astype(np.int32)
        nE = M - M // 3
        op["E"], op["I"] = perm[:nE], perm[nE:]
        cnt = rng.integers(0, 10, M)
        cnt[0] = 0
        op["ptr"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        nnz = int(op["ptr"][-1])
        op["col"] = rng.integers(0, n, nnz).astype(np.int32)
        op["ze"], op["dI"], op["vals"] = rng.standard_normal(nE), 10.0 ** rng.uniform(-3, 3, M - nE), rng.standard_normal(nnz)
    return op


# ------------------------------------------------------------------------------------------------------------------------------------------
# Twins of the active-set and optimal-face kernels (asm_as_kernels.hip.h), written from the kernels' statement lists.  A state is a dict with
# the sizes, scale_q, one float64 vector per name of AS_VECTORS and one int32 vector per name of AS_IVECTORS (true lengths), `cnt` (AC_*) and
# `scal` (AS_*).  A twin returns (exact, bounded): `exact` maps a vector name / "cnt.X" / "scal.X" to what the kernel must leave there bit for
# bit - whole vectors, so entries the kernel does not write carry their input; vectors longer than the true length state the padding the
# kernel owns - and `bounded` maps a name to (value, magnitude, k) in long double as for the interior-point twins.  Decisions are taken in long
# double from the inputs; as_cmp files each one as clear (at least 64 rounding bounds away from its threshold), tie (exactly on it) or between,
# and counts the branch it took in the census.  A maximum of rounded terms is stated as (max of the values, max of the magnitudes, k): the
# maximum is 1-Lipschitz, so the bound on the terms carries over.
AS_KINDS = ("identify", "clip0", "sl", "sl_values", "smax", "setup", "rhs", "res_p", "scatter_h", "add_f", "rd", "gather_h", "add_yh", "merge", "finish",
            "primal_finish", "ns_combine", "ns_step", "ns_col", "ns_z", "ns_unmark", "dual_finish", "kkt", "pack", "copy_sets")
AS_VECTORS = ("Fmask p z pB pF cF rd tN xfull nu Hmask sl y act t bH v u yH yfull uacc ax s pref zero p0 z0 pa pf zf y0 act0 acta actf yf s0 sa sf "
              "q lb ub r w slo scoef ip.p ip.tL ip.tU ip.muL ip.muU ip.g ip.pi ip.y ip.ts ip.mus ip.s").split()
AS_IVECTORS = ["S%d.%s" % (k, nm) for k in range(6) for nm in ("rowst", "bst", "sst")] + "ksoft Hidx hpos Fidx fpos rtype rs0 rs1 srow rperm".split()
AS_N = "Fmask p z pB pF cF rd tN xfull nu pref zero p0 z0 pa pf zf q lb ub ip.p ip.tL ip.tU ip.muL ip.muU S.bst Fidx fpos".split()
AS_M = "Hmask sl y act t bH v u yH yfull uacc ax y0 act0 acta actf yf r ip.g ip.pi ip.y S.rowst ksoft Hidx hpos rtype rs0 rs1 rperm".split()
AC = {nm: i for i, nm in enumerate("NH NF ANYSOFT NCHG NDIFF NVIOL NREL".split())}
AS = {nm: i for i, nm in enumerate("PR DU EQRES HARDRES".split())}
TOL_P, TOL_D, FACE_TOL_M = 1e-9, 1e-6, 1e-9
ISENT = -77               # pre-fill of every int output
# branches of every kernel's decision tree (the census must count each at least once over AS_CASES x seeds)
AS_BRANCHES = {
    "identify": "fixed lower upper both free slack_basic slack_bound row_eq row_active row_inactive row_forced_rs0 row_forced_rs1".split(),
    "setup": "soft_rs0 soft_rs1 hard inactive active_soft free at_lower at_upper any_soft no_soft pref_null pref_given rperm_on rperm_off".split(),
    "finish": ("row_soft row_eq row_drop row_add row_keep col_fixed col_release_lo col_release_up col_fix_lo col_fix_up col_keep slack_free slack_low "
               "slack_keep row_reactivated have_prev no_prev").split(),
    "primal_finish": ("grow release unchanged check_only viol_row viol_lo viol_up viol_slack grow_row grow_lo grow_up grow_slack rel_row rel_slack "
                      "rel_lo rel_up rel_mandatory_kept row_reactivated").split(),
    # (a ratio a / (a - g1) with g1 < 0 is below 1: the kernel's fmin(alpha, 1.0) never binds, so it is no branch of the census)
    "ns_step": "feasible blocked fam_row fam_slack fam_lower fam_upper alpha_below_1 nonbasic_reset".split(),
    "ns_col": "fam_row fam_slack fam_lower fam_upper".split(),
    "ns_unmark": "fam_row fam_slack fam_lower fam_upper".split(),
    "dual_finish": "col_lo col_up col_keep row_drop row_keep slack_basic slack_keep row_reactivated none".split(),
    "kkt": "row_eq row_ge row_le row_inactive col_fixed col_lo col_up col_free slack_basic slack_bound".split(),
    "clip0": "src_null src_given below above inside".split(),
    "scatter_h": "hard other accumulate plain".split(),
    "merge": "with_y without_y".split(),
    "rhs": "soft no_soft yref_null yref_given free bound".split(),
}


def as_len(st, nm):
    if nm.startswith("S") and "." in nm and nm[1].isdigit():
        nm = "S." + nm.split(".")[1]
    return st["n"] if nm in AS_N else (st["M"] if nm in AS_M else st["ns"])


def as_new_census():
    return {k: {b: 0 for b in v} for k, v in AS_BRANCHES.items()}


class AsBook:
    """Census of branches and classes of decisions of one or more twin runs."""

    def __init__(self):
        self.census = as_new_census()
        self.cls = {"clear": 0, "tie": 0, "between": 0}

    def hit(self, kernel, branch, cnt=1):
        self.census[kernel][branch] += int(cnt)

    def cmp(self, val, mag, k, op, thr, mask=None):
        """val `op` thr, element by element in long double, filing each entry of `mask`."""
        val, mag, thr = np.asarray(val, LD), np.asarray(mag, LD), np.asarray(thr, LD)
        val, mag, thr = np.broadcast_arrays(val, mag, thr)
        res = {"<": val < thr, "<=": val <= thr, ">": val > thr, ">=": val >= thr}[op]
        m = np.ones(val.shape, bool) if mask is None else mask
        tie = (val == thr) & m
        near = (np.abs(val - thr) < 64 * gamma(k) * mag) & ~tie & m
        self.cls["tie"] += int(tie.sum())
        self.cls["between"] += int(near.sum())
        self.cls["clear"] += int(m.sum() - tie.sum() - near.sum())
        return res


def as_slack_lists(M, srow):
    return ipm_slack_lists(M, srow)


def _near(rng, cnt, frac=0.35):
    """Factors that put a decision quantity near its threshold: a third of the entries at 0.2 .. 5 thresholds of either sign, the rest far."""
    c = np.where(rng.random(cnt) < 0.5, 1.0, -1.0) * rng.uniform(0.2, 5.0, cnt)
    return np.where(rng.random(cnt) < frac, c, np.nan)


def as_state(seed, n, M, ns, scale_q=4.0):
    """A scrambled active-set state: LP vectors with fixed columns, all three row types, both signs of scoef, rows with two, one and no slack
    column; an interior-point iterate; six working sets; work vectors of O(1) entries; index lists of a consistent earlier k_as_setup on set 0.
    About a third of the quantities that a kernel compares with a tolerance sit at 0.2 .. 5 times that tolerance (through t, p, y, tN, uacc, nu),
    the others at O(1).  Nothing is re-drawn: a factor of 0.2 .. 5 leaves a distance of at least 0.2 tolerances (2e-10), six orders above 64
    rounding bounds of O(1) data, so no entry can land between the classes - which the tests assert on every state they use."""
    rng = np.random.default_rng(seed)
    assert n >= 1 and 0 <= ns <= 2 * M
    st = {"n": n, "M": M, "ns": ns, "scale_q": scale_q}
    st["rtype"] = rng.integers(-1, 2, M).astype(np.int32)
    npair = max(ns - M, ns // 3) if ns >= 2 else 0
    rows = rng.permutation(M)[:ns - npair]
    st["srow"] = np.sort(np.concatenate([rows, rows[:npair]])).astype(np.int32)
    st["rs0"], st["rs1"] = ipm_slack_lists(M, st["srow"])
    st["rperm"] = rng.permutation(M).astype(np.int32)
    for nm in AS_VECTORS:
        st[nm] = np.round(rng.standard_normal(as_len(st, nm)) * 2.0 ** 20) / 2.0 ** 20
    st["scoef"] = np.where(rng.random(ns) < 0.5, 1.0, -1.0) * rng.choice([0.5, 1.0, 2.0], ns)
    st["lb"] = -rng.uniform(0.1, 3.0, n)
    st["ub"] = rng.uniform(0.1, 3.0, n)
    fx = rng.random(n) < 0.1
    st["ub"][fx] = st["lb"][fx]
    for a, b, cnt in (("ip.tL", "ip.muL", n), ("ip.tU", "ip.muU", n), ("ip.ts", "ip.mus", ns), ("ip.g", "ip.pi", M)):
        st[a] = 10.0 ** rng.uniform(-6, 2, cnt)
        st[b] = 1e-3 / st[a] * 10.0 ** rng.uniform(-1, 1, cnt)
    for k in range(6):
        st["S%d.rowst" % k] = rng.integers(0, 2, M).astype(np.int32)
        st["S%d.bst" % k] = rng.integers(-1, 2, n).astype(np.int32)
        st["S%d.sst" % k] = rng.integers(0, 2, ns).astype(np.int32)
        st["S%d.rowst" % k][st["srow"][st["S%d.sst" % k] == 1]] = 1            # (a basic slack makes its row active: every set the solver holds)
    st["cnt"] = np.full(len(AC), ISENT, np.int32)
    st["scal"] = np.full(len(AS), SENTINEL)
    for nm in "ksoft Hidx hpos Fidx fpos".split():
        st[nm] = np.full(as_len(st, nm), ISENT, np.int32)
    ex, _ = tw_as_setup(st, 0, None, 0, AsBook())                              # lists of set 0, natural order
    for nm in "ksoft Hidx hpos Fidx fpos Fmask Hmask".split():
        st[nm] = ex[nm][:as_len(st, nm)].copy()
    st["cnt"][:3] = [ex["cnt.NH"], ex["cnt.NF"], ex["cnt.ANYSOFT"]]
    # quantities near their tolerances
    den = 1.0 + np.abs(st["r"])
    c = _near(rng, M)
    hit = ~np.isnan(c) & (st["ksoft"] < 0)
    st["t"][hit] = (st["r"] - st["rtype"] * c * TOL_P * den - _as_sl(st))[hit]           # rt (r - act) / den = c tol_p
    c = _near(rng, M)
    hit = ~np.isnan(c)
    st["y"][hit] = (c * TOL_D * scale_q)[hit]
    st["uacc"][hit] = (c * FACE_TOL_M)[hit]
    st["sl"] = _as_sl(st).astype(np.float64)
    c = _near(rng, n)
    hit = ~np.isnan(c)
    st["tN"][hit] = (st["q"] - c * TOL_D * scale_q)[hit]                                  # z = c td
    c = _near(rng, n)
    lo = ~np.isnan(c) & (rng.random(n) < 0.5)
    up = ~np.isnan(c) & ~lo
    st["p"][lo] = (st["lb"] - c * TOL_P)[lo]
    st["p"][up] = (st["ub"] + c * TOL_P)[up]
    c = _near(rng, n)
    hit = ~np.isnan(c)
    st["nu"][hit] = (c * FACE_TOL_M)[hit]
    st["pa"] = st["lb"] + (st["ub"] - st["lb"]) * rng.uniform(0.1, 0.9, n)                # a feasible anchor
    st["sa"] = st["slo"] + rng.uniform(0.1, 2.0, ns)
    st["acta"] = st["r"] + st["rtype"] * rng.uniform(0.1, 2.0, M)
    return st


def _as_sl(st):
    a, _, _ = _slack_sum(st, st["slo"])
    return a.astype(np.float64)                   # at most two terms: tw_as_sl states the bound


def _sets(st, k):
    return st["S%d.rowst" % k], st["S%d.bst" % k], st["S%d.sst" % k]


def tw_as_identify(st, dst, bk):
    sq = LD(st["scale_q"])
    lb, ub, tL, tU, muL, muU, ts, mus, slo, g, pi, r = _l(st, "lb", "ub", "ip.tL", "ip.tU", "ip.muL", "ip.muU", "ip.ts", "ip.mus", "slo", "ip.g", "ip.pi", "r")
    free = st["ub"] > st["lb"]
    width = np.where(free, ub - lb, LD(1))
    # a / b < c / d with b, d > 0: compared as a d - c b against 0 would change the rounding; the kernel divides, so the twin states both
    # quotients (k = 3: width, quotient) and compares their difference with 0
    lo = bk.cmp(tL / width - muL / sq, np.abs(tL / width) + np.abs(muL / sq), 4, "<", 0, free)
    up = bk.cmp(tU / width - muU / sq, np.abs(tU / width) + np.abs(muU / sq), 4, "<", 0, free)
    bst = np.where(free, np.where(up, 1, np.where(lo, -1, 0)), -1).astype(np.int32)
    sd = 1 + np.abs(slo)
    sst = bk.cmp(ts / sd - mus / sq, np.abs(ts / sd) + np.abs(mus / sq), 4, ">=", 0).astype(np.int32)
    rd = 1 + np.abs(r)
    ineq = st["rtype"] != 0
    ra = bk.cmp(g / rd - pi / sq, np.abs(g / rd) + np.abs(pi / sq), 4, "<", 0, ineq)
    rowst = np.where(ineq, ra, True)
    f0 = np.zeros(st["M"], bool)
    f1 = np.zeros(st["M"], bool)
    if st["ns"]:
        h0, h1 = st["rs0"] >= 0, st["rs1"] >= 0
        f0[h0] = sst[st["rs0"][h0]] == 1
        f1[h1] = sst[st["rs1"][h1]] == 1
    for nm, c in (("fixed", (~free).sum()), ("lower", (free & lo & ~up).sum()), ("upper", (free & up & ~lo).sum()), ("both", (free & lo & up).sum()),
                  ("free", (free & ~lo & ~up).sum()), ("slack_basic", sst.sum()), ("slack_bound", (sst == 0).sum()), ("row_eq", (~ineq).sum()),
                  ("row_active", (ineq & ra).sum()), ("row_inactive", (ineq & ~ra & ~f0 & ~f1).sum()), ("row_forced_rs0", (~rowst & f0).sum()),
                  ("row_forced_rs1", (~rowst & ~f0 & f1).sum())):
        bk.hit("identify", nm, c)
    rowst = (rowst | f0 | f1).astype(np.int32)
    return {"S%d.rowst" % dst: rowst, "S%d.bst" % dst: bst, "S%d.sst" % dst: sst}, {}


def tw_as_clip0(st, src, out, bk):
    """src: name or None; out: name."""
    s = np.zeros(st["n"]) if src is None else st[src]
    bk.hit("clip0", "src_null" if src is None else "src_given")
    bk.hit("clip0", "below", (s < st["lb"]).sum()); bk.hit("clip0", "above", (s > st["ub"]).sum()); bk.hit("clip0", "inside", ((s >= st["lb"]) & (s <= st["ub"])).sum())
    return {out: np.minimum(np.maximum(s, st["lb"]), st["ub"])}, {}


def tw_as_sl(st, values=False):
    a, m, c = _slack_sum(st, st["s"] if values else st["slo"])
    ex = {"ksoft": np.full(st["M"], -1, np.int32)} if values else {}
    return ex, {"sl": (a, m, c + 1)}


def tw_as_smax(st, src, dst):
    return {dst: np.maximum(st[src], st["slo"])}, {}


def tw_as_setup(st, cur, p_ref, use_rperm, bk, ldn=None, ldT=None):
    n, M, ns = st["n"], st["M"], st["ns"]
    rowst, bst, sst = _sets(st, cur)
    ldn = n if ldn is None else ldn
    ldT = M if ldT is None else ldT
    ks = np.full(M, -1, np.int32)
    if ns:
        h0, h1 = st["rs0"] >= 0, st["rs1"] >= 0
        b0 = np.zeros(M, bool); b1 = np.zeros(M, bool)
        b0[h0] = sst[st["rs0"][h0]] == 1
        b1[h1] = sst[st["rs1"][h1]] == 1
        ks = np.where(b0, st["rs0"], np.where(b1, st["rs1"], -1)).astype(np.int32)
        bk.hit("setup", "soft_rs0", b0.sum()); bk.hit("setup", "soft_rs1", (~b0 & b1).sum())
    soft = ks >= 0
    y = np.where(soft, st["w"][np.maximum(ks, 0)] * st["scoef"][np.maximum(ks, 0)], 0.0) if ns else np.zeros(M)
    hard = (rowst == 1) & ~soft
    order = st["rperm"].astype(np.int64) if use_rperm else np.arange(M)
    Hidx = st["Hidx"].copy()
    hl = order[hard[order]]
    Hidx[:len(hl)] = hl
    hpos = np.full(M, -1, np.int32)
    hpos[hl] = np.arange(len(hl))
    Hmask = np.zeros(ldT)
    Hmask[:M] = hard
    fr = bst == 0
    Fidx = st["Fidx"].copy()
    fl = np.nonzero(fr)[0]
    Fidx[:len(fl)] = fl
    fpos = np.full(n, -1, np.int32)
    fpos[fl] = np.arange(len(fl))
    ref = np.zeros(n) if p_ref is None else st[p_ref]
    pj = np.where(bst < 0, st["lb"], np.where(bst > 0, st["ub"], ref))
    pad = lambda v: np.concatenate([v, np.zeros(ldn - n)])
    for nm, c in (("hard", hard.sum()), ("inactive", ((rowst != 1) & ~soft).sum()), ("active_soft", soft.sum()), ("free", fr.sum()), ("at_lower", (bst < 0).sum()),
                  ("at_upper", (bst > 0).sum()), ("any_soft", soft.any()), ("no_soft", not soft.any()), ("pref_null", p_ref is None), ("pref_given", p_ref is not None),
                  ("rperm_on", bool(use_rperm)), ("rperm_off", not use_rperm)):
        bk.hit("setup", nm, c)
    ex = {"ksoft": ks, "y": y, "Hmask": Hmask, "hpos": hpos, "Hidx": Hidx, "Fmask": pad(fr.astype(np.float64)), "p": pad(pj), "pB": pad(np.where(fr, 0.0, pj)),
          "pF": pad(np.where(fr, ref, 0.0)), "fpos": fpos, "Fidx": Fidx, "s": st["slo"].copy(), "cnt.NH": len(hl), "cnt.NF": len(fl), "cnt.ANYSOFT": int(soft.any())}
    return ex, {}


def tw_as_rhs(st, y_ref, bk):
    n, nH = st["n"], int(st["cnt"][AC["NH"]])
    soft = st["cnt"][AC["ANYSOFT"]] != 0
    H = st["Hidx"][:nH]
    r, t, sl, q, tN = _l(st, "r", "t", "sl", "q", "tN")
    bH = st["bH"].astype(LD); mg = np.zeros(st["M"], LD)
    bH[:nH] = r[H] - t[H] - sl[H]
    mg[:nH] = np.abs(r[H]) + np.abs(t[H]) + np.abs(sl[H])
    yH = st["yH"].copy(); yH[:nH] = 0.0 if y_ref is None else st[y_ref][H]
    ua = st["uacc"].copy(); ua[:nH] = 0.0
    fm = st["Fmask"] != 0.0
    cF = np.where(fm, st["q"] - (st["tN"] if soft else 0.0), 0.0)                 # one subtraction: exact in float64
    bk.hit("rhs", "soft" if soft else "no_soft"); bk.hit("rhs", "yref_null" if y_ref is None else "yref_given"); bk.hit("rhs", "free", fm.sum()); bk.hit("rhs", "bound", (~fm).sum())
    own = np.zeros(st["M"], bool); own[:nH] = True
    return {"yH": yH, "uacc": ua, "cF": cF}, {"bH": (bH, mg, 3, own)}


def tw_as_res_p(st):
    nH = int(st["cnt"][AC["NH"]])
    v = st["v"].copy(); v[:nH] = st["bH"][:nH] - st["t"][st["Hidx"][:nH]]
    return {"v": v}, {}


def tw_as_gather_h(st):
    nH = int(st["cnt"][AC["NH"]])
    v = st["v"].copy(); v[:nH] = st["t"][st["Hidx"][:nH]]
    return {"v": v}, {}


def tw_as_add_yh(st):
    nH = int(st["cnt"][AC["NH"]])
    yH = st["yH"].copy(); yH[:nH] = yH[:nH] + st["u"][:nH]
    return {"yH": yH}, {}


def tw_as_scatter_h(st, src, accumulate, bk):
    pos = st["hpos"]; hd = pos >= 0
    yf = np.where(hd, st[src][np.maximum(pos, 0)], 0.0)
    ex = {"yfull": yf}
    if accumulate:
        ua = st["uacc"].copy(); ua[pos[hd]] = ua[pos[hd]] + st[src][pos[hd]]
        ex["uacc"] = ua
    bk.hit("scatter_h", "hard", hd.sum()); bk.hit("scatter_h", "other", (~hd).sum()); bk.hit("scatter_h", "accumulate" if accumulate else "plain")
    return ex, {}


def tw_as_add_f(st):
    pF, Fm, tN = _l(st, "pF", "Fmask", "tN")
    return {}, {"pF": (pF + Fm * tN, np.abs(pF) + np.abs(Fm * tN), 3)}


def tw_as_rd(st):
    return {"rd": st["Fmask"] * (st["cF"] - st["tN"])}, {}                         # difference, then a product with 0 / 1: no a*b +/- c shape


def tw_as_merge(st, with_y, bk):
    ex = {"p": np.where(st["Fmask"] != 0.0, st["pF"], st["p"])}
    if with_y:
        pos = st["hpos"]
        ex["y"] = np.where(pos >= 0, st["yH"][np.maximum(pos, 0)], st["y"])
    bk.hit("merge", "with_y" if with_y else "without_y")
    return ex, {}


def _as_rows(st, ks):
    """Basic slack values and activities of the tail kernels: (snew, its magnitude, act, its magnitude), long double, from t, sl, ksoft."""
    r, t, sl, slo, scoef = _l(st, "r", "t", "sl", "slo", "scoef")
    a0 = t + sl
    m0 = np.abs(t) + np.abs(sl)
    soft = ks >= 0
    k = np.maximum(ks, 0)
    if st["ns"] == 0:
        return soft, k, np.zeros(0, LD), np.zeros(0, LD), a0, m0
    snew = slo[k] + (r - a0) / scoef[k]
    ms = np.abs(slo[k]) + (np.abs(r) + m0) / np.abs(scoef[k])
    act = np.where(soft, a0 + scoef[k] * (snew - slo[k]), a0)
    ma = np.where(soft, m0 + np.abs(scoef[k]) * (ms + np.abs(slo[k])), m0)
    return soft, k, snew, ms, act, ma


def tw_as_finish(st, cur, nx, prev, have_prev, tol_p, tol_d, bk):
    n, M, ns = st["n"], st["M"], st["ns"]
    rowst, bst, sst = _sets(st, cur)
    td = LD(tol_d) * LD(st["scale_q"])
    r, y, q, tN, p, lb, ub, w, slo, scoef = _l(st, "r", "y", "q", "tN", "p", "lb", "ub", "w", "slo", "scoef")
    soft, k, snew, ms, act, ma = _as_rows(st, st["ksoft"])
    s = st["s"].astype(LD); smag = np.abs(s)
    sown = np.zeros(ns, bool)
    if ns:
        s[k[soft]] = snew[soft]; smag[k[soft]] = ms[soft]; sown[k[soft]] = True
    rt = st["rtype"].astype(LD); ineq = st["rtype"] != 0
    den = 1 + np.abs(r)
    viol = np.where(ineq, np.maximum(0, rt * (r - act)), np.abs(act - r)) / den
    pr_v, pr_m = [viol], [(ma + np.abs(r)) / den]
    dr = np.where(rowst == 0, np.abs(y), np.where(st["rtype"] == 1, np.maximum(-y, 0), np.where(st["rtype"] == -1, np.maximum(y, 0), 0)))
    du_v, du_m = [dr], [np.abs(dr)]
    drop = bk.cmp(rt * y, np.abs(y), 1, "<", -td, ineq & (rowst == 1)) & ineq & (rowst == 1)
    add = bk.cmp(rt * (r - act) / den, (ma + np.abs(r)) / den, 9, ">", tol_p, ineq & (rowst == 0)) & ineq & (rowst == 0)
    nrow = np.where(drop, 0, np.where(add, 1, rowst)).astype(np.int32)
    z = st["q"] - st["tN"]
    zl = z.astype(LD)
    fixed = st["ub"] <= st["lb"]
    pr_v += [np.maximum(lb - p, 0), np.maximum(p - ub, 0)]; pr_m += [np.abs(lb) + np.abs(p), np.abs(p) + np.abs(ub)]
    dz = np.where(fixed, 0, np.where(bst < 0, np.maximum(-zl, 0), np.where(bst > 0, np.maximum(zl, 0), np.abs(zl))))
    du_v.append(dz); du_m.append(dz)
    rl = bk.cmp(zl, np.abs(zl), 1, "<", -td, ~fixed & (bst < 0)) & ~fixed & (bst < 0)
    ru = bk.cmp(zl, np.abs(zl), 1, ">", td, ~fixed & (bst > 0)) & ~fixed & (bst > 0)
    fl = bk.cmp(p - (lb - LD(tol_p)), np.abs(p) + np.abs(lb) + tol_p, 3, "<", 0, bst == 0) & (bst == 0)
    fu = bk.cmp(p - (ub + LD(tol_p)), np.abs(p) + np.abs(ub) + tol_p, 3, ">", 0, (bst == 0) & ~fl) & (bst == 0) & ~fl
    nb = np.where(rl | ru, 0, np.where(fl, -1, np.where(fu, 1, bst))).astype(np.int32)
    bnd = {}
    if ns:
        sd = 1 + np.abs(slo)
        pr_v.append(np.maximum(slo - s, 0) / sd); pr_m.append((np.abs(slo) + smag) / sd)
        zs = w - scoef * y[st["srow"]]
        zm = np.abs(w) + np.abs(scoef * y[st["srow"]])
        du_v.append(np.where(sst == 0, np.maximum(-zs, 0), np.abs(zs))); du_m.append(zm)
        sf = bk.cmp(zs, zm, 3, "<", -td, sst == 0) & (sst == 0)
        thr = slo - LD(tol_p) * sd
        sl_ = bk.cmp(s - thr, smag + np.abs(slo) + tol_p * sd, 9, "<", 0, sst == 1) & (sst == 1)
        nss = np.where(sf, 1, np.where(sl_, 0, sst)).astype(np.int32)
        re = np.zeros(M, bool); re[st["srow"][nss == 1]] = True
        bk.hit("finish", "row_reactivated", (re & (nrow == 0)).sum())
        nrow = np.where(re, 1, nrow).astype(np.int32)
        bk.hit("finish", "slack_free", sf.sum()); bk.hit("finish", "slack_low", sl_.sum()); bk.hit("finish", "slack_keep", (~sf & ~sl_).sum())
        bnd["s"] = (s, smag, 5, sown)
    else:
        sf = sl_ = np.zeros(0, bool); nss = sst.copy()
    nchg = int(drop.sum() + add.sum() + rl.sum() + ru.sum() + fl.sum() + fu.sum() + sf.sum() + sl_.sum())
    for nm, c in (("row_soft", soft.sum()), ("row_eq", (~ineq).sum()), ("row_drop", drop.sum()), ("row_add", add.sum()), ("row_keep", (ineq & ~drop & ~add).sum()),
                  ("col_fixed", fixed.sum()), ("col_release_lo", rl.sum()), ("col_release_up", ru.sum()), ("col_fix_lo", fl.sum()), ("col_fix_up", fu.sum()),
                  ("col_keep", (~rl & ~ru & ~fl & ~fu).sum()), ("have_prev", bool(have_prev)), ("no_prev", not have_prev)):
        bk.hit("finish", nm, c)
    ex = {"z": z, "S%d.rowst" % nx: nrow, "S%d.bst" % nx: nb, "S%d.sst" % nx: nss, "cnt.NCHG": nchg}
    if have_prev:
        pr_, pb, ps = _sets(st, prev)
        ex["cnt.NDIFF"] = int((nrow != pr_).sum() + (nb != pb).sum() + (nss != ps).sum())
    else:
        ex["cnt.NDIFF"] = -1
    cat = lambda vs: np.concatenate([np.atleast_1d(np.asarray(v, LD)) for v in vs] + [np.zeros(1, LD)])
    bnd["act"] = (act, ma, 5)
    bnd["scal.PR"] = (cat(pr_v).max(), cat(pr_m).max(), 9)
    bnd["scal.DU"] = (cat(du_v).max() / LD(st["scale_q"]), cat(du_m).max() / LD(st["scale_q"]), 4)
    return ex, bnd


def tw_face_dual_finish(st, D, tol_m, bk):
    rowst, bst, sst = (a.copy() for a in _sets(st, D))
    td = LD(tol_m) * LD(st["scale_q"])
    z = st["q"] - st["tN"]
    zl = z.astype(LD)
    y, w, scoef = _l(st, "y", "w", "scoef")
    free = st["ub"] > st["lb"]
    cl = bk.cmp(zl, np.abs(zl), 1, "<", -td, free & (bst < 0)) & free & (bst < 0)
    cu = bk.cmp(zl, np.abs(zl), 1, ">", td, free & (bst > 0)) & free & (bst > 0)
    bst[cl | cu] = 0
    rt = st["rtype"].astype(LD)
    m = (st["hpos"] >= 0) & (st["rtype"] != 0)
    rd = bk.cmp(rt * y, np.abs(y), 1, "<", -td, m) & m
    rowst[rd] = 0
    nv = int(cl.sum() + cu.sum() + rd.sum())
    if st["ns"]:
        zs = w - scoef * y[st["srow"]]
        sb = bk.cmp(zs, np.abs(w) + np.abs(scoef * y[st["srow"]]), 3, "<", -td, sst == 0) & (sst == 0)
        sst[sb] = 1
        re = np.zeros(st["M"], bool); re[st["srow"][sst == 1]] = True
        bk.hit("dual_finish", "row_reactivated", (re & (rowst == 0)).sum())
        rowst[re] = 1
        nv += int(sb.sum())
        bk.hit("dual_finish", "slack_basic", sb.sum()); bk.hit("dual_finish", "slack_keep", (~sb).sum())
    for nm, c in (("col_lo", cl.sum()), ("col_up", cu.sum()), ("col_keep", (~cl & ~cu).sum()), ("row_drop", rd.sum()), ("row_keep", (~rd).sum()), ("none", nv == 0)):
        bk.hit("dual_finish", nm, c)
    return {"z": z, "S%d.rowst" % D: rowst, "S%d.bst" % D: bst, "S%d.sst" % D: sst, "cnt.NVIOL": nv}, {}


def tw_face_kkt(st, D, bk):
    rowst, bst, sst = _sets(st, D)
    rt = st["rtype"]
    a, r, y, p, z = st["act"], st["r"], st["y"], st["p"], st["z"]
    viol = np.where(rt == 0, np.abs(a - r), np.maximum(0.0, rt * (r - a))) / (1.0 + np.abs(r))
    pr = max(viol.max(initial=0.0), np.maximum(st["lb"] - p, 0.0).max(initial=0.0), np.maximum(p - st["ub"], 0.0).max(initial=0.0))
    dr = np.where(rowst == 0, np.abs(y), np.where(rt == 1, np.maximum(-y, 0.0), np.where(rt == -1, np.maximum(y, 0.0), 0.0)))
    fixed = st["ub"] <= st["lb"]
    dz = np.where(fixed, 0.0, np.where(bst < 0, np.maximum(-z, 0.0), np.where(bst > 0, np.maximum(z, 0.0), np.abs(z))))
    du_v = [dr.astype(LD), dz.astype(LD), np.zeros(1, LD)]; du_m = list(du_v)
    if st["ns"]:
        pr = max(pr, (np.maximum(st["slo"] - st["s"], 0.0) / (1.0 + np.abs(st["slo"]))).max(initial=0.0))
        w, scoef, yl = _l(st, "w", "scoef", "y")
        zs = w - scoef * yl[st["srow"]]
        du_v.append(np.where(sst == 0, np.maximum(-zs, 0), np.abs(zs))); du_m.append(np.abs(w) + np.abs(scoef * yl[st["srow"]]))
        bk.hit("kkt", "slack_basic", (sst == 1).sum()); bk.hit("kkt", "slack_bound", (sst == 0).sum())
    for nm, c in (("row_eq", (rt == 0).sum()), ("row_ge", ((rt == 1) & (rowst != 0)).sum()), ("row_le", ((rt == -1) & (rowst != 0)).sum()), ("row_inactive", (rowst == 0).sum()),
                  ("col_fixed", fixed.sum()), ("col_lo", (~fixed & (bst < 0)).sum()), ("col_up", (~fixed & (bst > 0)).sum()), ("col_free", (~fixed & (bst == 0)).sum())):
        bk.hit("kkt", nm, c)
    sq = LD(st["scale_q"])
    return {"scal.PR": pr}, {"scal.DU": (np.concatenate(du_v).max() / sq, np.concatenate(du_m).max() / sq, 4)}


def tw_as_pack(st, S):
    n, M, ns = st["n"], st["M"], st["ns"]
    rowst, bst, sst = _sets(st, S)
    d = np.concatenate([st["p"], st["z"], st["y"], st["act"], st["s"]])
    i = np.concatenate([rowst, bst, sst]).astype(np.int32)
    return d, i


def tw_as_copy_sets(st, dst, src):
    return {"S%d.%s" % (dst, nm): st["S%d.%s" % (src, nm)].copy() for nm in ("rowst", "bst", "sst")}, {}


def tw_face_ns_combine(p0, Z, u):
    """p = p0 + sum_c u_c z_c: (value, magnitude, k) with k = 2 terms + 1."""
    p0, Z, u = np.asarray(p0, LD), np.asarray(Z, LD), np.asarray(u, LD)
    val = p0 + (u[:, None] * Z).sum(axis=0) if len(u) else p0.copy()
    mag = np.abs(p0) + (np.abs(u[:, None] * Z)).sum(axis=0) if len(u) else np.abs(p0)
    return val, mag, 2 * len(u) + 1


def tw_face_ns_z(st):
    rd, Fm, tN = _l(st, "rd", "Fmask", "tN")
    return {}, {"z": (rd - Fm * tN, np.abs(rd) + np.abs(Fm * tN), 3)}


def tw_face_ns_unmark(st, W, fam, e, bk):
    rowst, bst, sst = (a.copy() for a in _sets(st, W))
    if fam == 0:
        rowst[e] = 0
    elif fam == 1:
        sst[e] = 1; rowst[st["srow"][e]] = 1
    else:
        bst[e] = 0
    bk.hit("ns_unmark", ("fam_row", "fam_slack", "fam_lower", "fam_upper")[fam])
    return {"S%d.rowst" % W: rowst, "S%d.bst" % W: bst, "S%d.sst" % W: sst}, {}


def as_col_row(st, fam, e):
    """The row of the matrix k_face_ns_col reads for (fam, e), -1 for a bound."""
    return e if fam == 0 else (int(st["srow"][e]) if fam == 1 else -1)


def tw_face_ns_col(st, arow, fam, e, p0, t0, bk):
    """arow: the row as_col_row names (n entries; unused for a bound)."""
    n = st["n"]
    row = as_col_row(st, fam, e)
    if row >= 0:
        c = st["Fmask"] * arow[:n]
        g = (LD(st["r"][row]) - LD(st["sl"][row]) - LD(st[t0][row]), abs(LD(st["r"][row])) + abs(LD(st["sl"][row])) + abs(LD(st[t0][row])), 3)
    else:
        c = np.zeros(n); c[e] = 1.0
        b = st["lb"][e] if fam == 2 else st["ub"][e]
        g = (LD(b) - LD(st[p0][e]), abs(LD(b)) + abs(LD(st[p0][e])), 2)
    cl = c.astype(LD)
    bk.hit("ns_col", ("fam_row", "fam_slack", "fam_lower", "fam_upper")[fam])
    return {"rd": c}, {"scal.EQRES": g, "scal.PR": ((cl * cl).sum(), (cl * cl).sum(), 2 * n + 1)}


def as_step_candidates(st, W, act, s, tol_p):
    """Eligible entries of the ratio test of k_face_ns_step in float64, as the kernel states them, from the activities `act` and slack values `s`
    (the device's, or the twin's): per family (0 row, 1 slack, 2 lower, 3 upper) the index list and the ratios."""
    rowst, bst, sst = _sets(st, W)
    rt = st["rtype"]
    den = 1.0 + np.abs(st["r"])

    def ratio(g0, g1):
        a = np.maximum(g0, 0.0)
        return a / (a - g1)
    out = []
    with np.errstate(all="ignore"):
        g1 = rt * (act - st["r"]) / den
        m = (rt != 0) & (rowst == 0) & (g1 < -tol_p)
        out.append((np.nonzero(m)[0], ratio(rt * (st["acta"] - st["r"]) / den, g1)[m]))
        sd = 1.0 + np.abs(st["slo"])
        g1 = (s - st["slo"]) / sd
        m = (sst == 1) & (g1 < -tol_p)
        out.append((np.nonzero(m)[0], ratio((st["sa"] - st["slo"]) / sd, g1)[m]))
        g1 = st["p"] - st["lb"]
        m = (bst == 0) & (g1 < -tol_p)
        out.append((np.nonzero(m)[0], ratio(st["pa"] - st["lb"], g1)[m]))
        g1 = st["ub"] - st["p"]
        m = (bst == 0) & (g1 < -tol_p)
        out.append((np.nonzero(m)[0], ratio(st["ub"] - st["pa"], g1)[m]))
    return out


def tw_face_ns_step(st, W, tol_p, bk, dev=None):
    """k_face_ns_step.  The ratios are quotients of differences - no a*b +/- c shape - so, given the activities and slack values (dev = the
    device's (act, s); default: float64 evaluation of the twin's own), the ratio test is a float64-exact statement: nviol, the step, family and
    index (ties: family order, lowest index).  The anchor update pa + al (p - pa) is bounded (k = 4)."""
    n, M, ns = st["n"], st["M"], st["ns"]
    rowst, bst, sst = (a.copy() for a in _sets(st, W))
    ks = np.full(M, -1, np.int32)
    if ns:
        h0, h1 = st["rs0"] >= 0, st["rs1"] >= 0
        b0 = np.zeros(M, bool); b1 = np.zeros(M, bool)
        b0[h0] = sst[st["rs0"][h0]] == 1
        b1[h1] = sst[st["rs1"][h1]] == 1
        ks = np.where(b0, st["rs0"], np.where(b1, st["rs1"], -1)).astype(np.int32)
    soft, k, snew, ms, act, ma = _as_rows(st, ks)
    s = st["s"].astype(LD); smag = np.abs(s); sown = np.zeros(ns, bool)
    if ns:
        s[k[soft]] = snew[soft]; smag[k[soft]] = ms[soft]; sown[k[soft]] = True
        s = np.where(sst == 1, s, st["slo"].astype(LD))                       # A.s of the non-basic slacks: reset to slo
        smag = np.where(sst == 1, smag, np.abs(st["slo"]).astype(LD))
        sown |= sst != 1
        bk.hit("ns_step", "nonbasic_reset", (sst != 1).sum())
    a64, s64 = (act.astype(np.float64), s.astype(np.float64)) if dev is None else dev
    cand = as_step_candidates(st, W, a64, s64, tol_p)
    nviol = sum(len(i) for i, _ in cand)
    hard = (rowst == 1) & ~soft
    hres = (np.abs(a64 - st["r"]) / (1.0 + np.abs(st["r"])))[hard].max(initial=0.0)
    ex = {"ksoft": ks, "cnt.NVIOL": nviol, "scal.HARDRES": hres}
    bnd = {"act": (act, ma, 5), "s": (s, smag, 5, sown)}
    info = {"nviol": nviol}
    if nviol == 0:
        bk.hit("ns_step", "feasible")
        return ex, bnd, info
    alpha = min(float(r_.min()) for i, r_ in cand if len(i))
    fam = min(f for f, (i, r_) in enumerate(cand) if len(i) and r_.min() == alpha)
    e = int(cand[fam][0][cand[fam][1] == alpha].min())
    al = min(alpha, 1.0)
    if fam == 0:
        rowst[e] = 1
    elif fam == 1:
        sst[e] = 0
    else:
        bst[e] = -1 if fam == 2 else 1
    bk.hit("ns_step", "blocked"); bk.hit("ns_step", ("fam_row", "fam_slack", "fam_lower", "fam_upper")[fam]); bk.hit("ns_step", "alpha_below_1")
    ex.update({"S%d.rowst" % W: rowst, "S%d.bst" % W: bst, "S%d.sst" % W: sst, "cnt.NCHG": fam, "cnt.NDIFF": e})
    all_ = LD(al)
    for anc, cur_ in (("acta", a64), ("pa", st["p"]), ("sa", s64)):
        x, c = st[anc].astype(LD), np.asarray(cur_, LD)
        bnd[anc] = (x + all_ * (c - x), np.abs(x) + np.abs(all_) * (np.abs(c) + np.abs(x)), 4)
    info.update({"alpha": alpha, "fam": fam, "e": e, "cand": cand})
    return ex, bnd, info


def tw_face_primal_finish(st, W, part, tol_p, tol_m, check_only, bk):
    n, M, ns = st["n"], st["M"], st["ns"]
    rowst, bst, sst = (a.copy() for a in _sets(st, W))
    prow, pb, ps = _sets(st, part)
    r, p, lb, ub, slo, scoef, tN, uacc = _l(st, "r", "p", "lb", "ub", "slo", "scoef", "tN", "uacc")
    soft, k, snew, ms, act, ma = _as_rows(st, st["ksoft"])
    s = st["s"].astype(LD); smag = np.abs(s); sown = np.zeros(ns, bool)
    if ns:
        s[k[soft]] = snew[soft]; smag[k[soft]] = ms[soft]; sown[k[soft]] = True
    rt = st["rtype"].astype(LD); ineq = st["rtype"] != 0
    den = 1 + np.abs(r)
    m = ineq & (rowst == 0)
    vr = bk.cmp(rt * (r - act) / den, (ma + np.abs(r)) / den, 9, ">", tol_p, m) & m
    hd = st["hpos"] >= 0
    hres_v = (np.abs(act - r) / den)[hd]; hres_m = ((ma + np.abs(r)) / den)[hd]
    fb = bst == 0
    vl = bk.cmp(p - (lb - LD(tol_p)), np.abs(p) + np.abs(lb) + tol_p, 3, "<", 0, fb) & fb
    vu = bk.cmp(p - (ub + LD(tol_p)), np.abs(p) + np.abs(ub) + tol_p, 3, ">", 0, fb) & fb
    if ns:
        sd = 1 + np.abs(slo)
        vs = bk.cmp(s - (slo - LD(tol_p) * sd), smag + np.abs(slo) + tol_p * sd, 9, "<", 0, sst == 1) & (sst == 1)
    else:
        vs = np.zeros(0, bool)
    nviol = int(vr.sum() + (vl | vu).sum() + vs.sum())
    for nm, c in (("viol_row", vr.sum()), ("viol_lo", vl.sum()), ("viol_up", vu.sum()), ("viol_slack", vs.sum())):
        bk.hit("primal_finish", nm, c)
    nrel = 0
    if check_only:
        bk.hit("primal_finish", "check_only")
    elif nviol:
        rowst[vr] = 1; bst[vl] = -1; bst[vu & ~vl] = 1
        if ns:
            sst[vs] = 0
        bk.hit("primal_finish", "grow")
        for nm, c in (("grow_row", vr.sum()), ("grow_lo", vl.sum()), ("grow_up", (vu & ~vl).sum()), ("grow_slack", vs.sum())):
            bk.hit("primal_finish", nm, c)
    else:
        pos = np.maximum(st["hpos"], 0)
        m = hd & (prow != 1) & ineq
        rr = bk.cmp(rt * uacc[pos], np.abs(uacc[pos]), 1, "<", -LD(tol_m), m) & m
        bk.hit("primal_finish", "rel_mandatory_kept", (hd & (prow == 1) & ineq).sum())
        rowst[rr] = 0
        nrel = int(rr.sum())
        if ns:
            ps_ = np.maximum(st["hpos"][st["srow"]], 0)
            m = (sst == 0) & (ps != 0) & (st["hpos"][st["srow"]] >= 0)
            rs = bk.cmp(scoef * uacc[ps_], np.abs(scoef * uacc[ps_]), 2, ">", tol_m, m) & m
            sst[rs] = 1
            nrel += int(rs.sum())
            bk.hit("primal_finish", "rel_slack", rs.sum())
        nu = (p - tN)
        m = (bst != 0) & (pb == 0) & (st["ub"] > st["lb"])
        rl = bk.cmp(nu, np.abs(p) + np.abs(tN), 2, "<", -LD(tol_m), m & (bst < 0)) & m & (bst < 0)
        ru = bk.cmp(nu, np.abs(p) + np.abs(tN), 2, ">", tol_m, m & (bst > 0)) & m & (bst > 0)
        bst[rl | ru] = 0
        nrel += int(rl.sum() + ru.sum())
        if ns:
            re = np.zeros(M, bool); re[st["srow"][sst == 1]] = True
            bk.hit("primal_finish", "row_reactivated", (re & (rowst == 0)).sum())
            rowst[re] = 1
        bk.hit("primal_finish", "release" if nrel else "unchanged")
        for nm, c in (("rel_row", rr.sum()), ("rel_lo", rl.sum()), ("rel_up", ru.sum())):
            bk.hit("primal_finish", nm, c)
    ex = {"nu": st["p"] - st["tN"], "S%d.rowst" % W: rowst, "S%d.bst" % W: bst, "S%d.sst" % W: sst, "cnt.NVIOL": nviol, "cnt.NREL": nrel}
    bnd = {"act": (act, ma, 5), "scal.HARDRES": (hres_v.max(initial=0), hres_m.max(initial=0), 9)}
    if ns:
        bnd["s"] = (s, smag, 5, sown)
    return ex, bnd


# (n, M, ns): ns = 0 and M = 0; one below, at and above 64, 256 and 1024; above 2048 (three and more sweeps of the one-workgroup loops); around
# 70 000 in n and in M; ns > M (rows with two slack columns) and rows with none.  Each case runs with rperm null and with a permutation.
AS_CASES = [
    (1, 1, 0), (256, 0, 0), (64, 63, 65), (63, 65, 64), (65, 64, 63), (256, 256, 257), (1024, 1024, 1023), (255, 257, 256), (257, 255, 300), (1025, 1023, 1024), (1023, 1025, 1500), (2049, 3100, 2500), (4097, 2050, 0),
    (70001, 1030, 257), (1030, 70003, 5000),
]


def as_grid_all(n, M, ns):
    return (max(n, M, ns, 1) + 255) // 256


# ---- planted ties: every operand a small dyadic rational, tolerances and scale_q powers of two, so the float64 evaluation is exact in any
# association and the quantity sits exactly on its threshold: the side taken follows from < / <= / >= alone
TIE_TOL_P, TIE_TOL_D, TIE_TOL_M, TIE_SQ = 2.0 ** -30, 2.0 ** -20, 2.0 ** -30, 4.0
AS_TIE_SIZE = (2100, 2100, 1500)
AS_TIES = {"identify": "lower upper slack row forced".split(), "finish": "row_drop row_add rel_lo rel_up fix_lo fix_up slack_free slack_low".split(),
           "dual_finish": "col_lo col_up row slack".split(), "primal_finish": "viol_row viol_lo viol_up rel_row rel_lo rel_up".split(),
           "ns_step": "thr_row thr_lower thr_upper thr_slack".split()}


def _spots(mask):
    """Entries of `mask` nearest to the first and last element, a wavefront edge (63 | 64) and a sweep edge (1023 | 1024)."""
    idx = np.nonzero(mask)[0]
    out = []
    for want in (0, 63, 64, 1023, 1024, len(mask) - 1):
        if len(idx):
            out.append(int(idx[np.argmin(np.abs(idx - want))]))
    return sorted(set(out))


def as_tie_state(kernel, which, seed=5):
    """A state of AS_TIE_SIZE with the comparison `which` of `kernel` planted exactly on its threshold at the _spots; returns (state, planted
    index list).  scale_q and the tolerances to use are TIE_*."""
    n, M, ns = AS_TIE_SIZE
    st = as_state(seed, n, M, ns, TIE_SQ)
    tp, td, tm = TIE_TOL_P, (TIE_TOL_M if kernel == "dual_finish" else TIE_TOL_D) * TIE_SQ, TIE_TOL_M      # (k_face_dual_finish: td = tol_m scale_q)
    free = st["ub"] > st["lb"]
    noslack = (st["rs0"] < 0)
    if kernel == "identify":
        if which in ("lower", "upper"):
            I = _spots(free)
            st["lb"][I], st["ub"][I] = -1.0, 1.0                                  # width 2
            a, b = ("ip.tL", "ip.muL") if which == "lower" else ("ip.tU", "ip.muU")
            st[a][I], st[b][I] = 1.0, 2.0                                          # 1 / 2 == 2 / 4
        elif which == "slack":
            I = _spots(np.ones(ns, bool))
            st["slo"][I], st["ip.ts"][I], st["ip.mus"][I] = 1.0, 1.0, 2.0
        elif which == "row":
            I = _spots(noslack)
            st["rtype"][I] = 1
            st["r"][I], st["ip.g"][I], st["ip.pi"][I] = 1.0, 1.0, 2.0
        else:                                                                      # a row made active only by a slack exactly on its threshold
            I = _spots(st["rs1"] >= 0)
            st["rtype"][I] = 1
            st["ip.g"][I], st["ip.pi"][I] = 1.0, 0.0
            for i in I:
                st["ip.ts"][st["rs0"][i]], st["ip.mus"][st["rs0"][i]] = 1e-9, 1.0     # rs0 clearly at its bound
                k = st["rs1"][i]
                st["slo"][k], st["ip.ts"][k], st["ip.mus"][k] = 1.0, 1.0, 2.0
        return st, I
    if kernel in ("finish", "dual_finish", "primal_finish") and which in ("row_drop", "row", "rel_row"):
        m = noslack & (st["S0.rowst"] == 1) if kernel != "primal_finish" else (st["hpos"] >= 0)
        I = _spots(m)
        st["rtype"][I] = 1
        st["y"][I] = -td
        st["uacc"][st["hpos"][I]] = -tm
        for k in range(1, 6):
            st["S%d.rowst" % k][I] = 1 if k != 3 else 0                            # in W and D, not mandatory
        return st, I
    if which in ("row_add", "viol_row", "thr_row"):
        m = noslack & (st["S0.rowst"] == 0)
        I = _spots(m)
        st["rtype"][I] = 1
        st["r"][I] = 1.0
        st["t"][I] = 1.0 - 2.0 * tp                                                # rt (r - a) / 2 == tol_p ; g1 == -tol_p
        st["sl"][I] = 0.0
        for k in range(1, 6):
            st["S%d.rowst" % k][I] = 0
        st["acta"][I] = 2.0
        return st, I
    if which in ("rel_lo", "rel_up", "col_lo", "col_up"):
        lo = which.endswith("lo")
        I = _spots(free)
        for k in range(6):
            st["S%d.bst" % k][I] = -1 if lo else 1
        st["S3.bst"][I] = 0                                                        # not mandatory
        st["q"][I] = 1.0
        st["tN"][I] = 1.0 + td if lo else 1.0 - td                                 # z == -td | td
        st["p"][I] = -tm if lo else tm                                             # primal_finish: nu = p - tN
        if kernel == "primal_finish":
            st["tN"][I] = 0.0
        return st, I
    if which in ("fix_lo", "fix_up", "viol_lo", "viol_up", "thr_lower", "thr_upper"):
        lo = which.endswith("lo") or which.endswith("lower")
        I = _spots(free)
        for k in range(6):
            st["S%d.bst" % k][I] = 0
        st["lb"][I], st["ub"][I] = -1.0, 1.0
        st["p"][I] = -1.0 - tp if lo else 1.0 + tp
        st["pa"][I] = 0.0
        return st, I
    if which in ("slack_free", "slack"):
        I = _spots(np.ones(ns, bool))
        for k in range(6):
            st["S%d.sst" % k][I] = 0
        st["w"][I], st["scoef"][I] = 1.0, 1.0
        st["y"][st["srow"][I]] = 1.0 + td                                          # zs == -td
        return st, I
    if which in ("slack_low", "thr_slack"):
        # a basic slack whose value lands exactly on slo - tol (1 + |slo|): slo = 1, scoef = 1, r = 1, sl = 1 (one slack column), t = 2 tol
        I = [k for k in _spots(np.ones(ns, bool)) if st["rs1"][st["srow"][k]] < 0]
        for k in range(6):
            st["S%d.sst" % k][I] = 1
            st["S%d.rowst" % k][st["srow"][I]] = 1
        st["slo"][I], st["scoef"][I] = 1.0, 1.0
        rows = st["srow"][I]
        st["ksoft"][rows] = np.asarray(I, np.int32)
        st["r"][rows], st["sl"][rows], st["t"][rows] = 1.0, 1.0, 2.0 * tp          # snew = 1 + (1 - 1 - 2 tol) = 1 - 2 tol
        st["sa"][I] = 2.0
        st["rtype"][rows] = 0
        return st, I
    raise KeyError((kernel, which))


def as_ratio_tie_state(fams, spots, decoys=True, seed=9):
    """k_face_ns_step: a feasible state (no violated inequality) into which entries with the exactly representable ratio 1 / 4 are planted in
    the families `fams` at the index positions `spots` (wanted positions; the nearest admissible entry is taken), plus - with `decoys` -
    ineligible entries that would have ratio 1 / 8: a row already in W, an equality row, a column in W, a margin g1 = -tol / 2 >= -tol.
    Anchor margin g0 = 1 / 4 (rows: times den 2), candidate margin g1 = -3 / 4: ratio = (1/4) / (1/4 + 3/4)."""
    n, M, ns = AS_TIE_SIZE
    st = as_state(seed, n, M, ns, TIE_SQ)
    W = 4
    rowst, bst, sst = _sets(st, W)
    noslack = st["rs0"] < 0
    # feasible everywhere: rows of W-inactive inequalities sit at act = r + rt, free columns inside their box, basic slacks above slo
    sst[:] = 0
    st["sl"] = _as_sl(st)
    st["t"] = st["r"] + st["rtype"] * 1.0 - st["sl"]
    st["p"] = np.clip(st["p"], st["lb"], st["ub"])
    planted = []

    def near(mask, want, fam):
        mask = mask.copy()
        mask[[j for f, j in planted if (f >= 2) == (fam >= 2) and (f == fam or fam != 1 and f != 1)]] = False      # one plant per row / slack / column
        idx = np.nonzero(mask)[0]
        return int(idx[np.argmin(np.abs(idx - want))])
    for fam in fams:
        for want in spots:
            if fam == 0:
                i = near(noslack & (st["rtype"] != 0), want, fam)
                rowst[i] = 0; st["rtype"][i] = 1; st["r"][i] = 1.0; st["sl"][i] = 0.0
                st["acta"][i], st["t"][i] = 1.5, -0.5                               # g0 = 0.5 / 2, g1 = -1.5 / 2
            elif fam == 1:
                k = near(st["rs1"][st["srow"]] < 0, want, fam)
                i = st["srow"][k]
                sst[k] = 1; rowst[i] = 1
                st["slo"][k], st["scoef"][k], st["r"][i], st["sl"][i], st["rtype"][i] = 1.0, 1.0, 1.0, 1.0, 0
                st["t"][i] = 1.5                                                     # snew = 1 + (1 - 2.5) = -0.5 ; g1 = -1.5 / 2
                st["sa"][k] = 1.5                                                    # g0 = 0.5 / 2
                i = k
            else:
                i = near(st["ub"] > st["lb"], want, fam)
                bst[i] = 0; st["lb"][i], st["ub"][i] = -1.0, 1.0
                st["pa"][i], st["p"][i] = (-0.75, -1.75) if fam == 2 else (0.75, 1.75)
            planted.append((fam, i))
    if decoys:
        free_rows = np.nonzero(noslack)[0]
        used = {i for f, i in planted if f == 0}
        dr = [i for i in free_rows if i not in used][:3]
        for j, i in enumerate(dr):                                                  # ratio 1 / 8 if they counted: g0 = 1/4 (den 2), g1 = -7/4
            st["r"][i], st["sl"][i], st["acta"][i], st["t"][i] = 1.0, 0.0, 1.5, -2.5
            st["rtype"][i] = 1
        rowst[dr[0]] = 1                                                            # already in W
        st["rtype"][dr[1]] = 0; rowst[dr[1]] = 1                                    # an equality row (kept out of the hard residual's way: t = r)
        st["t"][dr[1]] = 1.0
        rowst[dr[2]] = 0; st["t"][dr[2]] = 1.0 - TIE_TOL_P                          # g1 = -tol / 2: not below -tol
        usedc = {i for f, i in planted if f >= 2}
        dc = [j for j in np.nonzero(st["ub"] > st["lb"])[0] if j not in usedc][:1]
        for j in dc:
            st["lb"][j], st["ub"][j], st["pa"][j], st["p"][j] = -1.0, 1.0, -0.75, -2.75
            bst[j] = -1                                                             # a column in W
    return st, planted


# ---- one equality-constrained solve as Solver::as_solve sequences it (modes 0, 1, 2), with the products and the H-system solve done here in long
# double.  `do(st, kind, **kw)` runs one stage - a twin on the CPU, the kernel on the device - and returns the state after it.
def as_chain_lp(seed, n=48, M=30, ns=14):
    """A small dense LP with a working set (set 0) whose A_HF has orthonormal rows times a diagonal of condition <= 100, so that the H-system
    is well conditioned by construction (condition of S = A_HF A_HF' at most 1e4)."""
    rng = np.random.default_rng(seed)
    st = as_state(seed, n, M, ns, 8.0)
    st["q"][0] = 8.0
    rowst, bst, sst = _sets(st, 0)
    ex, _ = tw_as_setup(st, 0, None, 0, AsBook())
    H, F = ex["Hidx"][:ex["cnt.NH"]], ex["Fidx"][:ex["cnt.NF"]]
    while len(H) > len(F) - 2:                                       # more free columns than hard rows
        j = int(np.nonzero(bst != 0)[0][0]); bst[j] = 0
        ex, _ = tw_as_setup(st, 0, None, 0, AsBook())
        H, F = ex["Hidx"][:ex["cnt.NH"]], ex["Fidx"][:ex["cnt.NF"]]
    A = rng.standard_normal((M, n))
    Q, _ = np.linalg.qr(rng.standard_normal((len(F), len(H))))
    A[np.ix_(H, F)] = (10.0 ** rng.uniform(-1, 1, len(H)))[:, None] * Q.T
    st["sl"] = _as_sl(st)
    st["s"] = st["slo"].copy()
    return st, A


def as_chain(st, A, cur, mode, p_ref, y_ref, do):
    """k_as_setup ... k_as_merge and the final products, as Solver::as_solve launches them; returns the state before the tail kernel."""
    n, M = st["n"], st["M"]
    Al = A.astype(LD)
    mul = lambda x: (Al @ x.astype(LD)).astype(np.float64)
    mulT = lambda y: (Al.T @ y.astype(LD)).astype(np.float64)
    st = do(st, "setup", cur=cur, p_ref=p_ref)
    nH, nF, soft = (int(st["cnt"][AC[k]]) for k in ("NH", "NF", "ANYSOFT"))
    if nH > 0:
        st = dict(st, t=mul(st["pB"]))
        if soft:
            st = dict(st, tN=mulT(st["y"]))
        st = do(st, "rhs", y_ref=y_ref)
    if nH > 0 and nF > 0:
        H = st["Hidx"][:nH]
        AHF = Al[H] * st["Fmask"].astype(LD)
        S = AHF @ AHF.T

        def solve(v):
            u = st["u"].copy()
            u[:nH] = _ld_solve(S, v[:nH].astype(LD))
            return u
        for _ in range(3 if mode == 1 else 4):
            if mode != 2:
                st = dict(st, t=mul(st["pF"]))
                st = do(st, "res_p", k=nH)
                st = dict(st, u=solve(st["v"]))
                st = do(st, "scatter_h", src="u", accumulate=1 if mode == 1 else 0)
                st = dict(st, tN=mulT(st["yfull"]))
                st = do(st, "add_f")
            if mode != 1:
                st = do(st, "scatter_h", src="yH", accumulate=0)
                st = dict(st, tN=mulT(st["yfull"]))
                st = do(st, "rd")
                st = dict(st, t=mul(st["rd"]))
                st = do(st, "gather_h", k=nH)
                st = dict(st, u=solve(st["v"]))
                st = do(st, "add_yh", k=nH)
    if nH > 0:
        st = do(st, "merge", with_y=0 if mode == 1 else 1)
    st = dict(st, t=mul(st["p"]))
    if mode == 1:
        st = do(st, "scatter_h", src="uacc", accumulate=0)
        st = dict(st, tN=mulT(st["yfull"]))
    else:
        st = dict(st, tN=mulT(st["y"]))
    return st


def _ld_solve(S, b):
    """Cholesky solve in long double (S symmetric positive definite by construction)."""
    N = len(b)
    L = np.zeros((N, N), LD)
    for j in range(N):
        L[j, j] = np.sqrt(S[j, j] - (L[j, :j] * L[j, :j]).sum())
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    x = b.copy()
    for i in range(N):
        x[i] = (x[i] - (L[i, :i] * x[:i]).sum()) / L[i, i]
    for i in range(N - 1, -1, -1):
        x[i] = (x[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
    return x.astype(np.float64)


def as_apply(st, tw):
    """The state after a kernel whose twin result is `tw`: exact outputs as stated, bounded ones rounded to float64."""
    st = dict(st)
    ex, bnd = tw[0], tw[1]
    for nm, want in ex.items():
        if nm.startswith("cnt."):
            st["cnt"] = st["cnt"].copy(); st["cnt"][AC[nm[4:]]] = want
        elif nm.startswith("scal."):
            st["scal"] = st["scal"].copy(); st["scal"][AS[nm[5:]]] = want
        else:
            st[nm] = np.asarray(want)[:len(st[nm])].astype(st[nm].dtype)
    for nm, b in bnd.items():
        if nm.startswith("scal."):
            st["scal"] = st["scal"].copy(); st["scal"][AS[nm[5:]]] = float(b[0])
        else:
            own = np.ones(len(st[nm]), bool) if len(b) < 4 else b[3]
            v = st[nm].copy(); v[own] = np.asarray(b[0])[own].astype(np.float64)
            st[nm] = v
    return st


def as_twin_do(bk):
    """The `do` of as_chain that runs the twins."""
    def do(st, kind, **kw):
        tw = {"setup": lambda: tw_as_setup(st, kw["cur"], kw["p_ref"], 0, bk), "rhs": lambda: tw_as_rhs(st, kw["y_ref"], bk), "res_p": lambda: tw_as_res_p(st),
              "scatter_h": lambda: tw_as_scatter_h(st, kw["src"], kw["accumulate"], bk), "add_f": lambda: tw_as_add_f(st), "rd": lambda: tw_as_rd(st),
              "gather_h": lambda: tw_as_gather_h(st), "add_yh": lambda: tw_as_add_yh(st), "merge": lambda: tw_as_merge(st, kw["with_y"], bk)}[kind]()
        return as_apply(st, tw)
    return do


def as_oracle_lp(st, A, rp=0):
    """The oracle's LP container for a state and a dense matrix."""
    from oracle import lp_solver as O
    lp = O.LP(st["q"], A, st["rtype"], st["r"], st["lb"], st["ub"], st["srow"], st["scoef"], st["w"], st["slo"])
    if rp:
        lp.row_pos = np.empty(lp.M, np.int64)
        lp.row_pos[st["rperm"]] = np.arange(lp.M)
    return lp


def as_chain_errors(st0, A, fin, mode, p_ref, y_ref):
    """A finished chain against oracle.eqp on the same working set.  The yardstick is the oracle's own error: eqp is run a second time on the
    same LP with its rows and columns in reverse order (the same numbers summed in another order) and the two answers, mapped back, differ by
    d_self - the rounding noise of this solve on this LP, measured, not estimated.  The chain must agree with the oracle within 10 d_self (and
    never less than 10 units in the last place of the largest entry, for LPs on which the oracle happens to reproduce itself exactly).
    Returns {name: (error, d_self, error / allowance)}.  Mode 1 compares p, mode 2 y, mode 0 both."""
    from oracle import lp_solver as O
    n, M, ns = st0["n"], st0["M"], st0["ns"]
    lp = as_oracle_lp(st0, A)
    sets = tuple(a.astype(np.int64) for a in _sets(st0, 0))
    pr_ = np.zeros(n) if p_ref is None else st0[p_ref]
    yr_ = np.zeros(M) if y_ref is None else st0[y_ref]
    refine = 3 if mode == 1 else 4
    p, s, y, _ = O.eqp(lp, sets, pr_, yr_, refine=refine)
    lr = O.LP(st0["q"][::-1], A[::-1, ::-1], st0["rtype"][::-1], st0["r"][::-1], st0["lb"][::-1], st0["ub"][::-1], M - 1 - st0["srow"], st0["scoef"], st0["w"], st0["slo"])      # (slack columns keep their order: the first basic slack of a row counts)
    p2, s2, y2, _ = O.eqp(lr, (sets[0][::-1], sets[1][::-1], sets[2]), pr_[::-1], yr_[::-1], refine=refine)
    out = {}
    for nm, a, b, c in (("p", p, p2[::-1], fin["p"]), ("y", y, y2[::-1], fin["y"])):
        if (nm == "p" and mode == 2) or (nm == "y" and mode == 1):
            continue
        d_self = float(np.abs(a - b).max())
        allow = 10.0 * max(d_self, U * float(np.abs(a).max(initial=0.0)))
        err = float(np.abs(c - a).max())
        out[nm] = (err, d_self, err / allow if allow > 0 else (0.0 if err == 0 else np.inf))
    return out, lp, sets


# ---- the kernels of a null-space interior-point iteration (asm_ns_kernels.hip.h; tests/test_ns_stages_*.py).  Twins as above: name -> (value in
# long double, magnitude, k).  A sum of L products carries k = L + 2 (one rounding per product, at most L - 1 per partial sum in any order, one
# spare), plus one per further operation of the statement.  Statements of one operation are exact: float64 NumPy, bit for bit.
NS_STAGE_KINDS = ("theta", "factor", "e0", "zt", "gemv_t", "e1", "wm_neg", "kx", "rhs1_bi", "ht", "ru", "reduced_solve", "direction", "rows", "newton",
                  "chol_solve", "symv_res", "add", "relres", "dp", "update", "update_dev", "dinf", "gather_e", "scatter_e", "rowvec_e", "fill")
NS_VEC = {"dpb": 0, "kdpb": 1, "ht": 2, "v": 3, "yM": 5, "bI": 7, "ru": 10, "du": 11, "rr": 12, "dd": 13, "e": 14}      # Solver::nsv numbers
NS_COL_COUNTS = (1, 7, 8, 9, 17, 0, 3, 2, 5, 4)      # entries per column, dealt in turn: eight lanes per column in k_ns_spmvt_*; 17 = three sweeps with a tail
NS_SMALL_USE = 256


def ns_state(seed, n, M, k, nI, mu=1.0, orth=True):
    """An equality-rich sparse LP state without slack columns (ipm_state with ns = 0) for the null-space form: nI inequality rows of both signs,
    the others hard equalities; columns 0 and n - 1 among the fixed ones; a sparse matrix with one empty row, one empty column (5) and column
    lengths NS_COL_COUNTS (column n - 2, the last free one, has 7; the fixed column n - 1 is not empty); Zt with k orthonormal rows that are zero on the fixed columns (for k above the number of
    free columns no such matrix exists: the rows beyond it are random unit vectors - the kernels treat Zt as a dense operand); GI' = (A_I Z)';
    N0 = Zt Th Zt' + GI' D_I^-1 GI from the state's own theta~, N = N0 with the diagonal regularised as k_ns_reduce_lower does."""
    rng = np.random.default_rng(seed)
    st = ipm_state(seed, n, M, 0, mu)
    assert 0 <= nI < M and 1 <= k <= n
    rt = np.zeros(M, np.int32)
    rows_i = np.sort(rng.permutation(M)[:nI])
    rt[rows_i] = np.where(rng.random(nI) < 0.5, 1, -1)
    st["rtype"] = rt
    eq = rt == 0
    t = 10.0 ** rng.uniform(-6, 2, M)
    st["g"], st["pi"] = np.where(eq, 1.0, t), np.where(eq, 0.0, mu / t * 10.0 ** rng.uniform(-1, 1, M))
    st["y"] = np.where(eq, st["y"], rt * st["pi"])
    fx = st["ub"] == st["lb"]
    fx[0] = fx[n - 1] = True
    if n >= 3 and fx[n - 2]:      # the last free column is n - 2: its eight-lane sum reaches an output (a fixed column is written as 0 whatever the sum)
        fx[n - 2] = False
        st["ub"][n - 2] = st["lb"][n - 2] + 3.0
        st["tL"][n - 2] = st["tU"][n - 2] = 0.5
        st["muL"][n - 2] = st["muU"][n - 2] = 2.0 * mu
        st["thp_inv"][n - 2] = 0.25
    st["ub"] = np.where(fx, st["lb"], st["ub"])
    st["tL"][fx] = st["tU"][fx] = 1.0
    st["muL"][fx] = st["muU"][fx] = 0.0
    st["thp_inv"][fx] = 0.0
    st["ncomp"] = max(2 * int((~fx).sum()) + nI, 1)
    A = np.zeros((M, n))
    empty_row = M // 2
    rows = np.array([i for i in range(M) if i != empty_row])
    for j in range(n):
        c = 7 if j == n - 2 else (0 if j == 5 else min(max(NS_COL_COUNTS[j % len(NS_COL_COUNTS)], 1 if j == n - 1 else 0), len(rows)))
        A[rng.choice(rows, c, replace=False), j] = rng.standard_normal(c)
    st["A"] = A
    ptr, col, vals = [0], [], []
    for i in range(M):
        nz = np.flatnonzero(A[i])
        col += list(nz); vals += list(A[i, nz]); ptr.append(len(col))
    st["ptr"], st["col"], st["vals"] = np.array(ptr, np.int32), np.array(col, np.int32), np.array(vals)
    st["E"], st["I"] = np.flatnonzero(eq), np.flatnonzero(~eq)
    fr = np.flatnonzero(~fx)
    kk = min(k, len(fr))
    Zt = np.zeros((k, n))
    Zt[:kk, fr] = np.linalg.qr(rng.standard_normal((len(fr), kk)))[0].T
    for c in range(kk, k):
        z = rng.standard_normal(len(fr))
        Zt[c, fr] = z / np.linalg.norm(z)
    st["k"], st["Zt"] = k, Zt
    st["GI"] = (A[st["I"]] @ Zt.T).T.copy()                       # k x nI
    th = ns_theta_exact(st, IPM_RHO_P)
    st["th"], st["thI"] = th["th"], th["thI"]
    st["N0"], st["N"] = ns_reduced_matrix(st)
    for nm in NS_VEC:
        st[nm] = rng.standard_normal(M if nm in ("yM", "bI") else n)
    for nm in ("ru", "du", "rr", "dd"):
        st[nm] = st[nm][:k].copy()
    st["e"][fx] = 0.0
    st["pbar"] = np.where(fx, st["lb"], rng.standard_normal(n))
    st["scal"][SC["NSERR"]] = 0.0
    return st


def ns_reduced_matrix(st):
    """(N0, N) of the state's theta~ in long double, rounded: N0 = Zt Th Zt' + GI' D_I^-1 GI, N = N0 with N_ii += 1e-13 N_ii + 1e-30."""
    Zt, GI = st["Zt"].astype(LD), st["GI"].astype(LD)
    N0 = np.asarray((Zt * st["th"].astype(LD)) @ Zt.T + (GI * st["thI"].astype(LD)) @ GI.T, np.float64)
    N0 = 0.5 * (N0 + N0.T)
    N = N0.copy()
    d = np.arange(len(N0))
    N[d, d] = N0[d, d] + (1e-13 * N0[d, d] + 1e-30)
    return N0, N


def ns_theta_exact(st, rho_p):
    """theta~ of k_ipm_theta_ns in float64 (quotients and plain sums in the kernel's order: nothing to contract): the column part (zero on
    fixed columns) and 1 / dS by position in I; with it k_ipm_theta's own outputs (ipm_theta_exact)."""
    fr = _free(st)
    with np.errstate(all="ignore"):
        th = np.where(fr, st["muL"] / st["tL"] + st["muU"] / st["tU"] + rho_p, 0.0)
        I = np.flatnonzero(st["rtype"] != 0)
        thI = 1.0 / (st["g"][I] / st["pi"][I])
    out = ipm_theta_exact(st, rho_p)
    out.update(th=th, thI=thI)
    return out


def _rows_dot(st, x):
    """Row sums of A x over the stored entries: (value, magnitude, entries) per row."""
    A, x = st["A"].astype(LD), np.asarray(x, LD)
    return A @ x, np.abs(A) @ np.abs(x), np.diff(st["ptr"]).astype(np.int64)


def _cols_dot(st, y):
    A, y = st["A"].astype(LD), np.asarray(y, LD)
    return A.T @ y, np.abs(A).T @ np.abs(y), (st["A"] != 0).sum(0).astype(np.int64)


def _at_I(st, vI, fill=0):
    """An M-vector with vI on the inequality rows (by position in I), `fill` on the equality rows."""
    out = np.full(st["M"], fill, LD)
    out[st["I"]] = vI
    return out


def tw_ns_wm_neg(st):
    """dpbar = -e and *clear = 0 (exact), wM = D_I^-1 (A dpbar) on the inequality rows, zero on the equality rows."""
    a, m, L = _rows_dot(st, -st["e"])
    thI = _at_I(st, st["thI"].astype(LD))
    return {"dpb": -st["e"], "NSERR": 0.0, "yM": (thI * a, thI * m, L + 3)}


def tw_ns_kx(st):
    """K dpbar = Th dpbar + A' yM on the free columns (th != 0), zero elsewhere."""
    a, m, L = _cols_dot(st, st["yM"])
    th, x = _l(st, "th", "dpb")
    on = st["th"] != 0
    return {"kdpb": (np.where(on, th * x + a, 0), np.where(on, np.abs(th * x) + m, 0), L + 4)}


def tw_ns_rhs1_bi(st, base, mode, res, dev):
    """k_ipm_rhs1's complementarity right-hand sides (tw_rhs1, ns = 0), then from the device's own rcg: bI = -res rp + sg rcg / pi and, from
    the device's bI, yM = D_I^-1 bI (one product: exact) on the inequality rows; both zero on the equality rows."""
    out = tw_rhs1(st, base, mode, dev=dev)
    out.pop("rcs", None); out.pop("hs", None)
    ineq = st["rtype"] != 0
    rp, pi = _l(st, "rp", "pi")
    rcg = dev["rcg"].astype(LD)
    with np.errstate(all="ignore"):
        q = np.where(ineq, st["rtype"] * rcg / np.where(ineq, pi, 1), 0)
    out["bI"] = (np.where(ineq, -LD(res) * rp + q, 0), np.where(ineq, abs(res) * np.abs(rp) + np.abs(q), 0), 5)
    out["yM_exact"] = np.where(ineq, np.asarray(_at_I(st, st["thI"].astype(LD)), np.float64) * dev["bI"], 0.0)
    return out


def tw_ns_ht(st, res, dev):
    """h~ = hp + A' yM on the free columns, and from the device's own h~: v = h~ - res K dpbar; zero on fixed columns."""
    a, m, L = _cols_dot(st, st["yM"])
    hp, kd = _l(st, "hp", "kdpb")
    on = st["th"] != 0
    h = dev["ht"].astype(LD)
    return {"ht": (np.where(on, hp + a, 0), np.where(on, np.abs(hp) + m, 0), L + 3),
            "v": (np.where(on, h - LD(res) * kd, 0), np.where(on, np.abs(h) + abs(res) * np.abs(kd), 0), 3)}


def tw_ns_zt(st, x):
    """Zt x: k sums of n products."""
    Z, x = st["Zt"].astype(LD), np.asarray(x, LD)
    return (Z @ x, np.abs(Z) @ np.abs(x), st["n"] + 2)


def tw_ns_gemv_t(st, u):
    """Zt' u: n sums of k products (k_gemv_t_small, or the two-stage kernels: any association)."""
    Z, u = st["Zt"].astype(LD), np.asarray(u, LD)
    return (Z.T @ u, np.abs(Z).T @ np.abs(u), st["k"] + 2)


def tw_ns_symv_res(N0, x, rhs):
    N0, x, rhs = np.asarray(N0, LD), np.asarray(x, LD), np.asarray(rhs, LD)
    return (rhs - N0 @ x, np.abs(rhs) + np.abs(N0) @ np.abs(x), len(x) + 3)


def ns_relres_exact(prev, r, rhs):
    """max(prev, max|r| / max(1, max|rhs|)): maxima and one quotient, exact; a NaN entry is dropped by the maxima (fmax), as by Python's max()."""
    a = float(np.fmax.reduce(np.abs(r), initial=0.0))
    b = float(np.fmax.reduce(np.abs(rhs), initial=1.0))
    return float(np.fmax(prev, a / b))


def tw_ns_dp(st, D, res, dev, zu=None):
    """dp = res dpbar + Z du on the free columns (zu given: the product is an input, k_ns_dp), and from the device's own dp the bound
    multipliers' directions; zeros on the fixed columns."""
    on = st["th"] != 0
    dpb, rcL, rcU, muL, muU, tL, tU = _l(st, "dpb", "rcL", "rcU", "muL", "muU", "tL", "tU")
    if zu is None:
        a, m, kk = tw_ns_gemv_t(st, st["du"])
    else:
        a, m, kk = np.asarray(zu, LD), np.abs(np.asarray(zu, LD)), 1
    dp = dev[D + ".dp"].astype(LD)
    return {D + ".dp": (np.where(on, LD(res) * dpb + a, 0), np.where(on, abs(res) * np.abs(dpb) + m, 0), kk + 2),
            D + ".dmuL": (np.where(on, (rcL - muL * dp) / tL, 0), np.where(on, (np.abs(rcL) + np.abs(muL * dp)) / tL, 0), 4),
            D + ".dmuU": (np.where(on, (rcU + muU * dp) / tU, 0), np.where(on, (np.abs(rcU) + np.abs(muU * dp)) / tU, 0), 4)}


def tw_ns_rows(st, D, dev):
    """aM = A dp; on the inequality rows dy = D_I^-1 (bI - aM), wM = D_I^-1 aM, and from the device's own dy: dpi = sg dy (exact),
    dg = (rcg - g dpi) / pi; zeros on the equality rows."""
    a, m, L = _rows_dot(st, st[D + ".dp"])
    ineq = st["rtype"] != 0
    thI = _at_I(st, st["thI"].astype(LD))
    bI, rcg, g, pi = _l(st, "bI", "rcg", "g", "pi")
    dpi = dev[D + ".dpi"].astype(LD)
    with np.errstate(all="ignore"):
        dg = np.where(ineq, (rcg - g * dpi) / np.where(ineq, pi, 1), 0)
        mg = np.where(ineq, (np.abs(rcg) + np.abs(g * dpi)) / np.where(ineq, pi, 1), 0)
    return {D + ".dy": (thI * (bI - a), thI * (np.abs(bI) + m), L + 4), "yM": (thI * a, thI * m, L + 3), D + ".dg": (dg, mg, 4),
            D + ".dpi_exact": np.where(ineq, st["rtype"] * dev[D + ".dy"], 0.0)}


def tw_ns_update(st, C, al, be, es, dev):
    """k_ipm_update (tw_update, ns = 0) and e *= es (one product: exact)."""
    out = tw_update(st, C, al, be, dev)
    for nm in ("s", "ts", "mus"):
        out.pop(nm)
    out["e_exact"] = st["e"] * es
    return out


def ns_ld_chol_solve(L, Linv, b):
    """(L L')^-1 b in long double from the factor as returned.  Linv (the inverses of the 64-wide diagonal blocks) is what the one-workgroup
    solve multiplies by; in exact arithmetic that is the substitution with L's diagonal blocks, which is what is computed here."""
    L = np.tril(np.asarray(L, LD))
    return _ld_trsv(L.T, _ld_trsv(L, np.asarray(b, LD), True), False)


def _ld_trsv(T, b, lower):
    k = len(b)
    x = np.zeros(k, LD)
    for i in (range(k) if lower else range(k - 1, -1, -1)):
        x[i] = (b[i] - T[i] @ x) / T[i, i]
    return x


def tw_ns_reduced_solve(Lf, N0, ru, dtype=LD):
    """The reduced solve as the kernels state it (oracle: solve_ns): du = N^-1 ru through the factor, one refinement sweep on N0, and the
    relative residual.  dtype float64: the same algorithm in plain NumPy (the measured allowance of the test)."""
    if dtype is LD:
        solve = lambda b: ns_ld_chol_solve(Lf, None, b)
    else:
        from scipy.linalg import solve_triangular
        Lt = np.tril(Lf)
        solve = lambda b: solve_triangular(Lt.T, solve_triangular(Lt, b, lower=True), lower=False)
    N0, ru = np.asarray(N0, dtype), np.asarray(ru, dtype)
    du = solve(ru)
    du = du + solve(ru - N0 @ du)
    return du, ru - N0 @ du


def ns_twin_iteration(lp, st, nsp, ns_e):
    """One iteration of oracle IPM.run in null-space form from the twin's stages, every stage the float64 rounding of its long-double value; the
    reduced solve in long double on the oracle's guarded factor of the twin's own N.  st as ipm_twin_start makes it, with A, ptr, col, Zt,
    GI, E, I, k of the oracle's basis `nsp`.  Returns (pinf, dinf, mu, ap, ad, nserr) and the new e."""
    from oracle import lp_solver as O
    A = lp.A
    st["act"], st["aty"] = A @ st["p"], A.T @ st["y"]
    _f(tw_measures(st), st, ["rp", "rdp", "rds", "MU"])
    for nm, v in ipm_measures_exact(st, st["rp"], st["rdp"], st["rds"]).items():
        st["scal"][SC[nm]] = v
    zr = np.asarray(tw_ns_zt(st, st["rdp"])[0], np.float64)
    st["scal"][SC["DINF"]] = float(np.abs(zr).max(initial=0.0)) / st["scale_q"]
    pinf, dinf, mu = st["scal"][SC["PINF"]], st["scal"][SC["DINF"]], st["scal"][SC["MU"]]
    th = ns_theta_exact(st, IPM_RHO_P)
    st.update(th)
    st["N0"], st["N"] = ns_reduced_matrix(st)
    Lf = O.chol_guard(st["N"].copy(), np.diag(st["N0"]).copy())
    if ns_e is None:
        d0 = np.where(_free(st), st["p"] - nsp.pbar, 0.0)
        zz = np.asarray(tw_ns_gemv_t(st, np.asarray(tw_ns_zt(st, d0)[0], np.float64))[0], np.float64)
        ns_e = np.where(_free(st), d0 - zz, 0.0)
    st["e"] = ns_e
    t = tw_ns_wm_neg(st)
    st["dpb"], st["yM"], nserr = t["dpb"], np.asarray(t["yM"][0], np.float64), 0.0
    _f(tw_ns_kx(st), st, ["kdpb"])

    def newton(mode, base, D):
        nonlocal nserr
        _f(tw_rhs1(st, base, mode), st, ["rcL", "rcU", "rcg"])
        _f(tw_rhs1(st, base, mode, dev=dict(st, hp=st["hp"])), st, ["hp"])
        _f(tw_ns_rhs1_bi(st, base, mode, 1.0, dict(st)), st, ["bI"])
        st["yM"] = tw_ns_rhs1_bi(st, base, mode, 1.0, dict(st))["yM_exact"]
        _f(tw_ns_ht(st, 1.0, dict(st)), st, ["ht"])
        _f(tw_ns_ht(st, 1.0, dict(st)), st, ["v"])
        st["ru"] = np.asarray(tw_ns_zt(st, st["v"])[0], np.float64)
        du, rr = tw_ns_reduced_solve(Lf, st["N0"], st["ru"])
        st["du"] = np.asarray(du, np.float64)
        rr = np.asarray(tw_ns_symv_res(st["N0"], st["du"], st["ru"])[0], np.float64)
        nserr = ns_relres_exact(nserr, rr, st["ru"])
        _f(tw_ns_dp(st, D, 1.0, dict(st)), st, [D + ".dp"])
        _f(tw_ns_dp(st, D, 1.0, dict(st)), st, [D + ".dmuL", D + ".dmuU"])
        _f(tw_ns_rows(st, D, dict(st)), st, [D + ".dy"])
        st[D + ".dpi"] = tw_ns_rows(st, D, dict(st))[D + ".dpi_exact"]
        t2 = tw_ns_rows(st, D, dict(st))
        st[D + ".dg"], st["yM"] = np.asarray(t2[D + ".dg"][0], np.float64), np.asarray(t2["yM"][0], np.float64)

    def steps(D):
        e_ = ipm_steps_exact(st, D)
        st["scal"][SC["AP"]], st["scal"][SC["AD"]] = e_["AP"], e_["AD"]
        return e_["AP"], e_["AD"]
    newton(0, "A", "A")
    steps("A")
    _f(tw_muaff(st, "A", 3), st, ["SM"])
    newton(1, "A", "C")
    ap, ad = steps("C")
    eta = 0.995 if mu >= 1.0 else min(max(0.995, 1.0 - mu / st["scale_q"]), 0.999999)
    al, be = min(1.0, eta * ap), min(1.0, eta * ad)
    new_pi = np.asarray(tw_update(st, "C", al, be, {"pi": st["pi"]})["pi"][0], np.float64)
    tu = tw_ns_update(st, "C", al, be, 1.0 - al, {"pi": new_pi})
    _f(tu, st)
    st["scal"][SC["NSERR"]] = nserr
    return (pinf, dinf, mu, ap, ad, nserr), tu["e_exact"]


# --------------------------------------------------------------------------------------------------------------------------------------
# Basis set-up of the null-space form (tests/test_ns_setup_cpu.py, tests/test_ns_setup_gpu.py): twins of the launch sites of Solver::ns_setup
# (asm_test_ns_setup_stages), written from the statements of oracle/lp_solver.py (class NullSpace) and the comments of asm_ns_kernels.hip.h, on
# the operand as it stands on the device: Ah (M x n), the equality rows Eidx in the order of the factor of S0, the inequality rows Iidx, the
# mask fm of the free columns.  A twin of the second group returns (value, magnitude, K) in long double for bound (a); the exact ones return
# float64 arrays; the algorithms (substitutions, factorisations) are functions of a dtype: long double for the reference, float64 for the
# measured allowance of convention (c).
NSS_KINDS = ("s0_factor", "rhs_cols", "rows_e", "trsm", "pj", "gather_t", "gram", "factor_n", "ortho", "gi", "set_diag", "diag", "count_big", "reproject",
             "basis_from", "setup")       # enum ASM_NSS_* of include/asm_hip.h
NSS_LAYOUT = "ldn nEp nIp ldg nE nI band ld0 cap fld wb n M ldT Mp".split()
NS_BIG, NS_WARM_THR, NS_ZWARM_THR, NS_SEL_THR, NS_MAX_RATIO = 0.5e128, 1e-6, 0.25, (1e-2, 1e-4, 1e-7, 1e-10), 0.3
NSS_PATHS = {"basis": 1, "columns": 2, "cold": 3}


def nss_kcap(k):
    """NsLayout::kcap: rows reserved for a basis of k rows."""
    return (k + k // 4 + 64 + 63) // 64 * 64


def nss_wb(ld):
    """ns_alloc_factor: wide-block width of a factor of pitch ld."""
    return 1024 if (ld <= 1024 or ld > 1536) else 512


def _up32(x):
    return (x + 31) // 32 * 32


class NssOp:
    """The operand of the set-up twins."""

    def __init__(self, Ah, Eidx, Iidx, fm):
        self.A = np.ascontiguousarray(Ah, np.float64)
        self.E, self.I = np.asarray(Eidx, np.int64), np.asarray(Iidx, np.int64)
        self.fm = np.asarray(fm, np.float64)
        self.M, self.n = self.A.shape
        self.nE, self.nI = len(self.E), len(self.I)
        self.ldn, self.nEp, self.nIp = _up32(self.n), _up32(self.nE), _up32(max(self.nI, 1))
        self.ldg = self.ldn + self.nIp
        self.AE, self.AI = self.A[self.E], self.A[self.I]
        self.AEF = self.AE * self.fm
        self.free = self.fm != 0

    def with_fm(self, fm):
        return NssOp(self.A, self.E, self.I, fm)


def _nss_rows_dot(rows, Z):
    """Z (k x n, long double) against the sparse rows `rows` (r x n): (value, magnitude) k x r and K (r) = non-zeros of each row, at least 1."""
    k, r = Z.shape[0], rows.shape[0]
    val, mag, K = np.zeros((k, r), LD), np.zeros((k, r), LD), np.ones(r, np.int64)
    aZ = np.abs(Z)
    for t in range(r):
        c = np.nonzero(rows[t])[0]
        if len(c):
            a = rows[t, c].astype(LD)
            val[:, t], mag[:, t], K[t] = Z[:, c] @ a, aZ[:, c] @ np.abs(a), len(c)
    return val, mag, K


def tw_nss_rhs_cols(op, J=None):
    """k_ns_rhs_cols (exact): row c = column J[c] (None: column c of all n) of A_EF on the rows E, zero over the rest of the pitch nEp; a fixed
    column gives a zero row."""
    cols = np.arange(op.n) if J is None else np.asarray(J, np.int64)
    R = np.zeros((len(cols), op.nEp))
    R[:, :op.nE] = np.where(op.free[cols][:, None], op.AE[:, cols].T, 0.0)
    return R


def tw_nss_rows_e(op, Zt):
    """k_ns_rows_e: R[c, e] = sum_j A[E[e], j] fm_j Zt[c, j] (k x nEp; exactly 0 beyond nE).  K = non-zeros of the row."""
    val, mag, K = _nss_rows_dot(op.AEF, np.asarray(Zt[:, :op.n], LD))
    pad = ((0, 0), (0, op.nEp - op.nE))
    return np.pad(val, pad), np.pad(mag, pad), np.pad(K, (0, op.nEp - op.nE), constant_values=1)


def tw_nss_gi(op, Zt):
    """k_ns_gi: GI'[c, t] = sum_j A[I[t], j] Zt[c, j] (k x nIp; exactly 0 beyond nI).  K = non-zeros of the row."""
    val, mag, K = _nss_rows_dot(op.AI, np.asarray(Zt[:, :op.n], LD))
    pad = ((0, 0), (0, op.nIp - op.nI))
    return np.pad(val, pad), np.pad(mag, pad), np.pad(K, (0, op.nIp - op.nI), constant_values=1)


def tw_nss_pj(op, W, J=None, prev=None):
    """k_ns_pj: PJ[c, j] = fm_j (base[c, j] - sum_{e} W[c, e] A[E[e], j]), base = delta(j, J[c]) in the first pass and the row already there
    (prev) in the second (k x ldn; exactly 0 in the fixed columns and in [n, ldn)).  K = entries of column j on the equality rows, plus 1."""
    k = W.shape[0]
    base = np.zeros((k, op.n), LD)
    if prev is None:
        base[np.arange(k), np.asarray(J, np.int64)] = 1
    else:
        base[:] = prev[:, :op.n]
    Wl = np.asarray(W[:, :op.nE], LD)
    val, mag, K = _nss_rows_dot(np.ascontiguousarray(op.AE.T), Wl)
    val, mag = base - val, np.abs(base) + mag
    K = np.where(np.count_nonzero(op.AE, axis=0) > 0, K, 0) + 1
    val[:, ~op.free] = 0
    mag[:, ~op.free] = 0
    pad = ((0, 0), (0, op.ldn - op.n))
    return np.pad(val, pad), np.pad(mag, pad), np.pad(K, (0, op.ldn - op.n), constant_values=1)


def tw_nss_gather_t(PJ, J):
    """k_ns_gather_t (exact): T[c, d] = PJ[c, J[d]] for d <= c; the strictly upper part is not the kernel's."""
    return np.tril(PJ[:len(J)][:, np.asarray(J, np.int64)])


def tw_nss_ortho_rows(L, G, dev):
    """k_ns_ortho, row c of Zt = L^-1 G from the rows the DEVICE wrote before it: (G[c] - sum_{d < c} L[c, d] dev[d]) / L[c, c].  K = c + 1."""
    k = G.shape[0]
    Ll, Dl = np.tril(np.asarray(L[:k, :k], LD), -1), np.asarray(dev, LD)
    dg = np.asarray(np.diag(L)[:k], LD)[:, None]
    val, mag = np.asarray(G, LD).copy(), np.abs(np.asarray(G, LD))
    for i0 in range(0, k, 128):      # (the lower triangle only, a block of rows at a time)
        i1 = min(k, i0 + 128)
        val[i0:i1] -= Ll[i0:i1, :i1] @ Dl[:i1]
        mag[i0:i1] += np.abs(Ll[i0:i1, :i1]) @ np.abs(Dl[:i1])
    return val / dg, mag / np.abs(dg), (np.arange(k) + 1)[:, None]


def nss_chol_guard(S, d0, thr, dtype=LD):
    """Guarded Cholesky factor of the lower triangle of S in `dtype` (oracle: _chol_guard_loop): a pivot <= thr d0[j] becomes PIV_BIG^2."""
    S = np.asarray(S, dtype)
    N = S.shape[0]
    L = np.zeros((N, N), dtype)
    for j in range(N):
        d = S[j, j] - L[j, :j] @ L[j, :j]
        if not (d > thr * d0[j]):
            d = dtype(1e128) * dtype(1e128)
        L[j, j] = np.sqrt(d)
        if j + 1 < N:
            L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _nss_potrf64(D, d0, thr):
    """The diagonal-block step of the panel kernels (asm_kernels.hip.h: potrf64_body) in float64: the factor L of the nb x nb block D
    (nb <= 64) in 16-wide sub-blocks - a column is scaled by the reciprocal square root of its guarded pivot (the pivot itself becomes
    d / sqrt(d)), the columns of the sub-block are updated one by one over all rows below, the rest of the triangle by one rank-16 update -
    and W = L^-1 by 16 x 16 blocks: diagonal blocks by substitution with the stored reciprocals, W_ij = -W_ii sum_k L_ik W_kj level by level."""
    nb = D.shape[0]
    A, dinv = np.tril(D).copy(), np.ones(nb)
    for c0 in range(0, nb, 16):
        c1 = min(nb, c0 + 16)
        for j in range(c0, c1):
            d = A[j, j]
            if not (d > thr * d0[j]):
                d = 1e256
            inv = 1.0 / np.sqrt(d)
            col = A[j:, j] * inv
            col[0] = d * inv
            A[j:, j], dinv[j] = col, inv
            for c in range(j + 1, c1):
                A[c:, c] -= A[c:, j] * A[c, j]
        if c1 < nb:
            X = A[c1:, c0:c1]
            A[c1:, c1:] -= np.tril(X @ X.T)
    L, W = np.tril(A), np.zeros((nb, nb))
    blocks = [slice(b0, min(nb, b0 + 16)) for b0 in range(0, nb, 16)]
    for sb in blocks:
        m = sb.stop - sb.start
        for t in range(m):
            x = np.zeros(m)
            for r in range(t, m):
                x[r] = ((1.0 if r == t else 0.0) - L[sb.start + r, sb.start:sb.start + r] @ x[:r]) * dinv[sb.start + r]
            W[sb, sb.start + t] = x
    for lev in range(1, len(blocks)):
        for j in range(len(blocks) - lev):
            i = j + lev
            T = sum(L[blocks[i], blocks[q]] @ W[blocks[q], blocks[j]] for q in range(j, i))
            W[blocks[i], blocks[j]] = -(W[blocks[i], blocks[i]] @ T)
    return L, W


def nss_chol_blocked(S, d0, thr):
    """The guarded factor of the lower triangle of S by the device's algorithm, in float64 NumPy (asm_kernels.hip.h: the panel kernels):
    right-looking in 64-wide steps - the diagonal block and its explicit inverse (_nss_potrf64), the panel below as a product with that
    inverse, a rank-64 update of what remains.  This, not a column loop with divisions, is "the same algorithm" convention (c) measures its
    allowance with: on an ill-conditioned matrix the two differ tenfold in what they leave, in the same columns as the device."""
    S = np.tril(np.asarray(S, np.float64)).copy()
    N = S.shape[0]
    for b0 in range(0, N, 64):
        b1 = min(N, b0 + 64)
        L, W = _nss_potrf64(S[b0:b1, b0:b1], d0[b0:b1], thr)
        S[b0:b1, b0:b1] = L
        if b1 < N:
            P = S[b1:, b0:b1] @ W.T
            S[b1:, b0:b1] = P
            S[b1:, b1:] -= np.tril(P @ P.T)
    return S


def nss_trsm_rows(L, B, backward, dtype=LD):
    """Rows of B solved against the lower factor L: L x = b, then (backward) L' x = z.  Long double: substitution; float64: LAPACK."""
    N = L.shape[0]
    if dtype is not LD:
        from scipy.linalg import solve_triangular
        Lt = np.tril(np.asarray(L, np.float64))
        X = solve_triangular(Lt, np.asarray(B, np.float64).T, lower=True)
        return (solve_triangular(Lt.T, X, lower=False) if backward else X).T
    Ll, X = np.tril(np.asarray(L, LD)), np.zeros(B.shape, LD)
    Bl = np.asarray(B, LD)
    for i in range(N):
        X[:, i] = (Bl[:, i] - X[:, :i] @ Ll[i, :i]) / Ll[i, i]
    if backward:
        Z, X = X, np.zeros(B.shape, LD)
        for i in range(N - 1, -1, -1):
            X[:, i] = (Z[:, i] - X[:, i + 1:] @ Ll[i + 1:, i]) / Ll[i, i]
    return X


def nss_ortho(L, G, dtype=LD):
    """Zt = L^-1 G (forward substitution down the rows)."""
    return nss_trsm_rows(L, np.asarray(G).T, False, dtype).T


def _f64(x):
    return np.asarray(x, np.float64)


def nss_chain(op, dtype=LD, hint_J=None, warm_Z=None, M=None):
    """The whole set-up from the twins' statements (oracle: NullSpace.__init__), every stage evaluated in `dtype` from the float64 rounding of
    the stage before: dict(path, k, dropped, J, Zt, GI, L0) - path None and no basis when the LP keeps the row form."""
    n, nE = op.n, op.nE
    AEF, AI, fm = op.AEF.astype(dtype), op.AI.astype(dtype), op.fm
    one = np.ones(n)
    S0 = _f64(AEF @ AEF.T)
    L0 = _f64(nss_chol_guard(S0, np.diag(S0), 1e-10, dtype))
    dropped = int((np.diag(L0) >= NS_BIG).sum())
    k = int(fm.sum()) - (nE - dropped)
    out = dict(path=None, k=k, dropped=dropped, J=None, L0=L0)
    if k < 1 or (M is not None and k > 1.5 * NS_MAX_RATIO * M + 8):
        return out

    def reproject(G, thr):
        R = _f64(np.asarray(G, dtype) @ AEF.T)
        W = _f64(nss_trsm_rows(L0, R, True, dtype))
        Z1 = _f64((np.asarray(G, dtype) - np.asarray(W, dtype) @ AEF) * fm)
        Gm = _f64(np.tril(np.asarray(Z1, dtype) @ np.asarray(Z1, dtype).T))
        L1 = _f64(nss_chol_guard(Gm, one, thr, dtype))
        if (np.diag(L1) >= NS_BIG).any():
            return None
        return _f64(nss_ortho(L1, Z1, dtype))

    def basis_from(J):
        R = tw_nss_rhs_cols(op, J)[:, :nE]
        W = _f64(nss_trsm_rows(L0, R, True, dtype))
        EJ = np.zeros((len(J), n))
        EJ[np.arange(len(J)), J] = 1.0
        PJ = _f64((EJ - np.asarray(W, dtype) @ AEF) * fm)
        LJ = _f64(nss_chol_guard(tw_nss_gather_t(PJ, J), one, NS_WARM_THR, dtype))
        if (np.diag(LJ) >= NS_BIG).any():
            return None
        return reproject(_f64(nss_ortho(LJ, PJ, dtype)), NS_WARM_THR)

    Zt, path, J = None, None, None
    if warm_Z is not None and warm_Z.shape[0] == k:
        Zt = reproject(warm_Z[:, :n], NS_ZWARM_THR)
        path = "basis" if Zt is not None else None
    if Zt is None and hint_J is not None and len(hint_J) == k and np.all(fm[np.asarray(hint_J, np.int64)] > 0):
        J = np.asarray(hint_J, np.int64)
        Zt = basis_from(J)
        path = "columns" if Zt is not None else None
    if Zt is None:
        Yt = _f64(nss_trsm_rows(L0, tw_nss_rhs_cols(op)[:, :nE], False, dtype))
        T = _f64(np.diag(fm) - np.asarray(Yt, dtype) @ np.asarray(Yt, dtype).T)
        for thr in NS_SEL_THR:
            LT = nss_chol_guard(T, one, thr, dtype)
            J = np.nonzero(_f64(np.diag(LT)) < NS_BIG)[0]
            if len(J) == k:
                Zt = basis_from(J)
                if Zt is not None:
                    path = "cold"
                    break
    if Zt is None:
        return out
    out.update(path=path, J=J if path != "basis" else (None if hint_J is None else np.asarray(hint_J, np.int64)), Zt=Zt,
               GI=_f64(np.asarray(Zt, dtype) @ AI.T))
    return out


def nss_quality(op, Zt, GIt=None):
    """max |A_EF Zt'|, max |Zt Zt' - I| and (with GIt) max |GI' - (A_I Zt')'| in long double."""
    Z = np.asarray(Zt[:, :op.n], LD)
    a = float(np.abs(Z @ op.AEF.astype(LD).T).max())
    b = 0.0
    for i0 in range(0, Z.shape[0], 128):      # (the lower triangle only, a block of rows at a time)
        i1 = min(Z.shape[0], i0 + 128)
        b = max(b, float(np.abs(Z[i0:i1] @ Z[:i1].T - np.eye(i1, dtype=LD)[i0:i1]).max()))
    c = None if GIt is None else float(np.abs(np.asarray(GIt[:, :op.nI], LD) - _nss_rows_dot(op.AI, Z)[0]).max(initial=0.0))
    return a, b, c


# cases of the set-up tests: name -> (generator arguments or "banded", fixed columns, dependent equality row, k_reserve or None).  The
# "banded-eq" skeleton of tests/test_builds_gpu.py (n = 500, 300 equality rows, M = 520) does not get the form - n - nE = 200 > 0.3 M - so the
# banded case is the same generator and seed with n = 400.
NSS_CASES = {
    "small": ((61, 100, 70, 50), 0, False, None),             # the smallest qualifying shape: ldn - n = 28, nEp - nE = 26, nIp - nI = 14, k = 30
    "small-fixed": ((61, 100, 70, 50), 6, False, None),       # k = 24: the zeros of the fixed columns
    "small-dep": ((61, 100, 70, 50), 0, True, None),          # A[5] = 2 A[3]: one dropped pivot of S0, k = 31
    "small-reserve": ((61, 100, 70, 50), 6, False, 30),       # the buffers of an earlier LP with fewer fixed columns
    "k1": ((61, 100, 70, 50), -1, False, None),               # all but nE + 1 columns fixed
    "one-ineq": ((64, 100, 99, 1), 0, False, None),           # nI = 1 (and k = 1): M = 100 is the least that qualifies with n = 100
    "dense": ((62, 300, 260, 160), 5, False, None),           # dense S0, k = 35
    "banded": ("banded", 0, False, None),                     # banded S0 (band 14 of 300): banded_subproblem(503, 400, 520, 300, 0), k = 100
    "wide": ((63, 900, 64, 2800), 0, False, None),            # k = 836 > fN.wb = 512: k_ns_ortho, two wide blocks in the k x k factor; S0 is 64 x 64 with band 4
    "wide-fixed": ((63, 900, 64, 2800), 400, False, 836),     # k <= 512 inside a factor of pitch 1152: the product branch of ns_ortho
}


def nss_case(name):
    """(sub-problem, fm, k_reserve or None) of a case of NSS_CASES."""
    gen, nfix, dep, kres = NSS_CASES[name]
    sp = banded_subproblem(503, 400, 520, 300, 0) if gen == "banded" else equality_rich_subproblem(*gen)
    n = sp["n"]
    if dep:      # row 5 = 2 x row 3, entry by entry (the generator deals per_row = 4 entries to every row)
        sp["j_col"], sp["dE"] = sp["j_col"].copy(), sp["dE"].copy()
        sp["j_col"][20:24], sp["dE"][20:24] = sp["j_col"][12:16], 2.0 * sp["dE"][12:16]
        sp["c_lb"], sp["c_ub"] = sp["c_lb"].copy(), sp["c_ub"].copy()
        sp["c_lb"][5] = sp["c_ub"][5] = 2.0 * sp["c_lb"][3]
    fm = np.ones(n)
    rng = np.random.default_rng(1000 + max(nfix, 0))
    if nfix > 0:
        fm[rng.choice(n, nfix, replace=False)] = 0.0
    elif nfix < 0:      # free: the column every equality row owns (a permuted identity: full row rank) and one more
        neq = gen[2]
        own = np.asarray(sp["j_col"])[np.arange(neq) * 4] - 1
        fm[:] = 0.0
        fm[own] = 1.0
        fm[np.nonzero(fm == 0)[0][7]] = 1.0
    return sp, fm, kres
