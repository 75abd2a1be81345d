"""NumPy twins of the five stages of asm_test_skeleton_stages (include/asm_hip.h): the kernels Dev launches between "dE is on the device" and
"the scaled LP matrix is ready and can be multiplied", and the cases the CPU and GPU tests share.

  assemble    the oracle's own assembly (oracle.subproblem: compute_jacobian_matrix + QpModel.build_lp, the stale-entry rule of the range rows
              included) - no twin of its own; `image` lays a matrix into the Mp x ldn buffer the device keeps, zero padding included
  colscale    k_row_absmax / k_sp_row_absmax, k_col_relmax_stage1/2 / k_sp_col_relmax and the host statement for c, statement by statement: row
              maxima with the 0 -> 1 rule, ONE division per entry, maxima (order-free), pow2_round by frexp
  scale       k_scale_rows / k_sp_scale_rows: t = J_ij c_j, rho_i = pow2_round(max |t|), Ah_ij = t (1 / rho_i)
  products    A x and A'y in long double with the magnitudes sum |a_ij| |x_j| the bars are built from
  norms       row norms in long double

Scaling quantities carry no bar: they are compared for equality.  A sum of L products in any order, with or without FMA, is within
(L + 2) eps sum |a| |x| of the exact value (eps = 2^-52); L is the number of terms a lane or thread chain can see - ldn on the dense row
routes, the entry count of the row or column on the sparse ones, M on the column routes (transposed copy and two-stage reduction).  Norms:
(L + 2) eps ||row||.  All magnitudes of the cases stay inside [2^-400, 2^400]: products with powers of two are exact there and
x (1 / rho) = x / rho; outside that range the behaviour is not specified."""
import functools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
INF = np.inf
T_SQRT_HALF = 0.70710678118654752          # the literal of pow2_round (oracle/lp_solver.py, asm_hip.hip, asm_kernels.hip.h)
TMAXCHUNKS = 128
ROUTE_CSC, ROUTE_COPY, ROUTE_TWO_STAGE = 0, 1, 2
ASSEMBLE, COLSCALE, SCALE, PRODUCTS, NORMS, ALL = 1, 2, 4, 8, 16, 31


def round_up(x, a):
    return (x + a - 1) // a * a


def dims(n, M):
    """ldn, Mp of the skeleton (IpmLayout)."""
    return round_up(n, 32), round_up(max(M, 1), 16)


def chunks(M):
    """R, chunk of the two-stage column reductions (Dev::col_chunks)."""
    R = min((M + 31) // 32, TMAXCHUNKS)
    chunk = (M + R - 1) // R
    return (M + chunk - 1) // chunk, chunk


def image(A, n, M):
    """A (M x n) in the device's Mp x ldn buffer."""
    ldn, Mp = dims(n, M)
    out = np.zeros((Mp, ldn))
    out[:M, :n] = A
    return out


def pow2_round(x):
    x = np.asarray(x, float)
    f, e = np.frexp(np.where(x > 0, x, 1.0))
    return np.where(x > 0, np.ldexp(1.0, np.where(f < T_SQRT_HALF, e - 1, e)), 1.0)


def twin_colscale(J, lb, ub):
    """rmax (M), rel (n), c (n)."""
    M, n = J.shape
    a = np.abs(J)
    rmax = a.max(axis=1, initial=0.0)
    rmax = np.where(rmax > 0.0, rmax, 1.0)
    rel = (a / rmax[:, None]).max(axis=0, initial=0.0)
    c_mat = np.ones(n)
    c_mat[rel > 0.0] = 1.0 / rel[rel > 0.0]
    with np.errstate(invalid="ignore"):
        c = pow2_round(np.minimum(np.maximum(ub, -lb), c_mat))
    return rmax, rel, c


def twin_scale(J, c):
    """rho (M), Ah (M x n)."""
    t = J * c
    rho = pow2_round(np.abs(t).max(axis=1, initial=0.0))
    return rho, t * (1.0 / rho)[:, None]


def pattern_of(case):
    """Structural pattern of the LP matrix (M x n bool): the unique Jacobian entries and their copies in the range rows."""
    m, n = case["m"], case["n"]
    P = np.zeros((m, n), bool)
    P[case["j_row"] - 1, case["j_col"] - 1] = True
    return np.vstack([P, P[case["adj"]]])


def products_ref(A, x, y):
    """(A x, its magnitudes, A'y, its magnitudes) in long double."""
    Al, xl, yl = A.astype(LD), x.astype(LD), y.astype(LD)
    return Al @ xl, np.abs(Al) @ np.abs(xl), Al.T @ yl, np.abs(Al).T @ np.abs(yl)


def product_bars(case, sparse):
    """(L of A x per row, L of A'y per column)."""
    n, M = case["n"], case["M"]
    if sparse:
        P = pattern_of(case)
        return P.sum(axis=1), P.sum(axis=0)
    return np.full(M, dims(n, M)[0]), np.full(n, M)


def norms_ref(J):
    Jl = J.astype(LD)
    return np.sqrt((Jl * Jl).sum(axis=1))


def ratio(out, ref, mag, L):
    """Largest |out - ref| / ((L + 2) eps mag); 0 where both vanish, inf where the bar is zero and the value differs."""
    err = np.abs(np.asarray(out, LD) - ref)
    bar = (np.asarray(L, LD) + 2) * LD(EPS) * mag
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / bar)
    return float(r.max(initial=0.0))


# ----------------------------------------------------------------------------- the oracle's matrices
class Oracle:
    """The oracle's sub-problem model of a case: assembles call after call as the reference does (the range rows keep stale entries)."""

    def __init__(self, case):
        from oracle.subproblem import QpModel
        self.case = case
        self.qp = QpModel(self._data(np.zeros(len(case["j_row"]))), case["j_row"], case["j_col"])

    def _data(self, dE):
        from oracle.subproblem import QpData, compute_jacobian_matrix
        c = self.case
        A, stored = compute_jacobian_matrix(c["m"], c["n"], c["j_row"] - 1, c["j_col"] - 1, dE)
        return QpData(np.zeros(c["n"]), 0.0, A, np.zeros(c["m"]), c["c_lb"], c["c_ub"], -np.ones(c["n"]), np.ones(c["n"]), stored)

    def assemble(self, dE):
        self.qp.data = self._data(dE)
        return self.qp.build_lp(np.zeros(self.case["n"]), 0.5, False).A


def oracle_scale(A, lb, ub):
    """c, rho, Ah of oracle.lp_solver.scale_lp - the specification."""
    from oracle import lp_solver as L
    M, n = A.shape
    s, c, rho, _ = L.scale_lp(L.LP(np.zeros(n), A, np.zeros(M, np.int64), np.zeros(M), lb, ub))
    return c, rho, s.A


# ----------------------------------------------------------------------------- cases
def _row_bounds(m, n_range, rng):
    """Equalities, one-sided rows, and n_range two-sided rows at the end."""
    c_lb = np.full(m, -INF); c_ub = np.full(m, INF)
    kind = rng.integers(0, 3, m)
    c_lb[kind == 0] = 0.0; c_ub[kind == 0] = 0.0
    c_lb[kind == 1] = -0.5
    c_ub[kind == 2] = 0.5
    for i in range(n_range):
        c_lb[m - 1 - i] = -0.25; c_ub[m - 1 - i] = 0.75
    return c_lb, c_ub


def _pattern_full(n, m, rng):
    r, c = np.divmod(np.arange(m * n), n)
    return r, c, 0


def _pattern_general(n, m, rng):
    """Fill about 0.3, a quarter of the entries dealt twice, j_str order shuffled, five range rows."""
    mask = rng.random((m, n)) < 0.3
    mask[np.arange(m), rng.integers(0, n, m)] = True
    r, c = np.nonzero(mask)
    pick = rng.integers(0, len(r), len(r) // 4)
    r = np.concatenate([r, r[pick]]); c = np.concatenate([c, c[pick]])
    p = rng.permutation(len(r))
    return r[p], c[p], 5


COL_DEAL = (0, 1, 7, 8, 9, 17)      # entries per column, in turn: eight lanes per column in k_spmv_t - a tail, an empty column, three sweeps
ROW_DEAL = (0, 1, 2, 5)             # entries per row, in turn, of the first rows


def _pattern_sparse(n, m, rng):
    """Columns [0, nA): COL_DEAL entries each in rows [8, m); rows [0, 8): ROW_DEAL entries each in columns [nA, n); six range rows, among them
    rows of either kind.  nnz 16 <= M n holds with the range copies (asserted by the tests through info)."""
    nA = (n * 2 // 5 if m < 100 else n - 40) // 6 * 6
    r, c = [], []
    for j in range(nA):
        k = COL_DEAL[j % 6]
        r += list(8 + rng.choice(m - 8, k, replace=False)); c += [j] * k
    for i in range(8):
        k = ROW_DEAL[i % 4]
        r += [i] * k; c += list(nA + rng.choice(n - nA, k, replace=False))
    r, c = np.array(r), np.array(c)
    p = rng.permutation(len(r))
    return r[p], c[p], 6


def _threshold_values(rng, size):
    """T 2^e with T the double nearest sqrt(1/2)'s literal or one of its neighbours, either sign."""
    t = np.array([np.nextafter(T_SQRT_HALF, 0.0), T_SQRT_HALF, np.nextafter(T_SQRT_HALF, 1.0)])
    return rng.choice([-1.0, 1.0], size) * np.ldexp(t[rng.integers(0, 3, size)], rng.integers(-20, 21, size))


def values(case, kind, seed):
    """dE, lb, ub of one value class on a case's pattern.  Every class plants, where the shape has room (m, n >= 3): a row whose dE entries
    are all zero, a column whose entries are all zero, an infinite box on a column with entries."""
    rng = np.random.default_rng(seed)
    n, m, r, c = case["n"], case["m"], case["j_row"] - 1, case["j_col"] - 1
    nnz = len(r)
    if kind in ("normal", "holes"):          # negative entries included; holes: four entries in ten are zero - on a handle that has seen
        dE = rng.standard_normal(nnz)        # other values the range rows keep their stale entries, the dense copy of Ah must not
        if kind == "holes":
            dE[rng.random(nnz) < 0.4] = 0.0
        w = rng.uniform(0.1, 3.0, n)
    elif kind == "pow2":          # rows and columns scaled by powers of two between 2^-100 and 2^100
        dE = rng.standard_normal(nnz) * np.ldexp(1.0, rng.integers(-100, 101, m))[r] * np.ldexp(1.0, rng.integers(-100, 101, n))[c]
        w = rng.uniform(0.5, 1.0, n) * np.ldexp(1.0, rng.integers(-100, 101, n))
    elif kind == "threshold":     # entries and box widths on the pow2_round threshold
        dE = _threshold_values(rng, nnz)
        w = np.abs(_threshold_values(rng, n))
    else:
        raise ValueError(kind)
    lb = -w * rng.choice([1.0, 0.5, 0.0], n); ub = w.copy()      # max(ub, -lb) = w
    flip = rng.random(n) < 0.3
    lb[flip], ub[flip] = -ub[flip], -lb[flip]
    if m >= 3 and n >= 3:
        R, chunk = chunks(case["M"])
        edges = sorted({chunk - 1, chunk if R > 1 else chunk - 1, case["M"] - 1})      # of the row chunks of the column reduction
        rows_with = [i for i in np.unique(r) if i not in edges]
        i0 = rows_with[len(rows_with) // 2]
        dE[r == i0] = 0.0
        cols_with = np.unique(c[r != i0])
        j0, j1 = cols_with[len(cols_with) // 3], cols_with[2 * len(cols_with) // 3]
        dE[c == j0] = 0.0
        lb[j1], ub[j1] = -INF, INF
        # the edges of the row chunks of the column reduction: the last row of the first chunk, the first row of the second, the last row of
        # all carry the largest entry of their row in a column of their own - that column's rel = 1 comes from this row alone
        # (a matrix much taller than wide has a row maximum in every column, rel = 1 throughout and nothing to see: there one column is
        # made dominant, so that the other columns' rel is the maximum of a ratio over all rows)
        if case["M"] > 4 * n:
            dE[c == cols_with[0]] *= 2.0 ** 12
        J0 = np.zeros((m, n))
        np.add.at(J0, (r, c), np.abs(dE))
        top = np.abs(J0).argmax(axis=1)
        used = {j0}
        for i in edges:
            taken = used | set(np.delete(top, i).tolist()) if i < m else set()
            ks = [k for k in np.nonzero(r == i)[0] if c[k] not in taken] if i < m and i != i0 else []
            if ks:
                base = dE[ks[0]] if dE[ks[0]] != 0.0 else 1.0          # scaled by a power of two: a threshold value stays one
                total = max(np.abs(dE[r == i]).sum(), abs(base))
                dE[ks[0]] = np.ldexp(base, int(np.ceil(np.log2(8.0 * total / abs(base)))))
                used.add(c[ks[0]])
    return dE, lb, ub


def make_case(name, kind, n, m, seed):
    """kind: 'fast' (full row-major pattern, no range rows), 'general' (dense, duplicates, range rows), 'sparse', 'padded' (the sparse pattern of
    the same n, m, seed with explicit entries added until it is general dense - its dE carries zeros there)."""
    rng = np.random.default_rng(seed)
    build = dict(fast=_pattern_full, general=_pattern_general, sparse=_pattern_sparse, padded=_pattern_sparse)[kind]
    r, c, n_range = build(n, m, rng)
    c_lb, c_ub = (np.zeros(m), np.zeros(m)) if kind == "fast" else _row_bounds(m, n_range, rng)
    n_own = len(r)
    if kind == "padded":          # one explicit entry in eight of the matrix on top: fill above 1/16, never full
        er, ec = np.nonzero(np.random.default_rng(seed + 1).random((m, n)) < 0.125)
        r = np.concatenate([r, er]); c = np.concatenate([c, ec])
    adj = np.nonzero((c_lb < c_ub) & (c_lb > -INF) & (c_ub < INF))[0]
    M = m + len(adj)
    prng = np.random.default_rng(seed + 2)
    return dict(name=name, kind=kind, n=n, m=m, M=M, adj=adj, j_row=r + 1, j_col=c + 1, n_own=n_own, c_lb=c_lb, c_ub=c_ub,
                x=prng.standard_normal(n), y=prng.standard_normal(M), seed=seed)


def case_values(case, vkind, seed=None):
    """values() for a case; a padded case takes the values of its sparse twin and zeros on the added entries."""
    seed = case["seed"] + 10 + VALUE_KINDS.index(vkind) if seed is None else seed
    if case["kind"] != "padded":
        return values(case, vkind, seed)
    own = dict(case, j_row=case["j_row"][:case["n_own"]], j_col=case["j_col"][:case["n_own"]])
    dE, lb, ub = values(own, vkind, seed)
    return np.concatenate([dE, np.zeros(len(case["j_row"]) - case["n_own"])]), lb, ub


SHAPES = [("fast-1x1", "fast", 1, 1), ("fast-31x1", "fast", 31, 1), ("fast-33x17", "fast", 33, 17), ("fast-65x33", "fast", 65, 33),
          ("fast-257x40", "fast", 257, 40), ("general-60x40", "general", 60, 40), ("general-130x70", "general", 130, 70),
          ("sparse-300x70", "sparse", 300, 70), ("sparse-520x260", "sparse", 520, 260),
          ("padded-300x70", "padded", 300, 70), ("padded-520x260", "padded", 520, 260),
          ("chunk-M32", "fast", 40, 32), ("chunk-M33", "fast", 40, 33), ("chunk-M4100", "fast", 40, 4100)]
VALUE_KINDS = ("normal", "pow2", "threshold", "holes")      # run in this order on one handle and one oracle model
EXPECT = {   # info the hook must report: sparse pattern, dense_fast; the routes of J'y and Ah'y
    "fast": (0, 1, ROUTE_TWO_STAGE, ROUTE_COPY), "general": (0, 0, ROUTE_TWO_STAGE, ROUTE_COPY),
    "padded": (0, 0, ROUTE_TWO_STAGE, ROUTE_COPY), "sparse": (1, 0, ROUTE_CSC, ROUTE_CSC)}
CHUNKS = {"chunk-M32": (1, 32), "chunk-M33": (2, 17), "chunk-M4100": (125, 33)}      # R, chunk: one chunk; a second, short one; R capped at 128, then 125 of 33 rows, the last of 8


def get_case(name):
    for i, (nm, kind, n, m) in enumerate(SHAPES):
        if nm == name:
            seed = 100 * (1 + [s[0] for s in SHAPES].index(nm.replace("padded", "sparse")))
            return make_case(nm, kind, n, m, seed)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def runs(name):
    """(case, one dict per value kind in VALUE_KINDS order): the inputs, the oracle's assembled J after this and the earlier runs, and the
    twins' rmax, rel, c, rho, Ah.  Computed once per case and shared; nobody writes into it."""
    case = get_case(name)
    orc = Oracle(case)
    out = []
    for vk in VALUE_KINDS:
        dE, lb, ub = case_values(case, vk)
        J = orc.assemble(dE)
        rmax, rel, c = twin_colscale(J, lb, ub)
        rho, Ah = twin_scale(J, c)
        out.append(dict(vkind=vk, dE=dE, lb=lb, ub=ub, J=J, rmax=rmax, rel=rel, c=c, rho=rho, Ah=Ah))
    return case, out
