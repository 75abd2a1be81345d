"""Problem definitions that feed the SLP hot path (inputs only - no solver logic lives here).

Each builder returns a `Problem` with the data the reference's `Model` (src/model.jl:1-61) receives
from the MOI wrapper (src/MOI_wrapper.jl:1014-1152): dimensions, bounds, the 1-based COO Jacobian
pattern `j_str` in the wrapper's row order (src/MOI_wrapper.jl:683-746), the start point
(src/MOI_wrapper.jl:1113-1130) and the four evaluation callbacks (src/MOI_wrapper.jl:1037-1069).

  toy_problem()            examples/toy_example.jl:12-18 == test/ext_solver.jl:12-18
  toy_expr_problem()       the same toy as the example writes it: affine row, three @NLconstraint rows as expressions
  hs071_problem()          Hock-Schittkowski 71: expression objective and constraints
  synthetic_dense_nlp()    BASELINE.json configs[1]  ("C2")
"""
import numpy as np

INF = np.inf
_MASK = (1 << 64) - 1


class Problem:
    def __init__(self, name, n, m, x_L, x_U, g_L, g_U, j_row, j_col, x0, eval_f, eval_grad_f, eval_g, eval_jac_g):
        self.name = name
        self.n, self.m = int(n), int(m)
        self.x_L, self.x_U = np.asarray(x_L, float), np.asarray(x_U, float)
        self.g_L, self.g_U = np.asarray(g_L, float), np.asarray(g_U, float)
        self.j_row = np.asarray(j_row, np.int64)      # 1-based, duplicates allowed
        self.j_col = np.asarray(j_col, np.int64)
        self.x0 = np.asarray(x0, float)
        self.eval_f, self.eval_grad_f, self.eval_g, self.eval_jac_g = eval_f, eval_grad_f, eval_g, eval_jac_g

    @property
    def nnz(self):
        return len(self.j_row)

    @property
    def j_str(self):
        return list(zip(self.j_row.tolist(), self.j_col.tolist()))


# --------------------------------------------------------------------------- toy (config C1)
def toy_problem():
    """min X^2 + X  s.t.  X >= -2 (affine row, first: src/MOI_wrapper.jl:683-689),
    X^2 - X == 2, X*Y == 1, X*Y >= 0 (NLP block).  Start (0,0).  Reference answer (-1,-1), LOCALLY_SOLVED
    (test/runtests.jl:11-13)."""
    def eval_f(x):
        return x[0] * x[0] + x[0]

    def eval_grad_f(x, g):
        g[0] = 2.0 * x[0] + 1.0
        g[1] = 0.0
        return g

    def eval_g(x, g):
        g[0] = x[0]
        g[1] = x[0] * x[0] - x[0]
        g[2] = x[0] * x[1]
        g[3] = x[0] * x[1]
        return g

    def eval_jac_g(x, v):
        v[0] = 1.0
        v[1] = 2.0 * x[0] - 1.0
        v[2] = x[1]
        v[3] = x[0]
        v[4] = x[1]
        v[5] = x[0]
        return v

    return Problem("toy", 2, 4, [-INF, -INF], [INF, INF], [-2.0, 2.0, 1.0, 0.0], [INF, 2.0, 1.0, INF],
                   [1, 2, 3, 3, 4, 4], [1, 1, 1, 2, 1, 2], [0.0, 0.0], eval_f, eval_grad_f, eval_g, eval_jac_g)


# --------------------------------------------------------------------------- synthetic dense NLP (config C2)
def splitmix64(seed, count):
    """`count` successive SplitMix64 outputs for `seed` (uint64 array)."""
    gamma = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over='ignore'):
        z = np.uint64(seed & _MASK) + gamma * np.arange(1, count + 1, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def uniform01(seed, count):
    """53-bit uniforms in (0,1): ((z >> 11) + 0.5) * 2^-53."""
    z = splitmix64(seed, count)
    return ((z >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def normal01(seed, count):
    """Box-Muller on consecutive uniform pairs (cos branch then sin branch)."""
    k = (count + 1) // 2
    u = uniform01(seed, 2 * k)
    r = np.sqrt(-2.0 * np.log(u[0::2]))
    t = 2.0 * np.pi * u[1::2]
    out = np.empty(2 * k)
    out[0::2] = r * np.cos(t)
    out[1::2] = r * np.sin(t)
    return out[:count]


def synthetic_dense_nlp(n=1000, m=500):
    """g_i(x) = sum_j a_ij x_j + 1/2 q_ij x_j^2  (fully dense Jacobian J_ij = a_ij + q_ij x_j, row-major
    j_str); rows 0..m/2-1 equalities g_i = g_i(x*), the rest `<= g_i(x*) + 0.1`;
    f(x) = c'x + 1/2 sum d_j x_j^2; -1 <= x <= 1; x0 = 0.  Seeds: A 1, Q 2, x* 3, c 4, d 5."""
    A = normal01(1, m * n).reshape(m, n) / np.sqrt(n)
    Q = (0.1 * uniform01(2, m * n)).reshape(m, n) / n
    xs = uniform01(3, n) - 0.5
    c = normal01(4, n)
    d = 0.5 + uniform01(5, n)
    gs = A @ xs + 0.5 * (Q @ (xs * xs))
    h = m // 2
    g_L = np.full(m, -INF)
    g_U = np.full(m, INF)
    g_L[:h] = gs[:h]
    g_U[:h] = gs[:h]
    g_U[h:] = gs[h:] + 0.1
    j_row = np.repeat(np.arange(1, m + 1, dtype=np.int64), n)
    j_col = np.tile(np.arange(1, n + 1, dtype=np.int64), m)

    def eval_f(x):
        return float(c @ x + 0.5 * np.sum(d * x * x))

    def eval_grad_f(x, g):
        g[:] = c + d * x
        return g

    def eval_g(x, g):
        g[:] = A @ x + 0.5 * (Q @ (x * x))
        return g

    def eval_jac_g(x, v):
        v[:] = (A + Q * x).ravel()
        return v

    pr = Problem("synthetic_dense_n%d_m%d" % (n, m), n, m, -np.ones(n), np.ones(n), g_L, g_U, j_row, j_col,
                 np.zeros(n), eval_f, eval_grad_f, eval_g, eval_jac_g)
    pr.data = dict(A=A, Q=Q, c=c, d=d, xs=xs)
    return pr


def synthetic_dense_function_model(n=1000, m=500, hessian=False):
    """The synthetic dense NLP as a FunctionModel: quadratic objective in the affine / quadratic store, the dense rows as an NLP
    block with the `dense_quadratic` device kernel (csrc/asm_eval_kernels.hip.h).  Same problem as `synthetic_dense_nlp`.
    hessian=True: the block also announces its second derivatives (device kind "dense_quadratic_hess", k_nlp_dense_hess): hess g_i is
    diag(Q_i), so the pattern is the n diagonal entries and entry j is sum_i lam_i Q_ij, i ascending from 0.0.
    "dense_quadratic_hess" is the block kernel with its derivative entries: the block also carries data_gradient / data_cross, the
    derivatives with respect to its own dpar (A then Q, row-major; the signatures of nlexpr.ExprBlock's, `scale` unused: the block has
    no objective), the host twins of k_nlp_dense_data_grad and k_nlp_dense_cross_w / _u.  The rows are linear in dpar, so neither
    reads A or Q:  out[A_ij] = (-lam_i) x_j,  out[Q_ij] = (-lam_i) (0.5 (x_j x_j));  along dc = (dA, dQ):  w_i = sum_j dA_ij x_j +
    0.5 dQ_ij x_j^2  and  u_j = -sum_i lam_i (dA_ij + dQ_ij x_j), i ascending from 0.0 (gradient and u bit for bit the device's, w
    to summation order)."""
    from .moi_evaluator import FunctionModel, ScalarFunction, NlpBlock
    pr = synthetic_dense_nlp(n, m)
    d = pr.data
    fm = FunctionModel(n, pr.x_L, pr.x_U)
    fm.objective = ScalarFunction(0.0, [(float(d["c"][j]), j + 1) for j in range(n)], [(float(d["d"][j]), j + 1, j + 1) for j in range(n)])
    dpar = np.concatenate([d["A"].ravel(), d["Q"].ravel()])
    if not hessian:
        fm.nlp = NlpBlock(pr.g_L, pr.g_U, pr.j_row, pr.j_col, pr.eval_g, pr.eval_jac_g, device=("dense_quadratic", np.zeros(1, np.int64), dpar))
        return fm
    Q = np.asarray(d["Q"], float).reshape(m, n)

    def eval_hess(x, obj_factor, lam, values):
        g = np.zeros(n)
        for i in range(m):
            g = g + float(lam[i]) * Q[i]
        values[:n] = g
        return values

    def data_gradient(x, lam, scale=1.0):
        x, w = np.asarray(x, float), -np.asarray(lam, float)
        return np.concatenate([np.outer(w, x).ravel(), np.outer(w, 0.5 * (x * x)).ravel()])

    def data_cross(x, lam, dc, scale=1.0):
        x, lam, dc = np.asarray(x, float), np.asarray(lam, float), np.asarray(dc, float)
        if dc.shape != (2 * m * n,):
            raise ValueError("%d data directions for %d coefficients" % (dc.size, 2 * m * n))
        dA, dQ = dc[:m * n].reshape(m, n), dc[m * n:].reshape(m, n)
        g = np.zeros(n)
        for i in range(m):
            g = g + float(lam[i]) * (dA[i] + dQ[i] * x)
        return -g, (dA * x + 0.5 * dQ * x * x).sum(axis=1)

    def data_cross_t(x, lam, vx, vl, scale=1.0):
        """The transposed cross derivative (k_nlp_dense_cross_t), bit for bit: out[A_ij] = (-lam_i) vx_j + vl_i x_j and out[Q_ij] =
        (-lam_i) (x_j vx_j) + vl_i (0.5 (x_j x_j))."""
        x, w, vx, vl = np.asarray(x, float), -np.asarray(lam, float), np.asarray(vx, float), np.asarray(vl, float)
        return np.concatenate([(np.outer(w, vx) + np.outer(vl, x)).ravel(), (np.outer(w, x * vx) + np.outer(vl, 0.5 * (x * x))).ravel()])
    data_cross.transposed = data_cross_t                    # (how a block carries it: NlpBlock.data_cross_t)
    diag = np.arange(1, n + 1, dtype=np.int64)
    fm.nlp = NlpBlock(pr.g_L, pr.g_U, pr.j_row, pr.j_col, pr.eval_g, pr.eval_jac_g, device=("dense_quadratic_hess", np.zeros(1, np.int64), dpar),
                      hess_rows=diag, hess_cols=diag, eval_hess=eval_hess, data_gradient=data_gradient, data_cross=data_cross)
    return fm


# --------------------------------------------------------------------------- expression models (nlexpr.py, nlp_kind 3)
def toy_expr_function_model():
    """examples/toy_example.jl as written: @objective X^2 + X (a quadratic function of the wrapper), @NLconstraint X^2 - X == 2,
    X*Y == 1, X*Y >= 0 (the expression block) and @constraint X >= -2 (an affine row, first in the wrapper's row order)."""
    from .moi_evaluator import FunctionModel, ScalarFunction
    from .nlexpr import ExprBlock, variables
    X, Y = variables(2)
    fm = FunctionModel(2)
    fm.objective = ScalarFunction(0.0, [(1.0, 1)], [(2.0, 1, 1)])
    fm.add_constraint(ScalarFunction(0.0, [(1.0, 1)]), "ge", -2.0)
    fm.nlp = ExprBlock([(X ** 2 - X, 2.0, 2.0), (X * Y, 1.0, 1.0), (X * Y, 0.0, INF)], n=2)
    return fm


def toy_expr_problem():
    return toy_expr_function_model().to_problem("toy-expr")


def hs071_function_model():
    """Hock-Schittkowski problem 71:  min x1 x4 (x1 + x2 + x3) + x3  s.t.  x1 x2 x3 x4 >= 25,  x1^2 + x2^2 + x3^2 + x4^2 == 40,
    1 <= xi <= 5, start (1, 5, 5, 1).  Objective and both constraints are expressions (an @NLobjective overrides the model's)."""
    from .moi_evaluator import FunctionModel
    from .nlexpr import ExprBlock, variables
    x1, x2, x3, x4 = variables(4)
    fm = FunctionModel(4, np.ones(4), np.full(4, 5.0))
    fm.start = {1: 1.0, 2: 5.0, 3: 5.0, 4: 1.0}
    fm.nlp = ExprBlock([(x1 * x2 * x3 * x4, 25.0, INF), (x1 ** 2 + x2 ** 2 + x3 ** 2 + x4 ** 2, 40.0, 40.0)],
                       objective=x1 * x4 * (x1 + x2 + x3) + x3, n=4)
    return fm


def hs071_problem():
    return hs071_function_model().to_problem("hs071")


def parametric_function_model(a=0.5, p=4.0):
    """A parameterised model with a known solution (nlexpr.parameters at dpar[0] = a, dpar[1] = p):
        min a x1^2 + x2^2 + x1   s.t.  x1 x2 - p >= 0,  x2 - x1 >= 0,  0.5 <= xi <= 10,  start (3, 3).
    For 0 < a < 1 and sqrt(p) (1 - a) > 1/2 both rows are active at the optimum x1 = x2 = sqrt(p) (a vertex, which an SLP reaches in a
    few steps) with multipliers (a + 1 + 1 / (2 sqrt(p)), sqrt(p) (1 - a) - 1/2); the optimal value V = (a + 1) p + sqrt(p) has
    dV/da = p and dV/dp = a + 1 + 1 / (2 sqrt(p)) - what the data gradient of the Lagrangian gives at the solution."""
    from .moi_evaluator import FunctionModel
    from .nlexpr import ExprBlock, parameters, variables
    x1, x2 = variables(2)
    pa, pp = parameters([a, p])
    fm = FunctionModel(2, np.full(2, 0.5), np.full(2, 10.0))
    fm.start = {1: 3.0, 2: 3.0}
    fm.nlp = ExprBlock([(x1 * x2 - pp, 0.0, INF), (x2 - x1, 0.0, INF)], objective=pa * x1 ** 2 + x2 ** 2 + x1, n=2, parameters=[pa, pp])
    return fm


def parametric_solution(a=0.5, p=4.0):
    """(x*, V, dV/d(a, p)) of parametric_function_model."""
    s = float(np.sqrt(p))
    return np.array([s, s]), (a + 1.0) * p + s, np.array([p, a + 1.0 + 0.5 / s])
