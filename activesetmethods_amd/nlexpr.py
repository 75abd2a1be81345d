"""General nonlinear expressions for the NLP block: what the reference's users write as @NLconstraint / @NLobjective, and what
a Julia binding receives from `MOI.constraint_expr` / `MOI.objective_expr` after `MOI.initialize(evaluator, [:ExprGraph])`.

    x = variables(n)                       x[j] is variable j (0-based)
    e = x[0] * x[1] - sin(x[2]) / 2        + - * / unary -, ** int, sin cos exp log sqrt
    e = pow(x[0], 1.5) + abs(x[1] - 1)      abs tan asin acos atan sinh cosh tanh log10 log2 log1p expm1 cbrt, pow(u, v),
                                           atan(y, x), minimum(...), maximum(...)
    ExprBlock(constraints=[(e, lo, hi)], objective=None, n=n)

ExprBlock flattens every row (and every objective term) into the tape of include/asm_hip.h ("Expression block", nlp_kind 3):
nodes (op, a, b) in SSA order, references local to the row, shared sub-expressions emitted once, each variable once per row.
It is an NlpBlock (moi_evaluator.py) whose `device` is ("expr", ipar, dpar) and whose host callbacks interpret the same tape with
the same formulas in the same order as the kernels of csrc/asm_eval_kernels.hip.h (vectorised over rows, one IEEE operation per
node and row): with + - * / unary -, **, abs, minimum and maximum only, host and device agree bit for bit.

The objective, when given, is split into terms along its left spine of additions (((t1 + t2) + t3) -> [t1, t2, t3]) and summed
in term order from 0.0; it replaces the FunctionModel's own objective (`has_objective`, MOI_wrapper.jl:809-861).

Parameters (JuMP-style, for scenario and sensitivity studies): p = parameters([1.0, 2.0]) gives nodes that act as constants whose
values change without a new tape.  ExprBlock(..., parameters=p) puts them at dpar[0:P] in declaration order, never merged with
constants or with each other; set_parameter_values / asm_eval_set_data change them, data_gradient / asm_eval_data_gradient give the
derivative of the Lagrangian with respect to every dpar entry (at an SLP solution: the derivative of the optimal value).

Second derivatives: hessian_structure() / hessian_values(x, obj_factor, lam) are the host twin of the block's part of
asm_eval_hessian_structure / asm_eval_hessian_lagrangian (forward over reverse per (row, seed variable); include/asm_hip.h,
"Hessian of the Lagrangian"); the lists behind them are built when first asked for.

Cross derivatives with respect to the data: data_cross(x, lam, dc) is the host twin of asm_eval_data_cross - the same sweep seeded in
the constants - and gives d/dc (grad_x (f - lam' g)) . dc and (dg/dc) . dc, the right-hand sides of a solution sensitivity
(activesetmethods_amd/sensitivity.py).
"""
import numbers
import struct

import numpy as np

from .moi_evaluator import NlpBlock

# op codes of include/asm_hip.h (ASM_OP_*)
(CONST, VAR, ADD, SUB, MUL, DIV, NEG, POWI, SQRT, EXP, LOG, SIN, COS, ABS, TAN, ASIN, ACOS, ATAN, SINH, COSH, TANH, LOG10, LOG2,
 LOG1P, EXPM1, CBRT, POW, ATAN2, MIN, MAX) = range(30)
OP_COUNT = 30
MAX_POWI = 64
_BINARY = (ADD, SUB, MUL, DIV, POW, ATAN2, MIN, MAX)
LN10, LN2 = 2.302585092994045684, 0.6931471805599453094     # EXPR_LN10 / EXPR_LN2 of the kernels (log(10), log(2) as doubles)


class Expr:
    """A node of an expression graph: op code, operands (Expr), and for CONST the value, for VAR the variable, for POWI the
    exponent."""
    __slots__ = ("op", "args", "arg")
    __array_priority__ = 100                    # numpy scalars on the left defer to Expr's reflected operators

    def __init__(self, op, args=(), arg=None):
        self.op, self.args, self.arg = op, tuple(args), arg

    # ---- operator overloading
    def __add__(self, o): return Expr(ADD, (self, _wrap(o)))
    def __radd__(self, o): return Expr(ADD, (_wrap(o), self))
    def __sub__(self, o): return Expr(SUB, (self, _wrap(o)))
    def __rsub__(self, o): return Expr(SUB, (_wrap(o), self))
    def __mul__(self, o): return Expr(MUL, (self, _wrap(o)))
    def __rmul__(self, o): return Expr(MUL, (_wrap(o), self))
    def __truediv__(self, o): return Expr(DIV, (self, _wrap(o)))
    def __rtruediv__(self, o): return Expr(DIV, (_wrap(o), self))
    def __neg__(self): return Expr(NEG, (self,))
    def __pos__(self): return self
    def __abs__(self): return Expr(ABS, (self,))

    def __pow__(self, e):
        if not isinstance(e, numbers.Integral) or isinstance(e, bool):
            raise TypeError("only integer exponents are supported (x ** k)")
        e = int(e)
        if e == 0:
            return Expr(CONST, arg=1.0)
        if e == 1:
            return self
        if abs(e) > MAX_POWI:
            raise ValueError("exponent magnitude above %d" % MAX_POWI)
        return Expr(POWI, (self,), e)

    def __repr__(self):
        return "Expr(op=%d, arg=%r, %d args)" % (self.op, self.arg, len(self.args))


class Parameter(Expr):
    """A parameter node: a CONST whose dpar slot belongs to it alone (ExprBlock(..., parameters=...) places it)."""
    __slots__ = ()

    def __repr__(self):
        return "Parameter(%r)" % (self.arg,)


def parameters(values):
    """One parameter node per value, in order (their dpar slots are fixed by the ExprBlock that declares them)."""
    return [Parameter(CONST, arg=float(v)) for v in np.atleast_1d(np.asarray(values, np.float64))]


def _wrap(v):
    if isinstance(v, Expr):
        return v
    if isinstance(v, numbers.Real):
        return Expr(CONST, arg=float(v))
    raise TypeError("cannot use %r in an expression" % (v,))


def const(v):
    return Expr(CONST, arg=float(v))


def var(j):
    return Expr(VAR, arg=int(j))


def variables(n):
    return [var(j) for j in range(n)]


def _unary(op):
    def f(u):
        return Expr(op, (_wrap(u),))
    return f


sqrt, exp, log, sin, cos = (_unary(o) for o in (SQRT, EXP, LOG, SIN, COS))
tan, asin, acos, sinh, cosh, tanh, log10, log2, log1p, expm1, cbrt = (
    _unary(o) for o in (TAN, ASIN, ACOS, SINH, COSH, TANH, LOG10, LOG2, LOG1P, EXPM1, CBRT))


def atan(y, x=None):
    """atan(y) or, as Julia's atan(y, x), the angle of (x, y)."""
    if x is None:
        return Expr(ATAN, (_wrap(y),))
    return Expr(ATAN2, (_wrap(y), _wrap(x)))


def pow(u, v):
    """u ^ v for any exponent, a number or an expression (a POW node; ** keeps integer exponents to POWI)."""
    return Expr(POW, (_wrap(u), _wrap(v)))


def _chain(op, args):
    if not args:
        raise TypeError("at least one argument is needed")
    e = _wrap(args[0])
    for v in args[1:]:
        e = Expr(op, (e, _wrap(v)))
    return e


def minimum(*args):
    """min(a, b, c, ...) as a left-to-right chain of MIN nodes (a tie or a NaN takes the left operand and its derivative)."""
    return _chain(MIN, args)


def maximum(*args):
    """max(a, b, c, ...) as a left-to-right chain of MAX nodes."""
    return _chain(MAX, args)


def _split_terms(e):
    terms = []
    while e.op == ADD:
        terms.append(e.args[1])
        e = e.args[0]
    terms.append(e)
    return terms[::-1]


# ---------------------------------------------------------------------------------------------------- tape
class Tape:
    """Rows (constraint rows, then objective terms) as flat arrays: ptr [R+T+1], op / a / b [L] with row-local references, the
    constants in `dpar`: the parameters first (one entry each, in declaration order), then one entry per distinct constant value."""

    def __init__(self, rows, n_constraint_rows, params=()):
        self.R, self.T = n_constraint_rows, len(rows) - n_constraint_rows
        self.consts, cidx = [float(p.arg) for p in params], {}
        pidx = {id(p): i for i, p in enumerate(params)}
        if len(pidx) != len(self.consts):
            raise ValueError("a parameter is declared twice")
        ptr, op, a, b = [0], [], [], []
        for root in rows:
            memo, vidx = {}, {}
            stack = [(root, False)]
            while stack:                                  # post-order without recursion (long sums make deep graphs)
                e, done = stack.pop()
                if id(e) in memo:
                    continue
                if not done:
                    stack.append((e, True))
                    for c in reversed(e.args):
                        if id(c) not in memo:
                            stack.append((c, False))
                    continue
                k = len(op) - ptr[-1]
                if isinstance(e, Parameter):
                    if id(e) not in pidx:
                        raise ValueError("an expression uses a parameter the block does not declare (ExprBlock(..., parameters=...))")
                    op.append(CONST); a.append(pidx[id(e)]); b.append(0)
                elif e.op == CONST:
                    key = struct.pack("<d", e.arg)
                    if key not in cidx:
                        cidx[key] = len(self.consts)
                        self.consts.append(e.arg)
                    op.append(CONST); a.append(cidx[key]); b.append(0)
                elif e.op == VAR:
                    if e.arg in vidx:                     # each variable once per row
                        memo[id(e)] = vidx[e.arg]
                        continue
                    vidx[e.arg] = k
                    op.append(VAR); a.append(e.arg); b.append(0)
                elif e.op in _BINARY:
                    op.append(e.op); a.append(memo[id(e.args[0])]); b.append(memo[id(e.args[1])])
                elif e.op == POWI:
                    op.append(POWI); a.append(memo[id(e.args[0])]); b.append(e.arg)
                else:
                    op.append(e.op); a.append(memo[id(e.args[0])]); b.append(0)
                memo[id(e)] = k
            ptr.append(len(op))
        self.ptr = np.asarray(ptr, np.int64)
        self.op, self.a, self.b = (np.asarray(v, np.int64) for v in (op, a, b))
        self.L = len(op)

    def ipar(self):
        return np.concatenate([[self.R, self.T, self.L], self.ptr, self.op, self.a, self.b]).astype(np.int64)

    def dpar(self):
        return np.asarray(self.consts, np.float64)


def parse_ipar(ipar):
    """(R, T, L, ptr, op, a, b) of an ipar array (no checks: the library validates)."""
    ipar = np.asarray(ipar, np.int64)
    R, T, L = (int(v) for v in ipar[:3])
    ptr = ipar[3:3 + R + T + 1]
    o = 3 + R + T + 1
    return R, T, L, ptr, ipar[o:o + L], ipar[o + L:o + 2 * L], ipar[o + 2 * L:o + 3 * L]


def _powi(u, e):
    """u ** e and its derivative with the factors of expr_powi (asm_eval_kernels.hip.h)."""
    k = abs(e)
    p = np.ones_like(u)
    for _ in range(1, k):
        p = p * u
    pk = p * u
    if e > 0:
        return pk, float(e) * p
    return 1.0 / pk, float(e) / (pk * u)


def _atan2_scaled(u, y):
    """(s, us, ys, ts) of ExprAtan2 (asm_eval_kernels.hip.h): u and y scaled by the power of two s that puts the larger magnitude in
    [1/2, 1), ts = us us + ys ys; ((w ys) / ts) s is (w y) / (u u + y y) without the underflow or overflow of the squares."""
    e = np.frexp(np.fmax(np.abs(u), np.abs(y)))[1]
    s = np.ldexp(1.0, np.where(e < -1000, 1000, np.where(e > 1000, -1000, -e)))
    us, ys = u * s, y * s
    return s, us, ys, us * us + ys * ys


_NP_UNARY = {ABS: np.abs, TAN: np.tan, ASIN: np.arcsin, ACOS: np.arccos, ATAN: np.arctan, SINH: np.sinh, COSH: np.cosh,
             TANH: np.tanh, LOG10: np.log10, LOG2: np.log2, LOG1P: np.log1p, EXPM1: np.expm1, CBRT: np.cbrt}


class _Sweep:
    """The host twin of expr_forward / expr_reverse for a group of rows: rows padded to the longest, node position k evaluated
    for all rows at once, grouped by op (each node of each row is still the one IEEE operation the kernel performs)."""

    def __init__(self, ptr, op, a, b, slot, lens=None):
        """Rows ptr[r] .. ptr[r + 1]; with `lens`, row r is the nodes ptr[r] .. ptr[r] + lens[r] (rows may then repeat)."""
        if lens is None:
            lens = np.diff(ptr)
        self.nr = len(lens)
        self.lens = lens
        self.K = int(lens.max()) if self.nr else 0
        self.last = lens - 1
        self.steps = []
        for k in range(self.K):
            rows = np.nonzero(lens > k)[0]
            g = ptr[rows] + k
            ops = op[g]
            groups = []
            for o in np.unique(ops):
                sel = ops == o
                r = rows[sel]
                groups.append((int(o), r, a[g[sel]], b[g[sel]], slot[g[sel]]))
            self.steps.append(groups)

    def forward(self, x, consts):
        V = np.zeros((self.nr, max(self.K, 1)))
        with np.errstate(all="ignore"):
            for k, groups in enumerate(self.steps):
                for o, r, a, b, _ in groups:
                    if o == CONST:
                        v = consts[a]
                    elif o == VAR:
                        v = x[a]
                    elif o == ADD:
                        v = V[r, a] + V[r, b]
                    elif o == SUB:
                        v = V[r, a] - V[r, b]
                    elif o == MUL:
                        v = V[r, a] * V[r, b]
                    elif o == DIV:
                        v = V[r, a] / V[r, b]
                    elif o == NEG:
                        v = -V[r, a]
                    elif o == POWI:
                        v = np.empty(len(r))
                        for e in np.unique(b):
                            s = b == e
                            v[s] = _powi(V[r[s], a[s]], int(e))[0]
                    elif o == SQRT:
                        v = np.sqrt(V[r, a])
                    elif o == EXP:
                        v = np.exp(V[r, a])
                    elif o == LOG:
                        v = np.log(V[r, a])
                    elif o == SIN:
                        v = np.sin(V[r, a])
                    elif o == COS:
                        v = np.cos(V[r, a])
                    elif o in _NP_UNARY:
                        v = _NP_UNARY[o](V[r, a])
                    elif o == POW:
                        v = np.power(V[r, a], V[r, b])
                    elif o == ATAN2:
                        v = np.arctan2(V[r, a], V[r, b])
                    elif o == MIN:
                        u, y = V[r, a], V[r, b]
                        v = np.where(y < u, y, u)
                    else:                                 # MAX
                        u, y = V[r, a], V[r, b]
                        v = np.where(y > u, y, u)
                    V[r, k] = v
        return V, V[np.arange(self.nr), self.last]

    def reverse(self, V, out, accumulate, weight=None):
        """Adjoints from the last node of every row back; VAR-node adjoints added to (or stored into) out[slot].  With `weight`
        (one per row; the data gradient, expr_reverse<EXPR_DATA>): weight[row] * the adjoint of every CONST node stored into
        out[slot], nothing for the VAR nodes."""
        W = np.zeros_like(V)
        W[np.arange(self.nr), self.last] = 1.0
        with np.errstate(all="ignore"):
            for k in range(self.K - 1, -1, -1):
                for o, r, a, b, slot in self.steps[k]:
                    w = W[r, k]
                    if o == CONST:
                        if weight is not None:
                            out[slot] = weight[r] * w
                        continue
                    if o == VAR:
                        if weight is None:
                            out[slot] = out[slot] + w if accumulate else w
                    elif o == ADD:
                        W[r, a] = W[r, a] + w
                        W[r, b] = W[r, b] + w
                    elif o == SUB:
                        W[r, a] = W[r, a] + w
                        W[r, b] = W[r, b] - w
                    elif o == MUL:
                        va, vb = V[r, a], V[r, b]
                        W[r, a] = W[r, a] + w * vb
                        W[r, b] = W[r, b] + w * va
                    elif o == DIV:
                        t = w / V[r, b]
                        W[r, a] = W[r, a] + t
                        W[r, b] = W[r, b] - t * V[r, k]
                    elif o == NEG:
                        W[r, a] = W[r, a] - w
                    elif o == POWI:
                        d = np.empty(len(r))
                        for e in np.unique(b):
                            s = b == e
                            d[s] = _powi(V[r[s], a[s]], int(e))[1]
                        W[r, a] = W[r, a] + w * d
                    elif o == SQRT:
                        W[r, a] = W[r, a] + (0.5 * w) / V[r, k]
                    elif o == EXP:
                        W[r, a] = W[r, a] + w * V[r, k]
                    elif o == LOG:
                        W[r, a] = W[r, a] + w / V[r, a]
                    elif o == SIN:
                        W[r, a] = W[r, a] + w * np.cos(V[r, a])
                    elif o == COS:
                        W[r, a] = W[r, a] - w * np.sin(V[r, a])
                    elif o == ABS:
                        W[r, a] = W[r, a] + w * np.copysign(1.0, V[r, a])
                    elif o == TAN:
                        v = V[r, k]
                        W[r, a] = W[r, a] + w * (1.0 + v * v)
                    elif o == ASIN:
                        u = V[r, a]
                        W[r, a] = W[r, a] + w / np.sqrt((1.0 - u) * (1.0 + u))
                    elif o == ACOS:
                        u = V[r, a]
                        W[r, a] = W[r, a] - w / np.sqrt((1.0 - u) * (1.0 + u))
                    elif o == ATAN:
                        u = V[r, a]
                        W[r, a] = W[r, a] + w / (1.0 + u * u)
                    elif o == SINH:
                        W[r, a] = W[r, a] + w * np.cosh(V[r, a])
                    elif o == COSH:
                        W[r, a] = W[r, a] + w * np.sinh(V[r, a])
                    elif o == TANH:
                        v = V[r, k]
                        W[r, a] = W[r, a] + w * (1.0 - v * v)
                    elif o == LOG10:
                        W[r, a] = W[r, a] + w / (V[r, a] * LN10)
                    elif o == LOG2:
                        W[r, a] = W[r, a] + w / (V[r, a] * LN2)
                    elif o == LOG1P:
                        W[r, a] = W[r, a] + w / (1.0 + V[r, a])
                    elif o == EXPM1:
                        W[r, a] = W[r, a] + w * (V[r, k] + 1.0)
                    elif o == CBRT:
                        v = V[r, k]
                        W[r, a] = W[r, a] + w / (3.0 * (v * v))
                    elif o == POW:
                        u, y = V[r, a], V[r, b]
                        W[r, a] = W[r, a] + w * (y * np.power(u, y - 1.0))
                        W[r, b] = W[r, b] + w * (V[r, k] * np.log(u))
                    elif o == ATAN2:
                        s, us, ys, ts = _atan2_scaled(V[r, a], V[r, b])
                        W[r, a] = W[r, a] + ((w * ys) / ts) * s
                        W[r, b] = W[r, b] - ((w * us) / ts) * s
                    else:                                 # MIN, MAX: all of w to the chosen operand (ties and NaN: a)
                        u, y = V[r, a], V[r, b]
                        c = np.where(y < u if o == MIN else y > u, b, a)
                        W[r, c] = W[r, c] + w


def _powi2(u, e):
    """u ** e, its first and its second derivative with the factors of expr_powi2 (asm_eval_kernels.hip.h)."""
    k = abs(e)
    p, q = np.ones_like(u), np.ones_like(u)
    for _ in range(1, k):
        q = p
        p = p * u
    pk = p * u
    ee = float(e) * float(e - 1)
    if e > 0:
        return pk, float(e) * p, (ee * q if k > 1 else np.zeros_like(u))
    pu = pk * u
    return 1.0 / pk, float(e) / pu, ee / (pu * u)


def interaction_pairs(op, a, b):
    """The interaction set P(last node) of one row (row-local references) as a set of (i, j), i >= j: the pattern rule of
    include/asm_hip.h ("Hessian of the Lagrangian"), node by node."""
    L, P = [], []
    for o, ka, kb in zip(op.tolist(), a.tolist(), b.tolist()):
        sq = lambda A, B: {(max(i, j), min(i, j)) for i in A for j in B}
        if o == CONST:
            L.append(frozenset()); P.append(frozenset())
        elif o == VAR:
            L.append(frozenset([ka])); P.append(frozenset())
        elif o in (ADD, SUB, MIN, MAX):
            L.append(L[ka] | L[kb]); P.append(P[ka] | P[kb])
        elif o == NEG or (o == POWI and kb == 1):
            L.append(L[ka]); P.append(P[ka])
        elif o == MUL:
            L.append(L[ka] | L[kb]); P.append(P[ka] | P[kb] | sq(L[ka], L[kb]))
        elif o == DIV:
            L.append(L[ka] | L[kb]); P.append(P[ka] | P[kb] | sq(L[ka], L[kb]) | sq(L[kb], L[kb]))
        elif o in (POW, ATAN2):
            L.append(L[ka] | L[kb]); P.append(frozenset(sq(L[-1], L[-1])))
        else:                                         # every other unary op, POWI
            L.append(L[ka]); P.append(P[ka] | sq(L[ka], L[ka]))
    return set(P[-1])


class _HessSweep(_Sweep):
    """The host twin of expr_forward2 / expr_reverse2: one "row" per seed thread (a row or term of the tape with one seed variable),
    node position k evaluated for all threads at once.  start / lens: the thread's nodes in the tape; seed: its seed variable;
    okey: thread * n + variable of every occurrence, ascending (its index is the occurrence's place in hocc)."""

    def __init__(self, start, lens, op, a, b, seed, okey, n):
        super().__init__(start, op, a, b, np.zeros(len(op), np.int64), lens=lens)
        self.start = start
        self.aux = []
        for groups in self.steps:
            aux = []
            for o, r, ka, kb, _ in groups:
                if o == VAR:
                    key = r * n + ka
                    pos = np.minimum(np.searchsorted(okey, key), max(len(okey) - 1, 0))
                    hit = (okey[pos] == key) if len(okey) else np.zeros(len(r), bool)
                    aux.append(((ka == seed[r]).astype(np.float64), r[hit], pos[hit]))
                elif o == POW:
                    aux.append(op[start[r] + kb] == CONST)
                else:
                    aux.append(None)
            self.aux.append(aux)

    def forward2(self, x, consts, dc=None, vx=None):
        """Values V and tangents D.  With `dc` (the data cross derivatives, expr_forward2<EXPR2_DATA>): the seed is that direction in
        the constants - a CONST node with operand a has the tangent dc[a], every VAR node 0.  With `vx` (the transposed cross
        derivatives, EXPR2_DATA_T): a direction in the variables - a VAR node of variable a has the tangent vx[a], every CONST node 0."""
        V = np.zeros((self.nr, max(self.K, 1)))
        D = np.zeros_like(V)
        with np.errstate(all="ignore"):
            for k, groups in enumerate(self.steps):
                for (o, r, a, b, _), aux in zip(groups, self.aux[k]):
                    if o == CONST:
                        V[r, k] = consts[a]
                        if dc is not None:
                            D[r, k] = dc[a]
                        continue
                    if o == VAR:
                        V[r, k], D[r, k] = x[a], (vx[a] if vx is not None else aux[0] if dc is None else 0.0)
                        continue
                    u, du = V[r, a], D[r, a]
                    if o in _BINARY:
                        y, dy = V[r, b], D[r, b]
                    if o == ADD:
                        v, d = u + y, du + dy
                    elif o == SUB:
                        v, d = u - y, du - dy
                    elif o == MUL:
                        v, d = u * y, du * y + u * dy
                    elif o == DIV:
                        v = u / y
                        d = (du - v * dy) / y
                    elif o == NEG:
                        v, d = -u, -du
                    elif o == POWI:
                        v, d = np.empty(len(r)), np.empty(len(r))
                        for e in np.unique(b):
                            s = b == e
                            v[s], d1, _ = _powi2(u[s], int(e))
                            d[s] = d1 * du[s]
                    elif o == SQRT:
                        v = np.sqrt(u)
                        d = (0.5 * du) / v
                    elif o == EXP:
                        v = np.exp(u)
                        d = du * v
                    elif o == LOG:
                        v, d = np.log(u), du / u
                    elif o == SIN:
                        v, d = np.sin(u), du * np.cos(u)
                    elif o == COS:
                        v, d = np.cos(u), -(du * np.sin(u))
                    elif o == ABS:
                        v, d = np.abs(u), du * np.copysign(1.0, u)
                    elif o == MIN or o == MAX:
                        c = y < u if o == MIN else y > u
                        v, d = np.where(c, y, u), np.where(c, dy, du)
                    elif o == POW:
                        v = np.power(u, y)
                        d = du * (y * np.power(u, y - 1.0))
                        # a CONST exponent has a tangent with `dc` alone; its term enters only where that is nonzero
                        d = np.where(aux & (dy == 0.0) if dc is not None else aux, d, d + dy * (v * np.log(u)))
                    elif o == ATAN2:
                        v = np.arctan2(u, y)
                        s, us, ys, ts = _atan2_scaled(u, y)
                        d = ((du * ys) / ts) * s - ((dy * us) / ts) * s
                    else:
                        v = _NP_UNARY[o](u)
                        if o == TAN:
                            d = du * (1.0 + v * v)
                        elif o == ASIN:
                            d = du / np.sqrt((1.0 - u) * (1.0 + u))
                        elif o == ACOS:
                            d = -(du / np.sqrt((1.0 - u) * (1.0 + u)))
                        elif o == ATAN:
                            d = du / (1.0 + u * u)
                        elif o == SINH:
                            d = du * np.cosh(u)
                        elif o == COSH:
                            d = du * np.sinh(u)
                        elif o == TANH:
                            d = du * (1.0 - v * v)
                        elif o == LOG10:
                            d = du / (u * LN10)
                        elif o == LOG2:
                            d = du / (u * LN2)
                        elif o == LOG1P:
                            d = du / (1.0 + u)
                        elif o == EXPM1:
                            d = du * (v + 1.0)
                        else:                             # CBRT
                            d = du / (3.0 * (v * v))
                    V[r, k], D[r, k] = v, d
        return V, D

    def reverse2(self, V, D, hocc, weight=None, cslot=None, wadj=None, both=None):
        """Adjoints W and their tangents Z from the last node of every thread back; the adjoint tangent of a VAR node whose
        variable is in the thread's occurrence list is added to hocc there.  With `weight` (one per thread; expr_reverse2<EXPR2_DATA>):
        every VAR node is an occurrence of its own, hocc[node in the tape] = weight * its adjoint tangent.  With `cslot` as well (the
        slot of every node of the tape; EXPR2_DATA_T): the CONST nodes are the occurrences instead, hocc[cslot[node]] = weight *
        adjoint tangent + wadj * adjoint for the threads named in `both`, weight * adjoint tangent alone for the others."""
        W = np.zeros_like(V)
        Z = np.zeros_like(V)
        W[np.arange(self.nr), self.last] = 1.0
        with np.errstate(all="ignore"):
            for k in range(self.K - 1, -1, -1):
                for (o, r, a, b, _), aux in zip(self.steps[k], self.aux[k]):
                    if o == CONST:
                        if cslot is not None:
                            t1 = weight[r] * Z[r, k]
                            hocc[cslot[self.start[r] + k]] = np.where(both[r], t1 + wadj[r] * W[r, k], t1)
                        continue
                    w, z = W[r, k], Z[r, k]
                    if o == VAR:
                        if cslot is not None:
                            continue
                        if weight is not None:
                            hocc[self.start[r] + k] = weight[r] * z
                            continue
                        _, rh, pos = aux
                        hocc[pos] = hocc[pos] + Z[rh, k]
                        continue
                    u, du, v, d = V[r, a], D[r, a], V[r, k], D[r, k]
                    if o in _BINARY:
                        y, dy = V[r, b], D[r, b]

                    def add(c, dw, dz):
                        W[r, c] = W[r, c] + dw
                        Z[r, c] = Z[r, c] + dz

                    def sub(c, dw, dz):
                        W[r, c] = W[r, c] - dw
                        Z[r, c] = Z[r, c] - dz
                    if o == ADD:
                        add(a, w, z); add(b, w, z)
                    elif o == SUB:
                        add(a, w, z); sub(b, w, z)
                    elif o == MUL:
                        add(a, w * y, z * y + w * dy)
                        add(b, w * u, z * u + w * du)
                    elif o == DIV:
                        t = w / y
                        dt = (z - t * dy) / y
                        add(a, t, dt)
                        sub(b, t * v, dt * v + t * d)
                    elif o == NEG:
                        sub(a, w, z)
                    elif o == POWI:
                        d1, d2 = np.empty(len(r)), np.empty(len(r))
                        for e in np.unique(b):
                            s = b == e
                            _, d1[s], d2[s] = _powi2(u[s], int(e))
                        add(a, w * d1, z * d1 + w * (d2 * du))
                    elif o == SQRT:
                        s = (0.5 * w) / v
                        add(a, s, (0.5 * z - s * d) / v)
                    elif o == EXP:
                        add(a, w * v, z * v + w * d)
                    elif o == LOG:
                        q = w / u
                        add(a, q, (z - q * du) / u)
                    elif o == SIN:
                        c, s = np.cos(u), np.sin(u)
                        add(a, w * c, z * c - w * (s * du))
                    elif o == COS:
                        c, s = np.cos(u), np.sin(u)
                        sub(a, w * s, z * s + w * (c * du))
                    elif o == ABS:
                        s = np.copysign(1.0, u)
                        add(a, w * s, z * s)
                    elif o == TAN:
                        g = 1.0 + v * v
                        add(a, w * g, z * g + w * (2.0 * (v * d)))
                    elif o == ASIN or o == ACOS:
                        rt = np.sqrt((1.0 - u) * (1.0 + u))
                        q = w / rt
                        dr = -((u * du) / rt)
                        (add if o == ASIN else sub)(a, q, (z - q * dr) / rt)
                    elif o == ATAN:
                        g = 1.0 + u * u
                        q = w / g
                        add(a, q, (z - q * (2.0 * (u * du))) / g)
                    elif o == SINH:
                        c, s = np.cosh(u), np.sinh(u)
                        add(a, w * c, z * c + w * (s * du))
                    elif o == COSH:
                        c, s = np.cosh(u), np.sinh(u)
                        add(a, w * s, z * s + w * (c * du))
                    elif o == TANH:
                        g = 1.0 - v * v
                        add(a, w * g, z * g - w * (2.0 * (v * d)))
                    elif o == LOG10 or o == LOG2:
                        ln = LN10 if o == LOG10 else LN2
                        g = u * ln
                        q = w / g
                        add(a, q, (z - q * (du * ln)) / g)
                    elif o == LOG1P:
                        g = 1.0 + u
                        q = w / g
                        add(a, q, (z - q * du) / g)
                    elif o == EXPM1:
                        g = v + 1.0
                        add(a, w * g, z * g + w * d)
                    elif o == CBRT:
                        g = 3.0 * (v * v)
                        q = w / g
                        add(a, q, (z - q * (6.0 * (v * d))) / g)
                    elif o == POW:
                        # bc: no term with dy; nb: nothing to b (expr_reverse2).  Hessian: a CONST exponent has neither.  EXPR2_DATA: its
                        # terms enter where its tangent dc[a] is nonzero.  EXPR2_DATA_T: its tangent is 0, and it receives W and Z
                        bc = nb = aux
                        if cslot is not None:
                            nb = np.zeros_like(aux)
                        elif weight is not None:
                            bc = nb = aux & (dy == 0.0)
                        p1, p2, lu = np.power(u, y - 1.0), np.power(u, y - 2.0), np.log(u)
                        A = y * p1
                        dp1 = du * ((y - 1.0) * p2)
                        dp1 = np.where(bc, dp1, dp1 + dy * (p1 * lu))
                        dA = y * dp1
                        dA = np.where(bc, dA, dA + dy * p1)
                        add(a, w * A, z * A + w * dA)
                        B = v * lu
                        dB = d * lu + v * (du / u)
                        tb = ~nb
                        rb, cb = r[tb], b[tb]
                        W[rb, cb] = W[rb, cb] + (w * B)[tb]
                        Z[rb, cb] = Z[rb, cb] + (z * B + w * dB)[tb]
                    elif o == ATAN2:
                        s, us, ys, ts = _atan2_scaled(u, y)
                        dts = 2.0 * (us * du) + 2.0 * (ys * dy)
                        qa, qb = ((w * ys) / ts) * s, ((w * us) / ts) * s
                        add(a, qa, (((z * ys + (w * dy) * s) - qa * dts) / ts) * s)
                        sub(b, qb, (((z * us + (w * du) * s) - qb * dts) / ts) * s)
                    else:                                 # MIN, MAX
                        c = np.where(y < u if o == MIN else y > u, b, a)
                        add(c, w, z)


class ExprBlock(NlpBlock):
    """An NLP block of expressions: `constraints` = [(expr, lo, hi)] (lo == hi: equality; +-inf: one-sided), `objective` = an
    expression or None, `parameters` = the parameter nodes (nlexpr.parameters) the expressions use, at dpar[0:P] in this order.
    Rows of the Jacobian pattern: each row's distinct variables in ascending order (1-based block rows and columns, as NlpBlock)."""

    def __init__(self, constraints=(), objective=None, n=None, parameters=()):
        cons = [(_wrap(e), float(lo), float(hi)) for e, lo, hi in constraints]
        terms = _split_terms(_wrap(objective)) if objective is not None else []
        params = list(parameters)
        if not all(isinstance(p, Parameter) for p in params):
            raise TypeError("parameters must be nodes made by nlexpr.parameters")
        tape = Tape([e for e, _, _ in cons] + terms, len(cons), params)
        self.n_params = len(params)
        self.params = params                               # the parameter nodes, in dpar order
        self.exprs = [e for e, _, _ in cons] + terms      # the graphs behind the tape: constraint rows, then objective terms
        self.tape = tape
        R, T = tape.R, tape.T
        ptr, op, a = tape.ptr, tape.op, tape.a
        if n is not None and np.any(a[op == VAR] >= n):
            raise ValueError("a variable index is out of range for n = %d" % n)
        # pattern and slots: rows -> position in the block's Jacobian values; terms -> position in the per-variable gradient lists
        slot = np.full(tape.L, -1, np.int64)
        rows, cols = [], []
        for r in range(R):
            k = np.arange(ptr[r], ptr[r + 1])
            kv = k[op[k] == VAR]
            vs = np.unique(a[kv])
            slot[kv] = len(cols) + np.searchsorted(vs, a[kv])
            rows += [r + 1] * len(vs)
            cols += (vs + 1).tolist()
        n_var = int(n) if n is not None else (int(a[op == VAR].max()) + 1 if np.any(op == VAR) else 0)
        kt = np.arange(ptr[R], tape.L)
        kv = kt[op[kt] == VAR]
        order = np.lexsort((kv, a[kv]))                    # by variable, then (term, node) = node order
        slot[kv[order]] = np.arange(len(kv))
        self.g_ptr = np.concatenate([[0], np.cumsum(np.bincount(a[kv], minlength=n_var))]).astype(np.int64)
        # data gradient: the CONST nodes grouped by dpar index, node order inside a group (the cptr / slot of asm_eval_setup)
        kc = np.nonzero(op == CONST)[0]
        slot[kc[np.argsort(a[kc], kind="stable")]] = np.arange(len(kc))
        self.c_ptr = np.concatenate([[0], np.cumsum(np.bincount(a[kc], minlength=len(tape.consts)))]).astype(np.int64)
        self.n_var = n_var
        self._consts = tape.dpar()
        self._slot = slot
        self._rows = _Sweep(ptr[:R + 1], op, tape.a, tape.b, slot)
        self._terms = _Sweep(ptr[R:] - ptr[R], op[ptr[R]:], tape.a[ptr[R]:], tape.b[ptr[R]:], slot[ptr[R]:])
        self._n_occ = len(kv)
        self._hess = None                                  # second-order lists: made when a Hessian is first asked for
        self._cross = None                                 # the same for the data cross derivatives
        super().__init__([lo for _, lo, _ in cons], [hi for _, _, hi in cons], rows, cols, self._eval_g, self._eval_jac_g,
                         device=("expr", tape.ipar(), self._consts),
                         has_objective=T > 0, eval_f=self._eval_f if T > 0 else None, eval_grad_f=self._eval_grad_f if T > 0 else None,
                         eval_hess=self._eval_hess)

    # ---- Hessian of the Lagrangian (the twin of asm_eval_hessian_*'s block part: k_nlp_expr_hess, k_nlp_expr_hess_gather)
    def _hess_prepare(self):
        if self._hess is None:
            tape, n = self.tape, max(self.n_var, 1)
            ptr, op, a, b = tape.ptr, tape.op, tape.a, tape.b
            start, lens, seed, srow, okey, pairs = [], [], [], [], [], []
            for t in range(tape.R + tape.T):
                k0, k1 = int(ptr[t]), int(ptr[t + 1])
                new = True
                for j, i in sorted((j, i) for i, j in interaction_pairs(op[k0:k1], a[k0:k1], b[k0:k1])):
                    if new or seed[-1] != j:                # one seed thread per smaller index j of the row's pairs
                        start.append(k0); lens.append(k1 - k0); seed.append(j); srow.append(t)
                        new = False
                    okey.append((len(seed) - 1) * n + i)
                    pairs.append(i * n + j)
            i64 = lambda v: np.asarray(v, np.int64)
            okey, pairs, srow = i64(okey), i64(pairs), i64(srow)
            keys = np.unique(pairs)                        # the entries: distinct (i, j), i >= j, sorted by (i, j)
            oent = np.searchsorted(keys, pairs)
            self._hess = dict(sweep=_HessSweep(i64(start), i64(lens), op, a, b, i64(seed), okey, n), srow=srow, othread=okey // n,
                              rows=keys // n + 1, cols=keys % n + 1, eocc=np.argsort(oent, kind="stable"),
                              eptr=np.concatenate([[0], np.cumsum(np.bincount(oent, minlength=len(keys)))]).astype(np.int64))
            self.hess_rows, self.hess_cols = self._hess["rows"], self._hess["cols"]
        return self._hess

    def hessian_structure(self):
        """(rows, cols), 1-based: the distinct pairs (i, j), i >= j, sorted by (i, j), of the rows' and terms' interaction sets."""
        H = self._hess_prepare()
        return H["rows"], H["cols"]

    def hessian_values(self, x, obj_factor, lam):
        """Values of the block's entries of obj_factor * hess(sum of the terms) + sum_r lam[r] hess g_r (`lam`: the multipliers of the
        block's rows; `obj_factor` with the sense scale already in it).  Per (row or term, seed variable j) a forward sweep with
        tangent and a reverse sweep with adjoint tangents; every entry sums weight * h over its rows, then terms, from 0.0."""
        H = self._hess_prepare()
        x, lam = np.asarray(x, float), np.asarray(lam, float)
        R, sweep, srow = self.tape.R, H["sweep"], H["srow"]
        hocc = np.zeros(len(H["othread"]))
        if sweep.nr:
            V, D = sweep.forward2(x, self._consts)
            sweep.reverse2(V, D, hocc)
            wt = np.where(srow < R, lam[np.minimum(srow, R - 1)] if R else 0.0, float(obj_factor))
            hocc = wt[H["othread"]] * hocc
        eptr, eocc = H["eptr"], H["eocc"]
        cnt = np.diff(eptr)
        vals = np.zeros(len(cnt))
        for i in range(int(cnt.max()) if len(cnt) else 0):
            s = cnt > i
            vals[s] = vals[s] + hocc[eocc[eptr[:-1][s] + i]]
        return vals

    def _eval_hess(self, x, obj_factor, lam, values):
        values[:] = self.hessian_values(x, obj_factor, lam)
        return values

    # ---- parameters
    def set_parameter_values(self, values):
        """New values of the P parameters (declaration order): the host callbacks and the `device` tuple use them from now on."""
        v = np.asarray(values, np.float64).ravel()
        if len(v) != self.n_params:
            raise ValueError("%d parameter values for %d parameters" % (len(v), self.n_params))
        consts = self._consts.copy()
        consts[:self.n_params] = v
        self._consts = consts
        self.device = ("expr", self.device[1], consts)

    def data_gradient(self, x, lam, scale=1.0):
        """Host twin of asm_eval_data_gradient: d(scale * f - lam' g) / d dpar[c] for every dpar entry c, with `lam` the multipliers
        of the block's rows and `scale` the objective's sense scale.  The occurrences of every constant - (-lam[r]) * adjoint in a row
        r, scale * adjoint in a term - are summed from 0.0 in (row, then term; node) order, as k_nlp_expr_data_gather does."""
        x = np.asarray(x, float)
        lam = np.asarray(lam, float)
        R = self.tape.R
        cocc = np.zeros(int(self.c_ptr[-1]))
        if R:
            V, _ = self._rows.forward(x, self._consts)
            self._rows.reverse(V, cocc, False, weight=-lam[:R])
        if self.tape.T:
            V, _ = self._terms.forward(x, self._consts)
            self._terms.reverse(V, cocc, False, weight=np.full(self.tape.T, float(scale)))
        cnt = np.diff(self.c_ptr)
        g = np.zeros(len(cnt))
        for i in range(int(cnt.max()) if len(cnt) else 0):
            s = cnt > i
            g[s] = g[s] + cocc[self.c_ptr[:-1][s] + i]
        return g

    def data_cross(self, x, lam, dc, scale=1.0):
        """Host twin of asm_eval_data_cross: (u, w) with u [n_var] = d/d dpar (grad_x (scale * f - lam' g)) . dc and w [R] =
        (d g / d dpar) . dc, `lam` the multipliers of the block's rows, `dc` a direction in dpar.  Per row or term the forward-over-
        reverse sweep of the Hessian seeded in the constants; the adjoint tangent of every VAR node, times -lam[r] in a row r and
        `scale` in a term, is an occurrence; u[j] sums those of variable j from 0.0, rows before terms, nodes descending inside one
        (k_nlp_expr_cross, k_nlp_expr_cross_gather)."""
        tape = self.tape
        R, T, L = tape.R, tape.T, tape.L
        x, lam, dc = np.asarray(x, float), np.asarray(lam, float), np.asarray(dc, float)
        if len(dc) != len(self._consts):
            raise ValueError("%d data directions for %d constants" % (len(dc), len(self._consts)))
        if self._cross is None:
            ptr, op, a = tape.ptr, tape.op, tape.a
            kv = np.nonzero(op == VAR)[0]
            row = np.searchsorted(ptr, kv, side="right") - 1
            order = np.lexsort((-kv, row, a[kv]))          # by variable, then row / term, then node descending
            n_var = max(self.n_var, 1)
            vptr = np.concatenate([[0], np.cumsum(np.bincount(a[kv], minlength=n_var))]).astype(np.int64)
            sweep = _HessSweep(ptr[:-1].copy(), np.diff(ptr), op, a, tape.b, np.full(R + T, -1, np.int64), np.zeros(0, np.int64), n_var)
            self._cross = (sweep, vptr, kv[order])
        sweep, vptr, vnode = self._cross
        u, w = np.zeros(len(vptr) - 1), np.zeros(R)
        if not np.any(tape.op == CONST) or R + T == 0:
            return u[:self.n_var], w
        V, D = sweep.forward2(x, self._consts, dc=dc)
        w[:] = D[np.arange(R), sweep.last[:R]]
        vocc = np.zeros(L)
        sweep.reverse2(V, D, vocc, weight=np.concatenate([-lam[:R], np.full(T, float(scale))]))
        cnt = np.diff(vptr)
        for i in range(int(cnt.max()) if len(cnt) else 0):
            s = cnt > i
            u[s] = u[s] + vocc[vnode[vptr[:-1][s] + i]]
        return u[:self.n_var], w

    def data_cross_t(self, x, lam, vx, vl, scale=1.0):
        """Host twin of asm_eval_data_cross_t: out [n_dpar] with out[c] = d/d dpar[c] [D_vx (scale * f - lam' g) + vl' g], `lam` and
        `vl` on the block's rows, `vx` a direction in the variables: dc' out = vx' u + vl' w for (u, w) = data_cross(x, lam, dc).  The
        sweep of data_cross seeded in the variables; every CONST node is an occurrence - (-lam[r]) * adjoint tangent + vl[r] * adjoint
        in a row r, scale * adjoint tangent in a term - and out[c] sums those of dpar[c] from 0.0 in data_gradient's order
        (k_nlp_expr_cross_t, k_nlp_expr_data_gather)."""
        tape = self.tape
        R, T = tape.R, tape.T
        x, lam, vx, vl = (np.asarray(v, float) for v in (x, lam, vx, vl))
        cnt = np.diff(self.c_ptr)
        out = np.zeros(len(cnt))
        if not np.any(tape.op == CONST) or R + T == 0:
            return out
        ptr = tape.ptr
        sweep = _HessSweep(ptr[:-1].copy(), np.diff(ptr), tape.op, tape.a, tape.b, np.full(R + T, -1, np.int64), np.zeros(0, np.int64),
                           max(self.n_var, 1))
        V, D = sweep.forward2(x, self._consts, vx=vx)
        cocc = np.zeros(int(self.c_ptr[-1]))
        sweep.reverse2(V, D, cocc, weight=np.concatenate([-lam[:R], np.full(T, float(scale))]), cslot=self._slot,
                       wadj=np.concatenate([vl[:R], np.zeros(T)]), both=np.arange(R + T) < R)
        for i in range(int(cnt.max()) if len(cnt) else 0):
            s = cnt > i
            out[s] = out[s] + cocc[self.c_ptr[:-1][s] + i]
        return out

    # ---- host callbacks (the twins of k_nlp_expr_rows / _terms / _objective / _gradient)
    def _eval_g(self, x, out):
        out[:] = self._rows.forward(np.asarray(x, float), self._consts)[1]
        return out

    def _eval_jac_g(self, x, out):
        V, _ = self._rows.forward(np.asarray(x, float), self._consts)
        vals = np.zeros(len(self.rows))
        self._rows.reverse(V, vals, True)
        out[:] = vals
        return out

    def _eval_f(self, x):
        """The sum of the terms in term order from 0.0 (unscaled: FunctionModel applies the sense)."""
        tv = self._terms.forward(np.asarray(x, float), self._consts)[1]
        v = 0.0
        for t in tv:
            v = v + float(t)
        return v

    def _eval_grad_f(self, x, grad):
        """Per variable, the adjoints of its VAR nodes in (term, node) order from 0.0 (unscaled)."""
        V, _ = self._terms.forward(np.asarray(x, float), self._consts)
        occ = np.zeros(self._n_occ)
        self._terms.reverse(V, occ, False)
        n = len(grad)
        gp = np.zeros(n + 1, np.int64)
        gp[:len(self.g_ptr)] = self.g_ptr
        gp[len(self.g_ptr):] = self.g_ptr[-1]
        cnt = np.diff(gp)
        g = np.zeros(n)
        for i in range(int(cnt.max()) if n else 0):
            s = cnt > i
            g[s] = g[s] + occ[gp[:-1][s] + i]
        grad[:] = g
        return grad
