"""The expression tape's derivatives against exact math (tests/expr_exact.py: mpmath, mp.diff), op by op at the edges, on the host twin.

One block holds every (op, point) of TABLE as a row of its own over its own two variables, row r = op(x[2r], x[2r+1]), then the same
table once more with every operand split between a variable and a parameter, row = op(x + p, x' + p') with x = p = point / 2 (the sum is
exact, so the operand is the point and every data derivative has a value to be checked against); a CONST exponent is a parameter of its own
row.  The same rows are repeated as objective terms over variables and parameters of their own.  R and T are above 256: the second
workgroup and the >= R / >= T / >= S guards of the device kernels run in the same launches (tests/test_expr_exact_gpu.py runs this file's
checks through the handle API).

The bar, per entry:  |got - E| <= K eps (|E| + C + F),  eps = 2^-52, E and C from the reference (C = sum |in_i| |dE / d in_i|: what one
rounding of the inputs moves), an entry with E = C = F = 0 exactly 0.
  K  is counted from the statements of include/asm_hip.h for the op and the sweep - one per arithmetic operation, L_f per use of a value of
     library function f, plus one (_k below) - and is not fitted to what the sweeps return.
  L_f is the library's own error: the value rows measure it (a value is one call and nothing else) over the table, which holds the
     arguments of the derivative statements as well (pow(u, y - 1), pow(u, y - 2), cosh at sinh's points, ...); the largest error in
     units of eps |exact|, doubled, rounded up, at least 1.  NUMPY_L: NumPy's figures on the host (test_library_errors_are_as_recorded
     measures them again); the device's are in tests/test_expr_exact_gpu.py and DESIGN.md.
  F  is 0 except for the ops of F_TERMS: the terms of a statement that cancels, in absolute value (the magnitude convention of
     tests/util.py::bound_ratio).

ABS, MIN and MAX at their kinks (+-0.0, ties, a NaN operand) are checked against the header's convention in closed form.  An entry whose
exact value is not real (d/dq of pow(u, q) at u < 0) or is beyond the double range must come back as NaN or inf; an entry whose bar is
itself beyond the double range (C of the mixed second derivative of atan2 at (1e-200, 1e-200) is 1e400) asserts nothing.
"""
import numpy as np
import pytest
from mpmath import mp, mpf

from activesetmethods_amd import nlexpr as nx
from activesetmethods_amd.moi_evaluator import FunctionModel
from activesetmethods_amd.nlexpr import Expr, ExprBlock, parameters, variables
from tests.expr_exact import ExactRow, ratio

EPS = float(np.finfo(float).eps)
NAN = float("nan")
DBL_MAX = mpf(float(np.finfo(float).max))

UNARY = {"sqrt": nx.SQRT, "exp": nx.EXP, "log": nx.LOG, "sin": nx.SIN, "cos": nx.COS, "abs": nx.ABS, "tan": nx.TAN, "asin": nx.ASIN,
         "acos": nx.ACOS, "atan": nx.ATAN, "sinh": nx.SINH, "cosh": nx.COSH, "tanh": nx.TANH, "log10": nx.LOG10, "log2": nx.LOG2,
         "log1p": nx.LOG1P, "expm1": nx.EXPM1, "cbrt": nx.CBRT, "neg": nx.NEG}
BINARY = {"add": nx.ADD, "sub": nx.SUB, "mul": nx.MUL, "div": nx.DIV, "pow": nx.POW, "atan2": nx.ATAN2, "min": nx.MIN, "max": nx.MAX}

# (kind, a, b): unary ops read a; "powi:e" is a ** e; "powc" is pow(a, q) with the CONST exponent q = b; every other kind is op(a, b).
# Magnitudes are chosen so that every derivative up to order 2 is inside the normal double range (log''(1e-150) = -1e300, sqrt''(1e200) =
# -2.5e-301), and for POW so that u^(y - 2) is as well at every point and at the points of AUX: the second-order statement forms it whatever
# the tangents are.
TABLE = [
    ("sqrt", 1e-200, 0), ("sqrt", 1e-8, 0), ("sqrt", 1.0, 0), ("sqrt", 2.0, 0), ("sqrt", 1e200, 0),
    ("exp", 1e-30, 0), ("exp", -1e-9, 0), ("exp", 1.0, 0), ("exp", -700.0, 0), ("exp", 700.0, 0),
    ("log", 1e-150, 0), ("log", 0.999999999, 0), ("log", 1.000000001, 0), ("log", 0.5, 0), ("log", 1e150, 0),
    ("sin", 1e-30, 0), ("sin", 1e-5, 0), ("sin", 1.5707963, 0), ("sin", 3.1415926, 0), ("sin", 1e6, 0), ("sin", -2.0, 0),
    ("cos", 1e-30, 0), ("cos", 1e-5, 0), ("cos", 1.5707963, 0), ("cos", 3.1415926, 0), ("cos", 1e6, 0), ("cos", -2.0, 0),
    ("tan", 1e-30, 0), ("tan", 1e-5, 0), ("tan", 1.5707963, 0), ("tan", 1.5707964, 0), ("tan", -1.5707963, 0), ("tan", 1e6, 0),
    ("asin", 1e-30, 0), ("asin", 1e-5, 0), ("asin", 0.999999, 0), ("asin", -0.9999999, 0), ("asin", 0.5, 0), ("asin", -0.999999, 0),
    ("acos", 1e-30, 0), ("acos", 0.999999, 0), ("acos", -0.9999999, 0), ("acos", 0.5, 0), ("acos", -0.5, 0),
    ("atan", 1e-30, 0), ("atan", 1.0, 0), ("atan", -1e8, 0), ("atan", 1e100, 0),
    ("sinh", 1e-30, 0), ("sinh", 1e-5, 0), ("sinh", 1.0, 0), ("sinh", -20.0, 0), ("sinh", 700.0, 0),
    ("cosh", 1e-30, 0), ("cosh", 1e-5, 0), ("cosh", 1.0, 0), ("cosh", -20.0, 0), ("cosh", 700.0, 0),
    ("tanh", 1e-30, 0), ("tanh", 1e-5, 0), ("tanh", 1.0, 0), ("tanh", 9.0, 0), ("tanh", 18.0, 0), ("tanh", -9.0, 0),
    ("log10", 1e-45, 0), ("log10", 0.999999999, 0), ("log10", 1.000000001, 0), ("log10", 1e45, 0),
    ("log2", 1e-45, 0), ("log2", 0.999999999, 0), ("log2", 1.000000001, 0), ("log2", 1e45, 0),
    ("log1p", 1e-30, 0), ("log1p", -1e-10, 0), ("log1p", -0.9999999, 0), ("log1p", -0.5, 0), ("log1p", 1e45, 0),
    ("expm1", 1e-30, 0), ("expm1", 1e-10, 0), ("expm1", -1e-10, 0), ("expm1", -20.0, 0), ("expm1", 1.0, 0), ("expm1", 700.0, 0),
    ("cbrt", 1e-45, 0), ("cbrt", -1e-45, 0), ("cbrt", 1.0, 0), ("cbrt", -8.0, 0), ("cbrt", 1e45, 0),
    # POWI: e in {1, 2, 3, -1, -3, 64, -64}, u negative, tiny and near 1
    ("powi:1", -1.5, 0), ("powi:1", 1e-50, 0), ("powi:1", 0.9999999, 0),
    ("powi:2", -1.5, 0), ("powi:2", 1e-50, 0), ("powi:2", 0.9999999, 0),
    ("powi:3", -1.5, 0), ("powi:3", 1e-50, 0), ("powi:3", 0.9999999, 0),
    ("powi:-1", -1.5, 0), ("powi:-1", 1e-50, 0), ("powi:-1", 0.9999999, 0),
    ("powi:-3", -1.5, 0), ("powi:-3", 1e-50, 0), ("powi:-3", 0.9999999, 0),
    ("powi:64", -1.5, 0), ("powi:64", 1e-4, 0), ("powi:64", 0.9999999, 0),
    ("powi:-64", -1.5, 0), ("powi:-64", 1e-4, 0), ("powi:-64", 0.9999999, 0),
    # POW with a VAR exponent: y = 1, y = 2, u near 1 with a large y, the mixed entry that cancels (1 + y log u near 0 at (0.5, 1.5))
    ("pow", 0.5, 1.5), ("pow", 1.3, 2.5), ("pow", 2.0, 1.0), ("pow", 3.0, 2.0), ("pow", 0.9999999, 1e6), ("pow", 1.0000001, -1e6),
    ("pow", 1e-60, 1.5), ("pow", 10.0, -3.5),
    # POW with a CONST exponent: 2.0, 3.0, 1.0 and 0.5, u < 0 where it is defined, tiny u
    ("powc", 1.7, 2.0), ("powc", -1.3, 2.0), ("powc", 1e-60, 2.0), ("powc", 1.7, 3.0), ("powc", -1.3, 3.0), ("powc", 1e-60, 3.0),
    ("powc", 1.7, 1.0), ("powc", -1.3, 1.0), ("powc", 1e-60, 1.0), ("powc", 1.7, 0.5), ("powc", 1e-60, 0.5), ("powc", 1.3, 2.5),
    # ATAN2(a, b) = the angle of (b, a): four quadrants, both axes, and where a * a underflows
    ("atan2", 0.7, 1.3), ("atan2", 0.7, -1.3), ("atan2", -0.7, -1.3), ("atan2", -0.7, 1.3),
    ("atan2", 1.0, 0.0), ("atan2", -1.0, 0.0), ("atan2", 0.0, 1.0), ("atan2", 0.0, -1.0), ("atan2", 1e-200, 1e-200),
    ("div", 0.5, 1e-100), ("div", 1.0, 3.0), ("div", -7.0, 1e100), ("div", 1e-30, 3.0),
    ("add", 0.1, 0.2), ("add", 1e16, 1.0), ("sub", 1.0000001, 1.0), ("sub", 0.1, -0.2), ("mul", 3.0, -7.0), ("mul", 1e150, 1e-150),
    ("neg", 1.5, 0), ("neg", 1e-30, 0),
    # ABS, MIN, MAX away from their kinks ...
    ("abs", 1.5, 0), ("abs", -2.5, 0), ("abs", 1e-30, 0), ("abs", -1e-30, 0),
    ("min", 1.0, 2.0), ("min", 2.0, 1.0), ("min", -1e-30, 1e-30), ("max", 1.0, 2.0), ("max", 2.0, 1.0), ("max", -1e-30, 1e-30),
    # ... and at them: the header's convention (KINKS)
    ("abs", 0.0, 0), ("abs", -0.0, 0),
    ("min", 1.5, 1.5), ("min", 0.0, -0.0), ("min", -0.0, 0.0), ("min", NAN, 1.0), ("min", 1.0, NAN),
    ("max", 1.5, 1.5), ("max", 0.0, -0.0), ("max", -0.0, 0.0), ("max", NAN, 1.0), ("max", 1.0, NAN),
]
# the arguments the derivative statements hand to the library: pow(u, y - 1), pow(u, y - 2) and log(u) at every POW point with u > 0
# (sin / cos and sinh / cosh share their points above)
AUX = ([("pow", a, b - k) for kind, a, b in TABLE if kind in ("pow", "powc") and a > 0 for k in (1.0, 2.0)]
       + [("log", a, 0) for kind, a, b in TABLE if kind in ("pow", "powc") and a > 0])
ALL_POINTS = TABLE + AUX


def kink(kind, a, b):
    """(value, d/da, d/db) by the header's convention where the op is not differentiable, else None: ABS d = copysign(1, u); MIN / MAX
    take b only where b < a (b > a) holds - a tie or a NaN operand takes a, with a's value and all of the adjoint."""
    if kind == "abs" and a == 0.0:
        return (0.0, float(np.copysign(1.0, a)), 0.0)
    if kind in ("min", "max") and (a == b or a != a or b != b):
        return (a, 1.0, 0.0)
    return None


# ---- K: (arithmetic operations, {library function: uses of its value}) for the value, a first-order statement (adjoint or tangent)
# and a second-order statement (adjoint tangent, with the tangents it reads), counted from include/asm_hip.h, "Expression block" and
# "Hessian of the Lagrangian", 2.; a value the statement uses k times counts k times
def _k(kind):
    if kind.startswith("powi:"):
        e = abs(int(kind[5:]))
        return (e + 1, {}), (e + 4, {}), (2 * e + 10, {})
    return {
        "add": ((1, {}), (1, {}), (1, {})), "sub": ((1, {}), (1, {}), (1, {})), "neg": ((1, {}), (1, {}), (1, {})),
        "min": ((1, {}), (1, {}), (1, {})), "max": ((1, {}), (1, {}), (1, {})), "abs": ((1, {}), (2, {}), (3, {})),
        "mul": ((1, {}), (2, {}), (4, {})), "div": ((1, {}), (4, {}), (12, {})),
        "sqrt": ((0, {"sqrt": 1}), (3, {"sqrt": 1}), (9, {"sqrt": 3})),
        "exp": ((0, {"exp": 1}), (2, {"exp": 1}), (5, {"exp": 2})),
        "log": ((0, {"log": 1}), (2, {}), (5, {})),
        "sin": ((0, {"sin": 1}), (2, {"cos": 1}), (5, {"sin": 1, "cos": 1})),
        "cos": ((0, {"cos": 1}), (2, {"sin": 1}), (5, {"sin": 1, "cos": 1})),
        "tan": ((0, {"tan": 1}), (4, {"tan": 2}), (11, {"tan": 5})),
        "asin": ((0, {"asin": 1}), (5, {"sqrt": 1}), (16, {"sqrt": 3})),
        "acos": ((0, {"acos": 1}), (5, {"sqrt": 1}), (16, {"sqrt": 3})),
        "atan": ((0, {"atan": 1}), (4, {}), (11, {})),
        "sinh": ((0, {"sinh": 1}), (2, {"cosh": 1}), (5, {"sinh": 1, "cosh": 1})),
        "cosh": ((0, {"cosh": 1}), (2, {"sinh": 1}), (5, {"sinh": 1, "cosh": 1})),
        "tanh": ((0, {"tanh": 1}), (4, {"tanh": 2}), (11, {"tanh": 5})),
        "log10": ((0, {"log10": 1}), (4, {}), (11, {})), "log2": ((0, {"log2": 1}), (4, {}), (11, {})),
        "log1p": ((0, {"log1p": 1}), (3, {}), (7, {})),
        "expm1": ((0, {"expm1": 1}), (3, {"expm1": 1}), (7, {"expm1": 2})),
        "cbrt": ((0, {"cbrt": 1}), (4, {"cbrt": 2}), (13, {"cbrt": 7})),
        "pow": ((0, {"pow": 1}), (4, {"pow": 1, "log": 1}), (17, {"pow": 4, "log": 3})),
        "powc": ((0, {"pow": 1}), (4, {"pow": 1, "log": 1}), (17, {"pow": 4, "log": 3})),
        "atan2": ((0, {"atan2": 1}), (6, {}), (22, {})),
    }[kind]


def K(kind, order, L, extra=0):
    arith, uses = _k(kind)[order]
    return arith + sum(n * L[f] for f, n in uses.items()) + 1 + extra


# ---- L_f of NumPy on the host, measured by test_library_errors_are_as_recorded over ALL_POINTS (largest error in eps |exact|, doubled,
# rounded up, at least 1); the largest errors themselves are in DESIGN.md, "Expression derivatives against exact math"
NUMPY_L = {"sqrt": 1, "exp": 1, "log": 1, "sin": 1, "cos": 1, "tan": 1, "asin": 1, "acos": 1, "atan": 1, "sinh": 1, "cosh": 1, "tanh": 1,
           "log10": 1, "log2": 1, "log1p": 1, "expm1": 1, "cbrt": 1, "pow": 1, "atan2": 1}
LIB_OF = {k: k for k in NUMPY_L}
LIB_OF["powc"] = "pow"

# ---- F: the terms of the statement that cancels, in absolute value, as functions of the op's exact value v: (first order, second order).
# TANH forms 1 - v * v (terms 1 and v^2) - the second-order statement multiplies it by 2 v; EXPM1 forms v + 1 (terms |v| and 1).
# Both read the library's v, whose rounding is eps |v| ~ eps while the difference is far smaller: no statement with the same calls removes
# that (DESIGN.md has the measured losses).
F_TERMS = {"tanh": (lambda v: 1.0 + v * v, lambda v: 2.0 * abs(v) * (1.0 + v * v)),
           "expm1": (lambda v: abs(v) + 1.0, lambda v: abs(v) + 1.0)}


def op_expr(kind, A, B):
    if kind.startswith("powi:"):
        return Expr(nx.POWI, (A,), int(kind[5:]))
    if kind in UNARY:
        return Expr(UNARY[kind], (A,))
    return Expr(BINARY["pow" if kind == "powc" else kind], (A, B))


def op_code(kind):
    return nx.POWI if kind.startswith("powi:") else UNARY[kind] if kind in UNARY else BINARY["pow" if kind == "powc" else kind]


def is_binary(kind):
    return kind in BINARY or kind == "powc"


class Rec:
    """One row or term: its table entry, its variables xa, xb, its parameters pa, pb (dpar slots; None: none), its graph."""
    __slots__ = ("kind", "a", "b", "data", "xa", "xb", "pa", "pb", "expr", "index", "is_row", "canon")


def table_model(sense="MIN_SENSE"):
    """(fm, recs, x): the block of the module docstring as a FunctionModel with nothing else in it, and the point."""
    N = len(ALL_POINTS)
    xs = variables(8 * N)
    xv, pv, recs = np.zeros(8 * N), [], []
    plist = []

    def param(v):
        p = parameters([v])[0]
        plist.append(p)
        pv.append(v)
        return p, len(plist) - 1

    for is_row in (True, False):
        for data in (False, True):
            for i, (kind, a, b) in enumerate(ALL_POINTS):
                r = Rec()
                r.kind, r.a, r.b, r.data, r.is_row = kind, float(a), float(b), data, is_row
                r.index = len([q for q in recs if q.is_row == is_row])
                base = 2 * r.index + (0 if is_row else 4 * N)
                r.xa, r.xb, r.pa, r.pb = base, base + 1, None, None
                A, B = xs[r.xa], xs[r.xb] if is_binary(kind) and kind != "powc" else None
                sa, sb = (0.5, 0.5) if data else (1.0, 1.0)
                xv[r.xa], xv[r.xb] = sa * r.a, (sb * r.b if B is not None else 0.0)
                if data:
                    p, r.pa = param(0.5 * r.a)
                    A = A + p
                    if B is not None:
                        p, r.pb = param(0.5 * r.b)
                        B = B + p
                if kind == "powc":
                    B, r.pb = param(r.b)
                r.expr = op_expr(kind, A, B)
                recs.append(r)
    rows = [r for r in recs if r.is_row]
    terms = [r for r in recs if not r.is_row]
    obj = terms[0].expr
    for t in terms[1:]:
        obj = obj + t.expr
    blk = ExprBlock([(r.expr, 0.0, np.inf) for r in rows], objective=obj, n=8 * N, parameters=plist)
    fm = FunctionModel(8 * N, -1e6 * np.ones(8 * N), 1e6 * np.ones(8 * N))          # (bounds play no part in an evaluation)
    fm.sense = sense
    fm.nlp = blk
    assert np.array_equal(blk.device[2], np.asarray(pv), equal_nan=True) and blk.tape.R == len(rows) and blk.tape.T == len(terms)
    return fm, recs, xv


class Reference:
    """The exact numbers of every (table entry, variant), computed once on a canonical copy of the row: variables 0, 1, parameters 0, 1."""

    def __init__(self):
        self.rows = {}

    def of(self, rec):
        key = (rec.kind, repr(rec.a), repr(rec.b), rec.data)
        if key not in self.rows:
            x = variables(2)
            vals, ps = [], []
            sa = 0.5 if rec.data else 1.0
            A, B = x[0], x[1] if rec.xb is not None and is_binary(rec.kind) and rec.kind != "powc" else None
            pa = pb = None
            if rec.data:
                pa = parameters([sa * rec.a])[0]
                ps.append(pa); vals.append(sa * rec.a)
                A = A + pa
                if B is not None:
                    pb = parameters([sa * rec.b])[0]
                    ps.append(pb); vals.append(sa * rec.b)
                    B = B + pb
            if rec.kind == "powc":
                pb = parameters([rec.b])[0]
                ps.append(pb); vals.append(rec.b)
                B = pb
            ids = {id(p): k for k, p in enumerate(ps)}
            row = ExactRow(op_expr(rec.kind, A, B), lambda e: ids[id(e)], [sa * rec.a, sa * rec.b], vals)
            role = {"xa": ("x", 0), "xb": ("x", 1), "pa": ("c", ids[id(pa)]) if pa is not None else None,
                    "pb": ("c", ids[id(pb)]) if pb is not None else None}
            self.rows[key] = (row, role, {})
        return self.rows[key]

    def entry(self, rec, *roles):
        """(E, C) of d row / d roles (e.g. "xa", "pb"); a role the row does not have: (0, 0).  A kink: the closed form, C = 0."""
        row, role, memo = self.of(rec)
        roles = tuple(sorted(roles))
        if roles not in memo:
            kk = kink(rec.kind, rec.a, rec.b)
            if any(role[r] is None for r in roles):
                memo[roles] = (mpf(0), mpf(0))
            elif kk is not None:
                side = {"xa": 1, "pa": 1, "xb": 2, "pb": 2}
                v = kk[0] if not roles else kk[side[roles[0]]] if len(roles) == 1 else 0.0
                memo[roles] = (mpf(v) if v == v else mp.nan, mpf(0))
            else:
                orders = {}
                for r in roles:
                    orders[role[r]] = orders.get(role[r], 0) + 1
                memo[roles] = row.entry(orders)
        return memo[roles]


REF = Reference()


class Sweep:
    """Collects |got - wgt E| / (K eps |wgt| (|E| + C + F)) of one sweep, and what missed."""

    def __init__(self, name):
        self.name, self.worst, self.where, self.bad, self.count = name, 0.0, None, [], 0

    def add(self, rec, roles, got, wgt, k, F=0.0):
        E, C = REF.entry(rec, *roles)
        self.count += 1
        tag = "%s(%r, %r)%s %s d%s" % (rec.kind, rec.a, rec.b, " data" if rec.data else "", "row" if rec.is_row else "term", "/".join(roles))
        got = float(got)
        if mp.isnan(E) or abs(E) * abs(wgt) > DBL_MAX:               # not real, or beyond the double range: NaN or inf
            if np.isfinite(got):
                self.bad.append((tag, got, "NaN or inf"))
            return
        bar = k * EPS * abs(mpf(wgt)) * (abs(E) + C + mpf(F))
        if bar > DBL_MAX:                                             # one rounding of the inputs moves the entry across the whole range
            return
        q = ratio(got, mpf(wgt) * E, bar)
        if q > self.worst:
            self.worst, self.where = q, tag
        if q > 1.0:
            self.bad.append((tag, got, "%s, ratio %.3g (K %d)" % (mp.nstr(mpf(wgt) * E, 17), q, k)))

    def report(self):
        print("%-28s %5d entries, worst error / bar %.3f at %s" % (self.name, self.count, self.worst, self.where))
        return self


def F_of(rec, order):
    if rec.kind not in F_TERMS:
        return 0.0
    v = float(REF.entry(rec)[0])
    return F_TERMS[rec.kind][order - 1](v)


class Twin:
    """The host twin behind the calls the checks make; tests/test_expr_exact_gpu.py has the handle's."""

    def __init__(self, fm):
        self.fm, self.blk, self.scale = fm, fm.nlp, fm.objective_scale

    def row_values(self, x):
        return self.blk._eval_g(x, np.zeros(self.blk.m))

    def term_values(self, x):
        return self.blk._terms.forward(np.asarray(x, float), self.blk._consts)[1]

    def jacobian(self, x):
        return self.blk.rows - 1, self.blk.cols - 1, self.blk._eval_jac_g(x, np.zeros(len(self.blk.rows)))

    def gradient(self, x):
        return self.scale * self.blk._eval_grad_f(x, np.zeros(self.fm.n))

    def hessian(self, x, obj_factor, lam):
        r, c = self.blk.hessian_structure()
        return r - 1, c - 1, self.blk.hessian_values(x, obj_factor * self.scale, lam)

    def hessian_product(self, x, obj_factor, lam, v):
        r, c, h = self.hessian(x, obj_factor, lam)
        out = np.zeros(self.fm.n)
        with np.errstate(all="ignore"):
            np.add.at(out, r, h * v[c])
            off = r != c
            np.add.at(out, c[off], h[off] * v[r[off]])
        return out

    def data_gradient(self, x, lam):
        return self.blk.data_gradient(x, lam, self.scale)

    def data_cross(self, x, lam, dc):
        return self.blk.data_cross(x, lam, dc, self.scale)

    def data_cross_t(self, x, lam, vx, vl):
        return self.blk.data_cross_t(x, lam, vx, vl, self.scale)


def measure_library(values_of_rows):
    """f -> the largest |value - exact| / (eps |exact|) over the plain rows whose op is one call of f."""
    fm, recs, xv = table_model()
    got = values_of_rows(fm, xv)
    worst = {}
    for r in recs:
        if r.is_row and not r.data and r.kind in LIB_OF:
            E, _ = REF.entry(r)
            q = ratio(got[r.index], E, EPS * abs(E))
            worst[LIB_OF[r.kind]] = max(worst.get(LIB_OF[r.kind], 0.0), q)
    return worst


def check_table(api, fm, recs, xv, L, seed):
    """Every sweep of `api` over the whole table; returns the Sweep records (the caller asserts and prints)."""
    rng = np.random.default_rng(seed)
    rows = [r for r in recs if r.is_row]
    terms = [r for r in recs if not r.is_row]
    R, n, scale = len(rows), fm.n, fm.objective_scale
    lam = rng.uniform(0.5, 2.0, R) * rng.choice([-1.0, 1.0], R)
    obj_factor = 1.75
    nd = len(fm.nlp.device[2])
    out = []

    def sweep(name):
        out.append(Sweep(name))
        return out[-1]

    # values
    s = sweep("value (rows)")
    ev = api.row_values(xv)
    for r in rows:
        s.add(r, (), ev[r.index], 1.0, K(r.kind, 0, L))
    if hasattr(api, "term_values"):
        s = sweep("value (terms)")
        tv = api.term_values(xv)
        for t in terms:
            s.add(t, (), tv[t.index], 1.0, K(t.kind, 0, L))
    # Jacobian: every row has the entries of its own variables and no other
    s = sweep("Jacobian")
    jr, jc, jv = api.jacobian(xv)
    J = {(int(i), int(j)): v for i, j, v in zip(jr, jc, jv)}
    assert len(J) == len(jv) == sum(2 if is_binary(r.kind) and r.kind != "powc" else 1 for r in rows)
    for r in rows:
        for role, j in (("xa", r.xa), ("xb", r.xb)):
            if role == "xb" and (r.kind == "powc" or not is_binary(r.kind)):
                assert (r.index, j) not in J
                continue
            s.add(r, (role,), J[(r.index, j)], 1.0, K(r.kind, 1, L), F_of(r, 1))
    # gradient
    s = sweep("gradient")
    g = api.gradient(xv)
    for t in terms:
        s.add(t, ("xa",), g[t.xa], scale, K(t.kind, 1, L), F_of(t, 1))
        s.add(t, ("xb",), g[t.xb], scale, K(t.kind, 1, L), F_of(t, 1))
    assert not g[:4 * len(ALL_POINTS)].any()
    # Hessian of the Lagrangian and its product with the unit vectors of the first and of the second variable of every row
    s = sweep("Hessian of the Lagrangian")
    hr, hc, hv = api.hessian(xv, obj_factor, lam)
    H = {(int(i), int(j)): v for i, j, v in zip(hr, hc, hv)}
    assert len(H) == len(hv)
    for r in recs:
        w = lam[r.index] if r.is_row else obj_factor * scale
        for roles, key in ((("xa", "xa"), (r.xa, r.xa)), (("xa", "xb"), (r.xb, r.xa)), (("xb", "xb"), (r.xb, r.xb))):
            s.add(r, roles, H.pop(key, 0.0), w, K(r.kind, 2, L, 1), F_of(r, 2))
    assert not H, "Hessian entries outside the rows' own variables"
    s = sweep("Hessian product")
    ea, eb = np.zeros(n), np.zeros(n)
    ea[0::2], eb[1::2] = 1.0, 1.0
    ha, hb = api.hessian_product(xv, obj_factor, lam, ea), api.hessian_product(xv, obj_factor, lam, eb)
    for r in recs:
        w = lam[r.index] if r.is_row else obj_factor * scale
        for roles, got in ((("xa", "xa"), ha[r.xa]), (("xa", "xb"), ha[r.xb]), (("xa", "xb"), hb[r.xa]), (("xb", "xb"), hb[r.xb])):
            s.add(r, roles, got, w, K(r.kind, 2, L, 2), F_of(r, 2))
    # data gradient
    s = sweep("data gradient")
    dg = api.data_gradient(xv, lam)
    assert dg.shape == (nd,)
    for r in recs:
        w = -lam[r.index] if r.is_row else scale
        for role, c in (("pa", r.pa), ("pb", r.pb)):
            if c is not None:
                s.add(r, (role,), dg[c], w, K(r.kind, 1, L, 1), F_of(r, 1))
    # data cross derivatives: the unit direction of the first parameter of every row at once, then of the second
    s = sweep("data cross")
    for role, pick in (("pa", lambda r: r.pa), ("pb", lambda r: r.pb)):
        dc = np.zeros(nd)
        dc[[pick(r) for r in recs if pick(r) is not None]] = 1.0
        u, w = api.data_cross(xv, lam, dc)
        for r in recs:
            if pick(r) is None:
                continue
            wt = -lam[r.index] if r.is_row else scale
            s.add(r, ("xa", role), u[r.xa], wt, K(r.kind, 2, L, 1), F_of(r, 2))
            s.add(r, ("xb", role), u[r.xb], wt, K(r.kind, 2, L, 1), F_of(r, 2))
            if r.is_row:
                s.add(r, (role,), w[r.index], 1.0, K(r.kind, 1, L, 2), F_of(r, 1))
    # transposed: vx the unit vectors of the first variables, of the second, then vl = 1
    s = sweep("data cross, transposed")
    for role, vx, vl in (("xa", ea, np.zeros(R)), ("xb", eb, np.zeros(R)), (None, np.zeros(n), np.ones(R))):
        o = api.data_cross_t(xv, lam, vx, vl)
        assert o.shape == (nd,)
        for r in recs:
            for prole, c in (("pa", r.pa), ("pb", r.pb)):
                if c is None:
                    continue
                if role is None:
                    if r.is_row:
                        s.add(r, (prole,), o[c], 1.0, K(r.kind, 1, L, 2), F_of(r, 1))
                    elif not (o[c] == 0.0 or mp.isnan(REF.entry(r, prole)[0]) and not np.isfinite(o[c])):
                        s.bad.append(("%s(%r, %r) term d%s, weight vl" % (r.kind, r.a, r.b, prole), float(o[c]), "0: vl has no part in a term"))
                elif mp.isnan(REF.entry(r, prole)[0]):               # the exponent's own entry at u < 0: NaN or inf whatever the weights
                    if np.isfinite(o[c]):
                        s.bad.append(("%s(%r, %r) d%s" % (r.kind, r.a, r.b, prole), float(o[c]), "NaN or inf"))
                else:
                    s.add(r, (role, prole), o[c], -lam[r.index] if r.is_row else scale, K(r.kind, 2, L, 2), F_of(r, 2))
    return out


def assert_sweeps(sweeps):
    bad = []
    for s in sweeps:
        s.report()
        bad += ["%s: %s: got %r, want %s" % (s.name, t, g, w) for t, g, w in s.bad]
    assert not bad, "%d entries miss their bar:\n%s" % (len(bad), "\n".join(bad[:60]))


# ------------------------------------------------------------------------------------------------ the tests
def test_the_table_covers_every_op_and_fills_two_workgroups():
    assert len(TABLE) == 172 and len(ALL_POINTS) == len(TABLE) + len(AUX)
    assert {op_code(k) for k, _, _ in TABLE} == set(range(nx.ADD, nx.MAX + 1))
    fm, recs, xv = table_model()
    assert fm.nlp.tape.R == fm.nlp.tape.T == 2 * len(ALL_POINTS) > 256
    assert set(fm.nlp.tape.op.tolist()) == set(range(nx.CONST, nx.MAX + 1))
    for e in (1, 2, 3, -1, -3, 64, -64):
        assert sum(1 for k, _, _ in TABLE if k == "powi:%d" % e) == 3
    assert sum(1 for k, a, b in TABLE if kink(k, a, b) is not None) == 12


def test_library_errors_are_as_recorded():
    """NumPy's error per function over the table against NUMPY_L: L_f = the largest error, doubled, rounded up, at least 1."""
    worst = measure_library(lambda fm, xv: Twin(fm).row_values(xv))
    for f in sorted(worst):
        print("%-6s largest error %.3f eps |exact|   L = %d" % (f, worst[f], NUMPY_L[f]))
    assert set(worst) == set(NUMPY_L)
    assert {f: max(1, int(np.ceil(2.0 * q))) for f, q in worst.items()} == NUMPY_L


@pytest.mark.parametrize("sense", ["MIN_SENSE", "MAX_SENSE"])
def test_every_sweep_of_the_twin_against_exact_math(sense):
    fm, recs, xv = table_model(sense)
    assert_sweeps(check_table(Twin(fm), fm, recs, xv, NUMPY_L, seed=len(sense)))


# ------------------------------------------------------------------------------------------------ C. data derivatives in every position
# Small composite rows and terms over four variables and three declared parameters: every op takes a parameter as its operand a and, the
# binary ones, as b - the POW exponent, the POW base and both, either argument of ATAN2, the selected and the unselected operand of MIN and
# MAX, under every unary op - and a literal constant is an exponent too.  data_gradient, data_cross for each unit dc and data_cross_t
# against the reference, normwise at LIBM_BAR (library values carried through a few operations of size O(1), tests/test_sensitivity_gpu.py).
from tests.test_block_data_cpu import LIBM_BAR                      # noqa: E402
from tests.test_nlhess_cpu import PARITY                            # noqa: E402
from tests.test_sensitivity_cpu import KKT_BAR, _dpar_index         # noqa: E402

POSITION_X = np.array([0.9, 0.6, 0.8, 1.2])
POSITION_P = [0.7, 1.9, 0.35]


def position_model(sense="MIN_SENSE"):
    x = variables(4)
    p = parameters(POSITION_P)
    un = [nx.sqrt, nx.exp, nx.log, nx.sin, nx.cos, abs, nx.tan, nx.asin, nx.acos, nx.atan, nx.sinh, nx.cosh, nx.tanh, nx.log10, nx.log2,
          nx.log1p, nx.expm1, nx.cbrt, lambda u: -u]
    row0 = None
    for k, f in enumerate(un):                                       # under every unary op (asin and acos: the parameters below 1)
        t = x[k % 4] * f(p[0] if f is nx.asin else p[2] if f is nx.acos else p[k % 3])
        row0 = t if row0 is None else row0 + t
    row1 = ((p[0] + x[0]) * (p[1] - x[1]) + p[2] * x[2] + p[0] / x[3] + nx.pow(p[1], x[0]) + nx.atan(p[0], x[1])
            + nx.minimum(p[0], x[2]) + nx.maximum(p[1], x[3]) + nx.minimum(p[1], x[0]) + p[1] ** 3 * x[0])          # operand a
    row2 = ((x[0] + p[0]) * (x[1] - p[1]) + x[2] * p[2] + x[3] / p[1] + nx.pow(x[0], p[1]) + nx.atan(x[1], p[2])
            + nx.minimum(x[2], p[0]) + nx.maximum(x[3], p[1]) + nx.maximum(x[1], p[2]) + nx.pow(p[0], p[1]) * x[2]
            + nx.pow(x[1], 2.5))                                                                                    # operand b, both, a literal
    row3 = nx.minimum(p[0] * x[0], x[1]) * x[2] + nx.maximum(x[3], p[1] * x[2]) * x[1]
    obj = nx.pow(x[0] * p[0], p[1]) + nx.atan(p[2], x[1] * p[0]) + nx.tanh(p[0] * x[2]) * x[3] + nx.expm1(x[1] - p[2])
    blk = ExprBlock([(r, 0.0, np.inf) for r in (row0, row1, row2, row3)], objective=obj, n=4, parameters=p)
    fm = FunctionModel(4, np.full(4, 0.1), np.full(4, 10.0))
    fm.sense = sense
    fm.nlp = blk
    return fm


def position_reference(fm, xv):
    """(G [nd], U [nd x n], W [nd x R]) per unit of weight: G_e[c] = d expr_e / dc, ... as lists per row / term, in mpmath."""
    blk = fm.nlp
    slot = _dpar_index(blk)
    consts = np.asarray(blk.device[2], float)
    nd, n = len(consts), fm.n
    refs = [ExactRow(e, slot, xv, consts) for e in blk.exprs]
    D1 = [[r.number({("c", c): 1}) for c in range(nd)] for r in refs]
    D2 = [[[r.number({("x", j): 1, ("c", c): 1}) for j in range(n)] for c in range(nd)] for r in refs]
    return D1, D2


def check_positions(api, fm, xv, D1, D2, seed):
    """data_gradient, data_cross for each unit dc and data_cross_t of `api` against the reference, and the identity between the two."""
    blk, scale = fm.nlp, fm.objective_scale
    R, n, nd = blk.tape.R, fm.n, len(blk.device[2])
    rng = np.random.default_rng(seed)
    lam, vx, vl = rng.standard_normal(R), rng.standard_normal(n), rng.standard_normal(R)
    wt = [mpf(-v) for v in lam] + [mpf(scale)] * blk.tape.T

    def rel(got, want):
        want = np.array([float(v) for v in want])
        return float(np.abs(np.asarray(got) - want).max() / max(1.0, np.abs(want).max()))

    g = api.data_gradient(xv, lam)
    eg = rel(g, [sum(w * d[c] for w, d in zip(wt, D1)) for c in range(nd)])
    out_t = api.data_cross_t(xv, lam, vx, vl)
    worst_u = worst_w = 0.0
    want_t = []
    for c in range(nd):
        dc = np.zeros(nd)
        dc[c] = 1.0
        u, w = api.data_cross(xv, lam, dc)
        wu = [sum(q * d[c][j] for q, d in zip(wt, D2)) for j in range(n)]
        ww = [D1[r][c] for r in range(R)]
        assert any(v != 0 for v in wu) or any(v != 0 for v in ww), c
        worst_u, worst_w = max(worst_u, rel(u, wu)), max(worst_w, rel(w, ww))
        want_t.append(sum(mpf(a) * b for a, b in zip(vx, wu)) + sum(mpf(a) * b for a, b in zip(vl, ww)))
        lhs, rhs = float(out_t[c]), float(vx @ u + vl @ w)                                 # dc' out = vx' u + vl' w for dc = e_c
        size = abs(out_t[c]) + float(np.abs(vx * u).sum() + np.abs(vl * w).sum())
        assert abs(lhs - rhs) <= LIBM_BAR * size, (c, lhs, rhs)
    et = rel(out_t, want_t)
    print("%s: rel error against exact math: data_gradient %.3e, data_cross u %.3e w %.3e, data_cross_t %.3e (bar %.1e)"
          % (fm.sense, eg, worst_u, worst_w, et, LIBM_BAR))
    assert max(eg, worst_u, worst_w, et) <= LIBM_BAR
    return eg, worst_u, worst_w, et


@pytest.fixture(scope="module")
def position_exact():
    return position_reference(position_model(), POSITION_X)


def test_the_position_model_has_a_parameter_in_every_position():
    blk = position_model().nlp
    op, a, b, ptr = blk.tape.op, blk.tape.a, blk.tape.b, blk.tape.ptr
    row = np.searchsorted(ptr, np.arange(len(op)), side="right") - 1
    ca = {int(op[k]) for k in range(len(op)) if op[k] >= nx.ADD and op[k] != nx.POWI and op[ptr[row[k]] + a[k]] == nx.CONST}
    ca |= {nx.POWI for k in range(len(op)) if op[k] == nx.POWI and op[ptr[row[k]] + a[k]] == nx.CONST}
    cb = {int(op[k]) for k in range(len(op)) if op[k] in nx._BINARY and op[ptr[row[k]] + b[k]] == nx.CONST}
    assert ca == set(range(nx.ADD, nx.MAX + 1)) and cb == set(nx._BINARY)
    assert blk.n_params == 3 and len(blk.device[2]) == 4 and blk.device[2][3] == 2.5 and blk.tape.R == 4 and blk.n_var == 4
    # MIN and MAX: the parameter is the operand taken and the operand left, on either side
    x, p = POSITION_X, POSITION_P
    assert p[0] <= x[2] and x[0] < p[1] and p[0] < x[2] and p[1] > x[3] and not p[2] > x[1] and not x[3] > p[1]


@pytest.mark.parametrize("sense", ["MIN_SENSE", "MAX_SENSE"])
def test_data_derivatives_in_every_position(position_exact, sense):
    fm = position_model(sense)
    check_positions(Twin(fm), fm, POSITION_X, *position_exact, seed=len(sense))


# ---- a solution sensitivity with respect to an exponent:  min x2  s.t.  x2 - x1^q >= 0,  x1 - a == 0  (dpar = (q, a)).  Both rows are
# active at x* = (a, a^q) with lam* = (1, q a^(q-1)): a vertex, so d x*/dq = (0, a^q log a) and d lam*/dq = (0, a^(q-1) (1 + q log a)).
EXPONENT_SCENARIOS = ((2.5, 1.3), (1.5, 0.8), (3.0, 2.0))


def exponent_model(q=2.5, a=1.3):
    x = variables(2)
    p = parameters([q, a])
    fm = FunctionModel(2, np.full(2, 0.1), np.full(2, 50.0))
    fm.start = {1: 1.0, 2: 1.0}
    fm.nlp = ExprBlock([(x[1] - nx.pow(x[0], p[0]), 0.0, np.inf), (x[0] - p[1], 0.0, 0.0)], objective=1.0 * x[1], n=2, parameters=p)
    return fm


def exponent_solution(q, a):
    """(x*, lam*, d x*/dq, d lam*/dq) in closed form."""
    la = float(np.log(a))
    return (np.array([a, a ** q]), np.array([1.0, q * a ** (q - 1.0)]), np.array([0.0, a ** q * la]),
            np.array([0.0, a ** (q - 1.0) * (1.0 + q * la)]))


@pytest.mark.parametrize("q,a", EXPONENT_SCENARIOS)
def test_solution_sensitivity_to_an_exponent_parameter(q, a):
    from activesetmethods_amd import sensitivity
    fm = exponent_model(q, a)
    x, lam, wx, wl = exponent_solution(q, a)
    rs, bs = np.ones(2, np.int32), np.zeros(2, np.int32)
    pr = fm.to_problem()
    assert np.abs(pr.eval_grad_f(x, np.zeros(2)) - sensitivity.dense_jacobian(fm, x).T @ lam).max() <= 1e-14 * lam.max()      # a KKT point
    dc = np.zeros(len(fm.nlp.device[2]))                               # (q, a, the literal 1.0 of the objective)
    dc[0] = 1.0
    u, w = fm.nlp.data_cross(x, lam, dc, fm.objective_scale)
    dx, dlam, dz = sensitivity.kkt_reference(fm, x, lam, rs, bs, u, w)
    print("q %g a %g: dx %r (exact %r), dlam %r (exact %r)" % (q, a, dx, wx, dlam, wl))
    assert np.abs(dx - wx).max() <= KKT_BAR * max(1.0, np.abs(wx).max()) and np.abs(dlam - wl).max() <= KKT_BAR * max(1.0, np.abs(wl).max())
    assert wx[1] != 0.0 and wl[1] != 0.0 and not dz.any()
    for gx, gl in ((np.array([1.0, -2.0]), np.array([0.5, 3.0])), (np.array([0.0, 1.0]), np.array([-1.25, 0.0]))):
        out = sensitivity.adjoint_reference(fm, x, lam, rs, bs, gx, gl)[0]
        want = float(gx @ wx + gl @ wl)
        assert abs(out[0] - want) <= KKT_BAR * max(1.0, abs(want)), (out[0], want)


# ------------------------------------------------------------------------------------------------ ASIN and ACOS: nothing lost to cancellation
def check_asin_acos(api, fm, recs, xv, L):
    """The first and second derivatives of the plain ASIN and ACOS rows within K eps |E| - without C.  sqrt((1 - u) (1 + u)) has no
    cancellation to excuse: 1 - u is exact for 1/2 <= u <= 2 and one rounding otherwise, so every operation of the statements is a
    relative error of eps / 2 and K of them stay within K eps |E|.  (sqrt(1 - u*u) lost 2.5e4 eps |E| at u = 0.999999 and 9e4 at
    -0.9999999, which C - 5e5 |E| there - would have let pass.)  Returns the worst error / bar of each order."""
    rows = [r for r in recs if r.is_row and not r.data and r.kind in ("asin", "acos")]
    assert len(rows) == 11
    lam = np.ones(sum(1 for r in recs if r.is_row))
    jr, jc, jv = api.jacobian(xv)
    J = {(int(i), int(j)): v for i, j, v in zip(jr, jc, jv)}
    hr, hc, hv = api.hessian(xv, 1.0, lam)
    H = {(int(i), int(j)): v for i, j, v in zip(hr, hc, hv)}
    worst = [0.0, 0.0]
    for r in rows:
        for order, got in ((1, J[(r.index, r.xa)]), (2, H[(r.xa, r.xa)])):
            E, _ = REF.entry(r, *(("xa",) * order))
            q = ratio(got, E, K(r.kind, order, L, order - 1) * EPS * abs(E))
            print("%s(%r) derivative %d: error / (K eps |E|) = %.3g" % (r.kind, r.a, order, q))
            worst[order - 1] = max(worst[order - 1], q)
    return worst


def test_asin_and_acos_lose_nothing_to_cancellation():
    fm, recs, xv = table_model()
    assert max(check_asin_acos(Twin(fm), fm, recs, xv, NUMPY_L)) <= 1.0
