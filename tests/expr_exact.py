"""An exact reference for expression rows (activesetmethods_amd.nlexpr.Expr graphs): the value and its partial derivatives in mpmath.

A row is walked in mpmath as a function of its inputs - every variable and every CONST leaf it reaches, exponent CONSTs included, keyed
("x", j) and ("c", dpar slot) - at the float64 inputs taken exactly.  Derivatives come from mp.diff alone: no derivative formula is written
here, which is the point of the module.  Every number is formed at two precisions and the two must agree to 1e-25 relative; a number
that does not is an error of the reference, never a point to drop.  One case is not a disagreement: a derivative that is exactly 0
(d2 (u / y) / du2) leaves the stencil's rounding noise, 0 at one precision and 1e-5000 at the other - where, with the extra bits, both are below 1e-60 of the
size such a derivative has when it is not 0 (|row| / prod |in_i|^order_i) the number is 0.

    ref = ExactRow(root, slot_of_const, x, consts)
    E, C = ref.entry({("x", 0): 2})            d2 row / dx0^2 and C = sum_i |in_i| |dE / d in_i| over the row's inputs
    E, C = ref.entry({("x", 0): 1, ("c", 3): 1})

E is NaN where the derivative does not exist over the reals (d/dy of pow(u, y) at u < 0: the stencil leaves the reals).

Precision: mp.diff sizes its working precision for a function whose derivatives scale with its value.  exp at 1e-300 is not one - the
stencil values differ from 1 by 1e-300, both precisions round them to 1 and agree on a derivative of 0 - nor is atan at 1e100 (value
pi / 2, third derivative 6e-400).  So each level of differences is given the bits it loses: order times (precision + 10 + |log2 |in_i||),
on top of what the level above it needs (_pdiff); where the two precisions still disagree, 2000 more.

Steps: mp.diff's default step is absolute, 2^-(precision + 10) - at an input of 1e-300 the stencil crosses zero and pow turns complex.
Here the step of input i is relative, |in_i| 2^-(precision + 10) (for an input that is exactly 0: that times the smallest nonzero input of
the row, or 1), so a stencil never leaves the side of 0, of +-1 or of any other edge its float64 centre is on.

Choices a float64 sweep makes on the sign or the order of values are frozen at the centre, so that the reference is the smooth function
the sweep differentiates: ABS is sign * u with the centre's sign bit, MIN and MAX the operand chosen at the centre (ties and NaN: the
left one), and ATAN2 on its branch cut continues the centre's branch.  The kinks themselves are not this module's business: the tests
state them in closed form.
"""
import numpy as np
from mpmath import mp, mpf

from activesetmethods_amd import nlexpr as nx

DPS = (60, 80)                       # the two precisions (decimal digits); the reference is the second
AGREE = mpf(10) ** -25
EXTRA_BITS = (0, 2000)               # more bits for the stencil values where the two precisions disagree without them


class ReferenceError_(AssertionError):
    pass


def _inputs(root, slot):
    """The input keys of the graph in first-visit order, and its nodes in evaluation order."""
    keys, order, seen, stack = [], [], set(), [(root, False)]
    while stack:
        e, done = stack.pop()
        if id(e) in seen:
            continue
        if not done:
            stack.append((e, True))
            stack += [(a, False) for a in reversed(e.args) if id(a) not in seen]
            continue
        seen.add(id(e))
        order.append(e)
        if e.op == nx.CONST or e.op == nx.VAR:
            k = ("c", slot(e)) if e.op == nx.CONST else ("x", e.arg)
            if k not in keys:
                keys.append(k)
    return keys, order


def _f64_branches(order, key_of, base):
    """node id -> the choice the float64 sweep makes at the centre: the sign bit of ABS's operand, the operand MIN / MAX take, the branch
    of ATAN2 for a negative second argument.  Values by NumPy, as the host twin forms them (only their signs and order are used)."""
    un = dict(nx._NP_UNARY)
    un.update({nx.NEG: np.negative, nx.SQRT: np.sqrt, nx.EXP: np.exp, nx.LOG: np.log, nx.SIN: np.sin, nx.COS: np.cos})
    val, choice = {}, {}
    with np.errstate(all="ignore"):
        for e in order:
            a = [val[id(q)] for q in e.args]
            if e.op in (nx.CONST, nx.VAR):
                v = np.float64(base[key_of(e)])
            elif e.op == nx.POWI:
                v = nx._powi(np.float64(a[0]), int(e.arg))[0]
            elif e.op == nx.ADD:
                v = a[0] + a[1]
            elif e.op == nx.SUB:
                v = a[0] - a[1]
            elif e.op == nx.MUL:
                v = a[0] * a[1]
            elif e.op == nx.DIV:
                v = a[0] / a[1]
            elif e.op == nx.POW:
                v = np.power(a[0], a[1])
            elif e.op == nx.ATAN2:
                v = np.arctan2(a[0], a[1])
                choice[id(e)] = -1 if np.signbit(a[0]) else 1
            elif e.op in (nx.MIN, nx.MAX):
                c = bool(a[1] < a[0]) if e.op == nx.MIN else bool(a[1] > a[0])
                choice[id(e)] = 1 if c else 0
                v = a[1] if c else a[0]
            else:
                if e.op == nx.ABS:
                    choice[id(e)] = -1 if np.signbit(a[0]) else 1
                v = un[e.op](a[0])
            val[id(e)] = np.float64(v)
    return choice


class ExactRow:
    def __init__(self, root, slot, x, consts):
        """`slot`: CONST node -> dpar slot; x, consts: the float64 variables and dpar entries."""
        self.keys, self.order = _inputs(root, slot)
        self.root = root
        self.key_of = lambda e: ("c", slot(e)) if e.op == nx.CONST else ("x", e.arg)
        self.base = {k: float(consts[k[1]] if k[0] == "c" else x[k[1]]) for k in self.keys}
        self.choice = _f64_branches(self.order, self.key_of, self.base)
        nz = [abs(v) for v in self.base.values() if v != 0.0 and np.isfinite(v)]
        self.zero_scale = min(nz) if nz else 1.0
        self._memo = {}

    # ---- the walk
    def _value(self, args):
        val = {}
        for e in self.order:
            a = [val[id(q)] for q in e.args]
            o = e.op
            if o in (nx.CONST, nx.VAR):
                v = args[self.key_of(e)]
            elif o == nx.ADD:
                v = a[0] + a[1]
            elif o == nx.SUB:
                v = a[0] - a[1]
            elif o == nx.MUL:
                v = a[0] * a[1]
            elif o == nx.DIV:
                v = a[0] / a[1]
            elif o == nx.NEG:
                v = -a[0]
            elif o == nx.POWI:
                v = a[0] ** int(e.arg)
            elif o == nx.ABS:
                v = self.choice[id(e)] * a[0]
            elif o in (nx.MIN, nx.MAX):
                v = a[self.choice[id(e)]]
            elif o == nx.CBRT:
                v = mp.cbrt(a[0]) if a[0] >= 0 else -mp.cbrt(-a[0])
            elif o == nx.LOG2:
                v = mp.log(a[0]) / mp.log(2)
            elif o == nx.POW:
                v = mp.power(a[0], a[1])
            elif o == nx.ATAN2:
                u, y = a
                # on and beside the cut (y < 0) the centre's branch is continued: pi (or -pi) + atan(u / y) is atan2 there and analytic
                v = self.choice[id(e)] * mp.pi + mp.atan(u / y) if y < 0 else mp.atan2(u, y)
            else:
                v = {nx.SQRT: mp.sqrt, nx.EXP: mp.exp, nx.LOG: mp.log, nx.SIN: mp.sin, nx.COS: mp.cos, nx.TAN: mp.tan, nx.ASIN: mp.asin,
                     nx.ACOS: mp.acos, nx.ATAN: mp.atan, nx.SINH: mp.sinh, nx.COSH: mp.cosh, nx.TANH: mp.tanh, nx.LOG10: mp.log10,
                     nx.LOG1P: mp.log1p, nx.EXPM1: mp.expm1}[o](a[0])
            if not isinstance(v, mpf):
                if getattr(v, "imag", 0) != 0:
                    raise _Complex()
                v = mp.mpf(v.real) if hasattr(v, "real") else mpf(v)
            val[id(e)] = v
        return val[id(self.root)]

    def _pdiff(self, xs, orders, prec0, p_out, extra):
        """d^orders of the row at xs (one entry per key), good to p_out bits: mp.diff variable by variable, each with its relative step.
        A level of order n loses n (prec0 + 10 + |log2 |in_i||) bits to the differences of its stencil, so its values are formed with
        that many bits on top of p_out (mp.diff's addprec), the levels below it to that precision in turn."""
        for i, n in enumerate(orders):
            if n:
                break
        else:
            return self._value(dict(zip(self.keys, xs)))
        rest = orders[:i] + (0,) + orders[i + 1:]
        centre = mpf(self.base[self.keys[i]])
        size = abs(centre) if centre != 0 else mpf(self.zero_scale)
        need = p_out + n * (prec0 + 10 + int(abs(mp.log(size, 2))) + 1) + 32 + extra
        h = mp.ldexp(size, -(prec0 + 10))
        with mp.workprec(p_out):
            return mp.diff(lambda t: self._pdiff(xs[:i] + (t,) + xs[i + 1:], rest, prec0, need, extra), xs[i], n, h=h,
                           addprec=-((p_out * (n + 1) - need) // (2 * (n + 1))))

    def _at(self, orders, dps, extra):
        with mp.workdps(dps):
            try:
                return +self._pdiff(tuple(mpf(self.base[k]) for k in self.keys), orders, mp.prec, mp.prec, extra)
            except _Complex:
                return mp.nan

    def _scale(self, orders):
        """The size a derivative of these orders has when it is not 0: |row| / prod |in_i|^order_i at the centre."""
        with mp.workdps(DPS[1]):
            try:
                S = abs(self._value({k: mpf(v) for k, v in self.base.items()}))
            except _Complex:
                return mpf(0)
            for k, n in zip(self.keys, orders):
                S /= mpf(abs(self.base[k]) if self.base[k] != 0.0 else self.zero_scale) ** n
            return S

    def _number(self, orders):
        """One reference number: at both precisions, agreeing to 1e-25 relative."""
        if orders not in self._memo:
            for extra in EXTRA_BITS:
                lo, hi = (self._at(orders, d, extra) for d in DPS)
                if mp.isnan(lo) and mp.isnan(hi) or abs(lo - hi) <= AGREE * max(abs(lo), abs(hi)):
                    break
                if extra == EXTRA_BITS[-1] and max(abs(lo), abs(hi)) <= mpf(10) ** -DPS[0] * self._scale(orders):
                    hi = mpf(0)              # rounding noise of the stencil around a derivative that is 0 (d2 (u / y) / du2)
                    break
            else:
                raise ReferenceError_("the reference disagrees with itself: orders %r at %r: %s against %s" % (orders, self.base, mp.nstr(lo, 30), mp.nstr(hi, 30)))
            self._memo[orders] = hi
        return self._memo[orders]

    def number(self, orders):
        """E alone, as mpf, for the derivative named by {key: order}; 0 for a key the row does not reach."""
        if any(k not in self.keys for k in orders):
            return mpf(0)
        return self._number(tuple(int(orders.get(k, 0)) for k in self.keys))

    def entry(self, orders):
        """(E, C) as mpf for the derivative named by {key: order} (empty: the value).  A key the row does not reach: (0, 0)."""
        if any(k not in self.keys for k in orders):
            return mpf(0), mpf(0)
        o = tuple(int(orders.get(k, 0)) for k in self.keys)
        E = self._number(o)
        if mp.isnan(E):
            return E, mp.nan
        C = mpf(0)
        for i, k in enumerate(self.keys):
            v = self.base[k]
            if v != 0.0:
                dE = self._number(o[:i] + (o[i] + 1,) + o[i + 1:])
                if mp.isnan(dE):
                    continue                 # (E does not move along an input whose derivative is not real: no share of C)
                C += abs(mpf(v)) * abs(dE)
        return E, C


class _Complex(Exception):
    pass


def ratio(got, E, bar):
    """|got - E| / bar in mpmath; 0 for an exact hit, inf where the bar is 0 and the value is not hit, or where got is not finite."""
    got = float(got)
    if not np.isfinite(got):
        return float("inf")
    err = abs(mpf(got) - E)
    if err == 0:
        return 0.0
    return float(err / bar) if bar > 0 else float("inf")
