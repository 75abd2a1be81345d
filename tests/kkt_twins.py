"""Long-double twins of the kernels of asm_kkt_kernels.hip.h and asm_eqp_kernels.hip.h, one per stage of asm_test_kkt_stages.

A twin reads a state - a dict of NumPy arrays under the buffer names the caller chose, plus the fixed names `scal` (64 x 16 + 1 doubles),
`mask`, `rad`, `part`, `cnt`, `act`, `hscal`, `hseq`, `wrow`, `wpos`, `rows`, and the sizes in `dims` - and returns a list of Out: the
entries the kernel owns in a buffer, what they must hold, and how closely.

  err is None    exact: bitwise for doubles, equal for integers.  Gathers, scatters, cleared padding, codes, flags, counts, and the sums whose
                 order the header fixes with contraction off (k_kktm_hess_product, k_kkts_vals, k_eqp_face, t and d of k_eqp_trial), which
                 the twin forms as float64 loops in the kernel's order.
  err an array   |out - val| <= err, with err = gamma_k * magnitude (util.gamma): k the operations on the path, the magnitude the sum of
                 absolute terms.  For a sum of `len` products in any order k = len.  A scalar that is a function of such sums (alpha, tau,
                 theta, ...) carries the bound that follows from them operation by operation (class E below: every operation adds one
                 rounding of the result to the propagated input bounds; a fused multiply-add rounds less, so the bound holds for it too).
  err == "nan"   the entry must be a NaN;  err == "own": owned, its value not compared (the partial sums of a column whose sum is a NaN).

A twin with decisions also returns them as (name, distance from the threshold, rounding bound of that distance): a case whose distance is
not larger than its bound sits on the threshold, where the device may decide either way - tests/test_kkt_stages_cpu.py asserts that no
random case does, and the planted ties are exact by construction (small integers and powers of two: bound 0 in effect, any order)."""
import numpy as np

from tests import util

LD = util.LD
U = LD(util.U)
INF = float("inf")
KK = dict(RG=0, PHP=1, ALPHA=2, BETA=3, GG=4, R0=5, STOP=6, RSTAT=7, RFEAS=8, ITERS=9, THETA=10, DT2=11, BND=12, NNORM=13, MODEL=14, NSTEP=15)
KKM_SCAL, KKM_CW, KK_MAXWG, KK_SLOTS = 16, 64, 64, 4
WORD = KKM_CW * KKM_SCAL            # the active-column word behind the columns' scalar blocks
KINDS = ("gather", "gather_t", "hess_product", "axpby", "scatter", "cross_rhs", "cross_rhs_cols", "bound_rhs", "cg_p", "normal", "cg_curv", "cg_step",
         "cg_dir", "finish", "kkts_vals", "kkts_wpos", "kkts_mul_a", "kkts_mul_at", "eqp_face", "eqp_trial")
LA, LAT = 4, 8                      # lanes per working row / per variable of the sparse products


def round_up(x, a):
    return (x + a - 1) // a * a


def dims(n, M, nW, capW, cols):
    """The sizes asm_test_kkt_stages derives (include/asm_hip.h)."""
    return dict(n=n, M=M, nW=nW, capW=capW, cols=cols, ldn=round_up(n, 32), ldT=round_up(max(capW, 1), 32), Mp=max(round_up(max(M, 1), 16), 32),
                nWp=round_up(nW, 32), nWg=round_up(nW, 64))


def grids(d):
    """Workgroups (x times y) of every launch site from the sizes, as KktSites computes them."""
    n, nW, cols, ldn, ldT, nWp, nWg = (d[k] for k in ("n", "nW", "cols", "ldn", "ldT", "nWp", "nWg"))
    bl = lambda v, per=256: (v + per - 1) // per
    gred = min(bl(ldn), KK_MAXWG)
    return dict(gather=bl(ldn) * nWg, gather_t=bl(ldn, 64) * bl(nWp, 64), hess_product=bl(n), axpby=bl(ldn) * cols, axpby_rows=bl(nWg) * cols, scatter=bl(nWg) * cols,
                cross_rhs=bl(max(n, nW)), cross_rhs_cols=bl(max(n, nW)) * cols, bound_rhs=bl(max(ldn, ldT)) * cols, cg_p=bl(ldn) * cols, normal=cols,
                cg_curv=gred * cols, cg_step=bl(ldn) * cols, cg_dir=gred * cols, finish=cols, kkts_wpos=1, kkts_mul_a=bl(nWg * LA) * cols,
                kkts_mul_at=bl(ldn * LAT) * cols, gred=gred)


def grid_vals(nu):
    return min((nu + 255) // 256, 4096)


def grid_eqp(n, m=0):
    return min((max(n, m) + 255) // 256, KK_MAXWG)


class Out:
    """Entries `idx` (flat) of buffer `buf` must hold `val`: exactly (err None), within err, be NaN (err == "nan") or are just owned ("own")."""

    def __init__(self, buf, idx, val, err=None):
        self.buf, self.idx = buf, np.atleast_1d(np.asarray(idx, np.int64))
        self.val = np.atleast_1d(np.asarray(val))
        self.err = err if err is None or isinstance(err, str) else np.broadcast_to(np.atleast_1d(np.asarray(err, LD)), self.val.shape)
        assert self.idx.shape == self.val.shape, (buf, self.idx.shape, self.val.shape)


def ratio(out, val, err):
    """Largest |out - val| / err (util.bound_ratio with the bound handed over as gamma_1 times a magnitude)."""
    return util.bound_ratio(out, val, np.asarray(err, LD) / util.gamma(1), 1)


def apply(st, outs):
    """The state after the kernel, as the twin has it: every owned entry at its value rounded to the buffer's type."""
    for o in outs:
        flat = st[o.buf].reshape(-1)
        flat[o.idx] = np.nan if isinstance(o.err, str) else o.val.astype(flat.dtype)


# ---- a value with a bound on the error of its float64 evaluation on the device
class E:
    def __init__(self, v, e=0.0):
        self.v, self.e = np.asarray(v, LD), np.asarray(e, LD)


def _r(v, e):          # the result v of one operation on inputs whose errors propagate to e, then rounded once
    return E(v, e + U * (np.abs(v) + e))


def e_add(a, b):
    return _r(a.v + b.v, a.e + b.e)


def e_sub(a, b):
    return _r(a.v - b.v, a.e + b.e)


def e_mul(a, b):
    return _r(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e)


def e_div(a, b):
    den = np.abs(b.v) - b.e
    with np.errstate(divide="ignore", invalid="ignore"):
        q = a.v / b.v
        return _r(q, np.where(den > 0, (a.e + np.abs(q) * b.e) / den, np.inf))


def e_sqrt(a):
    v = np.sqrt(np.maximum(a.v, 0))
    return _r(v, v - np.sqrt(np.maximum(a.v - a.e, 0)))


def e_dot(a, b):
    """A sum of len products in any order, fused or not: gamma_len times the sum of the absolute products."""
    t = np.asarray(a, LD) * np.asarray(b, LD)
    return E(t.sum(), util.gamma(t.size) * np.abs(t).sum()) if t.size else E(0.0)


def scal2d(st):
    return st["scal"][:WORD].reshape(KKM_CW, KKM_SCAL)


def _sidx(c, name):
    return c * KKM_SCAL + KK[name]


def _wg_of(length, G):
    """The workgroup that handles entry j of a grid-stride loop over `length` entries with G workgroups of 256."""
    return (np.arange(length) // 256) % G


def _part_outs(outs, c, G, length, slot_terms):
    """The partial sums the G > 1 workgroups of column c store: slot -> (terms, kind).  A sum: within gamma_count of its terms."""
    if G <= 1:
        return
    nch = (length + 255) // 256
    w = np.arange(G)
    for slot, (terms, kind) in slot_terms.items():
        t = np.zeros(nch * 256, LD)
        t[:length] = np.asarray(terms, LD)[:length]
        t = t.reshape(nch, 256)
        val = np.array([t[k::G].sum() for k in range(G)], LD)
        mag = np.array([np.abs(t[k::G]).sum() for k in range(G)], LD)
        cnt = np.array([min(256 * len(range(k, nch, G)), length) for k in range(G)])
        outs.append(Out("part", (c * KK_MAXWG + w) * KK_SLOTS + slot, val, util.gamma(np.maximum(cnt, 1)) * mag))


# ---------------------------------------------------------------------------------------------------- gathers, right-hand sides
def tw_gather(st, J, Aw):
    d = st["dims"]
    nW, ldn = d["nW"], d["ldn"]
    Jm = st[J].reshape(-1, ldn)
    val = np.where(st["mask"][None, :] != 0.0, Jm[st["wrow"][:nW]], 0.0)
    return [Out(Aw, np.arange(nW * ldn), val.reshape(-1))]


def tw_gather_t(st, J, AT, masked):
    d = st["dims"]
    nW, nWp, ldn, ldT = d["nW"], d["nWp"], d["ldn"], d["ldT"]
    Jm = st[J].reshape(-1, ldn)
    g = Jm[st["wrow"][:nW]]
    if masked:
        g = np.where(st["mask"][None, :] != 0.0, g, 0.0)
    val = np.zeros((ldn, nWp))
    val[:, :nW] = g.T
    idx = np.arange(ldn)[:, None] * ldT + np.arange(nWp)[None, :]
    return [Out(AT, idx.reshape(-1), val.reshape(-1))]


def tw_hess_product(st, V, OUT, values, pptr, pent, poth):
    """Entry order, from 0.0, no contraction: a float64 loop - the same bits."""
    d = st["dims"]
    n, cols, ldn = d["n"], d["cols"], d["ldn"]
    Vm, vals = st[V].reshape(-1, ldn), st[values]
    g = np.zeros((cols, n))
    cnt = pptr[1:n + 1] - pptr[:n]
    for t in range(int(cnt.max()) if n else 0):
        rows = np.nonzero(cnt > t)[0]
        q = pptr[rows] + t
        g[:, rows] = g[:, rows] + vals[pent[q]][None, :] * Vm[:cols, poth[q]]
    idx = np.arange(cols)[:, None] * ldn + np.arange(n)[None, :]
    return [Out(OUT, idx.reshape(-1), g.reshape(-1))]


def tw_axpby(st, a, b, out, sa, sb, masked=True, scal=False, rows=False):
    d = st["dims"]
    length, ld = (d["nW"], d["ldT"]) if rows else (d["ldn"], d["ldn"])
    S = scal2d(st)
    outs = []
    free = st["mask"] != 0.0 if (masked and not rows) else np.ones(length, bool)
    for c in range(d["cols"]):
        if scal and not rows and S[c, KK["STOP"]] != 0.0:
            continue
        e = c * ld + np.arange(length)
        t1 = LD(sa) * st[a].reshape(-1)[e].astype(LD)
        val, mag, k = t1, np.abs(t1), 1
        if b is not None:
            t2 = LD(sb) * st[b].reshape(-1)[e].astype(LD)
            val, mag, k = t1 + t2, np.abs(t1) + np.abs(t2), 3
        outs.append(Out(out, e[free], val[free], util.gamma(k) * mag[free]))
        if not free.all():
            outs.append(Out(out, e[~free], np.zeros((~free).sum())))
    return outs


def tw_scatter(st, y, out):
    d = st["dims"]
    nW, ldT, Mp = d["nW"], d["ldT"], d["Mp"]
    w = st["wrow"][:nW].astype(np.int64)
    return [Out(out, c * Mp + w, st[y].reshape(-1)[c * ldT:c * ldT + nW]) for c in range(d["cols"])] if nW else []


def tw_cross_rhs(st, cx, ru, rww, n_fn, ldc=None):
    """ldc None: the one-column kernel (ru, rww plain vectors); else the column kernel on blocks."""
    d = st["dims"]
    n, nW = d["n"], d["nW"]
    w = st["wrow"][:nW].astype(np.int64)
    outs = []
    for c in range(1 if ldc is None else d["cols"]):
        x = st[cx].reshape(-1)[(0 if ldc is None else c * ldc):]
        outs.append(Out(ru, (0 if ldc is None else c * d["ldn"]) + np.arange(n), x[:n]))
        if nW:
            outs.append(Out(rww, (0 if ldc is None else c * d["ldT"]) + np.arange(nW), np.where(w >= n_fn, x[n + np.maximum(w - n_fn, 0)], 0.0)))
    return outs


def tw_bound_rhs(st, delta, ru, rww):
    d = st["dims"]
    nW, ldn, ldT = d["nW"], d["ldn"], d["ldT"]
    outs = []
    for c in range(d["cols"]):
        v = np.zeros(ldT)
        hit = np.nonzero(st["wrow"][:nW] == st["rows"][c])[0]
        v[hit] = -(st[delta][c] if delta is not None else 1.0)
        outs += [Out(ru, c * ldn + np.arange(ldn), np.zeros(ldn)), Out(rww, c * ldT + np.arange(ldT), v)]
    return outs


# ---------------------------------------------------------------------------------------------------- the projected CG round
def tw_cg_p(st, g, p):
    d = st["dims"]
    ldn, S = d["ldn"], scal2d(st)
    outs = []
    for c in range(d["cols"]):
        if S[c, KK["STOP"]] != 0.0:
            continue
        e = c * ldn + np.arange(ldn)
        t = LD(S[c, KK["BETA"]]) * st[p].reshape(-1)[e].astype(LD)
        gv = st[g].reshape(-1)[e].astype(LD)
        outs.append(Out(p, e, t - gv, util.gamma(2) * (np.abs(t) + np.abs(gv))))
    return outs


def tw_normal(st, dx0, share):
    """Returns (outs, decisions).  theta == 1: dx0 is not owned."""
    d = st["dims"]
    ldn = d["ldn"]
    outs, dec = [], []
    for c in range(d["cols"]):
        e = c * ldn + np.arange(ldn)
        v = st[dx0].reshape(-1)[e]
        rad = float(st["rad"][c])
        nn = e_sqrt(e_dot(v, v))
        sc = lambda name: _sidx(c, name)
        outs.append(Out("scal", sc("BND"), 0.0))
        if not np.isfinite(rad):
            outs += [Out("scal", sc("THETA"), 1.0), Out("scal", sc("NNORM"), nn.v, nn.e), Out("scal", sc("DT2"), INF)]
            continue
        cap = e_mul(E(share), E(rad))
        dec.append(("normal c%d: nn - share * radius" % c, float(nn.v - cap.v), float(nn.e + cap.e)))
        if nn.v > cap.v:
            theta = e_div(cap, nn)
            outs.append(Out("scal", sc("THETA"), theta.v, theta.e))
            sv = e_mul(E(np.broadcast_to(theta.v, v.shape), np.broadcast_to(theta.e, v.shape)), E(v))
            outs.append(Out(dx0, e, sv.v, sv.e))
            tn = e_mul(theta, nn)
        else:
            outs.append(Out("scal", sc("THETA"), 1.0))
            tn = nn
        dt2 = e_sub(e_mul(E(rad), E(rad)), e_mul(tn, tn))
        outs += [Out("scal", sc("NNORM"), tn.v, tn.e), Out("scal", sc("DT2"), np.maximum(dt2.v, 0), dt2.e)]
    return outs, dec


def tw_cg_curv(st, p, hp_raw, dvec, hp, trust):
    """Returns (outs, decisions)."""
    d = st["dims"]
    ldn, S, G = d["ldn"], scal2d(st), grids(d)["gred"]
    free = st["mask"] != 0.0
    outs, dec = [], []
    for c in range(d["cols"]):
        if S[c, KK["STOP"]] != 0.0:
            continue
        e = c * ldn + np.arange(ldn)
        v = np.where(free, st[hp_raw].reshape(-1)[e], 0.0)
        pj, dj = st[p].reshape(-1)[e], st[dvec].reshape(-1)[e]
        outs.append(Out(hp, e, v))
        sc = lambda name: _sidx(c, name)
        with np.errstate(invalid="ignore"):
            php = e_dot(pj, v)
        slots = {0: (pj.astype(LD) * v.astype(LD), "sum")}
        dt2 = E(S[c, KK["DT2"]]) if trust else E(INF)
        tau, gap = E(0.0), None
        if trust:
            dd, dp, pp = e_dot(dj, dj), e_dot(dj, pj), e_dot(pj, pj)
            slots.update({1: (dj.astype(LD) ** 2, "sum"), 2: (dj.astype(LD) * pj.astype(LD), "sum"), 3: (pj.astype(LD) ** 2, "sum")})
            if np.isfinite(dt2.v):
                gap = e_sub(dt2, dd)
                if gap.v > 0:
                    tau = e_div(gap, e_add(dp, e_sqrt(e_add(e_mul(dp, dp), e_mul(pp, gap)))))
        if np.isnan(php.v):
            outs.append(Out("scal", sc("PHP"), np.nan, "nan"))
        else:
            outs.append(Out("scal", sc("PHP"), php.v, php.e))
            _part_outs(outs, c, G, ldn, slots)
            dec.append(("cg_curv c%d: p'Hp against 0" % c, float(php.v), float(php.e)))
        if np.isnan(php.v) and G > 1:      # the partial sums of a NaN column: owned, not compared
            wg = np.arange(G)
            for slot in slots:
                outs.append(Out("part", (c * KK_MAXWG + wg) * KK_SLOTS + slot, np.full(G, np.nan), "own"))
        use_tau = False
        if not php.v > 0:
            if np.isfinite(dt2.v):
                outs.append(Out("scal", sc("BND"), 2.0))
                use_tau = True
            else:
                outs += [Out("scal", sc("STOP"), 2.0), Out("act", c, np.uint32(0))]
        else:
            alpha = e_div(E(S[c, KK["RG"]]), php)
            if trust:
                lhs = e_add(e_add(dd, e_mul(e_mul(E(2.0), alpha), dp)), e_mul(e_mul(alpha, alpha), pp))
                if np.isfinite(dt2.v):
                    dec.append(("cg_curv c%d: trial norm against Dt^2" % c, float(lhs.v - dt2.v), float(lhs.e)))
                if lhs.v >= dt2.v:
                    outs.append(Out("scal", sc("BND"), 1.0))
                    use_tau = True
            if not use_tau:
                outs.append(Out("scal", sc("ALPHA"), alpha.v, alpha.e))
        if use_tau:
            outs.append(Out("scal", sc("ALPHA"), tau.v, tau.e))
            dec.append(("cg_curv c%d: gap against 0" % c, float(gap.v), float(gap.e)))
    return outs, dec


def tw_cg_step(st, p, hp, dvec, r):
    d = st["dims"]
    ldn, S = d["ldn"], scal2d(st)
    outs = []
    for c in range(d["cols"]):
        if S[c, KK["STOP"]] != 0.0:
            continue
        e = c * ldn + np.arange(ldn)
        al = LD(S[c, KK["ALPHA"]])
        for tgt, src in ((dvec, p), (r, hp)):
            t, b = al * st[src].reshape(-1)[e].astype(LD), st[tgt].reshape(-1)[e].astype(LD)
            outs.append(Out(tgt, e, b + t, util.gamma(2) * (np.abs(b) + np.abs(t))))
    return outs


def tw_cg_dir(st, r, init, rtol, pub, tr):
    """Returns (outs, decisions)."""
    d = st["dims"]
    ldn, cols, S, G = d["ldn"], d["cols"], scal2d(st), grids(d)["gred"]
    act = st["act"].copy()
    outs, dec = [], []
    for c in range(cols):
        if not init and S[c, KK["STOP"]] != 0.0:
            continue
        v = st[r].reshape(-1)[c * ldn:(c + 1) * ldn]
        gg = e_dot(v, v)
        _part_outs(outs, c, G, ldn, {0: (v.astype(LD) ** 2, "sum")})
        sc = lambda name: _sidx(c, name)
        outs += [Out("scal", sc("RG"), gg.v, gg.e), Out("scal", sc("GG"), gg.v, gg.e)]
        if init:
            r0 = e_sqrt(gg)
            outs += [Out("scal", sc("R0"), r0.v, r0.e)] + [Out("scal", sc(nm), 0.0) for nm in ("BETA", "ALPHA", "PHP", "ITERS")]
            stop = 1.0 if gg.v == 0 else 0.0
        else:
            beta = e_div(gg, E(S[c, KK["RG"]]))
            outs += [Out("scal", sc("BETA"), beta.v, beta.e), Out("scal", sc("ITERS"), S[c, KK["ITERS"]] + 1.0)]
            sq, thr = e_sqrt(gg), e_mul(E(rtol), E(S[c, KK["R0"]]))
            dec.append(("cg_dir c%d: ||g|| against rtol ||g0||" % c, float(sq.v - thr.v), float(sq.e + thr.e)))
            stop = 1.0 if (sq.v <= thr.v or (tr and S[c, KK["BND"]] != 0.0)) else 0.0
        act[c] = 0 if stop else 1
        outs += [Out("scal", sc("STOP"), stop), Out("act", c, np.uint32(act[c]))]
    word = float(act[:cols].sum())
    outs.append(Out("scal", WORD, word))
    if pub:
        outs += [Out("hscal", 0, word), Out("hseq", 0, np.uint32(pub))]
    return outs, dec


def tw_finish(st, hdx, ru, jtl, adx, rww, dz, dx):
    d = st["dims"]
    n, nW, ldn, ldT, S = d["n"], d["nW"], d["ldn"], d["ldT"], scal2d(st)
    free = st["mask"][:n] != 0.0
    outs = []
    for c in range(d["cols"]):
        e = c * ldn + np.arange(n)
        get = lambda nm: st[nm].reshape(-1)[e].astype(LD)
        h, u_, jt = get(hdx), get(ru), get(jtl)
        v, ve = (h + u_) - jt, util.gamma(2) * (np.abs(h) + np.abs(u_) + np.abs(jt))
        outs.append(Out(dz, e[free], np.zeros(free.sum())))
        outs.append(Out(dz, e[~free], v[~free], ve[~free]))
        sc = lambda name: _sidx(c, name)
        outs.append(Out("scal", sc("RSTAT"), np.abs(v[free]).max() if free.any() else 0.0, ve[free].max() if free.any() else 0.0))
        theta = LD(S[c, KK["THETA"]]) if dx is not None else LD(1)
        if nW:
            q = c * ldT + np.arange(nW)
            a_, t_ = st[adx].reshape(-1)[q].astype(LD), theta * st[rww].reshape(-1)[q].astype(LD)
            outs.append(Out("scal", sc("RFEAS"), np.abs(a_ + t_).max(), (util.gamma(2) * (np.abs(a_) + np.abs(t_))).max()))
        else:
            outs.append(Out("scal", sc("RFEAS"), 0.0))
        if dx is not None:
            x = st[dx].reshape(-1)[e]
            model = e_add(e_dot(st[ru].reshape(-1)[e], x), e_mul(E(0.5), e_dot(x, st[hdx].reshape(-1)[e])))
            ns = e_sqrt(e_dot(x, x))
            outs += [Out("scal", sc("MODEL"), model.v, model.e), Out("scal", sc("NSTEP"), ns.v, ns.e)]
    return outs


# ---------------------------------------------------------------------------------------------------- the sparse form
def tw_kkts_vals(st, dE, vals, perm, ustart, nu):
    """k_assemble's sum: the duplicates in list order, from 0.0, no contraction - a float64 loop."""
    acc = np.zeros(nu)
    cnt = ustart[1:nu + 1] - ustart[:nu]
    for t in range(int(cnt.max()) if nu else 0):
        u = np.nonzero(cnt > t)[0]
        acc[u] = acc[u] + st[dE][perm[ustart[u] + t]]
    return [Out(vals, np.arange(nu), acc)]


def tw_kkts_wpos(st):
    d = st["dims"]
    M, nW = max(d["M"], 1), d["nW"]
    w = np.full(M, -1, np.int32)
    w[st["wrow"][:nW]] = np.arange(nW, dtype=np.int32)
    return [Out("wpos", np.arange(M), w)]


def tw_kkts_mul_a(st, ptr, col, val, V, T):
    d = st["dims"]
    nW, cols, ldn, ldT = d["nW"], d["cols"], d["ldn"], d["ldT"]
    Vm = st[V].reshape(-1, ldn)[:cols].astype(LD)
    outs = []
    for q in range(nW):
        r = int(st["wrow"][q])
        ks = np.arange(st[ptr][r], st[ptr][r + 1])
        j = st[col][ks]
        t = (st[val][ks].astype(LD) * st["mask"][j].astype(LD))[None, :] * Vm[:, j]
        outs.append(Out(T, np.arange(cols) * ldT + q, t.sum(axis=1), util.gamma(len(ks) + 2) * np.abs(t).sum(axis=1)))
    return outs


def tw_kkts_mul_at(st, cptr, row, pos, val, Y, V, masked):
    d = st["dims"]
    n, cols, ldn, ldT = d["n"], d["cols"], d["ldn"], d["ldT"]
    Ym = st[Y].reshape(-1, ldT)[:cols].astype(LD)
    res, err = np.zeros((cols, ldn), LD), np.zeros((cols, ldn), LD)
    for j in range(n):
        if masked and st["mask"][j] == 0.0:
            continue
        ks = np.arange(st[cptr][j], st[cptr][j + 1])
        p_ = st["wpos"][st[row][ks]]
        ks, p_ = ks[p_ >= 0], p_[p_ >= 0]
        if len(ks):
            t = st[val][st[pos][ks]].astype(LD)[None, :] * Ym[:, p_]
            res[:, j], err[:, j] = t.sum(axis=1), util.gamma(len(ks) + 1) * np.abs(t).sum(axis=1)
    idx = np.arange(cols)[:, None] * ldn + np.arange(ldn)[None, :]
    return [Out(V, idx.reshape(-1), res.reshape(-1), err.reshape(-1))]


# ---------------------------------------------------------------------------------------------------- the SLP-EQP trial step
def tw_eqp_face(st, names, n, m, tol):
    """names: E g_L g_U x x_L x_U rw | lp_rows lp_bnd twin rows bnd side counts.  Everything exact: one subtraction, compares, counts."""
    E_, gL, gU, x, xL, xU, rw, lp_rows, lp_bnd, twin, rows, bnd, side, counts = names
    outs = []
    G = grid_eqp(n, m)
    lo, up = st[gL][:m], st[gU][:m]
    tw = st[twin][:m]
    eq = lo == up
    lr = st[lp_rows]
    twin_on = (tw >= 0) & (lr[np.minimum(m + np.maximum(tw, 0), len(lr) - 1)] != 0) if m else np.zeros(0, bool)
    inn = eq | (st[lp_rows][:m] != 0) | twin_on
    upper = ~eq & (twin_on | ~(lo > -INF))
    with np.errstate(invalid="ignore"):
        rwv = np.where(inn, st[E_][:m] - np.where(upper, up, lo), 0.0)
    outs += [Out(rows, np.arange(m), inn.astype(np.int32)), Out(side, np.arange(m), np.where(inn, np.where(upper, 1, -1), 0).astype(np.int32)),
             Out(rw, np.arange(m), rwv)]
    xv, xl, xu, s = st[x][:n], st[xL][:n], st[xU][:n], st[lp_bnd][:n]
    with np.errstate(invalid="ignore"):
        lower = (s == -1) & (xl > -INF) & (np.abs(xv - xl) <= tol * (1.0 + np.abs(xl)))
        uppr = ~lower & (s == 1) & (xu < INF) & (np.abs(xv - xu) <= tol * (1.0 + np.abs(xu)))
    b = np.where(lower, -1, np.where(uppr, 1, 0)).astype(np.int32)
    outs += [Out(bnd, np.arange(n), b), Out(counts, [0, 1], np.array([inn.sum(), (b == 0).sum()], np.int32))]
    if G > 1:
        L = max(n, m)
        wg = _wg_of(L, G)
        for w in range(G):
            outs.append(Out("part", w * KK_SLOTS + 0, np.float64(inn[wg[:m] == w].sum())))
            outs.append(Out("part", w * KK_SLOTS + 1, np.float64((b[wg[:n] == w] == 0).sum())))
    return outs


def tw_eqp_trial(st, names, n):
    """names: dx x x_L x_U d out.  t and d are float64 in the kernel's own operations (contraction off): exact."""
    dx_, x_, xL, xU, d_, out = names
    dx, x, lo, hi = st[dx_][:n], st[x_][:n], st[xL][:n], st[xU][:n]
    t = 1.0
    upm, dn = dx > 0.0, dx < 0.0
    if upm.any():
        t = min(t, float(((hi[upm] - x[upm]) / dx[upm]).min()))
    if dn.any():
        t = min(t, float(((lo[dn] - x[dn]) / dx[dn]).min()))
    t = max(t, 0.0)
    dv = t * dx
    G = grid_eqp(n)
    nrm = e_sqrt(e_dot(dv, dv))
    outs = [Out(d_, np.arange(n), dv), Out(out, 0, t), Out(out, 1, nrm.v, nrm.e), Out(out, 2, np.abs(dv).max()), Out(out, 3, float((dv != 0.0).sum()))]
    if G > 1:
        wg = _wg_of(n, G)
        for w in range(G):
            sel = dv[wg == w]
            sq = e_dot(sel, sel)
            outs += [Out("part", w * KK_SLOTS + 0, sq.v, sq.e), Out("part", w * KK_SLOTS + 1, float((sel != 0.0).sum())),
                     Out("part", w * KK_SLOTS + 2, np.abs(sel).max() if sel.size else 0.0)]
    return outs, t


# ---------------------------------------------------------------------------------------------------- steps 3 to 6 from the stage twins
def _ld_cholesky(S):
    N = len(S)
    L = np.zeros((N, N), LD)
    for j in range(N):
        L[j, j] = np.sqrt(S[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _ld_solve(L, B):
    """Rows of B solved against S = L L' in long double."""
    N = len(L)
    Y = np.zeros(B.shape, LD)
    for i in range(N):
        Y[:, i] = (B[:, i] - Y[:, :i] @ L[i, :i]) / L[i, i]
    Z = np.zeros(B.shape, LD)
    for i in range(N - 1, -1, -1):
        Z[:, i] = (Y[:, i] - Z[:, i + 1:] @ L[i + 1:, i]) / L[i, i]
    return Z


def chain_columns(H, J, row_state, bound_state, RU, RW, radii=None, share=0.8, rtol=1e-12, max_iter=None):
    """kkt_columns of the library (steps 3 to 6) with every launch of the family replaced by its stage twin, in the driver's order and on the
    driver's blocks; the products with A, A', H and the substitutions are NumPy's in long double, rounded to float64 as the device stores
    them.  Returns per column (dx, dlam, dz, info) and the decisions the twins took."""
    n, m = H.shape[0], J.shape[0]
    W = np.nonzero(np.asarray(row_state) == 1)[0]
    nW, cols = len(W), len(RU)
    d = dims(n, m, nW, max(nW, 1), cols)
    ldn, ldT, Mp = d["ldn"], d["ldT"], d["Mp"]
    trust = radii is not None
    st = dict(dims=d, scal=np.zeros(WORD + 1), mask=np.zeros(ldn), rad=np.zeros(KKM_CW), part=np.zeros(KKM_CW * KK_MAXWG * KK_SLOTS), cnt=np.zeros(KKM_CW + 1, np.uint32),
              act=np.zeros(KKM_CW, np.uint32), hscal=np.zeros(1), hseq=np.zeros(1, np.uint32), wrow=np.zeros(Mp, np.int32), wpos=np.zeros(Mp, np.int32),
              rows=np.zeros(KKM_CW, np.int32), dlf=np.zeros(KKM_CW * Mp))
    st["mask"][:n] = np.asarray(bound_state) == 0
    st["wrow"][:nW] = W
    nF = int(st["mask"].sum())
    for nm in "b_ru dx0 d r p hraw hp tt dx hdx q jtl dz g".split():
        st[nm] = np.zeros(KKM_CW * ldn)
    for nm in "rww tw spare dlw adx".split():
        st[nm] = np.zeros(KKM_CW * ldT)
    if trust:
        st["rad"][:cols] = radii
    A = np.zeros((nW, ldn), LD)
    A[:, :n] = J[W].astype(LD) * st["mask"][None, :n]
    Jw, Hl = J[W].astype(LD), H.astype(LD)
    L = _ld_cholesky(A @ A.T) if nW else None
    V = lambda nm: st[nm].reshape(KKM_CW, -1)
    decisions = []

    def run(res):
        outs, dec = res if isinstance(res, tuple) else (res, [])
        apply(st, outs)
        decisions.extend(dec)

    def hess(src, dst):
        V(dst)[:cols, :n] = (V(src)[:cols, :n].astype(LD) @ Hl.T).astype(float)

    def mul_A(src, dst):
        V(dst)[:cols, :nW] = (V(src)[:cols].astype(LD) @ A.T).astype(float)

    def solve_S(src, dst):
        V(dst)[:cols, :nW] = _ld_solve(L, V(src)[:cols, :nW].astype(LD)).astype(float)

    def mul_AT(src, dst):
        V(dst)[:cols] = (V(src)[:cols, :nW].astype(LD) @ A).astype(float)

    def normal_back(b, t):
        solve_S(b, t)
        mul_AT(t, "tt")

    def project(v, scal):
        if nW == 0:
            return
        mul_A(v, "tw")
        normal_back("tw", "tw")
        run(tw_axpby(st, v, "tt", v, 1.0, -1.0, scal=scal))

    V("b_ru")[:cols, :n] = RU
    V("rww")[:cols, :nW] = np.asarray(RW)[:, W]
    if nW:
        normal_back("rww", "tw")
        run(tw_axpby(st, "tt", None, "dx0", -1.0, 0.0))
        mul_A("dx0", "adx")
        run(tw_axpby(st, "adx", "rww", "tw", 1.0, 1.0, rows=True))
        normal_back("tw", "tw")
        run(tw_axpby(st, "dx0", "tt", "dx0", 1.0, -1.0))
    if trust:
        run(tw_normal(st, "dx0", share))
    run_cg = nF > nW
    if max_iter is None:
        max_iter = 2 * (nF - nW) + 20
    if run_cg:
        hess("dx0", "hraw")
        run(tw_axpby(st, "b_ru", "hraw", "r", 1.0, 1.0))
        project("r", False)
        project("r", False)
        run(tw_cg_dir(st, "r", 1, rtol, 1, int(trust)))
        it = 0
        while st["hscal"][0] > 0 and it < max_iter:
            run(tw_cg_p(st, "r", "p"))
            hess("p", "hraw")
            run(tw_cg_curv(st, "p", "hraw", "d", "hp", trust))
            run(tw_cg_step(st, "p", "hp", "d", "r"))
            project("r", True)
            project("r", True)
            run(tw_cg_dir(st, "r", 0, rtol, 2 + it, int(trust)))
            it += 1
    run(tw_axpby(st, "dx0", "d", "dx", 1.0, 1.0))
    hess("dx", "hdx")
    if nW:
        run(tw_axpby(st, "hdx", "b_ru", "q", 1.0, 1.0))
        mul_A("q", "tw")
        solve_S("tw", "dlw")
        mul_AT("dlw", "tt")
        run(tw_axpby(st, "q", "tt", "g", 1.0, -1.0))
        mul_A("g", "tw")
        solve_S("tw", "tw")
        run(tw_axpby(st, "dlw", "tw", "dlw", 1.0, 1.0, rows=True))
        run(tw_scatter(st, "dlw", "dlf"))
        mul_A("dx", "adx")
        V("jtl")[:cols, :n] = (V("dlw")[:cols, :nW].astype(LD) @ Jw).astype(float)
    run(tw_finish(st, "hdx", "b_ru", "jtl", "adx", "rww", "dz", "dx" if trust else None))
    S = scal2d(st)
    res = []
    for c in range(cols):
        stop = int(S[c, KK["STOP"]]) if run_cg else 1
        info = dict(status=2 if stop == 2 else (1 if stop == 0 else 0), cg_iters=int(S[c, KK["ITERS"]]) if run_cg else 0, n_free=nF, n_rows=nW,
                    boundary=int(S[c, KK["BND"]]) if (run_cg and trust) else 0, res_stat=S[c, KK["RSTAT"]], res_feas=S[c, KK["RFEAS"]], theta=S[c, KK["THETA"]],
                    norm_normal=S[c, KK["NNORM"]], norm_step=S[c, KK["NSTEP"]], model=S[c, KK["MODEL"]], stop=stop)
        res.append((V("dx")[c, :n].copy(), st["dlf"].reshape(KKM_CW, Mp)[c, :m].copy(), V("dz")[c, :n].copy(), info))
    return res, decisions
