"""The kernels of the KKT column family (asm_kkt_kernels.hip.h) and of the SLP-EQP trial step (asm_eqp_kernels.hip.h), one launch at a time,
through the launch sites the drivers use.

The hook asm_test_kkt_stages loads a caller-made state into blocks with the solver's pitches and runs a list of stages.  Per kernel and case,
one hook call and these assertions against the long-double twins of tests/kkt_twins.py:
(a) rounding-bound outputs: |out - twin| <= gamma_k magnitude with constant 1;
(b) exact outputs - stop and boundary codes, active flags, the active-column word, iteration counts, counts, rows / bnd / side, wpos, gathers,
    scatters, cleared padding, and the sums whose order the header fixes - bitwise / integer equal;
(c) ownership: every double and int that the kernel does not own comes back bit for bit (util.SENTINEL / util.ISENT or the loaded state):
    d, r, p, hp and all scalar slots of frozen columns, the partial-sum slots of workgroups >= gridDim.x, dx0 when theta = 1, hscal / hseq
    when pub == 0; the arrival counters and the column counter are 0 after every call;
(d) geometry: grid_out equals the formula of the launch site;
(e) planted ties (small integers and powers of two: every sum is exact in any order) decide as the comparisons dictate;
(f) a column's bits do not depend on the number of columns or its place among them;
(g) two runs of the same call give bit-identical blocks;
(h) one chained round - cg_p, cg_curv, cg_step, axpby with the scalar block, cg_dir - with no host synchronisation between the stages.
`pytest -s` prints the largest ratio of (a) per kernel."""
import ctypes as C

import numpy as np
import pytest

from activesetmethods_amd import _lib
from tests import kkt_twins as T
from tests import util
from tests.test_kkt_stages_cpu import (FACE_NAMES, FACE_SIZES, RBLOCKS, ROWS, SHAPE_IDS, SHAPES, TRIAL_KINDS, TRIAL_NAMES, VBLOCKS, base_state, curv_case,
                                       dir_case, face_state, fill, freeze, normal_case, trial_state)

pytestmark = pytest.mark.gpu
KIND = {nm: i for i, nm in enumerate(T.KINDS)}
KK, LD, INF = T.KK, util.LD, float("inf")
FIXED_D = VBLOCKS + RBLOCKS + ["dlf", "mask", "rad", "scal", "part"]
FIXED_I = ["wrow", "wpos", "rows", "counts"]
SEPARATE = ["cnt", "act", "hscal", "hseq"]
WORST = {}
U32 = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = C.c_void_p()
    assert hip_lib.asm_create(0, C.byref(h)) == 0
    yield h
    hip_lib.asm_destroy(h)
    for k in sorted(WORST):
        print("largest ratio of (a), %-14s %.3f" % (k, WORST[k]))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


class Call:
    """The blocks of one state: the fixed buffers at the offsets the hook reports, every other array of the state behind them."""

    def __init__(self, lib, h, st):
        self.lib, self.h, self.st = lib, h, st
        d = st["dims"]
        lay = np.zeros(20, np.int64)
        rc = lib.asm_test_kkt_stages(h, d["n"], d["M"], d["nW"], d["capW"], d["cols"], _lib.i64ptr(lay), None, 0, None, 0, None, 0, None, None, None, None, None, 0, None)
        assert rc == 0, lib.asm_last_error(h)
        assert [int(v) for v in lay[:5]] == [d["ldn"], d["ldT"], d["Mp"], d["nWp"], d["nWg"]] and (int(lay[18]), int(lay[19])) == (T.KKM_SCAL, T.KK_MAXWG * T.KK_SLOTS)
        self.ndbl, self.nint = int(lay[5]), int(lay[6])
        o_vec, o_row, o_dlf, o_mask, o_rad, o_scal, o_part = (int(v) for v in lay[7:14])
        self.off = {nm: ("D", o_vec + k * T.KKM_CW * d["ldn"]) for k, nm in enumerate(VBLOCKS)}
        self.off.update({nm: ("D", o_row + k * T.KKM_CW * d["ldT"]) for k, nm in enumerate(RBLOCKS)})
        self.off.update(dlf=("D", o_dlf), mask=("D", o_mask), rad=("D", o_rad), scal=("D", o_scal), part=("D", o_part))
        self.off.update({nm: ("I", int(lay[14 + k])) for k, nm in enumerate(FIXED_I)})
        nD, nI, nL = self.ndbl, self.nint, 0
        for nm, a in st.items():
            if not isinstance(a, np.ndarray) or nm in self.off or nm in SEPARATE:
                continue
            if a.dtype == np.float64:
                self.off[nm], nD = ("D", nD), nD + a.size
            elif a.dtype == np.int32:
                self.off[nm], nI = ("I", nI), nI + a.size
            else:
                assert a.dtype == np.int64, (nm, a.dtype)
                self.off[nm], nL = ("L", nL), nL + a.size
        self.len = {"D": nD, "I": nI, "L": nL}

    def blocks(self):
        B = {"D": np.full(self.len["D"], util.SENTINEL), "I": np.full(self.len["I"], util.ISENT, np.int32), "L": np.zeros(max(self.len["L"], 1), np.int64)}
        for nm, (blk, o) in self.off.items():
            a = self.st[nm]
            B[blk][o:o + a.size] = a.reshape(-1)
        for nm in SEPARATE:
            B[nm] = self.st[nm].copy()
        return B

    def stage(self, kind, x=(), ix=(), lx=(), flag=(), s=(), ln=(), pub=0):
        g = _lib.KktStage()
        g.kind, g.pub = KIND[kind], pub
        for k in range(7):
            g.x[k] = g.ix[k] = -1
        for field, names in (("x", x), ("ix", ix), ("lx", lx)):
            for k, nm in enumerate(names):
                getattr(g, field)[k] = -1 if nm is None else self.off[nm][1]
        for k, v in enumerate(flag):
            g.flag[k] = int(v)
        for k, v in enumerate(s):
            g.s[k] = float(v)
        for k, v in enumerate(ln):
            g.len[k] = int(v)
        return g

    def run(self, stages, refuse=False, B=None, dims=None):
        d = dict(self.st["dims"], **(dims or {}))
        B = self.blocks() if B is None else B
        inp = {k: v.copy() for k, v in B.items()}
        arr = (_lib.KktStage * max(len(stages), 1))(*stages)
        grid = np.zeros(max(len(stages), 1), np.uint32)
        rc = self.lib.asm_test_kkt_stages(self.h, d["n"], d["M"], d["nW"], d["capW"], d["cols"], _lib.i64ptr(np.zeros(20, np.int64)), _lib.dptr(B["D"]), len(B["D"]),
                                          _lib.i32ptr(B["I"]), len(B["I"]), _lib.i64ptr(B["L"]), self.len["L"], B["cnt"].ctypes.data_as(U32), B["act"].ctypes.data_as(U32),
                                          _lib.dptr(B["hscal"]), B["hseq"].ctypes.data_as(U32), arr, len(stages), grid.ctypes.data_as(U32))
        if refuse:
            assert rc == -1, rc
            for k in B:
                assert np.array_equal(bits(B[k]), bits(inp[k])), "a refused call changed block %s" % k
            return None
        assert rc == 0, self.lib.asm_last_error(self.h)
        return inp, B, [int(g) for g in grid[:len(stages)]]

    def view(self, B, nm):
        if nm in SEPARATE:
            return B[nm]
        blk, o = self.off[nm]
        return B[blk][o:o + self.st[nm].size]


def twin_of(st, kind, kw):
    """(outs, decisions, expected workgroups) of one stage from its arguments."""
    x, ix, lx, flag, s, ln = (kw.get(k, ()) for k in ("x", "ix", "lx", "flag", "s", "ln"))
    d = st["dims"]
    g = T.grids(d)
    fl = lambda k: bool(flag[k]) if len(flag) > k else False
    dec = []
    if kind == "gather":
        outs, grid = T.tw_gather(st, x[0], x[1]), g["gather"]
    elif kind == "gather_t":
        outs, grid = T.tw_gather_t(st, x[0], x[1], fl(0)), g["gather_t"]
    elif kind == "hess_product":
        outs, grid = T.tw_hess_product(st, x[0], x[1], x[2], st[lx[0]], st[lx[1]], st[lx[2]]), g["hess_product"]
    elif kind == "axpby":
        outs, grid = T.tw_axpby(st, x[0], x[1], x[2], s[0], s[1], masked=fl(0), scal=fl(1), rows=fl(2)), g["axpby_rows" if fl(2) else "axpby"]
    elif kind == "scatter":
        outs, grid = T.tw_scatter(st, x[0], x[1]), g["scatter"]
    elif kind == "cross_rhs":
        outs, grid = T.tw_cross_rhs(st, x[0], x[1], x[2], ln[0]), g["cross_rhs"]
    elif kind == "cross_rhs_cols":
        outs, grid = T.tw_cross_rhs(st, x[0], x[1], x[2], ln[0], ldc=ln[1]), g["cross_rhs_cols"]
    elif kind == "bound_rhs":
        outs, grid = T.tw_bound_rhs(st, x[0], x[1], x[2]), g["bound_rhs"]
    elif kind == "cg_p":
        outs, grid = T.tw_cg_p(st, x[0], x[1]), g["cg_p"]
    elif kind == "normal":
        (outs, dec), grid = T.tw_normal(st, x[0], s[0]), g["normal"]
    elif kind == "cg_curv":
        (outs, dec), grid = T.tw_cg_curv(st, x[0], x[1], x[2], x[3], fl(0)), g["cg_curv"]
    elif kind == "cg_step":
        outs, grid = T.tw_cg_step(st, x[0], x[1], x[2], x[3]), g["cg_step"]
    elif kind == "cg_dir":
        (outs, dec), grid = T.tw_cg_dir(st, x[0], int(fl(0)), s[0], kw.get("pub", 0), int(fl(1))), g["cg_dir"]
    elif kind == "finish":
        outs, grid = T.tw_finish(st, x[0], x[1], x[2], x[3], x[4], x[5], x[6] if len(x) > 6 else None), g["finish"]
    elif kind == "kkts_vals":
        outs, grid = T.tw_kkts_vals(st, x[0], x[1], st[lx[0]], st[lx[1]], ln[0]), T.grid_vals(ln[0])
    elif kind == "kkts_wpos":
        outs, grid = T.tw_kkts_wpos(st), 1
    elif kind == "kkts_mul_a":
        outs, grid = T.tw_kkts_mul_a(st, ix[0], ix[1], x[0], x[1], x[2]), g["kkts_mul_a"]
    elif kind == "kkts_mul_at":
        outs, grid = T.tw_kkts_mul_at(st, ix[0], ix[1], ix[2], x[0], x[1], x[2], fl(0)), g["kkts_mul_at"]
    elif kind == "eqp_face":
        outs, grid = T.tw_eqp_face(st, list(x) + list(ix), ln[0], ln[1], s[0]), T.grid_eqp(ln[0], ln[1])
    else:
        assert kind == "eqp_trial"
        outs, grid = T.tw_eqp_trial(st, list(x), ln[0])[0], T.grid_eqp(ln[0])
    return outs, dec, grid


def run_and_check(lib, h, st, specs, tag, twice=False):
    """One hook call of the stages `specs` = [(kind, arguments)] on the state st, checked (a) to (d) against the twins applied in turn;
    twice: (g) as well.  Returns (the call, the blocks it left, the twin's state, the outs of the last stage)."""
    call = Call(lib, h, st)
    stages = [call.stage(kind, **kw) for kind, kw in specs]
    inp, B, grid = call.run(stages)
    tw = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    want = {}          # buffer -> [value (long double), bound (-1: exact, -2: NaN, -3: owned only), owned]
    outs, want_grid = [], []
    for kind, kw in specs:
        outs, _, g = twin_of(tw, kind, kw)
        want_grid.append(g)
        for o in outs:
            if o.buf not in want:
                size = tw[o.buf].size
                want[o.buf] = [np.zeros(size, LD), np.full(size, -1.0, LD), np.zeros(size, bool)]
            val, err, own = want[o.buf]
            own[o.idx] = True
            if isinstance(o.err, str):
                err[o.idx] = -2.0 if o.err == "nan" else -3.0
            else:
                val[o.idx] = o.val
                err[o.idx] = -1.0 if o.err is None else o.err
        T.apply(tw, outs)
    assert grid == want_grid, (tag, grid, want_grid)                                                    # (d)
    owned = {k: np.zeros(len(v), bool) for k, v in B.items()}
    worst = 0.0
    for buf, (val, err, own) in want.items():
        got = call.view(B, buf)
        if buf in SEPARATE:
            owned[buf] |= own
        else:
            blk, o = call.off[buf]
            owned[blk][o:o + len(own)] |= own
        ex = own & (err == -1.0)
        ref = val[ex].astype(got.dtype)
        assert np.array_equal(bits(got[ex]), bits(ref)), (tag, buf, "exact", np.flatnonzero(ex)[np.flatnonzero(bits(got[ex]) != bits(ref))[:5]])   # (b)
        nan = own & (err == -2.0)
        assert np.isnan(got[nan]).all(), (tag, buf, "NaN expected")
        bd = own & (err >= 0.0)
        if bd.any():
            r = T.ratio(got[bd], val[bd], err[bd])
            worst = max(worst, r)
            assert r <= 1.0, (tag, buf, r)                                                                # (a)
    for k in B:                                                                                           # (c)
        keep = ~owned[k]
        bad = np.flatnonzero(bits(B[k])[keep] != bits(inp[k])[keep])
        assert bad.size == 0, (tag, "block %s: %d entries the kernel does not own have changed, the first at %d" % (k, bad.size, np.flatnonzero(keep)[bad[0]]))
    assert not B["cnt"].any(), (tag, "a counter is not back at 0", np.flatnonzero(B["cnt"]))
    name = specs[-1][0] if len(specs) == 1 else "round"
    WORST[name] = max(WORST.get(name, 0.0), worst)
    if twice:                                                                                             # (g)
        _, B2, _ = call.run(stages)
        for k in B:
            assert np.array_equal(bits(B[k]), bits(B2[k])), (tag, "two runs differ in block %s" % k)
    return call, B, tw, outs


def scal_of(call, B):
    return call.view(B, "scal")[:T.WORD].reshape(T.KKM_CW, T.KKM_SCAL)


# ---------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_are_refused_before_any_launch(hip_lib, handle):
    st, rng = base_state(33, 9, 3, 5, 3, 1)
    st["J"] = rng.standard_normal(9 * st["dims"]["ldn"])
    st["Aw"] = np.full(3 * st["dims"]["ldn"], util.SENTINEL)
    st["ptr"], st["col"] = np.arange(10, dtype=np.int32), rng.integers(0, 33, 9).astype(np.int32)
    st["val"] = rng.standard_normal(9)
    st["l_pptr"], st["l_pent"], st["l_poth"] = np.arange(34, dtype=np.int64), np.arange(33, dtype=np.int64), np.arange(33, dtype=np.int64)
    st["values"] = rng.standard_normal(33)
    call = Call(hip_lib, handle, st)
    good = [call.stage("gather", x=["J", "Aw"], ln=[9]), call.stage("kkts_mul_a", x=["val", "p", "tw"], ix=["ptr", "col"]),
            call.stage("hess_product", x=["p", "hp", "values"], lx=["l_pptr", "l_pent", "l_poth"], ln=[33])]
    assert call.run(good) is not None
    def broken(mod):
        B = call.blocks()
        stages = [call.stage("gather", x=["J", "Aw"], ln=[9]), call.stage("kkts_mul_a", x=["val", "p", "tw"], ix=["ptr", "col"]),
                  call.stage("hess_product", x=["p", "hp", "values"], lx=["l_pptr", "l_pent", "l_poth"], ln=[33])]
        dims = mod(B, stages) or {}
        call.run(stages, refuse=True, B=B, dims=dims)
    I = lambda nm: call.off[nm][1]
    def set_(blk, nm, k, v):
        def m(B, stages):
            B[blk][I(nm) + k] = v
        return m
    broken(set_("I", "wrow", 1, 9))                     # a working row outside [0, M)
    broken(set_("I", "wrow", 0, -1))
    broken(set_("I", "rows", 2, 9))
    broken(set_("I", "col", 4, 33))                     # a column index outside [0, n)
    broken(set_("I", "ptr", 3, 7))                      # a pointer list that decreases
    broken(set_("L", "l_poth", 5, 33))
    broken(set_("L", "l_pent", 5, 33))
    broken(set_("L", "l_pptr", 2, 9))
    def off_end(B, stages):
        stages[0].x[1] = len(B["D"]) - 5
    broken(off_end)
    def negative(B, stages):
        stages[1].x[0] = -1
    broken(negative)
    def few_rows(B, stages):
        stages[0].len[0] = 8
    broken(few_rows)
    def unknown(B, stages):
        stages[2].kind = 99
    broken(unknown)
    broken(lambda B, stages: dict(cols=65))
    broken(lambda B, stages: dict(cols=0))
    broken(lambda B, stages: dict(nW=6))                # more working rows than capW
    def short(B, stages):
        B["D"] = B["D"][:call.ndbl - 1].copy()
    broken(short)


def test_bad_lists_of_the_sparse_form_and_the_face_are_refused(hip_lib, handle):
    """row, pos, a loaded wpos, perm, ustart, twin and the LP's states: each out of range once, everything else in order."""
    st, rng = sparse_state(9, 25, 5, 2, 2, (0, 1, 3), (0, 1, 7, 8))
    fill(st, rng, ["dlw"])
    fst, _, tol = face_state(12, 5)
    st.update({k: fst[k] for k in FACE_NAMES})
    na = len(st["lp_rows"]) - 5
    assert na >= 1
    st["l_perm"], st["l_ustart"] = np.arange(6, dtype=np.int64), np.array([0, 2, 3, 6], np.int64)
    st["dE"], st["vals"] = rng.standard_normal(6), np.full(3, util.SENTINEL)
    call = Call(hip_lib, handle, st)

    def stages():
        return [call.stage("kkts_mul_at", x=["sp_val", "dlw", "tt"], ix=["sc_ptr", "sc_row", "sc_pos"], ln=[len(st["sp_val"])], flag=[1]),
                call.stage("kkts_vals", x=["dE", "vals"], lx=["l_perm", "l_ustart"], ln=[3, 6]),
                call.stage("eqp_face", x=FACE_NAMES[:7], ix=FACE_NAMES[7:], ln=[12, 5, na], s=[tol])]
    assert call.run(stages()) is not None
    for blk, nm, k, v in [("I", "sc_row", 1, 25), ("I", "sc_row", 0, -1), ("I", "sc_pos", 2, len(st["sp_val"])), ("I", "sc_ptr", 4, 0), ("I", "wpos", 3, 5), ("I", "wpos", 0, -2),
                          ("L", "l_perm", 4, 6), ("L", "l_perm", 0, -1), ("L", "l_ustart", 2, 1), ("L", "l_ustart", 0, -1), ("I", "twin", 1, na), ("I", "twin", 0, -2),
                          ("I", "lp_rows", 5, 2), ("I", "lp_rows", 0, -1), ("I", "lp_bnd", 11, 2), ("I", "lp_bnd", 0, -2)]:
        B = call.blocks()
        B[blk][call.off[nm][1] + k] = v
        call.run(stages(), refuse=True, B=B)
    for field, k, v in [("len", 2, 6), ("len", 0, -1), ("x", 6, -1), ("ix", 6, 10 ** 9), ("lx", 1, 10 ** 9)]:
        g = stages()
        getattr(g[2 if field != "lx" else 1], field)[k] = v
        call.run(g, refuse=True)


# ---------------------------------------------------------------------------------------------------- gathers and right-hand sides
@pytest.mark.parametrize("nW", ROWS[1:])
def test_gathers(hip_lib, handle, nW):
    n, M = 257, nW + 5
    for masked in (1, 0):
        st, rng = base_state(n, M, nW, nW + 2, 1, 20 + nW)
        ldn, ldT = st["dims"]["ldn"], st["dims"]["ldT"]
        st["J"] = rng.standard_normal(M * ldn)
        st["Aw"], st["AT"] = np.full((nW + 2) * ldn, util.SENTINEL), np.full(ldn * ldT + 7, util.SENTINEL)
        if masked:
            run_and_check(hip_lib, handle, st, [("gather", dict(x=["J", "Aw"], ln=[M]))], "gather nW=%d" % nW)
        run_and_check(hip_lib, handle, st, [("gather_t", dict(x=["J", "AT"], ln=[M], flag=[masked]))], "gather_t nW=%d masked=%d" % (nW, masked))


@pytest.mark.parametrize("cols", [1, 3, 8, 9, 16, 17, 32, 33, 64])
def test_hess_product_in_every_template(hip_lib, handle, cols):
    """Lists of 0 to 9 entries, a second workgroup, rows >= cols of V read but not written; bitwise against the loop in entry order."""
    n = 300
    st, rng = base_state(n, 4, 0, 1, cols, 30 + cols)
    ldn = st["dims"]["ldn"]
    st["p"] = rng.standard_normal(T.KKM_CW * ldn)          # all 64 rows are read
    cnt = rng.integers(0, 10, n)
    cnt[:3] = (0, 9, 1)
    pptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    nnz, nv = int(pptr[-1]), 57
    st["l_pptr"], st["l_pent"], st["l_poth"] = pptr, rng.integers(0, nv, nnz).astype(np.int64), rng.integers(0, n, nnz).astype(np.int64)
    st["values"] = rng.standard_normal(nv)
    run_and_check(hip_lib, handle, st, [("hess_product", dict(x=["p", "hp", "values"], lx=["l_pptr", "l_pent", "l_poth"], ln=[nv]))], "hess_product cols=%d" % cols)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_axpby_over_the_variables(hip_lib, handle, shape):
    n, cols = shape
    for variant, (b, masked, scal, out) in enumerate([("hraw", 1, 0, "r"), (None, 1, 0, "dx0"), ("tt", 1, 1, "r"), ("tt", 0, 0, "g")]):
        st, rng = base_state(n, 4, 0, 1, cols, 40 + variant)
        fill(st, rng, ["b_ru", "r", "tt", "hraw"])
        if scal:
            freeze(st, rng)
        a = "r" if out == "r" and scal else "b_ru"
        run_and_check(hip_lib, handle, st, [("axpby", dict(x=[a, b, out], s=[1.5, -0.75], flag=[masked, scal, 0]))], "axpby %s variant %d" % (shape, variant))


@pytest.mark.parametrize("nW", ROWS)
def test_kernels_over_the_working_rows(hip_lib, handle, nW):
    """axpby on the row blocks, scatter, bound_rhs (a row inside and outside W, delta and none), both cross_rhs kernels."""
    n, M, cols = 70, nW + 5, 3
    st, rng = base_state(n, M, nW, nW + 2, cols, 50 + nW)
    d = st["dims"]
    fill(st, rng, ["adx", "rww", "dlw"])
    run_and_check(hip_lib, handle, st, [("axpby", dict(x=["adx", "rww", "tw"], s=[1.0, 1.0], flag=[0, 0, 1]))], "axpby rows nW=%d" % nW)
    run_and_check(hip_lib, handle, st, [("axpby", dict(x=["dlw", "adx", "dlw"], s=[1.0, 1.0], flag=[0, 0, 1]))], "axpby rows in place nW=%d" % nW)
    run_and_check(hip_lib, handle, st, [("scatter", dict(x=["dlw", "dlf"]))], "scatter nW=%d" % nW)
    inW = set(st["wrow"][:nW].tolist())
    outside = [i for i in range(M) if i not in inW]
    st["rows"][:3] = [st["wrow"][0] if nW else 0, outside[0], st["wrow"][nW - 1] if nW else outside[1]]
    st["delta"] = np.array([2.5, 1.25, 0.0])
    for delta in ("delta", None):
        _, B, _, _ = run_and_check(hip_lib, handle, st, [("bound_rhs", dict(x=[delta, "b_ru", "rww"]))], "bound_rhs nW=%d" % nW)
    n_fn = M // 2
    st["cx"] = rng.standard_normal(n + M - n_fn)
    st["ru1"], st["rw1"] = np.full(n + 3, util.SENTINEL), np.full(nW + 3, util.SENTINEL)
    run_and_check(hip_lib, handle, st, [("cross_rhs", dict(x=["cx", "ru1", "rw1"], ln=[n_fn]))], "cross_rhs nW=%d" % nW)
    ldc = n + M - n_fn + 3
    st["cxc"] = rng.standard_normal(cols * ldc)
    run_and_check(hip_lib, handle, st, [("cross_rhs_cols", dict(x=["cxc", "b_ru", "rww"], ln=[n_fn, ldc]))], "cross_rhs_cols nW=%d" % nW)
    assert d["nW"] == nW and nW <= d["nWg"] and d["nWp"] <= d["ldT"]


# ---------------------------------------------------------------------------------------------------- the projected CG round
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_cg_p_and_cg_step(hip_lib, handle, shape):
    n, cols = shape
    st, rng = base_state(n, 4, 0, 1, cols, 60)
    fill(st, rng, ["r", "p", "hp", "d"])
    frozen = freeze(st, rng)
    run_and_check(hip_lib, handle, st, [("cg_p", dict(x=["r", "p"]))], "cg_p %s" % (shape,))
    call, B, _, _ = run_and_check(hip_lib, handle, st, [("cg_step", dict(x=["p", "hp", "d", "r"]))], "cg_step %s" % (shape,))
    for c in frozen:          # (c), spelled out: a frozen column's d and r keep their bits
        for nm in ("d", "r"):
            ldn = st["dims"]["ldn"]
            assert np.array_equal(bits(call.view(B, nm)[c * ldn:(c + 1) * ldn]), bits(st[nm][c * ldn:(c + 1) * ldn]))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_normal_step(hip_lib, handle, shape):
    n, cols = shape
    st, share = normal_case(n, cols)
    call, B, _, _ = run_and_check(hip_lib, handle, st, [("normal", dict(x=["dx0"], s=[share]))], "normal %s" % (shape,))
    S = scal_of(call, B)
    assert [S[c, KK["THETA"]] < 1.0 for c in range(cols)] == [c % 3 == 0 and np.any(st["dx0"].reshape(T.KKM_CW, -1)[c] != 0.0) for c in range(cols)]


@pytest.mark.parametrize("n", [33, 257, 16417])
def test_normal_step_on_the_threshold(hip_lib, handle, n):
    """nn = share * radius exactly (3-4-5 scaled by powers of two): theta = 1, dx0 is not written at all, Dt^2 = radius^2 - nn^2 exactly; one
    unit in the last place above: the step is scaled."""
    st, rng = base_state(n, 4, 0, 1, 3, 70)
    X = st["dx0"].reshape(T.KKM_CW, -1)
    X[:3] = 0.0
    X[0, [0, n - 1]], X[1, [0, n - 1]], X[2, [0, n - 1]] = (3.0, 4.0), (0.75, 1.0), (3.0, 4.0)
    st["rad"][:3] = (10.0, 2.5, np.nextafter(10.0, 0.0))
    call, B, _, outs = run_and_check(hip_lib, handle, st, [("normal", dict(x=["dx0"], s=[0.5]))], "normal tie n=%d" % n)
    S = scal_of(call, B)
    assert not any(o.buf == "dx0" and o.idx[0] < 2 * st["dims"]["ldn"] for o in outs)          # the twin leaves dx0 of columns 0 and 1 unowned
    assert list(S[:2, KK["THETA"]]) == [1.0, 1.0] and list(S[:2, KK["NNORM"]]) == [5.0, 1.25] and list(S[:2, KK["DT2"]]) == [75.0, 4.6875] and S[2, KK["THETA"]] < 1.0


def curv_spec(trust):
    return [("cg_curv", dict(x=["p", "hraw", "d", "hp"], flag=[int(trust)]))]


@pytest.mark.parametrize("trust", [False, True], ids=["plain", "tr"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_cg_curv(hip_lib, handle, shape, trust):
    n, cols = shape
    st = curv_case(n, cols, trust)
    call, B, tw, _ = run_and_check(hip_lib, handle, st, curv_spec(trust), "cg_curv %s tr=%d" % (shape, trust), twice=n in (257, 16417) and cols == 3)
    S, S0 = scal_of(call, B), T.scal2d(st)
    for c in range(cols):
        if S0[c, KK["STOP"]] != 0.0:          # (c), spelled out: every scalar slot and hp of a frozen column
            ldn = st["dims"]["ldn"]
            assert np.array_equal(bits(S[c]), bits(S0[c])) and np.array_equal(bits(call.view(B, "hp")[c * ldn:(c + 1) * ldn]), bits(st["hp"][c * ldn:(c + 1) * ldn]))
    G = T.grids(st["dims"])["gred"]
    assert G == {1: 1, 33: 1, 255: 1, 257: 2, 2049: 9, 16417: 64}[n]


def tie_state(n, cols=6, seed=80):
    """Columns of small integers on variables 0 and n - 1 (two workgroups apart where n > 256), everything else 0, no variable on a bound."""
    st, rng = base_state(n, 4, 0, 1, cols, seed)
    st["mask"][:n] = 1.0
    for nm in ("p", "hraw", "d", "r", "hp"):
        st[nm].reshape(T.KKM_CW, -1)[:cols] = 0.0
    return st


@pytest.mark.parametrize("n", [33, 257, 16417])
def test_cg_curv_on_its_thresholds(hip_lib, handle, n):
    """p'Hp exactly 0 and NaN; the trial norm exactly Dt^2; gap exactly 0 and below; Dt^2 = +inf with p'Hp <= 0."""
    st = tie_state(n, 7)
    P, HR, D, S = [st[nm].reshape(T.KKM_CW, -1) for nm in ("p", "hraw", "d")] + [T.scal2d(st)]
    e = [0, n - 1]
    # 0: p'Hp = 2 * 3 - 1 * 6 = 0, finite Dt^2 -> boundary code 2, alpha = tau = gap / (dp + sqrt(dp^2 + pp gap)) with d = 0: sqrt(gap / pp) = 2
    P[0, e], HR[0, e], S[0, KK["DT2"]] = (2.0, 1.0), (3.0, -6.0), 20.0
    # 1: the same direction, Dt^2 = +inf -> stop 2, active flag 0
    P[1, e], HR[1, e], S[1, KK["DT2"]] = (2.0, 1.0), (3.0, -6.0), INF
    # 2: p'Hp = NaN -> not > 0: boundary code 2
    P[2, e], HR[2, e], S[2, KK["DT2"]] = (2.0, 1.0), (np.nan, 1.0), 20.0
    # 3: p'Hp = 8, rg = 4 -> alpha = 1/2; d = (1, 0), p = (2, 2): dd + 2 alpha dp + alpha^2 pp = 1 + 2 + 2 = 5 = Dt^2 -> boundary code 1 (>=)
    P[3, e], HR[3, e], D[3, e], S[3, KK["RG"]], S[3, KK["DT2"]] = (2.0, 2.0), (2.0, 2.0), (1.0, 0.0), 4.0, 5.0
    # 4: the same with Dt^2 one unit in the last place above 5 -> inside, alpha = 1/2
    P[4, e], HR[4, e], D[4, e], S[4, KK["RG"]], S[4, KK["DT2"]] = (2.0, 2.0), (2.0, 2.0), (1.0, 0.0), 4.0, np.nextafter(5.0, 6.0)
    # 5: gap = Dt^2 - d'd = 0 with p'Hp < 0 -> tau = 0, boundary code 2
    P[5, e], HR[5, e], D[5, e], S[5, KK["DT2"]] = (1.0, 1.0), (-1.0, -1.0), (2.0, 1.0), 5.0
    # 6: gap < 0 and the trial point outside -> tau = 0, boundary code 1
    P[6, e], HR[6, e], D[6, e], S[6, KK["RG"]], S[6, KK["DT2"]] = (2.0, 2.0), (2.0, 2.0), (2.0, 1.0), 4.0, 4.0
    st["act"][:7] = 1
    call, B, _, _ = run_and_check(hip_lib, handle, st, curv_spec(True), "cg_curv ties n=%d" % n)
    Sg = scal_of(call, B)
    assert list(Sg[:7, KK["BND"]]) == [2.0, 0.0, 2.0, 1.0, 0.0, 2.0, 1.0]
    assert list(Sg[:7, KK["STOP"]]) == [0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0] and list(call.view(B, "act")[:7]) == [1, 0, 1, 1, 1, 1, 1]
    # tau: column 0 and 2 sqrt(20 / 5) = 2; column 3 gap = 4, dp = 2, pp = 8: 4 / (2 + sqrt(4 + 32)) = 1/2; columns 5 and 6: gap <= 0, tau = 0
    assert list(Sg[[0, 2, 3, 4, 5, 6], KK["ALPHA"]]) == [2.0, 2.0, 0.5, 0.5, 0.0, 0.0] and Sg[0, KK["PHP"]] == 0.0 and np.isnan(Sg[2, KK["PHP"]])
    # the plain form: exactly 0 and NaN are the curvature stop
    st2 = tie_state(n, 3)
    P, HR = (st2[nm].reshape(T.KKM_CW, -1) for nm in ("p", "hraw"))
    P[0, e], HR[0, e], P[1, e], HR[1, e], P[2, e], HR[2, e] = (2.0, 1.0), (3.0, -6.0), (2.0, 1.0), (np.nan, 1.0), (2.0, 1.0), (3.0, -5.0)
    st2["act"][:3] = 1
    call, B, _, _ = run_and_check(hip_lib, handle, st2, curv_spec(False), "cg_curv plain ties n=%d" % n)
    assert list(scal_of(call, B)[:3, KK["STOP"]]) == [2.0, 2.0, 0.0] and list(call.view(B, "act")[:3]) == [0, 0, 1]


def dir_spec(init, rtol, pub, tr):
    return [("cg_dir", dict(x=["r"], flag=[init, tr], s=[rtol], pub=pub))]


@pytest.mark.parametrize("mode", [(1, 0, 7), (0, 0, 8), (0, 1, 9), (0, 1, 0)], ids=["init", "round", "round-tr", "round-tr-unpublished"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_cg_dir(hip_lib, handle, shape, mode):
    n, cols = shape
    init, tr, pub = mode
    st, rtol = dir_case(n, cols, init, tr)
    call, B, tw, _ = run_and_check(hip_lib, handle, st, dir_spec(init, rtol, pub, tr), "cg_dir %s %s" % (shape, mode), twice=n in (257, 16417) and cols == 3)
    if pub == 0:          # (c), spelled out
        assert B["hscal"][0] == util.SENTINEL and B["hseq"][0] == 777
    else:
        assert B["hseq"][0] == pub and B["hscal"][0] == call.view(B, "scal")[T.WORD] == float(call.view(B, "act")[:cols].sum())


@pytest.mark.parametrize("n", [33, 257, 16417])
def test_cg_dir_on_its_thresholds(hip_lib, handle, n):
    """sqrt(g'g) = rtol R0 exactly (converged: <=) and one unit in the last place above (not); init with g0 = 0; a boundary code set in the
    same round stops the column whatever its residual."""
    st = tie_state(n, 4)
    R, S = st["r"].reshape(T.KKM_CW, -1), T.scal2d(st)
    e = [0, n - 1]
    R[0, e], R[1, e], R[2, e], R[3, e] = (3.0, 4.0), (3.0, 4.0), (3.0, 4.0), (0.0, 0.0)
    S[:4, KK["RG"]] = 50.0
    S[:4, KK["R0"]] = (20.0, np.nextafter(20.0, 0.0), 2.0, 1.0)          # rtol = 1/4: 5 <= 5; 5 <= 4.99..: no; 5 <= 0.5: no, but its boundary code is set
    S[2, KK["BND"]] = 1.0
    st["act"][:4] = 1
    call, B, _, _ = run_and_check(hip_lib, handle, st, dir_spec(0, 0.25, 3, 1), "cg_dir ties n=%d" % n)
    Sg = scal_of(call, B)
    assert list(Sg[:4, KK["STOP"]]) == [1.0, 0.0, 1.0, 1.0] and list(call.view(B, "act")[:4]) == [0, 1, 0, 0] and B["hscal"][0] == 1.0
    assert list(Sg[:3, KK["BETA"]]) == [0.5, 0.5, 0.5] and list(Sg[:3, KK["GG"]]) == [25.0] * 3
    st["r"].reshape(T.KKM_CW, -1)[1] = 0.0
    call, B, _, _ = run_and_check(hip_lib, handle, st, dir_spec(1, 0.25, 4, 1), "cg_dir init ties n=%d" % n)
    Sg = scal_of(call, B)
    assert list(Sg[:4, KK["STOP"]]) == [0.0, 1.0, 0.0, 1.0] and list(Sg[:4, KK["R0"]]) == [5.0, 0.0, 5.0, 0.0] and B["hscal"][0] == 2.0


@pytest.mark.parametrize("with_dx", [0, 1], ids=["solve", "step"])
@pytest.mark.parametrize("case", [(1, 0, 1), (33, 1, 3), (257, 31, 64), (2049, 33, 3), (16417, 65, 3), (300, 64, 1)], ids=lambda c: "n%d-W%d-c%d" % c)
def test_finish(hip_lib, handle, case, with_dx):
    n, nW, cols = case
    st, rng = base_state(n, nW + 3, nW, nW + 2, cols, 90 + nW)
    fill(st, rng, ["hdx", "b_ru", "jtl", "adx", "rww", "dx"])
    T.scal2d(st)[:, KK["THETA"]] = 0.25 + 0.5 * rng.random(T.KKM_CW)
    run_and_check(hip_lib, handle, st, [("finish", dict(x=["hdx", "b_ru", "jtl", "adx", "rww", "dz"] + (["dx"] if with_dx else [])))], "finish %s dx=%d" % (case, with_dx))


# ---------------------------------------------------------------------------------------------------- the sparse form
@pytest.mark.parametrize("nu", [1, 300, 5000])
def test_kkts_vals(hip_lib, handle, nu):
    st, rng = base_state(8, 4, 0, 1, 1, 100)
    dup = np.array([1, 2, 5])[rng.integers(0, 3, nu)]
    dup[:3] = (5, 1, 2)[:min(nu, 3)]
    ustart = np.concatenate([[0], np.cumsum(dup)]).astype(np.int64)
    nE = int(ustart[-1]) + 4
    st["l_perm"], st["l_ustart"] = rng.permutation(nE)[:int(ustart[-1])].astype(np.int64), ustart
    st["dE"], st["vals"] = rng.standard_normal(nE), np.full(nu + 3, util.SENTINEL)
    run_and_check(hip_lib, handle, st, [("kkts_vals", dict(x=["dE", "vals"], lx=["l_perm", "l_ustart"], ln=[nu, nE]))], "kkts_vals nu=%d" % nu)


def sparse_state(n, M, nW, cols, seed, row_lens, col_lens):
    """A CSR / CSC pattern whose working rows have the list lengths row_lens in turn and whose variables have col_lens in turn (as far as the
    pattern admits both: the CSC lists are made from the CSR ones, then padded rows are added to reach the wanted column lengths)."""
    st, rng = base_state(n, M, nW, nW + 2, cols, seed)
    rows_of = [[] for _ in range(n)]
    for j in range(n):
        want = col_lens[j % len(col_lens)]
        rows_of[j] = sorted(rng.choice(M, size=min(want, M), replace=False).tolist())
    entries = sorted((i, j) for j in range(n) for i in rows_of[j])
    ptr = np.zeros(M + 1, np.int32)
    for i, _ in entries:
        ptr[i + 1] += 1
    ptr = np.cumsum(ptr).astype(np.int32)
    col = np.array([j for _, j in entries], np.int32).reshape(-1)
    where = {e: k for k, e in enumerate(entries)}
    cptr = np.concatenate([[0], np.cumsum([len(r) for r in rows_of])]).astype(np.int32)
    row = np.array([i for j in range(n) for i in rows_of[j]], np.int32).reshape(-1)
    pos = np.array([where[(i, j)] for j in range(n) for i in rows_of[j]], np.int32).reshape(-1)
    st.update(sp_ptr=ptr, sp_col=np.concatenate([col, np.full(3, util.ISENT, np.int32)]), sc_ptr=cptr, sc_row=np.concatenate([row, np.full(3, util.ISENT, np.int32)]),
              sc_pos=np.concatenate([pos, np.full(3, util.ISENT, np.int32)]), sp_val=rng.standard_normal(len(entries) + 2))
    return st, rng


@pytest.mark.parametrize("nW", ROWS)
def test_sparse_products(hip_lib, handle, nW):
    """k_kkts_mul_a with 4 lanes per row on lists of 0, 1, 3, 4, 5, 9 entries; k_kkts_mul_at with 8 lanes per variable on lists of 0, 1, 7, 8, 9,
    17, rows outside W (wpos = -1), masked variables, with and without the mask; k_kkts_wpos."""
    M, cols = nW + 20, 3
    n = 9 if nW < 33 else 300
    st, rng = sparse_state(n, M, nW, cols, 110 + nW, (0, 1, 3, 4, 5, 9), (0, 1, 7, 8, 9, 17))
    lens = [(0, 1, 3, 4, 5, 9)[i % 6] for i in range(M)]          # CSR lists of exactly 0, 1, 3, 4, 5, 9 entries: a pattern of its own for mul_a
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    st["a_ptr"], st["a_col"], st["a_val"] = ptr, rng.integers(0, n, int(ptr[-1])).astype(np.int32), rng.standard_normal(int(ptr[-1]))
    fill(st, rng, ["p", "dlw"])
    run_and_check(hip_lib, handle, st, [("kkts_mul_a", dict(x=["a_val", "p", "tw"], ix=["a_ptr", "a_col"]))], "kkts_mul_a nW=%d" % nW)
    for masked in (1, 0):
        run_and_check(hip_lib, handle, st, [("kkts_mul_at", dict(x=["sp_val", "dlw", "tt"], ix=["sc_ptr", "sc_row", "sc_pos"], ln=[len(st["sp_val"])], flag=[masked]))],
                      "kkts_mul_at nW=%d masked=%d" % (nW, masked))
    st["wpos"][:] = util.ISENT
    run_and_check(hip_lib, handle, st, [("kkts_wpos", {}), ("kkts_mul_at", dict(x=["sp_val", "dlw", "tt"], ix=["sc_ptr", "sc_row", "sc_pos"], ln=[len(st["sp_val"])], flag=[1]))],
                  "kkts_wpos nW=%d" % nW)


def test_kkts_wpos_over_more_rows_than_one_pass(hip_lib, handle):
    st, _ = base_state(8, 2500, 65, 67, 1, 120)
    st["wpos"][:] = util.ISENT
    run_and_check(hip_lib, handle, st, [("kkts_wpos", {})], "kkts_wpos M=2500")


# ---------------------------------------------------------------------------------------------------- the SLP-EQP trial step
def face_spec(n, m, na, tol):
    return [("eqp_face", dict(x=FACE_NAMES[:7], ix=FACE_NAMES[7:], ln=[n, m, na], s=[tol]))]


@pytest.mark.parametrize("n,m", FACE_SIZES)
def test_eqp_face(hip_lib, handle, n, m):
    """m > n, m < n, m = 0, equalities, range rows with active and inactive twins, g_L = -inf, infinite variable bounds with a nonzero LP state,
    x on, inside (tol / 2) and outside (3 tol) the activity tolerance, 2 workgroups and the 64-workgroup clamp."""
    st, P, tol = face_state(n, m)
    na = len(st["lp_rows"]) - m
    call, B, _, _ = run_and_check(hip_lib, handle, st, face_spec(n, m, na, tol), "eqp_face n=%d m=%d" % (n, m), twice=True)
    assert T.grid_eqp(n, m) == {12: 1, 7: 1, 300: 2, 16417: 64}[max(n, m)]


@pytest.mark.parametrize("n", [40, 300])
def test_eqp_face_on_the_tolerance(hip_lib, handle, n):
    """|x - bound| = tol (1 + |bound|) exactly is active (<=), one unit in the last place further is not: bounds -1 and 3, tol = 2^-10."""
    st, P, _ = face_state(n, 3)
    tol = 2.0 ** -10
    st["x_L"][:], st["x_U"][:] = -1.0, 3.0
    st["lp_bnd"][:] = np.where(np.arange(n) % 2 == 0, -1, 1)
    on = np.where(st["lp_bnd"] == -1, -1.0 + 2.0 * tol, 3.0 - 4.0 * tol)
    off = np.where(st["lp_bnd"] == -1, np.nextafter(-1.0 + 2.0 * tol, 1.0), np.nextafter(3.0 - 4.0 * tol, 0.0))
    st["x"][:] = np.where(np.arange(n) % 4 < 2, on, off)
    call, B, _, _ = run_and_check(hip_lib, handle, st, face_spec(n, 3, len(st["lp_rows"]) - 3, tol), "eqp_face tie n=%d" % n)
    assert list(call.view(B, "f_bnd")) == [0 if j % 4 >= 2 else (-1 if j % 2 == 0 else 1) for j in range(n)]


@pytest.mark.parametrize("kind", sorted(TRIAL_KINDS))
@pytest.mark.parametrize("n", [1, 257, 16417])
def test_eqp_trial(hip_lib, handle, n, kind):
    st = trial_state(n, kind)
    call, B, _, _ = run_and_check(hip_lib, handle, st, [("eqp_trial", dict(x=TRIAL_NAMES, ln=[n]))], "eqp_trial n=%d %s" % (n, kind), twice=kind == "cut")
    out = call.view(B, "t_out")
    if n > 1:
        assert out[0] == TRIAL_KINDS[kind]
    if kind in ("on_bound", "outside", "zero"):
        assert out[3] == 0.0 and out[1] == 0.0 and not call.view(B, "t_d").any()


# ---------------------------------------------------------------------------------------------------- (f) column independence
@pytest.mark.parametrize("n", [257, 16417])
def test_a_column_does_not_depend_on_its_neighbours(hip_lib, handle, n):
    """The same column data alone, as column 5 of 7 and as column 63 of 64: bit-identical vectors and scalars in normal, cg_curv (both forms),
    cg_dir and finish."""
    base, rng = base_state(n, 8, 5, 7, 1, 130)
    names = ["p", "hraw", "d", "r", "dx0", "hdx", "b_ru", "jtl", "adx", "rww", "dx"]
    fill(base, rng, names)
    ldn, ldT = base["dims"]["ldn"], base["dims"]["ldT"]
    base["hraw"][:ldn] = 3.0 * base["p"][:ldn] + 0.01 * base["hraw"][:ldn]
    T.scal2d(base)[0, KK["DT2"]] = 1e6
    base["rad"][0] = 0.1
    specs = [("normal", dict(x=["dx0"], s=[0.8])), ("cg_curv", dict(x=["p", "hraw", "d", "hp"], flag=[1])), ("cg_curv", dict(x=["p", "hraw", "d", "q"], flag=[0])),
             ("cg_dir", dict(x=["r"], flag=[0, 1], s=[1e-3], pub=2)), ("finish", dict(x=["hdx", "b_ru", "jtl", "adx", "rww", "dz", "dx"]))]
    results = []
    for place, cols in ((0, 1), (5, 7), (63, 64)):
        st, rng2 = base_state(n, 8, 5, 7, cols, 131 + cols)
        st["mask"], st["wrow"], st["wpos"] = base["mask"].copy(), base["wrow"].copy(), base["wpos"].copy()
        fill(st, rng2, names)
        for nm in names + ["hp", "q", "dz"]:
            ld = ldn if nm in VBLOCKS else ldT
            st[nm][place * ld:(place + 1) * ld] = base[nm][:ld]
        T.scal2d(st)[place] = T.scal2d(base)[0]
        T.scal2d(st)[:, KK["DT2"]] = 1e6
        st["rad"][:] = 0.1
        st["rad"][place] = base["rad"][0]
        got = {}
        for kind, kw in specs:
            call = Call(hip_lib, handle, st)
            _, B, _ = call.run([call.stage(kind, **kw)])
            for nm in ("dx0", "hp", "q", "dz"):
                got[(kind, len(got), nm)] = call.view(B, nm)[place * ldn:(place + 1) * ldn].copy()
            got[(kind, len(got), "scal")] = scal_of(call, B)[place].copy()
        results.append(list(got.values()))
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------- (h) one chained round
@pytest.mark.parametrize("n", [257, 16417])
def test_one_round_chained_without_a_host_wait(hip_lib, handle, n):
    """cg_p, cg_curv, cg_step, axpby with the scalar block, cg_dir in one call: column 0 goes on, column 1 is frozen beforehand, column 2 stops
    in this round (its residual vanishes), column 3 is column 0 with Dt^2 exactly at its trial norm: in the trust-region form its k_kktm_cg_curv
    sets boundary code 1 and the k_kktm_cg_dir of the same round stops it.  Small integers and powers of two: every intermediate result is exact, so each stage's twin reads
    the bits the device reads and its bound holds as for a single stage; the scalars travel from kernel to kernel in HBM."""
    for trust in (0, 1):
        st = tie_state(n, 4, 140)
        e = [0, n - 1]
        R, P, HR, D, TT, S = [st[nm].reshape(T.KKM_CW, -1) for nm in ("r", "p", "hraw", "d", "tt")] + [T.scal2d(st)]
        TT[:4] = 0.0
        for c in (0, 1, 2, 3):
            R[c, e], P[c, e], D[c, e], TT[c, e] = (2.0, -4.0), (4.0, 8.0), (1.0, 2.0), (0.5, -0.25)
            S[c, KK["BETA"]], S[c, KK["RG"]], S[c, KK["R0"]], S[c, KK["DT2"]] = 0.5, 20.0, 64.0, 2.0 ** 20
        # p <- 0.5 p - r = (0, 8); hp_raw: column 0 (1, 2) -> p'Hp = 16, alpha = 20 / 16; column 2 (3, 5) -> p'Hp = 40, alpha = 1/2 and
        # r + alpha hp - tt = (2, -4) + (1.5, 2.5) - (3.5, -1.5) = 0
        # column 3: d'd + 2 alpha d'p + alpha^2 p'p = 5 + 40 + 100 = 145 = Dt^2; tau = 140 / (16 + sqrt(256 + 64 * 140)) = 140 / 112 = alpha
        HR[0, e], HR[1, e], HR[2, e], HR[3, e] = (1.0, 2.0), (1.0, 2.0), (3.0, 5.0), (1.0, 2.0)
        S[3, KK["DT2"]] = 145.0
        TT[2, e] = (3.5, -1.5)
        S[1, KK["STOP"]] = 1.0
        st["act"][:4] = (1, 0, 1, 1)
        specs = [("cg_p", dict(x=["r", "p"])), ("cg_curv", dict(x=["p", "hraw", "d", "hp"], flag=[trust])), ("cg_step", dict(x=["p", "hp", "d", "r"])),
                 ("axpby", dict(x=["r", "tt", "r"], s=[1.0, -1.0], flag=[1, 1, 0])), ("cg_dir", dict(x=["r"], flag=[0, trust], s=[2.0 ** -10], pub=11))]
        call, B, tw, _ = run_and_check(hip_lib, handle, st, specs, "round n=%d tr=%d" % (n, trust), twice=True)
        Sg = scal_of(call, B)
        assert list(Sg[:4, KK["STOP"]]) == [0.0, 1.0, 1.0, float(trust)] and list(call.view(B, "act")[:4]) == [1, 0, 0, 1 - trust]
        assert B["hscal"][0] == 2.0 - trust and B["hseq"][0] == 11 and Sg[3, KK["BND"]] == float(trust)
        assert list(Sg[[0, 2, 3], KK["ALPHA"]]) == [1.25, 0.5, 1.25] and Sg[2, KK["GG"]] == 0.0 and np.array_equal(bits(Sg[1]), bits(T.scal2d(st)[1]))
        ldn = st["dims"]["ldn"]
        for nm in ("d", "r", "p", "hp"):
            assert np.array_equal(bits(call.view(B, nm)[ldn:2 * ldn]), bits(st[nm][ldn:2 * ldn]))
