"""The LP skeleton's scaling and product kernels, launch by launch (asm_test_skeleton_stages, include/asm_hip.h), on the skeletons
asm_sublp_setup makes for the patterns of tests/skeleton_twins.py: dense_fast, general dense, sparse, and the sparse patterns padded with
explicit zeros until they are general dense.

  assemble   J, padding included, equals the oracle's assembled matrix bit for bit
  scaling    rel, c, rho, Ah (padding included) and d_spv_Ah equal the twin bit for bit - the twin equals oracle.lp_solver.scale_lp
             (tests/test_skeleton_stages_cpu.py)
  products   J x, J'y, Ah x, Ah'y within (L + 2) eps sum |a| |x| of the long-double reference; the route of either transposed product asserted
  norms      within (L + 2) eps ||row||; k_sp_row_norms equals k_row_norms bit for bit

Every case runs the four value kinds in turn on ONE handle (skeleton_twins.VALUE_KINDS), so every run after the first also meets the copies
the previous one left.  The worst ratio to the bar of each stage is printed per case (DESIGN.md quotes them)."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import skeleton_twins as T
from tests.util import abi_create, abi_setup, random_subproblem, oracle_solve, hip_solve, rel_err

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3
NAMES = [s[0] for s in T.SHAPES]
_DEVICE = {}          # case name -> (info, the outputs of its runs): one device pass per case, shared by the tests


def _d(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _info(lib, h):
    info = np.zeros(10, np.int64)
    assert lib.asm_test_skeleton_stages(h, 0, None, None, None, None, None, None, info.ctypes.data_as(C.POINTER(C.c_int64)), *[None] * 14) == 0
    return dict(zip(("n", "m", "M", "Mp", "ldn", "sp_ok", "sp_nnz", "dense_fast", "R", "chunk"), (int(v) for v in info)))


def _stages(lib, h, info, stages, dE=None, lb=None, ub=None, c_in=None, x=None, y=None):
    """One call of the hook; every output buffer is pre-filled with a sentinel, so an entry a stage does not write shows."""
    n, m, M, Mp, ldn = (info[k] for k in ("n", "m", "M", "Mp", "ldn"))
    f = lambda *shape: np.full(shape, -7.25)
    o = dict(J=f(Mp, ldn), rmax=f(M), rel=f(n), c=f(n), rho=f(M), Ah=f(Mp, ldn), spvAh=f(max(info["sp_nnz"], 1)), Jx=f(M), JTy=f(n), Ahx=f(M), AhTy=f(n),
             norms=f(m), spnorms=f(m))
    route = np.full(2, -9, np.int32)
    inf2 = np.zeros(10, np.int64)
    ins = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (dE, lb, ub, c_in, x, y)]
    rc = lib.asm_test_skeleton_stages(h, stages, *[_d(a) for a in ins], inf2.ctypes.data_as(C.POINTER(C.c_int64)),
                                      *[_d(o[k]) for k in ("J", "rmax", "rel", "c", "rho", "Ah", "spvAh", "Jx", "JTy", "Ahx", "AhTy")],
                                      route.ctypes.data_as(C.POINTER(C.c_int32)), _d(o["norms"]), _d(o["spnorms"]))
    assert rc == 0, lib.asm_last_error(h)
    o["route"] = route
    return o


def _handle_for(lib, case):
    h = abi_create(lib)
    sp = dict(case, v_lb=-np.ones(case["n"]), v_ub=np.ones(case["n"]))
    assert abi_setup(lib, h, sp) == 0, lib.asm_last_error(h)
    return h


def _device_runs(lib, name):
    if name not in _DEVICE:
        case, runs = T.runs(name)
        t0 = time.perf_counter()
        h = _handle_for(lib, case)
        t1 = time.perf_counter()
        info = _info(lib, h)
        outs = [_stages(lib, h, info, T.ALL, r["dE"], r["lb"], r["ub"], None, case["x"], case["y"]) for r in runs]
        lib.asm_destroy(h)
        print("%s: set-up %.2f s, %d runs %.2f s" % (name, t1 - t0, len(runs), time.perf_counter() - t1))
        _DEVICE[name] = (info, outs)
    return _DEVICE[name]


def _pattern_values(case, A):
    """The entries of A (M x n) in the order of the sparse copy: rows, then columns."""
    P = T.pattern_of(case)
    return A[P]


@pytest.mark.parametrize("name", NAMES)
def test_stages(hip_lib, name):
    """chunk-M4100 is the one case well above the others: its set-up allocates the 4112 x 4112 factor and the Python oracle assembles
    164 000 entries four times (the times are printed)."""
    case, runs = T.runs(name)
    info, outs = _device_runs(hip_lib, name)
    n, m, M = case["n"], case["m"], case["M"]
    ldn, Mp = T.dims(n, M)
    sparse, fast, route_J, route_Ah = T.EXPECT[case["kind"]]
    assert (info["n"], info["m"], info["M"], info["Mp"], info["ldn"]) == (n, m, M, Mp, ldn)
    assert (info["sp_ok"], info["dense_fast"]) == (sparse, fast)
    assert (info["R"], info["chunk"]) == T.chunks(M)
    if name in T.CHUNKS:
        assert (info["R"], info["chunk"]) == T.CHUNKS[name]
    if sparse:
        assert info["sp_nnz"] == int(T.pattern_of(case).sum())
    Lx, Ly = T.product_bars(case, bool(sparse))
    worst = dict(Jx=0.0, JTy=0.0, Ahx=0.0, AhTy=0.0, norms=0.0)
    for r, o in zip(runs, outs):
        tag = (name, r["vkind"])
        # stage 1
        assert _bits(o["J"]) == _bits(T.image(r["J"], n, M)), tag
        # stages 2 and 3
        for k in ("rmax", "rel", "c", "rho"):
            assert _bits(o[k]) == _bits(r[k]), (tag, k)
        assert _bits(o["Ah"]) == _bits(T.image(r["Ah"], n, M)), tag
        if sparse:
            assert _bits(o["spvAh"]) == _bits(_pattern_values(case, r["Ah"])), tag
        # stage 4
        assert tuple(o["route"]) == (route_J, route_Ah), tag
        for A, kx, ky in ((r["J"], "Jx", "JTy"), (r["Ah"], "Ahx", "AhTy")):
            ax, magx, aty, magy = T.products_ref(A, case["x"], case["y"])
            worst[kx] = max(worst[kx], T.ratio(o[kx], ax, magx, Lx))
            worst[ky] = max(worst[ky], T.ratio(o[ky], aty, magy, Ly))
        # stage 5
        nr = T.norms_ref(r["J"][:m])
        worst["norms"] = max(worst["norms"], T.ratio(o["norms"], nr, nr, Lx[:m] if sparse else np.full(m, ldn)))
        if sparse:
            assert _bits(o["spnorms"]) == _bits(o["norms"]), tag
        else:
            assert (o["spnorms"] == -7.25).all(), tag          # no sparse copy: the hook leaves the buffer alone
    print("%s: worst ratio to the bar: %s" % (name, "  ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("pair", ["300x70", "520x260"])
def test_sparse_and_padded_agree(hip_lib, pair):
    """The same pattern and dE on a sparse-pattern handle and on a handle whose pattern carries explicit zeros until it is general dense:
    identical rel, c, rho, Ah; the products agree within the bar of the dense route (the longer chain of the two)."""
    case, runs = T.runs("sparse-" + pair)
    si, so = _device_runs(hip_lib, "sparse-" + pair)
    pi, po = _device_runs(hip_lib, "padded-" + pair)
    assert (si["sp_ok"], pi["sp_ok"], pi["dense_fast"]) == (1, 0, 0)
    Ld = T.product_bars(case, False)
    for r, a, b in zip(runs, so, po):
        for k in ("J", "rmax", "rel", "c", "rho", "Ah"):
            assert _bits(a[k]) == _bits(b[k]), (pair, r["vkind"], k)
        for A, kx, ky in ((r["J"], "Jx", "JTy"), (r["Ah"], "Ahx", "AhTy")):
            _, magx, _, magy = T.products_ref(A, case["x"], case["y"])
            for k, mag, ld in ((kx, magx, Ld[0]), (ky, magy, Ld[1])):
                bar = (ld + 2) * T.LD(T.EPS) * mag
                assert (np.abs(a[k].astype(T.LD) - b[k]) <= bar).all(), (pair, r["vkind"], k)
        assert _bits(a["norms"]) == _bits(b["norms"]), (pair, r["vkind"])


CACHED = {"fast": (13, 120, 60, 1.0, 0.0, 0), "general": (12, 40, 25, 0.3, 0.3, 3), "sparse": (43, 300, 70, 0.04, 0.2, 5)}


@pytest.mark.parametrize("kind", list(CACHED))
def test_cached_state(hip_lib, kind):
    """One handle, no new set-up: all stages; all stages with a second dE (four entries in ten zero); then a second column scale c_in on the
    same J.  The second and third results equal, bit for bit, those of a fresh handle that has only ASSEMBLED the first dE (the range rows
    keep stale entries by specification; no gathered, scaled or transposed copy of the first dE exists there) - and the twins.  Then an
    ordinary solve on the handle against the oracle."""
    from activesetmethods_amd.subproblem import QpData, HipSubOptimizer
    sp = random_subproblem(*CACHED[kind])
    n, m = sp["n"], sp["m"]
    adj = np.nonzero((sp["c_lb"] < sp["c_ub"]) & (sp["c_lb"] > -T.INF) & (sp["c_ub"] < T.INF))[0]
    case = dict(n=n, m=m, M=m + len(adj), adj=adj, j_row=sp["j_row"], j_col=sp["j_col"], c_lb=sp["c_lb"], c_ub=sp["c_ub"])
    rng = np.random.default_rng(5)
    dE1 = sp["dE"]
    dE2 = rng.standard_normal(len(dE1))
    dE2[rng.random(len(dE1)) < 0.4] = 0.0
    ub = rng.uniform(0.1, 2.0, n); lb = -ub
    c2 = np.ldexp(1.0, rng.integers(-3, 4, n))
    x, y = rng.standard_normal(n), rng.standard_normal(case["M"])
    opt = HipSubOptimizer(QpData(sp['df'], sp['f'], sp['dE'], sp['E'], sp['c_lb'], sp['c_ub'], sp['v_lb'], sp['v_ub']), sp['j_row'], sp['j_col'])
    h = opt._h
    info = _info(hip_lib, h)
    assert (info["sp_ok"], info["dense_fast"]) == T.EXPECT[kind][:2]
    first = _stages(hip_lib, h, info, T.ALL, dE1, lb, ub, None, x, y)
    second = _stages(hip_lib, h, info, T.ALL, dE2, lb, ub, None, x, y)
    third = _stages(hip_lib, h, info, T.SCALE | T.PRODUCTS | T.NORMS, None, None, None, c2, x, y)

    def fresh(stages, c_in):
        g = abi_create(hip_lib)
        assert abi_setup(hip_lib, g, sp) == 0
        _stages(hip_lib, g, info, T.ASSEMBLE, dE1)
        out = _stages(hip_lib, g, info, stages, dE2, lb, ub, c_in, x, y)
        hip_lib.asm_destroy(g)
        return out

    keys2 = ("J", "rmax", "rel", "c", "rho", "Ah", "spvAh", "Jx", "JTy", "Ahx", "AhTy", "norms", "spnorms")
    f2 = fresh(T.ALL, None)
    for k in keys2:
        assert _bits(second[k]) == _bits(f2[k]), (kind, "second dE", k)
    f3 = fresh(T.ASSEMBLE | T.SCALE | T.PRODUCTS | T.NORMS, c2)
    for k in keys2[4:]:
        assert _bits(third[k]) == _bits(f3[k]), (kind, "second c", k)
    assert np.array_equal(second["route"], f2["route"]) and np.array_equal(third["route"], f3["route"])
    # ... and the twins, on the oracle's matrices of the same sequence
    orc = T.Oracle(case)
    J1 = orc.assemble(dE1)
    J2 = orc.assemble(dE2)
    if len(adj):
        assert not np.array_equal(J2[m:], T.Oracle(case).assemble(dE2)[m:])          # stale entries are in play
    for o, J, c_in in ((first, J1, None), (second, J2, None), (third, J2, c2)):
        if c_in is None:
            assert _bits(o["J"]) == _bits(T.image(J, n, case["M"]))
            rmax, rel, c = T.twin_colscale(J, lb, ub)
            assert _bits(o["rmax"]) == _bits(rmax) and _bits(o["rel"]) == _bits(rel) and _bits(o["c"]) == _bits(c)
        rho, Ah = T.twin_scale(J, c if c_in is None else c_in)
        assert _bits(o["rho"]) == _bits(rho) and _bits(o["Ah"]) == _bits(T.image(Ah, n, case["M"]))
        if info["sp_ok"]:
            assert _bits(o["spvAh"]) == _bits(_pattern_values(case, Ah))
        Lx, Ly = T.product_bars(case, bool(info["sp_ok"]))
        for A, kx, ky in ((J, "Jx", "JTy"), (Ah, "Ahx", "AhTy")):
            ax, magx, aty, magy = T.products_ref(A, x, y)
            assert T.ratio(o[kx], ax, magx, Lx) <= 1.0 and T.ratio(o[ky], aty, magy, Ly) <= 1.0
    # the hook leaves the handle usable
    _, o_out = oracle_solve(sp)
    _, h_out = hip_solve(sp, opt=opt)
    assert o_out[5] == h_out[5] == 1
    assert rel_err(h_out[0], o_out[0]) < 1e-10 and rel_err(h_out[1], o_out[1]) < 1e-10
    opt.close()


def test_refusals(hip_lib):
    """Before set-up, null pointers and an unknown stage bit: the project's error codes, and nothing runs (the outputs keep their fill)."""
    h = abi_create(hip_lib)
    info = np.full(10, -5, np.int64)
    ip = info.ctypes.data_as(C.POINTER(C.c_int64))
    none14 = [None] * 14
    assert hip_lib.asm_test_skeleton_stages(h, 0, None, None, None, None, None, None, ip, *none14) == ERR_STATE
    assert (info == -5).all()
    case = T.get_case("fast-33x17")
    sp = dict(case, v_lb=-np.ones(case["n"]), v_ub=np.ones(case["n"]))
    assert abi_setup(hip_lib, h, sp) == 0
    inf = _info(hip_lib, h)
    dE, lb, ub = T.case_values(case, "normal")
    good = _stages(hip_lib, h, inf, T.ALL, dE, lb, ub, None, case["x"], case["y"])
    n, M = case["n"], case["M"]
    f = lambda *shape: np.full(shape, -7.25)
    bufs = dict(J=f(inf["Mp"], inf["ldn"]), rmax=f(M), rel=f(n), c=f(n), rho=f(M), Ah=f(inf["Mp"], inf["ldn"]), spvAh=f(1), Jx=f(M), JTy=f(n), Ahx=f(M),
                AhTy=f(n), norms=f(case["m"]), spnorms=f(case["m"]))
    route = np.full(2, -9, np.int32)
    order = ("J", "rmax", "rel", "c", "rho", "Ah", "spvAh", "Jx", "JTy", "Ahx", "AhTy")

    def call(stages, ins, drop=(), info_ptr=ip):
        outs = [None if k in drop else _d(bufs[k]) for k in order]
        return hip_lib.asm_test_skeleton_stages(h, stages, *[_d(a) for a in ins], info_ptr, *outs,
                                                None if "route" in drop else route.ctypes.data_as(C.POINTER(C.c_int32)),
                                                None if "norms" in drop else _d(bufs["norms"]), _d(bufs["spnorms"]))

    full = [np.ascontiguousarray(a) for a in (dE, lb, ub)] + [None, case["x"], case["y"]]
    assert call(32, full) == ERR_ARG and call(T.ALL | 64, full) == ERR_ARG                    # unknown stage bits
    assert call(T.ALL, full, info_ptr=None) == ERR_ARG
    assert call(T.ALL, [None] + full[1:]) == ERR_ARG                                           # dE
    assert call(T.ALL, full[:1] + [None] + full[2:]) == ERR_ARG                                # lb
    assert call(T.ALL, full[:4] + [None, full[5]]) == ERR_ARG                                  # x
    assert call(T.ALL, full[:5] + [None]) == ERR_ARG                                           # y
    assert call(T.SCALE, full) == ERR_ARG                                                      # a scale without a c
    for k in ("J", "rmax", "rel", "c", "rho", "Ah", "Jx", "JTy", "Ahx", "AhTy", "route", "norms"):
        assert call(T.ALL, full, drop=(k,)) == ERR_ARG, k
    assert all((b == -7.25).all() for b in bufs.values()) and (route == -9).all()              # nothing ran, nothing was written
    # the refused calls left the device state alone: products and norms alone still give the earlier call's bits
    again = _stages(hip_lib, h, inf, T.PRODUCTS | T.NORMS, None, None, None, None, case["x"], case["y"])
    for k in ("Jx", "JTy", "Ahx", "AhTy", "norms"):
        assert _bits(again[k]) == _bits(good[k]), k
    assert call(T.ALL, full) == 0                                                              # and the handle works on
    hip_lib.asm_destroy(h)
