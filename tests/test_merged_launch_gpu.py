"""Every kernel family in MERGED launches of a scenario batch, launch by launch.

A kernel receives its arguments in one of two ways: as kernel arguments (a plain handle), or - in a merged launch of a scenario batch - from
entry blockIdx.z / gz of an argument table that the recorder packs (csrc/asm_batch.hip.h) and ASM_BARGS unpacks (csrc/asm_bt.hip.h).  The
stage tests (test_*_stages_gpu.py, test_kernels_gpu.py, test_builds_gpu.py) pin the first way against float128 / exact twins.  Here the same
hooks run on the fibers of a batch (asm_batch_test_run), and every output array, layout record, grid_out and status of every scenario must
equal, BYTE FOR BYTE, what the same call leaves on a plain handle - the call those tests check.  The merged path's correctness thereby
chains to the twins with no tolerance of its own.

Per family (inputs from the builders of the stage tests, one seed per scenario, the smallest case with a grid of several workgroups):
 1. three scenarios of the same shapes and stage list on three slots: every kernel in the merge table has operations == 3 * launches and
    nb == 3, the table is not empty, and it names the kernels a one-slot batch records for one of the scenarios;
 2. five scenarios on three slots: the second pass merges two fibers while the third is finished;
 3. three scenarios of which the middle one has another stage list (two stages in the other order, a stage left out) or another size: its
    operations stop matching inside a round and go out alone, the other two still merge - a kernel with nb == 2 and a launch with nb == 1
    must both occur;
 4. (skeleton and KKT) four slots in two groups, two scenarios merged on each group's stream.
`pytest -s` prints the kernels seen in a merged launch (nb >= 2) against the kernels of the library, and the ones not reached."""
import ctypes as C
import numpy as np
import pytest

from activesetmethods_amd import _lib
from tests import merged, util
from tests.merged import Capture, run_batch

pytestmark = pytest.mark.gpu


def _d(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


class Batches:
    def __init__(self, lib):
        self.lib = lib
        self.one, self.three, self.four = merged.make_batch(lib, 1), merged.make_batch(lib, 3), merged.make_batch(lib, 4, groups=2)

    def setup(self, args):
        for b in (self.one, self.three, self.four):
            assert self.lib.asm_batch_setup(b, *args) == 0, self.lib.asm_batch_last_error(b)


@pytest.fixture(scope="module")
def batches(hip_lib):
    B = Batches(hip_lib)
    yield B
    for b in (B.one, B.three, B.four):
        hip_lib.asm_batch_destroy(b)
    print("\n" + "\n".join(merged.coverage_report()))


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = C.c_void_p()
    assert hip_lib.asm_create(0, C.byref(h)) == 0
    yield h
    hip_lib.asm_destroy(h)


def names(tab):
    return set(r[0] for r in tab)


def show(tag, tab):
    print("\n%s: %d kernels" % (tag, len(tab)))
    for name, ops, launches, nb, gz in tab:
        print("    %-40s operations %4d launches %4d nb_max %d gz %d" % (merged.short(name)[:40], ops, launches, nb, gz))


def constellations(lib, B, tag, same, other, two_groups=False):
    """same: five scenarios of one shape and stage list (calls made on the plain handle, tests.merged.Scenario); other: one that leaves the
    common path.  Returns the table of constellation 1."""
    # What a slot solved before decides how many buffers its next set-up frees and makes (each free is a round of its own), so slots with
    # different histories drift apart by a few rounds.  One pass of the same scenarios first gives every slot the same history
    run_batch(lib, B.three, same[:3], tag + " (first pass)")
    run_batch(lib, B.one, same[:1], tag + " (first pass, one slot)")
    # 1: three of a kind
    tab = run_batch(lib, B.three, same[:3], tag + " (1)")
    show(tag + " (1) three scenarios on three slots", tab)
    assert tab, "%s: the batch recorded no kernel" % tag
    for name, ops, launches, nb, gz in tab:
        assert ops == 3 * launches and nb == 3, (tag, merged.short(name), ops, launches, nb, gz)
    one = run_batch(lib, B.one, same[:1], tag + " (one slot)")
    assert names(one) == names(tab), (tag, sorted(merged.short(k) for k in names(one) ^ names(tab)))
    assert all(nb == 1 for _, _, _, nb, _ in one)
    merged.note_merged(tab)
    # 2: five on three
    tab2 = run_batch(lib, B.three, same, tag + " (2)")
    assert names(tab2) == names(tab) and max(r[3] for r in tab2) == 3 and sum(r[1] for r in tab2) == 5 * sum(r[1] for r in one)
    assert any(launches > ops // 3 for _, ops, launches, _, _ in tab2), "no second pass"
    # 3: the middle scenario leaves the common path
    tab3 = run_batch(lib, B.three, [same[0], other, same[1]], tag + " (3)")
    show(tag + " (3) one scenario of another kind", tab3)
    assert any(nb == 2 for _, _, _, nb, _ in tab3), "%s: no launch merged two scenarios" % tag
    assert any(nb == 1 or (nb == 2 and ops < 2 * launches) for _, ops, launches, nb, _ in tab3), "%s: no launch went out alone" % tag
    merged.note_merged(tab3)
    # 4: two groups
    if two_groups:
        run_batch(lib, B.four, same[:4], tag + " (first pass, two groups)")
        tab4 = run_batch(lib, B.four, same[:4], tag + " (4)")
        assert names(tab4) == names(tab)
        for name, ops, launches, nb, gz in tab4:
            assert ops == 2 * launches and nb == 2, (tag, merged.short(name), ops, launches, nb, gz)
    return tab


# ------------------------------------------------------------------------------------------------------------------ the dense kernel hooks
def spd(N, seed):
    rng = np.random.default_rng(seed)
    Bm = rng.standard_normal((N, N + 5))
    return Bm @ Bm.T + 0.1 * np.eye(N), rng


# The main factor buffers of a handle take 512-wide blocks up to N = 1536 (1024-wide above).  A factor of ONE wide block (N <= 512) gets its
# explicit inverse inside the panel launch (Dev::chol: panel_inv, its grid of at most 72 workgroups fits every share), and band_panels_ok
# is false for a dense matrix, so N = 513 is the smallest order at which Dev::chol ends in trtri_launches<512>: two wide blocks, the levels
# hh = 1, 2, 4 with gridDim.z = hh * hh = 1, 4, 16.  Its only resident launch is k_chol_panel_solo with 9 workgroups (one per 64-row tile):
# three scenarios make 27, inside the group's share (480 on an MI355X; read from the batch), so the merge is not split.
N_TRTRI = 513


def chol_call(cap, h, N, seed):
    S, _ = spd(N, seed)
    L = np.full((N, N), util.SENTINEL)
    assert cap.asm_test_cholesky(h, _d(S), N, _d(L)) == 0, cap.asm_last_error(h)
    return cap.last()


def chol_solve_call(cap, h, N, seed):
    S, rng = spd(N, seed)
    b, x = rng.standard_normal(N), np.full(N, util.SENTINEL)
    assert cap.asm_test_chol_solve(h, _d(S), N, _d(b), _d(x)) == 0, cap.asm_last_error(h)
    return cap.last()


@pytest.mark.parametrize("call", [chol_call, chol_solve_call], ids=["cholesky", "chol_solve"])
def test_cholesky_with_trtri_levels_in_grid_z(hip_lib, handle, batches, call):
    cap = Capture(hip_lib)
    same = [call(cap, handle, N_TRTRI, 10 + s) for s in range(5)]
    other = call(cap, handle, N_TRTRI + 64, 20)          # one more row tile: other grids
    tab = constellations(hip_lib, batches, call.__name__, same, other)
    levels = {gz: (ops, launches, nb) for name, ops, launches, nb, gz in tab if "k_trtri_level" in name}
    assert levels == {1: (6, 2, 3), 4: (6, 2, 3), 16: (6, 2, 3)}, levels          # two launches per level, each for all three scenarios
    assert all("512" in name for name, _, _, _, gz in tab if "k_trtri_level" in name)
    assert any("k_chol_panel_solo" in name for name in names(tab))
    st = _lib.BatchStats()
    assert hip_lib.asm_batch_get_stats(batches.three, C.byref(st)) == 0
    share = hip_lib.asm_test_batch_panel_share(batches.three, 0)          # what the library gave the batch's only group
    assert share >= 27 and hip_lib.asm_test_batch_panel_share(batches.three, 1) == -1
    assert 27 <= st.panel_grid_max <= share, (st.panel_grid_max, share)


def gemm_call(cap, h, Ma, Mb, K, mode, seed):
    rng = np.random.default_rng(seed)
    A, Bm, C0 = rng.standard_normal((Ma, K)), rng.standard_normal((Mb, K)), rng.standard_normal((Ma, Mb))
    out = np.full((Ma, Mb), util.SENTINEL)
    assert cap.asm_test_gemm_nt(h, _d(A), _d(Bm), _d(C0), Ma, Mb, K, mode, _d(out)) == 0, cap.asm_last_error(h)
    return cap.last()


def gemv_call(cap, h, M, K, seed):
    rng = np.random.default_rng(seed)
    A, x, y = rng.standard_normal((M, K)), rng.standard_normal(K), rng.standard_normal(M)
    Ax, ATy = np.full(M, util.SENTINEL), np.full(K, util.SENTINEL)
    assert cap.asm_test_gemv(h, _d(A), M, K, _d(x), _d(y), _d(Ax), _d(ATy)) == 0, cap.asm_last_error(h)
    return cap.last()


def trsm_call(cap, h, N, nrhs, backward, seed):
    S, rng = spd(N, seed)
    R, X = rng.standard_normal((nrhs, N)), np.full((nrhs, N), util.SENTINEL)
    assert cap.asm_test_trsm_rows(h, _d(S), N, _d(R), nrhs, backward, _d(X)) == 0, cap.asm_last_error(h)
    return cap.last()


def syrk_call(cap, h, M, K, Ms, tile, seed):
    rng = np.random.default_rng(seed)
    A, theta = rng.standard_normal((M, K)), rng.uniform(0.0, 2.0, K)
    theta[rng.random(K) < 0.2] = 0.0
    idx, diag = np.sort(rng.choice(M, Ms, replace=False)).astype(np.int32), rng.uniform(0.0, 1.0, Ms)
    S = np.full((Ms, Ms), util.SENTINEL)
    assert cap.asm_test_syrk(h, _d(A), M, K, _lib.i32ptr(idx), Ms, _d(theta), _d(diag), _d(S), tile) == 0, cap.asm_last_error(h)
    return cap.last()


def syrk_update_call(cap, h, Ms, K, MsB, srow0, tile, seed):
    rng = np.random.default_rng(seed)
    P, S = rng.standard_normal((Ms, K)), rng.standard_normal((Ms, Ms))
    assert cap.asm_test_syrk_update(h, _d(P), Ms, K, MsB, srow0, _d(S), tile) == 0, cap.asm_last_error(h)
    return cap.last()


def build_split_call(cap, h, k, K, nsplit, seed):
    G, theta = util.split_operand(seed, k, K)
    ld = (k + 31) // 32 * 32
    parts, S, N0, d0 = (np.full(shape, util.SENTINEL) for shape in ((nsplit, ld, ld), (ld, ld), (ld, ld), (ld,)))
    assert cap.asm_test_build_split(h, _d(G), k, K, _d(theta), nsplit, 1e-10, 1e-14, _d(parts), _d(S), _d(N0), _d(d0)) == 0, cap.asm_last_error(h)
    return cap.last()


DENSE = {      # hook -> (the call, arguments of the five scenarios, arguments of the one that leaves the common path)
    "gemm_nt": (gemm_call, (130, 200, 96, 1), (64, 200, 96, 1)),
    "gemv": (gemv_call, (130, 77), (200, 77)),
    "trsm_rows": (trsm_call, (700, 37, 1), (600, 37, 1)),
    "syrk": (syrk_call, (200, 333, 200, 2), (100, 70, 37, 1)),
    "syrk_update": (syrk_update_call, (300, 64, -1, 0, 1), (300, 64, 130, 64, 1)),
    "syrk_update_tile4": (syrk_update_call, (300, 128, -1, 64, 4), (300, 128, 130, 0, 4)),
    "build_split": (build_split_call, (137, 288, 3), (137, 288, 1)),
}


@pytest.mark.parametrize("hook", list(DENSE))
def test_dense_kernel_hooks(hip_lib, handle, batches, hook):
    call, args, odd = DENSE[hook]
    cap = Capture(hip_lib)
    same = [call(cap, handle, *args, 30 + s) for s in range(5)]
    constellations(hip_lib, batches, hook, same, call(cap, handle, *odd, 40))


# ------------------------------------------------------------------------------------------------------------------ the stage hooks
def test_ipm_stages(hip_lib, handle, batches):
    from tests.test_ipm_stages_gpu import Run, stage
    case = min((c for c in util.IPM_CASES if util.ipm_red_grid(*c) > 1), key=lambda c: max(c))      # reductions of several workgroups: arrival counters
    cap = Capture(hip_lib)

    def state(seed):
        st = util.ipm_state(seed, *case, mu=1e-2)
        rng = np.random.default_rng(900 + seed)
        st["sres"] = 0.5 * st["pcg"] + 0.2 * rng.standard_normal(st["M"])
        st["corr"] = 0.5 * st["res"] + 0.2 * rng.standard_normal(st["M"])
        st["scal"][util.SC["RZ"]], st["scal"][util.SC["RZ0"]] = 0.7, 2.1
        return st
    seq = [stage("measures", pub=0), stage("steps", D="A", pub=0), stage("muaff", D="A", sexp=3), stage("steps", D="C", pub=0), stage("pcg_step1", D="A", pub=5)]
    same = []
    for s in range(5):
        Run(cap, handle, state(600 + s), seq)
        same.append(cap.last())
    Run(cap, handle, state(650), [seq[0], seq[1], seq[3], seq[2], seq[4]])          # steps C before muaff
    constellations(hip_lib, batches, "ipm_stages n%d M%d ns%d" % case, same, cap.last())


def test_as_stages(hip_lib, handle, batches):
    from tests.test_as_stages_gpu import Run, stage
    case = (256, 256, 257)          # two workgroups over each of the three ranges
    assert case in util.AS_CASES and util.as_grid_all(*case) > 1
    cap = Capture(hip_lib)
    seq = [stage("identify", set=[3]), stage("sl"), stage("sl_values"), stage("rhs", x=[-1]), stage("add_f"), stage("rd"), stage("merge", with_y=1)]
    same = []
    for s in range(5):
        Run(cap, handle, util.as_state(700 + s, *case), seq)
        same.append(cap.last())
    Run(cap, handle, util.as_state(750, *case), seq[:2] + seq[4:])
    constellations(hip_lib, batches, "as_stages n%d M%d ns%d" % case, same, cap.last())


def test_ns_stages(hip_lib, handle, batches):
    from tests.test_ns_stages_gpu import CASES, Run, stage
    case = (257, 257, 64, 100)
    assert case in CASES
    cap = Capture(hip_lib)
    seq = [stage("theta", rho_p=util.IPM_RHO_P), stage("e1"), stage("wm_neg"), stage("kx")]
    same = []
    for s in range(5):
        Run(cap, handle, util.ns_state(800 + s, *case), seq)
        same.append(cap.last())
    Run(cap, handle, util.ns_state(850, *case), [seq[0], seq[1], seq[3], seq[2]])          # kx before wm_neg
    constellations(hip_lib, batches, "ns_stages n%d M%d k%d nI%d" % case, same, cap.last())


def test_kkt_stages(hip_lib, handle, batches):
    from tests.test_kkt_stages_cpu import base_state, fill, freeze
    from tests.test_kkt_stages_gpu import Call
    cap = Capture(hip_lib)

    def one(seed, specs):
        st, rng = base_state(257, 4, 0, 1, 3, seed)
        fill(st, rng, ["r", "p", "hp", "d", "b_ru", "hraw"])
        freeze(st, rng)
        call = Call(cap, handle, st)
        call.run([call.stage(kind, **kw) for kind, kw in specs])
        return cap.last()
    specs = [("cg_p", dict(x=["r", "p"])), ("cg_step", dict(x=["p", "hp", "d", "r"])), ("axpby", dict(x=["b_ru", "hraw", "r"], s=[1.5, -0.75], flag=[1, 0, 0]))]
    same = [one(60 + s, specs) for s in range(5)]
    constellations(hip_lib, batches, "kkt_stages n257 cols3", same, one(70, [specs[0], specs[2], specs[1]]), two_groups=True)


@pytest.mark.parametrize("name", ["general-130x70", "sparse-300x70"])
def test_skeleton_stages(hip_lib, batches, name):
    from tests import skeleton_twins as T
    from tests.test_skeleton_stages_gpu import _handle_for, _info, _stages
    cap = Capture(hip_lib)
    case = T.get_case(name)
    h = _handle_for(cap, case)
    try:
        batches.setup(cap.setup)
        info = _info(hip_lib, h)

        def one(seed, stages):
            dE, lb, ub = T.case_values(case, "normal", seed=seed)
            _stages(cap, h, info, stages, dE, lb, ub, None, case["x"], case["y"])
            return cap.last()
        same = [one(90 + s, T.ALL) for s in range(5)]
        constellations(hip_lib, batches, "skeleton_stages " + name, same, one(95, T.ALL & ~T.PRODUCTS), two_groups=True)
    finally:
        hip_lib.asm_destroy(h)


def test_ns_setup_stages(hip_lib, batches):
    from tests.test_ns_setup_gpu import Case, rand_rows
    cap = Capture(hip_lib)
    c = Case(cap, "dense")
    try:
        batches.setup(cap.setup)

        def one(seed, stages):
            c.run(stages, G=rand_rows(c, seed))
            return cap.last()
        same = [one(110 + s, ["rows_e", "gi", "gram"]) for s in range(5)]
        constellations(hip_lib, batches, "ns_setup_stages dense", same, one(120, ["rows_e", "gram", "gi"]))
    finally:
        c.close()
