"""Kernel-level checks of libasmhip against NumPy (float64), through the C ABI test hooks."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = C.c_void_p()
    assert hip_lib.asm_create(0, C.byref(h)) == 0
    yield h
    hip_lib.asm_destroy(h)


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.mark.parametrize("M,K,Ms,tile", [(40, 50, 40, 1), (100, 70, 37, 1), (200, 333, 200, 2), (300, 129, 211, 4),
                                           (500, 1000, 500, 0), (130, 64, 130, 4)])
def test_syrk_matches_numpy(hip_lib, handle, M, K, Ms, tile):
    rng = np.random.default_rng(M * 7 + K)
    A = rng.standard_normal((M, K))
    theta = rng.uniform(0.0, 2.0, K)
    theta[rng.random(K) < 0.2] = 0.0
    idx = np.sort(rng.choice(M, Ms, replace=False)).astype(np.int32)
    diag = rng.uniform(0.0, 1.0, Ms)
    S = np.zeros((Ms, Ms))
    rc = hip_lib.asm_test_syrk(handle, _d(A), M, K, idx.ctypes.data_as(C.POINTER(C.c_int32)), Ms, _d(theta), _d(diag), _d(S), tile)
    assert rc == 0, hip_lib.asm_last_error(handle)
    ref = (A[idx] * theta) @ A[idx].T + np.diag(diag)
    err = np.abs(np.tril(S) - np.tril(ref)).max() / np.abs(ref).max()
    assert err < 1e-13          # f64 MFMA accumulation, K <= 1000


@pytest.mark.parametrize("Ms,K,MsB,srow0,tile", [
    (3100, 1024, -1, 0, 4),        # triangular trailing update, rows not a multiple of the 128-tile: k_syrk_upd, XCD-aware tile order
    (4001, 256, -1, 64, 4),        # odd size, offset origin
    (3333, 256, 768, 128, 4),      # rectangular in-panel update: all rows x the first 768 columns
    (3200, 64, 130, 0, 4),         # shortest k (two ring stages of the update kernel never fill), ragged column count
    (1000, 256, -1, 0, 2), (1000, 256, 300, 64, 2), (300, 64, -1, 0, 1),      # the generic kernel on the small sizes
])
def test_cholesky_update_matches_numpy(hip_lib, handle, Ms, K, MsB, srow0, tile):
    """S -= P P' on the lower triangle (columns < MsB), as the factorisation launches it."""
    rng = np.random.default_rng(Ms + K)
    P = rng.standard_normal((Ms, K))
    S0 = rng.standard_normal((Ms, Ms))
    S = S0.copy()
    rc = hip_lib.asm_test_syrk_update(handle, _d(P), Ms, K, MsB, srow0, _d(S), tile)
    assert rc == 0, hip_lib.asm_last_error(handle)
    ref = S0 - P @ P.T
    mask = np.tril(np.ones((Ms, Ms), bool))
    if MsB >= 0:
        mask[:, MsB:] = False
    scale = np.abs(ref).max()
    assert np.abs(S - ref)[mask].max() / scale < 1e-13
    assert np.array_equal(S[~mask], S0[~mask])          # nothing outside the updated region is touched


@pytest.mark.parametrize("N", [1, 17, 64, 65, 200, 513, 519, 530, 1000, 2500, 4700])      # (519: the thin ninth row tile of the C4 reduced matrix; 530: 18 live rows, padded sub-blocks only)
def test_cholesky_and_solve(hip_lib, handle, N):
    rng = np.random.default_rng(N)
    B = rng.standard_normal((N, N + 5))
    S = B @ B.T + 0.1 * np.eye(N)
    L = np.zeros((N, N))
    assert hip_lib.asm_test_cholesky(handle, _d(S), N, _d(L)) == 0, hip_lib.asm_last_error(handle)
    Lref = np.linalg.cholesky(S)
    assert np.abs(L - Lref).max() / np.abs(Lref).max() < 1e-11
    b = rng.standard_normal(N)
    x = np.zeros(N)
    assert hip_lib.asm_test_chol_solve(handle, _d(S), N, _d(b), _d(x)) == 0
    xref = np.linalg.solve(S, b)
    assert np.abs(x - xref).max() / np.abs(xref).max() < 1e-9
    assert np.abs(S @ x - b).max() < 1e-10 * max(1.0, np.abs(S).max() * np.abs(x).max())


def test_cholesky_pivot_guard(hip_lib, handle):
    """A duplicated row makes S singular: the static guard drops it instead of producing NaNs."""
    rng = np.random.default_rng(3)
    B = rng.standard_normal((30, 50))
    B[7] = B[3]
    S = B @ B.T
    L = np.zeros((30, 30))
    assert hip_lib.asm_test_cholesky(handle, _d(S), 30, _d(L)) == 0
    assert np.isfinite(L).all()
    assert L[7, 7] > 1e100


@pytest.mark.parametrize("M,K", [(5, 3), (130, 77), (500, 1000), (1000, 129)])
def test_gemv(hip_lib, handle, M, K):
    """A x by k_gemv_n and A'y on a dense Ah loaded into a test skeleton.  A'y reaches the transposed-copy route of launch_gemv_t only
    (k_transpose_dense + k_gemv_n_exact); the CSC and the two-stage routes are in tests/test_skeleton_stages_gpu.py.  A sum of L products in
    any order, with or without FMA, is within (L + 2) eps sum |a| |x| of the exact value: L = ldn along a row, M along a column."""
    rng = np.random.default_rng(M + K)
    A = rng.standard_normal((M, K)); x = rng.standard_normal(K); y = rng.standard_normal(M)
    Ax = np.zeros(M); ATy = np.zeros(K)
    assert hip_lib.asm_test_gemv(handle, _d(A), M, K, _d(x), _d(y), _d(Ax), _d(ATy)) == 0
    LD, eps, ldn = np.longdouble, np.longdouble(2.0 ** -52), (K + 31) // 32 * 32
    Al, xl, yl = A.astype(LD), x.astype(LD), y.astype(LD)
    assert (np.abs(Ax - Al @ xl) <= (ldn + 2) * eps * (np.abs(Al) @ np.abs(xl))).all()
    assert (np.abs(ATy - Al.T @ yl) <= (M + 2) * eps * (np.abs(Al).T @ np.abs(yl))).all()


@pytest.mark.parametrize("seed,n,m,density,dup,nrange", [(1, 7, 5, 0.5, 0.5, 2), (2, 60, 40, 0.1, 0.3, 5), (3, 50, 30, 1.0, 0.0, 0),
                                                         (4, 33, 21, 0.3, 1.0, 3)])
def test_assembly_bit_exact(hip_lib, seed, n, m, density, dup, nrange):
    """Duplicate accumulation in j_str order is bitwise identical to the oracle's restatement of
    common.jl:12-20, including the stale-entry rule of the extra range rows (subproblem.jl:448-457)."""
    from tests.util import random_subproblem
    from activesetmethods_amd.subproblem import QpData, HipSubOptimizer
    from oracle.subproblem import QpData as OQpData, QpModel, compute_jacobian_matrix
    sp = random_subproblem(seed, n, m, density, dup, nrange)
    opt = HipSubOptimizer(QpData(sp['df'], sp['f'], sp['dE'], sp['E'], sp['c_lb'], sp['c_ub'], sp['v_lb'], sp['v_ub']),
                          sp['j_row'], sp['j_col'])
    qp = None
    rng = np.random.default_rng(seed + 100)
    for call in range(3):
        dE = sp['dE'].copy()
        if call == 1:
            dE[rng.random(len(dE)) < 0.4] = 0.0          # entries vanish: stale coefficients must persist
        if call == 2:
            dE = rng.standard_normal(len(dE))
        A, stored = compute_jacobian_matrix(m, n, sp['j_row'] - 1, sp['j_col'] - 1, dE)
        data = OQpData(sp['df'], sp['f'], A, sp['E'], sp['c_lb'], sp['c_ub'], sp['v_lb'], sp['v_ub'], stored)
        if qp is None:
            qp = QpModel(data, sp['j_row'], sp['j_col'])
        qp.data = data
        lp = qp.build_lp(sp['x_k'], 0.4, False)
        M = m + len(qp.adj)
        Jg = np.zeros((M, n))
        assert hip_lib.asm_test_assemble(opt._h, _d(np.ascontiguousarray(dE)), _d(Jg)) == 0
        assert np.array_equal(Jg, lp.A)
    opt.close()


def test_mfma_f64_probe_runs(hip_lib, handle):
    """The FP64 matrix-core probe used for the roofline discussion (profiles/r01_mfma_f64_probe.txt)."""
    t = C.c_double(0.0)
    assert hip_lib.asm_test_mfma_peak(handle, 20000, 2, C.byref(t)) == 0
    assert 5.0 < t.value < 200.0


# ----------------------------------------------------------------------------- round 3: kernels of the null-space form
@pytest.mark.parametrize("Ma,Mb,K,mode", [(64, 64, 32, 0), (130, 200, 96, 0), (130, 200, 96, 1), (519, 1024, 1024, 1), (37, 469, 480, 0)])
def test_gemm_nt_matches_numpy(hip_lib, handle, Ma, Mb, K, mode, monkeypatch):
    """C = (C0) -/+ A B' on the matrix cores (k_gemm_nt and its 32 x 64 / 32 x 96 tile variants): ragged tile edges, both modes, in-place
    accumulation; the variants give the same bits (every entry is the same sum in the same order)."""
    rng = np.random.default_rng(Ma + Mb + K)
    A = rng.standard_normal((Ma, K)); B = rng.standard_normal((Mb, K)); C0 = rng.standard_normal((Ma, Mb))
    ref = A @ B.T if mode == 0 else C0 - A @ B.T
    outs = []
    for variant in ("64", "32", "32w"):
        monkeypatch.setenv("ASM_TEST_GEMM", variant)
        Cout = np.zeros((Ma, Mb))
        rc = hip_lib.asm_test_gemm_nt(handle, _d(A), _d(B), _d(C0), Ma, Mb, K, mode, _d(Cout))
        assert rc == 0, hip_lib.asm_last_error(handle)
        assert np.abs(Cout - ref).max() / np.abs(ref).max() < 1e-13, variant
        outs.append(Cout)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


@pytest.mark.parametrize("N,nrhs,backward", [(100, 5, 1), (700, 37, 0), (700, 37, 1), (1500, 64, 1), (2600, 130, 1), (981, 107, 1), (3000, 520, 1)])      # (the last: 32 x 96 tiles, k_gemm_nt32w)
def test_multi_rhs_triangular_solves(hip_lib, handle, N, nrhs, backward):
    """Rows of R solved against the Cholesky factor by right-looking block substitution (products with the explicit inverses of
    the wide diagonal blocks + one update of all remaining columns per block): forward only and forward + backward."""
    from scipy.linalg import solve_triangular
    rng = np.random.default_rng(N + nrhs)
    Bm = rng.standard_normal((N, N + 5))
    S = Bm @ Bm.T + 0.1 * np.eye(N)
    R = rng.standard_normal((nrhs, N))
    X = np.zeros((nrhs, N))
    rc = hip_lib.asm_test_trsm_rows(handle, _d(S), N, _d(R), nrhs, backward, _d(X))
    assert rc == 0, hip_lib.asm_last_error(handle)
    L = np.linalg.cholesky(S)
    ref = solve_triangular(L, R.T, lower=True).T
    if backward:
        ref = solve_triangular(L.T, ref.T, lower=False).T
    assert np.abs(X - ref).max() / np.abs(ref).max() < 1e-9
    if backward:
        assert np.abs(X @ S - R).max() < 1e-9 * max(1.0, np.abs(S).max() * np.abs(X).max())


@pytest.mark.parametrize("N", [11192, 18637])
def test_cholesky_and_solve_at_case1354_sizes(hip_lib, handle, N):
    """The three-level blocked factorisation with look-ahead at the sizes the case1354pegase-sized LPs factor (n = 11192, M = 18637):
    ||L (L'v) - S v|| / (||S|| ||v||) <= 1e-12 for several v, the solve's residual, and at N = 11192 the factor against LAPACK."""
    rng = np.random.default_rng(N)
    Bm = rng.standard_normal((N, 96))
    S = Bm @ Bm.T
    S[np.arange(N), np.arange(N)] += rng.uniform(1.0, 3.0, N) * 96.0
    L = np.zeros((N, N))
    assert hip_lib.asm_test_cholesky(handle, _d(S), N, _d(L)) == 0, hip_lib.asm_last_error(handle)
    assert np.isfinite(L).all() and (np.diag(L) > 0).all() and (np.diag(L) < 1e100).all()
    nS = np.abs(S).sum(axis=1).max()
    for t in range(4):
        v = rng.standard_normal(N) if t else np.ones(N)
        r = L @ (L.T @ v) - S @ v
        assert np.abs(r).max() <= 1e-12 * nS * np.abs(v).max(), (t, np.abs(r).max() / (nS * np.abs(v).max()))
    if N <= 12000:
        Lref = np.linalg.cholesky(S)
        assert np.abs(L - Lref).max() / np.abs(Lref).max() < 1e-11
    del L
    b = rng.standard_normal(N)
    x = np.zeros(N)
    assert hip_lib.asm_test_chol_solve(handle, _d(S), N, _d(b), _d(x)) == 0, hip_lib.asm_last_error(handle)
    assert np.abs(S @ x - b).max() <= 1e-11 * max(1.0, nS * np.abs(x).max())


def test_panel_wait_timeout_is_reported_once_and_the_handle_survives(hip_lib, handle):
    """The dataflow panel kernel's bounded wait with a producer that never publishes: every waiting workgroup gives up (the first after
    the full bound, the others at their next look at the timeout word), the host reports ASM_ERR_HIP with the kernel's message once,
    and the same handle factors correctly afterwards."""
    import time
    t0 = time.time()
    rc = hip_lib.asm_test_panel_timeout(handle, 8)
    dt = time.time() - t0
    assert rc == -2, rc                                         # ASM_ERR_HIP
    assert b"timed out" in hip_lib.asm_last_error(handle)
    assert dt < 60.0
    N = 300
    rng = np.random.default_rng(5)
    Bm = rng.standard_normal((N, N + 5))
    S = Bm @ Bm.T + 0.1 * np.eye(N)
    L = np.zeros((N, N))
    assert hip_lib.asm_test_cholesky(handle, _d(S), N, _d(L)) == 0, hip_lib.asm_last_error(handle)      # no stale timeout
    assert np.abs(L - np.linalg.cholesky(S)).max() < 1e-10


@pytest.mark.parametrize("N,band,nrhs", [(700, 90, 33), (2300, 267, 70), (3100, 1398, 130), (5000, 150, 40), (2245, 40, 137)])
def test_banded_cholesky_and_solves(hip_lib, handle, N, band, nrhs):
    """A banded SPD matrix (the S0 = A_EF A_EF' of the null-space form in reverse Cuthill-McKee order): with the band declared, the
    factorisation, the single right-hand-side solve and the multi right-hand-side block substitution stop at the band - same factor
    and solutions as the dense NumPy reference."""
    from scipy.linalg import solve_triangular
    rng = np.random.default_rng(N + band)
    Bm = np.zeros((N, N))
    for d in range(0, band // 2 + 1):                 # B has half-bandwidth band // 2 -> B B' has half-bandwidth <= band
        v = rng.standard_normal(N - d)
        Bm[np.arange(d, N), np.arange(0, N - d)] = v
    S = Bm @ Bm.T + 0.5 * np.eye(N)
    i, j = np.nonzero(S)
    assert np.abs(i - j).max() <= band
    assert hip_lib.asm_test_set_band(handle, band) == 0
    try:
        L = np.zeros((N, N))
        assert hip_lib.asm_test_cholesky(handle, _d(S), N, _d(L)) == 0, hip_lib.asm_last_error(handle)
        Lref = np.linalg.cholesky(S)
        assert np.abs(L - Lref).max() / np.abs(Lref).max() < 1e-11
        b = rng.standard_normal(N)
        x = np.zeros(N)
        assert hip_lib.asm_test_chol_solve(handle, _d(S), N, _d(b), _d(x)) == 0
        assert np.abs(S @ x - b).max() < 1e-10 * max(1.0, np.abs(S).max() * np.abs(x).max())
        R = rng.standard_normal((nrhs, N))
        for backward in (0, 1):
            X = np.zeros((nrhs, N))
            assert hip_lib.asm_test_trsm_rows(handle, _d(S), N, _d(R), nrhs, backward, _d(X)) == 0, hip_lib.asm_last_error(handle)
            ref = solve_triangular(Lref, R.T, lower=True).T
            if backward:
                ref = solve_triangular(Lref.T, ref.T, lower=False).T
            assert np.abs(X - ref).max() / np.abs(ref).max() < 1e-9
    finally:
        assert hip_lib.asm_test_set_band(handle, 0) == 0


# ----------------------------------------------------------------------------- the Cholesky family in every launch configuration
# Handles whose per-handle knobs (asm_create reads them) select the other launch sequences of Dev::chol / chol_chain (asm_hip.hip):
#   D     the default (panel_wgs = 2 #CU - 32 = 480 on an MI355X: one workgroup per row tile, G = nrt)
#   W1/5/16  ASM_PANEL_WGS: G = min(nrt, panel_wgs) < nrt, each workgroup owns row tiles rt, rt + G, ...; no k_chol_panel_band (the generic banded
#            chain: k_chol_panel + rowlim + banded rank-K updates) and no k_chol_panel_inv (k_trtri_* instead)
#   W175  the budget just below the old worst-case gate of the in-launch inverse (ASM_PNL_WT (ASM_PNL_NS + 1) = 176); the gate is the launch's
#         own grid (at most 144 for a factor of one 1024-wide block), so W175 takes D's sequence
CONFIGS = {"D": {}, "W1": {"ASM_PANEL_WGS": "1"}, "W5": {"ASM_PANEL_WGS": "5"}, "W16": {"ASM_PANEL_WGS": "16"},
           "W175": {"ASM_PANEL_WGS": "175"}}
PANEL_WGS_D = 480
U64 = 2.0 ** -53
# condition-free backward-error bars (u = 2^-53); largest ratios measured on an MI355X over every shape and configuration: 2.12 (factor,
# N = 1), 1.43 (solves); the printed "ratio" lines of the tests (pytest -s) give them per case
C_FAC = 4.0        # factor: ||S v - L (L' v)||_inf <= C_FAC N u ||S||_inf ||v||_inf
C_SOL = 4.0        # solves: ||S x - b||_inf <= C_SOL N u (||S||_inf ||x||_inf + ||b||_inf), the same for the rows of the triangular solves


@pytest.fixture(scope="module")
def config_handle(hip_lib):
    """config_handle(name): a handle created under the configuration's environment (made on first use, destroyed with the module)."""
    made = {}

    def get(name):
        if name not in made:
            with pytest.MonkeyPatch.context() as mp:
                mp.delenv("ASM_PANEL_WGS", raising=False)
                for k, v in CONFIGS[name].items():
                    mp.setenv(k, v)
                h = C.c_void_p()
                assert hip_lib.asm_create(0, C.byref(h)) == 0
            made[name] = h
        return made[name]
    yield get
    for h in made.values():
        hip_lib.asm_destroy(h)


def _wide_block(layout, N, band_hint):
    """The wide-block width the factor's substitutions use: main buffers h->wb (pitch Mp >= N), a factor buffer ns_alloc_factor's rule."""
    if layout == 0:
        return 1024 if N > 1536 else 512
    ld = -(-N // 32) * 32
    wb = 1024 if (ld <= 1024 or ld > 1536) else 512
    return 512 if (band_hint > 0 and band_hint <= 512 and ld > 1024) else wb


def kernel_selection(config, layout, N, band=0, band_hint=0):
    """The launch sequence Dev::chol chooses for this configuration (band_panels_ok, the gate of the in-launch inverse panel_inv_grid),
    everything but the grid G = min(nrt, panel_wgs) of the panel launches.  Configurations with the same selection give the same factor,
    inverses and solutions BIT FOR BIT: a row tile's sums are made in the same order by whichever workgroup owns it (chol_panel_body), the
    helpers of k_chol_panel_inv and the k_trtri_* / substitution launches do not depend on G."""
    env = CONFIGS[config]
    pw = int(env.get("ASM_PANEL_WGS", PANEL_WGS_D))
    nb, nbi = 64, 512
    if band > 0 and N > nbi + 2 * nb:
        nrt = (nbi + 2 * nb + -(-band // 64) * 64 + nb - 1) // nb + 1
        m = nrt - nbi // nb
        if nrt <= 40 and nrt + m * (m + 1) // 2 <= pw:
            return ("band",)
    inv = False
    if band == 0 and N <= _wide_block(layout, N, band_hint):
        T, grid, I0 = -(-N // nb), 0, 0
        while I0 < N:
            I1 = N if N - I0 <= nbi + 2 * nb else min(I0 + nbi, N)
            grid = max(grid, max(1, min(-(-(N - I0) // nb), pw)) + (-(-(I1 - I0) // nb)) * T)
            I0 = I1
        inv = grid <= pw
    return ("panel", inv)


def _ld(a):
    return np.asarray(a, np.longdouble)


def _spd(N, band, seed):
    rng = np.random.default_rng(seed)
    if band:
        Bm = np.zeros((N, N))
        for d in range(0, band // 2 + 1):
            Bm[np.arange(d, N), np.arange(0, N - d)] = rng.standard_normal(N - d)
        return Bm @ Bm.T + 0.5 * np.eye(N), rng
    Bm = rng.standard_normal((N, N + 5))
    return Bm @ Bm.T + 0.1 * np.eye(N), rng


def _run_hooks(hip_lib, h, S, b, R, setting, layout, band, band_hint, wf, wb_):
    """L, x = S^-1 b, rows of R forward-solved (first wf) and fully solved (first wb_) through the hooks with the given factor settings."""
    N = S.shape[0]
    mode, rel, absv, thr = setting
    assert hip_lib.asm_test_set_band(h, band) == 0
    assert hip_lib.asm_test_set_factor(h, layout, band_hint, mode, rel, absv, thr) == 0
    try:
        L = np.zeros((N, N))
        assert hip_lib.asm_test_cholesky(h, _d(S), N, _d(L)) == 0, hip_lib.asm_last_error(h)
        x = np.zeros(N)
        assert hip_lib.asm_test_chol_solve(h, _d(S), N, _d(b), _d(x)) == 0, hip_lib.asm_last_error(h)
        Xf = np.zeros((wf, N)); Xb = np.zeros((wb_, N))
        assert hip_lib.asm_test_trsm_rows(h, _d(S), N, _d(np.ascontiguousarray(R[:wf])), wf, 0, _d(Xf)) == 0, hip_lib.asm_last_error(h)
        assert hip_lib.asm_test_trsm_rows(h, _d(S), N, _d(np.ascontiguousarray(R[:wb_])), wb_, 1, _d(Xb)) == 0, hip_lib.asm_last_error(h)
    finally:
        assert hip_lib.asm_test_set_factor(h, 0, 0, 0, 0.0, 0.0, 1e-14) == 0
        assert hip_lib.asm_test_set_band(h, 0) == 0
    return L, x, Xf, Xb


RATIOS = {}


def _check_bounds(tag, S, Sl, nS, L, x, b, Xf, Xb, R, Sv, V):
    """Condition-free backward errors in long double: the factor on probe vectors, the solve, the forward rows (L x' = r') and the full rows."""
    N = S.shape[0]
    Ll = _ld(L)
    fac = np.abs(Sv - Ll @ (Ll.T @ V)).max(axis=0) / (N * U64 * nS * np.abs(V).max(axis=0))
    sol = np.abs(Sl @ _ld(x) - _ld(b)).max() / (N * U64 * (nS * np.abs(x).max() + np.abs(b).max()))
    nL = np.abs(L).sum(axis=1).max()
    fwd = (np.abs(_ld(Xf) @ Ll.T - _ld(R[:len(Xf)])).max(axis=1) / (N * U64 * (nL * np.abs(Xf).max(axis=1) + np.abs(R[:len(Xf)]).max(axis=1)))).max()
    bwd = (np.abs(_ld(Xb) @ Sl - _ld(R[:len(Xb)])).max(axis=1) / (N * U64 * (nS * np.abs(Xb).max(axis=1) + np.abs(R[:len(Xb)]).max(axis=1)))).max()
    r = (float(fac.max()), float(sol), float(fwd), float(bwd))
    RATIOS[tag] = r
    print("ratio %s fac %.3f sol %.3f fwd %.3f bwd %.3f" % ((tag,) + r))
    assert r[0] <= C_FAC, (tag, r)
    assert max(r[1:]) <= C_SOL, (tag, r)


# (layout, N, band, band_hint): blocking edges ASM_NB 64, CHOL_NBI 512 (+128 remainder rule), CHOL_NBO 1024, wb switch at 1536, look-ahead from
# N > 2048, thin last tile at N mod 64 <= 16; the factor layout (one 1024-wide block up to 1024: k_chol_panel_inv at the k x k orders of the
# null-space form); banded factors (k_chol_panel_band on D, the generic banded chain elsewhere) and S0's narrow band in a factor buffer (wb 512)
SHAPES = ([(0, N, 0, 0) for N in (1, 2, 63, 64, 65, 129, 512, 513, 519, 530, 640, 641, 1031, 1536, 1537, 2113, 3079)]
          + [(1, N, 0, 0) for N in (257, 512, 519, 530, 700, 1024, 1031, 1600)]
          + [(0, N, bd, 0) for N, bd in ((700, 90), (2300, 267), (3100, 1398), (5000, 150), (2245, 40), (1100, 40), (2049, 500))]
          + [(1, 2100, 268, 268)])


@pytest.mark.parametrize("layout,N,band,band_hint", SHAPES)
def test_cholesky_in_every_launch_configuration(hip_lib, config_handle, layout, N, band, band_hint):
    """Factor, single right-hand-side solve and multi right-hand-side block substitution (forward only / forward + backward) in every
    configuration: condition-free backward errors against long-double products, the factor against LAPACK, and bit-identity of the
    configurations whose launch sequence differs only in the panel grid."""
    S, rng = _spd(N, band, N + 7 * band + layout)
    b = rng.standard_normal(N)
    big = N > 1600
    wf, wb_ = ((1, 4) if big else (130, 1)) if N % 2 else ((4, 1) if big else (1, 130))
    R = rng.standard_normal((max(wf, wb_), N))
    Sl = _ld(S)
    nS = float(np.abs(S).sum(axis=1).max())
    V = np.column_stack([np.ones(N)] + [rng.standard_normal(N) for _ in range(3)])
    Sv = Sl @ _ld(V)
    Lref = np.linalg.cholesky(S)
    out, sel = {}, {}
    for cfg in CONFIGS:
        sel[cfg] = kernel_selection(cfg, layout, N, band, band_hint)
        L, x, Xf, Xb = out[cfg] = _run_hooks(hip_lib, config_handle(cfg), S, b, R, (0, 0.0, 0.0, 1e-14), layout, band, band_hint, wf, wb_)
        assert np.isfinite(L).all() and np.abs(L - Lref).max() / np.abs(Lref).max() < 1e-11, cfg
        same = [c for c in out if c != cfg and sel[c] == sel[cfg]]
        if same:               # the same kernels, another grid: the same bits (and so the same error ratios)
            for a, c in zip(out[cfg], out[same[0]]):
                assert np.array_equal(a, c), (cfg, same[0], sel[cfg])
        else:
            _check_bounds("%d/%d/%d/%s" % (layout, N, band, cfg), S, Sl, nS, L, x, b, Xf, Xb, R, Sv, V)


# ----------------------------------------------------------------------------- dropped pivots (static guard) in every configuration
# dependent rows (pivot / diag0 = 1e-12, tests/util.py:designed_pivot_spd) at the tile edges 63 / 64, the inner-panel edge 511 / 512, the outer-panel
# edge 1023 / 1024 (N > 2048: row 1024 is factored by the look-ahead chain beside the trailing update), in the thin last tile, inside band panels;
# row 0 a zero row.  (layout, N, band, rows)
PIVOT_CASES = [(0, 2113, 0, (0, 63, 64, 511, 512, 1023, 1024, 2112)),
               (1, 705, 0, (0, 63, 64, 511, 512, 704)),                   # one 1024-wide block: k_chol_panel_inv with dropped pivots
               (0, 1100, 40, (1, 63, 64, 130, 511, 512, 1099))]


@pytest.mark.parametrize("layout,N,band,rows", PIVOT_CASES)
@pytest.mark.parametrize("setting", ["s0", "ipm", "hook"])
def test_cholesky_dropped_pivots(hip_lib, config_handle, layout, N, band, rows, setting):
    """The production guard settings on matrices with designed dependent rows: the dropped set is the designed one and the oracle's
    (_chol_guard_loop on the same prepared matrix) in every configuration, L is finite and its other columns are the oracle's, the solution
    solves the system with the dropped rows and columns removed and its dropped unknowns are ~ 0."""
    from oracle.lp_solver import _chol_guard_loop
    from tests.util import designed_pivot_spd, guard_prepare, expected_dropped, GUARD_SETTINGS, DEP_LEVEL
    st = GUARD_SETTINGS[setting]
    S, lv = designed_pivot_spd(N + len(rows), N, {j: (0.0 if j == 0 else DEP_LEVEL) for j in rows}, band=band)
    Sp, d0 = guard_prepare(S, *st[:3])
    Lo = _chol_guard_loop(Sp, d0, st[3])
    want = expected_dropped(lv, setting)
    assert np.array_equal(np.flatnonzero(np.diag(Lo) > 1e100), want)
    keep = np.setdiff1d(np.arange(N), want)
    rng = np.random.default_rng(N)
    b = rng.standard_normal(N)
    b[lv == 0.0] = 0.0                  # (a zero row kept by the regularised guard: its unknown is b_j / 1e-30)
    R = rng.standard_normal((3, N))
    Sk = _ld(Sp[np.ix_(keep, keep)])
    nS = float(np.abs(Sp[np.ix_(keep, keep)]).sum(axis=1).max())
    scale = np.abs(Lo[:, keep]).max()
    near_singular = bool((lv[keep] < 1.0).any())
    Vk = _ld(rng.standard_normal((len(keep), 4)))
    SkV = Sk @ Vk
    out, sel = {}, {}
    for cfg in CONFIGS:
        sel[cfg] = kernel_selection(cfg, layout, N, band, 0)
        L, x, Xf, Xb = out[cfg] = _run_hooks(hip_lib, config_handle(cfg), S, b, R, st, layout, band, 0, 3, 3)
        assert np.isfinite(L).all() and np.isfinite(x).all(), cfg
        assert np.array_equal(np.flatnonzero(np.diag(L) > 1e100), want), (cfg, np.flatnonzero(np.diag(L) > 1e100))
        below = np.arange(N)[:, None] > want[None, :]            # the entries under the dropped pivots: S_ij / 1e128
        assert np.abs(L[:, want]).max(initial=0.0) < 1e129 and np.abs(L[:, want][below]).max(initial=0.0) < 1e-100, cfg
        assert np.abs(x[want]).max(initial=0.0) < 1e-100 and np.abs(Xb[:, want]).max(initial=0.0) < 1e-100, cfg
        if near_singular:
            # kept rows with pivots of 1e-12: their columns of L are determined to ~1e-7 only and the substitutions through explicit block
            # inverses are not backward stable at that condition - the factor's backward error on the kept rows is what is condition-free
            Lk = _ld(L[np.ix_(keep, keep)])
            ratio = (np.abs(SkV - Lk @ (Lk.T @ Vk)).max(axis=0) / (N * U64 * nS * np.abs(Vk).max(axis=0))).max()
            print("ratio pivots %d/%d/%d/%s/%s fac %.3f" % (layout, N, band, setting, cfg, ratio))
            assert ratio <= C_FAC, (cfg, ratio)
        else:
            assert np.abs(L[:, keep] - Lo[:, keep]).max() / scale < 1e-11, cfg
            ratio = np.abs(Sk @ _ld(x[keep]) - _ld(b[keep])).max() / (N * U64 * (nS * np.abs(x[keep]).max() + np.abs(b[keep]).max()))
            ratio_b = max(np.abs(Sk @ _ld(Xb[r, keep]) - _ld(R[r, keep])).max() / (N * U64 * (nS * np.abs(Xb[r, keep]).max() + np.abs(R[r, keep]).max()))
                          for r in range(3))
            print("ratio pivots %d/%d/%d/%s/%s sol %.3f rows %.3f" % (layout, N, band, setting, cfg, ratio, ratio_b))
            assert max(ratio, ratio_b) <= C_SOL, (cfg, ratio, ratio_b)
        same = [c for c in out if c != cfg and sel[c] == sel[cfg]]
        if same:
            for a, c in zip(out[cfg], out[same[0]]):
                assert np.array_equal(a, c), (cfg, same[0], sel[cfg])


def test_cholesky_selection_threshold_ladder(hip_lib, config_handle):
    """The thresholds of the cold basis-column selection (NS_SEL_THR, absolute on a matrix of unit diagonal there): designed pivots at 1e-1,
    1e-3, 1e-6, 1e-9 and 1e-13 of a unit-diagonal matrix give the expected dropped set at each threshold, in every configuration."""
    from oracle.lp_solver import _chol_guard_loop
    from tests.util import designed_pivot_spd
    N = 300
    ladder = {63: 1e-1, 64: 1e-3, 130: 1e-6, 256: 1e-9, 299: 1e-13}
    S, lv = designed_pivot_spd(11, N, ladder)
    dg = 1.0 / np.sqrt(np.diag(S))
    S = S * dg[:, None] * dg[None, :]          # unit diagonal: the relative guard is the absolute one (the pivot levels are scale-free)
    for thr in (1e-2, 1e-4, 1e-7, 1e-10):
        want = np.array(sorted(j for j, l in ladder.items() if l < thr))
        assert np.array_equal(np.flatnonzero(np.diag(_chol_guard_loop(S, np.ones(N), thr)) > 1e100), want)
        for cfg in CONFIGS:
            h = config_handle(cfg)
            assert hip_lib.asm_test_set_factor(h, 0, 0, 0, 0.0, 0.0, thr) == 0
            L = np.zeros((N, N))
            try:
                assert hip_lib.asm_test_cholesky(h, _d(S), N, _d(L)) == 0, hip_lib.asm_last_error(h)
            finally:
                assert hip_lib.asm_test_set_factor(h, 0, 0, 0, 0.0, 0.0, 1e-14) == 0
            assert np.isfinite(L).all() and np.array_equal(np.flatnonzero(np.diag(L) > 1e100), want), (thr, cfg)
