// Kernels of the KKT solve on a working set (asm_kkt_solve, the multi entries and the trust-region step asm_kkt_step; include/asm_hip.h,
// "The KKT solve on a working set", "Many right-hand sides on one factor" and "Trust-region step on the working set"): the gathers of the working rows into dense operands, masked block updates, and the fused
// updates of the projected conjugate-gradient iteration.  One family serves every entry: the right-hand sides of a chunk are the rows
// of row-major blocks - up to KKM_CW rows of pitch ldv over the variables, of pitch ldr over the working rows - and every kernel has the
// column in blockIdx.y; asm_kkt_solve launches them with one column.  The columns are independent iterations that advance together.  A
// column whose stop code is set is frozen - no kernel writes its d, r or p again.  Every sum of a column runs in an order fixed by the
// vector length alone, so a column's bits depend neither on the number of columns nor on its place among them.
// The products with A, A' and H and the substitutions with S = A A' are not here: the host has two back ends for them (KktOneColumn:
// k_gemv_n, k_gemv_n_exact, k_gemv_t_stage*, k_hess_product and the factor's own substitution; KktBlock: k_gemm_nt through Dev::gemm_nt
// and Dev::trsm_rows, and k_kktm_hess_product below) for the dense form and a third, KktSparse, for the sparse form: its value assembly
// and its products with A and A' are at the end of this file.
// Blocks over the variables are zero beyond n and on the bound set B (mask[j] = 0 there).
// Dot products: every workgroup of a column reduces its share (wavefront shuffles, then LDS), stores its partial sums with agent-scope
// stores and counts itself in; the last one to arrive adds the partials in workgroup order - a fixed order, no atomics on doubles - and
// writes the column's scalars into its block in HBM that the next kernel reads (alpha, beta and the curvature test never visit the
// host).  The host reads one word per round: the number of active columns, published through the handle's host-mapped scalar block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "asm_bt.hip.h"

// the scalar block.  KK_STOP: 0 go on, 1 converged (or stopped on the trust-region boundary), 2 curvature p'Hp <= 0 (the iterate stays
// where it is)
enum { KK_RG = 0, KK_PHP, KK_ALPHA, KK_BETA, KK_GG, KK_R0, KK_STOP, KK_RSTAT, KK_RFEAS, KK_COUNT };
#define KK_MAXWG 64
#define KK_SLOTS 4         // partial sums per workgroup: p'Hp (g'g in k_kktm_cg_dir), then d'd, d'p, p'p of the trust-region step
struct KktRed {
    double* part;        // KK_MAXWG x KK_SLOTS partial sums
    unsigned* cnt;       // arrival counter, 0 between launches
    double* scal;        // KK_COUNT scalars in HBM
};

// true in every thread of the workgroup that arrives last; called by all threads (as red_last_arrival of the interior-point kernels)
__device__ __forceinline__ bool kk_last_arrival(const KktRed& R, bool* sh_flag) {
    if (gridDim.x == 1) return true;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        const unsigned t = __hip_atomic_fetch_add(R.cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        *sh_flag = (t == gridDim.x - 1);
        if (*sh_flag) __hip_atomic_store(R.cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    return *sh_flag;
}
__device__ __forceinline__ void kk_store(const KktRed& R, int slot, double v) {
    __hip_atomic_store(R.part + (int64_t)blockIdx.x * KK_SLOTS + slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double kk_total(const KktRed& R, int slot) {
    double s = 0.0;
    for (int w = 0; w < (int)gridDim.x; ++w) s += __hip_atomic_load(R.part + (int64_t)w * KK_SLOTS + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return s;
}

// Aw[q, j] = J[wrow[q], j] for j in F, 0 on B and in the padding: the working rows as a dense nW x ldn operand (blockIdx.y = q)
__global__ __launch_bounds__(256) void k_kkt_gather(AsmBt abt, const double* __restrict__ J, int64_t ldn, const int* __restrict__ wrow, const double* __restrict__ mask, int64_t nW, double* __restrict__ Aw) {
    ASM_BARGS(abt, J, ldn, wrow, mask, nW, Aw);
    const int64_t q = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (q >= nW || j >= ldn) return;
    Aw[q * ldn + j] = mask[j] != 0.0 ? J[(int64_t)wrow[q] * ldn + j] : 0.0;
}

// The column state.  KKM_CW columns per chunk at the most; per column KKM_SCAL doubles: the KK_* slots and its iteration count.
#define KKM_CW 64          // columns per chunk (= ASM_KKT_CHUNK)
#define KKM_SCAL 16        // doubles per column's scalar block: the KK_* slots, then
// ... the iterations the column has completed and, for the trust-region step (asm_kkt_step) alone: theta, Dt^2 = radius^2 - ||theta dx0||^2,
// the boundary code (0 inside, 1 boundary on positive curvature, 2 boundary along p'Hp <= 0), ||theta dx0||, the model value and ||dx||
enum { KKM_ITERS = KK_COUNT, KKM_THETA, KKM_DT2, KKM_BND, KKM_NNORM, KKM_MODEL, KKM_NSTEP };
struct KktMulti {
    double* part;        // KKM_CW x KK_MAXWG x KK_SLOTS partial sums
    unsigned* cnt;       // KKM_CW arrival counters of the columns' workgroups, then [KKM_CW] the counter of finished columns; 0 between launches
    double* scal;        // KKM_CW x KKM_SCAL scalars in HBM, then [KKM_CW * KKM_SCAL] the number of active columns (as a double)
    unsigned* active;    // KKM_CW flags: the column's iteration goes on
    double* hscal;       // host-mapped: [0] the number of active columns
    unsigned* hseq;      // its sequence word
};
__device__ __forceinline__ KktRed kkm_col(const KktMulti& M, int c) {
    return KktRed{M.part + (int64_t)c * KK_MAXWG * KK_SLOTS, M.cnt + c, M.scal + (int64_t)c * KKM_SCAL};
}

// AT[j, q] = J[wrow[q], j] for q < nW (mask != nullptr: 0 where mask[j] == 0), 0 for nW <= q < nWp: the working rows transposed into an
// ldn x ldt operand, its k-padding cleared (64 x 64 LDS tiles; blockIdx.x over j, blockIdx.y over q)
__global__ __launch_bounds__(256) void k_kktm_gather_t(AsmBt abt, const double* __restrict__ J, int64_t ldn, const int* __restrict__ wrow, const double* __restrict__ mask, int64_t nW, int64_t nWp, double* __restrict__ AT, int64_t ldt) {
    ASM_BARGS(abt, J, ldn, wrow, mask, nW, nWp, AT, ldt);
    __shared__ double tile[64 * 65];
    const int64_t q0 = (int64_t)blockIdx.y * 64, j0 = (int64_t)blockIdx.x * 64;
    _Pragma("unroll") for (int e_it = 0; e_it < 16; ++e_it) {
        const int e = threadIdx.x + 256 * e_it;
        const int r = e >> 6, c = e & 63;          // row q0 + r of the gather, column j0 + c
        double v = 0.0;
        if (q0 + r < nW && j0 + c < ldn && (!mask || mask[j0 + c] != 0.0)) v = J[(int64_t)wrow[q0 + r] * ldn + j0 + c];
        tile[r * 65 + c] = v;
    }
    __syncthreads();
    _Pragma("unroll") for (int e_it = 0; e_it < 16; ++e_it) {
        const int e = threadIdx.x + 256 * e_it;
        const int r = e >> 6, c = e & 63;          // out row j0 + r, out column q0 + c
        if (j0 + r < ldn && q0 + c < nWp) AT[(j0 + r) * ldt + q0 + c] = tile[c * 65 + r];
    }
}
// OUT[c, :] = H V[c, :] for the NC columns of a chunk from the values evaluated once: one thread per variable walks its list as
// k_hess_product does and uses every (value, other index) pair it reads for all the columns.  Per column the sum is k_hess_product's:
// entry order, from 0.0, no contraction - the same bits.  Rows >= cols of V are read (they exist: the blocks have KKM_CW rows), not written.
template <int NC>
__global__ __launch_bounds__(256) void k_kktm_hess_product(AsmBt abt, const int64_t* __restrict__ pptr, const int64_t* __restrict__ pent, const int64_t* __restrict__ poth, const double* __restrict__ values, const double* __restrict__ V, int64_t ldv, int64_t n, int cols, double* __restrict__ OUT) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, pptr, pent, poth, values, V, ldv, n, cols, OUT);
    const int64_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double g[NC];
    _Pragma("unroll") for (int c = 0; c < NC; ++c) g[c] = 0.0;
    for (int64_t q = pptr[i]; q < pptr[i + 1]; ++q) {
        const double val = values[pent[q]];
        const double* v = V + poth[q];
        _Pragma("unroll") for (int c = 0; c < NC; ++c) g[c] = g[c] + val * v[(int64_t)c * ldv];
    }
    _Pragma("unroll") for (int c = 0; c < NC; ++c)
        if (c < cols) OUT[(int64_t)c * ldv + i] = g[c];
}
// out[c, j] = sa * a[c, j] + sb * b[c, j] where mask[j] != 0, 0 elsewhere (b == nullptr: sa * a; mask == nullptr, blocks over the rows:
// everywhere); scal != nullptr: the frozen columns are left alone.  Blocks of pitch ld, blockIdx.y = c.  (out may be a)
__global__ __launch_bounds__(256) void k_kktm_axpby(AsmBt abt, double sa, const double* a, double sb, const double* b, const double* __restrict__ mask, int64_t len, int64_t ld, const double* __restrict__ scal, double* out) {
    ASM_BARGS(abt, sa, a, sb, b, mask, len, ld, scal, out);
    const int64_t c = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= len || (scal && scal[c * KKM_SCAL + KK_STOP] != 0.0)) return;
    const int64_t e = c * ld + j;
    double v = sa * a[e];
    if (b) v += sb * b[e];
    out[e] = (!mask || mask[j] != 0.0) ? v : 0.0;
}
// out[c, wrow[q]] = y[c, q] (out cleared before; pitches ldy, ldo)
__global__ __launch_bounds__(256) void k_kktm_scatter(AsmBt abt, const double* __restrict__ y, int64_t ldy, const int* __restrict__ wrow, int64_t nW, double* __restrict__ out, int64_t ldo) {
    ASM_BARGS(abt, y, ldy, wrow, nW, out, ldo);
    const int64_t c = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
    if (q < nW) out[c * ldo + wrow[q]] = y[c * ldy + q];
}
// the right-hand sides of one direction from the cross-derivative sweep's output cx = [u (n) | w of the expression rows]:
// ru[j] = u[j], rww[q] = w[wrow[q]] (0 for a working row of the function store: its data are not parameters)
__global__ __launch_bounds__(256) void k_kktm_cross_rhs(AsmBt abt, const double* __restrict__ cx, int64_t n, int64_t n_fn, const int* __restrict__ wrow, int64_t nW, double* __restrict__ ru, double* __restrict__ rww) {
    ASM_BARGS(abt, cx, n, n_fn, wrow, nW, ru, rww);
    const int64_t j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) ru[j] = cx[j];
    if (j < nW) {
        const int64_t i = wrow[j];
        rww[j] = i >= n_fn ? cx[n + i - n_fn] : 0.0;
    }
}
// the same for a chunk of directions at once (the block kernels' cross derivatives, k_nlp_ohm_cross / k_nlp_dense_cross_*): column
// c = blockIdx.y of cx has pitch ldc, of ru pitch ldn, of rww pitch ldT
__global__ __launch_bounds__(256) void k_kktm_cross_rhs_cols(AsmBt abt, const double* __restrict__ cx, int64_t ldc, int64_t n, int64_t n_fn, const int* __restrict__ wrow, int64_t nW, double* __restrict__ ru, int64_t ldn, double* __restrict__ rww, int64_t ldT) {
    ASM_BARGS(abt, cx, ldc, n, n_fn, wrow, nW, ru, ldn, rww, ldT);
    const int64_t c = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    cx += c * ldc;
    if (j < n) ru[c * ldn + j] = cx[j];
    if (j < nW) {
        const int64_t i = wrow[j];
        rww[c * ldT + j] = i >= n_fn ? cx[n + i - n_fn] : 0.0;
    }
}
// The right-hand sides of a chunk of bound sensitivities (asm_bound_sensitivity_multi): column c = blockIdx.y is ru = 0 and
// rw[rows[c]] = -delta[c] (delta == nullptr: -1.0), nothing else.  Every thread clears its entry of the column's ru (pitch ldn, all of
// it) and rww (pitch ldT, all of it); the thread whose place in the working-row list wrow (the order the form solves in) holds rows[c]
// stores -delta[c] instead - a row outside the working set has no such place and the column stays zero.  One writer per entry.
__global__ __launch_bounds__(256) void k_kktm_bound_rhs(AsmBt abt, const int* __restrict__ rows, const double* __restrict__ delta, const int* __restrict__ wrow, int64_t nW, double* __restrict__ ru, int64_t ldn, double* __restrict__ rww, int64_t ldT) {
    ASM_BARGS(abt, rows, delta, wrow, nW, ru, ldn, rww, ldT);
    const int64_t c = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j < ldn) ru[c * ldn + j] = 0.0;
    if (j < ldT) rww[c * ldT + j] = (j < nW && wrow[j] == rows[c]) ? -(delta ? delta[c] : 1.0) : 0.0;
}
// ---- The right-hand sides of a chunk of variable-bound sensitivities (asm_var_bound_sensitivity_multi): column c = blockIdx.y moves the
// bound of variable j = vars[c] by delta[c] (delta == nullptr: 1.0) and is ru = delta H[:, j] over all n entries, rw = delta J[W, j].  A
// variable outside B (mask[j] != 0) gives the zero column.  Four kernels, one writer per entry each:
//   k_kktm_var_unit   E[c, :] = e_j (the zero row for a variable outside B): the operand of the chunk's Hessian product
//   k_kktm_var_rhs    ru[c, k] = delta hcol[c, k] (one multiplication of what the Hessian product stored, 0 beyond n) and, dense form
//                     (J != nullptr), rww[c, q] = delta J[wrow[q], j]; sparse form (J == nullptr) rww is cleared for
//   k_kkts_var_col    rww[c, wpos[row]] = delta val over the CSC list of column j, rows outside W skipped (one workgroup per column)
//   k_kktm_var_dx     after the finish step: dx[c, j] = delta for a variable of B
__global__ __launch_bounds__(256) void k_kktm_var_unit(AsmBt abt, const int* __restrict__ vars, const double* __restrict__ mask, double* __restrict__ E, int64_t ldn) {
    ASM_BARGS(abt, vars, mask, E, ldn);
    const int64_t c = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= ldn) return;
    const int64_t j = vars[c];
    E[c * ldn + k] = (k == j && mask[j] == 0.0) ? 1.0 : 0.0;
}
__global__ __launch_bounds__(256) void k_kktm_var_rhs(AsmBt abt, const int* __restrict__ vars, const double* __restrict__ delta, const double* __restrict__ mask, const double* __restrict__ hcol, int64_t n, const double* __restrict__ J, const int* __restrict__ wrow, int64_t nW, double* __restrict__ ru, int64_t ldn, double* __restrict__ rww, int64_t ldT) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, vars, delta, mask, hcol, n, J, wrow, nW, ru, ldn, rww, ldT);
    const int64_t c = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    const int64_t j = vars[c];
    const bool in_b = mask[j] == 0.0;
    const double d = delta ? delta[c] : 1.0;
    if (k < ldn) ru[c * ldn + k] = (in_b && k < n) ? d * hcol[c * ldn + k] : 0.0;
    if (k < ldT) rww[c * ldT + k] = (in_b && J && k < nW) ? d * J[(int64_t)wrow[k] * ldn + j] : 0.0;
}
__global__ __launch_bounds__(256) void k_kkts_var_col(AsmBt abt, const int* __restrict__ vars, const double* __restrict__ delta, const double* __restrict__ mask, const int* __restrict__ cptr, const int* __restrict__ row, const int* __restrict__ pos, const double* __restrict__ val, const int* __restrict__ wpos, double* __restrict__ rww, int64_t ldT) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, vars, delta, mask, cptr, row, pos, val, wpos, rww, ldT);
    const int64_t c = blockIdx.y;
    const int j = vars[c];
    if (mask[j] != 0.0) return;
    const double d = delta ? delta[c] : 1.0;
    for (int k = cptr[j] + (int)threadIdx.x; k < cptr[j + 1]; k += 256) {
        const int p = wpos[row[k]];
        if (p >= 0) rww[c * ldT + p] = d * val[pos[k]];
    }
}
__global__ __launch_bounds__(256) void k_kktm_var_dx(AsmBt abt, const int* __restrict__ vars, const double* __restrict__ delta, const double* __restrict__ mask, int cols, double* __restrict__ dx, int64_t ldn) {
    ASM_BARGS(abt, vars, delta, mask, cols, dx, ldn);
    const int64_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    const int64_t j = vars[c];
    if (mask[j] == 0.0) dx[c * ldn + j] = delta ? delta[c] : 1.0;
}
// ---- The weights on the bound multipliers of the adjoint entries (asm_solution_adjoint_z*): gzb[c, j] = gz[c, j] on B, 0.0 on F and beyond
// n - z exists on B only - and, by the workgroups of column 0, the complementary mask cmask[j] = 1.0 on B, 0.0 elsewhere
__global__ __launch_bounds__(256) void k_kktm_gz_mask(AsmBt abt, const double* __restrict__ gz, const double* __restrict__ mask, int64_t n, int64_t ldn, double* __restrict__ gzb, double* __restrict__ cmask) {
    ASM_BARGS(abt, gz, mask, n, ldn, gzb, cmask);
    const int64_t c = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= ldn) return;
    const bool b = j < n && mask[j] == 0.0;
    gzb[c * ldn + j] = b ? gz[c * ldn + j] : 0.0;
    if (c == 0) cmask[j] = b ? 1.0 : 0.0;
}
// p[c] = -g[c] + beta_c p[c] for the active columns
__global__ __launch_bounds__(256) void k_kktm_cg_p(AsmBt abt, const double* __restrict__ scal, const double* __restrict__ g, double* __restrict__ p, int64_t len, int64_t ldv) {
    ASM_BARGS(abt, scal, g, p, len, ldv);
    const int64_t c = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const double* sc = scal + c * KKM_SCAL;
    if (j >= len || sc[KK_STOP] != 0.0) return;
    const double beta = sc[KK_BETA];
    p[c * ldv + j] = beta * p[c * ldv + j] - g[c * ldv + j];
}
// The normal step of the trust-region columns, one workgroup each (the column in blockIdx.x): nn = ||dx0||_2; where nn > share * radius
// the column's dx0 is scaled by theta = share * radius / nn, theta = 1 elsewhere (dx0 is then not written); Dt^2 = radius^2 - (theta nn)^2,
// not below 0; the boundary code starts at 0.  An infinite radius gives theta = 1 and Dt^2 = +inf.
__global__ __launch_bounds__(1024) void k_kktm_normal(AsmBt abt, double* __restrict__ scal, const double* __restrict__ radius, double share, double* __restrict__ dx0, int64_t len, int64_t ldv) {
    ASM_BARGS(abt, scal, radius, share, dx0, len, ldv);
    __shared__ double sh[16];
    const int64_t c = blockIdx.x;
    double s2 = 0.0;
    for (int64_t j = threadIdx.x; j < len; j += 1024) {
        const double v = dx0[c * ldv + j];
        s2 += v * v;
    }
    s2 = blk_reduce_sum(s2, sh);
    const double nn = sqrt(s2), rad = radius[c], cap = share * rad;
    const double theta = nn > cap ? cap / nn : 1.0;
    if (theta != 1.0)
        for (int64_t j = threadIdx.x; j < len; j += 1024) dx0[c * ldv + j] *= theta;
    if (threadIdx.x == 0) {
        double* sc = scal + c * KKM_SCAL;
        const double tn = theta * nn;
        sc[KKM_THETA] = theta;
        sc[KKM_NNORM] = tn;
        sc[KKM_DT2] = fmax(rad * rad - tn * tn, 0.0);
        sc[KKM_BND] = 0.0;
    }
}
// per active column: hp = (H p) on F; p'Hp; alpha = r'g / p'Hp, or the curvature stop.
// TR (asm_kkt_step): the same pass also sums d'd, d'p and p'p (partial-sum slots 1 to 3, added in workgroup order as slot 0 is), and the
// thread that has the totals applies the Steihaug-Toint rule: with gap = Dt^2 - d'd and tau = gap / (d'p + sqrt((d'p)^2 + p'p gap)) (0
// when gap <= 0), a finite Dt^2 and p'Hp <= 0 give alpha = tau and boundary code 2; p'Hp > 0 and d'd + 2 alpha d'p + alpha^2 p'p >= Dt^2
// give alpha = tau and boundary code 1.  Such a column takes this alpha in the round's k_kktm_cg_step and is frozen by its k_kktm_cg_dir.
template <bool TR>
__global__ __launch_bounds__(256) void k_kktm_cg_curv(AsmBt abt, KktMulti M, const double* __restrict__ p, const double* __restrict__ hp_raw, const double* __restrict__ mask, const double* __restrict__ d, double* __restrict__ hp, int64_t len, int64_t ldv) {
    ASM_BARGS(abt, M, p, hp_raw, mask, d, hp, len, ldv);
    __shared__ double sh[4];
    __shared__ bool last;
    const int64_t c = blockIdx.y;
    const KktRed R = kkm_col(M, (int)c);
    if (R.scal[KK_STOP] != 0.0) return;          // (set by an earlier launch: the same in every workgroup of the column)
    double acc = 0.0, dd = 0.0, dp = 0.0, pp = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < len; j += (int64_t)gridDim.x * 256) {
        const double v = mask[j] != 0.0 ? hp_raw[c * ldv + j] : 0.0;
        hp[c * ldv + j] = v;
        const double pj = p[c * ldv + j];
        acc += pj * v;
        if (TR) {
            const double dj = d[c * ldv + j];
            dd += dj * dj;
            dp += dj * pj;
            pp += pj * pj;
        }
    }
    acc = blk_reduce_sum(acc, sh);
    if (TR) {
        dd = blk_reduce_sum(dd, sh);
        dp = blk_reduce_sum(dp, sh);
        pp = blk_reduce_sum(pp, sh);
    }
    if (gridDim.x > 1) {
        if (threadIdx.x == 0) {
            kk_store(R, 0, acc);
            if (TR) { kk_store(R, 1, dd); kk_store(R, 2, dp); kk_store(R, 3, pp); }
        }
        if (!kk_last_arrival(R, &last)) return;
        if (threadIdx.x == 0) {
            acc = kk_total(R, 0);
            if (TR) { dd = kk_total(R, 1); dp = kk_total(R, 2); pp = kk_total(R, 3); }
        }
    }
    if (threadIdx.x == 0) {
        R.scal[KK_PHP] = acc;
        const double dt2 = TR ? R.scal[KKM_DT2] : INFINITY;
        double tau = 0.0;
        if (TR) {
            const double gap = dt2 - dd;
            if (gap > 0.0 && gap < INFINITY) tau = gap / (dp + sqrt(dp * dp + pp * gap));
        }
        if (!(acc > 0.0)) {
            if (dt2 < INFINITY) {      // along the direction of non-positive curvature to the boundary
                R.scal[KK_ALPHA] = tau;
                R.scal[KKM_BND] = 2.0;
            } else {                   // the curvature stop: the column leaves the active count that the round's k_kktm_cg_dir adds up
                R.scal[KK_STOP] = 2.0;
                __hip_atomic_store(M.active + c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else {
            const double alpha = R.scal[KK_RG] / acc;
            if (TR && dd + 2.0 * alpha * dp + alpha * alpha * pp >= dt2) {
                R.scal[KK_ALPHA] = tau;
                R.scal[KKM_BND] = 1.0;
            } else {
                R.scal[KK_ALPHA] = alpha;
            }
        }
    }
}
// d[c] += alpha_c p[c], r[c] += alpha_c hp[c] for the active columns
__global__ __launch_bounds__(256) void k_kktm_cg_step(AsmBt abt, const double* __restrict__ scal, const double* __restrict__ p, const double* __restrict__ hp, double* __restrict__ d, double* __restrict__ r, int64_t len, int64_t ldv) {
    ASM_BARGS(abt, scal, p, hp, d, r, len, ldv);
    const int64_t c = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const double* sc = scal + c * KKM_SCAL;
    if (j >= len || sc[KK_STOP] != 0.0) return;
    const double alpha = sc[KK_ALPHA];
    const int64_t e = c * ldv + j;
    d[e] += alpha * p[e];
    r[e] += alpha * hp[e];
}
// per active column, with the projected residual r = g in place: r'g and g'g, beta, the convergence test against the column's own
// ||g0|| and its iteration count (init: the reference norm, beta = 0, g0 = 0 stops at once).  The workgroup that finishes a column
// counts the column in; the one that finishes the last column counts the columns still active and hands that word to the host.
// tr != 0 (asm_kkt_step): a column whose k_kktm_cg_curv of this round set a boundary code has taken its last step and stops here; the
// boundary move counts as a completed iteration.
__global__ __launch_bounds__(256) void k_kktm_cg_dir(AsmBt abt, KktMulti M, const double* __restrict__ r, int64_t len, int64_t ldv, int init, double rtol, unsigned pub, int tr) {
    ASM_BARGS(abt, M, r, len, ldv, init, rtol, pub, tr);
    __shared__ double sh[4];
    __shared__ bool last, lastcol;
    const int64_t c = blockIdx.y;
    const KktRed R = kkm_col(M, (int)c);
    if (!init && R.scal[KK_STOP] != 0.0) {        // frozen by an earlier launch: only counted in, by one of its workgroups
        if (blockIdx.x != 0) return;
    } else {
        double gg = 0.0;
        for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < len; j += (int64_t)gridDim.x * 256) {
            const double gj = r[c * ldv + j];
            gg += gj * gj;
        }
        gg = blk_reduce_sum(gg, sh);
        if (gridDim.x > 1) {
            if (threadIdx.x == 0) kk_store(R, 0, gg);
            if (!kk_last_arrival(R, &last)) return;
            if (threadIdx.x == 0) gg = kk_total(R, 0);
        }
        if (threadIdx.x == 0) {
            double stop;
            if (init) {
                R.scal[KK_RG] = gg; R.scal[KK_GG] = gg; R.scal[KK_R0] = sqrt(gg); R.scal[KK_BETA] = 0.0; R.scal[KK_ALPHA] = 0.0; R.scal[KK_PHP] = 0.0;
                R.scal[KKM_ITERS] = 0.0;
                stop = gg == 0.0 ? 1.0 : 0.0;
            } else {
                R.scal[KK_BETA] = gg / R.scal[KK_RG];
                R.scal[KK_RG] = gg; R.scal[KK_GG] = gg;
                R.scal[KKM_ITERS] += 1.0;
                stop = sqrt(gg) <= rtol * R.scal[KK_R0] || (tr && R.scal[KKM_BND] != 0.0) ? 1.0 : 0.0;
            }
            R.scal[KK_STOP] = stop;
            __hip_atomic_store(M.active + c, stop == 0.0 ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // this workgroup has finished its column
    if (threadIdx.x == 0) {
        unsigned* colcnt = M.cnt + KKM_CW;
        __threadfence();
        const unsigned t = __hip_atomic_fetch_add(colcnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        lastcol = (t == gridDim.y - 1);
        if (lastcol) __hip_atomic_store(colcnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!lastcol) return;
    double act = 0.0;
    for (int cc = threadIdx.x; cc < (int)gridDim.y; cc += 256) act += (double)__hip_atomic_load(M.active + cc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    act = blk_reduce_sum(act, sh);
    if (threadIdx.x == 0) {
        M.scal[KKM_CW * KKM_SCAL] = act;
        if (pub != 0) {
            M.hscal[0] = act;
            __threadfence_system();
            __hip_atomic_store(M.hseq, pub, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
// the bound multipliers and the residuals of every column, one workgroup each (the column in blockIdx.x):
//   dz[j] = (H dx)[j] + ru[j] - (J' dlam)[j] on B, 0 on F;   res_stat = max over F of |(H dx)[j] + ru[j] - (J' dlam)[j]|;
//   res_feas = max over the working rows of |(A dx)[q] + rw[q]|
// dx != nullptr (asm_kkt_step): rw is theta rw, and the column's model value ru'dx + 1/2 dx'(H dx) and ||dx||_2 join its scalars
__global__ __launch_bounds__(1024) void k_kktm_finish(AsmBt abt, double* __restrict__ scal, const double* __restrict__ hdx, const double* __restrict__ ru, const double* __restrict__ jtl, const double* __restrict__ mask, int64_t n, int64_t ldv, const double* __restrict__ adx, const double* __restrict__ rww, int64_t nW, int64_t ldr, double* __restrict__ dz, const double* __restrict__ dx) {
    ASM_BARGS(abt, scal, hdx, ru, jtl, mask, n, ldv, adx, rww, nW, ldr, dz, dx);
    __shared__ double sh[16];
    const int64_t c = blockIdx.x;
    const double theta = dx ? scal[c * KKM_SCAL + KKM_THETA] : 1.0;
    double rs = 0.0, rf = 0.0, lin = 0.0, quad = 0.0, sq = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += 1024) {
        const int64_t e = c * ldv + j;
        const double v = (hdx[e] + ru[e]) - jtl[e];
        const bool fr = mask[j] != 0.0;
        dz[e] = fr ? 0.0 : v;
        if (fr) rs = fmax(rs, fabs(v));
        if (dx) {
            const double x = dx[e];
            lin += ru[e] * x;
            quad += x * hdx[e];
            sq += x * x;
        }
    }
    for (int64_t q = threadIdx.x; q < nW; q += 1024) rf = fmax(rf, fabs(adx[c * ldr + q] + theta * rww[c * ldr + q]));
    rs = blk_reduce_max(rs, sh);
    rf = blk_reduce_max(rf, sh);
    if (dx) {
        lin = blk_reduce_sum(lin, sh);
        quad = blk_reduce_sum(quad, sh);
        sq = blk_reduce_sum(sq, sh);
    }
    if (threadIdx.x == 0) {
        scal[c * KKM_SCAL + KK_RSTAT] = rs;
        scal[c * KKM_SCAL + KK_RFEAS] = rf;
        if (dx) { scal[c * KKM_SCAL + KKM_MODEL] = lin + 0.5 * quad; scal[c * KKM_SCAL + KKM_NSTEP] = sqrt(sq); }
    }
}

// ---- the sparse form (asm_kkt_set_form, ASM_KKT_SPARSE): A = J[W, F] stays in the skeleton's CSR / CSC pattern, the working rows in the
// reverse Cuthill-McKee order of their coupling graph (wrow lists them in that order, wpos[i] is the place of row i in it, -1: not in W).
// The products run on the same row-major blocks as the dense back ends.  Mapping ("KKT solve: the sparse form"): the outputs
// of ONE right-hand side along the lanes, LANES lanes per output walking its entry list, the right-hand side in blockIdx.y.  A wavefront
// then reads neighbouring outputs' lists (contiguous) and gathers from one row of the block (neighbouring rows of a banded order share
// columns); lanes across the right-hand sides would read the block with stride ldv, one cache line per lane.  A sum runs in an order
// fixed by the list and LANES alone - entries k, k + LANES, ... per lane, then an xor tree - so a column's bits depend neither on the
// number of columns nor on its place; no atomics.

// vals[u] = sum of dE over the duplicates of unique Jacobian entry u (k_assemble's sum, without a dense J): the first nu entries of the
// CSR list are the unique entries in the same order
__global__ __launch_bounds__(256) void k_kkts_vals(AsmBt abt, const double* __restrict__ dE, const int64_t* __restrict__ perm, const int64_t* __restrict__ ustart, int64_t nu, double* __restrict__ vals) {
    ASM_BARGS(abt, dE, perm, ustart, nu, vals);
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < nu; u += (int64_t)gridDim.x * blockDim.x) {
        double acc = 0.0;
        for (int64_t k = ustart[u]; k < ustart[u + 1]; ++k) acc = acc + dE[perm[k]];
        vals[u] = acc;
    }
}
// the static row order (asm_kkt_set_order): the position list from the uploaded working rows, wpos[i] = -1 for all M LP rows and then
// wpos[wrow[q]] = q, q < nW.  One workgroup, so that the clearing is ordered before the scatter by its barrier; the grid is (1) for
// every working set and every scenario.  S is then built by k_schur_sparse from the row-index pairs of all rows through this list.
__global__ __launch_bounds__(1024) void k_kkts_wpos(AsmBt abt, const int* __restrict__ wrow, int64_t nW, int64_t M, int* __restrict__ wpos) {
    ASM_BARGS(abt, wrow, nW, M, wpos);
    for (int64_t i = threadIdx.x; i < M; i += 1024) wpos[i] = -1;
    __syncthreads();
    for (int64_t q = threadIdx.x; q < nW; q += 1024) wpos[wrow[q]] = (int)q;
}
// T[c, q] = sum over the CSR list of row wrow[q] of val_k mask[col_k] V[c, col_k], q < nW (the k-padding of T beyond nW is not written)
template <int LANES>
__global__ __launch_bounds__(256) void k_kkts_mul_a(AsmBt abt, const int* __restrict__ ptr, const int* __restrict__ col, const double* __restrict__ val, const int* __restrict__ wrow, const double* __restrict__ mask, const double* __restrict__ V, int64_t ldv, int64_t nW, double* __restrict__ T, int64_t ldt) {
    ASM_BARGS(abt, ptr, col, val, wrow, mask, V, ldv, nW, T, ldt);
    const int64_t c = blockIdx.y, q = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LANES;
    const int sub = threadIdx.x & (LANES - 1);
    const double* v = V + c * ldv;
    double acc = 0.0;
    if (q < nW) {
        const int r = wrow[q];
        for (int k = ptr[r] + sub; k < ptr[r + 1]; k += LANES) {
            const int j = col[k];
            acc += val[k] * mask[j] * v[j];
        }
    }
    _Pragma("unroll") for (int o = LANES / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (sub == 0 && q < nW) T[c * ldt + q] = acc;
}
// V[c, j] = mask[j] * sum over the CSC list of column j of val Y[c, wpos[row]], rows outside W skipped (mask == nullptr: no mask, J_W' y
// over all variables); 0 for n <= j < ldn
template <int LANES>
__global__ __launch_bounds__(256) void k_kkts_mul_at(AsmBt abt, const int* __restrict__ cptr, const int* __restrict__ row, const int* __restrict__ pos, const double* __restrict__ val, const int* __restrict__ wpos, const double* __restrict__ mask, const double* __restrict__ Y, int64_t ldy, int64_t n, int64_t ldn, double* __restrict__ V, int64_t ldv) {
    ASM_BARGS(abt, cptr, row, pos, val, wpos, mask, Y, ldy, n, ldn, V, ldv);
    const int64_t c = blockIdx.y, j = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LANES;
    const int sub = threadIdx.x & (LANES - 1);
    const double* y = Y + c * ldy;
    double acc = 0.0;
    if (j < n && (!mask || mask[j] != 0.0)) {
        for (int k = cptr[j] + sub; k < cptr[j + 1]; k += LANES) {
            const int p = wpos[row[k]];
            if (p >= 0) acc += val[pos[k]] * y[p];
        }
    }
    _Pragma("unroll") for (int o = LANES / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (sub == 0 && j < ldn) V[c * ldv + j] = acc;
}
