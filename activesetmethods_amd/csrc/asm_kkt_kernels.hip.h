// Kernels of the KKT solve on a working set (asm_kkt_solve; include/asm_hip.h, "The KKT solve on a working set"): the gather of the
// working rows into a dense operand, masked vector updates, and the fused updates of the projected conjugate-gradient iteration.
// The matrix products (k_gemv_n, k_gemv_n_exact, k_gemv_t_stage*), the rank-K build, the Cholesky factorisation and its substitutions
// and the Hessian product (k_hess_product) are the library's existing kernels.  A and S are dense here: the sparse, banded and
// null-space forms of the LP solver have no counterpart.
// Vectors over the variables have the pitch ldn of the dense operands and are zero beyond n and on the bound set B (mask[j] = 0 there).
// Dot products: every workgroup reduces its share (wavefront shuffles, then LDS), stores its partial sums with agent-scope stores and
// counts itself in; the last one to arrive adds the partials in workgroup order - a fixed order, no atomics on doubles - and writes
// the scalars of the iteration into a block in HBM that the next kernel reads (alpha, beta and the curvature test never visit the
// host).  The host reads one word per iteration: the stop code, published through the handle's host-mapped scalar block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "asm_bt.hip.h"

// the scalar block.  KK_STOP: 0 go on, 1 converged, 2 curvature p'Hp <= 0 (the iterate stays where it is)
enum { KK_RG = 0, KK_PHP, KK_ALPHA, KK_BETA, KK_GG, KK_R0, KK_STOP, KK_RSTAT, KK_RFEAS, KK_COUNT };
#define KK_MAXWG 64
#define KK_SLOTS 2
struct KktRed {
    double* part;        // KK_MAXWG x KK_SLOTS partial sums
    unsigned* cnt;       // arrival counter, 0 between launches
    double* scal;        // KK_COUNT scalars in HBM
    double* hscal;       // the same block in host-mapped memory
    unsigned* hseq;      // its sequence word
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
// the workgroup that wrote R.scal hands the block to the host: stores into host-mapped memory, a system-scope fence, the sequence word
__device__ __forceinline__ void kk_publish(const KktRed& R, unsigned pub) {
    if (pub == 0) return;
    __syncthreads();
    if (threadIdx.x < KK_COUNT) R.hscal[threadIdx.x] = R.scal[threadIdx.x];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(R.hseq, pub, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Aw[q, j] = J[wrow[q], j] for j in F, 0 on B and in the padding: the working rows as a dense nW x ldn operand (blockIdx.y = q)
__global__ __launch_bounds__(256) void k_kkt_gather(AsmBt abt, const double* __restrict__ J, int64_t ldn, const int* __restrict__ wrow, const double* __restrict__ mask, int64_t nW, double* __restrict__ Aw) {
    ASM_BARGS(abt, J, ldn, wrow, mask, nW, Aw);
    const int64_t q = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (q >= nW || j >= ldn) return;
    Aw[q * ldn + j] = mask[j] != 0.0 ? J[(int64_t)wrow[q] * ldn + j] : 0.0;
}
// out[wrow[q]] = y[q]: the multipliers of the working rows into their places among all m rows (out cleared before)
__global__ __launch_bounds__(256) void k_kkt_scatter(AsmBt abt, const double* __restrict__ y, const int* __restrict__ wrow, int64_t nW, double* __restrict__ out) {
    ASM_BARGS(abt, y, wrow, nW, out);
    const int64_t q = blockIdx.x * 256 + threadIdx.x;
    if (q < nW) out[wrow[q]] = y[q];
}
// out[j] = sa * a[j] + sb * b[j] on F, 0 elsewhere (b == nullptr: sa * a[j]; mask == nullptr, a vector over the rows: everywhere)
__global__ __launch_bounds__(256) void k_kkt_axpby_mask(AsmBt abt, double sa, const double* a, double sb, const double* __restrict__ b, const double* __restrict__ mask, int64_t len, double* out) {      // (out may be a)
    ASM_BARGS(abt, sa, a, sb, b, mask, len, out);
    const int64_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= len) return;
    double v = sa * a[j];
    if (b) v += sb * b[j];
    out[j] = (!mask || mask[j] != 0.0) ? v : 0.0;
}
// p = -g + beta p, beta from the scalar block (0 before the first iteration)
__global__ __launch_bounds__(256) void k_kkt_cg_p(AsmBt abt, const double* __restrict__ scal, const double* __restrict__ g, double* __restrict__ p, int64_t len) {
    ASM_BARGS(abt, scal, g, p, len);
    const int64_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= len) return;
    const double beta = scal[KK_BETA];
    p[j] = beta * p[j] - g[j];
}
// hp = (H p) on F; p'Hp; alpha = r'g / p'Hp, or the curvature stop when p'Hp <= 0 (or not a number)
__global__ __launch_bounds__(256) void k_kkt_cg_curv(AsmBt abt, KktRed R, const double* __restrict__ p, const double* __restrict__ hp_raw, const double* __restrict__ mask, double* __restrict__ hp, int64_t len) {
    ASM_BARGS(abt, R, p, hp_raw, mask, hp, len);
    __shared__ double sh[4];
    __shared__ bool last;
    double acc = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < len; j += (int64_t)gridDim.x * 256) {
        const double v = mask[j] != 0.0 ? hp_raw[j] : 0.0;
        hp[j] = v;
        acc += p[j] * v;
    }
    acc = blk_reduce_sum(acc, sh);
    if (gridDim.x > 1) {
        if (threadIdx.x == 0) kk_store(R, 0, acc);
        if (!kk_last_arrival(R, &last)) return;
        if (threadIdx.x == 0) acc = kk_total(R, 0);
    }
    if (threadIdx.x == 0) {
        R.scal[KK_PHP] = acc;
        if (R.scal[KK_STOP] == 0.0) {
            if (!(acc > 0.0)) R.scal[KK_STOP] = 2.0;
            else R.scal[KK_ALPHA] = R.scal[KK_RG] / acc;
        }
    }
}
// d += alpha p, r += alpha hp; nothing after a stop
__global__ __launch_bounds__(256) void k_kkt_cg_step(AsmBt abt, const double* __restrict__ scal, const double* __restrict__ p, const double* __restrict__ hp, double* __restrict__ d, double* __restrict__ r, int64_t len) {
    ASM_BARGS(abt, scal, p, hp, d, r, len);
    const int64_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= len || scal[KK_STOP] != 0.0) return;
    const double alpha = scal[KK_ALPHA];
    d[j] += alpha * p[j];
    r[j] += alpha * hp[j];
}
// g = P r has been formed (the residual is kept projected: the caller passes r = g): r'g and g'g; beta = r'g / (the previous r'g); the
// convergence test ||g|| <= rtol ||g0||.  init: the first projected residual - its norm is the reference of the test, beta = 0, and
// g0 = 0 stops at once.  The block goes to the host (pub != 0).
__global__ __launch_bounds__(256) void k_kkt_cg_dir(AsmBt abt, KktRed R, const double* r, const double* g, int64_t len, int init, double rtol, unsigned pub) {
    ASM_BARGS(abt, R, r, g, len, init, rtol, pub);
    __shared__ double sh[4];
    __shared__ bool last;
    double rg = 0.0, gg = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < len; j += (int64_t)gridDim.x * 256) {
        const double gj = g[j];
        rg += r[j] * gj;
        gg += gj * gj;
    }
    rg = blk_reduce_sum(rg, sh);
    gg = blk_reduce_sum(gg, sh);
    if (gridDim.x > 1) {
        if (threadIdx.x == 0) { kk_store(R, 0, rg); kk_store(R, 1, gg); }
        if (!kk_last_arrival(R, &last)) return;
        if (threadIdx.x == 0) { rg = kk_total(R, 0); gg = kk_total(R, 1); }
    }
    if (threadIdx.x == 0) {
        if (init) {
            R.scal[KK_RG] = rg; R.scal[KK_GG] = gg; R.scal[KK_R0] = sqrt(gg); R.scal[KK_BETA] = 0.0; R.scal[KK_ALPHA] = 0.0; R.scal[KK_PHP] = 0.0;
            R.scal[KK_STOP] = gg == 0.0 ? 1.0 : 0.0;
        } else if (R.scal[KK_STOP] == 0.0) {
            R.scal[KK_BETA] = rg / R.scal[KK_RG];
            R.scal[KK_RG] = rg; R.scal[KK_GG] = gg;
            if (sqrt(gg) <= rtol * R.scal[KK_R0]) R.scal[KK_STOP] = 1.0;
        }
    }
    kk_publish(R, pub);
}
// the bound multipliers and the residuals of the returned solution, one workgroup:
//   dz[j] = (H dx)[j] + ru[j] - (J' dlam)[j] on B, 0 on F;   res_stat = max over F of |(H dx)[j] + ru[j] - (J' dlam)[j]|;
//   res_feas = max over the working rows of |(A dx)[q] + rw[q]|
__global__ __launch_bounds__(1024) void k_kkt_finish(AsmBt abt, KktRed R, const double* __restrict__ hdx, const double* __restrict__ ru, const double* __restrict__ jtl, const double* __restrict__ mask, int64_t n, const double* __restrict__ adx, const double* __restrict__ rww, int64_t nW, double* __restrict__ dz) {
    ASM_BARGS(abt, R, hdx, ru, jtl, mask, n, adx, rww, nW, dz);
    __shared__ double sh[16];
    double rs = 0.0, rf = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += 1024) {
        const double v = (hdx[j] + ru[j]) - jtl[j];
        const bool fr = mask[j] != 0.0;
        dz[j] = fr ? 0.0 : v;
        if (fr) rs = fmax(rs, fabs(v));
    }
    for (int64_t q = threadIdx.x; q < nW; q += 1024) rf = fmax(rf, fabs(adx[q] + rww[q]));
    rs = blk_reduce_max(rs, sh);
    rf = blk_reduce_max(rf, sh);
    if (threadIdx.x == 0) { R.scal[KK_RSTAT] = rs; R.scal[KK_RFEAS] = rf; }
}
