// Kernels of the validity ranges (asm_sensitivity_range_multi; include/asm_hip.h, "Validity ranges"): for every column (dx, dlam, dz) of a
// chunk and both signs of t, the first t at which x + t dx, lam + t dlam, z + t dz leave the working set - an inactive row or a free
// variable reaches a bound, the multiplier of a working row or of a bound reaches zero.
//   rows part        k_range_rows_sparse / k_range_rows_dense: V = J dx for every row and the candidates of kinds 1, 2 and 5
//   variables part   k_range_vars: the candidates of kinds 3, 4 and 6, then the minimum over everything
// One thread owns one row (or variable) and RG_CPT columns; a wavefront owns 64 rows and its RG_CPT columns, a workgroup of four wavefronts
// RG_CPB columns, grid.y the groups of RG_CPB columns of the chunk.  An entry of J is loaded once per RG_CPT columns.
// V_i of a column is one thread's sum over the row's CSR list (sparse) or over j = 0 .. n - 1 (dense), from 0.0, product then sum, no
// contraction: the order is the row's own, and a column's bits depend neither on the number of columns nor on its place.
// The minimum: a candidate is (ratio, position, kind), ordered by ratio and then by position (rows 0 .. m - 1, variables m .. m + n - 1).
// A wavefront reduces its 64 candidates by an xor tree - the order of a minimum does not change its value - and stores one partial
// candidate per (workgroup, column, side) with agent-scope stores.  The workgroups of k_range_vars count themselves in per grid.y; the
// last one to arrive combines the partial candidates of both launches in workgroup order (k_range_rows_* has finished: stream order) -
// the pattern of KktRed / kk_last_arrival.  No atomics on doubles.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "asm_bt.hip.h"

#define RG_CW 64           // columns per chunk (= ASM_KKT_CHUNK)
#define RG_CPT 8           // columns per thread
#define RG_CPB 32          // columns per workgroup: four wavefronts of RG_CPT
#define RG_TILE 64         // rows or variables per workgroup: one per lane
#define RG_DJ 32           // dense rows: columns of J per tile in LDS

// the point: what the evaluator left at x (E), the problem's bounds, the multipliers and the states
struct RangePoint {
    const double *E, *g_L, *g_U, *lam;      // m
    const int* rs;                          // m: row_state
    const double *x, *x_L, *x_U, *z;        // n
    const int* bs;                          // n: bound_state
    int64_t m, n;
};
// the partial candidates: slot w of k_range_rows_* is workgroup w, of k_range_vars n_row_wg + w; per slot RG_CW columns x 2 sides
struct RangeRed {
    double* pt;          // slots x RG_CW x 2 ratios
    int* pk;             // slots x RG_CW x 2 x { position, kind }
    unsigned* cnt;       // arrival counters of k_range_vars, one per blockIdx.y; 0 between launches
};
// what the host reads: asm_range_info of the header
struct RangeOut {
    double t_lo, t_hi;
    int pos_lo, kind_lo, pos_hi, kind_hi;
};

struct RangeCand {
    double t;
    int pos, kind;
};
__device__ __forceinline__ RangeCand rg_none() { return RangeCand{INFINITY, -1, 0}; }
// a ratio clamped from below at 0 as a candidate; one that is not below +inf (or is NaN) is no candidate
__device__ __forceinline__ RangeCand rg_offer(double r, int pos, int kind) {
    r = r < 0.0 ? 0.0 : r;
    return r < INFINITY ? RangeCand{r, pos, kind} : rg_none();
}
__device__ __forceinline__ RangeCand rg_min(const RangeCand& a, const RangeCand& b) { return (b.t < a.t || (b.t == a.t && b.pos < a.pos)) ? b : a; }
__device__ __forceinline__ RangeCand rg_wave_min(RangeCand c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const RangeCand b{__shfl_xor(c.t, o, 64), __shfl_xor(c.pos, o, 64), __shfl_xor(c.kind, o, 64)};
        c = rg_min(c, b);
    }
    return c;
}
__device__ __forceinline__ void rg_store(const RangeRed& R, int64_t slot, int c, int side, const RangeCand& b) {
    const int64_t at = (slot * RG_CW + c) * 2 + side;
    __hip_atomic_store(R.pt + at, b.t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(R.pk + 2 * at, b.pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(R.pk + 2 * at + 1, b.kind, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the candidate of row i on side sg (-1.0 / +1.0) from V_i = (J dx)_i and dlam_i: kinds 1, 2 (i outside W) and 5 (i in W, not an equality)
__device__ __forceinline__ RangeCand rg_row(double sg, int i, int rs, double E, double lo, double up, double lam, double V, double dlam) {
    if (rs == 0) {
        const double v = sg * V;
        if (v < 0.0 && lo > -INFINITY) return rg_offer((lo - E) / v, i, 1);
        if (v > 0.0 && up < INFINITY) return rg_offer((up - E) / v, i, 2);
        return rg_none();
    }
    if (lo == up) return rg_none();
    const bool upper = !(lo > -INFINITY) || (up < INFINITY && fabs(E - up) < fabs(E - lo));
    const double dl = sg * dlam;
    if (upper ? dl > 0.0 : dl < 0.0) return rg_offer(-lam / dl, i, 5);
    return rg_none();
}
// the candidate of variable j at position pos = m + j: kinds 3, 4 (j in F) and 6 (j in B)
__device__ __forceinline__ RangeCand rg_var(double sg, int pos, int bs, double x, double lo, double up, double z, double dx, double dz) {
    if (bs == 0) {
        const double v = sg * dx;
        if (v < 0.0 && lo > -INFINITY) return rg_offer((lo - x) / v, pos, 3);
        if (v > 0.0 && up < INFINITY) return rg_offer((up - x) / v, pos, 4);
        return rg_none();
    }
    const double dv = sg * dz;
    if (bs > 0 ? dv > 0.0 : dv < 0.0) return rg_offer(-z / dv, pos, 6);
    return rg_none();
}

// the rows part after V: the candidates of the thread's row for its RG_CPT columns, both sides, the wavefront's minimum, one store each
__device__ __forceinline__ void rg_rows_finish(const RangePoint& P, const RangeRed& R, int64_t i, int c0, const double (&acc)[RG_CPT], const double* __restrict__ DLAM, int64_t ldm,
                                               int cols) {
    const bool in = i < P.m;
    const int rs = in ? P.rs[i] : 0;
    const double E = in ? P.E[i] : 0.0, lo = in ? P.g_L[i] : 0.0, up = in ? P.g_U[i] : 0.0, lam = in ? P.lam[i] : 0.0;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < RG_CPT; ++q) {
        const int c = c0 + q;
        if (c >= cols) break;      // (uniform in the wavefront)
        const double dl = in ? DLAM[(int64_t)c * ldm + i] : 0.0;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const double sg = side ? 1.0 : -1.0;
            const RangeCand b = rg_wave_min(in ? rg_row(sg, (int)i, rs, E, lo, up, lam, acc[q], dl) : rg_none());
            if (lane == 0) rg_store(R, blockIdx.x, c, side, b);
        }
    }
}

// Rows part, J as the CSR list of the skeleton's pattern (ptr, col over the LP rows; val: the values of the first m rows).  DX cols x ldn,
// DLAM cols x ldm.  Grid (ceil(m / RG_TILE), ceil(cols / RG_CPB)), 256 threads.
__global__ __launch_bounds__(256) void k_range_rows_sparse(AsmBt abt, RangePoint P, const int* __restrict__ ptr, const int* __restrict__ col, const double* __restrict__ val, const double* __restrict__ DX, int64_t ldn, const double* __restrict__ DLAM, int64_t ldm, int cols, RangeRed R) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, P, ptr, col, val, DX, ldn, DLAM, ldm, cols, R);
    const int64_t i = (int64_t)blockIdx.x * RG_TILE + (threadIdx.x & 63);
    const int c0 = (int)blockIdx.y * RG_CPB + (int)(threadIdx.x >> 6) * RG_CPT;
    if (c0 >= cols) return;      // (a whole wavefront; no barrier follows)
    double acc[RG_CPT];
#pragma unroll
    for (int q = 0; q < RG_CPT; ++q) acc[q] = 0.0;
    if (i < P.m) {
        const double* d0 = DX + (int64_t)c0 * ldn;      // (the block has RG_CW rows: columns beyond cols are read, not used)
        for (int k = ptr[i]; k < ptr[i + 1]; ++k) {
            const double a = val[k];
            const int j = col[k];
#pragma unroll
            for (int q = 0; q < RG_CPT; ++q) acc[q] = acc[q] + a * d0[(int64_t)q * ldn + j];
        }
    }
    rg_rows_finish(P, R, i, c0, acc, DLAM, ldm, cols);
}

// Rows part, J as dense rows of pitch ldn: the workgroup's 64 rows go through LDS in tiles of RG_DJ columns, loaded along the rows, and
// every thread sums its row over j = 0 .. n - 1 in that order.  The same grid.
__global__ __launch_bounds__(256) void k_range_rows_dense(AsmBt abt, RangePoint P, const double* __restrict__ J, const double* __restrict__ DX, int64_t ldn, const double* __restrict__ DLAM, int64_t ldm, int cols, RangeRed R) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, P, J, DX, ldn, DLAM, ldm, cols, R);
    __shared__ double tile[RG_TILE][RG_DJ + 1];
    const int lane = threadIdx.x & 63;
    const int64_t i0 = (int64_t)blockIdx.x * RG_TILE, i = i0 + lane;
    const int c0 = (int)blockIdx.y * RG_CPB + (int)(threadIdx.x >> 6) * RG_CPT;
    const bool on = c0 < cols;      // (every wavefront takes part in the loads and the barriers)
    double acc[RG_CPT];
#pragma unroll
    for (int q = 0; q < RG_CPT; ++q) acc[q] = 0.0;
    const double* d0 = DX + (int64_t)(on ? c0 : 0) * ldn;
    const int jj = threadIdx.x & (RG_DJ - 1), r0 = threadIdx.x / RG_DJ;
    for (int64_t j0 = 0; j0 < P.n; j0 += RG_DJ) {
        __syncthreads();
        for (int r = r0; r < RG_TILE; r += 256 / RG_DJ) {
            const int64_t row = i0 + r, j = j0 + jj;
            tile[r][jj] = (row < P.m && j < P.n) ? J[row * ldn + j] : 0.0;
        }
        __syncthreads();
        if (on && i < P.m) {
            const int w = (int)(P.n - j0 < RG_DJ ? P.n - j0 : RG_DJ);
            for (int t = 0; t < w; ++t) {
                const double a = tile[lane][t];
#pragma unroll
                for (int q = 0; q < RG_CPT; ++q) acc[q] = acc[q] + a * d0[(int64_t)q * ldn + j0 + t];
            }
        }
    }
    if (on) rg_rows_finish(P, R, i, c0, acc, DLAM, ldm, cols);
}

// Variables part and the minimum.  DX, DZ cols x ldn; n_row_wg: the workgroups of the rows part (0 for a problem without rows); out:
// RG_CW results.  Grid (ceil(n / RG_TILE), ceil(cols / RG_CPB)), 256 threads.
__global__ __launch_bounds__(256) void k_range_vars(AsmBt abt, RangePoint P, const double* __restrict__ DX, const double* __restrict__ DZ, int64_t ldn, int cols, int n_row_wg, RangeRed R, RangeOut* __restrict__ out) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, P, DX, DZ, ldn, cols, n_row_wg, R, out);
    __shared__ bool last;
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * RG_TILE + lane;
    const int c0 = (int)blockIdx.y * RG_CPB + (int)(threadIdx.x >> 6) * RG_CPT;
    const bool in = j < P.n;
    const int bs = in ? P.bs[j] : 0;
    const double x = in ? P.x[j] : 0.0, lo = in ? P.x_L[j] : 0.0, up = in ? P.x_U[j] : 0.0, z = in ? P.z[j] : 0.0;
    const int64_t slot = (int64_t)n_row_wg + blockIdx.x;
#pragma unroll
    for (int q = 0; q < RG_CPT; ++q) {
        const int c = c0 + q;
        if (c >= cols) break;      // (uniform in the wavefront)
        const double dx = in ? DX[(int64_t)c * ldn + j] : 0.0, dz = in ? DZ[(int64_t)c * ldn + j] : 0.0;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const double sg = side ? 1.0 : -1.0;
            const RangeCand b = rg_wave_min(in ? rg_var(sg, (int)(P.m + j), bs, x, lo, up, z, dx, dz) : rg_none());
            if (lane == 0) rg_store(R, slot, c, side, b);
        }
    }
    // the last workgroup of this blockIdx.y to arrive (as kk_last_arrival; four lanes have stored here, each fences its own stores)
    __threadfence();
    __syncthreads();
    if (gridDim.x > 1) {
        if (threadIdx.x == 0) {
            unsigned* cnt = R.cnt + blockIdx.y;
            const unsigned t = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            last = (t == gridDim.x - 1);
            if (last) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (!last) return;
        __threadfence();
    }
    // one thread per (column, side) of this blockIdx.y: the partial candidates in workgroup order, rows first
    if (threadIdx.x >= 2 * RG_CPB) return;
    const int c = (int)blockIdx.y * RG_CPB + (int)(threadIdx.x >> 1), side = threadIdx.x & 1;
    if (c >= cols) return;
    RangeCand best = rg_none();
    const int slots = n_row_wg + (int)gridDim.x;
    for (int w = 0; w < slots; ++w) {
        const int64_t at = ((int64_t)w * RG_CW + c) * 2 + side;
        const RangeCand b{__hip_atomic_load(R.pt + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __hip_atomic_load(R.pk + 2 * at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                          __hip_atomic_load(R.pk + 2 * at + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)};
        best = rg_min(best, b);
    }
    if (side) { out[c].t_hi = best.t; out[c].pos_hi = best.pos; out[c].kind_hi = best.kind; }
    else { out[c].t_lo = 0.0 - best.t; out[c].pos_lo = best.pos; out[c].kind_lo = best.kind; }
}
