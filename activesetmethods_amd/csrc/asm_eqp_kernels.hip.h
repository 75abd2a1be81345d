// Kernels of the SLP-EQP trial step (asm_eqp_trial; include/asm_hip.h, "SLP-EQP"): the working set an LP's active set names at the
// evaluator's point, and the step that stays inside the variable bounds.  The trust-region step between the two is asm_kkt_step's driver
// and kernels (asm_kkt_kernels.hip.h), the merit values are k_slp_tr_quality's (asm_eval_kernels.hip.h).
// Both kernels read x, E and the bounds where the evaluator keeps them in HBM.  Counts and sums follow the rule of the KKT kernels: every
// workgroup stores its partial values with agent-scope stores and counts itself in, the last one to arrive adds them in workgroup order -
// a fixed order, no atomics on doubles.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "asm_bt.hip.h"
#include "asm_kkt_kernels.hip.h"

struct EqpFace {
    const double *E, *g_L, *g_U, *x, *x_L, *x_U;      // the evaluator's results and the problem's bounds (m, m, m, n, n, n)
    const int* lp_rows;      // the LP's row_state, m + n_adj: rows m.. are the `<=` twins of the range rows
    const int* lp_bnd;       // the LP's bound_state, n
    const int* twin;         // m: the place of a row's twin among rows m.., -1 for a row without one
    int64_t n, m;
    double tol;
};
enum { EQP_NW = 0, EQP_NF, EQP_COUNTS };
// The face: rows[i] = 1 for an equality, a row the LP holds active and a row whose twin is active; side[i] = -1 where such a row sits at
// g_L (an equality; a row without an active twin whose g_L is finite), +1 at g_U, 0 outside W; rw[i] = E[i] - that bound, 0 outside W.
// bnd[j] = -1 / +1 where the LP reports the variable at that bound and x[j] is within tol (1 + |bound|) of the problem's finite bound on
// that side, else 0.  counts = { |W|, |F| }.  Grid-stride over max(m, n), at most KK_MAXWG workgroups.
__global__ __launch_bounds__(256) void k_eqp_face(AsmBt abt, EqpFace P, KktRed R, int* __restrict__ rows, int* __restrict__ bnd, int* __restrict__ side, double* __restrict__ rw, int* __restrict__ counts) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, P, R, rows, bnd, side, rw, counts);
    __shared__ double sh[4];
    __shared__ bool last;
    const int64_t stride = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double nw = 0.0, nf = 0.0;
    for (int64_t i = first; i < P.m; i += stride) {
        const double lo = P.g_L[i], up = P.g_U[i];
        const int tw = P.twin[i];
        const bool eq = lo == up, twin_on = tw >= 0 && P.lp_rows[P.m + tw] != 0;
        const bool in = eq || P.lp_rows[i] != 0 || twin_on;
        const bool upper = !eq && (twin_on || !(lo > -INFINITY));
        rows[i] = in ? 1 : 0;
        side[i] = in ? (upper ? 1 : -1) : 0;
        rw[i] = in ? P.E[i] - (upper ? up : lo) : 0.0;
        nw += in ? 1.0 : 0.0;
    }
    for (int64_t j = first; j < P.n; j += stride) {
        const double xj = P.x[j], lo = P.x_L[j], up = P.x_U[j];
        const int s = P.lp_bnd[j];
        int b = 0;
        if (s == -1 && lo > -INFINITY && fabs(xj - lo) <= P.tol * (1.0 + fabs(lo))) b = -1;
        else if (s == 1 && up < INFINITY && fabs(xj - up) <= P.tol * (1.0 + fabs(up))) b = 1;
        bnd[j] = b;
        nf += b == 0 ? 1.0 : 0.0;
    }
    nw = blk_reduce_sum(nw, sh);          // (counts below 2^53: exact in any order)
    nf = blk_reduce_sum(nf, sh);
    if (gridDim.x > 1) {
        if (threadIdx.x == 0) { kk_store(R, 0, nw); kk_store(R, 1, nf); }
        if (!kk_last_arrival(R, &last)) return;
        if (threadIdx.x == 0) { nw = kk_total(R, 0); nf = kk_total(R, 1); }
    }
    if (threadIdx.x == 0) { counts[EQP_NW] = (int)nw; counts[EQP_NF] = (int)nf; }
}

enum { EQP_T = 0, EQP_NORM2, EQP_NORMINF, EQP_NONZERO, EQP_SCAL };
// The trial step: t = the largest value in [0, 1] with x_L <= x + t dx <= x_U (eqp.fraction_to_box: the minimum of (x_U - x) / dx over
// dx > 0 and of (x_L - x) / dx over dx < 0, not above 1, not below 0), d = t dx, and out = { t, ||d||_2, ||d||_inf, the number of
// components of d that are not zero }.  Every workgroup forms t itself from all n components - a minimum has one value in any order -
// and then writes its share of d: one launch, no wait between workgroups.  The price is that G = min(ceil(n / 256), KK_MAXWG) workgroups
// each read 32 n bytes: n^2 / 8 bytes in all up to n = 16 384, 2 048 n beyond.  Against a second launch this has not been measured; by
// the arithmetic (a few microseconds per launch, terabytes per second out of the L2) it should hold to n of some ten thousands - the
// models run so far have n <= 2 400 - and a two-launch form is the one to write when a model comes with n far beyond that.
__global__ __launch_bounds__(256) void k_eqp_trial(AsmBt abt, const double* __restrict__ dx, const double* __restrict__ x, const double* __restrict__ x_L, const double* __restrict__ x_U, int64_t n, KktRed R, double* __restrict__ d, double* __restrict__ out) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, dx, x, x_L, x_U, n, R, d, out);
    __shared__ double sh[4];
    __shared__ bool last;
    double t = 1.0;
    for (int64_t j = threadIdx.x; j < n; j += 256) {
        const double v = dx[j];
        if (v > 0.0) t = fmin(t, (x_U[j] - x[j]) / v);
        else if (v < 0.0) t = fmin(t, (x_L[j] - x[j]) / v);
    }
    t = fmax(blk_reduce_min(t, sh), 0.0);
    double sq = 0.0, mx = 0.0, nz = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
        const double v = t * dx[j];
        d[j] = v;
        sq += v * v;
        mx = fmax(mx, fabs(v));
        nz += v != 0.0 ? 1.0 : 0.0;
    }
    sq = blk_reduce_sum(sq, sh);
    nz = blk_reduce_sum(nz, sh);
    mx = blk_reduce_max(mx, sh);
    if (gridDim.x > 1) {
        if (threadIdx.x == 0) { kk_store(R, 0, sq); kk_store(R, 1, nz); kk_store(R, 2, mx); }
        if (!kk_last_arrival(R, &last)) return;
        if (threadIdx.x == 0) {
            sq = kk_total(R, 0);
            nz = kk_total(R, 1);
            mx = 0.0;
            for (int w = 0; w < (int)gridDim.x; ++w) mx = fmax(mx, __hip_atomic_load(R.part + (int64_t)w * KK_SLOTS + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
    }
    if (threadIdx.x == 0) { out[EQP_T] = t; out[EQP_NORM2] = sqrt(sq); out[EQP_NORMINF] = mx; out[EQP_NONZERO] = nz; }
}
