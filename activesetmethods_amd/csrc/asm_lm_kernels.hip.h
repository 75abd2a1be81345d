// Limited-memory BFGS approximation B of the Hessian of L = f - lambda' g (include/asm_hip.h, "Limited-memory Hessian"; DESIGN.md,
// "Limited-memory Hessian").  Compact form of Byrd, Nocedal and Schnabel:
//     B v = sigma v - Psi' W Psi v,   Psi = [sigma S; Y],   W = [[sigma S S', L], [L', -D]]^-1
// The store keeps the raw rows [S; Y] (P = memory rows each, pitch ld) in ring slots and folds sigma into the explicit matrix: with
// Ws = diag(sigma I, I) W diag(sigma I, I) the product is  B v = sigma v - [S; Y]' Ws [S; Y] v, so a push never rescales a stored row.
// Everything a product or a push decides from - the pair count, the ring head, sigma, the Gram entries, Ws - is in HBM; unused rows of
// [S; Y] and of Ws are zero, so every launch is sized from the memory P, never from the count.  No floating-point atomics: every sum
// has an order fixed by n, P and the lane count.
#pragma once
#include "asm_bt.hip.h"

constexpr int LM_PMAX = 32;         // ASM_LM_MAX of the header
enum { LM_COUNT = 0, LM_HEAD, LM_PUSHED, LM_SKIP_ZERO, LM_SKIP_CURV, LM_SLOT, LM_WORDS = 8 };      // the store's integer words
constexpr int LM_CHUNK = 1024;      // variables per workgroup of the reductions over n (16 per lane)
constexpr int LM_DOTWG = 64;        // most workgroups of the three dots of a new pair

struct LmStore {
    double* R;          // [S; Y]: 2 P rows of pitch ld, row slot holds s, row P + slot holds y
    double* ss;         // P x P, ss[i, j] = s_i' s_j by slot
    double* sy;         // P x P, sy[i, j] = s_i' y_j by slot
    double* W;          // Ws, 2 P x 2 P by slot (S part first)
    double* sigma;      // one double: y'y / s'y of the newest pair, 1.0 while there is none
    int* st;            // LM_WORDS words
    int64_t n, ld;
    int P, pad;
};

// the empty store's words (the buffers are cleared by fills): B = I
__global__ __launch_bounds__(64) void k_lm_clear(AsmBt abt, LmStore L) {
    ASM_BARGS(abt, L);
    if (threadIdx.x < LM_WORDS) L.st[threadIdx.x] = threadIdx.x == LM_SLOT ? -1 : 0;
    if (threadIdx.x == 0) L.sigma[0] = 1.0;
}

// asm_lm_begin: the point and the gradient of the Lagrangian where the evaluator left them, gs = df - J' lambda
__global__ __launch_bounds__(256) void k_lm_save(AsmBt abt, const double* __restrict__ x, const double* __restrict__ df, const double* __restrict__ jtl, int64_t n, double* __restrict__ xs, double* __restrict__ gs) {
    ASM_BARGS(abt, x, df, jtl, n, xs, gs);
    const int64_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    xs[j] = x[j];
    gs[j] = df[j] - jtl[j];
}
// asm_lm_end: s = x - x_prev, y = (df - J' lambda) - g_prev
__global__ __launch_bounds__(256) void k_lm_diff(AsmBt abt, const double* __restrict__ x, const double* __restrict__ df, const double* __restrict__ jtl, const double* __restrict__ xs, const double* __restrict__ gs, int64_t n, double* __restrict__ s, double* __restrict__ y) {
    ASM_BARGS(abt, x, df, jtl, xs, gs, n, s, y);
    const int64_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    s[j] = x[j] - xs[j];
    y[j] = (df[j] - jtl[j]) - gs[j];
}

// the sum of one value per thread over a workgroup of 256 in a fixed order: the butterfly of each wave, then the four waves in order
__device__ __forceinline__ double lm_block_sum(double v, double* sh4) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh4[0] + sh4[1]) + sh4[2]) + sh4[3];
}

// s's, y'y and s'y of a new pair, stage one: workgroup g sums the variables g * per .. (g + 1) * per into part[3 g ..]
__global__ __launch_bounds__(256) void k_lm_pair_dots(AsmBt abt, const double* __restrict__ s, const double* __restrict__ y, int64_t n, int64_t per, double* __restrict__ part) {
    ASM_BARGS(abt, s, y, n, per, part);
    __shared__ double sh[4];
    const int64_t j0 = blockIdx.x * per, j1 = j0 + per < n ? j0 + per : n;
    double a = 0.0, b = 0.0, c = 0.0;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) {
        const double sj = s[j], yj = y[j];
        a += sj * sj; b += yj * yj; c += sj * yj;
    }
    a = lm_block_sum(a, sh); b = lm_block_sum(b, sh); c = lm_block_sum(c, sh);
    if (threadIdx.x == 0) { part[3 * blockIdx.x] = a; part[3 * blockIdx.x + 1] = b; part[3 * blockIdx.x + 2] = c; }
}
// stage two and the skip rule: the pair is stored only if ||s|| > 0, s'y > 0 and s'y >= 1e-8 ||s|| ||y||.  A stored pair gets the slot behind the
// newest, or - the store full - the slot of the oldest, whose successor becomes the head; LM_SLOT tells the next two kernels (-1: skipped)
__global__ __launch_bounds__(64) void k_lm_pair_decide(AsmBt abt, LmStore L, const double* __restrict__ part, int nwg) {
    ASM_BARGS(abt, L, part, nwg);
    if (threadIdx.x != 0) return;
    double a = 0.0, b = 0.0, c = 0.0;
    for (int g = 0; g < nwg; ++g) { a += part[3 * g]; b += part[3 * g + 1]; c += part[3 * g + 2]; }
    int* st = L.st;
    st[LM_PUSHED] += 1;
    const double ns = sqrt(a), ny = sqrt(b);
    if (!(ns > 0.0)) { st[LM_SKIP_ZERO] += 1; st[LM_SLOT] = -1; return; }
    if (!(c > 0.0 && c >= 1e-8 * ns * ny)) { st[LM_SKIP_CURV] += 1; st[LM_SLOT] = -1; return; }      // (c > 0 too: y = 0 meets the inequality)
    const int cnt = st[LM_COUNT], head = st[LM_HEAD];
    int slot;
    if (cnt < L.P) { slot = (head + cnt) % L.P; st[LM_COUNT] = cnt + 1; }
    else { slot = head; st[LM_HEAD] = (head + 1) % L.P; }
    st[LM_SLOT] = slot;
    L.sigma[0] = b / c;
}
// the rows of the new pair
__global__ __launch_bounds__(256) void k_lm_pair_store(AsmBt abt, LmStore L, const double* __restrict__ s, const double* __restrict__ y) {
    ASM_BARGS(abt, L, s, y);
    const int slot = L.st[LM_SLOT];
    const int64_t j = blockIdx.x * 256 + threadIdx.x;
    if (slot < 0 || j >= L.n) return;
    L.R[slot * L.ld + j] = s[j];
    L.R[(L.P + slot) * L.ld + j] = y[j];
}
// the Gram entries of the new pair: workgroup i takes the dots of slot i with the new rows (which k_lm_pair_store has written: i = slot
// gives the diagonal) - s_i's, s_i'y and y_i's over n - and writes row and column `slot` of ss and sy.  An empty slot holds zeros.
__global__ __launch_bounds__(256) void k_lm_pair_gram(AsmBt abt, LmStore L) {
    ASM_BARGS(abt, L);
    __shared__ double sh[4];
    const int slot = L.st[LM_SLOT], i = blockIdx.x, P = L.P;
    if (slot < 0) return;
    const double *si = L.R + i * L.ld, *yi = L.R + (P + i) * L.ld, *sn = L.R + slot * L.ld, *yn = L.R + (P + slot) * L.ld;
    double a = 0.0, b = 0.0, c = 0.0;
    for (int64_t j = threadIdx.x; j < L.n; j += 256) {
        const double u = si[j], w = sn[j];
        a += u * w; b += u * yn[j]; c += w * yi[j];
    }
    a = lm_block_sum(a, sh); b = lm_block_sum(b, sh); c = lm_block_sum(c, sh);
    if (threadIdx.x == 0) {
        L.ss[i * P + slot] = a; L.ss[slot * P + i] = a;
        L.sy[i * P + slot] = b;      // s_i' y_new
        L.sy[slot * P + i] = c;      // s_new' y_i   (i = slot: b and c are the same sum in the same order)
    }
}

// Ws from the Gram entries, one workgroup.  Chronological index k is slot (head + k) mod P.  With A = sigma S S', L the strictly lower
// part of S Y' and D its diagonal (> 0 by the skip rule), C = A + L D^-1 L' is symmetric positive definite and
//     W = [[C^-1, G], [G', D^-1 L' G - D^-1]],  G = C^-1 L D^-1
// C = R R' by an unpivoted Cholesky, C^-1 column by column from two substitutions.  Ws scales the S rows and columns by sigma and goes
// out by slot; rows and columns of empty slots are zero.
__global__ __launch_bounds__(256) void k_lm_middle(AsmBt abt, LmStore L) {
    ASM_BARGS(abt, L);
    constexpr int Q = LM_PMAX, LDQ = Q + 1;
    __shared__ double C[Q * LDQ], Ci[Q * LDQ], Lm[Q * LDQ], G[Q * LDQ], dinv[Q];
    __shared__ int slot_of[Q];
    const int P = L.P, p = L.st[LM_COUNT], head = L.st[LM_HEAD], tid = threadIdx.x;
    const double sigma = L.sigma[0];
    for (int e = tid; e < 4 * P * P; e += 256) L.W[e] = 0.0;
    if (p == 0) return;
    if (tid < p) {
        const int sl = (head + tid) % P;
        slot_of[tid] = sl;
        dinv[tid] = 1.0 / L.sy[sl * P + sl];
    }
    __syncthreads();
    for (int e = tid; e < p * p; e += 256) {
        const int i = e / p, j = e % p;
        Lm[i * LDQ + j] = i > j ? L.sy[slot_of[i] * P + slot_of[j]] : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < p * p; e += 256) {
        const int i = e / p, j = e % p;
        double c = 0.0;
        for (int k = 0; k < p; ++k) c += Lm[i * LDQ + k] * dinv[k] * Lm[j * LDQ + k];
        C[i * LDQ + j] = sigma * L.ss[slot_of[i] * P + slot_of[j]] + c;
    }
    __syncthreads();
    // C = R R' in place (lower): column k by the first wave, one row per lane
    for (int k = 0; k < p; ++k) {
        if (tid == 0) C[k * LDQ + k] = sqrt(C[k * LDQ + k]);
        __syncthreads();
        if (tid > k && tid < p) C[tid * LDQ + k] /= C[k * LDQ + k];
        __syncthreads();
        for (int e = tid; e < p * p; e += 256) {
            const int i = e / p, j = e % p;
            if (j > k && i >= j) C[i * LDQ + j] -= C[i * LDQ + k] * C[j * LDQ + k];
        }
        __syncthreads();
    }
    // column c of C^-1: R z = e_c, R' w = z
    if (tid < p) {
        const int c = tid;
        for (int i = 0; i < p; ++i) {
            double z = i == c ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) z -= C[i * LDQ + k] * Ci[k * LDQ + c];
            Ci[i * LDQ + c] = z / C[i * LDQ + i];
        }
        for (int i = p - 1; i >= 0; --i) {
            double z = Ci[i * LDQ + c];
            for (int k = i + 1; k < p; ++k) z -= C[k * LDQ + i] * Ci[k * LDQ + c];
            Ci[i * LDQ + c] = z / C[i * LDQ + i];
        }
    }
    __syncthreads();
    for (int e = tid; e < p * p; e += 256) {
        const int i = e / p, j = e % p;
        double g = 0.0;
        for (int k = 0; k < p; ++k) g += Ci[i * LDQ + k] * Lm[k * LDQ + j];
        G[i * LDQ + j] = g * dinv[j];
    }
    __syncthreads();
    const int P2 = 2 * P;
    for (int e = tid; e < p * p; e += 256) {
        const int i = e / p, j = e % p, si = slot_of[i], sj = slot_of[j];
        double t = 0.0;
        for (int k = 0; k < p; ++k) t += Lm[k * LDQ + i] * G[k * LDQ + j];
        L.W[si * P2 + sj] = sigma * sigma * Ci[i * LDQ + j];
        L.W[si * P2 + P + sj] = sigma * G[i * LDQ + j];
        L.W[(P + sj) * P2 + si] = sigma * G[i * LDQ + j];
        L.W[(P + si) * P2 + P + sj] = dinv[i] * t - (i == j ? dinv[i] : 0.0);
    }
}

// B V for `cols` columns (rows of V, pitch ldv), stage one: T = V [S; Y]'.  Workgroup (g, b) takes the variables g * LM_CHUNK .. and
// the columns b * LM_COLS ..; wave w the rows w, w + 4, ..: a lane holds its 16 entries of the row, read once and coalesced, and uses
// them for the workgroup's columns, whose loads are in flight together.  [S; Y] comes from HBM once per launch and from L2 once per
// group of LM_COLS columns.  The partial sum of (column c, row r, workgroup g) is the lane's 16 products in order, then the butterfly:
// it depends on column c alone (no contraction: the bits do not depend on how a column's slot was scheduled).
constexpr int LM_COLS = 8;
__global__ __launch_bounds__(256) void k_lm_psi_v(AsmBt abt, LmStore L, const double* __restrict__ V, int64_t ldv, int cols, double* __restrict__ part) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, L, V, ldv, cols, part);
    constexpr int PL = LM_CHUNK / 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, P2 = 2 * L.P, nwg = gridDim.x, c0 = blockIdx.y * LM_COLS;
    const int64_t j0 = (int64_t)blockIdx.x * LM_CHUNK + lane;
    for (int r = wave; r < P2; r += 4) {
        const double* row = L.R + r * L.ld;
        double a[PL], acc[LM_COLS];
#pragma unroll
        for (int k = 0; k < PL; ++k) {
            const int64_t j = j0 + 64 * k;
            a[k] = j < L.n ? row[j] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < LM_COLS; ++q) {
            double sum = 0.0;
            if (c0 + q < cols) {
                const double* v = V + (c0 + q) * ldv;
#pragma unroll
                for (int k = 0; k < PL; ++k) {
                    const int64_t j = j0 + 64 * k;
                    sum += a[k] * (j < L.n ? v[j] : 0.0);
                }
            }
            acc[q] = sum;
        }
#pragma unroll
        for (int q = 0; q < LM_COLS; ++q) {
            if (c0 + q < cols) {      // (the same for the whole workgroup)
                const double sum = wave_sum(acc[q]);
                if (lane == 0) part[((int64_t)(c0 + q) * nwg + blockIdx.x) * P2 + r] = sum;
            }
        }
    }
}
// stage two: OUT = sigma V - (T Ws) [S; Y].  A thread owns one variable and holds its column of [S; Y] in registers, read once.  The
// columns of V go in groups of LM_GROUP: the workgroup sums the group's partials in workgroup order (t, one (column, row) per thread
// and pass), forms u = Ws t in LDS (Ws staged there once), and every thread subtracts sum_r R[r, j] u[r], r ascending, from sigma v[j] for each column of the
// group.  A column's arithmetic does not depend on its group.
constexpr int LM_GROUP = 16;
__global__ __launch_bounds__(256) void k_lm_apply(AsmBt abt, LmStore L, const double* __restrict__ V, int64_t ldv, int cols, const double* __restrict__ part, int nwg, double* __restrict__ OUT, int64_t ldo) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, L, V, ldv, cols, part, nwg, OUT, ldo);
    constexpr int Q2 = 2 * LM_PMAX;
    __shared__ double t[LM_GROUP * Q2], u[LM_GROUP * Q2], Wl[Q2 * (Q2 + 1)];
    const int P2 = 2 * L.P, ldw = P2 | 1, tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * 256 + tid;
    const bool in = j < L.n;
    const double sigma = L.sigma[0];
    for (int e = tid; e < P2 * P2; e += 256) Wl[(e / P2) * ldw + e % P2] = L.W[e];      // (the first barrier of the loop orders it)
    double col[Q2];
#pragma unroll
    for (int r = 0; r < Q2; ++r) col[r] = (r < P2 && in) ? L.R[r * L.ld + j] : 0.0;
    for (int c0 = 0; c0 < cols; c0 += LM_GROUP) {
        const int nc = cols - c0 < LM_GROUP ? cols - c0 : LM_GROUP;
        __syncthreads();      // (the last group's u has been read)
        for (int e = tid; e < nc * P2; e += 256) {
            const int q = e / P2, r = e % P2;
            double a = 0.0;
            for (int g = 0; g < nwg; ++g) a += part[((int64_t)(c0 + q) * nwg + g) * P2 + r];
            t[q * Q2 + r] = a;
        }
        __syncthreads();
        for (int e = tid; e < nc * P2; e += 256) {
            const int q = e / P2, r = e % P2;
            double a = 0.0;
            for (int k = 0; k < P2; ++k) a += Wl[r * ldw + k] * t[q * Q2 + k];
            u[q * Q2 + r] = a;
        }
        __syncthreads();
        if (in) {
            for (int q = 0; q < nc; ++q) {
                double a = 0.0;
#pragma unroll
                for (int r = 0; r < Q2; ++r)
                    if (r < P2) a += col[r] * u[q * Q2 + r];
                OUT[(c0 + q) * ldo + j] = sigma * V[(c0 + q) * ldv + j] - a;
            }
        }
    }
}
