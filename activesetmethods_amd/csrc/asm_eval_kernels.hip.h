// Device-side evaluation of the functions the SLP hot path consumes (eval_functions!, src/algorithms/slp.jl:186-191):
//   * the affine / quadratic evaluator of the MOI wrapper (src/MOI_wrapper.jl:776-944) on a flattened function store -
//     term by term in the reference's order, with explicit round-to-nearest multiplies and adds (no fused multiply-add),
//     so that values, gradient and Jacobian entries are BIT-IDENTICAL to the host restatement
//     (activesetmethods_amd/moi_evaluator.py);
//   * two NLP-block kernels: Ohm's-law rows of the polar ACOPF model (test/opf.jl:6-10) and the dense quadratic rows of the
//     synthetic NLP of BASELINE.json configs[1]; and the kernels of a general expression block (a tape of the reference's
//     @NLconstraint / @NLobjective expressions, reverse-mode derivatives);
//   * the per-iteration reductions of the SLP callers (KT_residuals, norm_violations, norm_complementarity: common.jl:35-98;
//     compute_phi, compute_derivative: slp.jl:79-147) on the evaluation results already in HBM.
// Jacobian values are written straight into the handle's `dE` buffer in j_str order: they never cross PCIe.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/asm_hip.h"

struct FnStore {
    int64_t n_rows, n;
    const int64_t *aff_ptr, *aff_var, *quad_ptr, *q_v1, *q_v2, *jac_off, *g_ptr, *g_kind, *g_other;
    const double *aff_coef, *q_coef, *constant, *g_coef;
    double objective_scale;
};

// eval_function (MOI_wrapper.jl:780-807) of row r
// (`#pragma clang fp contract(off)` + plain operators: hipcc would otherwise fuse a * b + c into one fma - one rounding instead
// of the reference's two; the __dmul_rn / __dadd_rn spellings do not prevent that, their bodies are inlined with contraction on)
__device__ __forceinline__ double fn_value(const FnStore& F, int64_t r, const double* __restrict__ x) {
#pragma clang fp contract(off)
    double v = F.constant[r];
    for (int64_t k = F.aff_ptr[r]; k < F.aff_ptr[r + 1]; ++k) { const double t = F.aff_coef[k] * x[F.aff_var[k]]; v = v + t; }
    for (int64_t k = F.quad_ptr[r]; k < F.quad_ptr[r + 1]; ++k) {
        const int64_t a = F.q_v1[k], b = F.q_v2[k];
        const double c = F.q_coef[k];
        const double t = a == b ? ((0.5 * c) * x[a]) * x[b] : (c * x[a]) * x[b];
        v = v + t;
    }
    return v;
}
// eval_constraint + eval_constraint_jacobian of the affine / quadratic rows (MOI_wrapper.jl:875-944): one thread per row
// (blockIdx.y = trial point of a batched line search: x and E advance by ldx / ldE per trial; the Jacobian is only written for one point)
__global__ __launch_bounds__(256) void k_fn_rows(AsmBt abt, FnStore F, const double* __restrict__ x, double* __restrict__ E, double* __restrict__ dE, int write_jac, int64_t ldx, int64_t ldE) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, F, x, E, dE, write_jac, ldx, ldE);
    int64_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= F.n_rows) return;
    x += blockIdx.y * ldx;
    E += blockIdx.y * ldE;
    E[r] = fn_value(F, r, x);
    if (!write_jac) return;
    int64_t o = F.jac_off[r];
    for (int64_t k = F.aff_ptr[r]; k < F.aff_ptr[r + 1]; ++k) dE[o++] = F.aff_coef[k];
    for (int64_t k = F.quad_ptr[r]; k < F.quad_ptr[r + 1]; ++k) {
        const int64_t a = F.q_v1[k], b = F.q_v2[k];
        const double c = F.q_coef[k];
        dE[o++] = c * x[b];
        if (a != b) dE[o++] = c * x[a];
    }
}
// eval_objective (one thread: the sum is sequential in the reference) and its sense scale (MOI_wrapper.jl:1046-1049)
// (blockIdx.x = trial point.)  The terms are formed by all threads - each behind two or three dependent loads, which one thread walking the
// list pays one after the other: 226 us for the 2 000 terms of the dense synthetic objective - and ADDED by one thread in list order, so the
// sum is the reference's, bit for bit.
__global__ __launch_bounds__(256) void k_fn_objective(AsmBt abt, FnStore F, const double* __restrict__ x, double* __restrict__ f_out, int64_t ldx) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, F, x, f_out, ldx);
    __shared__ double term[1024];
    x += blockIdx.x * ldx;
    const int64_t r = F.n_rows;
    const int64_t a0 = F.aff_ptr[r], na = F.aff_ptr[r + 1] - a0, q0 = F.quad_ptr[r], nq = F.quad_ptr[r + 1] - q0;
    double v = F.constant[r];
    for (int64_t base = 0; base < na + nq; base += 1024) {
        for (int64_t e = base + threadIdx.x; e < min(base + (int64_t)1024, na + nq); e += 256) {
            double t;
            if (e < na) {
                const int64_t k = a0 + e;
                t = F.aff_coef[k] * x[F.aff_var[k]];
            } else {
                const int64_t k = q0 + (e - na);
                const int64_t a = F.q_v1[k], b = F.q_v2[k];
                const double c = F.q_coef[k];
                t = a == b ? ((0.5 * c) * x[a]) * x[b] : (c * x[a]) * x[b];
            }
            term[e - base] = t;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int64_t e = base; e < min(base + (int64_t)1024, na + nq); ++e) v = v + term[e - base];
        __syncthreads();
    }
    if (threadIdx.x == 0) f_out[blockIdx.x] = F.objective_scale * v;
}
// fill_gradient! (MOI_wrapper.jl:827-850): one thread per variable sums its contributions in term order
__global__ __launch_bounds__(256) void k_fn_gradient(AsmBt abt, FnStore F, const double* __restrict__ x, double* __restrict__ df) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, F, x, df);
    int64_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= F.n) return;
    double g = 0.0;
    for (int64_t k = F.g_ptr[j]; k < F.g_ptr[j + 1]; ++k)
        { const double t = F.g_kind[k] == 0 ? F.g_coef[k] : F.g_coef[k] * x[F.g_other[k]]; g = g + t; }
    df[j] = g * F.objective_scale;
}

// ---- NLP block 1: Ohm's law of the polar ACOPF (activesetmethods_amd/acopf.py: _flows, eval_g, eval_jac_g).
// ipar: [nl, va0, vm0, pf0, pt0, qf0, qt0, then f_bus[nl], t_bus[nl]] ; dpar: 10 coefficient arrays of length nl
// (k_ff_p, k_ff_q, k_tt_p, k_tt_q, a_f, b_f, a_t, b_t).  Rows: pfr, qfr, pto, qto (nl each) from row r0; Jacobian values from
// j0 in 4 groups x 5 sub-blocks of nl (d/d flow variable, vm_f, vm_t, va_f, va_t).
__global__ __launch_bounds__(256) void k_nlp_acopf_ohm(AsmBt abt, const int64_t* __restrict__ ipar, const double* __restrict__ dpar, const double* __restrict__ x, double* __restrict__ E, double* __restrict__ dE, int64_t r0, int64_t j0, int write_jac, int64_t ldx, int64_t ldE) {
    ASM_BARGS(abt, ipar, dpar, x, E, dE, r0, j0, write_jac, ldx, ldE);
    const int64_t nl = ipar[0];
    int64_t l = blockIdx.x * 256 + threadIdx.x;
    if (l >= nl) return;
    x += blockIdx.y * ldx;
    E += blockIdx.y * ldE;
    const int64_t va0 = ipar[1], vm0 = ipar[2], pf0 = ipar[3], pt0 = ipar[4], qf0 = ipar[5], qt0 = ipar[6];
    const int64_t fb = ipar[7 + l], tb = ipar[7 + nl + l];
    const double kffp = dpar[l], kffq = dpar[nl + l], kttp = dpar[2 * nl + l], kttq = dpar[3 * nl + l];
    const double af = dpar[4 * nl + l], bf = dpar[5 * nl + l], at = dpar[6 * nl + l], bt = dpar[7 * nl + l];
    const double vf = x[vm0 + fb], vt = x[vm0 + tb];
    const double d = x[va0 + fb] - x[va0 + tb];
    const double cs = cos(d), sn = sin(d);
    const double vv = vf * vt;
    const double pfr = kffp * vf * vf + af * vv * cs + bf * vv * sn;
    const double qfr = kffq * vf * vf - bf * vv * cs + af * vv * sn;
    const double pto = kttp * vt * vt + at * vv * cs - bt * vv * sn;
    const double qto = kttq * vt * vt - bt * vv * cs - at * vv * sn;
    E[r0 + l] = x[pf0 + l] - pfr;
    E[r0 + nl + l] = x[qf0 + l] - qfr;
    E[r0 + 2 * nl + l] = x[pt0 + l] - pto;
    E[r0 + 3 * nl + l] = x[qt0 + l] - qto;
    if (!write_jac) return;
    const double dvf[4] = {2 * kffp * vf + af * vt * cs + bf * vt * sn, 2 * kffq * vf - bf * vt * cs + af * vt * sn,
                           at * vt * cs - bt * vt * sn, -bt * vt * cs - at * vt * sn};
    const double dvt[4] = {af * vf * cs + bf * vf * sn, -bf * vf * cs + af * vf * sn, 2 * kttp * vt + at * vf * cs - bt * vf * sn,
                           2 * kttq * vt - bt * vf * cs - at * vf * sn};
    const double dth[4] = {-af * vv * sn + bf * vv * cs, bf * vv * sn + af * vv * cs, -at * vv * sn - bt * vv * cs, bt * vv * sn - at * vv * cs};
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        double* o = dE + j0 + (int64_t)g * 5 * nl + l;
        o[0] = 1.0;
        o[nl] = -dvf[g];
        o[2 * nl] = -dvt[g];
        o[3 * nl] = -dth[g];
        o[4 * nl] = dth[g];
    }
}
// ---- NLP block 2: dense quadratic rows  g_i = sum_j A_ij x_j + 1/2 Q_ij x_j^2 ,  J_ij = A_ij + Q_ij x_j  (row-major pattern).
// dpar: A (m x n) then Q (m x n); one wavefront per row.
__global__ __launch_bounds__(256) void k_nlp_dense_quadratic(AsmBt abt, const double* __restrict__ dpar, int64_t mrows, int64_t n, const double* __restrict__ x, double* __restrict__ E, double* __restrict__ dE, int64_t r0, int64_t j0, int write_jac, int64_t ldx, int64_t ldE) {
    ASM_BARGS(abt, dpar, mrows, n, x, E, dE, r0, j0, write_jac, ldx, ldE);
    int64_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= mrows) return;
    x += blockIdx.y * ldx;
    E += blockIdx.y * ldE;
    const int lane = threadIdx.x & 63;
    const double* Ar = dpar + i * n;
    const double* Qr = dpar + mrows * n + i * n;
    double acc = 0.0;
    for (int64_t j = lane; j < n; j += 64) {
        const double xj = x[j], a = Ar[j], q = Qr[j];
        acc += a * xj + 0.5 * q * xj * xj;
        if (write_jac) dE[j0 + i * n + j] = a + q * xj;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) E[r0 + i] = acc;
}

// ---- NLP block 3: expression tape (include/asm_hip.h, "Expression block").  Rows 0..R-1 are constraint rows, R..R+T-1 objective terms.
// Set up by asm_eval_setup: node references a / b made absolute (index into the whole tape), VAR nodes of a row carry the offset of
// their Jacobian value from j0 in `slot`, VAR nodes of a term the position of their adjoint in the per-variable gradient list, CONST nodes
// their place in the per-dpar occurrence list of the data gradient.
// The node values live in HBM (val: 8 trial points x L) - a runtime-indexed per-thread array would spill to scratch; adj: L adjoints
// (one point: the Jacobian and the gradient are only formed at the iterate).
struct ExprTape {
    const int64_t *ptr, *jptr, *a, *b, *slot, *gptr;   // ptr [R+T+1], jptr [R+1] (row Jacobian ranges from j0), gptr [n+1]
    const int32_t* op;
    const double* cst;
    double *val, *adj, *tval, *gocc;                   // tval [8 x T] term values, gocc [gptr[n]] term adjoints of the VAR nodes
    int64_t R, T, L, n;
};
// u ^ e (e != 0): |e| - 1 products left to right, then one more; 1 / u^|e| for e < 0.  *d = d/du, with the same factors.
__device__ __forceinline__ double expr_powi(double u, int64_t e, double* d) {
#pragma clang fp contract(off)
    const int64_t k = e < 0 ? -e : e;
    double p = 1.0;
    for (int64_t i = 1; i < k; ++i) p = p * u;
    const double pk = p * u;
    if (e > 0) { *d = (double)e * p; return pk; }
    *d = (double)e / (pk * u);
    return 1.0 / pk;
}
// ln 10 and ln 2 rounded to double (the adjoints of LOG10 / LOG2; the host twin uses the same two values)
constexpr double EXPR_LN10 = 2.302585092994045684, EXPR_LN2 = 0.6931471805599453094;
// The math-library ops after COS, out of line: inlined into the node loops, their polynomial constants are hoisted out of the
// loop and held in registers across it (256 VGPRs, occupancy 2, against 98 and 4 with the call).  y: b's value (POW, ATAN2).
__device__ __noinline__ double expr_libm(int32_t op, double u, double y) {
    switch (op) {
        case ASM_OP_TAN: return tan(u);
        case ASM_OP_ASIN: return asin(u);
        case ASM_OP_ACOS: return acos(u);
        case ASM_OP_ATAN: return atan(u);
        case ASM_OP_SINH: return sinh(u);
        case ASM_OP_COSH: return cosh(u);
        case ASM_OP_TANH: return tanh(u);
        case ASM_OP_LOG10: return log10(u);
        case ASM_OP_LOG2: return log2(u);
        case ASM_OP_LOG1P: return log1p(u);
        case ASM_OP_EXPM1: return expm1(u);
        case ASM_OP_CBRT: return cbrt(u);
        case ASM_OP_POW: return pow(u, y);
        default: return atan2(u, y);      // ASM_OP_ATAN2
    }
}
// ATAN2's adjoints (w y) / t and (w u) / t, t = u u + y y, with u and y scaled by a power of two s first: us = u s and ys = y s have their
// larger magnitude in [1/2, 1), so ts = us us + ys ys neither underflows nor overflows where the quotients are representable (at
// (1e-200, 1e-200) u u is 0 and the plain form returns inf for 5e199).  A power of two scales exactly: q(w, ys) = ((w ys) / ts) s has the bits
// of (w y) / t wherever that form neither underflows nor overflows.  The exponent is kept within +-1000 so that s itself is a normal number.
struct ExprAtan2 {
    double s, us, ys, ts;
    __device__ __forceinline__ ExprAtan2(double u, double y) {
#pragma clang fp contract(off)
        int e;
        (void)frexp(fmax(fabs(u), fabs(y)), &e);
        s = ldexp(1.0, e < -1000 ? 1000 : (e > 1000 ? -1000 : -e));
        us = u * s; ys = y * s;
        ts = us * us + ys * ys;
    }
    __device__ __forceinline__ double q(double w, double vs) const {
#pragma clang fp contract(off)
        return ((w * vs) / ts) * s;
    }
};
// forward sweep over nodes [k0, k1) at x: every node value into val (absolute indices), returns the last one
__device__ __forceinline__ double expr_forward(const ExprTape& X, int64_t k0, int64_t k1, const double* __restrict__ x, double* val) {
#pragma clang fp contract(off)
    double v = 0.0;
    for (int64_t k = k0; k < k1; ++k) {
        const int64_t a = X.a[k], b = X.b[k];
        switch (X.op[k]) {
            case ASM_OP_CONST: v = X.cst[a]; break;
            case ASM_OP_VAR: v = x[a]; break;
            case ASM_OP_ADD: v = val[a] + val[b]; break;
            case ASM_OP_SUB: v = val[a] - val[b]; break;
            case ASM_OP_MUL: v = val[a] * val[b]; break;
            case ASM_OP_DIV: v = val[a] / val[b]; break;
            case ASM_OP_NEG: v = -val[a]; break;
            case ASM_OP_POWI: { double d; v = expr_powi(val[a], b, &d); break; }
            case ASM_OP_SQRT: v = sqrt(val[a]); break;
            case ASM_OP_EXP: v = exp(val[a]); break;
            case ASM_OP_LOG: v = log(val[a]); break;
            case ASM_OP_SIN: v = sin(val[a]); break;
            case ASM_OP_COS: v = cos(val[a]); break;
            case ASM_OP_ABS: v = fabs(val[a]); break;
            case ASM_OP_TAN: case ASM_OP_ASIN: case ASM_OP_ACOS: case ASM_OP_ATAN: case ASM_OP_SINH: case ASM_OP_COSH: case ASM_OP_TANH:
            case ASM_OP_LOG10: case ASM_OP_LOG2: case ASM_OP_LOG1P: case ASM_OP_EXPM1: case ASM_OP_CBRT: case ASM_OP_POW: case ASM_OP_ATAN2:
                v = expr_libm(X.op[k], val[a], val[b]);
                break;
            case ASM_OP_MIN: { const double u = val[a], y = val[b]; v = y < u ? y : u; break; }
            default: { const double u = val[a], y = val[b]; v = y > u ? y : u; break; }   // ASM_OP_MAX (asm_eval_setup admits no other op)
        }
        val[k] = v;
    }
    return v;
}
// what a reverse sweep writes: EXPR_JAC the adjoint of every VAR node added to out[slot] (constraint rows, several VAR nodes may share a
// Jacobian value); EXPR_GRAD the adjoint of every VAR node stored to out[slot] (term occurrences); EXPR_DATA wt * the adjoint of every CONST
// node stored to out[slot] (data-gradient occurrences), nothing for the VAR nodes
enum { EXPR_JAC = 0, EXPR_GRAD = 1, EXPR_DATA = 2 };
// reverse sweep over nodes [k0, k1) (values from the forward sweep in val): adjoints into adj, the node adjoints MODE names to out
template <int MODE>
__device__ __forceinline__ void expr_reverse(const ExprTape& X, int64_t k0, int64_t k1, const double* val, double* adj, double* out, double wt = 0.0) {
#pragma clang fp contract(off)
    for (int64_t k = k0; k < k1 - 1; ++k) adj[k] = 0.0;
    adj[k1 - 1] = 1.0;
    for (int64_t k = k1 - 1; k >= k0; --k) {
        const double w = adj[k];
        const int64_t a = X.a[k], b = X.b[k];
        switch (X.op[k]) {
            case ASM_OP_CONST:
                if constexpr (MODE == EXPR_DATA) out[X.slot[k]] = wt * w;
                break;
            case ASM_OP_VAR:
                if constexpr (MODE == EXPR_JAC) out[X.slot[k]] = out[X.slot[k]] + w;
                else if constexpr (MODE == EXPR_GRAD) out[X.slot[k]] = w;
                break;
            case ASM_OP_ADD: adj[a] = adj[a] + w; adj[b] = adj[b] + w; break;
            case ASM_OP_SUB: adj[a] = adj[a] + w; adj[b] = adj[b] - w; break;
            case ASM_OP_MUL: { const double va = val[a], vb = val[b]; adj[a] = adj[a] + w * vb; adj[b] = adj[b] + w * va; break; }
            case ASM_OP_DIV: { const double t = w / val[b]; adj[a] = adj[a] + t; adj[b] = adj[b] - t * val[k]; break; }
            case ASM_OP_NEG: adj[a] = adj[a] - w; break;
            case ASM_OP_POWI: { double d; (void)expr_powi(val[a], b, &d); adj[a] = adj[a] + w * d; break; }
            case ASM_OP_SQRT: adj[a] = adj[a] + (0.5 * w) / val[k]; break;
            case ASM_OP_EXP: adj[a] = adj[a] + w * val[k]; break;
            case ASM_OP_LOG: adj[a] = adj[a] + w / val[a]; break;
            case ASM_OP_SIN: adj[a] = adj[a] + w * cos(val[a]); break;
            case ASM_OP_COS: adj[a] = adj[a] - w * sin(val[a]); break;
            case ASM_OP_ABS: adj[a] = adj[a] + w * copysign(1.0, val[a]); break;
            case ASM_OP_TAN: { const double v = val[k]; adj[a] = adj[a] + w * (1.0 + v * v); break; }
            case ASM_OP_ASIN: { const double u = val[a]; adj[a] = adj[a] + w / sqrt((1.0 - u) * (1.0 + u)); break; }
            case ASM_OP_ACOS: { const double u = val[a]; adj[a] = adj[a] - w / sqrt((1.0 - u) * (1.0 + u)); break; }
            case ASM_OP_ATAN: { const double u = val[a]; adj[a] = adj[a] + w / (1.0 + u * u); break; }
            case ASM_OP_SINH: adj[a] = adj[a] + w * expr_libm(ASM_OP_COSH, val[a], 0.0); break;
            case ASM_OP_COSH: adj[a] = adj[a] + w * expr_libm(ASM_OP_SINH, val[a], 0.0); break;
            case ASM_OP_TANH: { const double v = val[k]; adj[a] = adj[a] + w * (1.0 - v * v); break; }
            case ASM_OP_LOG10: adj[a] = adj[a] + w / (val[a] * EXPR_LN10); break;
            case ASM_OP_LOG2: adj[a] = adj[a] + w / (val[a] * EXPR_LN2); break;
            case ASM_OP_LOG1P: adj[a] = adj[a] + w / (1.0 + val[a]); break;
            case ASM_OP_EXPM1: adj[a] = adj[a] + w * (val[k] + 1.0); break;
            case ASM_OP_CBRT: { const double v = val[k]; adj[a] = adj[a] + w / (3.0 * (v * v)); break; }
            case ASM_OP_POW: {
                const double u = val[a], y = val[b];
                adj[a] = adj[a] + w * (y * expr_libm(ASM_OP_POW, u, y - 1.0));
                adj[b] = adj[b] + w * (val[k] * log(u));
                break;
            }
            case ASM_OP_ATAN2: {
                const ExprAtan2 S(val[a], val[b]);
                adj[a] = adj[a] + S.q(w, S.ys);
                adj[b] = adj[b] - S.q(w, S.us);
                break;
            }
            case ASM_OP_MIN: { const int64_t c = val[b] < val[a] ? b : a; adj[c] = adj[c] + w; break; }
            default: { const int64_t c = val[b] > val[a] ? b : a; adj[c] = adj[c] + w; break; }   // ASM_OP_MAX
        }
    }
}
// constraint rows: one thread per row; E at r0 + row, Jacobian values at j0 + jptr[row].. (blockIdx.y = trial point, as k_fn_rows)
__global__ __launch_bounds__(256) void k_nlp_expr_rows(AsmBt abt, ExprTape X, const double* __restrict__ x, double* __restrict__ E, double* __restrict__ dE, int64_t r0, int64_t j0, int write_jac, int64_t ldx, int64_t ldE) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, X, x, E, dE, r0, j0, write_jac, ldx, ldE);
    const int64_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= X.R) return;
    x += blockIdx.y * ldx;
    E += blockIdx.y * ldE;
    double* val = X.val + blockIdx.y * X.L;
    const int64_t k0 = X.ptr[r], k1 = X.ptr[r + 1];
    E[r0 + r] = expr_forward(X, k0, k1, x, val);
    if (!write_jac || blockIdx.y) return;
    double* o = dE + j0;
    for (int64_t j = X.jptr[r]; j < X.jptr[r + 1]; ++j) o[j] = 0.0;
    expr_reverse<EXPR_JAC>(X, k0, k1, val, X.adj, o);
}
// objective terms: one thread per term; its value to tval[trial * T + term], with write_grad (one point) its VAR-node adjoints to gocc
__global__ __launch_bounds__(256) void k_nlp_expr_terms(AsmBt abt, ExprTape X, const double* __restrict__ x, int write_grad, int64_t ldx) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, X, x, write_grad, ldx);
    const int64_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= X.T) return;
    x += blockIdx.y * ldx;
    double* val = X.val + blockIdx.y * X.L;
    const int64_t k0 = X.ptr[X.R + t], k1 = X.ptr[X.R + t + 1];
    X.tval[blockIdx.y * X.T + t] = expr_forward(X, k0, k1, x, val);
    if (!write_grad || blockIdx.y) return;
    expr_reverse<EXPR_GRAD>(X, k0, k1, val, X.adj, X.gocc);
}
// the objective: one thread sums the term values in term order and applies the sense scale (as k_fn_objective); blockIdx.x = trial point
__global__ __launch_bounds__(64) void k_nlp_expr_objective(AsmBt abt, ExprTape X, double scale, double* __restrict__ f_out) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, X, scale, f_out);
    if (threadIdx.x) return;
    const double* tv = X.tval + blockIdx.x * X.T;
    double v = 0.0;
    for (int64_t t = 0; t < X.T; ++t) v = v + tv[t];
    f_out[blockIdx.x] = scale * v;
}
// the objective gradient: one thread per variable gathers its term adjoints in (term, node) order (as k_fn_gradient)
__global__ __launch_bounds__(256) void k_nlp_expr_gradient(AsmBt abt, ExprTape X, double scale, double* __restrict__ df) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, X, scale, df);
    const int64_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= X.n) return;
    double g = 0.0;
    for (int64_t o = X.gptr[j]; o < X.gptr[j + 1]; ++o) g = g + X.gocc[o];
    df[j] = g * scale;
}
// ---- data gradient of the Lagrangian (asm_eval_data_gradient): out[c] = d f / d dpar[c] - sum_r lam_r d g_r / d dpar[c].  The CONST nodes
// are grouped by dpar index in cptr [n_dpar+1]; a CONST node's `slot` is its place in that list (node order inside a group), cocc the list.
// Step 1: one thread per row (t < R) or term: forward sweep at x, reverse sweep with unit seed, and every CONST adjoint times the row's
// weight -lam[t] (lam: the multipliers of the block's rows) or the objective's sense scale into cocc.  No Jacobian or gradient output.
__global__ __launch_bounds__(256) void k_nlp_expr_const_adj(AsmBt abt, ExprTape X, const double* __restrict__ x, const double* __restrict__ lam, double scale, double* __restrict__ cocc) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, X, x, lam, scale, cocc);
    const int64_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= X.R + X.T) return;
    const int64_t k0 = X.ptr[t], k1 = X.ptr[t + 1];
    (void)expr_forward(X, k0, k1, x, X.val);
    expr_reverse<EXPR_DATA>(X, k0, k1, X.val, X.adj, cocc, t < X.R ? -lam[t] : scale);
}
// Step 2: one thread per dpar index sums its weighted occurrences in list order from 0.0 (fixed order, no atomics: the host twin's sum)
__global__ __launch_bounds__(256) void k_nlp_expr_data_gather(AsmBt abt, const int64_t* __restrict__ cptr, const double* __restrict__ cocc, int64_t n_dpar, double* __restrict__ out) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, cptr, cocc, n_dpar, out);
    const int64_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_dpar) return;
    double g = 0.0;
    for (int64_t o = cptr[c]; o < cptr[c + 1]; ++o) g = g + cocc[o];
    out[c] = g;
}

// ---- Hessian of the Lagrangian (asm_eval_hessian_*; include/asm_hip.h, "Hessian of the Lagrangian").
// Function store: one thread per pattern entry = one stored quadratic term; value = factor * q_coef (fill_hessian_lagrangian!,
// MOI_wrapper.jl:946-958), factor = wobj (obj_factor * objective_scale) for a term of the objective row (row < 0), else lambda[row].
__global__ __launch_bounds__(256) void k_fn_hessian(AsmBt abt, const int64_t* __restrict__ hq_term, const int64_t* __restrict__ hq_row, const double* __restrict__ q_coef, const double* __restrict__ lam, double wobj, int64_t count, double* __restrict__ values) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, hq_term, hq_row, q_coef, lam, wobj, count, values);
    const int64_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    const int64_t r = hq_row[e];
    values[e] = (r < 0 ? wobj : lam[r]) * q_coef[hq_term[e]];
}
// Expression block, forward over reverse: one thread per (row or term, seed variable j of its distinct variables).  The thread runs the
// forward sweep with its tangent for x' = e_j (val, tval), then the reverse sweep with the tangent of every adjoint statement (adj, tadj):
// the adjoint tangent that reaches the VAR nodes of variable i is d2(row) / dx_i dx_j.  Its four node arrays are a segment of the HBM
// workspace (woff[s] = first node; the segments of a row's seed threads follow each other).  The thread's occurrence list
// ovar[optr[s] .. optr[s+1]) names the variables i >= j of the row's interaction set, ascending; hocc[o] receives weight * h.
struct ExprHess {
    const int64_t *srow, *svar, *woff, *optr, *ovar;   // srow / svar / woff [S], optr [S+1], ovar [optr[S]]
    double *val, *tval, *adj, *tadj, *hocc;             // four node arrays [woff[S-1] + nodes of the last row], hocc [optr[S]]
    int64_t S;
};
// u ^ e with d = d/du (the factors of expr_powi) and d2 = d2/du2 = e (e - 1) u^(e-2): ((double)e * (double)(e - 1)) times the product of
// |e| - 2 factors u (left to right from 1.0) for e >= 2, 0.0 for e = 1, ((double)e * (double)(e - 1)) / ((u^|e| * u) * u) for e < 0
__device__ __forceinline__ double expr_powi2(double u, int64_t e, double* d, double* d2) {
#pragma clang fp contract(off)
    const int64_t k = e < 0 ? -e : e;
    double p = 1.0, q = 1.0;
    for (int64_t i = 1; i < k; ++i) { q = p; p = p * u; }
    const double pk = p * u, ee = (double)e * (double)(e - 1);
    if (e > 0) { *d = (double)e * p; *d2 = k > 1 ? ee * q : 0.0; return pk; }
    const double pu = pk * u;
    *d = (double)e / pu;
    *d2 = ee / (pu * u);
    return 1.0 / pk;
}
// sin, cos, exp and log of the second-order sweeps, out of line for the reason expr_libm is
__device__ __noinline__ double expr_libm2(int32_t op, double u) {
    switch (op) {
        case ASM_OP_SIN: return sin(u);
        case ASM_OP_COS: return cos(u);
        case ASM_OP_EXP: return exp(u);
        default: return log(u);           // ASM_OP_LOG
    }
}
// what seeds a second-order sweep and what it writes: EXPR2_HESS the unit tangent of variable `seed`, adjoint tangents of the VAR nodes into
// the thread's occurrence list; EXPR2_DATA a direction dc in the constants, the adjoint tangent of every VAR node an occurrence of its own
// (asm_eval_data_cross); EXPR2_DATA_T a direction vx in the variables, an occurrence per CONST node (asm_eval_data_cross_t)
enum { EXPR2_HESS = 0, EXPR2_DATA = 1, EXPR2_DATA_T = 2 };
// forward sweep with tangent: tval = d val / d x_seed, statement by statement the tangent of expr_forward.  EXPR2_DATA: the seed is a direction
// dc in the constants instead - a CONST node with operand a has the tangent dc[a], every VAR node 0 (asm_eval_data_cross).  EXPR2_DATA_T: the
// seed is a direction in the variables, passed as dc - a VAR node of variable a has the tangent dc[a], every CONST node 0
template <int DATA = EXPR2_HESS>
__device__ __forceinline__ void expr_forward2(const ExprTape& X, int64_t k0, int64_t k1, const double* __restrict__ x, int64_t seed, double* val, double* tval,
                                              const double* __restrict__ dc = nullptr) {
#pragma clang fp contract(off)
    for (int64_t k = k0; k < k1; ++k) {
        const int64_t a = X.a[k], b = X.b[k];
        const int32_t op = X.op[k];
        double v, d;
        if (op == ASM_OP_CONST) {
            v = X.cst[a];
            if constexpr (DATA == EXPR2_DATA) d = dc[a];
            else d = 0.0;
        }
        else if (op == ASM_OP_VAR) {
            v = x[a];
            if constexpr (DATA == EXPR2_DATA) d = 0.0;
            else if constexpr (DATA == EXPR2_DATA_T) d = dc[a];
            else d = a == seed ? 1.0 : 0.0;
        }
        else {
            const double u = val[a], du = tval[a];
            const bool binary = (op >= ASM_OP_ADD && op <= ASM_OP_DIV) || op >= ASM_OP_POW;
            const double y = binary ? val[b] : 0.0, dy = binary ? tval[b] : 0.0;
            switch (op) {
                case ASM_OP_ADD: v = u + y; d = du + dy; break;
                case ASM_OP_SUB: v = u - y; d = du - dy; break;
                case ASM_OP_MUL: v = u * y; d = du * y + u * dy; break;
                case ASM_OP_DIV: v = u / y; d = (du - v * dy) / y; break;
                case ASM_OP_NEG: v = -u; d = -du; break;
                case ASM_OP_POWI: { double d1, d2; v = expr_powi2(u, b, &d1, &d2); d = d1 * du; break; }
                case ASM_OP_SQRT: v = sqrt(u); d = (0.5 * du) / v; break;
                case ASM_OP_EXP: v = expr_libm2(ASM_OP_EXP, u); d = du * v; break;
                case ASM_OP_LOG: v = expr_libm2(ASM_OP_LOG, u); d = du / u; break;
                case ASM_OP_SIN: v = expr_libm2(ASM_OP_SIN, u); d = du * expr_libm2(ASM_OP_COS, u); break;
                case ASM_OP_COS: v = expr_libm2(ASM_OP_COS, u); d = -(du * expr_libm2(ASM_OP_SIN, u)); break;
                case ASM_OP_ABS: v = fabs(u); d = du * copysign(1.0, u); break;
                case ASM_OP_MIN: { const bool c = y < u; v = c ? y : u; d = c ? dy : du; break; }
                case ASM_OP_MAX: { const bool c = y > u; v = c ? y : u; d = c ? dy : du; break; }
                default:
                    v = expr_libm(op, u, y);
                    switch (op) {
                        case ASM_OP_TAN: d = du * (1.0 + v * v); break;
                        case ASM_OP_ASIN: d = du / sqrt((1.0 - u) * (1.0 + u)); break;
                        case ASM_OP_ACOS: d = -(du / sqrt((1.0 - u) * (1.0 + u))); break;
                        case ASM_OP_ATAN: d = du / (1.0 + u * u); break;
                        case ASM_OP_SINH: d = du * expr_libm(ASM_OP_COSH, u, 0.0); break;
                        case ASM_OP_COSH: d = du * expr_libm(ASM_OP_SINH, u, 0.0); break;
                        case ASM_OP_TANH: d = du * (1.0 - v * v); break;
                        case ASM_OP_LOG10: d = du / (u * EXPR_LN10); break;
                        case ASM_OP_LOG2: d = du / (u * EXPR_LN2); break;
                        case ASM_OP_LOG1P: d = du / (1.0 + u); break;
                        case ASM_OP_EXPM1: d = du * (v + 1.0); break;
                        case ASM_OP_CBRT: d = du / (3.0 * (v * v)); break;
                        case ASM_OP_POW:
                            d = du * (y * expr_libm(ASM_OP_POW, u, y - 1.0));
                            // a CONST exponent has a tangent in EXPR2_DATA alone (dc[a]); its term enters only where that is nonzero, so
                            // that pow(u, 2.0) at u <= 0 stays finite along every direction that leaves the exponent alone
                            if constexpr (DATA == EXPR2_DATA) { if (X.op[b] != ASM_OP_CONST || dy != 0.0) d = d + dy * (v * expr_libm2(ASM_OP_LOG, u)); }
                            else { if (X.op[b] != ASM_OP_CONST) d = d + dy * (v * expr_libm2(ASM_OP_LOG, u)); }
                            break;
                        default: { const ExprAtan2 S(u, y); d = S.q(du, S.ys) - S.q(dy, S.us); break; }   // ASM_OP_ATAN2
                    }
            }
        }
        val[k] = v;
        tval[k] = d;
    }
}
// reverse sweep with tangent: adj as expr_reverse forms it, tadj = d adj / d x_seed, statement by statement; the adjoint tangent of a VAR
// node whose variable is in the thread's occurrence list is added to hocc there (several VAR nodes of a variable: reverse node order).
// EXPR2_DATA: every VAR node is an occurrence of its own instead - hocc[node] = wt * its adjoint tangent (one product), no list.
// EXPR2_DATA_T: every CONST node k is an occurrence, hocc[slot[k]] = wt * tadj[k] + wa * adj[k] (two products, one sum; without `both` the
// first product alone), and the VAR nodes write nothing
template <int DATA = EXPR2_HESS>
__device__ __forceinline__ void expr_reverse2(const ExprTape& X, int64_t k0, int64_t k1, const double* val, const double* tval, double* adj, double* tadj,
                                              const int64_t* __restrict__ ovar, int64_t o0, int64_t o1, double* __restrict__ hocc, double wt = 0.0,
                                              double wa = 0.0, bool both = false) {
#pragma clang fp contract(off)
    for (int64_t k = k0; k < k1; ++k) { adj[k] = 0.0; tadj[k] = 0.0; }
    adj[k1 - 1] = 1.0;
    for (int64_t k = k1 - 1; k >= k0; --k) {
        const int32_t op = X.op[k];
        if (op == ASM_OP_CONST) {
            if constexpr (DATA == EXPR2_DATA_T) hocc[X.slot[k]] = both ? wt * tadj[k] + wa * adj[k] : wt * tadj[k];
            continue;
        }
        const double w = adj[k], z = tadj[k];
        const int64_t a = X.a[k], b = X.b[k];
        if (op == ASM_OP_VAR) {
            if constexpr (DATA == EXPR2_DATA) hocc[k] = wt * z;
            else if constexpr (DATA == EXPR2_HESS)
                for (int64_t o = o0; o < o1; ++o)
                    if (ovar[o] == a) { hocc[o] = hocc[o] + z; break; }
            continue;
        }
        const double u = val[a], du = tval[a], v = val[k], d = tval[k];
        switch (op) {
            case ASM_OP_ADD: adj[a] = adj[a] + w; tadj[a] = tadj[a] + z; adj[b] = adj[b] + w; tadj[b] = tadj[b] + z; break;
            case ASM_OP_SUB: adj[a] = adj[a] + w; tadj[a] = tadj[a] + z; adj[b] = adj[b] - w; tadj[b] = tadj[b] - z; break;
            case ASM_OP_MUL: {
                const double y = val[b], dy = tval[b];
                adj[a] = adj[a] + w * y; tadj[a] = tadj[a] + (z * y + w * dy);
                adj[b] = adj[b] + w * u; tadj[b] = tadj[b] + (z * u + w * du);
                break;
            }
            case ASM_OP_DIV: {
                const double y = val[b], dy = tval[b], t = w / y, dt = (z - t * dy) / y;
                adj[a] = adj[a] + t; tadj[a] = tadj[a] + dt;
                adj[b] = adj[b] - t * v; tadj[b] = tadj[b] - (dt * v + t * d);
                break;
            }
            case ASM_OP_NEG: adj[a] = adj[a] - w; tadj[a] = tadj[a] - z; break;
            case ASM_OP_POWI: {
                double d1, d2;
                (void)expr_powi2(u, b, &d1, &d2);
                adj[a] = adj[a] + w * d1; tadj[a] = tadj[a] + (z * d1 + w * (d2 * du));
                break;
            }
            case ASM_OP_SQRT: { const double s = (0.5 * w) / v; adj[a] = adj[a] + s; tadj[a] = tadj[a] + (0.5 * z - s * d) / v; break; }
            case ASM_OP_EXP: adj[a] = adj[a] + w * v; tadj[a] = tadj[a] + (z * v + w * d); break;
            case ASM_OP_LOG: { const double q = w / u; adj[a] = adj[a] + q; tadj[a] = tadj[a] + (z - q * du) / u; break; }
            case ASM_OP_SIN: {
                const double c = expr_libm2(ASM_OP_COS, u), s = expr_libm2(ASM_OP_SIN, u);
                adj[a] = adj[a] + w * c; tadj[a] = tadj[a] + (z * c - w * (s * du));
                break;
            }
            case ASM_OP_COS: {
                const double c = expr_libm2(ASM_OP_COS, u), s = expr_libm2(ASM_OP_SIN, u);
                adj[a] = adj[a] - w * s; tadj[a] = tadj[a] - (z * s + w * (c * du));
                break;
            }
            case ASM_OP_ABS: { const double s = copysign(1.0, u); adj[a] = adj[a] + w * s; tadj[a] = tadj[a] + z * s; break; }
            case ASM_OP_TAN: { const double g = 1.0 + v * v; adj[a] = adj[a] + w * g; tadj[a] = tadj[a] + (z * g + w * (2.0 * (v * d))); break; }
            case ASM_OP_ASIN: case ASM_OP_ACOS: {
                const double r = sqrt((1.0 - u) * (1.0 + u)), q = w / r, dr = -((u * du) / r), dq = (z - q * dr) / r;
                if (op == ASM_OP_ASIN) { adj[a] = adj[a] + q; tadj[a] = tadj[a] + dq; }
                else { adj[a] = adj[a] - q; tadj[a] = tadj[a] - dq; }
                break;
            }
            case ASM_OP_ATAN: { const double g = 1.0 + u * u, q = w / g; adj[a] = adj[a] + q; tadj[a] = tadj[a] + (z - q * (2.0 * (u * du))) / g; break; }
            case ASM_OP_SINH: {
                const double c = expr_libm(ASM_OP_COSH, u, 0.0), s = expr_libm(ASM_OP_SINH, u, 0.0);
                adj[a] = adj[a] + w * c; tadj[a] = tadj[a] + (z * c + w * (s * du));
                break;
            }
            case ASM_OP_COSH: {
                const double c = expr_libm(ASM_OP_COSH, u, 0.0), s = expr_libm(ASM_OP_SINH, u, 0.0);
                adj[a] = adj[a] + w * s; tadj[a] = tadj[a] + (z * s + w * (c * du));
                break;
            }
            case ASM_OP_TANH: { const double g = 1.0 - v * v; adj[a] = adj[a] + w * g; tadj[a] = tadj[a] + (z * g - w * (2.0 * (v * d))); break; }
            case ASM_OP_LOG10: case ASM_OP_LOG2: {
                const double ln = op == ASM_OP_LOG10 ? EXPR_LN10 : EXPR_LN2, g = u * ln, q = w / g;
                adj[a] = adj[a] + q; tadj[a] = tadj[a] + (z - q * (du * ln)) / g;
                break;
            }
            case ASM_OP_LOG1P: { const double g = 1.0 + u, q = w / g; adj[a] = adj[a] + q; tadj[a] = tadj[a] + (z - q * du) / g; break; }
            case ASM_OP_EXPM1: { const double g = v + 1.0; adj[a] = adj[a] + w * g; tadj[a] = tadj[a] + (z * g + w * d); break; }
            case ASM_OP_CBRT: { const double g = 3.0 * (v * v), q = w / g; adj[a] = adj[a] + q; tadj[a] = tadj[a] + (z - q * (6.0 * (v * d))) / g; break; }
            case ASM_OP_POW: {
                const double y = val[b], dy = tval[b];
                // bc: no term with dy; nb: nothing to b.  EXPR2_HESS: a CONST exponent has neither (its tangent is 0 and nobody reads its
                // adjoint).  EXPR2_DATA: its tangent is dc[a], the terms enter where that is nonzero (a zero direction on pow(u, 2.0) with
                // u <= 0 stays finite); the CONST node writes nothing.  EXPR2_DATA_T: its tangent is 0 - the terms with dy stay out, so no
                // 0 * log(u) forms and a's entries stay finite for u < 0 - and it receives adj and tadj: its occurrence is NaN or inf where
                // log(u) is, as in the first-order data sweep
                bool bc = X.op[b] == ASM_OP_CONST, nb = bc;
                if constexpr (DATA == EXPR2_DATA) { bc = bc && dy == 0.0; nb = bc; }
                else if constexpr (DATA == EXPR2_DATA_T) nb = false;
                const double p1 = expr_libm(ASM_OP_POW, u, y - 1.0), p2 = expr_libm(ASM_OP_POW, u, y - 2.0), A = y * p1;
                double dp1 = du * ((y - 1.0) * p2), lu = 0.0;
                if (!nb) lu = expr_libm2(ASM_OP_LOG, u);
                if (!bc) dp1 = dp1 + dy * (p1 * lu);
                double dA = y * dp1;
                if (!bc) dA = dA + dy * p1;
                adj[a] = adj[a] + w * A; tadj[a] = tadj[a] + (z * A + w * dA);
                if (!nb) {
                    const double B = v * lu, dB = d * lu + v * (du / u);
                    adj[b] = adj[b] + w * B; tadj[b] = tadj[b] + (z * B + w * dB);
                }
                break;
            }
            case ASM_OP_ATAN2: {
                // the statements of the header with numerator and t scaled by s and s s (ExprAtan2): the same bits where nothing underflows
                const double y = val[b], dy = tval[b];
                const ExprAtan2 S(u, y);
                const double dts = 2.0 * (S.us * du) + 2.0 * (S.ys * dy);
                const double qa = S.q(w, S.ys), qb = S.q(w, S.us);
                adj[a] = adj[a] + qa; tadj[a] = tadj[a] + (((z * S.ys + (w * dy) * S.s) - qa * dts) / S.ts) * S.s;
                adj[b] = adj[b] - qb; tadj[b] = tadj[b] - (((z * S.us + (w * du) * S.s) - qb * dts) / S.ts) * S.s;
                break;
            }
            case ASM_OP_MIN: { const int64_t c = val[b] < u ? b : a; adj[c] = adj[c] + w; tadj[c] = tadj[c] + z; break; }
            default: { const int64_t c = val[b] > u ? b : a; adj[c] = adj[c] + w; tadj[c] = tadj[c] + z; break; }   // ASM_OP_MAX
        }
    }
}
// lam: the multipliers of the block's rows; wobj = obj_factor * objective_scale, the weight of a term
__global__ __launch_bounds__(256) void k_nlp_expr_hess(AsmBt abt, ExprTape X, ExprHess H, const double* __restrict__ x, const double* __restrict__ lam, double wobj) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, X, H, x, lam, wobj);
    const int64_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= H.S) return;
    const int64_t t = H.srow[s], k0 = X.ptr[t], k1 = X.ptr[t + 1], wb = H.woff[s] - k0, o0 = H.optr[s], o1 = H.optr[s + 1];
    expr_forward2(X, k0, k1, x, H.svar[s], H.val + wb, H.tval + wb);
    for (int64_t o = o0; o < o1; ++o) H.hocc[o] = 0.0;
    expr_reverse2(X, k0, k1, H.val + wb, H.tval + wb, H.adj + wb, H.tadj + wb, H.ovar, o0, o1, H.hocc);
    const double wt = t < X.R ? lam[t] : wobj;
    for (int64_t o = o0; o < o1; ++o) H.hocc[o] = wt * H.hocc[o];
}
// one thread per block entry sums its occurrences in list order from 0.0 ((row, then term) order: no atomics, the host twin's sum)
__global__ __launch_bounds__(256) void k_nlp_expr_hess_gather(AsmBt abt, const int64_t* __restrict__ eptr, const int64_t* __restrict__ eocc, const double* __restrict__ hocc, int64_t count, double* __restrict__ values) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, eptr, eocc, hocc, count, values);
    const int64_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    double g = 0.0;
    for (int64_t q = eptr[e]; q < eptr[e + 1]; ++q) g = g + hocc[eocc[q]];
    values[e] = g;
}
// ---- second derivatives of NLP block 1 (nlp_kind ASM_NLP_ACOPF_OHM_HESS; include/asm_hip.h, "Hessian of the Lagrangian", 3.)
// Every row of a branch is F = k_f vf^2 + k_t vt^2 + vf vt (P cos d + Q sin d), d = va_f - va_t, with (P, Q | k_f, k_t) =
//   pfr (a_f, b_f | k_ff_p, 0)   qfr (-b_f, a_f | k_ff_q, 0)   pto (a_t, -b_t | 0, k_tt_p)   qto (-b_t, -a_t | 0, k_tt_q)
// and the constraint is x_flow - F: with lam the block's multipliers the weights are w = -lam.  One thread per branch forms the four
// weighted sums in row order (from the first term), b = Pw cos d + Qw sin d, r = Qw cos d - Pw sin d, and writes its ten occurrences
//   (vf,vf) (vt,vt) (vf,vt) (vf,va_f) (vf,va_t) (vt,va_f) (vt,va_t) (va_f,va_f) (va_t,va_t) (va_f,va_t)
// into hocc [10][nl] (a wavefront's stores are contiguous); k_nlp_expr_hess_gather sums each entry's occurrences.  The flow variables
// are linear and the block has no objective: nothing else enters.
__global__ __launch_bounds__(256) void k_nlp_ohm_hess(AsmBt abt, const int64_t* __restrict__ ipar, const double* __restrict__ dpar, const double* __restrict__ x, const double* __restrict__ lam, double* __restrict__ hocc) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, ipar, dpar, x, lam, hocc);
    const int64_t nl = ipar[0];
    const int64_t l = blockIdx.x * 256 + threadIdx.x;
    if (l >= nl) return;
    const int64_t va0 = ipar[1], vm0 = ipar[2];
    const int64_t fb = ipar[7 + l], tb = ipar[7 + nl + l];
    const double kffp = dpar[l], kffq = dpar[nl + l], kttp = dpar[2 * nl + l], kttq = dpar[3 * nl + l];
    const double af = dpar[4 * nl + l], bf = dpar[5 * nl + l], at = dpar[6 * nl + l], bt = dpar[7 * nl + l];
    const double w0 = -lam[l], w1 = -lam[nl + l], w2 = -lam[2 * nl + l], w3 = -lam[3 * nl + l];
    const double vf = x[vm0 + fb], vt = x[vm0 + tb];
    const double d = x[va0 + fb] - x[va0 + tb];
    const double cs = cos(d), sn = sin(d);
    const double skf = w0 * kffp + w1 * kffq;
    const double skt = w2 * kttp + w3 * kttq;
    const double Pw = ((w0 * af - w1 * bf) + w2 * at) - w3 * bt;
    const double Qw = ((w0 * bf + w1 * af) - w2 * bt) - w3 * at;
    const double b = Pw * cs + Qw * sn;
    const double r = Qw * cs - Pw * sn;
    const double vvb = (vf * vt) * b, vtr = vt * r, vfr = vf * r;
    double* o = hocc + l;
    o[0] = 2.0 * skf;
    o[nl] = 2.0 * skt;
    o[2 * nl] = b;
    o[3 * nl] = vtr;
    o[4 * nl] = -vtr;
    o[5 * nl] = vfr;
    o[6 * nl] = -vfr;
    o[7 * nl] = -vvb;
    o[8 * nl] = -vvb;
    o[9 * nl] = vvb;
}
// ---- second derivatives of NLP block 2 (nlp_kind ASM_NLP_DENSE_QUADRATIC_HESS): hess g_i = diag(Q_i), so the block's entries are the n
// diagonal ones and entry j is sum_i lam_i Q_ij, i ascending from 0.0.  One thread per variable (reads coalesced across j), straight into
// the value list: no occurrence array, no gather.
__global__ __launch_bounds__(256) void k_nlp_dense_hess(AsmBt abt, const double* __restrict__ dpar, int64_t mrows, int64_t n, const double* __restrict__ lam, double* __restrict__ values) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, dpar, mrows, n, lam, values);
    const int64_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const double* Q = dpar + mrows * n;
    double g = 0.0;
    for (int64_t i = 0; i < mrows; ++i) g = g + lam[i] * Q[i * n + j];
    values[j] = g;
}
// ---- cross derivatives with respect to the data (asm_eval_data_cross; include/asm_hip.h, "Cross derivatives"): the forward-over-reverse
// sweep of k_nlp_expr_hess seeded in the constants.  One thread per row (t < R) or term; its four node arrays are its nodes' places in four
// HBM arrays of L doubles (the workspace scheme of ExprHess with one segment per row).  The tangent of a row's last node is wrow[t]
// (d g_t / d dpar . dc); the adjoint tangent of every VAR node k, times -lam[t] or the objective's sense scale, is the occurrence vocc[k].
struct ExprCross {
    const int64_t *vptr, *vnode;                        // vptr [n+1]; vnode [vptr[n]]: the VAR nodes of each variable, (row, then term) ascending, node descending
    double *val, *tval, *adj, *tadj, *vocc;             // [L] each
};
__global__ __launch_bounds__(256) void k_nlp_expr_cross(AsmBt abt, ExprTape X, ExprCross C, const double* __restrict__ x, const double* __restrict__ dc, const double* __restrict__ lam, double scale, double* __restrict__ wrow) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, X, C, x, dc, lam, scale, wrow);
    const int64_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= X.R + X.T) return;
    const int64_t k0 = X.ptr[t], k1 = X.ptr[t + 1];
    expr_forward2<EXPR2_DATA>(X, k0, k1, x, -1, C.val, C.tval, dc);
    if (t < X.R) wrow[t] = C.tval[k1 - 1];
    expr_reverse2<EXPR2_DATA>(X, k0, k1, C.val, C.tval, C.adj, C.tadj, nullptr, 0, 0, C.vocc, t < X.R ? -lam[t] : scale);
}
// one thread per variable sums its occurrences in list order from 0.0 (fixed order, no atomics: the host twin's sum)
__global__ __launch_bounds__(256) void k_nlp_expr_cross_gather(AsmBt abt, ExprCross C, int64_t n, double* __restrict__ u) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, C, n, u);
    const int64_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double g = 0.0;
    for (int64_t q = C.vptr[j]; q < C.vptr[j + 1]; ++q) g = g + C.vocc[C.vnode[q]];
    u[j] = g;
}
// ---- data derivatives of NLP blocks 1 and 2 (kinds ASM_NLP_ACOPF_OHM_HESS and ASM_NLP_DENSE_QUADRATIC_HESS; include/asm_hip.h, "Data
// derivatives of the block kernels").  Both blocks are linear in their data, so nothing here reads dpar: the data gradient is the row's own
// expression with a unit coefficient, the cross derivative the block's kernel with the direction dc where dpar stands.  No fused
// multiply-add: every written operation is one rounding, left to right, which is what the NumPy twins do (acopf.py: _ohm_data_twins;
// problems.py: synthetic_dense_function_model).
// Ohm's-law block, data gradient: the constraint is x_flow - F_r(c), so out[c] = lam_r dF_r/dc.  One thread per branch, eight stores to
// out[q * nl + l] in dpar's layout (k_ff_p, k_ff_q, k_tt_p, k_tt_q, a_f, b_f, a_t, b_t); lam: the multipliers of the block's rows.
__global__ __launch_bounds__(256) void k_nlp_ohm_data_grad(AsmBt abt, const int64_t* __restrict__ ipar, const double* __restrict__ x, const double* __restrict__ lam, double* __restrict__ out) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, ipar, x, lam, out);
    const int64_t nl = ipar[0];
    const int64_t l = blockIdx.x * 256 + threadIdx.x;
    if (l >= nl) return;
    const int64_t va0 = ipar[1], vm0 = ipar[2];
    const int64_t fb = ipar[7 + l], tb = ipar[7 + nl + l];
    const double l0 = lam[l], l1 = lam[nl + l], l2 = lam[2 * nl + l], l3 = lam[3 * nl + l];
    const double vf = x[vm0 + fb], vt = x[vm0 + tb];
    const double d = x[va0 + fb] - x[va0 + tb];
    const double cs = cos(d), sn = sin(d);
    const double vv = vf * vt;
    const double vf2 = vf * vf, vt2 = vt * vt, vvc = vv * cs, vvs = vv * sn;
    double* o = out + l;
    o[0] = l0 * vf2;
    o[nl] = l1 * vf2;
    o[2 * nl] = l2 * vt2;
    o[3 * nl] = l3 * vt2;
    o[4 * nl] = l0 * vvc + l1 * vvs;
    o[5 * nl] = l0 * vvs - l1 * vvc;
    o[6 * nl] = l2 * vvc - l3 * vvs;
    o[7 * nl] = -(l2 * vvs) - l3 * vvc;
}
// Ohm's-law block, cross derivatives: one thread per (branch, column), the column in blockIdx.y.  With the column's direction (dc + column *
// ldc) where k_nlp_acopf_ohm reads dpar the thread forms that kernel's four flows F_r and its derivative families dvf_r, dvt_r, dth_r; it
// writes w = -F_r into cx[column * ldo + n + r * nl + l] (cx: [u (n) | w (4 nl)] per column) and, with lam the multipliers of the block's
// rows, its four occurrences of u into occ[column][4][nl]: sum_r lam_r dvf_r (vm_f), sum_r lam_r dvt_r (vm_t), theta = sum_r lam_r dth_r
// (va_f), -theta (va_t) - the sums in row order from the first term.  k_nlp_block_cross_gather sums the occurrences of each variable.
__global__ __launch_bounds__(256) void k_nlp_ohm_cross(AsmBt abt, const int64_t* __restrict__ ipar, const double* __restrict__ x, const double* __restrict__ dc, int64_t ldc, const double* __restrict__ lam, double* __restrict__ occ, double* __restrict__ cx, int64_t n, int64_t ldo) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, ipar, x, dc, ldc, lam, occ, cx, n, ldo);
    const int64_t nl = ipar[0];
    const int64_t l = blockIdx.x * 256 + threadIdx.x;
    if (l >= nl) return;
    const int64_t va0 = ipar[1], vm0 = ipar[2];
    const int64_t fb = ipar[7 + l], tb = ipar[7 + nl + l];
    const double* c = dc + blockIdx.y * ldc;
    const double kffp = c[l], kffq = c[nl + l], kttp = c[2 * nl + l], kttq = c[3 * nl + l];
    const double af = c[4 * nl + l], bf = c[5 * nl + l], at = c[6 * nl + l], bt = c[7 * nl + l];
    const double l0 = lam[l], l1 = lam[nl + l], l2 = lam[2 * nl + l], l3 = lam[3 * nl + l];
    const double vf = x[vm0 + fb], vt = x[vm0 + tb];
    const double d = x[va0 + fb] - x[va0 + tb];
    const double cs = cos(d), sn = sin(d);
    const double vv = vf * vt;
    const double pfr = kffp * vf * vf + af * vv * cs + bf * vv * sn;
    const double qfr = kffq * vf * vf - bf * vv * cs + af * vv * sn;
    const double pto = kttp * vt * vt + at * vv * cs - bt * vv * sn;
    const double qto = kttq * vt * vt - bt * vv * cs - at * vv * sn;
    const double dvf[4] = {2 * kffp * vf + af * vt * cs + bf * vt * sn, 2 * kffq * vf - bf * vt * cs + af * vt * sn,
                           at * vt * cs - bt * vt * sn, -bt * vt * cs - at * vt * sn};
    const double dvt[4] = {af * vf * cs + bf * vf * sn, -bf * vf * cs + af * vf * sn, 2 * kttp * vt + at * vf * cs - bt * vf * sn,
                           2 * kttq * vt - bt * vf * cs - at * vf * sn};
    const double dth[4] = {-af * vv * sn + bf * vv * cs, bf * vv * sn + af * vv * cs, -at * vv * sn - bt * vv * cs, bt * vv * sn - at * vv * cs};
    double* w = cx + blockIdx.y * ldo + n + l;
    w[0] = -pfr;
    w[nl] = -qfr;
    w[2 * nl] = -pto;
    w[3 * nl] = -qto;
    const double th = ((l0 * dth[0] + l1 * dth[1]) + l2 * dth[2]) + l3 * dth[3];
    double* o = occ + blockIdx.y * (4 * nl) + l;
    o[0] = ((l0 * dvf[0] + l1 * dvf[1]) + l2 * dvf[2]) + l3 * dvf[3];
    o[nl] = ((l0 * dvt[0] + l1 * dvt[1]) + l2 * dvt[2]) + l3 * dvt[3];
    o[2 * nl] = th;
    o[3 * nl] = -th;
}
// u of the Ohm's-law block: one thread per (variable, column) sums the variable's occurrences in list order from 0.0 - branch ascending,
// inside a branch the slot order of k_nlp_ohm_cross (k_nlp_expr_hess_gather's scheme with a column offset; no atomics, the host twin's
// sum).  vptr [n + 1], vocc [vptr[n]]: where each occurrence lives in a column's occ (locc doubles per column).  A variable without an
// occurrence (flows, generators) gets 0.
__global__ __launch_bounds__(256) void k_nlp_block_cross_gather(AsmBt abt, const int64_t* __restrict__ vptr, const int64_t* __restrict__ vocc, const double* __restrict__ occ, int64_t locc, int64_t n, double* __restrict__ cx, int64_t ldo) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, vptr, vocc, occ, locc, n, cx, ldo);
    const int64_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const double* oc = occ + blockIdx.y * locc;
    double g = 0.0;
    for (int64_t q = vptr[j]; q < vptr[j + 1]; ++q) g = g + oc[vocc[q]];
    cx[blockIdx.y * ldo + j] = g;
}
// Dense quadratic block, data gradient: g_i = sum_j A_ij x_j + 1/2 Q_ij x_j^2, so d(-lam' g)/dA_ij = (-lam_i) x_j and d/dQ_ij =
// (-lam_i) (1/2 x_j^2).  One thread per entry (i, j); out in dpar's layout, A then Q, row-major.
__global__ __launch_bounds__(256) void k_nlp_dense_data_grad(AsmBt abt, int64_t mrows, int64_t n, const double* __restrict__ x, const double* __restrict__ lam, double* __restrict__ out) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, mrows, n, x, lam, out);
    const int64_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= mrows * n) return;
    const int64_t i = e / n, j = e - i * n;
    const double xj = x[j], wi = -lam[i];
    out[e] = wi * xj;
    out[mrows * n + e] = wi * (0.5 * (xj * xj));
}
// Dense quadratic block, cross derivatives, w: the rows of k_nlp_dense_quadratic with the column's direction (dA, dQ) where dpar stands -
// one wavefront per row, lane-strided, then the xor tree; w_i into cx[column * ldo + n + i], the column in blockIdx.y.
__global__ __launch_bounds__(256) void k_nlp_dense_cross_w(AsmBt abt, const double* __restrict__ dc, int64_t ldc, int64_t mrows, int64_t n, const double* __restrict__ x, double* __restrict__ cx, int64_t ldo) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, dc, ldc, mrows, n, x, cx, ldo);
    const int64_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= mrows) return;
    const int lane = threadIdx.x & 63;
    const double* Ar = dc + blockIdx.y * ldc + i * n;
    const double* Qr = Ar + mrows * n;
    double acc = 0.0;
    for (int64_t j = lane; j < n; j += 64) {
        const double xj = x[j];
        acc = acc + (Ar[j] * xj + 0.5 * Qr[j] * xj * xj);
    }
    for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
    if (lane == 0) cx[blockIdx.y * ldo + n + i] = acc;
}
// ... and u: u_j = -sum_i lam_i (dA_ij + dQ_ij x_j), i ascending from 0.0.  One thread per (variable, column), reads coalesced across j
// (as k_nlp_dense_hess); lam: the multipliers of the block's rows.
__global__ __launch_bounds__(256) void k_nlp_dense_cross_u(AsmBt abt, const double* __restrict__ dc, int64_t ldc, int64_t mrows, int64_t n, const double* __restrict__ x, const double* __restrict__ lam, double* __restrict__ cx, int64_t ldo) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, dc, ldc, mrows, n, x, lam, cx, ldo);
    const int64_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const double* dA = dc + blockIdx.y * ldc;
    const double* dQ = dA + mrows * n;
    const double xj = x[j];
    double g = 0.0;
    for (int64_t i = 0; i < mrows; ++i) g = g + lam[i] * (dA[i * n + j] + dQ[i * n + j] * xj);
    cx[blockIdx.y * ldo + j] = -g;
}
// ---- transposed cross derivatives (asm_eval_data_cross_t; include/asm_hip.h, "Transposed cross derivatives"): for weights vx [n] and vl (the
// block's rows), out[c] = d/d dpar[c] [ D_vx L + vl' g ] - for every direction dc, dc' out = vx' u + vl' w with (u, w) of asm_eval_data_cross.
// Expression block: the sweep of k_nlp_expr_cross with the other seed - a VAR node of variable j has the tangent vx[j], a CONST node 0 (a
// CONST exponent of POW is a CONST node like any other: it receives its adjoint and adjoint tangent).  One thread per row (t < R) or term, its node arrays as in k_nlp_expr_cross; in the reverse pass
// every CONST node yields one occurrence into the cocc list of k_nlp_expr_const_adj (same slot, same cptr grouping): for a node of row t
// (-lam[t]) * tadj + vl[t] * adj - two products, one sum - and for a node of a term scale * tadj.  k_nlp_expr_data_gather sums per dpar index.
__global__ __launch_bounds__(256) void k_nlp_expr_cross_t(AsmBt abt, ExprTape X, ExprCross C, const double* __restrict__ x, const double* __restrict__ vx, const double* __restrict__ lam, const double* __restrict__ vl, double scale, double* __restrict__ cocc) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, X, C, x, vx, lam, vl, scale, cocc);
    const int64_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= X.R + X.T) return;
    const int64_t k0 = X.ptr[t], k1 = X.ptr[t + 1];
    const bool row = t < X.R;
    expr_forward2<EXPR2_DATA_T>(X, k0, k1, x, -1, C.val, C.tval, vx);
    expr_reverse2<EXPR2_DATA_T>(X, k0, k1, C.val, C.tval, C.adj, C.tadj, nullptr, 0, 0, cocc, row ? -lam[t] : scale, row ? vl[t] : 0.0, row);
}
// Ohm's-law block: one thread per (branch, column), the column in blockIdx.y; a column's weights are [vx (n) | vl (4 nl)] at v + column * ldv,
// its outputs out + column * ldo in dpar's layout.  The block is linear in its data, nothing reads dpar.  With the four basis values of
// k_nlp_ohm_data_grad, vf2 = vf*vf, vt2 = vt*vt, vvc = vv*cs, vvs = vv*sn, and their derivatives along vx at the branch's four variables
// (dvf, dvt the entries of vx at vm_f, vm_t; dd = vx[va_f] - vx[va_t]; tvv = dvf*vt + vf*dvt):
//   tvf2 = 2*(vf*dvf)    tvt2 = 2*(vt*dvt)    tvvc = tvv*cs - vvs*dd    tvvs = tvv*sn + vvc*dd
// every output is k_nlp_ohm_data_grad's pattern with (lam, derivative) minus the same pattern with (vl, value) - the constraint is x_flow - F_r.
__global__ __launch_bounds__(256) void k_nlp_ohm_cross_t(AsmBt abt, const int64_t* __restrict__ ipar, const double* __restrict__ x, const double* __restrict__ lam, const double* __restrict__ v, int64_t ldv, int64_t n, double* __restrict__ out, int64_t ldo) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, ipar, x, lam, v, ldv, n, out, ldo);
    const int64_t nl = ipar[0];
    const int64_t l = blockIdx.x * 256 + threadIdx.x;
    if (l >= nl) return;
    const int64_t va0 = ipar[1], vm0 = ipar[2];
    const int64_t fb = ipar[7 + l], tb = ipar[7 + nl + l];
    const double* vx = v + blockIdx.y * ldv;
    const double* vl = vx + n;
    const double l0 = lam[l], l1 = lam[nl + l], l2 = lam[2 * nl + l], l3 = lam[3 * nl + l];
    const double v0 = vl[l], v1 = vl[nl + l], v2 = vl[2 * nl + l], v3 = vl[3 * nl + l];
    const double vf = x[vm0 + fb], vt = x[vm0 + tb];
    const double d = x[va0 + fb] - x[va0 + tb];
    const double dvf = vx[vm0 + fb], dvt = vx[vm0 + tb];
    const double dd = vx[va0 + fb] - vx[va0 + tb];
    const double cs = cos(d), sn = sin(d);
    const double vv = vf * vt;
    const double vf2 = vf * vf, vt2 = vt * vt, vvc = vv * cs, vvs = vv * sn;
    const double tvv = dvf * vt + vf * dvt;
    const double tvf2 = 2.0 * (vf * dvf), tvt2 = 2.0 * (vt * dvt);
    const double tvvc = tvv * cs - vvs * dd, tvvs = tvv * sn + vvc * dd;
    double* o = out + blockIdx.y * ldo + l;
    o[0] = l0 * tvf2 - v0 * vf2;
    o[nl] = l1 * tvf2 - v1 * vf2;
    o[2 * nl] = l2 * tvt2 - v2 * vt2;
    o[3 * nl] = l3 * tvt2 - v3 * vt2;
    o[4 * nl] = (l0 * tvvc + l1 * tvvs) - (v0 * vvc + v1 * vvs);
    o[5 * nl] = (l0 * tvvs - l1 * tvvc) - (v0 * vvs - v1 * vvc);
    o[6 * nl] = (l2 * tvvc - l3 * tvvs) - (v2 * vvc - v3 * vvs);
    o[7 * nl] = (-(l2 * tvvs) - l3 * tvvc) - (-(v2 * vvs) - v3 * vvc);
}
// Dense quadratic block: one thread per entry (i, j) and column (blockIdx.y), weights and outputs laid out as for k_nlp_ohm_cross_t:
//   out[A_ij] = (-lam_i) * vx_j + vl_i * x_j        out[Q_ij] = (-lam_i) * (x_j * vx_j) + vl_i * (0.5 * (x_j * x_j))
__global__ __launch_bounds__(256) void k_nlp_dense_cross_t(AsmBt abt, int64_t mrows, int64_t n, const double* __restrict__ x, const double* __restrict__ lam, const double* __restrict__ v, int64_t ldv, double* __restrict__ out, int64_t ldo) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, mrows, n, x, lam, v, ldv, out, ldo);
    const int64_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= mrows * n) return;
    const int64_t i = e / n, j = e - i * n;
    const double* vx = v + blockIdx.y * ldv;
    const double xj = x[j], vxj = vx[j], wi = -lam[i], vli = vx[n + i];
    double* o = out + blockIdx.y * ldo;
    o[e] = wi * vxj + vli * xj;
    o[mrows * n + e] = wi * (xj * vxj) + vli * (0.5 * (xj * xj));
}
// out = H v from the values: one thread per variable walks its list of (entry, other variable) in entry order - an off-diagonal entry
// (i, j) is in the lists of i and of j - and sums values[entry] * v[other] from 0.0
__global__ __launch_bounds__(256) void k_hess_product(AsmBt abt, const int64_t* __restrict__ pptr, const int64_t* __restrict__ pent, const int64_t* __restrict__ poth, const double* __restrict__ values, const double* __restrict__ v, int64_t n, double* __restrict__ out) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, pptr, pent, poth, values, v, n, out);
    const int64_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double g = 0.0;
    for (int64_t q = pptr[i]; q < pptr[i + 1]; ++q) g = g + values[pent[q]] * v[poth[q]];
    out[i] = g;
}

__global__ __launch_bounds__(256) void k_axpy_out(AsmBt abt, const double* __restrict__ x, double alpha, const double* __restrict__ p, double* __restrict__ out, int64_t n) {
    ASM_BARGS(abt, x, alpha, p, out, n);
    int64_t j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) out[j] = x[j] + alpha * p[j];
}
// the trial points of a batched line search: out[t] = x + alpha[t] p, t = blockIdx.y
struct TrialAlphas { double a[8]; };
__global__ __launch_bounds__(256) void k_axpy_trials(AsmBt abt, const double* __restrict__ x, TrialAlphas al, const double* __restrict__ p, double* __restrict__ out, int64_t n, int64_t ldx) {
    ASM_BARGS(abt, x, al, p, out, n, ldx);
    int64_t j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) out[blockIdx.y * ldx + j] = x[j] + al.a[blockIdx.y] * p[j];
}

// ---- per-iteration reductions (one 1024-thread workgroup, fixed order)
enum { RN_PRIM_INF = 0, RN_PRIM_1, RN_KT, RN_COMPL, RN_COUNT };
struct SlpVecs {
    const double *E, *g_L, *g_U, *x, *x_L, *x_U, *df, *lam, *mU, *mL, *jtl, *rown;   // jtl = J' lambda, rown = row norms of J
    int64_t n, m;
};
// norm_violations (inf and 1 norm), norm_complementarity (inf norm), KT_residuals  - common.jl:35-98
__global__ __launch_bounds__(1024) void k_slp_norms(AsmBt abt, SlpVecs V, double* __restrict__ out) {
    ASM_BARGS(abt, V, out);
    __shared__ double sh[16];
    double vinf = 0.0, v1 = 0.0, cinf = 0.0, den = 0.0, res = 0.0, ndf = 0.0, sc = 0.0;
    for (int64_t i = threadIdx.x; i < V.m; i += 1024) {
        const double e = V.E[i], lo = V.g_L[i], up = V.g_U[i];
        const double v = e > up ? e - up : (e < lo ? lo - e : 0.0);
        vinf = fmax(vinf, v);
        v1 += v;
        if (lo != up) {
            const double l = V.lam[i];
            cinf = fmax(cinf, fabs(fmin(e - lo, up - e) * l));
            den += l * l;
        }
        sc = fmax(sc, fabs(V.lam[i]) * V.rown[i]);
    }
    for (int64_t j = threadIdx.x; j < V.n; j += 1024) {
        const double xj = V.x[j];
        const double v = xj > V.x_U[j] ? xj - V.x_U[j] : (xj < V.x_L[j] ? V.x_L[j] - xj : 0.0);
        vinf = fmax(vinf, v);
        v1 += v;
        const double r = V.df[j] - V.jtl[j] - V.mU[j] - V.mL[j];
        res += r * r;
        ndf += V.df[j] * V.df[j];
    }
    vinf = blk_reduce_max(vinf, sh);
    cinf = blk_reduce_max(cinf, sh);
    sc = blk_reduce_max(sc, sh);
    v1 = blk_reduce_sum(v1, sh);
    den = blk_reduce_sum(den, sh);
    res = blk_reduce_sum(res, sh);
    ndf = blk_reduce_sum(ndf, sh);
    if (threadIdx.x == 0) {
        out[RN_PRIM_INF] = vinf;
        out[RN_PRIM_1] = v1;
        out[RN_KT] = sqrt(res) / fmax(fmax(1.0, sqrt(ndf)), sc);
        out[RN_COMPL] = cinf / (1.0 + sqrt(den));
    }
}
// compute_phi (slp.jl:79-115) / compute_derivative (slp.jl:122-147).  Et = constraint values at the trial point (E itself for
// alpha = 0), ps = p_slack as 2 entries per row (second NaN when the row has one slack).
//   mode 0 (phi):        normal  f_trial + nu . viol(Et)                restoration  prim_infeas + alpha * sum(slacks) + nu . viol(lhs)
//   mode 1 (derivative): normal  df . p - nu . viol(E)                  restoration  sum(slacks) - nu . viol(E - viol(E))
// One workgroup's merit value (valid on thread 0): the body of k_slp_merit and of k_slp_tr_quality, so that both kernels make the same
// instructions in the same reduction order.
__device__ __forceinline__ double slp_merit_wg(const SlpVecs& V, const double* __restrict__ Et, const double* __restrict__ nu, const double* __restrict__ ps,
                                               const double* __restrict__ p, double alpha, int feasibility, double prim_infeas,
                                               const double* __restrict__ f_trial, int mode, double* sh) {
    double pen = 0.0, ssum = 0.0, dfp = 0.0;
    for (int64_t i = threadIdx.x; i < V.m; i += 1024) {
        const double lo = V.g_L[i], up = V.g_U[i], e = V.E[i];
        const double viol = fmax(0.0, fmax(e - up, lo - e));
        double lhs;
        if (!feasibility) lhs = mode == 0 ? Et[i] : e;
        else {
            const bool both = lo > -INFINITY && up < INFINITY;
            const double s1 = ps[2 * i], s2 = both ? ps[2 * i + 1] : 0.0;
            ssum += s1 + s2;
            lhs = (mode == 0 ? Et[i] : e) - viol;
            if (mode == 0) lhs += alpha * (both ? s1 - s2 : (lo > -INFINITY ? s1 : (up < INFINITY ? -s1 : 0.0)));
        }
        pen += nu[i] * fmax(0.0, fmax(lhs - up, lo - lhs));
    }
    if (mode == 1 && !feasibility)
        for (int64_t j = threadIdx.x; j < V.n; j += 1024) dfp += V.df[j] * p[j];
    pen = blk_reduce_sum(pen, sh);
    ssum = blk_reduce_sum(ssum, sh);
    dfp = blk_reduce_sum(dfp, sh);
    if (mode == 0) return feasibility ? prim_infeas + alpha * ssum + pen : f_trial[0] + pen;
    return feasibility ? ssum - pen : dfp - pen;
}
__global__ __launch_bounds__(1024) void k_slp_merit(AsmBt abt, SlpVecs V, const double* __restrict__ Et, const double* __restrict__ nu, const double* __restrict__ ps, const double* __restrict__ p, double alpha, int feasibility, double prim_infeas, const double* __restrict__ f_trial, int mode, double* __restrict__ out, TrialAlphas al, int64_t ldE) {
    ASM_BARGS(abt, V, Et, nu, ps, p, alpha, feasibility, prim_infeas, f_trial, mode, out, al, ldE);
    __shared__ double sh[16];
    if (gridDim.x > 1) {              // batched line search: one workgroup per trial point
        alpha = al.a[blockIdx.x];
        Et += blockIdx.x * ldE;
        f_trial += blockIdx.x;
        out += blockIdx.x;
    }
    const double v = slp_merit_wg(V, Et, nu, ps, p, alpha, feasibility, prim_infeas, f_trial, mode, sh);
    if (threadIdx.x == 0) out[0] = v;
}
// step_quality's three merit quantities (slp_trust_region.jl:213-216) in one launch of 3 workgroups, workgroup b = out[b]:
//   b = 0  compute_derivative            (mode 1, at E)
//   b = 1  compute_phi(x, 0, p)          (mode 0, alpha 0, at E and f)
//   b = 2  compute_phi(x, 1, p)          (mode 0, alpha 1, at the trial values Et and f_trial)
// each the value one asm_slp_merit call returns, bit for bit (same body, same reduction order).
__global__ __launch_bounds__(1024) void k_slp_tr_quality(AsmBt abt, SlpVecs V, const double* __restrict__ Et, const double* __restrict__ nu, const double* __restrict__ ps, const double* __restrict__ p, int feasibility, double prim_infeas, const double* __restrict__ f, const double* __restrict__ f_trial, double* __restrict__ out) {
    ASM_BARGS(abt, V, Et, nu, ps, p, feasibility, prim_infeas, f, f_trial, out);
    __shared__ double sh[16];
    const int b = blockIdx.x;
    const double v = slp_merit_wg(V, b == 2 ? Et : V.E, nu, ps, p, b == 2 ? 1.0 : 0.0, feasibility, prim_infeas, b == 2 ? f_trial : f, b == 0 ? 1 : 0, sh);
    if (threadIdx.x == 0) out[b] = v;
}
