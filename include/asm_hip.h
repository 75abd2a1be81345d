/* libasmhip - C ABI of the MI355X-native SLP sub-problem solver.
 *
 * This is the drop-in boundary for the per-iteration sub-LP path of exanauts/ActiveSetMethods:
 * everything `sub_optimize!(slp, Δ)` (src/algorithms/slp.jl:23-47) does below the SLP outer loop -
 * Jacobian assembly (src/algorithms/common.jl:12-20), LP formulation for the normal and the
 * feasibility-restoration phase (src/algorithms/subproblem.jl:51-215, 229-484), the LP solve that the
 * reference hands to an external MOI optimizer (subproblem.jl:490, GLPK in all its tests) and the
 * extraction of step / multipliers (subproblem.jl:494-541).
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary; every entry returns 0 on success, <0 on misuse or a
 *     HIP error (asm_last_error gives the text).  The LP outcome is reported only through `status`.
 *   - the caller owns every array; the library copies what it needs during the call and keeps no host
 *     pointer afterwards.  Device buffers belong to the handle and are freed by asm_destroy.
 *   - reals are IEEE double, indices int64 and 1-BASED exactly as the reference's `j_str`
 *     (src/MOI_wrapper.jl:726-746); +-Inf bounds are IEEE infinities.
 *   - one handle <-> one HIP stream; distinct handles may be used concurrently from different host
 *     threads / devices (needed for scenario batches); a single handle is not re-entrant.
 *
 * Reference-side binding (Julia `ccall`): see INTEGRATION.md.
 */
#ifndef ASM_HIP_H
#define ASM_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct asm_handle asm_handle;

/* MOI.TerminationStatusCode values this path can produce (subproblem.jl:491, 500-539). */
enum { ASM_OPTIMAL = 1, ASM_INFEASIBLE = 2, ASM_DUAL_INFEASIBLE = 3, ASM_OTHER = 4 };

/* error codes: ASM_ERR_ARG a bad argument (null pointer, size, value), ASM_ERR_HIP a device or HIP runtime failure, ASM_ERR_STATE a missing
 * earlier call (asm_sublp_setup, asm_eval_setup, asm_eval_functions), ASM_ERR_UNSUPPORTED valid input the library cannot represent (an LP
 * skeleton the reference cannot build).  A batch entry returns the code the per-handle entry returns for the same input. */
enum { ASM_OK = 0, ASM_ERR_ARG = -1, ASM_ERR_HIP = -2, ASM_ERR_STATE = -3, ASM_ERR_UNSUPPORTED = -11 };

/* Replaces `MOI.instantiate(slp.options.external_optimizer)` (slp.jl:32). */
int asm_create(int device, asm_handle** out);
int asm_destroy(asm_handle* h);
const char* asm_last_error(const asm_handle* h);

/* Replaces QpModel(...) + create_model! (subproblem.jl:16-215): fixes the pattern and the row/slack
 * layout.  j_row/j_col: nnz entries, 1-based, duplicates allowed, any order (order defines the
 * accumulation order of duplicates).  Rows with c_lb=-Inf and c_ub=+Inf are rejected
 * (ASM_ERR_UNSUPPORTED): create_model! adds no row for them and the reference's indexing breaks. */
int asm_sublp_setup(asm_handle* h, int64_t n, int64_t m, int64_t nnz,
                    const int64_t* j_row, const int64_t* j_col,
                    const double* c_lb, const double* c_ub,
                    const double* v_lb, const double* v_ub);

/* Same pattern, new bounds (a new scenario of a batch: the loads of an ACOPF scenario are constraint bounds): keeps every
 * device buffer, the assembly plan and the evaluator's function store; the retained active sets are dropped.  The kind of
 * each row (==, range, >= only, <= only) must not change - that would be another LP skeleton (create_model!,
 * subproblem.jl:137-214): ASM_ERR_UNSUPPORTED. */
int asm_sublp_set_bounds(asm_handle* h, const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub);

/* Replaces sub_optimize!(qp, x_k, Δ, feasibility) (subproblem.jl:229-542) with data = LpData(slp)
 * (slp.jl:8-21): dE = Jacobian values in j_str order, df = gradient (c), f = objective value (c0),
 * E = constraint values (b).
 * Outputs (caller-allocated): p[n] (Xsol), lambda[m], mult_x_U[n], mult_x_L[n],
 *   p_slack[2m]: p_slack[2i], p_slack[2i+1] = slack values of row i, second entry NaN when the row has
 *   one slack (Dict{Int,Vector{Float64}} of subproblem.jl:495-505);  status: enum above.
 * INFEASIBLE -> all outputs zero (subproblem.jl:532-536). */
int asm_sublp_solve(asm_handle* h, const double* dE, const double* df, double f, const double* E,
                    const double* x_k, double delta, int feasibility,
                    double* p, double* lambda, double* mult_x_U, double* mult_x_L, double* p_slack,
                    int32_t* status);

/* Split form of the same call for callers that keep the evaluation results resident in HBM:
 * upload once (or write the device buffers directly), then solve from device-resident inputs.
 * asm_sublp_solve == asm_sublp_upload + asm_sublp_solve_resident. */
int asm_sublp_upload(asm_handle* h, const double* dE, const double* df, double f, const double* E,
                     const double* x_k);
int asm_sublp_solve_resident(asm_handle* h, double delta, int feasibility,
                             double* p, double* lambda, double* mult_x_U, double* mult_x_L, double* p_slack,
                             int32_t* status);

/* The LP itself, in the form an MOI `external_optimizer` receives it from the UNMODIFIED reference (subproblem.jl:250-484):
 * after asm_sublp_setup has fixed the skeleton (row kinds -> row types and slack layout of create_model!, subproblem.jl:83-214),
 *   min q'p + w's   s.t.  J_i p + (slack terms of row i) (= | >= | <=) r_i ,  lb <= p <= ub (finite) ,  s >= slo
 * with J from dE (j_str order), r of length m + n_adj (rows m.. = the extra `<=` rows of range constraints, subproblem.jl:200-214).
 * use_slacks = 0: all slack columns fixed at 0 (normal phase, subproblem.jl:410-423), w / slo ignored.
 * Outputs: p[n], s[n_slack] (may be NULL), y[m + n_adj] row duals in the MOI sign convention, z[n] = q - J'y reduced costs,
 * bound_state[n] (-1 at lower, +1 at upper, 0 between; may be NULL), status.  This is what AsmHip.Optimizer calls
 * from MOI.optimize!; asm_sublp_solve is the same solve with the formulation done inside the library. */
int asm_lp_solve(asm_handle* h, const double* dE, const double* q, const double* r, const double* lb, const double* ub,
                 int use_slacks, const double* w, const double* slo,
                 double* p, double* s, double* y, double* z, int32_t* bound_state, int32_t* status);

/* Active set of the last OPTIMAL solve, as the reference could observe it from the LP solution:
 * row_state[m+nadj]: 1 active / 0 inactive (rows m.. are the extra `<=` rows of range constraints,
 * in the order of `adj`, subproblem.jl:200-214); bound_state[n]: -1 at lower, +1 at upper, 0 free;
 * slack_state[nslack]: 1 basic / 0 at its bound (all 0 in the normal phase).
 * Any pointer may be NULL.  n_rows/n_slack receive the array lengths. */
int asm_sublp_active_set(const asm_handle* h, int32_t* row_state, int32_t* bound_state, int32_t* slack_state,
                         int64_t* n_rows, int64_t* n_slack);

/* Drop the retained active sets (the analogue of GLPK's retained basis, slp.jl:38-40). */
int asm_sublp_reset_warm(asm_handle* h);

/* The other retained state of the normal phase: the columns J (0-based) whose projections span null(A_EF) - the null-space form's
 * counterpart of a simplex basis (its complement holds a basis of the equality rows).  k = 0 when the form is not in use.
 * J may be NULL to query k. */
int asm_sublp_ns_basis(const asm_handle* h, int32_t* J, int64_t* k);
/* Observability of the row order of the factorisations (nothing in the reference; oracle/lp_solver.py: rcm_order, row_order): the M rows
 * of the internal LP (m constraint rows, then the extra <= rows of the range constraints) by position in the reverse Cuthill-McKee
 * order of their coupling graph (perm[q] = row at position q; *band = half-bandwidth of their Gram matrix in that order, 0 = natural
 * order in use and perm untouched) and the hard equality rows of the null-space form in their own order (e_rows, *n_e of them, *e_band;
 * *n_e = 0 when the form is not available).  perm / e_rows may be NULL. */
int asm_sublp_row_order(const asm_handle* h, int32_t* perm, int64_t* band, int32_t* e_rows, int64_t* n_e, int64_t* e_band);

/* Statistics of the last solve / accumulated device-kernel timing. */
typedef struct {
    int32_t path;          /* 0 warm, 1 ipm stage0+polish, 2 stage1, 3 stage2, 4 ipm+face (non-unique optimum: least-norm point of the optimal
                            * face + basic multipliers), 5 unpolished (status OTHER), 6 infeasible (IPM duals), 7 infeasible (phase-1 duals),
                            * 8 jammed ipm + polish, 9 ipm+ref (non-unique optimum, projection of the iterate: fallback of 4),
                            * 10 ipm-conv (no active-set solve passed its test, the iterate converged to 1e-10 in all measures is the answer) */
    int32_t polished;
    int32_t ipm_iters;
    int32_t nfact;         /* Cholesky factorisations */
    int32_t eqp;           /* active-set (EQP) solves */
    int32_t M, n, ns;      /* LP rows, columns, slack columns */
    int32_t col_iters;     /* interior-point iterations that factored the n x n column form (restoration LPs) */
    int32_t ns_iters;      /* interior-point iterations that factored the k x k null-space form (normal-phase LPs with many equality rows) */
    int32_t ns_dim;        /* k = dimension of null(A_EF) when that form was set up, else 0 */
    int32_t ns_cold;       /* 1: the basis columns were selected from scratch in this LP (0: the previous LP's columns were re-used) */
    int32_t restored;      /* 1: no interior-point stage ended in a successful polish and the last stage ended 10x worse than the best one - the best
                            * iterate was brought back for the final attempts (best-iterate safeguard) */
    int32_t ns_path;       /* what made the basis of the null-space form in this LP: 1 the previous LP's basis re-projected, 2 the retained basis
                            * columns, 3 the cold selection; 0: the form is not in use (the field fills what was padding: the layout is unchanged) */
    double  ipm_pinf, ipm_dinf, ipm_gap;
    double  kkt_pr, kkt_du;
    double  wall_ms;       /* host wall time of the solve */
} asm_solve_stats;
int asm_sublp_last_stats(const asm_handle* h, asm_solve_stats* out);

/* Device time per kernel family, measured with HIP events on the handle's stream. */
/* ASM_K_SYRK: the Schur build; ASM_K_CHOL / ASM_K_TRSV: whole factorisation / solve (many launches);
 * ASM_K_SYRK_KERNEL: every single launch of the rank-K MFMA kernels k_syrk_upd (Cholesky updates) and k_syrk<T> (Schur builds). */
/* ASM_K_PANEL_KERNEL: every single launch of the dataflow panel kernels k_chol_panel / k_chol_panel_solo (the 64-wide steps of the Cholesky
 * factorisations: the dependent chain the path is bound by since round 3). */
enum { ASM_K_ASSEMBLE = 0, ASM_K_SCALE, ASM_K_GEMV, ASM_K_SYRK, ASM_K_CHOL, ASM_K_TRSV, ASM_K_SYRK_KERNEL, ASM_K_PANEL_KERNEL, ASM_K_COUNT };
typedef struct {
    double  ms[ASM_K_COUNT];      /* accumulated device milliseconds */
    int64_t calls[ASM_K_COUNT];   /* number of timed regions */
    double  flops[ASM_K_COUNT];   /* algorithmic flops issued */
    double  bytes[ASM_K_COUNT];   /* algorithmic bytes moved */
} asm_kernel_stats;
int asm_kernel_stats_get(asm_handle* h, asm_kernel_stats* out);
int asm_kernel_stats_reset(asm_handle* h);
/* 0: no HIP-event timing; 1: every launch of the rank-K and panel kernels (ASM_K_SYRK_KERNEL, ASM_K_PANEL_KERNEL); 2: every family
 * (perturbs latency-bound workloads).  Default from the environment (ASM_HIP_TIMING), else 1. */
int asm_kernel_timing(asm_handle* h, int level);

/* ---- per-iteration reductions that consume J, lambda already in HBM (common.jl:35-44) ----------- */
/* KT_residuals(df, lambda, mult_x_U, mult_x_L, J) with J = the Jacobian assembled by the last
 * upload/solve on this handle. */
int asm_kt_residuals(asm_handle* h, const double* df, const double* lambda,
                     const double* mult_x_U, const double* mult_x_L, double* out);
/* per-row 2-norms of the assembled Jacobian (compute_nu!, slp.jl:54-66). */
int asm_jac_row_norms(asm_handle* h, double* out_m);

/* ---- device-side evaluators: eval_functions! (slp.jl:186-191) without the host ------------------------------------
 * The affine / quadratic evaluator of the MOI wrapper (MOI_wrapper.jl:776-944) on a flattened function store, plus one
 * optional NLP block kernel; Jacobian values are written straight into the handle's dE buffer in the j_str order given to
 * asm_sublp_setup (which must precede this call).  Rows 0..n_rows-1 are the constraint functions in the wrapper's block
 * order (linear <=, >=, ==, quadratic <=, >=, ==; MOI_wrapper.jl:683-689), row n_rows is the objective (MOI_wrapper.jl:809-820).
 *   aff_ptr/quad_ptr [n_rows+2]  term ranges per row;  aff_var, q_v1, q_v2: 0-based variables;  constant [n_rows+1]
 *   jac_off [n_rows+1]           offset of each row's values in dE (affine terms, then per quadratic term 1 or 2 values:
 *                                fill_constraint_jacobian!, MOI_wrapper.jl:889-918)
 *   g_ptr [n+1], g_kind, g_coef, g_other   per-variable contributions to the objective gradient in term order
 *                                (fill_gradient!, MOI_wrapper.jl:827-850; kind 0: += coef, 1: += coef * x[other])
 *   objective_scale              +1 MIN, -1 MAX, 0 FEASIBILITY (MOI_wrapper.jl:1037-1054)
 *   nlp_kind                     0 none; 1 Ohm's-law rows of the polar ACOPF model (4 rows and 20 values per branch;
 *                                ipar = [n_branch, va0, vm0, pf0, pt0, qf0, qt0, f_bus.., t_bus..], dpar = 8 coefficient
 *                                arrays); 2 dense quadratic rows g = A x + 1/2 Q x^2 (dpar = A then Q, row-major);
 *                                3 expression block (below); 4 = kind 1 and 5 = kind 2 with second derivatives: the same ipar / dpar,
 *                                size checks, kernels and bits for values, Jacobian, asm_eval_set_data and every SLP launch - they
 *                                differ from kinds 1 and 2 only in that the derivative entries below accept them: they are the
 *                                block kernels with their derivative entries (the Hessian and the data derivatives)
 * The affine / quadratic part is bit-identical to the host evaluator (no fused multiply-add, the reference's term order).
 *
 * Expression block (nlp_kind = ASM_NLP_EXPR): the constraint and objective expressions of the reference's NLP block
 * (@NLconstraint / @NLobjective, MOI.constraint_expr / MOI.objective_expr) as a tape.
 *   R = nlp_rows constraint rows, then T >= 0 objective terms; each row / term is a list of nodes in SSA order, node = (op, a, b)
 *   with a / b the indices of EARLIER nodes of the same row or term, counted from its first node (0-based); its value is its
 *   last node.  Operands by op code:
 *     ASM_OP_CONST  a = index into dpar                 ASM_OP_VAR   a = variable (0-based)
 *     ASM_OP_ADD / SUB / MUL / DIV   a op b             ASM_OP_NEG   -a
 *     ASM_OP_POWI   a ^ b, b an integer, 1 <= |b| <= ASM_EXPR_MAX_POWI (|b| - 1 products left to right; 1 / that for b < 0)
 *     ASM_OP_SQRT / EXP / LOG / SIN / COS   of a        (b unused: 0)
 *     ASM_OP_ABS .. ASM_OP_CBRT   unary, of a (b unused: 0);  ASM_OP_POW .. ASM_OP_MAX   binary, a and b as for ADD..DIV
 *   Values and adjoints of the ops after COS (u = value of a, y = value of b, v = the node's value, w = the node's adjoint;
 *   "+=" is adj = adj + (the right side), each parenthesis one rounding, in this order):
 *     ABS    fabs(u)          adj[a] += w * copysign(1.0, u)           (+1 at +0.0, -1 at -0.0)
 *     TAN    tan(u)           adj[a] += w * (1 + v*v)
 *     ASIN   asin(u)          adj[a] += w / sqrt((1 - u) * (1 + u))    (not 1 - u*u: that cancels near +-1; 1 - u is exact for 1/2 <= u <= 2)
 *     ACOS   acos(u)          adj[a] -= w / sqrt((1 - u) * (1 + u))
 *     ATAN   atan(u)          adj[a] += w / (1 + u*u)
 *     SINH   sinh(u)          adj[a] += w * cosh(u)
 *     COSH   cosh(u)          adj[a] += w * sinh(u)
 *     TANH   tanh(u)          adj[a] += w * (1 - v*v)                  (1 - v*v cancels as |v| -> 1: the absolute error is that of v, a few eps - at u = 9, 1.6e7 eps of the result)
 *     LOG10  log10(u)         adj[a] += w / (u * ln10)                  (ln10, ln2: the doubles nearest to ln 10, ln 2)
 *     LOG2   log2(u)          adj[a] += w / (u * ln2)
 *     LOG1P  log1p(u)         adj[a] += w / (1 + u)
 *     EXPM1  expm1(u)         adj[a] += w * (v + 1)                    (v + 1 cancels as v -> -1: absolute error a few eps - at u = -20, 9e7 eps of the result)
 *     CBRT   cbrt(u)          adj[a] += w / (3 * (v*v))
 *     POW    pow(u, y)        adj[a] += w * (y * pow(u, y - 1));  then adj[b] += w * (v * log(u))  (a CONST b keeps it: its share of asm_eval_data_gradient, NaN or inf for u <= 0)
 *     ATAN2  atan2(u, y)      t = u*u + y*y;  adj[a] += (w * y) / t;  then adj[b] -= (w * u) / t   (Julia atan(a, b)).  Formed as
 *                             s = 2^-e, e the binary exponent of max(|u|, |y|) (kept within +-1000); us = u*s; ys = y*s; ts = us*us + ys*ys;
 *                             adj[a] += ((w * ys) / ts) * s;  adj[b] -= ((w * us) / ts) * s  - the same bits wherever u*u + y*y neither
 *                             underflows nor overflows, and the quotient itself where it does ((1e-200, 1e-200): 5e199, not inf)
 *     MIN    y < u ? y : u    w to the chosen operand: adj[b] += w if y < u, else adj[a] += w (ties and NaN go to a)
 *     MAX    y > u ? y : u    adj[b] += w if y > u, else adj[a] += w
 *   Domain errors (log of a negative number, asin outside [-1, 1], ...) give NaN or inf as the math library does.
 *   ipar = [R, T, L, ptr[R+T+1], op[L], a[L], b[L]] (ptr[0] = 0, ptr[R+T] = L, every row / term at least one node);
 *   dpar = the constants.
 *   Jacobian pattern: each row's distinct variables in ascending order, rows in order; nlp_nnz = the sum of their counts and
 *   the block's part of j_str (entries from jac_off[n_rows] on) must be exactly this pattern.
 *   T > 0: the objective is the sum of the T terms in term order (from 0.0), times objective_scale; it replaces the function
 *   store's objective row (has_objective of the reference's NLP block, MOI_wrapper.jl:809-861).  Gradient per variable: the
 *   adjoints of its VAR nodes summed in (term, node) order, times objective_scale.  Jacobian value: the adjoints of the row's
 *   VAR nodes of that variable, added in reverse node order.
 *   Derivatives are reverse-mode with fixed formulas and no fused multiply-add: with ADD..POWI, ABS, MIN and MAX only, device
 *   values equal the host twin (activesetmethods_amd/nlexpr.py) bit for bit; the other ops differ in the math library's last bits.
 *   A malformed tape (forward or out-of-row reference, unknown op, variable / constant out of range, bad POWI exponent, size
 *   mismatch, a pattern that differs from j_str) is rejected with ASM_ERR_ARG and the handle keeps its previous evaluator. */
enum { ASM_NLP_NONE = 0, ASM_NLP_ACOPF_OHM = 1, ASM_NLP_DENSE_QUADRATIC = 2, ASM_NLP_EXPR = 3, ASM_NLP_ACOPF_OHM_HESS = 4, ASM_NLP_DENSE_QUADRATIC_HESS = 5 };
enum { ASM_OP_CONST = 0, ASM_OP_VAR = 1, ASM_OP_ADD = 2, ASM_OP_SUB = 3, ASM_OP_MUL = 4, ASM_OP_DIV = 5, ASM_OP_NEG = 6, ASM_OP_POWI = 7,
       ASM_OP_SQRT = 8, ASM_OP_EXP = 9, ASM_OP_LOG = 10, ASM_OP_SIN = 11, ASM_OP_COS = 12,
       ASM_OP_ABS = 13, ASM_OP_TAN = 14, ASM_OP_ASIN = 15, ASM_OP_ACOS = 16, ASM_OP_ATAN = 17, ASM_OP_SINH = 18, ASM_OP_COSH = 19,
       ASM_OP_TANH = 20, ASM_OP_LOG10 = 21, ASM_OP_LOG2 = 22, ASM_OP_LOG1P = 23, ASM_OP_EXPM1 = 24, ASM_OP_CBRT = 25,
       ASM_OP_POW = 26, ASM_OP_ATAN2 = 27, ASM_OP_MIN = 28, ASM_OP_MAX = 29, ASM_OP_COUNT = 30 };
enum { ASM_EXPR_MAX_POWI = 64 };
int asm_eval_setup(asm_handle* h, int64_t n_rows, const int64_t* aff_ptr, const int64_t* aff_var, const double* aff_coef,
                   const int64_t* quad_ptr, const int64_t* q_v1, const int64_t* q_v2, const double* q_coef,
                   const double* constant, const int64_t* jac_off,
                   const int64_t* g_ptr, const int64_t* g_kind, const double* g_coef, const int64_t* g_other,
                   double objective_scale, int nlp_kind, int64_t nlp_rows, int64_t nlp_nnz,
                   const int64_t* nlp_ipar, int64_t n_ipar, const double* nlp_dpar, int64_t n_dpar);
/* f, df, E at x (returned) and dE (kept in HBM); equivalent to evaluating on the host + asm_sublp_upload. */
int asm_eval_functions(asm_handle* h, const double* x, double* f, double* df, double* E);
/* eval_f + eval_g at a trial point (line search / step quality); does not touch the inputs of the next LP. */
int asm_eval_constraints(asm_handle* h, const double* x, double* f, double* E);
/* copy of the dE buffer (tests). */
int asm_eval_jacobian_values(asm_handle* h, double* dE_out);

/* ---- NLP-block data: parameters of scenario and sensitivity studies ----------------------------------------------------------------
 * The data of the NLP block is its dpar as given to asm_eval_setup: kind 1 the 8 Ohm's-law coefficient arrays, kind 2 A then Q, kind 3
 * the tape constants (a binding that owns parameter slots - nlexpr.py puts them at dpar[0, P) - writes their values here).  The pattern
 * (ipar, j_str) never changes.
 * asm_eval_set_data: dpar[offset, offset + count) := values on the device, without a new asm_eval_setup.  ASM_ERR_STATE before
 * asm_eval_setup, ASM_ERR_ARG for a null pointer or a range outside [0, n_dpar).  No LP state changes (bounds, retained basis, hints);
 * every later evaluation (asm_eval_functions, asm_eval_constraints, the merit and line-search entries, asm_slp_run(_tr)) is bit-identical
 * to that of a handle set up from scratch with the changed dpar. */
int asm_eval_set_data(asm_handle* h, int64_t offset, int64_t count, const double* values);
/* The data gradient of the Lagrangian at (x, lambda), for expression blocks (kind 3) and for the block kernels with their derivative
 * entries (kinds 4 and 5: "Data derivatives of the block kernels" below); other kinds: ASM_ERR_ARG:
 *   out[c] = d f / d dpar[c] - sum_i lambda_i d g_i / d dpar[c]      c < n_dpar
 * f the objective as asm_eval_functions returns it (sense scale included), g the block's rows, lambda [m] in the sign convention of
 * asm_slp_run (KT residual df - J'lambda - mult_x_U - mult_x_L): at an SLP solution out is dV/d dpar, V the optimal value (envelope
 * theorem).  The inputs of the next LP are not touched (as asm_eval_constraints).
 * Order: per node of a row or term a reverse sweep from a unit seed at x (the derivative formulas above); the adjoint w of every CONST node
 * becomes one occurrence: (-lambda_r) * w for a node of block row r (problem row n_rows + r), objective_scale * w for a node of a term;
 * out[c] sums the occurrences of dpar index c from 0.0 in (row, then term; node) order - rows before terms, nodes ascending.  Device and
 * host twin (nlexpr.py: ExprBlock.data_gradient) agree bit for bit with ADD..POWI, ABS, MIN and MAX only, else in the last bits. */
int asm_eval_data_gradient(asm_handle* h, const double* x, const double* lambda, double* out);

/* ---- Cross derivatives of an expression block with respect to its data: how the stationarity and feasibility residuals of an SLP
 * solution move with dpar.  With L = f - lambda' g in the convention of asm_slp_run and asm_eval_data_gradient (f with the sense scale,
 * lambda [m]) and a direction dc [n_dpar] in the data:
 *   u [n] = d/d dpar (grad_x L) . dc        w [m] = (d g / d dpar) . dc    (0 for the rows of the function store: its constants are not data)
 * Expression blocks, and the block kernels with their derivative entries in the closed forms of the next section (other kinds:
 * ASM_ERR_ARG); ASM_ERR_STATE before asm_eval_setup, ASM_ERR_ARG for a null pointer.  The inputs of the
 * next LP are not touched (as asm_eval_constraints).  The per-variable occurrence list and the workspace are made by the first call after
 * asm_eval_setup.  A tape without CONST node: u = w = 0 without a launch.
 * Order: per row or term one forward-over-reverse sweep, the one of the Hessian (the statement tangents listed under "Hessian of the
 * Lagrangian" below, each parenthesis one rounding, no fused multiply-add) with another seed: a CONST node with operand a has the tangent
 * dc[a], every VAR node the tangent 0.  A CONST exponent of POW is a CONST node like any other: its tangent is dc[a], and the terms with it
 * (the "then" steps of POW below) enter where that tangent is nonzero.  Where it is 0 they are left out, not multiplied by 0: for u <= 0, where
 * log(u) is NaN or -inf, pow(u, 2.0) has finite u and w along every direction that leaves its exponent alone - and for a dc that is zero on
 * every exponent the results are those of a sweep that ignores exponents, bit for bit; a nonzero dc[a] at u <= 0 gives NaN or inf in that
 * row's or term's share of u and in its w.  w[n_rows + r] is the tangent of the last node of block row r.  The adjoint tangent z that reaches a
 * VAR node is one occurrence: (-lambda[n_rows + r]) * z for a node of block row r, objective_scale * z for a node of a term (one product).
 * u[j] sums the occurrences of variable j from 0.0 in this order: rows in row order, then terms in term order; inside a row or term its VAR
 * nodes of j in descending node order.  No atomics.  With ADD..POWI, ABS, MIN and MAX only, device and host twin (nlexpr.py:
 * ExprBlock.data_cross) agree bit for bit, else in the math library's last bits. */
int asm_eval_data_cross(asm_handle* h, const double* x, const double* lambda, const double* dc, double* u, double* w);

/* ---- Data derivatives of the block kernels: kinds 4 and 5 are the Ohm's-law and the dense quadratic kernel WITH THEIR DERIVATIVE ENTRIES -
 * besides the Hessian (below) the derivatives with respect to their own dpar, so that asm_eval_data_gradient, asm_eval_data_cross,
 * asm_solution_sensitivity(_multi) and asm_batch_data_gradient accept them as they accept kind 3, with the same conventions (L = f - lambda' g,
 * lambda in the sign convention of asm_slp_run, block row r = problem row n_rows + r) and the same errors.  Kinds 1 and 2 stay refused with
 * ASM_ERR_ARG.  Both blocks are linear in dpar and have no objective, so the derivatives are closed forms that never read dpar: the results
 * depend on (x, lambda) and the direction only, not on asm_eval_set_data or a scenario's data.  What the data gradient needs is made by
 * asm_eval_setup, the cross workspace (per-variable occurrence lists from ipar, occurrences, [u | w] per column) by the first cross call.
 * No fused multiply-add, no atomics; every written operation is one rounding, left to right.
 *   Ohm's-law block (kind 4), dpar = k_ff_p, k_ff_q, k_tt_p, k_tt_q, a_f, b_f, a_t, b_t (n_branch each) - the layout and the meaning of
 *   the 8 n_branch parameters of the same rows as an expression block with the coefficients as parameters.  Per branch l, vf, vt, d = va_f -
 *   va_t, cs = cos(d), sn = sin(d), vv = vf * vt as in the value kernel, l0..l3 the multipliers of its rows pfr, qfr, pto, qto (row = x_flow - F_r):
 *     data gradient out[q n_branch + l] = lambda_r dF_r/dc, with vf2 = vf*vf, vt2 = vt*vt, vvc = vv*cs, vvs = vv*sn:
 *       l0*vf2   l1*vf2   l2*vt2   l3*vt2   l0*vvc + l1*vvs   l0*vvs - l1*vvc   l2*vvc - l3*vvs   -(l2*vvs) - l3*vvc
 *     (one launch, one thread per branch; no sum runs across branches).
 *     cross derivatives along dc: F_r(dc) and the families dvf_r(dc), dvt_r(dc), dth_r(dc) are the value kernel's expressions for the flows
 *     and their derivatives with dc where dpar stands, e.g. F_pfr = k*vf*vf + a*vv*cs + b*vv*sn, evaluated left to right;
 *       w[n_rows + r n_branch + l] = -F_r(dc)
 *     and the branch has four occurrences in u, the sums in row order from the first term, ((l0*t0 + l1*t1) + l2*t2) + l3*t3:
 *       vm_f: sum_r lambda_r dvf_r     vm_t: sum_r lambda_r dvt_r     va_f: theta = sum_r lambda_r dth_r     va_t: -theta
 *     u[j] sums the occurrences of variable j from 0.0 by branch ascending and, inside a branch, in that slot order; a variable without one
 *     (flows, generators) gets 0.  A branch from a bus to itself needs no refusal here: its two occurrences of a variable add in slot order.
 *     Device and host twin (acopf.py: _ohm_data_twins) differ at most in the last bits of sin and cos.
 *   Dense quadratic block (kind 5), dpar = A then Q (m_blk x n, row-major), g_i = sum_j A_ij x_j + 1/2 Q_ij x_j^2:
 *     data gradient out[i n + j] = (-lambda_i) * x_j     out[m_blk n + i n + j] = (-lambda_i) * (0.5 * (x_j * x_j))
 *     cross derivatives along dc = (dA, dQ):  w[n_rows + i] = sum_j (dA_ij*x_j + 0.5*dQ_ij*x_j*x_j), one wavefront per row, lane-strided from
 *     0.0, then the xor tree of the value kernel;  u[j] = -(sum_i lambda_i * (dA_ij + dQ_ij * x_j)), i ascending from 0.0.  Gradient and u are
 *     bit-identical to the host twin (problems.py), w agrees to summation order.
 * asm_solution_sensitivity_multi on these kinds stages a chunk's directions once (one upload) and makes all its right-hand sides with one
 * launch of the cross kernel, one gather (kind 5: two launches) and one scatter into the chunk's blocks, the column in grid.y - in place of
 * one upload and three launches per direction.  Column c equals asm_eval_data_cross of that direction alone bit for bit, and a column's
 * answer depends on its own direction only.  The staging of a chunk is ASM_KKT_CHUNK x n_dpar doubles on the host and on the device, as for
 * every kind: for the dense block of the synthetic NLP with n = 1000, m = 500 (n_dpar = 10^6) that is 512 MB each. */

/* ---- Hessian of the Lagrangian: hessian_lagrangian_structure / eval_hessian_lagrangian (MOI_wrapper.jl:748-774, 946-978; eval_h_cb :1071-1083)
 *   H = obj_factor * objective_scale * hess f + sum_i lambda_i hess g_i        lambda [m], PLUS sign (the MOI convention, :960-978, :1080)
 * asm_slp_run's multipliers belong to df - J'lambda: the Hessian of that Lagrangian is this one at (obj_factor 1, -lambda).
 * Valid after asm_eval_setup (ASM_ERR_STATE before) for the function store alone (nlp_kind 0), with an expression block (kind 3), with the
 * Ohm's-law block announced as ASM_NLP_ACOPF_OHM_HESS (kind 4) or the dense quadratic block as ASM_NLP_DENSE_QUADRATIC_HESS (kind 5); kinds 1
 * and 2 and null pointers: ASM_ERR_ARG.  The calls do not touch the inputs of the next LP, the retained basis or hints (as
 * asm_eval_constraints).  Pattern, lists and workspace are made by the first of these calls after asm_eval_setup.
 * Pattern (rows, cols 1-based; an off-diagonal entry (i, j) stands for both symmetric positions; duplicates add), in this order:
 *   1. function store, as the reference: the objective row's quadratic terms (only when the block has no objective, T == 0), then the
 *      quadratic rows in row order; one entry per stored term, (q_v1 + 1, q_v2 + 1) as given - not sorted, not brought to one triangle,
 *      duplicates kept.  Value = factor * q_coef, factor = obj_factor * objective_scale (one product) or lambda[row].
 *   2. expression block: the distinct pairs (i, j), i >= j, sorted by (i, j), of the union over rows and terms of each one's interaction set
 *      P(last node).  With L(k) the variables node k depends on:
 *        CONST, VAR: P = {}        ADD SUB NEG MIN MAX: P(a) u P(b)        MUL: P(a) u P(b) u L(a) x L(b)
 *        DIV: P(a) u P(b) u L(a) x L(b) u L(b) x L(b)        POWI with exponent 1: P(a)        POW ATAN2: (L(a) u L(b))^2
 *        every other unary op and POWI: P(a) u L(a) x L(a)
 *      (pairs unordered, stored with the larger index first).
 *   Value of a block entry (i, j): the sum from 0.0, in (row, then term) order, of wt * h over the rows and terms whose interaction set
 *   holds the pair; wt = lambda[n_rows + r] for row r, obj_factor * objective_scale for a term; h = d2(row) / dx_i dx_j by forward over
 *   reverse with seed j: the forward sweep carries the tangent d of every node value for x' = e_j, the reverse sweep the tangent z of every
 *   adjoint, and h is the adjoint tangent that reaches the VAR nodes of variable i (several VAR nodes: added in reverse node order from 0.0).
 *   The formulas are the tangents of the first-order statements, statement by statement (u, y, v, w as above; du, dy, d = tangents of u, y,
 *   v; z = tangent of w; "tadj" the adjoint tangents; each parenthesis one rounding, no fused multiply-add):
 *     ADD  d = du + dy                     tadj[a] += z;  tadj[b] += z           (SUB: d = du - dy, tadj[b] -= z;  NEG: d = -du, tadj[a] -= z)
 *     MUL  d = du*y + u*dy                 tadj[a] += (z*y + w*dy);  tadj[b] += (z*u + w*du)
 *     DIV  d = (du - v*dy) / y             t = w/y;  dt = (z - t*dy) / y;  tadj[a] += dt;  tadj[b] -= (dt*v + t*d)
 *     POWI d = d1*du                       tadj[a] += (z*d1 + w*(d2*du)),  d1 as the first order, d2 = e (e-1) u^(e-2): ((double)e * (double)(e-1))
 *                                          times the product of |e| - 2 factors u from 1.0 (e >= 2), 0.0 (e = 1), ee / ((u^|e| * u) * u) (e < 0)
 *     SQRT d = (0.5*du) / v                s = (0.5*w) / v;  tadj[a] += (0.5*z - s*d) / v
 *     EXP  d = du*v                        tadj[a] += (z*v + w*d)
 *     LOG  d = du / u                      q = w/u;  tadj[a] += (z - q*du) / u
 *     SIN  d = du*cos(u)                   tadj[a] += (z*cos(u) - w*(sin(u)*du))
 *     COS  d = -(du*sin(u))                tadj[a] -= (z*sin(u) + w*(cos(u)*du))
 *     ABS  d = du*copysign(1.0, u)         tadj[a] += z*copysign(1.0, u)                                       (zero curvature)
 *     TAN  d = du*(1 + v*v)                g = 1 + v*v;  tadj[a] += (z*g + w*(2*(v*d)))
 *     ASIN d = du / sqrt((1 - u)*(1 + u))  r = sqrt((1 - u)*(1 + u));  q = w/r;  dr = -((u*du) / r);  tadj[a] += (z - q*dr) / r      (ACOS: d, tadj negated)
 *     ATAN d = du / (1 + u*u)              g = 1 + u*u;  q = w/g;  tadj[a] += (z - q*(2*(u*du))) / g
 *     SINH d = du*cosh(u)                  tadj[a] += (z*cosh(u) + w*(sinh(u)*du))
 *     COSH d = du*sinh(u)                  tadj[a] += (z*sinh(u) + w*(cosh(u)*du))
 *     TANH d = du*(1 - v*v)                g = 1 - v*v;  tadj[a] += (z*g - w*(2*(v*d)))
 *     LOG10 d = du / (u*ln10)              g = u*ln10;  q = w/g;  tadj[a] += (z - q*(du*ln10)) / g                            (LOG2: ln2)
 *     LOG1P d = du / (1 + u)               g = 1 + u;  q = w/g;  tadj[a] += (z - q*du) / g
 *     EXPM1 d = du*(v + 1)                 g = v + 1;  tadj[a] += (z*g + w*d)
 *     CBRT d = du / (3*(v*v))              g = 3*(v*v);  q = w/g;  tadj[a] += (z - q*(6*(v*d))) / g
 *     POW  p1 = pow(u, y-1), p2 = pow(u, y-2), lu = log(u), A = y*p1, B = v*lu;  d = du*A, then d = d + dy*B;
 *          dp1 = du*((y-1)*p2), then dp1 = dp1 + dy*(p1*lu);  dA = y*dp1, then dA = dA + dy*p1;  tadj[a] += (z*A + w*dA);
 *          dB = d*lu + v*(du/u);  tadj[b] += (z*B + w*dB).  A CONST b in the Hessian: every "then" step and the statements on b are left out
 *          (asm_eval_data_cross and asm_eval_data_cross_t say what they do with it).  TANH and EXPM1 carry the cancellation of their first-order
 *          statements: absolute errors of a few eps (1 + v*v) * 2|v| and a few eps (|v| + 1).
 *     ATAN2 t = u*u + y*y;  d = (du*y)/t - (dy*u)/t;  dt = 2*(u*du) + 2*(y*dy);  qa = (w*y)/t;  qb = (w*u)/t;
 *          tadj[a] += ((z*y + w*dy) - qa*dt) / t;  tadj[b] -= ((z*u + w*du) - qb*dt) / t  - formed with s, us, ys, ts of the first order:
 *          d = ((du*ys)/ts)*s - ((dy*us)/ts)*s;  dts = 2*(us*du) + 2*(ys*dy);  tadj[a] += (((z*ys + (w*dy)*s) - qa*dts) / ts) * s, b alike:
 *          the same bits wherever nothing underflows or overflows
 *     MIN / MAX  d and z follow the chosen operand (same tie rule)
 *   With ADD..POWI, ABS, MIN and MAX only, device values equal the host twin (nlexpr.py: ExprBlock.hessian_values) bit for bit.
 *   3. Ohm's-law block (kind 4), in place of 2.: every row of a branch is F = k_f vf^2 + k_t vt^2 + vf vt (P cos d + Q sin d), d = va_f - va_t,
 *      with (P, Q | k_f, k_t) = pfr (a_f, b_f | k_ff_p, 0), qfr (-b_f, a_f | k_ff_q, 0), pto (a_t, -b_t | 0, k_tt_p), qto (-b_t, -a_t | 0, k_tt_q);
 *      the row is x_flow - F, so its weight is w = -lambda.  Per branch, each product and each sum one rounding, left to right:
 *        Kf = w_pfr k_ff_p + w_qfr k_ff_q        Kt = w_pto k_tt_p + w_qto k_tt_q
 *        Pw = w_pfr a_f - w_qfr b_f + w_pto a_t - w_qto b_t        Qw = w_pfr b_f + w_qfr a_f - w_pto b_t - w_qto a_t
 *        b = Pw cos d + Qw sin d        r = Qw cos d - Pw sin d
 *      and the branch's ten occurrences, in this order:
 *        (vf,vf) 2 Kf   (vt,vt) 2 Kt   (vf,vt) b   (vf,va_f) vt r   (vf,va_t) -(vt r)   (vt,va_f) vf r   (vt,va_t) -(vf r)
 *        (va_f,va_f) -((vf vt) b)   (va_t,va_t) -((vf vt) b)   (va_f,va_t) (vf vt) b
 *      Pattern: the distinct pairs, larger index first, sorted by (i, j) - the block part of the pattern the same rows give as an
 *      expression block.  Value of an entry: the sum from 0.0 of its occurrences by branch ascending and, inside a branch, in the order
 *      above (parallel branches and branches that share a bus add into one entry).  The flow variables are linear and the block has no
 *      objective: obj_factor does not enter.  A branch whose two ends are the same bus is refused by the first Hessian call (ASM_ERR_ARG).
 *      Device and host twin (acopf.py) differ in the last bits of sin and cos only.
 *   4. dense quadratic block (kind 5), in place of 2.: the n diagonal entries (j, j), j ascending, whatever Q holds; value
 *      sum_i lambda[n_rows + i] Q_ij over i ascending from 0.0 (one product and one sum per term): bit-identical to the host twin.
 * asm_eval_hessian_structure: *nnz and, unless rows == cols == NULL, the pattern.
 * asm_eval_hessian_lagrangian: values [nnz] at (x, obj_factor, lambda).
 * asm_eval_hessian_product: out [n] = H v from those values: out[i] sums, from 0.0 and in entry order over all nnz entries, value * v[other
 * index] of the entries that name i (an off-diagonal entry contributes to both of its indices).  No atomics anywhere. */
int asm_eval_hessian_structure(const asm_handle* h, int64_t* nnz, int64_t* rows, int64_t* cols);
int asm_eval_hessian_lagrangian(asm_handle* h, const double* x, double obj_factor, const double* lambda, double* values);
int asm_eval_hessian_product(asm_handle* h, const double* x, double obj_factor, const double* lambda, const double* v, double* out);

/* ---- The KKT solve on a working set: the equality-constrained QP behind solution sensitivities and behind the step of SLP-EQP.
 * With F = {j : bound_state[j] = 0} (the free variables, B its complement), W = {i : row_state[i] = 1} (the working rows), H the Hessian of
 * f - lambda' g at x (what asm_eval_hessian_lagrangian(x, 1.0, -lambda) gives), J the Jacobian at x and A = J[W, F], asm_kkt_solve solves
 *   H_FF dx_F - A' dlam_W = -ru_F ,    A dx_F = -rw_W ,    dx_B = 0 ,    dlam_i = 0 (i not in W) ,
 *   dz_B = (H dx)_B + ru_B - (J_W' dlam_W)_B ,    dz_F = 0                       (dz may be NULL)
 * Valid where the Hessian calls are: nlp_kind 0, 3, 4 or 5 after asm_eval_setup (ASM_ERR_STATE before); kinds 1 and 2, a null pointer, a state
 * outside its value set (row_state 0 / 1, bound_state -1 / 0 / +1), |W| > |F| and par with max_iter < 0 or rtol not >= 0: ASM_ERR_ARG.
 * par == NULL: max_iter = 2 (|F| - |W|) + 20, rtol = 1e-12.
 * info.status is a result, not an error (the call returns ASM_OK and the handle works on):
 *   0 solved   1 iteration limit   2 the reduced Hessian is not positive definite (p'Hp <= 0 met; the outputs are the iterate reached)
 *   3 dependent working rows (dropped_pivots > 0; the answer is the least-squares one of the remaining rows)
 * cg_iters, n_free = |F|, n_rows = |W|; res_stat / res_feas: the infinity norms of H_FF dx_F - A' dlam_W + ru_F and of A dx_F + rw_W for
 * the returned solution.
 * Everything runs on the handle's stream in buffers of the solve's own, which live as long as the evaluator (until the next asm_eval_setup,
 * asm_sublp_setup or asm_destroy): the
 * inputs of the next LP (dE, df, E, x_k), the retained basis, hints and active sets and the solver's factors do not change.  In the
 * default form, described here, A and S = A A' are dense; asm_kkt_set_form (below, "The form of the KKT solve") selects a sparse form
 * with sparse products and a banded factor.
 * Method:
 *   1. the Hessian values at (x, 1, -lambda), once; the Jacobian at x into a value buffer and a dense J of the solve's own
 *   2. A gathered into a dense |W| x ldn operand with the columns of B zeroed; S = A A' by the rank-K build, factored by the library's
 *      Cholesky with its static pivot guard (a pivot <= 1e-10 of its diagonal entry is dropped: its row leaves the solves)
 *   3. particular solution dx0 = -A' S^-1 rw_W, with one refinement step of that normal-equation solve (dx0 -= A' S^-1 (A dx0 + rw_W))
 *   4. projected conjugate gradients on null(A) for  min 1/2 d' H_FF d + (ru_F + H_FF dx0)' d :  P v = v - A' S^-1 A v, applied twice per
 *      iteration; r0 = ru_F + H_FF dx0, g = P P r, p = -g; then  alpha = r'g / p'Hp, d += alpha p, r += alpha H p, g+ = P P r,
 *      beta = r'g+ / r'g, p = -g+ + beta p.  The residual is kept projected (r := g after every projection, the same iteration in exact
 *      arithmetic): its component in range(A') would otherwise stay as large as the right-hand side and the rounding of the normal-equation
 *      solves, cond(A A') times the unit roundoff of that component, would bound what ||g|| can reach.  Stop at ||g||_2 <= rtol ||g0||_2, at once when g0 = 0 or |F| = |W| (a vertex), with status 2
 *      when p'Hp <= 0.  H p is the Hessian product kernel on the values of step 1 with p zero on B.  alpha, beta and the curvature
 *      test stay on the device; the host reads one stop word per iteration.
 *   5. dx_F = dx0 + d;  dlam_W = S^-1 A q with q = H_FF dx_F + ru_F, and one refinement step dlam_W += S^-1 A (q - A' dlam_W);
 *   6. dz and the residual norms.
 * Sensitivity to constraint bounds needs no further entry: for a working row i whose bound moves by d(bound_i), call with ru = 0 and
 * rw_i = -d(bound_i) (the loads of the ACOPF scenarios are such bounds). */
typedef struct { int32_t max_iter; double rtol; } asm_kkt_params;
typedef struct {
    int32_t status, cg_iters, n_free, n_rows, dropped_pivots;
    double res_stat, res_feas;
} asm_kkt_info;
int asm_kkt_solve(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state,
                  const double* ru, const double* rw, const asm_kkt_params* par, double* dx, double* dlam, double* dz, asm_kkt_info* info);
/* Solution sensitivity of a block's data: asm_eval_data_cross(x, lambda, dc) followed by asm_kkt_solve(ru = u, rw = w).  At an
 * SLP solution with its working set, dx = (dx* / d dpar) . dc and dlam = (dlambda* / d dpar) . dc.  Expression blocks and the block
 * kernels with their derivative entries (kinds 3, 4, 5). */
int asm_solution_sensitivity(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state,
                             const double* dc, const asm_kkt_params* par, double* dx, double* dlam, double* dz, asm_kkt_info* info);

/* ---- Many right-hand sides on one factor: sensitivity matrices.
 * asm_kkt_solve_multi solves the KKT system above for nrhs right-hand sides at once; asm_solution_sensitivity_multi does so for nrhs
 * directions of the data.  All matrices are row-major with one right-hand side per row: RU, DX, DZ are nrhs x n, RW, DLAM nrhs x m, DC
 * nrhs x n_dpar, info has nrhs entries, and row c of DX / DLAM / DZ / info answers row c of RU / RW (of DC).  DZ may be NULL.
 * Validity, argument errors and defaults are asm_kkt_solve's (asm_solution_sensitivity's); nrhs < 1: ASM_ERR_ARG.  par, and the default
 * max_iter = 2 (|F| - |W|) + 20 and rtol = 1e-12, hold for every column.  For scenario batches: "Scenario batches: KKT solves and sensitivities" below.
 * Per column the mathematics is the method above, step by step.  Steps 1 and 2 - the Hessian values, the Jacobian, the gather, its
 * transposed copy, the rank-K build, the factorisation and the dropped-pivot count - run once per call.  Steps 3 to 6 run on blocks of
 * ASM_KKT_CHUNK columns; the factor and everything of steps 1 and 2 stay across the chunks, so memory is bounded whatever nrhs.
 *   One method, two product back ends: the set-up of steps 1 and 2, the driver of steps 3 to 6 and the element-wise and reduction kernels
 *   are the same code for asm_kkt_solve and for the multi entries - asm_kkt_solve is that driver on blocks of one column.  Only the
 *   products with H, A and A' and the substitutions with S differ: asm_kkt_solve and asm_solution_sensitivity use matrix-vector kernels
 *   and the factor's own substitution, the multi entries the block forms below.  The entry point chooses, never nrhs.
 *   Layout: a block holds its columns as rows, pitch ldn over the variables and round_up(min(m, n), 32) over the working rows.  The
 *   products with A and A' are k_gemm_nt launches on the matrix cores (T = V Aw', V = Y AwT'), the substitutions Dev::trsm_rows with the
 *   factor's wide-block inverses and its transposed copy.  Systems of every order take this path: the one-workgroup small solve serves one
 *   right-hand side and is not used.  H V is one launch that reads each Hessian entry once for all columns of the chunk; per column its
 *   sum is asm_eval_hessian_product's, bit for bit.  (J_W' dlam_W)_B comes from a second, unmasked transposed gather of the working rows.
 *   Lockstep iteration: the columns are independent conjugate-gradient iterations that advance together - no block method.  Each has its
 *   own alpha, beta, ||g0||, stop code and iteration count in HBM.  A column that has converged, has g0 = 0 or has met p'Hp <= 0 is
 *   frozen: no kernel writes its d, r or p again, and it leaves the active count in the round in which it stops (the curvature stop too).  The loop ends when no column is active or after max_iter rounds; a column still active
 *   then has status 1.  The host reads one word per round, the number of active columns, written by the workgroup that finishes the
 *   last column (through the host-mapped scalar block; by copy and synchronisation under ASM_HIP_SPIN=0).
 *   info[c]: the column's status, cg_iters, res_stat, res_feas; n_free, n_rows and dropped_pivots are the call's (dropped pivots: status 3
 *   in every column).
 *   Column independence: a column's outputs depend on its own right-hand side and the handle's data only - not on nrhs, not on its place,
 *   not on the other columns - bit for bit.  Every nrhs >= 1 takes the same kernels, every sum runs in an order fixed by the matrix
 *   dimensions, and the rows of a block beyond the chunk's columns are never part of a launch.  Against asm_kkt_solve the agreement is to
 *   tolerance: the summation orders of the two back ends' products differ.
 * asm_solution_sensitivity_multi makes (u, w) of each direction with the cross-derivative sweep of asm_eval_data_cross - one launch set per
 * direction, written straight into the chunk's blocks, no synchronisation between directions - and then runs the same solve (kinds 4
 * and 5: one launch set per chunk, "Data derivatives of the block kernels").
 * The buffers are made at the first multi call and released with asm_kkt_solve's; a handle that calls asm_kkt_solve alone holds blocks
 * of one column.
 * When to use it: a lockstep round launches block products whose time does not shrink with the number of columns, live or frozen - on
 * the case300-sized ACOPF a round costs about seven single-column iterations.  Below about 8 columns a loop of asm_kkt_solve /
 * asm_solution_sensitivity calls is faster; from there on the multi entries win, 4.5 times at 32 columns and 12.7 times at 64.
 * Bound sensitivities for a set of working rows: RU = 0 and RW[c, i_c] = -1 for the row i_c of column c (the recipe above).
 * asm_bound_sensitivity_multi is that recipe without the matrices: column c is asm_kkt_solve_multi with ru = 0 and rw[rows[c]] = -delta[c]
 * (delta == NULL: -1.0), bit for bit - DX, DLAM, DZ and info.  rows: nrhs 0-based row indices, duplicates allowed; an index outside [0, m),
 * or rows == NULL, is ASM_ERR_ARG.  A row outside the working set gives the zero column: status 0, no iteration, exact zeros.  A chunk's
 * right-hand sides are made on the device (k_kktm_bound_rhs: every entry cleared, and the thread whose place in the working-row list
 * holds rows[c] stores -delta[c]) from one upload of 12 bytes per column - nothing of length n or m is staged.  A derivative entry like
 * asm_solution_sensitivity_multi: the exact Hessian whatever asm_hessian_set_type chose, and that entry's refusals.
 * Variable-bound sensitivities: the bounds of variables in B move by delta, a vector supported on B, so dx_B = delta.  (dx_F, dlam, dz) is
 * the solve with ru = H delta over all n entries and rw = J delta on W, then dx += delta; the solve's own dz is already right (ru on B
 * carries H_BB delta).  asm_var_bound_sensitivity_multi is that recipe without the matrices: column c moves the bound of variable vars[c]
 * by delta[c] (delta == NULL: 1.0) and equals asm_kkt_solve_multi with RU[c] = delta[c] H[:, j], RW[c] = delta[c] J[:, j] bit for bit in
 * DLAM, DZ, info and DX, except that DX[c, j] = delta[c].  vars: nrhs 0-based variable indices, duplicates allowed; an index outside
 * [0, n), or vars == NULL, is ASM_ERR_ARG.  A variable outside B (bound_state[j] == 0) gives the zero column: status 0, no iteration,
 * exact zeros.  A chunk's right-hand sides are made on the device from one upload of 12 bytes per column - nothing of length n or m is
 * staged: k_kktm_var_unit writes the unit block, the chunk's Hessian product (the kernel of the solve's own products, its summation
 * order) gives H[:, j], k_kktm_var_rhs multiplies by delta[c] - one multiplication, no fused multiply-add - and reads J[wrow[q], j] from
 * the matrix the form itself uses: the solve's dense J, or (sparse form, k_kkts_var_col) the CSR values through the pattern's CSC column j
 * and the position list, rows outside W skipped, in both row orders.  After the finish step k_kktm_var_dx stores dx[j] = delta[c].  A
 * derivative entry with the refusals of asm_bound_sensitivity_multi; the function store alone (nlp_kind 0) is served. */
#define ASM_KKT_CHUNK 64
int asm_kkt_solve_multi(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state,
                        int32_t nrhs, const double* RU, const double* RW, const asm_kkt_params* par, double* DX, double* DLAM, double* DZ,
                        asm_kkt_info* info);
int asm_solution_sensitivity_multi(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state,
                                   const int32_t* bound_state, int32_t nrhs, const double* DC, const asm_kkt_params* par, double* DX,
                                   double* DLAM, double* DZ, asm_kkt_info* info);
int asm_bound_sensitivity_multi(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state,
                                int32_t nrhs, const int32_t* rows, const double* delta /* [nrhs], or NULL: 1.0 */, const asm_kkt_params* par,
                                double* DX, double* DLAM, double* DZ, asm_kkt_info* info);
int asm_var_bound_sensitivity_multi(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state,
                                    const int32_t* bound_state, int32_t nrhs, const int32_t* vars, const double* delta /* [nrhs], or NULL: 1.0 */,
                                    const asm_kkt_params* par, double* DX, double* DLAM, double* DZ, asm_kkt_info* info);

/* ---- Validity ranges: how far a sensitivity column may be followed before the working set changes.
 * The sensitivity entries return derivatives (dx, dlam, dz) on a fixed working set W, B.  asm_sensitivity_range_multi returns, per column,
 * the interval [t_lo, t_hi] of t on which x + t dx, lambda + t dlam, z + t dz keep that working set to first order: the ranging output of
 * LP and QP codes.  The rule uses E + t V with V = J dx; it is exact for affine rows and a quadratic objective, the linearised range else.
 *   Inputs: x [n], lambda [m], z [n] (z = mult_x_U + mult_x_L, read on B only), row_state [m] in {0, 1}, bound_state [n] in {-1, 0, +1};
 *   the problem's bounds g_L, g_U, x_L, x_U as asm_sublp_set_bounds left them; E = g(x) and J at x, evaluated by the entry; per column c
 *   row c of DX [nrhs x n], DLAM [nrhs x m], DZ [nrhs x n].  Signs are the drivers': lambda_i >= 0 at g_L, <= 0 at g_U, z_j >= 0 at a
 *   lower bound, <= 0 at an upper bound.
 *   For sg = +1 (the upper range) and sg = -1 (the lower one) the candidates are visited in position order - rows 0 .. m - 1, then
 *   variable j at position m + j - with v = sg V_i, dl = sg dlam_i, vx = sg dx_j, dv = sg dz_j:
 *     row i outside W:  if v < 0 and g_L_i > -inf: (g_L_i - E_i) / v, kind 1; else if v > 0 and g_U_i < inf: (g_U_i - E_i) / v, kind 2
 *     row i in W, g_L_i != g_U_i:  upper = !(g_L_i > -inf) || (g_U_i < inf && |E_i - g_U_i| < |E_i - g_L_i|);
 *                       if (upper ? dl > 0 : dl < 0): -lambda_i / dl, kind 5.  An equality row in W offers nothing.
 *     variable j in F:  if vx < 0 and x_L_j > -inf: (x_L_j - x_j) / vx, kind 3; else if vx > 0 and x_U_j < inf: (x_U_j - x_j) / vx, kind 4
 *     variable j in B:  if (bound_state_j > 0 ? dv > 0 : dv < 0): -z_j / dv, kind 6
 *   Every ratio is clamped from below at 0 (r < 0 ? 0 : r): a violated inactive row or a multiplier of the wrong sign makes the range 0 on
 *   that side.  A ratio that is not below +inf is no candidate.  The side's result is the smallest ratio, on equal ratios the smallest
 *   position; best = +inf, position -1 and kind 0 mean no candidate.  t_hi = best >= 0, t_lo = 0 - best <= 0.
 *   V_i is summed from 0.0 over the row's entries in the order of its pattern - the CSR list of the skeleton where the pattern has one,
 *   j = 0 .. n - 1 over the dense row otherwise - product then sum, no fused multiply-add, by one thread.  No atomics on doubles: partial
 *   minima per workgroup, combined by the last workgroup to arrive in workgroup order (asm_range_kernels.hip.h).  A column's result
 *   depends on that column alone, bit for bit: not on nrhs, its place, its neighbours or the KKT form set on the handle.
 * The entry evaluates E and the Jacobian values at x with the evaluator's own launches into buffers of its own, as the KKT entries do, for
 * every nlp_kind (first derivatives only).  Columns go in chunks of ASM_KKT_CHUNK: one upload and one read-back per chunk.  It does not
 * touch the next LP's inputs, the retained basis or the active sets.  Memory, made at the first call: the Jacobian values (nnz), the CSR
 * values (or Mp x ldn dense rows for a pattern without a CSR list), ASM_KKT_CHUNK x (2 ldn + Mp) doubles for a chunk,
 * (ceil(m / 64) + ceil(n / 64)) x ASM_KKT_CHUNK x 2 partial candidates of 16 bytes, and the pinned image of a chunk.
 * Errors: ASM_ERR_STATE before asm_sublp_setup and asm_eval_setup; a null pointer (lambda, row_state, DLAM may be NULL for m = 0),
 * nrhs < 1, a state outside its value set: ASM_ERR_ARG.  The handle works on afterwards.
 * asm_batch_sensitivity_range: the same with a leading scenario dimension on every array - bounds n_scen x m and n_scen x n as in
 * asm_batch_slp_run, x, z, bound_state n_scen x n, lambda, row_state n_scen x m, DX, DZ n_scen x nrhs x n, DLAM n_scen x nrhs x m, out
 * n_scen x nrhs.  Each scenario runs with its bounds and its row of the scenario data table; n_scen may exceed the slot count; the work
 * areas are made before any fiber starts, where the argument refusals happen too; scenario s is bit-identical to the per-handle entry on
 * a fresh handle with that scenario's bounds and data. */
typedef struct {
    double t_lo, t_hi;       /* the range of t: t_lo <= 0 <= t_hi, -inf / +inf without a candidate */
    int32_t pos_lo, kind_lo; /* what blocks at t_lo: position (row i, or m + variable j; -1 none) and kind (ASM_RANGE_*) */
    int32_t pos_hi, kind_hi; /* the same at t_hi */
} asm_range_info;
#define ASM_RANGE_NONE 0
#define ASM_RANGE_ROW_LOWER 1  /* an inactive row reaches g_L */
#define ASM_RANGE_ROW_UPPER 2  /* an inactive row reaches g_U */
#define ASM_RANGE_VAR_LOWER 3  /* a free variable reaches x_L */
#define ASM_RANGE_VAR_UPPER 4  /* a free variable reaches x_U */
#define ASM_RANGE_ROW_MULT 5   /* the multiplier of a working row reaches 0 */
#define ASM_RANGE_VAR_MULT 6   /* a bound multiplier reaches 0 */
int asm_sensitivity_range_multi(asm_handle* h, const double* x, const double* lambda, const double* z, const int32_t* row_state,
                                const int32_t* bound_state, int32_t nrhs, const double* DX, const double* DLAM, const double* DZ,
                                asm_range_info* out);

/* ---- Adjoint solution sensitivities: the gradient of one function of the solution with respect to all data, from one KKT solve.
 * The forward entries answer "how do x* and lambda* move along one direction dc of the data" at one KKT right-hand side per direction.  The
 * reverse question - given phi(x*, lambda*) with gradients gx [n] and gl [m], what is d phi / d dpar[c] for every c - needs one solve,
 * because the KKT matrix of the working set is symmetric: with u_k = d/d c_k (grad_x L), w_k = d g / d c_k and M = [H_FF, -A'; -A, 0],
 * the forward sensitivity is (dx, dlam) = M^-1 (-u_k, w_k), so gx'dx + gl'dlam = (M^-1 (gx, gl))' (-u_k, w_k).
 *   1. adjoint state: (ax, al) = asm_kkt_solve(ru = -gx, rw = gl), no dz; ax is zero on B and al outside W, as that solve guarantees.
 *   2. d phi / d dpar = asm_eval_data_cross_t(vx = -ax, vl = al), the transposed cross derivative below.
 *   3. d phi / d bound_i = -al_i for a working row i, 0.0 for every other row: the recipe "ru = 0, rw_i = -delta" read backwards.
 * Weights on the bound multipliers z and derivatives with respect to variable bounds: asm_solution_adjoint_z below.
 * Transposed cross derivatives.  asm_eval_data_cross_t: for weights vx [n], vl [m] at (x, lambda),
 *   out[c] = vx' d/d dpar[c] (grad_x L) + vl' d g / d dpar[c] = d/d dpar[c] [ D_vx L(x, lambda; dpar) + vl' g(x; dpar) ],   c < n_dpar,
 * L = f - lambda' g and D_vx the directional derivative along vx in x.  Rows of the function store contribute nothing.  For every dc,
 * dc' out = vx' u + vl' w with (u, w) of asm_eval_data_cross(dc).  Kinds, errors and refusals are asm_eval_data_cross's (kinds 3, 4, 5;
 * ASM_ERR_STATE before asm_eval_setup; kinds 0, 1, 2 and null pointers ASM_ERR_ARG); the inputs of the next LP are not touched.  The
 * workspace ([lam | vx | vl] and n_dpar outputs per column, one column, ASM_KKT_CHUNK from the first multi call on) is made by the first
 * call.  No fused multiply-add, no atomics; every written operation is one rounding, left to right, every sum in an order fixed by the model:
 *   expression block (kind 3): the forward-over-reverse sweep of the Hessian and of asm_eval_data_cross with the other seed - a VAR node
 *     of variable j has the tangent vx[j], a CONST node 0 - and the formulas of "Hessian of the Lagrangian", 2.  A CONST exponent of POW
 *     receives adj and tadj (the statements on b) and yields its occurrence like every CONST node; its tangent is 0, so the "then" steps stay
 *     out - no 0 * log(u) forms, and every entry that does not belong to the exponent stays finite for u < 0.  The exponent's own entry is NaN
 *     or inf where log(u) is (u <= 0), as in asm_eval_data_gradient.  One thread per row or term.  In the reverse pass a CONST
 *     node with adjoint adj and adjoint tangent tadj yields one occurrence: for a node of block row r
 *       (-lambda[n_rows + r]) * tadj + vl[n_rows + r] * adj        (two products, one sum)
 *     and for a node of a term objective_scale * tadj.  out[c] sums the occurrences of dpar[c] in the list order of
 *     asm_eval_data_gradient, from 0.0.  A tape without a CONST node: nothing is launched, out is all zero (empty for n_dpar = 0).  With
 *     ADD..POWI, ABS, MIN and MAX only, device and host twin (nlexpr.py: ExprBlock.data_cross_t) agree bit for bit.
 *   Ohm's-law block (kind 4): per branch l, with vf, vt, d, cs, sn, vv and the basis values vf2, vt2, vvc, vvs of the data gradient, l0..l3
 *     and v0..v3 the entries of lambda and vl on its rows pfr, qfr, pto, qto, dvf = vx[vm_f], dvt = vx[vm_t], dd = vx[va_f] - vx[va_t]:
 *       tvv = dvf*vt + vf*dvt    tvf2 = 2*(vf*dvf)    tvt2 = 2*(vt*dvt)    tvvc = tvv*cs - vvs*dd    tvvs = tvv*sn + vvc*dd
 *     and out[q n_branch + l], q = 0..7, is the data gradient's pattern with (lambda, derivative) minus that with (vl, value):
 *       l0*tvf2 - v0*vf2    l1*tvf2 - v1*vf2    l2*tvt2 - v2*vt2    l3*tvt2 - v3*vt2
 *       (l0*tvvc + l1*tvvs) - (v0*vvc + v1*vvs)        (l0*tvvs - l1*tvvc) - (v0*vvs - v1*vvc)
 *       (l2*tvvc - l3*tvvs) - (v2*vvc - v3*vvs)        (-(l2*tvvs) - l3*tvvc) - (-(v2*vvs) - v3*vvc)
 *     One thread per (branch, column).  Device and host twin (acopf.py: _ohm_data_twins) differ at most in the last bits of sin and cos.
 *   dense quadratic block (kind 5): one thread per entry (i, j) and column, li = lambda[n_rows + i], vi = vl[n_rows + i]:
 *       out[i n + j] = (-li)*vx_j + vi*x_j        out[m_blk n + i n + j] = (-li)*(x_j*vx_j) + vi*(0.5*(x_j*x_j))
 *     bit-identical to the host twin (problems.py).
 * asm_solution_adjoint: steps 1 to 3 - the solve through asm_kkt_solve's single-column back end, then asm_eval_data_cross_t on (-ax, al):
 * out equals that call on its own bit for bit.  out [n_dpar]; dbound [m], ax [n] and al [m] may be NULL.  info is the solve's; a status
 * other than 0 is a result, not an error, and the outputs then come from the iterate reached.  par as for asm_kkt_solve.  A derivative
 * entry like asm_solution_sensitivity: the exact Hessian whatever asm_hessian_set_type chose, and that entry's refusals - but for the
 * function store alone (nlp_kind 0), which the adjoint entries serve: there is no data and out is empty (n_dpar = 0, out may be NULL),
 * while dbound, ax and al need no data derivative.
 * asm_solution_adjoint_multi: nrhs functions at once, one per row of GX [nrhs x n] and GL [nrhs x m]; OUT nrhs x n_dpar, DBOUND and AL
 * nrhs x m, AX nrhs x n (DBOUND, AX, AL may be NULL), info [nrhs].  The solve is asm_kkt_solve_multi's - one factor, chunks of
 * ASM_KKT_CHUNK columns in lockstep - and the transposed sweep runs per chunk: one upload of the chunk's weights, one launch for all its
 * columns (kinds 4 and 5, the column in grid.y) or one launch pair per column (kind 3), one read-back.  Column independence holds as for
 * the other multi entries, bit for bit; against asm_solution_adjoint the agreement is to tolerance (the two back ends).  nrhs < 1:
 * ASM_ERR_ARG; validity and refusals are asm_solution_sensitivity_multi's.  The staging of a chunk is ASM_KKT_CHUNK x (n + n_dpar)
 * doubles.  Both KKT forms serve the entries: they add nothing form-specific. */
int asm_eval_data_cross_t(asm_handle* h, const double* x, const double* lambda, const double* vx, const double* vl, double* out);
int asm_solution_adjoint(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state,
                         const double* gx, const double* gl, const asm_kkt_params* par, double* out /* [n_dpar] */,
                         double* dbound /* [m], may be NULL */, double* ax /* [n], may be NULL */, double* al /* [m], may be NULL */,
                         asm_kkt_info* info);
int asm_solution_adjoint_multi(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state,
                               int32_t nrhs, const double* GX, const double* GL, const asm_kkt_params* par, double* OUT /* nrhs x n_dpar */,
                               double* DBOUND, double* AX, double* AL, asm_kkt_info* info);
/* The adjoint entries with weights on the bound multipliers and gradients with respect to variable bounds: phi(x*, lambda*, z*) has the
 * gradients gx [n], gl [m] and gz [n].  z exists on B only: entries of gz on F are ignored, they are treated as 0.0.  With
 * gx~ = gx + H gz and gl~ = gl - J gz the adjoint state is (ax, al, dz) = asm_kkt_solve(ru = -gx~, rw = gl~) with dz on, and
 *   d phi / d dpar     = asm_eval_data_cross_t(vx = gz - ax, vl = al)   (the supports of gz and ax are disjoint)
 *   d phi / d bound_i  = -al_i on W, 0.0 elsewhere
 *   d phi / d xbound_j = -dz_j on B, 0.0 on F: dxbound [n], may be NULL - the derivative with respect to the bound that variable j sits at.
 * gx~ and gl~ are made on the device: the chunk's gz goes up, k_kktm_gz_mask clears it on F, one Hessian product on the block gives H gz
 * and one product with J[W, B] - the columns that the solve's own products mask out - gives J gz on the working rows (dense form: the
 * working rows gathered with the complementary mask feeding k_gemm_nt, or k_gemv_n for one column; sparse form: k_kkts_mul_a with the
 * complementary mask).  gz == NULL: out, dbound, ax, al and info equal asm_solution_adjoint(_multi) bit for bit - the preparation is
 * skipped, not run with zeros - and dxbound is still returned.  Kinds, refusals, par, info, column independence and the function store
 * alone (nlp_kind 0: out empty) are as for asm_solution_adjoint(_multi); GZ nrhs x n, DXBOUND nrhs x n (both may be NULL). */
int asm_solution_adjoint_z(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state,
                           const double* gx, const double* gl, const double* gz /* [n], may be NULL = 0 */, const asm_kkt_params* par,
                           double* out /* [n_dpar] */, double* dbound /* [m], may be NULL */, double* dxbound /* [n], may be NULL */,
                           double* ax /* [n], may be NULL */, double* al /* [m], may be NULL */, asm_kkt_info* info);
int asm_solution_adjoint_z_multi(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state,
                                 int32_t nrhs, const double* GX, const double* GL, const double* GZ, const asm_kkt_params* par,
                                 double* OUT /* nrhs x n_dpar */, double* DBOUND, double* DXBOUND, double* AX, double* AL, asm_kkt_info* info);

/* ---- Trust-region step on the working set: Byrd-Omojokun with Steihaug-Toint truncation.
 * asm_kkt_step is asm_kkt_solve with an l2 radius: it minimises the model ru'dx + 1/2 dx'H dx over A dx_F = -theta rw_W, dx_B = 0,
 * ||dx||_2 <= radius - a normal step that may use only normal_share of the radius, then projected conjugate gradients that walk to the
 * boundary of the region where they leave it or meet non-positive curvature.  asm_kkt_step_multi does so for nrhs right-hand sides with
 * a radius each (RADIUS [nrhs]) on one factor, in the lockstep iteration of asm_kkt_solve_multi: with the rows of RU / RW equal it answers
 * a whole ladder of radii, which is what a trust-region driver needs after a rejected step.
 * Validity, argument errors and layouts are asm_kkt_solve's and asm_kkt_solve_multi's.  A radius that is not
 * > 0 (NaN included) and a normal_share outside (0, 1]: ASM_ERR_ARG.  par == NULL: asm_kkt_solve's defaults and normal_share = 0.8.
 * radius = +INFINITY is allowed and is asm_kkt_solve, bit for bit in dx, dlam, dz and the fields asm_kkt_info has.
 * Method per column (the steps of asm_kkt_solve; both entries run its driver and its kernels):
 *   1., 2. unchanged, once per call.
 *   3. dx0 as in asm_kkt_solve, with its refinement step.  nn = ||dx0||_2.  If nn > normal_share radius: theta = normal_share radius / nn
 *      and dx0 <- theta dx0; otherwise theta = 1.  Dt^2 = radius^2 - (theta nn)^2 (not below 0): dx0 in range(A') and d in null(A) are
 *      orthogonal, so ||dx||^2 = ||dx0||^2 + ||d||^2.
 *   4. the iteration of asm_kkt_solve; the pass that forms p'Hp also forms d'd, d'p and p'p, directly, not by recurrence.  With
 *      gap = Dt^2 - d'd and tau = gap / (d'p + sqrt((d'p)^2 + p'p gap)) (tau = 0 when gap <= 0), the positive root of ||d + tau p||^2 = Dt^2:
 *        p'Hp <= 0, radius finite:    d += tau p, boundary = 2, the column stops
 *        p'Hp <= 0, radius infinite:  as asm_kkt_solve (status 2, the iterate stays)
 *        p'Hp > 0 and d'd + 2 alpha d'p + alpha^2 p'p >= Dt^2 (alpha = r'g / p'Hp):   d += tau p, boundary = 1, the column stops
 *        otherwise the iteration is unchanged.
 *      A column that stops on the boundary takes tau in place of alpha in that round's step kernel and is frozen from then on, as a
 *      converged column is.  cg_iters counts completed iterations, and the boundary move is one: a column that reaches the boundary in
 *      its first iteration has cg_iters = 1.
 *   5., 6. as asm_kkt_solve with rw replaced by theta rw in res_feas; model = ru'dx + 1/2 dx'H dx, norm_normal = theta nn and
 *      norm_step = ||dx||_2 (summed directly from dx).
 * status keeps its four meanings; a column that stopped on the boundary has status 0.
 * Nothing of this visits the host: the radii go to the device with the right-hand sides, theta, Dt^2 and the boundary code live in the
 * column's scalar block, and the host still reads the one active-column word per round.  A round has the launches it had; one launch
 * per chunk (k_kktm_normal) scales the normal steps, and the model value and the step norm are sums of the finish launch.  The three
 * further sums use the rule of the others - per-workgroup partial sums, added in workgroup order by the last workgroup to arrive - so a
 * column's bits depend on its own right-hand side and radius alone. */
typedef struct { int32_t max_iter; double rtol; double normal_share; } asm_kkt_step_params;
typedef struct {
    int32_t status, cg_iters, n_free, n_rows, dropped_pivots;   /* as asm_kkt_info */
    int32_t boundary;          /* 0 inside the region, 1 boundary reached on positive curvature, 2 boundary reached along p'Hp <= 0 */
    double res_stat, res_feas; /* res_feas against theta * rw */
    double theta;              /* share of the normal step taken: A dx_F = -theta rw_W */
    double norm_normal, norm_step;   /* ||theta dx0||_2, ||dx||_2 */
    double model;              /* ru'dx + 1/2 dx'H dx */
} asm_kkt_step_info;
int asm_kkt_step(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state,
                 const double* ru, const double* rw, double radius, const asm_kkt_step_params* par, double* dx, double* dlam, double* dz,
                 asm_kkt_step_info* info);
int asm_kkt_step_multi(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state,
                       int32_t nrhs, const double* RU, const double* RW, const double* RADIUS, const asm_kkt_step_params* par, double* DX,
                       double* DLAM, double* DZ, asm_kkt_step_info* info);

/* ---- The form of the KKT solve: dense (the default, the method text above) or sparse.  Per handle: the scenario batches
 * (asm_batch_*) take their form from asm_batch_kkt_set_form, whatever is set here.
 * asm_kkt_set_form chooses the form of every later KKT entry on the handle - asm_kkt_solve(_multi), asm_solution_sensitivity(_multi),
 * asm_kkt_step(_multi), asm_eqp_trial and asm_slp_run_eqp - until the next asm_eval_setup, which starts from ASM_KKT_DENSE again.  Valid
 * after asm_eval_setup (ASM_ERR_STATE before); a form other than the two below: ASM_ERR_ARG.
 * ASM_KKT_SPARSE replaces steps 1 and 2 and the products of the method; the driver of steps 3 to 6, its kernels, statuses and outputs stay:
 *   1. the Jacobian values go from the value buffer into the CSR list of the LP's sparse pattern (one kernel; no dense J)
 *   2. the working rows are taken in the reverse Cuthill-McKee order of their coupling graph (two rows are coupled when they share a
 *      column); S = A A' is built entry by entry from its structural pairs, as the null-space form builds S0, and is banded in that
 *      order: the factorisation and the substitutions stop at the band.  A band of half the order or more is factored as a dense matrix.
 *      The order, band and pairs of the last row_state are kept and reused when the next call's row_state is equal (the structure of S over
 *      W does not depend on F).
 *   The products with A and A' are sparse (k_kkts_mul_a over the CSR lists of the working rows, k_kkts_mul_at over the CSC lists of the
 *   variables, for 1 to ASM_KKT_CHUNK columns); the substitutions are the factor's own (one column) or Dev::trsm_rows with a transposed
 *   copy of the band (blocks).  The column independence of the multi entries holds as stated above.  Against the dense form the agreement
 *   is to tolerance (other summation orders, another row order in the factor); dlam is returned by row as ever.
 * Fallback, not an error: when the handle has no sparse pattern (a dense model, fill above 1/16) or the pattern's coupling graph is too
 * dense to order (RCM_MAX_PAIRS), a call with ASM_KKT_SPARSE set runs the dense form and says so in form_used.
 * Memory: a handle that only ever runs the sparse form never allocates the dense J, A, its transposed copy and the unmasked transposed
 * rows (dense_bytes == 0); the factor (pitch^2 doubles, not band storage) and the blocks are shared by the forms.
 * asm_kkt_form_info describes the last KKT call on the handle (all zero but form_requested before the first). */
enum { ASM_KKT_DENSE = 0, ASM_KKT_SPARSE = 1 };
struct asm_kkt_form_info {     /* a tag, not a typedef: the entry below has the same name */
    int32_t form_requested, form_used;   /* ASM_KKT_* */
    int32_t band;              /* bandwidth of S in the order used (at least 1 when |W| > 0); 0: dense form */
    int32_t order_reused;      /* 1: the row order came from the cache */
    int64_t n_pairs;           /* structural entries of the lower triangle of S, diagonal included */
    int64_t dense_bytes, sparse_bytes;   /* device bytes of the buffers that only the dense / only the sparse form has made on this handle */
    double order_ms;           /* host milliseconds the call spent on the row order (0 when reused) */
};
int asm_kkt_set_form(asm_handle* h, int32_t form);
int asm_kkt_form_info(const asm_handle* h, struct asm_kkt_form_info* out);

/* ---- The row order of the sparse form.  asm_kkt_set_order has the state rules of asm_kkt_set_form (ASM_ERR_STATE before asm_eval_setup,
 * ASM_ERR_ARG for other values, back to the default at the next asm_eval_setup) and no effect in the dense form.
 *   ASM_KKT_ORDER_WORKING_SET (the default)  step 2 above: a reverse Cuthill-McKee order of every new working set, made on the host, its
 *       position list and pairs uploaded, the stream waited for.
 *   ASM_KKT_ORDER_STATIC  the reverse Cuthill-McKee order of ALL m rows, made once at the first sparse call, restricted to the working
 *       set.  The coupling graph of W is an induced subgraph and places only move closer, so S is banded with at most the all-rows band;
 *       the band used is the exact largest distance over the structural pairs of all rows with both rows in W (host, cached on an equal
 *       row_state like the order above: order_reused keeps its meaning), n_pairs their number.  Per call nothing is ordered, nothing
 *       goes up besides the one copy of the sets, and the stream is not waited for: k_kkts_wpos makes the position list on the device
 *       from the uploaded working rows, and S is built from the row-index pairs of all rows (on the device since the first call in this
 *       order) through that list, pairs with a row outside W skipped.  The band is not rounded.  Everything after the build of S is
 *       shared with the other order; the answers agree to tolerance (another row order in the factor).
 * asm_kkt_order_info: the order requested and the one the last KKT call used (ASM_KKT_ORDER_WORKING_SET for a dense call, the fallback
 * included), the band and the structural pairs of all m rows (0 before the first sparse call).  asm_kkt_row_order: the working rows of the
 * last KKT call in the order used (ascending in the dense form); rows may be NULL to read *nW alone.  band, n_pairs, order_reused and
 * order_ms of asm_kkt_form_info describe the call in either order. */
enum { ASM_KKT_ORDER_WORKING_SET = 0, ASM_KKT_ORDER_STATIC = 1 };
struct asm_kkt_order_info {
    int32_t order_requested, order_used;   /* ASM_KKT_ORDER_* */
    int64_t all_band, all_pairs;
};
int asm_kkt_set_order(asm_handle* h, int32_t order);
int asm_kkt_order_info(const asm_handle* h, struct asm_kkt_order_info* out);
int asm_kkt_row_order(const asm_handle* h, int32_t* rows, int64_t* nW);

/* ---- per-iteration reductions of the SLP callers on the evaluation results in HBM (need asm_eval_functions) ----------
 * out4 = { norm_violations(Inf), norm_violations(1), KT_residuals, norm_complementarity(Inf) }   (common.jl:35-98). */
int asm_slp_norms(asm_handle* h, const double* lambda, const double* mult_x_U, const double* mult_x_L, double* out4);
/* mode 0: compute_phi(x, alpha, p) (slp.jl:79-115; the trial point is evaluated on the device);
 * mode 1: compute_derivative (slp.jl:122-147).  p_slack as asm_sublp_solve returns it. */
int asm_slp_merit(asm_handle* h, int mode, double alpha, const double* p, const double* nu, const double* p_slack,
                  int feasibility, double prim_infeas, double* out);

/* compute_alpha (slp_line_search.jl:222-244): backtracking alpha = 1, tau, tau^2, ... on the merit function, the trial points evaluated on
 * the device eight at a time - one set of launches with the trial index in the grid (same alpha and merit values as one asm_slp_merit call per
 * trial).  *ok = 1: Armijo test passed at *alpha;
 * *ok = 0: alpha fell below min_alpha with the test still failing (*alpha is that last trial, as the reference leaves it). */
int asm_slp_line_search(asm_handle* h, const double* p, const double* nu, const double* p_slack, int feasibility, double prim_infeas, double phi0,
                        double D, double eta, double tau, double min_alpha, double* alpha, double* phi_alpha, int* trials, int* ok);
/* step_quality's merit values (slp_trust_region.jl:213-216): out3 = { compute_derivative, compute_phi(x, 0, p), compute_phi(x, 1, p) }
 * with x+p evaluated on the device; equal bit for bit to three asm_slp_merit calls.  Needs asm_eval_functions. */
int asm_slp_step_quality(asm_handle* h, const double* p, const double* nu, const double* p_slack, int feasibility, double prim_infeas, double* out3);

/* Seed the retained basis columns of the null-space form (0-based; what asm_sublp_ns_basis returns): the next normal-phase LP builds its
 * basis from them instead of selecting columns from scratch.  asm_sublp_set_bounds keeps the columns (same pattern), drops the basis. */
int asm_sublp_set_ns_basis(asm_handle* h, const int32_t* J, int64_t k);

/* ---- native SLP caller: run!(::SlpLS) (slp_line_search.jl:78-215) with every evaluation and reduction on the device ------------------
 * The same sequence of library calls as the host drivers make per outer iteration (asm_eval_functions, asm_slp_norms,
 * asm_sublp_solve_resident, asm_slp_merit x 2, asm_slp_line_search), so that one scenario solve is ONE call.  Parameters: src/parameters.jl:17-28. */
typedef struct {
    int32_t max_iter;          /* parameters.jl: max_iter */
    int32_t max_lp_solves;     /* 0 = no cap (bench: fixed number of steps) */
    double  tol_direction, tol_residual, tol_infeas, eta, tau, min_alpha;
} asm_slp_params;
typedef struct {
    int32_t status;            /* slp.ret: 0 optimal, 2 infeasible, 6 almost feasible, -1 iteration limit, -3 line-search failure, -5 not finished */
    int32_t iter, lp_solves, restoration_solves, ls_trials, slot;
    int32_t paths[12];         /* histogram of asm_solve_stats.path over the LPs of the run */
    int32_t ipm_iters, ns_cold;
    double  obj_val, prim_infeas, dual_infeas, compl_;
} asm_slp_result;
/* x0[n] -> x[n], lambda[m], mult_x_U[n], mult_x_L[n], g[m] (constraint values at the last evaluated iterate); any output may be NULL.
 * Needs asm_sublp_setup + asm_eval_setup on the handle. */
int asm_slp_run(asm_handle* h, const asm_slp_params* par, const double* x0, double* x, double* lambda, double* mult_x_U, double* mult_x_L,
                double* g, asm_slp_result* res);

/* ---- native SLP caller: run!(::SlpTR) (slp_trust_region.jl:87-251), the same library calls as the host driver (SlpTR.run with
 * device_eval): asm_eval_functions, asm_sublp_solve_resident at the radius, asm_jac_row_norms (first iteration), asm_slp_norms,
 * asm_slp_step_quality.  res is filled as asm_slp_run fills it (ls_trials = 0).  tr_size: the initial radius (parameters.jl: tr_size),
 * finite and > 0 (else ASM_ERR_ARG). */
typedef struct {
    double  delta;             /* final trust-region radius */
    int32_t accepted;          /* steps with rho >= 0 (x moved) */
    int32_t rejected;          /* steps with rho < 0 (x kept) */
    int32_t shrunk, expanded;  /* radius decreases / increases */
} asm_slp_tr_info;
int asm_slp_run_tr(asm_handle* h, const asm_slp_params* par, double tr_size, const double* x0, double* x, double* lambda,
                   double* mult_x_U, double* mult_x_L, double* g, asm_slp_result* res, asm_slp_tr_info* tr /* may be NULL */);

/* ---- SLP-EQP: the Trust-Region SLP with a second-order step on the working set the LP names (not in the reference).
 * At a solution that is not a vertex of the linearisation an LP step runs to the boundary of its region, is rejected, and the radius
 * shrinks until it falls below tol_direction: first-order convergence at best.  SLP-EQP inserts, between the evaluation at the top of an
 * iteration and the LP, the trust-region step of the equality-constrained QP (asm_kkt_step) on the working set of the last LP, with a
 * radius D_E of its own, and takes the step when it lowers the merit function.  The stop tests remain the Trust-Region driver's.
 *   A. Attempted only outside feasibility restoration, when the last LP solved was a normal-phase LP with status OPTIMAL.  S = its active
 *      set (asm_sublp_active_set), lambda = its multipliers.
 *   B. Working set.  adj = the rows with two distinct finite bounds, in index order; rows m.. of S's row_state are their `<=` twins.
 *      Row i is in W if it is an equality, if row_state[i] != 0 or if its twin is active; it sits at g_L (an equality), at g_U (twin
 *      active, or g_L infinite), else at g_L.  Variable j is in B only where S reports it at a bound and |x_j - bound| <= tol_active
 *      (1 + |bound|) for the problem's finite bound on that side: a variable the LP's trust region stopped is free.
 *   C. |W| > |F|: skipped (1).
 *   D. asm_kkt_step(x, lambda, W, B, ru = grad f(x), rw_W = E_W - bound_W, radius = D_E); status 3 (dependent rows): skipped (2).
 *   E. t = the largest value in [0, 1] with x_L <= x + t dx <= x_U, d = t dx; d identically zero: skipped (3).
 *   F. phi0, phi1 = the merit function f + nu' viol (asm_slp_merit mode 0) at alpha = 0 and 1 with p = d; accepted iff phi1 < phi0.
 *   G. accepted: x += d, lambda = dlam, mult_x_L = dz on B = -1, mult_x_U = dz on B = +1, 0 elsewhere; D_E = min(2 D_E, radius_max)
 *      if the step ended on its boundary (boundary != 0) with t = 1; the functions are evaluated again.  Rejected: D_E = ||d||_2 / 2.
 *      iter, lp_solves and the LP's radius are not touched.
 * asm_eqp_trial is steps B to F in one call, after asm_eval_functions at x (the point the evaluator holds: E, x and the gradient are
 * read where it left them in HBM).  lp_row_state [m + n_adj], lp_bound_state [n]: S.  nu [m]: the merit weights.  par == NULL: the
 * defaults of asm_kkt_step.  Outputs: d [n], lam_new [m], mult_x_U, mult_x_L [n] (all zero for a skipped trial), the working set used
 * (row_state [m] of 0 / 1, bound_state [n] of -1 / 0 / +1) and info.
 *   k_eqp_face makes the working set, the side each working row sits at, rw and the counts |W|, |F| in one launch; the step is
 *   asm_kkt_step's driver and kernels, unchanged; k_eqp_trial makes t, d, ||d||_2 and ||d||_inf in one launch - per-workgroup partial
 *   sums added in workgroup order, no atomics on doubles; the two merit values are the launch set of asm_slp_step_quality.  d is, bit
 *   for bit, t times the dx asm_kkt_step returns for the same working set, phi0 / phi1 are asm_slp_merit's values.
 * The inputs of the next LP, the retained basis and the active sets are not touched (asm_kkt_step's guarantee).
 * Validity and argument errors are asm_kkt_step's; tol_active not >= 0 or a state outside its value set ({0, 1} for rows, {-1, 0, +1} for
 * bounds): ASM_ERR_ARG; ASM_ERR_STATE unless the handle's last inputs came from asm_eval_functions (not asm_sublp_upload) at this very x.
 * The handle works on after any of them.  A per-handle call; asm_batch_slp_run_eqp runs it inside the library's scenario batch. */
typedef struct {
    int32_t status, cg_iters, n_free, n_rows, dropped_pivots, boundary;     /* as asm_kkt_step_info (n_free, n_rows: the face's counts) */
    double res_stat, res_feas, theta, norm_normal, norm_step, model;
    int32_t skipped;           /* 0 none, 1 more working rows than free variables, 2 dependent working rows, 3 zero step */
    double t;                  /* fraction of dx that stays inside the variable bounds */
    double norm_d, norm_d_inf; /* ||d||_2, ||d||_inf */
    double phi0, phi1;         /* merit function at x and at x + d */
} asm_eqp_info;
int asm_eqp_trial(asm_handle* h, const double* x, const double* lambda, const int32_t* lp_row_state, const int32_t* lp_bound_state,
                  double radius, const double* nu, double tol_active, const asm_kkt_step_params* par, double* d, double* lam_new,
                  double* mult_x_U, double* mult_x_L, int32_t* row_state, int32_t* bound_state, asm_eqp_info* info);
/* The native driver: asm_slp_run_tr with the insertion above - the library calls of SlpEQP.run in activesetmethods_amd/slp.py with
 * device_eval (asm_slp_run_tr's, asm_eqp_trial, asm_eval_functions after an accepted step).  enabled = 0 is asm_slp_run_tr, bit for bit.
 * radius0 (finite) and radius_max must be > 0, tol_active >= 0 (else ASM_ERR_ARG).  Needs a model with second derivatives (nlp_kind 0,
 * 3, 4 or 5, as asm_kkt_step).  tr and eqp_info may be NULL.  Its form over a scenario batch is asm_batch_slp_run_eqp. */
typedef struct {
    double radius0;            /* initial D_E */
    double radius_max;         /* cap on D_E */
    double tol_active;         /* the activity tolerance of step B */
    int32_t enabled;           /* 0: no step is attempted */
} asm_slp_eqp_params;
typedef struct {
    double  radius;            /* final D_E */
    int32_t attempts;          /* trials made (= accepted + rejected + the three skipped counts) */
    int32_t accepted, rejected;
    int32_t skipped_rows, skipped_dependent, skipped_zero;
    int32_t cg_iters;          /* conjugate-gradient iterations of all trials */
    int32_t boundary;          /* trials whose step ended on the boundary of its region */
} asm_slp_eqp_info;
int asm_slp_run_eqp(asm_handle* h, const asm_slp_params* par, double tr_size, const asm_slp_eqp_params* eqp_par, const double* x0,
                    double* x, double* lambda, double* mult_x_U, double* mult_x_L, double* g, asm_slp_result* res,
                    asm_slp_tr_info* tr /* may be NULL */, asm_slp_eqp_info* eqp_info /* may be NULL */);

/* ---- Limited-memory Hessian: SLP-EQP for models without second derivatives ---------------------------------------------------------------
 * A limited-memory BFGS approximation B of the Hessian of L = f - lambda' g, held on the device per handle, in the compact form of Byrd,
 * Nocedal and Schnabel over the stored pairs (s_i, y_i) in chronological order:
 *     B v = sigma v - Psi' W Psi v,   Psi = [sigma S; Y],   W = [[sigma S S', L], [L', -D]]^-1,
 * sigma = y'y / s'y of the newest pair, D = diag(s_i'y_i), L_ij = s_i'y_j for i > j.  No pairs: B = I.  A pair is stored only if
 * ||s|| > 0, s'y > 0 and s'y >= 1e-8 ||s|| ||y|| (decided on the device; the middle condition only adds y = 0), so B is positive definite.  A push to a
 * full store drops the oldest pair.  The count, sigma, the Gram entries and W live in HBM: pushes and products read nothing back.
 *
 * asm_hessian_set_type selects, per handle, what stands for H in asm_kkt_solve(_multi), asm_kkt_step(_multi), asm_eqp_trial and
 * asm_slp_run_eqp: ASM_HESS_EXACT (the default: every bit as without this section) or ASM_HESS_LM with 1 <= memory <= ASM_LM_MAX
 * (ASM_ERR_ARG outside, for either type).  With ASM_HESS_LM those entries take every nlp_kind: the Hessian values
 * are not evaluated and the Jacobian of kinds 1, 2, 4 and 5 comes from their own kernels.  The derivative entries stay exact and keep their
 * refusals whatever the type: asm_eval_hessian_*, asm_eval_data_cross, asm_solution_sensitivity(_multi), asm_batch_*.  A slot of an
 * asm_batch: ASM_ERR_ARG.  Every call clears the store; asm_sublp_setup and asm_eval_setup clear it too (the type and memory stay).
 *
 * asm_lm_push_pair feeds a pair from outside (n doubles each), under the skip rule.  asm_lm_begin / asm_lm_end make the pair of a step of
 * an SLP driver: begin, called before x changes, saves x and grad f - J' lambda from where asm_eval_functions left them (J' lambda as
 * asm_slp_norms forms it); end, called after the next asm_eval_functions with the same lambda, forms s = x - x_prev,
 * y = (grad f - J' lambda) - g_prev and pushes it.  end without a pending begin does nothing.  Both: ASM_ERR_STATE before
 * asm_eval_setup and before the first asm_eval_functions.  asm_lm_product: OUT = V B for row-major nrhs x n (a column's bits do not
 * depend on nrhs or its place).  All of them work whatever the selected type; before asm_sublp_setup: ASM_ERR_STATE.
 * asm_slp_run_eqp with ASM_HESS_LM makes the begin / end calls where SlpEQP of activesetmethods_amd/slp.py makes them. */
#define ASM_LM_MAX 32
enum { ASM_HESS_EXACT = 0, ASM_HESS_LM = 1 };
struct asm_lm_info {           /* a tag, not a typedef: the entry below has the same name */
    int32_t type;              /* ASM_HESS_EXACT or ASM_HESS_LM */
    int32_t memory;            /* pairs the store holds at most */
    int32_t pairs;             /* pairs it holds */
    int32_t pending;           /* 1 between asm_lm_begin and asm_lm_end */
    int64_t pushed;            /* pairs offered since the store was cleared (= stored + the two skipped counts + dropped as oldest) */
    int64_t skipped_zero;      /* ... refused for ||s|| = 0 */
    int64_t skipped_curvature; /* ... refused for s'y < 1e-8 ||s|| ||y|| */
    double  sigma;             /* 1.0 without pairs */
    int64_t bytes;             /* device bytes of the store */
};
int asm_hessian_set_type(asm_handle* h, int32_t type, int32_t memory);
int asm_lm_reset(asm_handle* h);
int asm_lm_push_pair(asm_handle* h, const double* s, const double* y);
int asm_lm_begin(asm_handle* h, const double* lambda);
int asm_lm_end(asm_handle* h, const double* lambda);
int asm_lm_product(asm_handle* h, const double* V, int32_t nrhs, double* OUT);
int asm_lm_info(asm_handle* h, struct asm_lm_info* out);

/* ---- scenario batches: B sub-problems with the same pattern advance through ONE launch sequence on ONE stream --------------------------
 * The reference has no batching (one Optimizer <-> one Model <-> one SLP object, src/MOI_wrapper.jl:1093-1152); these entries are
 * SURVEY.md section 8(b)'s "batch variants with a leading scenario dimension".  An asm_batch owns n_slots handles on one device; a batch
 * call runs one fiber per slot on the calling thread, records every slot's kernel launches and merges equal launches of different slots
 * into one (scenario index in the grid, argument table in HBM).  Results are bit-identical to the per-handle calls.
 * Arrays carry a leading scenario dimension (row-major, scenario s at offset s * length).
 * A failed round (ASM_ERR_HIP from a batch call: a device failure while the merged launches of the slots ran) stops every slot half way
 * through its solve.  From then on every entry except asm_batch_setup, asm_batch_set_groups, asm_batch_destroy and the getters answers ASM_ERR_STATE
 * ("asm_batch_setup first"); asm_batch_setup makes the batch whole again.  An error of one slot's own (bad input) is not of this kind. */
typedef struct asm_batch asm_batch;
int asm_batch_create(int device, int n_slots, asm_batch** out);
int asm_batch_destroy(asm_batch* b);
const char* asm_batch_last_error(const asm_batch* b);
int asm_batch_slots(const asm_batch* b);
/* The slots are split into groups: one stream and one host thread each (group 0 on the calling thread), so that one group's host work
 * (merging, launching) overlaps the other groups' device work.  Default: 2 groups from 16 slots on, 3 from 48 on (ASM_BATCH_GROUPS overrides). */
int asm_batch_set_groups(asm_batch* b, int n_groups);
int asm_batch_groups(const asm_batch* b);
/* the handle of a slot: the per-handle entries (statistics, asm_sublp_active_set, ...) work on it between batch calls */
asm_handle* asm_batch_handle(asm_batch* b, int slot);
/* asm_sublp_setup / asm_eval_setup for every slot (same pattern, same functions) */
int asm_batch_setup(asm_batch* b, int64_t n, int64_t m, int64_t nnz, const int64_t* j_row, const int64_t* j_col,
                    const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub);
int asm_batch_eval_setup(asm_batch* b, int64_t n_rows, const int64_t* aff_ptr, const int64_t* aff_var, const double* aff_coef,
                         const int64_t* quad_ptr, const int64_t* q_v1, const int64_t* q_v2, const double* q_coef,
                         const double* constant, const int64_t* jac_off,
                         const int64_t* g_ptr, const int64_t* g_kind, const double* g_coef, const int64_t* g_other,
                         double objective_scale, int nlp_kind, int64_t nlp_rows, int64_t nlp_nnz,
                         const int64_t* nlp_ipar, int64_t n_ipar, const double* nlp_dpar, int64_t n_dpar);
/* Per-scenario NLP-block data: table [n_scen x count] for dpar[offset, offset + count) (count = 0 clears it; the other arguments are then
 * ignored).  In asm_batch_slp_run(_tr), asm_batch_sublp_solve and asm_batch_data_gradient a slot that takes scenario s writes row s into its
 * evaluator's data (asm_eval_set_data) next to its bounds; without a table each scenario start restores the data of asm_batch_eval_setup,
 * so results never depend on what a slot solved before.  The reference basis-column LP on slot 0 uses scenario 0's data.  The table stays
 * set until it is cleared or asm_batch_eval_setup is called again; a batch call over another number of scenarios is ASM_ERR_ARG. */
int asm_batch_set_scenario_data(asm_batch* b, int64_t n_scen, int64_t offset, int64_t count, const double* table);
/* asm_eval_data_gradient of n_scen scenarios, each with its data: x [n_scen x n], lambda [n_scen x m], out [n_scen x n_dpar]; the kinds
 * of asm_eval_data_gradient (3, 4, 5).  For kinds 4 and 5 a scenario's result does not depend on its data at all, only on its (x, lambda):
 * the blocks are linear in dpar. */
int asm_batch_data_gradient(asm_batch* b, int64_t n_scen, const double* x, const double* lambda, double* out);
/* ---- Hessian of the Lagrangian of n_scen scenarios (asm_eval_hessian_* with a leading scenario dimension): the MOI plus-sign convention
 * of asm_eval_hessian_lagrangian - pass -lambda for the multipliers asm_batch_slp_run returns.  The pattern is the one
 * asm_eval_hessian_structure gives on any slot, in the same order.
 *   x, v, out [n_scen x n]; lambda [n_scen x m]; values [n_scen x nnz]; obj_factor [n_scen], or NULL for 1.0 in every scenario.
 * n_scen may exceed n_slots: the slots take the scenarios in index order, and a slot that takes scenario s first gets scenario s's data
 * (row s of the table of asm_batch_set_scenario_data, else the data of asm_batch_eval_setup), as in asm_batch_data_gradient.  The result
 * for scenario s is bit-identical to the per-handle call on a fresh handle with the same model and asm_eval_set_data of row s: the same
 * kernels run, merged over the slots into one launch each.  The LP inputs, retained bases and hints of the slots are not touched: an
 * asm_batch_slp_run after these calls returns the bits it returns without them.
 * The pattern and the index lists are built by the first of these calls after asm_batch_eval_setup, once for the batch, and shared by
 * the slots; a slot adds its workspace (four node arrays, occurrence values, value and product vectors) when it first takes a scenario.
 * asm_batch_eval_setup drops both.
 * ASM_ERR_STATE before asm_batch_setup + asm_batch_eval_setup.  ASM_ERR_ARG: a null batch or required pointer (lambda with m == 0 and
 * values with nnz == 0 are not required), n_scen < 1, rows without cols or the reverse, an n_scen other than the height of a set
 * scenario table, nlp_kind 1 or 2 (as the per-handle entries).  The batch works on after any of them.
 * asm_batch_hessian_structure: *nnz and, unless rows == cols == NULL, the pattern (1-based). */
int asm_batch_hessian_structure(asm_batch* b, int64_t* nnz, int64_t* rows, int64_t* cols);
int asm_batch_hessian_lagrangian(asm_batch* b, int64_t n_scen, const double* x, const double* obj_factor, const double* lambda, double* values);
int asm_batch_hessian_product(asm_batch* b, int64_t n_scen, const double* x, const double* obj_factor, const double* lambda, const double* v,
                              double* out);
/* basis columns every scenario of asm_batch_slp_run starts from (default: selected by one LP of scenario 0 on slot 0) */
int asm_batch_set_ns_basis(asm_batch* b, const int32_t* J, int64_t k);
int asm_batch_ns_basis(const asm_batch* b, int32_t* J, int64_t* k);
/* asm_sublp_set_bounds (when the four bound arrays are given) + asm_sublp_solve for `count` <= n_slots scenarios in lockstep:
 * c_lb, c_ub [count x m]; v_lb, v_ub, df, x_k, p, mult_x_U, mult_x_L [count x n]; dE [count x nnz]; f, delta, feasibility, status [count];
 * E, lambda [count x m]; p_slack [count x 2m]. */
int asm_batch_sublp_solve(asm_batch* b, int count, const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub,
                          const double* dE, const double* df, const double* f, const double* E, const double* x_k,
                          const double* delta, const int32_t* feasibility,
                          double* p, double* lambda, double* mult_x_U, double* mult_x_L, double* p_slack, int32_t* status);
/* n_scen complete SLP runs (asm_slp_run per scenario; n_scen may exceed n_slots: a slot takes the next scenario in index order when
 * it finishes one).  c_lb, c_ub, g [n_scen x m]; v_lb, v_ub, x0, x, mult_x_U, mult_x_L [n_scen x n]; lambda [n_scen x m]; res [n_scen].
 * Needs asm_batch_setup + asm_batch_eval_setup. */
int asm_batch_slp_run(asm_batch* b, int64_t n_scen, const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub,
                      const double* x0, const asm_slp_params* par,
                      double* x, double* lambda, double* mult_x_U, double* mult_x_L, double* g, asm_slp_result* res);
/* the same with asm_slp_run_tr per scenario (same reference basis-column selection); tr [n_scen] may be NULL */
int asm_batch_slp_run_tr(asm_batch* b, int64_t n_scen, const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub,
                         const double* x0, const asm_slp_params* par, double tr_size,
                         double* x, double* lambda, double* mult_x_U, double* mult_x_L, double* g, asm_slp_result* res,
                         asm_slp_tr_info* tr);
/* the same with asm_slp_run_eqp per scenario: SLP-EQP in lockstep.  Outputs for scenario s equal, bit for bit, those of asm_slp_run_eqp on
 * a fresh handle with that scenario's bounds and data and the batch's reference basis columns, whatever slot took the scenario and
 * whatever that slot solved before (asm_sublp_set_bounds at every scenario start forgets the slot's retained active sets and hints; the
 * step reads the active set of this run's own last LP).  enabled = 0 is asm_batch_slp_run_tr, bit for bit.
 *   The slots run the per-handle code as fibers: the Hessian, KKT and trial kernels are recorded and merged like the LP's.  The word the
 *   host reads per conjugate-gradient round arrives with the round that launches its kernel.  The grids over the working rows are sized
 *   from |W| rounded up to 64 (the kernels return beyond the |W| of their arguments), so that scenarios whose working sets differ by a
 *   few rows share a launch; the rank-K build, the factorisation and the substitutions follow |W| through their tile counts and merge
 *   where those agree.
 *   Memory: the first call after asm_batch_eval_setup makes, for every slot that will run and before any fiber starts, what asm_kkt_step
 *   and asm_eqp_trial make at their first call on a handle - dense J (Mp x ldn), Aw (min(m, n) x ldn), its transposed copy, the factor of
 *   order min(m, n) with its block inverses and the one-column work area - on the batch's shared Hessian lists.  asm_batch_setup and
 *   asm_batch_eval_setup release it; a batch that never makes this call with enabled != 0 holds none of it.
 * Errors are asm_slp_run_eqp's and asm_batch_slp_run_tr's: a null batch or required pointer (x0, par, eqp_par, res, the bounds),
 * n_scen < 1, tr_size / radius0 not finite or not > 0, radius_max not > 0, tol_active not >= 0, nlp_kind 1 or 2 and an n_scen other than
 * the height of a set scenario table: ASM_ERR_ARG; before asm_batch_setup + asm_batch_eval_setup: ASM_ERR_STATE - all before any fiber
 * starts.  The batch works on after any of them.  tr and eqp_info [n_scen] may be NULL. */
int asm_batch_slp_run_eqp(asm_batch* b, int64_t n_scen, const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub,
                          const double* x0, const asm_slp_params* par, double tr_size, const asm_slp_eqp_params* eqp_par,
                          double* x, double* lambda, double* mult_x_U, double* mult_x_L, double* g, asm_slp_result* res,
                          asm_slp_tr_info* tr /* [n_scen], may be NULL */, asm_slp_eqp_info* eqp_info /* [n_scen], may be NULL */);
/* The form and row order of the KKT solves of asm_batch_slp_run_eqp, for every slot.  Valid after asm_batch_eval_setup (ASM_ERR_STATE
 * before), which starts from (ASM_KKT_DENSE, ASM_KKT_ORDER_WORKING_SET) again.  (ASM_KKT_DENSE, either order) and (ASM_KKT_SPARSE,
 * ASM_KKT_ORDER_STATIC) are accepted; (ASM_KKT_SPARSE, ASM_KKT_ORDER_WORKING_SET) is ASM_ERR_ARG - that order is made on the host with
 * uploads and a wait at every new working set, which a round cannot do - and so are values outside the enums.  The batch works on after
 * a refusal, in the form it had.
 *   The next asm_batch_slp_run_eqp gives every slot that will run, before any fiber starts, what the chosen form needs and nothing of
 *   the other: a batch that only runs the sparse form has dense_bytes == 0 on every slot (asm_kkt_form_info through asm_batch_handle).
 *   The dense fallback is decided there once for all slots: without a sparse pattern on slot 0, or with one too dense to order, every
 *   slot runs the dense form.  Inside a round the static order neither allocates on the device, nor waits for the stream, nor copies
 *   from pageable memory.  Bit-identity as stated above: scenario s equals asm_slp_run_eqp on a fresh handle with the same form and
 *   order. */
int asm_batch_kkt_set_form(asm_batch* b, int32_t form, int32_t order);
/* ---- Scenario batches: KKT solves and sensitivities.
 * asm_kkt_solve_multi, asm_solution_sensitivity_multi and asm_bound_sensitivity_multi with a leading scenario dimension on every array
 * but rows and delta (and DC with dc_per_scenario == 0), which all scenarios share: x, bound_state are n_scen x n, lambda, row_state
 * n_scen x m, RU, DX, DZ n_scen x nrhs x n, RW, DLAM n_scen x nrhs x m, info n_scen x nrhs, DC nrhs x n_dpar or n_scen x nrhs x n_dpar.
 * n_scen may exceed the slot count: the slots take the scenarios in index order, each evaluated with its row of the scenario data table
 * (asm_batch_set_scenario_data) or, without a table, with the data of asm_batch_eval_setup.
 *   Per scenario the entry IS the per-handle entry, for every nrhs: scenario s is bit-identical to that entry on a fresh handle that has
 *   the scenario's data and the batch's form and order (asm_batch_kkt_set_form) - whatever the slot, the group, the slot count or the
 *   scenarios beside it.  The slots' launches merge as in every batch entry, and the lockstep rounds of the columns become rounds of the
 *   batch: the host reads one word per slot and round.
 *   Before any fiber starts every slot that will run gets the work area of ASM_KKT_CHUNK columns in the batch's form - per column
 *   14 ldn + 5 ldT + Mp doubles, and per slot the transposed factor (ld^2 doubles) and, dense form, the unmasked transposed working rows
 *   (ldn ldT doubles) - the Hessian workspace on the batch's shared lists and, for asm_batch_solution_sensitivity, the cross-derivative
 *   workspace: no allocation, no clearing fill and no blocking copy inside a round.  The dense fallback of the sparse form is decided on
 *   slot 0 for all slots.  The Hessian is the exact one.
 *   Errors: ASM_ERR_STATE before asm_batch_setup / asm_batch_eval_setup; a model without second derivatives is refused as by
 *   asm_batch_hessian_*, one without cross derivatives (asm_batch_solution_sensitivity) as by asm_solution_sensitivity_multi, both before
 *   any fiber starts; n_scen < 1, nrhs < 1, a null required pointer, a row index outside [0, m), dc_per_scenario outside {0, 1}:
 *   ASM_ERR_ARG; n_scen unequal to the height of a scenario table: as every batch entry.  A scenario's own refusal (more working rows
 *   than free variables, a state outside its values) is that slot's error with the per-handle code, and the batch stays usable.  A column
 *   status - iteration limit, indefinite reduced Hessian, dropped pivots - is reported in info and is not an error. */
int asm_batch_kkt_solve(asm_batch* b, int64_t n_scen, const double* x, const double* lambda, const int32_t* row_state,
                        const int32_t* bound_state, int32_t nrhs, const double* RU, const double* RW, const asm_kkt_params* par, double* DX,
                        double* DLAM, double* DZ /* may be NULL */, asm_kkt_info* info);
int asm_batch_solution_sensitivity(asm_batch* b, int64_t n_scen, const double* x, const double* lambda, const int32_t* row_state,
                                   const int32_t* bound_state, int32_t nrhs, const double* DC,
                                   int32_t dc_per_scenario /* 0: [nrhs x n_dpar] for all; 1: [n_scen x nrhs x n_dpar] */,
                                   const asm_kkt_params* par, double* DX, double* DLAM, double* DZ, asm_kkt_info* info);
int asm_batch_bound_sensitivity(asm_batch* b, int64_t n_scen, const double* x, const double* lambda, const int32_t* row_state,
                                const int32_t* bound_state, int32_t nrhs, const int32_t* rows /* [nrhs], shared */,
                                const double* delta /* [nrhs] or NULL: 1.0, shared */, const asm_kkt_params* par, double* DX, double* DLAM,
                                double* DZ, asm_kkt_info* info);
/* asm_solution_adjoint_multi with a leading scenario dimension on every array: GX, AX n_scen x nrhs x n, GL, DBOUND, AL n_scen x nrhs x m,
 * OUT n_scen x nrhs x n_dpar, info n_scen x nrhs (DBOUND, AX, AL may be NULL).  Everything said above holds: each scenario runs with its
 * row of the scenario data table, n_scen may exceed the slot count, the solves run in the batch's KKT form, the workspaces - the transposed
 * sweep's too - are made before the fibers start, and scenario s is bit-identical to asm_solution_adjoint_multi on a fresh handle with that
 * scenario's data.  Errors as for asm_batch_solution_sensitivity. */
int asm_batch_solution_adjoint(asm_batch* b, int64_t n_scen, const double* x, const double* lambda, const int32_t* row_state,
                               const int32_t* bound_state, int32_t nrhs, const double* GX, const double* GL, const asm_kkt_params* par,
                               double* OUT, double* DBOUND, double* AX, double* AL, asm_kkt_info* info);
/* asm_var_bound_sensitivity_multi with a leading scenario dimension, as asm_batch_bound_sensitivity: vars and delta are shared by the
 * scenarios, an index outside [0, n) is ASM_ERR_ARG, and scenario s is bit-identical to the per-handle entry on a fresh handle with that
 * scenario's data (dense form, and sparse form in the static order).
 * asm_solution_adjoint_z_multi with a leading scenario dimension, as asm_batch_solution_adjoint: GZ, DXBOUND n_scen x nrhs x n (both may
 * be NULL); what the weights need on a slot - the complementary mask and, dense form, J[W, B] (min(m, n) ldn doubles) - is made before
 * the fibers start. */
int asm_batch_var_bound_sensitivity(asm_batch* b, int64_t n_scen, const double* x, const double* lambda, const int32_t* row_state,
                                    const int32_t* bound_state, int32_t nrhs, const int32_t* vars /* [nrhs], shared */,
                                    const double* delta /* [nrhs] or NULL: 1.0, shared */, const asm_kkt_params* par, double* DX, double* DLAM,
                                    double* DZ, asm_kkt_info* info);
int asm_batch_solution_adjoint_z(asm_batch* b, int64_t n_scen, const double* x, const double* lambda, const int32_t* row_state,
                                 const int32_t* bound_state, int32_t nrhs, const double* GX, const double* GL, const double* GZ,
                                 const asm_kkt_params* par, double* OUT, double* DBOUND, double* DXBOUND, double* AX, double* AL,
                                 asm_kkt_info* info);
/* asm_sensitivity_range_multi with a leading scenario dimension ("Validity ranges" above) */
int asm_batch_sensitivity_range(asm_batch* b, int64_t n_scen, const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub,
                                const double* x, const double* lambda, const double* z, const int32_t* row_state, const int32_t* bound_state,
                                int32_t nrhs, const double* DX, const double* DLAM, const double* DZ, asm_range_info* out);
/* what the launch merging did since the batch was created */
typedef struct {
    int64_t rounds;        /* scheduler rounds (one blob copy + one completion wait each) */
    int64_t ops;           /* operations the slots recorded (= launches the per-handle path would have made) */
    int64_t launches;      /* launches actually made */
    int64_t releases;      /* barrier groups released */
    int64_t blob_bytes;    /* argument tables + copy payloads sent to the device */
    double  emit_ms, wait_ms, host_ms, wall_ms;   /* merging + launching, waiting for the device, solver host code, total */
    /* the dataflow panel kernels (k_chol_panel*: ASM_K_PANEL_KERNEL of a handle) as the batch runs them: HIP events around every merged launch
     * on its group's stream (ASM_HIP_TIMING != 0), the launches the slots recorded, and their algorithmic flops / bytes summed over the slots */
    double  panel_ms;
    int64_t panel_launches, panel_ops;
    double  panel_flops, panel_bytes;
    int64_t panel_grid_max;   /* most workgroups of any all-resident launch the batch made (merged launches included): stays within the
                               * group's share of the device's panel budget */
} asm_batch_stats;
int asm_batch_get_stats(const asm_batch* b, asm_batch_stats* out);

/* Test hook: the matrices loaded by asm_test_cholesky / asm_test_chol_solve / asm_test_trsm_rows are banded with this half-bandwidth
 * (0 = dense): factorisation and substitutions stop at the band, as they do for S0 = A_EF A_EF' of the null-space form (its equality
 * rows are put in reverse Cuthill-McKee order at set-up). */
int asm_test_set_band(asm_handle* h, int band);
/* Test hook: how asm_test_cholesky / asm_test_chol_solve / asm_test_trsm_rows factor from now on.  layout 0: in the main buffers (wide
 * blocks of 1024 above order 1536, else 512); layout 1: in a factor buffer of the null-space form's kind (ns_alloc_factor with band_hint:
 * one 1024-wide block up to order 1024).  mode / rel / absv: the regularisation of the diagonal (k_diag_prepare), thr: the static pivot
 * guard of the factorisation.  (0, 0, 0, 0.0, 0.0, 1e-14) are the settings the hooks use until this is called. */
int asm_test_set_factor(asm_handle* h, int layout, int band_hint, int mode, double rel, double absv, double thr);

/* ---- kernel-level test hooks (used by tests/ to check each kernel against NumPy) ---------------- */
int asm_test_syrk(asm_handle* h, const double* A, int64_t M, int64_t K, const int32_t* idx, int64_t Ms,
                  const double* theta, const double* diag, double* S_out /* Ms*Ms, lower valid */, int tile);
/* S[a,b] -= sum_k P[a,k] P[b,k], a >= b (b < MsB when MsB >= 0), the block at (srow0, srow0) of a larger matrix: the Cholesky update */
int asm_test_syrk_update(asm_handle* h, const double* P /* Ms*K */, int64_t Ms, int64_t K, int64_t MsB, int64_t srow0,
                         double* S_inout /* Ms*Ms */, int tile);
/* Test hook: the chunk-skipping Schur build as Dev::schur_syrk launches it for a row list (k_tile_nzflags, then k_syrk with the chunk list;
 * use_flags = 0: the same launch without flags), on the caller's operand A (M x K, K a multiple of 32, at most 32768).  tile 1 / 2 / 4, or 0 =
 * the solver's choice for Ms.  S_inout (ldS x ldS) is pre-filled by the caller; flags_out holds ceil(Ms / (32 tile)) x K / 32 bytes. */
int asm_test_build_flagged(asm_handle* h, const double* A, int64_t M, int64_t K, const int32_t* idx /* Ms or NULL */, int64_t Ms,
                           const double* theta /* K */, const double* diag /* Ms or NULL */, int tile, int use_flags, double* S_inout,
                           int64_t ldS, unsigned char* flags_out, double* fraction_out);
/* Test hook: the k x k matrix of a null-space iteration as the solver builds it, up to its factorisation (nsplit > 1: split-K slices and their
 * reduction; 1: the plain build, its copy and the diagonal preparation).  G is k x K; with ld = k rounded up to 32 the caller pre-fills
 * parts_inout (nsplit x ld x ld), S_inout, N0_inout (ld x ld) and diag0_inout (ld). */
int asm_test_build_split(asm_handle* h, const double* G, int64_t k, int64_t K, const double* theta /* K */, int nsplit, double rel,
                         double absv, double* parts_inout, double* S_inout, double* N0_inout, double* diag0_inout);
/* Test hook: the Newton-matrix builds of a handle set up by asm_sublp_setup, through the solver's own dispatch.  The Jacobian is assembled
 * from dE and scaled by rows (unit column scale).  which: 0 all rows (Pattern flags), 1 column form on the transposed copy, 2 the row list
 * idx (gathered with per-call flags, or from the structural pairs in a banded row order), 3 column form from the structural column pairs,
 * 4 S0 of the null-space form, < 0 only the outputs below.  S_inout is the whole factor buffer (info[4]^2 doubles, info[7]^2 for which = 4),
 * pre-filled by the caller.  info (12): M, n, row_band, col_band, main pitch, nE, S0 band, S0 pitch, column form possible, row flags valid,
 * column flags valid, sparse pattern.  Ah_out: the operand on the device (M x n).  Orders: position -> index, -1 without one. */
int asm_test_build_dispatch(asm_handle* h, const double* dE, int which, const int32_t* idx, int64_t Ms, const double* theta,
                            const double* diag, double* S_inout, double* Ah_out, int64_t* info, int32_t* row_order, int32_t* col_order,
                            int32_t* e_order);
/* Test hook: the interior-point stage kernels (asm_ipm_kernels.hip.h), one launch per stage with the solver's own launch geometry, on a state the
 * caller supplies.  The state of an LP with n columns, M rows and ns slack columns lives in an arena laid out by the solver's own binding
 * routine with the pitches asm_sublp_setup chooses for these sizes (ldn = n rounded up to 32, Mp = max(M, 1) and nsp = max(ns, 1) rounded up
 * to 16).  layout_out (ASM_IPM_LAYOUT_LEN) receives: ldn, Mp, nsp, arena length, snapshot length, int block length, number of scalars
 * (SC_COUNT), offset of the scalar block, then the offsets of the ASM_IPM_NVEC vectors in this order:
 *   q lb ub r w slo scoef | p s g y tL tU muL muU ts mus pi | act aty rp rdp rds thp_inv ths_inv dS hp hs tmpn t1 rhs res rcL rcU rcs rcg |
 *   dirA: dp ds dg dy dmuL dmuU dmus dpi | dirC: the same eight | sres corr pcg tN
 * (n-vectors have ldn, M-vectors Mp, slack vectors nsp entries).  With dbl_inout == NULL the call only reports the layout.
 *   dbl_inout  (ndbl >= arena length)  the arena, followed by any vectors of the caller's that helper stages name by offset; returned whole.
 *              The products with the LP matrix are inputs, not stages: the caller fills act, aty, t1, sres and tN.
 *   ints       (nint >= int block length)  rtype | rs0 | rs1 (Mp each; rs0 / rs1 = the up to two slack columns of a row, -1 for none) |
 *              srow (nsp), followed by the caller's index lists.
 *   snap_inout (snapshot length), rpart_inout (64 workgroups x 8 slots), rcnt_inout (1), hscal_inout (SC_COUNT; the host-mapped copy of the
 *              scalar block), hseq_inout (1; its sequence word): loaded before the first stage and returned after the last.
 *   stages     run in order on the handle's stream with no host synchronisation in between; grid_out[q] = workgroups stage q launched.
 * Scalars: PINF DINF MU YMAX AP AD SM EMAX RMAX RZ RPMAX RZ0 STOP NSERR SPEC (indices 0 .. 14).
 * Every offset, length and index is checked against the buffers before the first launch (ASM_ERR_ARG otherwise). */
enum {
    ASM_IPM_INIT_P = 0,   /* origin */
    ASM_IPM_INIT_REST,    /* mu_factor */
    ASM_IPM_MEASURES,     /* pub */
    ASM_IPM_THETA,        /* rho_p */
    ASM_IPM_RHS1,         /* mode 0 / 1 / 2, tp, td; B = base direction */
    ASM_IPM_RHS2,         /* res */
    ASM_IPM_VEC_MUL,      /* x[0] (in / out) *= x[1], len[0] entries */
    ASM_IPM_RES,          /* sres and D.dy; pub, spec, crel, floor_ */
    ASM_IPM_PCG_START,    /* z = corr, p = pcg */
    ASM_IPM_PCG_STEP1,    /* sres, p = pcg, x = D.dy; pub */
    ASM_IPM_PCG_STEP2,    /* z = corr, p = pcg */
    ASM_IPM_DIR,          /* D from D.dy and tN */
    ASM_IPM_STEPS,        /* D; pub */
    ASM_IPM_MUAFF,        /* D; sexp */
    ASM_IPM_DIRADD,       /* D += B */
    ASM_IPM_UPDATE,       /* D; al, be */
    ASM_IPM_SNAPSHOT,     /* dir 0 save / 1 restore; with_e: e = x[0] (ldn entries) */
    ASM_IPM_COL_PREP,     /* rho_p, fixed; dinv = x[0] (M), th = x[1] (n) */
    ASM_IPM_COL_SCALE,    /* dinv = x[0], r = x[1], u = x[2] (M each) */
    ASM_IPM_COL_FINISH,   /* dinv = x[0], u = x[1], w = x[2], out = x[3] (M each) */
    ASM_IPM_SDIAG_CSR,    /* ptr = ix[0] (len[0] + 1), col = ix[1]; vals = x[0], thinv = x[1] (len[1]), out = x[2] (len[0]) */
    ASM_IPM_RED_GATHER,   /* E = ix[0] (len[0] entries < len[1]); r = x[0] (len[1]), ce = x[1] */
    ASM_IPM_RED_SCATTER,  /* E = ix[0] (len[0]), ze = x[0]; I = ix[1] (len[1]), dI = x[1]; r = x[2], z = x[3] (len[2] each: the rows covered, at least max(len[0], len[1]): the grid is sized by it) */
    ASM_IPM_NKINDS
};
#define ASM_IPM_NVEC 56
#define ASM_IPM_LAYOUT_LEN (8 + ASM_IPM_NVEC)
typedef struct asm_ipm_stage {
    int32_t kind;                 /* ASM_IPM_* */
    int32_t mode, spec, sexp, origin, dir, with_e;
    int32_t D, B;                 /* 0 = dirA, 1 = dirC */
    uint32_t pub;                 /* publishing kernels: 0, or the sequence number to publish */
    double tp, td, res, crel, floor_, rho_p, mu_factor, al, be, fixed;
    int64_t x[4];                 /* offsets into dbl_inout */
    int64_t ix[2];                /* offsets into ints */
    int64_t len[3];
} asm_ipm_stage;
int asm_test_ipm_stages(asm_handle* h, int64_t n, int64_t M, int64_t ns, int64_t ncomp, double scale_q, int64_t* layout_out,
                        double* dbl_inout, int64_t ndbl, const int32_t* ints, int64_t nint, double* snap_inout, double* rpart_inout,
                        uint32_t* rcnt_inout, double* hscal_inout, uint32_t* hseq_inout, const asm_ipm_stage* stages, int64_t nstages,
                        uint32_t* grid_out);
/* Test hook: the active-set and optimal-face kernels (asm_as_kernels.hip.h), one launch per stage with the solver's own launch geometry, on a
 * state the caller supplies.  The state of an LP with n columns, M rows and ns slack columns (ns > 0 needs M > 0; M = 0 is admitted) lives in the
 * two arenas the solver's own binding routine lays out with the pitches asm_sublp_setup chooses (ldn, Mp, nsp as for asm_test_ipm_stages),
 * followed by the LP vectors and the part of the interior-point iterate that k_as_identify reads.  layout_out (ASM_AS_LAYOUT_LEN) receives:
 * ldn, Mp, nsp, length of the double block, length of the int block, offset of the scalar block `scal`, its length (PR DU EQRES HARDRES),
 * offset of the counter block `cnt` in the int block, its length (NH NF ANYSOFT NCHG NDIFF NVIOL NREL), then the offsets of the ASM_AS_NVEC
 * double vectors in this order:
 *   Fmask p z pB pF cF rd tN xfull nu | Hmask sl y act t bH v u yH yfull uacc ax | s |                                  (AsPtrs)
 *   pref zero p0 z0 pa pf zf | y0 act0 acta actf yf | s0 sa sf |                          (anchors and scratch vectors of the solver)
 *   q lb ub r w slo scoef | ip.p ip.tL ip.tU ip.muL ip.muU ip.g ip.pi ip.y ip.ts ip.mus ip.s          (LP, interior-point iterate)
 * and of the ASM_AS_NIVEC int vectors: rowst bst sst of the six working sets 0 .. 5 | ksoft Hidx hpos Fidx fpos | rtype rs0 rs1 srow rperm
 * (n-vectors have ldn, M-vectors Mp, slack vectors nsp entries).  With dbl_inout == NULL the call only reports the layout.
 *   dbl_inout (ndbl >= double block length)  the double block, followed by any vectors of the caller's that stages name by offset (x[]);
 *             loaded before the first stage, returned whole after the last.  Products with the LP matrix are inputs, not stages: the caller
 *             fills t and tN.
 *   int_inout (nint >= int block length)  the int block, in / out like the doubles: the kernels write sets and index lists.  rperm must hold
 *             row numbers whether a stage uses it or not.
 *   Ah        (ah_rows >= M rows of ldn doubles, row-major) the scaled LP matrix; read and uploaded only when a k_face_ns_col stage is present.
 *   stages    run in order on the handle's stream with no host synchronisation in between; grid_out[q] = workgroups stage q launched.
 * Checked before the first launch (ASM_ERR_ARG otherwise): every offset and length against the blocks, set numbers (0 .. 5), fam (0 .. 3) and e
 * (below M, ns, n, n for the families row, slack, lower, upper), k, rtype (-1 .. 1), rs0 / rs1 (-1 .. ns - 1), srow and rperm (0 .. M - 1); for a
 * stage that reads ksoft, Hidx, hpos or the count cnt[NH] before a stage of the same call has written them, the loaded values (ksoft -1 ..
 * ns - 1, Hidx 0 .. M - 1 over cnt[NH] <= M entries, hpos -1 .. Mp - 1).  k_face_ns_step marks the index its own ratio test finds; when
 * the test finds none although an inequality is violated (a ratio that is not a number) it marks nothing and reports NCHG = NDIFF = -1.
 * x[] entries of -1 pass a null pointer where the kernel takes one (*). */
enum {
    ASM_AS_IDENTIFY = 0,      /* set[0] = S (out); reads the ip.* vectors */
    ASM_AS_CLIP0,             /* src = x[0] (*), out = x[1]  (n each) */
    ASM_AS_SL,
    ASM_AS_SL_VALUES,
    ASM_AS_SMAX,              /* src = x[0], dst = x[1]  (ns each) */
    ASM_AS_SETUP,             /* set[0] = cur; p_ref = x[0] (*); rperm != 0: rows compacted in the order of rperm */
    ASM_AS_RHS,               /* y_ref = x[0] (*) */
    ASM_AS_RES_P,             /* k = the host's count of hard rows: sizes the grid */
    ASM_AS_SCATTER_H,         /* src = x[0] (Mp entries); accumulate */
    ASM_AS_ADD_F,
    ASM_AS_RD,
    ASM_AS_GATHER_H,          /* k as for RES_P */
    ASM_AS_ADD_YH,            /* k as for RES_P */
    ASM_AS_MERGE,             /* with_y */
    ASM_AS_FINISH,            /* set[0] = cur, set[1] = nx, set[2] = prev; have_prev, tol_p, tol_d */
    ASM_FACE_PRIMAL_FINISH,   /* set[0] = W, set[1] = part; tol_p, tol_m, check_only */
    ASM_FACE_NS_COMBINE,      /* p0 = x[0] (n), Zbuf = x[1] (k rows of ldn), u = x[2] (k), p = x[3] (n); k <= 4096 */
    ASM_FACE_NS_STEP,         /* set[0] = W; pa = x[0] (n), sa = x[1] (ns), acta = x[2] (M); tol_p */
    ASM_FACE_NS_COL,          /* fam, e; p0 = x[0] (n), t0 = x[1] (M); the matrix Ah */
    ASM_FACE_NS_Z,            /* z = x[0] (n) */
    ASM_FACE_NS_UNMARK,       /* set[0] = W; fam, e */
    ASM_FACE_DUAL_FINISH,     /* set[0] = D; tol_m */
    ASM_FACE_KKT,             /* set[0] = D */
    ASM_AS_PACK,              /* set[0] = S; dst = x[0]: 2n + 2M + ns doubles, then M + n + ns 32-bit integers */
    ASM_AS_COPY_SETS,         /* set[0] = dst, set[1] = src */
    ASM_AS_NKINDS
};
#define ASM_AS_NVEC 56
#define ASM_AS_NIVEC 28
#define ASM_AS_LAYOUT_LEN (9 + ASM_AS_NVEC + ASM_AS_NIVEC)
typedef struct asm_as_stage {
    int32_t kind;                 /* ASM_AS_* / ASM_FACE_* */
    int32_t with_y, accumulate, check_only, have_prev, rperm;      /* (the mode of an equality-constrained solve reaches its kernels as with_y / accumulate) */
    int32_t fam, k;
    int32_t set[3];               /* numbers of the working-set buffers the stage uses */
    int32_t pad_;
    int64_t e;
    double tol_p, tol_d, tol_m;
    int64_t x[4];                 /* offsets into dbl_inout */
} asm_as_stage;
int asm_test_as_stages(asm_handle* h, int64_t n, int64_t M, int64_t ns, double scale_q, int64_t* layout_out, double* dbl_inout, int64_t ndbl,
                       int32_t* int_inout, int64_t nint, const double* Ah, int64_t ah_rows, const asm_as_stage* stages, int64_t nstages,
                       uint32_t* grid_out);
/* Test hook: the kernels of one null-space interior-point iteration and of ns_finish_y (asm_ns_kernels.hip.h), one launch site per stage with
 * the solver's own launch geometry, on a state the caller supplies.  An LP with n columns and M rows (row types rtype: 0 = hard equality row,
 * at least one; no slack columns, as the form requires) and a null-space basis of k rows, 1 <= k <= n, k <= 1024.  One double block holds, in
 * this order: the interior-point arena (as for asm_test_ipm_stages with ns = 0) | theta~ (ldg = ldn + nIp) | the sixteen work vectors of the
 * form at the offsets the solver computes (0 dpbar, 1 K dpbar, 2 h~ / d0, 3 v / Z Zt d0, 5 yM, 7 bI, 10 ru, 11 du, 12 rr, 13 dd, 14 e) | Gt =
 * [Zt | GI'] (k + 1 rows of pitch ldg; the last row is never used) | the factor (fld x fld, fld = k rounded up to 32) | the inverses of its
 * 64-wide diagonal blocks | the unregularised N0 (fld x fld) | the scratch of Zt' u on the multi-launch path | any vectors of the caller's that
 * stages name by offset.  nEp = nE rounded up to 32, nIp = max(nI, 1) rounded up to 32.  layout_out (ASM_NS_LAYOUT_LEN) receives: ldn, Mp,
 * nEp, nIp, ldg, fld, nE, nI, length of the block, number of scalars, offset of the scalar block, of theta~, of Gt, rows of Gt, offset of the
 * factor, of the block inverses, their length, offset of N0, of the scratch, the largest order solved in one workgroup (ASM_SMALL_USE); then the
 * offsets of the sixteen work vectors; then those of the ASM_IPM_NVEC arena vectors in the order of asm_test_ipm_stages.  With dbl_inout ==
 * NULL the call only reports the layout (rtype is read, the matrix is not).
 *   ptr, col, vals  the LP matrix as CSR (M + 1 pointers, columns < n).  The hook makes the CSC view and the index lists with the routines
 *              asm_sublp_setup uses and returns them in idx_out: sc_ptr (n + 1) | sc_row | sc_pos (nnz each) | Eidx (nE) | Epos (M) | Iidx (nI) |
 *              Ipos (M).
 *   Nreg, N0   the regularised and the unregularised reduced matrix, dense k x k.  N0 is stored into the block as the solver's build stores it
 *              (lower triangle; mirrored into the upper one for k <= ASM_SMALL_USE).  ASM_NS_FACTOR factors Nreg in a buffer of the null-space
 *              form's kind with the pivot reference diag(N0), as Solver::ns_iter_setup does; the factor and its block inverses are returned in
 *              the block (what the block held there on entry is ignored).
 *   hscal_inout (number of scalars), hseq_inout (1): the host-mapped copy of the scalar block and its sequence word, in and out.
 *   stages     run in order on the handle's stream with no host synchronisation in between; grid_out[q] = workgroups of stage q (composite
 *              stages: of their first kernel of asm_ns_kernels.hip.h; 0 where none applies).
 * Checked before the first launch (ASM_ERR_ARG otherwise): the sizes, row types (-1 .. 1), CSR pointers (from 0, not decreasing), columns (< n),
 * every offset and length against the block, selectors, and that a stage that solves comes after ASM_NS_FACTOR in the same call. */
enum {
    ASM_NS_THETA = 0,         /* k_ipm_theta_ns; rho_p */
    ASM_NS_FACTOR,            /* Dev::chol(fN, k, 1e-14, no explicit inverse) */
    ASM_NS_E0,                /* k_ns_e0: pbar = x[0] (ldn) -> work vector 2 */
    ASM_NS_ZT,                /* gemv_rows: x[1] (k) = Zt x[0] (ldn) */
    ASM_NS_GEMV_T,            /* Solver::ns_gemv_t_dense: x[1] (ldn) = Zt' x[0] (k); k_gemv_t_small, or k_gemv_t_stage1 / 2 above ASM_SMALL_USE */
    ASM_NS_E1,                /* k_ns_e1: work vectors 2, 3 -> e */
    ASM_NS_WM_NEG,            /* k_ns_spmvn_wm_neg */
    ASM_NS_KX,                /* k_ns_spmvt_kx */
    ASM_NS_RHS1_BI,           /* k_ns_rhs1_bi; mode, B = base direction, res */
    ASM_NS_HT,                /* k_ns_spmvt_ht; res */
    ASM_NS_RU,                /* gemv_rows: ru = Zt v */
    ASM_NS_REDUCED_SOLVE,     /* Solver::ns_reduced_solve: k_ns_reduced_solve, or chol_solve_dev / k_ns_symv_res / chol_solve_add_dev (k_wtrsv_bwd_diag_add) / k_ns_relres above ASM_SMALL_USE */
    ASM_NS_DIRECTION,         /* Solver::ns_direction: k_gemv_t_small_dp, or k_gemv_t_stage1 + k_gemv_t_stage2_dp; D, res */
    ASM_NS_ROWS,              /* k_ns_spmvn_rows; D */
    ASM_NS_NEWTON,            /* Solver::ns_newton(mode, B, D): the six stages above in one */
    ASM_NS_CHOL_SOLVE,        /* Dev::chol_solve_dev on the factor: x[1] = N^-1 x[0] (k each); k_small_solve up to ASM_SMALL_USE */
    ASM_NS_SYMV_RES,          /* k_ns_symv_res: x[2] = x[1] - N0 x[0] (k each) */
    ASM_NS_ADD,               /* k_ns_add: x[2] = x[0] + x[1] (len) */
    ASM_NS_RELRES,            /* k_ns_relres: r = x[0], rhs = x[1] (k each) into scalar NSERR */
    ASM_NS_DP,                /* k_ns_dp; D, res, zu = x[0] (ldn) */
    ASM_NS_UPDATE,            /* k_ns_update; D, al, be, es */
    ASM_NS_UPDATE_DEV,        /* k_ns_update_dev; D, eta, rerr */
    ASM_NS_DINF,              /* k_ns_dinf: zr = x[0] (k); pub */
    ASM_NS_GATHER_E,          /* k_ns_gather_e: x[1] (nE) = scale * x[0][Eidx] (M) */
    ASM_NS_SCATTER_E,         /* k_ns_scatter_e: x[1][Eidx] (M) = (add ? x[1][Eidx] : 0) + x[0] (nE) */
    ASM_NS_ROWVEC_E,          /* k_ns_rowvec_e: x[1] (M) from x[0] (nE) */
    ASM_NS_FILL,              /* k_ns_fill: x[0][0:len] = val */
    ASM_NS_NKINDS
};
#define ASM_NS_LAYOUT_HEAD 20
#define ASM_NS_LAYOUT_LEN (ASM_NS_LAYOUT_HEAD + 16 + ASM_IPM_NVEC)
typedef struct asm_ns_stage {
    int32_t kind;                 /* ASM_NS_* */
    int32_t mode, add;
    int32_t D, B;                 /* 0 = dirA, 1 = dirC */
    uint32_t pub;
    double rho_p, res, al, be, es, eta, rerr, scale, val;
    int64_t x[4];                 /* offsets into dbl_inout */
    int64_t len;
} asm_ns_stage;
int asm_test_ns_stages(asm_handle* h, int64_t n, int64_t M, int64_t k, double scale_q, const int32_t* rtype, const int32_t* ptr,
                       const int32_t* col, const double* vals, const double* Nreg, const double* N0, int64_t* layout_out, int32_t* idx_out,
                       double* dbl_inout, int64_t ndbl, double* hscal_inout, uint32_t* hseq_inout, const asm_ns_stage* stages,
                       int64_t nstages, uint32_t* grid_out);
/* Test hook: the per-LP basis set-up of the null-space form (Solver::ns_setup with ns_reproject, ns_basis_from, ns_ortho and the cold column
 * selection), one launch site per stage with the solver's own launch geometry, on the form's own buffers.  The handle has been set up by
 * asm_sublp_setup and its skeleton has the form (ASM_ERR_ARG otherwise).  As in asm_test_build_dispatch the Jacobian is assembled from dE and
 * scaled by rows (unit column scale); take the operand from there (which < 0).
 *   fm         n entries, 1 = free column, 0 = fixed: the LP's bounds are lb = 0, ub = fm.
 *   k, k_reserve >= k   rows of the basis the primitive stages work on; the k-sized buffers are those Solver::ns_reserve makes for an earlier LP
 *              of the skeleton with k_reserve rows (cap = NsLayout::kcap(k_reserve) rows; buffers of another reservation are dropped first,
 *              those of the same one are kept with what they hold).
 *   J          the basis columns (k entries in [0, n); NULL where no stage reads them).
 *   layout_out (ASM_NSS_LAYOUT_LEN) receives ldn, nEp, nIp, ldg, nE, nI, band of S0 (0 = dense), pitch of S0, cap, pitch and wide-block width of
 *              the k x k factor fN, n, M, pitch of the main factor, Mp.  idx_out (nE + nI, or NULL): Eidx | Iidx.  With stages == NULL the call
 *              makes the reservation and reports these two only.
 *   G_inout (cap x ldg: Gt = [Zt | GI']), R_inout, X_inout (cap x nEp), SN_inout (the factor buffer of fN, pitch x pitch), Y_inout (the two
 *              blocks of the cold selection, ldn x nEp each: right-hand sides | L0^-1 a_j), T_inout (the main factor, pitch x pitch), d_inout
 *              (ldn: the vector ASM_NSS_DIAG writes): each loaded before the first stage and returned whole after the last; NULL: left as it is.
 *              The solver relies on the zeros the second block of Y is made with beyond column nE (the padding of L0^-1 a_j, an operand of
 *              the cold selection's matrix that no launch writes): the stages of the call see what the caller loaded there, the hook puts
 *              the zeros back before it returns.
 *   f0_out, Lt_out (nEp x nEp, or NULL): the factor of S0 and its transposed copy after the last stage.
 *   Zk, hint_J (nhint entries)  for ASM_NSS_SETUP: rows of the previous LP's basis in G (NsK::Zk) and the retained columns (SolveHint::ns_J).
 *   stages     run in order on the handle's stream; the host waits only where the solver does (the dropped-pivot counts, the diagonal of the
 *              cold selection).  grid_out[q]: workgroups (x) of the stage's kernel of asm_ns_kernels.hip.h, of the first one for REPROJECT and
 *              BASIS_FROM; 0 where the stage is a factorisation, a product or a substitution.  res_out[q]: the dropped pivots (S0_FACTOR,
 *              FACTOR_N), the count (COUNT_BIG), 1 / 0 for the composites.  setup_out (4 + n) of the last ASM_NSS_SETUP: what made the basis (1
 *              the previous basis, 2 the retained columns, 3 the cold selection, 0 none), k, dropped pivots of S0, length of J, J.
 * Checked before the first launch (ASM_ERR_ARG otherwise): the sizes (1 <= k <= n, k <= k_reserve <= 1.5 NS_MAX_RATIO M + 8), fm, every column
 * index, flags, and the order of the stages: TRSM, REPROJECT and BASIS_FROM after S0_FACTOR, ORTHO after FACTOR_N in the same call. */
enum {
    ASM_NSS_S0_FACTOR = 0,    /* the head of ns_setup: mask upload, Dev::ns_build_S0, diag_prepare, chol(f0, nE, 1e-10), ns_count_big, transpose into Lt */
    ASM_NSS_RHS_COLS,         /* k_ns_rhs_cols; flag 0: columns J into R (grid k), 1: all n columns into Y (cold selection) */
    ASM_NSS_ROWS_E,           /* k_ns_rows_e: R from Zt */
    ASM_NSS_TRSM,             /* Dev::trsm_rows on f0; flag 1: R, X with k rows, forward and backward; 0: the n rows of Y, forward only */
    ASM_NSS_PJ,               /* k_ns_pj; flag = second_pass */
    ASM_NSS_GATHER_T,         /* k_ns_gather_t */
    ASM_NSS_GRAM,             /* launch_syrk of Zt into fN.S as ns_reproject calls it */
    ASM_NSS_FACTOR_N,         /* pivot reference 1, chol(fN, k, thr), ns_count_big */
    ASM_NSS_ORTHO,            /* Solver::ns_ortho: k_transpose_dense + gemm_nt for k <= fN.wb, k_ns_ortho otherwise */
    ASM_NSS_GI,               /* k_ns_gi */
    ASM_NSS_SET_DIAG,         /* k_ns_set_diag on the main factor, order n; flag 0: the mask, 1: a null vector */
    ASM_NSS_DIAG,             /* k_ns_diag of the main factor, order n */
    ASM_NSS_COUNT_BIG,        /* k_ns_count_big on the main factor; flag = the order */
    ASM_NSS_REPROJECT,        /* Solver::ns_reproject(k, thr) */
    ASM_NSS_BASIS_FROM,       /* Solver::ns_basis_from(J) */
    ASM_NSS_SETUP,            /* Solver::ns_setup on the LP of fm */
    ASM_NSS_NKINDS
};
#define ASM_NSS_LAYOUT_LEN 16
typedef struct asm_nss_stage {
    int32_t kind;                 /* ASM_NSS_* */
    int32_t flag;
    double thr;
} asm_nss_stage;
int asm_test_ns_setup_stages(asm_handle* h, const double* dE, const double* fm, int64_t k, int64_t k_reserve, const int32_t* J,
                             int64_t* layout_out, int32_t* idx_out, double* G_inout, double* R_inout, double* X_inout, double* SN_inout,
                             double* Y_inout, double* T_inout, double* d_inout, double* f0_out, double* Lt_out, int32_t Zk,
                             const int32_t* hint_J, int64_t nhint, const asm_nss_stage* stages, int64_t nstages, uint32_t* grid_out,
                             int32_t* res_out, int32_t* setup_out);
/* Test hook: the kernels of the KKT column family (asm_kkt_kernels.hip.h) and of the SLP-EQP trial step (asm_eqp_kernels.hip.h), one launch
 * site per stage - the functions the drivers themselves launch through - on blocks the hook allocates with the solver's pitches.  Needs a
 * handle from asm_create only, no model.  n variables, M LP rows, nW <= capW working rows, cols <= ASM_KKT_CHUNK columns; ldn = n rounded up
 * to 32, ldT = max(capW, 1) rounded up to 32, Mp = max(M, 1) rounded up to 16 and not below 32, nWp / nWg = nW rounded up to 32 / 64.
 * layout_out (ASM_KKT_LAYOUT_LEN) receives: ldn, ldT, Mp, nWp, nWg, the length of the double block, of the int block, then the offsets in
 * the double block of: the 14 blocks over the variables (block k at + k 64 ldn: b_ru dx0 d r p hraw hp tt dx hdx q jtl dz g), the 5 blocks
 * over the working rows (block k at + k 64 ldT: rww tw spare dlw adx), dlf (64 x Mp), mask (ldn), rad (64), scal (64 x 16 + 1: the columns'
 * scalar blocks, then the active-column word), part (64 x KK_MAXWG x KK_SLOTS); then the offsets in the int block of wrow (Mp), wpos (Mp),
 * rows (64), counts (4); then the doubles per scalar block and the partial-sum slots per column.  With dbl_inout == NULL the call only
 * reports the layout.
 *   dbl_inout / int_inout   the blocks, each followed by vectors / lists of the caller's that stages name by offset; loaded before the first
 *                           stage, returned whole after the last.  i64 (ni64 entries): read-only 64-bit lists, named by offset lx[].
 *   cnt_inout (65), act_inout (64)   the arrival counters (the last one counts finished columns) and the active flags
 *   hscal_inout (1), hseq_inout (1)  the host-mapped active-column word and its sequence word, made as asm_sublp_setup makes the handle's
 * Products with A, A', H by the dense back ends and the substitutions are inputs, not stages.  The kernels run with an empty batch table.
 * Checked before the first launch (ASM_ERR_ARG otherwise): sizes, every offset and length against its block, every index a list holds
 * (wrow, wpos, rows, col, row, pos, poth, pent, perm, twin, the LP states), that pointer lists do not decrease, and cols.
 * x[] / ix[] entries of -1 pass a null pointer where the kernel takes one (*). */
enum {
    ASM_KKT_GATHER = 0,      /* J = x[0] (len[0] rows of ldn), Aw = x[1] (nW rows of ldn) */
    ASM_KKT_GATHER_T,        /* J = x[0] (len[0] rows), AT = x[1] (ldn x ldT); flag[0]: masked */
    ASM_KKT_HESS_PRODUCT,    /* V = x[0] (64 rows of ldn), OUT = x[1] (cols rows), values = x[2] (len[0]); pptr = lx[0] (n + 1), pent = lx[1], poth = lx[2] */
    ASM_KKT_AXPBY,           /* a = x[0], b = x[1] (*), out = x[2]; s[0] = sa, s[1] = sb; flag[0]: mask, flag[1]: scal, flag[2]: blocks over the working rows */
    ASM_KKT_SCATTER,         /* y = x[0] (cols rows of ldT), out = x[1] (cols rows of Mp) */
    ASM_KKT_CROSS_RHS,       /* cx = x[0] (n + M - len[0]), n_fn = len[0]; ru = x[1] (n), rww = x[2] (nW) */
    ASM_KKT_CROSS_RHS_COLS,  /* cx = x[0] (cols rows of pitch len[1] >= n + M - len[0]), n_fn = len[0]; ru = x[1], rww = x[2] (blocks) */
    ASM_KKT_BOUND_RHS,       /* delta = x[0] (*) (cols), ru = x[1], rww = x[2] (blocks); the rows list of the int block */
    ASM_KKT_CG_P,            /* g = x[0], p = x[1] */
    ASM_KKT_NORMAL,          /* dx0 = x[0]; s[0] = share; the radii of the double block */
    ASM_KKT_CG_CURV,         /* p = x[0], hp_raw = x[1], d = x[2], hp = x[3]; flag[0]: the trust-region form */
    ASM_KKT_CG_STEP,         /* p = x[0], hp = x[1], d = x[2], r = x[3] */
    ASM_KKT_CG_DIR,          /* r = x[0]; flag[0]: init, flag[1]: tr; s[0] = rtol; pub */
    ASM_KKT_FINISH,          /* hdx = x[0], ru = x[1], jtl = x[2], adx = x[3], rww = x[4], dz = x[5], dx = x[6] (*) */
    ASM_KKTS_VALS,           /* dE = x[0] (len[1]), vals = x[1] (len[0] = nu); perm = lx[0], ustart = lx[1] (nu + 1) */
    ASM_KKTS_WPOS,           /* wrow, wpos of the int block */
    ASM_KKTS_MUL_A,          /* val = x[0], V = x[1], T = x[2] (blocks); ptr = ix[0] (M + 1), col = ix[1] */
    ASM_KKTS_MUL_AT,         /* val = x[0] (len[0]), Y = x[1], V = x[2] (blocks); cptr = ix[0] (n + 1), row = ix[1], pos = ix[2]; flag[0]: masked */
    ASM_EQP_FACE,            /* len[0] = n, len[1] = m, len[2] = twins; s[0] = tol; E g_L g_U x x_L x_U = x[0 .. 5], rw = x[6]; lp_rows lp_bnd twin = ix[0 .. 2],
                                rows bnd side counts = ix[3 .. 6] */
    ASM_EQP_TRIAL,           /* len[0] = n; dx x x_L x_U = x[0 .. 3], d = x[4], out = x[5] (4) */
    ASM_KKT_NKINDS
};
#define ASM_KKT_LAYOUT_LEN 20
typedef struct asm_kkt_stage {
    int32_t kind;                 /* ASM_KKT_* / ASM_KKTS_* / ASM_EQP_* */
    int32_t flag[3];
    uint32_t pub;                 /* k_kktm_cg_dir: 0, or the sequence number to publish */
    int32_t pad_;
    double s[2];
    int64_t len[3];
    int64_t x[7];                 /* offsets into dbl_inout */
    int64_t ix[7];                /* offsets into int_inout */
    int64_t lx[3];                /* offsets into i64 */
} asm_kkt_stage;
int asm_test_kkt_stages(asm_handle* h, int64_t n, int64_t M, int64_t nW, int64_t capW, int32_t cols, int64_t* layout_out, double* dbl_inout,
                        int64_t ndbl, int32_t* int_inout, int64_t nint, const int64_t* i64, int64_t ni64, uint32_t* cnt_inout,
                        uint32_t* act_inout, double* hscal_inout, uint32_t* hseq_inout, const asm_kkt_stage* stages, int64_t nstages,
                        uint32_t* grid_out);
int asm_test_cholesky(asm_handle* h, const double* S /* N*N sym */, int64_t N, double* L_out /* N*N lower */);
int asm_test_chol_solve(asm_handle* h, const double* S, int64_t N, const double* b, double* x);
/* the bounded wait of the dataflow panel kernel with a producer that never publishes: returns ASM_ERR_HIP (reported once), the
 * handle stays usable */
int asm_test_panel_timeout(asm_handle* h, int workgroups);
/* on != 0: every active-set attempt (polish) of the following LPs on this handle fails, so that the solve ends on its last resort - the
 * converged interior iterate, asm_solve_stats.path 10 (oracle: tests patch eqp_loop / face_polish the same way) */
int asm_test_no_polish(asm_handle* h, int on);
/* the lockstep rounds the last asm_kkt_solve_multi / asm_solution_sensitivity_multi on this handle ran, summed over its chunks, and the last
 * active-column word its host loop read (0: the loop ended because no column was active) */
int asm_test_kkt_multi_rounds(const asm_handle* h, int64_t* rounds, int32_t* last_active);
/* C = (mode 1: C0) -/+ A B'  (A: Ma x K, B: Mb x K, row-major, K a multiple of 32) - the product kernel of the multi-right-hand-side
 * triangular solves of the null-space form */
int asm_test_gemm_nt(asm_handle* h, const double* A, const double* B, const double* C0, int64_t Ma, int64_t Mb, int64_t K, int mode,
                     double* C_out);
/* rows of R (nrhs x N) solved against the Cholesky factor of S: forward only (L x = r) or forward + backward (S x = r) */
int asm_test_trsm_rows(asm_handle* h, const double* S, int64_t N, const double* R, int64_t nrhs, int backward, double* X_out);
int asm_test_gemv(asm_handle* h, const double* A, int64_t M, int64_t K, const double* x, const double* y,
                  double* Ax, double* ATy);
int asm_test_assemble(asm_handle* h, const double* dE, double* J_out /* (m+nadj)*n */);
/* The stages between "dE is on the device" and "the scaled LP matrix is ready and can be multiplied", on the skeleton asm_sublp_setup made
 * (dense_fast, general dense or sparse pattern - whichever the set-up chose), through the functions asm_sublp_solve launches them by.  The
 * stages named in `stages` run in this order, each from the state the previous one (or an earlier call) left:
 *   ASM_SKS_ASSEMBLE   dE (nnz) is uploaded and J assembled; J_out: the whole Mp x ldn image of J, padding included
 *   ASM_SKS_COLSCALE   rmax_out (M): the row maxima max_k |J_ik| as the column reduction divides by them (1 for a row of zeros); rel_out (n): the
 *                      column maxima of |J_ij| / max_k |J_ik|; c_out (n): the column scale pow2_round(min(max(ub, -lb), 1 / rel)) of the box
 *                      lb / ub (n each)
 *   ASM_SKS_SCALE      Ah = diag(1 / rho) J diag(c) with c = c_in (n) when given, else the c of ASM_SKS_COLSCALE of this call (neither:
 *                      ASM_ERR_ARG); rho_out (M), Ah_out: the Mp x ldn image of Ah, spvAh_out (sp_nnz; may be NULL): on a sparse pattern the
 *                      scaled values in pattern order
 *   ASM_SKS_PRODUCTS   Jx_out = J x (M), JTy_out = J'y (n), Ahx_out = Ah x, AhTy_out = Ah'y for the probes x (n) and y (M); route_out[0 / 1]: the
 *                      route of J'y / Ah'y - 0 the CSC copy, 1 the transposed copy, 2 the two-stage column reduction, -1 an LP without rows
 *   ASM_SKS_NORMS      norms_out (m): the row norms of J by the dense kernel; spnorms_out (m; may be NULL): on a sparse pattern the same from
 *                      the CSR copy
 * info_out (ASM_SKS_INFO_LEN, filled by every accepted call, stages == 0 included): n, m, M, Mp, ldn, sparse pattern (0 / 1), its entries,
 * dense_fast (0 / 1), the chunk count R and the rows per chunk of the two-stage column reductions.  ASM_ERR_STATE before asm_sublp_setup;
 * a stage bit outside ASM_SKS_ALL, info_out == NULL or a null pointer among what a requested stage reads or writes (unless marked): ASM_ERR_ARG,
 * checked before anything runs.  ASM_SKS_ASSEMBLE drops the inputs of a resident solve (asm_sublp_upload again); bounds, retained sets and
 * hints stay, and asm_sublp_solve works on as before. */
enum { ASM_SKS_ASSEMBLE = 1, ASM_SKS_COLSCALE = 2, ASM_SKS_SCALE = 4, ASM_SKS_PRODUCTS = 8, ASM_SKS_NORMS = 16, ASM_SKS_ALL = 31 };
#define ASM_SKS_INFO_LEN 10
int asm_test_skeleton_stages(asm_handle* h, uint32_t stages, const double* dE, const double* lb, const double* ub, const double* c_in,
                             const double* x, const double* y, int64_t* info_out, double* J_out, double* rmax_out, double* rel_out,
                             double* c_out, double* rho_out, double* Ah_out, double* spvAh_out, double* Jx_out, double* JTy_out, double* Ahx_out,
                             double* AhTy_out, int32_t* route_out, double* norms_out, double* spnorms_out);
/* FP64 MFMA peak probe (back-to-back v_mfma_f64_16x16x4_f64, registers only): measured roofline denominator. */
int asm_test_mfma_peak(asm_handle* h, int iters, int waves_per_simd, double* tflops);

/* Test hook for the copy and fill operations of the stream recorder (csrc/asm_batch.hip.h: k_bcopy / k_bfill).  Two device buffers A and B of
 * 64 + span + 64 bytes each (a 64-byte margin on each side, the working area 64-byte aligned behind the first) are loaded with a_init / b_init
 * (64 + span + 64 bytes each), then asmb::copy_async / asmb::fill_async run on the handle's stream in this order, each with the call's `bytes`,
 * for every bit of `ops`:
 *   ASM_CF_H2D    host_src (bytes)  -> A + 64 + dst_off        ASM_CF_D2D   A + 64 + src_off -> B + 64 + dst_off
 *   ASM_CF_FILL   value -> B + 64 + fill_off                    ASM_CF_D2H   B + 64 + src_off -> host_out (bytes)
 * a_out / b_out: the whole buffers afterwards, margins included.  Offsets >= 0 and offset + bytes <= span, else ASM_ERR_ARG (nothing runs);
 * bytes == 0 is accepted and changes nothing.  On a plain handle these are the plain stream operations, on a batch slot
 * (asm_batch_test_run) recorded operations merged across the scenarios. */
enum { ASM_CF_H2D = 1, ASM_CF_D2D = 2, ASM_CF_FILL = 4, ASM_CF_D2H = 8, ASM_CF_ALL = 15 };
int asm_test_copy_fill(asm_handle* h, uint32_t ops, int64_t span, int64_t bytes, int64_t dst_off, int64_t src_off, int64_t fill_off, int32_t value,
                       const uint8_t* a_init, const uint8_t* b_init, const uint8_t* host_src, uint8_t* host_out, uint8_t* a_out, uint8_t* b_out);

/* The kernel hooks above on the fibers of a scenario batch: scenario s of n_scen runs hook `family` on its slot's handle exactly as the
 * per-handle hook would (the slots take the scenarios in index order, as in every asm_batch_* entry), so the launches, copies and fills of
 * the scenarios are recorded and merged.  records: n_scen records of the family's type below - the hook's parameters after h, in order;
 * status_out[s]: the code the per-handle hook would have returned for scenario s (its message in the slot handle's asm_last_error).  The
 * call itself fails only for a bad argument or a failed round.  Hooks that need asm_sublp_setup first need asm_batch_setup here.
 * asm_test_mfma_peak and asm_test_panel_timeout stay per-handle.  asm_batch_test_record_size: sizeof the family's record (-1: no such family). */
enum { ASM_TF_SKELETON_STAGES = 0, ASM_TF_IPM_STAGES, ASM_TF_AS_STAGES, ASM_TF_NS_STAGES, ASM_TF_NS_SETUP_STAGES, ASM_TF_KKT_STAGES, ASM_TF_CHOLESKY,
       ASM_TF_CHOL_SOLVE, ASM_TF_TRSM_ROWS, ASM_TF_GEMM_NT, ASM_TF_GEMV, ASM_TF_SYRK, ASM_TF_SYRK_UPDATE, ASM_TF_BUILD_SPLIT, ASM_TF_COPY_FILL, ASM_TF_COUNT };
typedef struct { uint32_t stages; const double *dE, *lb, *ub, *c_in, *x, *y; int64_t* info_out; double *J_out, *rmax_out, *rel_out, *c_out, *rho_out, *Ah_out,
                 *spvAh_out, *Jx_out, *JTy_out, *Ahx_out, *AhTy_out; int32_t* route_out; double *norms_out, *spnorms_out; } asm_test_skeleton_stages_args;
typedef struct { int64_t n, M, ns, ncomp; double scale_q; int64_t* layout_out; double* dbl_inout; int64_t ndbl; const int32_t* ints; int64_t nint;
                 double *snap_inout, *rpart_inout; uint32_t* rcnt_inout; double* hscal_inout; uint32_t* hseq_inout; const asm_ipm_stage* stages;
                 int64_t nstages; uint32_t* grid_out; } asm_test_ipm_stages_args;
typedef struct { int64_t n, M, ns; double scale_q; int64_t* layout_out; double* dbl_inout; int64_t ndbl; int32_t* int_inout; int64_t nint; const double* Ah;
                 int64_t ah_rows; const asm_as_stage* stages; int64_t nstages; uint32_t* grid_out; } asm_test_as_stages_args;
typedef struct { int64_t n, M, k; double scale_q; const int32_t *rtype, *ptr, *col; const double *vals, *Nreg, *N0; int64_t* layout_out; int32_t* idx_out;
                 double* dbl_inout; int64_t ndbl; double* hscal_inout; uint32_t* hseq_inout; const asm_ns_stage* stages; int64_t nstages;
                 uint32_t* grid_out; } asm_test_ns_stages_args;
typedef struct { const double *dE, *fm; int64_t k, k_reserve; const int32_t* J; int64_t* layout_out; int32_t* idx_out; double *G_inout, *R_inout, *X_inout,
                 *SN_inout, *Y_inout, *T_inout, *d_inout, *f0_out, *Lt_out; int32_t Zk; const int32_t* hint_J; int64_t nhint; const asm_nss_stage* stages;
                 int64_t nstages; uint32_t* grid_out; int32_t *res_out, *setup_out; } asm_test_ns_setup_stages_args;
typedef struct { int64_t n, M, nW, capW; int32_t cols; int64_t* layout_out; double* dbl_inout; int64_t ndbl; int32_t* int_inout; int64_t nint; const int64_t* i64;
                 int64_t ni64; uint32_t *cnt_inout, *act_inout; double* hscal_inout; uint32_t* hseq_inout; const asm_kkt_stage* stages; int64_t nstages;
                 uint32_t* grid_out; } asm_test_kkt_stages_args;
typedef struct { const double* S; int64_t N; double* L_out; } asm_test_cholesky_args;
typedef struct { const double* S; int64_t N; const double* b; double* x; } asm_test_chol_solve_args;
typedef struct { const double* S; int64_t N; const double* R; int64_t nrhs; int backward; double* X_out; } asm_test_trsm_rows_args;
typedef struct { const double *A, *B, *C0; int64_t Ma, Mb, K; int mode; double* C_out; } asm_test_gemm_nt_args;
typedef struct { const double* A; int64_t M, K; const double *x, *y; double *Ax, *ATy; } asm_test_gemv_args;
typedef struct { const double* A; int64_t M, K; const int32_t* idx; int64_t Ms; const double *theta, *diag; double* S_out; int tile; } asm_test_syrk_args;
typedef struct { const double* P; int64_t Ms, K, MsB, srow0; double* S_inout; int tile; } asm_test_syrk_update_args;
typedef struct { const double* G; int64_t k, K; const double* theta; int nsplit; double rel, absv; double *parts_inout, *S_inout, *N0_inout,
                 *diag0_inout; } asm_test_build_split_args;
typedef struct { uint32_t ops; int64_t span, bytes, dst_off, src_off, fill_off; int32_t value; const uint8_t *a_init, *b_init, *host_src; uint8_t *host_out,
                 *a_out, *b_out; } asm_test_copy_fill_args;
int asm_batch_test_run(asm_batch* b, int32_t family, int64_t n_scen, const void* records, int32_t* status_out);
int64_t asm_batch_test_record_size(int32_t family);

/* Per-kernel merge table of a batch: for every (kernel, gridDim.z of one scenario) the groups' schedulers launched while counting was on - the
 * kernel's name (hipKernelNameRefByPtr, cut to 255 characters), the operations the slots recorded, the launches made for them, the most
 * scenarios one launch served (nb_max) and gz.  asm_test_batch_kernel_counting switches the counting of every group (off by default unless
 * ASM_BATCH_VERBOSE=1; it survives asm_batch_set_groups) and clears the table; asm_test_batch_kernel_table writes up to `cap` rows, *n_rows =
 * the number there are (rows may be NULL with cap 0), and clears the table when reset != 0.  Rows are summed over the groups. */
typedef struct { char name[256]; int64_t operations, launches; int32_t nb_max, gz; } asm_batch_kernel_row;
int asm_test_batch_kernel_counting(asm_batch* b, int on);
/* the panel budget of a group of the batch: the most workgroups an all-resident launch of its scheduler may have, merged launches included
 * (the device's budget divided by the number of groups; asm_batch_stats.panel_grid_max stays within it).  -1: no such batch or group. */
int asm_test_batch_panel_share(const asm_batch* b, int group);
int asm_test_batch_kernel_table(asm_batch* b, asm_batch_kernel_row* rows, int64_t cap, int64_t* n_rows, int reset);

#ifdef __cplusplus
}
#endif
#endif
