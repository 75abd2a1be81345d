// libasmhip: host-side solver logic + C ABI (include/asm_hip.h) above the gfx950 kernels in
// asm_kernels.hip.h.  The algorithm (scaling -> warm active-set verify -> Mehrotra IPM in Schur form ->
// partition identification -> active-set Schur/Cholesky polish) is specified in DESIGN.md; reference
// citations for the formulation are given at each step (file:line under the reference tree).
//
// Split of work: the LP solve runs on the GPU from assembly to the polish, vector algebra included; the
// host chooses the path, launches, and reads back a few scalars per iteration to decide the next step.
// Stream operations of the solver go through asmb:: (asm_batch.hip.h): plain stream operations for a
// single handle, recorded and merged across scenarios inside a scenario batch.
#include "asm_kernels.hip.h"
#include "asm_ipm_kernels.hip.h"
#include "asm_as_kernels.hip.h"
#include "asm_ns_kernels.hip.h"
#include "asm_eval_kernels.hip.h"
#include "asm_kkt_kernels.hip.h"
#include "asm_eqp_kernels.hip.h"
#include "asm_range_kernels.hip.h"
#include "asm_lm_kernels.hip.h"
#include "asm_batch.hip.h"
#include "../../include/asm_hip.h"

#include <sched.h>
#include <time.h>
#include <atomic>
#include <thread>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <numeric>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

namespace {

const double INF = std::numeric_limits<double>::infinity();
const double TOL_P = 1e-9, TOL_D = 1e-6;
const int IPM_MAXIT = 60;
const double IPM_GAP_DONE = 1e-3, IPM_DINF_FLOOR = 1e-6;      // stage complete with the dual residual on the solves' accuracy floor (oracle/lp_solver.py)
const double JAM_PINF = 1e-6;    // below this a stagnating primal residual is rounding-level, not a jam (oracle/lp_solver.py)
const int IPM_MCC = 2;           // Gondzio centrality correctors per iteration (oracle/lp_solver.py)
const double MCC_DELTA = 0.3, MCC_BMIN = 0.1, MCC_BMAX = 10.0, MCC_GAMMA = 0.1;
// inner / outer panel widths of the three-level Cholesky.  Inner = 512 = eight 64-wide steps per dataflow launch (ASM_PNL_NS) and ONE
// K = 512 update of the rest of the outer panel; measured at M = 1024 / 1725 / 3889 / 11192 / 18637: 256 -> 0.603 / 1.093 / 2.79 / 14.7 /
// 44.95 ms, 512 -> 0.583 / 1.062 / 2.60 / 14.0 / 43.95 ms, 768 -> 0.674 / 1.226 / 2.96 / 15.0 / 45.0 ms, 1024 -> 0.847 / 1.365 / 3.24 /
// 15.7 / 46.4 ms (wider: the rank-64 updates inside the launch grow onto the critical path; narrower: more launches and more of the
// poorly filled in-panel updates)
const int CHOL_NBI = 512, CHOL_NBO = 1024;
// column (Sherman-Morrison-Woodbury) form of the Newton system for restoration LPs (oracle/lp_solver.py: COL_*)
const int COL_MIN_M = 64, COL_MAX_CG = 6;
const double COL_MAX_RATIO = 0.8, COL_FIXED = 1e200;
// reduced row form of the normal-phase Newton system, large sparse problems only (oracle/lp_solver.py: RED_*)
const int RED_MIN_M = 4096, RED_MAX_CG = 10;
const double RED_TAU = 100.0, RED_MIN_FRAC = 0.1;
// null-space form of the normal-phase Newton system (oracle/lp_solver.py: NS_*)
const int NS_MIN_E = 64;
const double NS_MAX_RATIO = 0.3, NS_WARM_THR = 1e-6, NS_ZWARM_THR = 0.25, NS_BIG = 0.5e128, NS_RERR = 1e-6;
const int NS_CMAX = 2;
const double IPM_DEGRADE = 10.0;  // oracle/lp_solver.py: a stage that ends this much worse than the best stage so far is undone (best-iterate safeguard)
const int WARM_BACKOFF_MAX = 6;  // oracle/lp_solver.py: pause after consecutive failed warm attempts doubles up to 2^6 - 1 LPs
const double EQP_RUNAWAY = 10.0, EQP_MAXCHG = 0.03;
const int EQP_MINCHG = 32;  // oracle/lp_solver.py: growth of the primal residual between two rounds of a bulk correction that ends the attempt
const int64_t RCM_MAX_PAIRS = 50000000;      // sum over the columns of (rows in the column)^2 beyond which no row order is computed
const double IPM_MU0_NORMAL = 0.3;      // oracle/lp_solver.py: initial complementarity of a normal-phase LP in units of scale_q
const double IPM_TOL0 = 3e-10;      // oracle/lp_solver.py: IPM_STAGES - tolerance of the first identification (then 0.1 IPM_TOL0, then 1e-12)
const int IPM_SIG_EXP = 3;          // oracle/lp_solver.py: centring parameter sigma = (mu_aff / mu) ** 3
const double IPM_ETA0 = 0.995;      // oracle/lp_solver.py: fraction of the step to the boundary while mu >= 1 (then max(IPM_ETA0, 1 - mu / scale_q), at most 0.999999)
const double IPM_ACCEPT = 1e-8, IPM_ACCEPT_DUAL = 1e-8;      // oracle/lp_solver.py: last-resort acceptance of a converged iterate (primal residual and gap; dual residual)
const int NS_MAX_SPLIT = 8;
const double NS_SEL_THR[4] = {1e-2, 1e-4, 1e-7, 1e-10};
const int PCG_MAXIT = 20;       // conjugate-gradient steps per Newton solve (preconditioner = the Cholesky factor)
const double PCG_KAPPA = 1e-3;  // Newton-system residual tolerance relative to the current primal residual
const double IPM_RHO_P = 1e-8;   // primal proximal regularisation of the Newton system
// canonical pair of a non-unique optimum (oracle/lp_solver.py: FACE_*)
const int FACE_BULK = 12, FACE_STEPS = 400;
const double FACE_TOL_M = 1e-9;

struct HipError : std::runtime_error {
    explicit HipError(const std::string& s) : std::runtime_error(s) {}
};
struct Unsupported : std::invalid_argument {      // valid input the library cannot represent (an LP skeleton the reference cannot build)
    explicit Unsupported(const std::string& s) : std::invalid_argument(s) {}
};
#define HIPCHK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            throw HipError(std::string(#expr) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + ":" +   \
                           std::to_string(__LINE__) + ")");                                              \
    } while (0)

inline int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

inline double pow2_round(double x) {
    if (!(x > 0.0)) return 1.0;
    int e;
    double f = std::frexp(x, &e);
    if (f < 0.70710678118654752) e -= 1;
    return std::ldexp(1.0, e);
}

typedef std::vector<double> vec;
typedef std::vector<int8_t> ivec;

struct ActiveSet {
    ivec rowst, bst, sst;
    bool valid = false;
};

// adaptive decisions carried from one LP of a phase to the next (oracle/lp_solver.py: solve_scaled `hint`)
struct SolveHint {
    int warm_fail = 0, warm_skip = 1;     // the first re-solve of a phase is not attempted
    bool stable = false;                  // the last two LPs of the phase ended on the same active sets
    bool prefer_ref;                      // starts true in the restoration phase: its LPs usually have a non-unique optimum (oracle/subproblem.py)
    std::vector<int> ns_J;                // basis columns of the null-space form retained from the previous LP of the phase
    explicit SolveHint(bool restoration) : prefer_ref(restoration) {}
};

struct TimedRegion {
    hipEvent_t a, b;
    int kind;
    hipStream_t stream;     // the stream the timed launches go to (the look-ahead stream has its own regions)
};

// one Cholesky factor with the explicit inverses the substitution kernels use (the null-space form keeps two besides the main one)
// Reverse Cuthill-McKee order of the rows `rows` of the CSR pattern (sp_ptr, sp_col); two rows are adjacent when they share a column.
// Deterministic (oracle: rcm_order): components are started from the unvisited row of least degree (ties: first in `rows`), the
// breadth-first search appends the unvisited neighbours by (degree, position in `rows`), the whole order is reversed.  Returns positions
// into `rows`; *bandwidth = the largest distance between two adjacent rows in the new order; *pairs = the (row, column) positions, in the
// new order, of the structural non-zeros of the lower triangle of the rows' Gram matrix.
static std::vector<int> rcm_order(const std::vector<int>& rows, const std::vector<int>& sp_ptr, const std::vector<int>& sp_col, int64_t ncols, int* bandwidth,
                                  std::vector<int>* pairs = nullptr) {
    const int nR = (int)rows.size();
    std::vector<std::vector<int>> col_rows((size_t)ncols);
    for (int i = 0; i < nR; ++i)
        for (int k = sp_ptr[rows[i]]; k < sp_ptr[rows[i] + 1]; ++k) col_rows[sp_col[k]].push_back(i);
    // a column shared by very many rows makes the coupling graph (and its Gram matrix) dense: no order then (oracle: RCM_MAX_PAIRS)
    {
        int64_t npair = 0;
        for (const auto& v : col_rows) npair += (int64_t)v.size() * (int64_t)v.size();
        if (npair > RCM_MAX_PAIRS) {
            std::vector<int> id(nR);
            for (int i = 0; i < nR; ++i) id[i] = i;
            if (bandwidth) *bandwidth = nR;
            if (pairs) pairs->clear();
            return id;
        }
    }
    std::vector<std::vector<int>> nbr((size_t)nR);
    for (int i = 0; i < nR; ++i) {
        std::vector<int>& v = nbr[i];
        for (int k = sp_ptr[rows[i]]; k < sp_ptr[rows[i] + 1]; ++k) v.insert(v.end(), col_rows[sp_col[k]].begin(), col_rows[sp_col[k]].end());
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        v.erase(std::remove(v.begin(), v.end(), i), v.end());
    }
    std::vector<int> deg(nR);
    for (int i = 0; i < nR; ++i) deg[i] = (int)nbr[i].size();
    auto by_deg = [&](int a, int b) { return deg[a] != deg[b] ? deg[a] < deg[b] : a < b; };
    for (int i = 0; i < nR; ++i) std::sort(nbr[i].begin(), nbr[i].end(), by_deg);
    std::vector<int> starts(nR), order;
    for (int i = 0; i < nR; ++i) starts[i] = i;
    std::sort(starts.begin(), starts.end(), by_deg);
    std::vector<char> seen(nR, 0);
    order.reserve(nR);
    for (int s0 : starts) {
        if (seen[s0]) continue;
        seen[s0] = 1;
        size_t head = order.size();
        order.push_back(s0);
        while (head < order.size()) {
            const int v = order[head++];
            for (int u : nbr[v])
                if (!seen[u]) { seen[u] = 1; order.push_back(u); }
        }
    }
    std::reverse(order.begin(), order.end());
    std::vector<int> pos(nR);
    for (int q = 0; q < nR; ++q) pos[order[q]] = q;
    int bw = 0;
    for (int i = 0; i < nR; ++i)
        for (int u : nbr[i]) bw = std::max(bw, std::abs(pos[i] - pos[u]));
    if (bandwidth) *bandwidth = bw;
    if (pairs) {                    // structural non-zeros (new row, new column <= row) of the rows' Gram matrix, diagonal included
        pairs->clear();
        for (int i = 0; i < nR; ++i) {
            pairs->push_back(pos[i]); pairs->push_back(pos[i]);
            for (int u : nbr[i])
                if (pos[u] < pos[i]) { pairs->push_back(pos[i]); pairs->push_back(pos[u]); }
        }
    }
    return order;
}
// CSC view of a CSR pattern with n columns: column pointers, row of every entry, and the place of its value in the CSR list (stable: rows
// ascending inside a column)
static void csc_from_csr(const std::vector<int>& sp_ptr, const std::vector<int>& sp_col, int64_t n, std::vector<int>& sc_ptr, std::vector<int>& sc_row, std::vector<int>& sc_pos) {
    const int64_t R = (int64_t)sp_ptr.size() - 1, nnzS = (int64_t)sp_col.size();
    sc_ptr.assign(n + 1, 0);
    for (int64_t k = 0; k < nnzS; ++k) sc_ptr[sp_col[k] + 1] += 1;
    for (int64_t j = 0; j < n; ++j) sc_ptr[j + 1] += sc_ptr[j];
    std::vector<int> fill(sc_ptr.begin(), sc_ptr.end() - 1);
    sc_row.resize(nnzS); sc_pos.resize(nnzS);
    for (int64_t i = 0; i < R; ++i)
        for (int k = sp_ptr[i]; k < sp_ptr[i + 1]; ++k) {
            const int q = fill[sp_col[k]]++;
            sc_row[q] = (int)i;
            sc_pos[q] = k;
        }
}
// Index lists of the null-space form for row types rtype[0:M] (0 = hard equality row): the equality rows E in reverse Cuthill-McKee order of
// their coupling graph (S0 = A_EF A_EF' and its factor are banded in that order), the inequality rows I in index order, and each row's place
// in its list (-1 in the other).  *s0_band / *s0_pairs: bandwidth and structural non-zeros of S0 in that order (rcm_order).
static void ns_index_lists(const int* rtype, int64_t M, const std::vector<int>& sp_ptr, const std::vector<int>& sp_col, int64_t ncols, std::vector<int>& eidx,
                           std::vector<int>& epos, std::vector<int>& iidx, std::vector<int>& ipos, int* s0_band, std::vector<int>* s0_pairs) {
    eidx.clear(); iidx.clear();
    epos.assign(M, -1); ipos.assign(M, -1);
    for (int64_t i = 0; i < M; ++i) {
        if (rtype[i] == 0) { epos[i] = (int)eidx.size(); eidx.push_back((int)i); }
        else { ipos[i] = (int)iidx.size(); iidx.push_back((int)i); }
    }
    const int nE = (int)eidx.size();
    const std::vector<int> ord = rcm_order(eidx, sp_ptr, sp_col, ncols, s0_band, s0_pairs);
    std::vector<int> e2(nE);
    for (int q = 0; q < nE; ++q) e2[q] = eidx[ord[q]];
    eidx.swap(e2);
    for (int q = 0; q < nE; ++q) epos[eidx[q]] = q;
}

struct FacBuf {
    double *S = nullptr, *Linv = nullptr, *Binv = nullptr, *BinvT = nullptr;
    int64_t ld = 0;
    int wb = 512;                   // wide-block width of its substitution kernels
    bool small = false;             // k x k systems of the null-space form: solved in one workgroup when the order is <= ASM_SMALL_MAX
    int band = 0;                   // > 0: the matrix is banded (entry (i, j) is zero when |i - j| > band) and so is its factor: every panel
                                    // operation stops `band` rows below the panel's last column
};

// the lockstep rounds of a KKT call, summed over its chunks, and the last active-column word it read
struct KktCounters { int64_t rounds = 0; int last_active = 0; };
// The buffers of the KKT solve on a working set, all in the evaluator's pool and made where first needed after asm_eval_setup (kk_prepare,
// kk_work); they go with the evaluator (EvalState).
struct KktWork {                    // steps 3 to 6 on blocks of up to `cap` columns (0: not made): 1 for asm_kkt_solve, KKM_CW for the multi entries
    int64_t cap = 0;
    double *vec = nullptr, *row = nullptr, *dlf = nullptr;      // 14 blocks cap x ldn over the variables, 5 cap x ldT over the working rows, cap x Mp over all rows
    double* rad = nullptr;                                      // cap trust-region radii (asm_kkt_step)
    double* bnd = nullptr;                                      // cap > 1: [delta (cap doubles) | rows or variables (cap ints)] of a chunk of bound sensitivities (k_kktm_bound_rhs, k_kktm_var_*)
    double* stage = nullptr;                                    // pinned: [ru | rw | directions] of a chunk, then its results
    double *Lt = nullptr, *AfT = nullptr;                       // cap > 1, the block products' own operands: the transposed factor, the unmasked transposed working rows (dense form only)
};
struct KktBufs {
    bool ready = false;
    int64_t capW = 0, ldT = 0;      // the most working rows the problem admits, min(m, n); the pitch of everything over them
    FacBuf fac;                     // S = A A' and its factor
    double *dE = nullptr, *J = nullptr, *Aw = nullptr, *AwT = nullptr;      // Jacobian values and dense J of the solve's own, A = J[W, F] and its transposed copy
    double *sets = nullptr, *h_sets = nullptr;                              // [mask (ldn doubles) | working-row list (Mp ints)] and its pinned image
    double *cmask = nullptr, *Ab = nullptr;                                 // asm_solution_adjoint_z* with weights on z (kk_gz): the mask of B, and J[W, B] (dense form only)
    int* dropped = nullptr;                                                 // the dropped-pivot count
    // the per-column reduction state, laid out for KKM_CW columns whatever the capacity (KktMulti)
    double *part = nullptr, *scal = nullptr;
    unsigned *cnt = nullptr, *act = nullptr;
    KktWork one, blk;
    // the form of the products and of S (asm_kkt_set_form) and what the last call did (asm_kkt_form_info)
    int form = ASM_KKT_DENSE;
    struct asm_kkt_form_info last{};
    bool dense_ready = false, sparse_ready = false;
    int64_t dense_bytes = 0, sparse_bytes = 0;      // device bytes of the buffers only the one form has
    // The factor is shared by the two forms, and the banded kernels never clear outside the band they are given, so the sparse branch of
    // KktFace clears explicitly: fac_full_rows = the leading rows of fac.S that a call may have filled over their whole width (a dense
    // call, or a sparse one whose band was too wide to use), fac_band_hw = the widest band a banded call has used since the buffer was made
    int64_t fac_full_rows = 0;
    int fac_band_hw = 0;
    // sparse form: the CSR values of the Jacobian at x, the place of every LP row in the order of the working rows, the structural pairs of S;
    // the order cache: the last row_state with its order (host), band and pairs (the device lists above are its device side)
    double* sp_vals = nullptr;
    int *wpos = nullptr, *pairs = nullptr;
    int64_t pairs_cap = 0, n_pairs = 0;
    std::vector<int32_t> c_state;
    std::vector<int> c_order;
    int c_band = 0;
    bool c_valid = false;
    // the row order of the sparse form (asm_kkt_set_order) and the one the last call used; c_kind: the order the cache above was made in (a
    // call in the other order misses: the two keep different lists on the device)
    int order = ASM_KKT_ORDER_WORKING_SET, order_used = ASM_KKT_ORDER_WORKING_SET, c_kind = ASM_KKT_ORDER_WORKING_SET;
    // static order: the reverse Cuthill-McKee order of all m rows (kk_sparse keeps it), its band, and the structural pairs of all rows as
    // row-index pairs - on the host for the band of a working set, on the device (kk_static, uploaded once) for the build of S.  s_place:
    // host scratch, the place of every row in the working set of the cache (-1: outside)
    std::vector<int> s_order, s_pairs_h, s_place;
    int* s_pairs = nullptr;
    int64_t s_npairs = 0;
    int s_band = 0;
    std::vector<int> last_rows;      // the working rows of the last KKT call in the order used (asm_kkt_row_order)
    // asm_eqp_trial (eq_prepare): [the LP's row_state (M) | its bound_state (n) | twin (m) || row_state (m) | bound_state (n) | counts (4) ||
    // side (m)], [rw (m) | dx (n) | d (n) | scalars (EQP_SCAL)], and the pinned image of both followed by n doubles for the gradient
    int* eq_i = nullptr;
    double *eq_d = nullptr, *eq_h = nullptr;
};

// What asm_sensitivity_range_multi keeps (rg_prepare, at the first call after asm_eval_setup): the Jacobian at the call's x as the values
// of the skeleton's CSR list (vals; a pattern without one: the dense rows J), the point's vectors, the blocks of a chunk's
// columns, the partial candidates of the two launches and the results.  Nothing here is read by another entry.
struct RangeBufs {
    bool ready = false;
    int64_t n_row_wg = 0, n_var_wg = 0;
    double *dE = nullptr, *vals = nullptr, *J = nullptr;        // nnz Jacobian values of the evaluation; sp_nnz CSR values, or Mp x ldn dense rows
    double* pt = nullptr;                                       // [lam (Mp) | z (ldn)] and behind them, as ints, [row_state (Mp) | bound_state (ldn)]
    double* cols = nullptr;                                     // a chunk's columns, packed: [DX (cols x ldn) | DZ (cols x ldn) | DLAM (cols x Mp)]
    double* part_t = nullptr;                                   // the partial candidates (RangeRed): slots x RG_CW x 2 ratios,
    int* part_k = nullptr;                                      // their positions and kinds,
    unsigned* cnt = nullptr;                                    // the arrival counters
    RangeOut* out = nullptr;                                    // RG_CW results
    double* stage = nullptr;                                    // pinned: the image of pt or of cols, then the results
};

// The device and pinned host buffers of one lifetime.  Each allocation is recorded with the field that points to it (and, for mapped host
// memory, the field that holds its device address); release() frees them all and nulls those fields.  Sizes are max(count, 1) elements.
class BufPool {
  public:
    enum Where { DEVICE, PINNED, MAPPED };      // MAPPED: pinned, host-mapped and coherent, its device address into *dev
    BufPool() = default;
    BufPool(const BufPool&) = delete;
    BufPool& operator=(const BufPool&) = delete;
    ~BufPool() { release(); }

    // uninitialised
    template <class T>
    T* alloc(T*& f, int64_t count, Where where = DEVICE, T** dev = nullptr) {
        const size_t bytes = std::max<int64_t>(count, 1) * sizeof(T);
        void* p = nullptr;
        if (where == DEVICE) HIPCHK(hipMalloc(&p, bytes));
        else HIPCHK(hipHostMalloc(&p, bytes, where == MAPPED ? hipHostMallocMapped | hipHostMallocCoherent : hipHostMallocDefault));
        own_.push_back({p, where != DEVICE, (void**)&f, (void**)dev});
        f = (T*)p;
        if (dev) HIPCHK(hipHostGetDevicePointer((void**)dev, p, 0));
        return f;
    }
    // device buffer cleared by asmb::fill_async on `s`, or by the synchronous asmb::fill without a stream
    template <class T>
    T* zeroed(T*& f, int64_t count, hipStream_t s) {
        HIPCHK(asmb::fill_async((void*)alloc(f, count), 0, std::max<int64_t>(count, 1) * sizeof(T), s));
        return f;
    }
    template <class T>
    T* zeroed(T*& f, int64_t count) {
        HIPCHK(asmb::fill((void*)alloc(f, count), 0, std::max<int64_t>(count, 1) * sizeof(T)));
        return f;
    }
    // device buffer holding src[0, count) (synchronous copy); zero_first: cleared by a synchronous fill before
    template <class T>
    T* upload(T*& f, const std::remove_const_t<T>* src, int64_t count, bool zero_first = false) {
        if (zero_first) zeroed(f, count);
        else alloc(f, count);
        if (count > 0) HIPCHK(asmb::copy((void*)f, src, count * sizeof(T), hipMemcpyHostToDevice));
        return f;
    }
    void release() {
        for (const Buf& b : own_) {
            if (b.host) (void)hipHostFree(b.p);
            else (void)asmb::free(b.p);
            *b.field = nullptr;
            if (b.dev) *b.dev = nullptr;
        }
        own_.clear();
    }

  private:
    struct Buf {
        void* p;
        bool host;
        void** field;
        void** dev;
    };
    std::vector<Buf> own_;
};

// What the Hessian of the Lagrangian needs besides a workspace, all of it fixed by the function store and the tape of asm_eval_setup: the
// pattern and the index lists in HBM.  A lone handle owns one; the slots of a batch share the batch's (asm_batch_hessian_*).
struct HsShared {
    BufPool mem;
    int64_t nfn = 0, wnodes = 0, S = 0, nocc = 0;   // entries of the function store (the block's follow); nodes of a workspace; seed threads; occurrences
    std::vector<int64_t> rows, cols;                // the pattern, 1-based
    int64_t *qterm = nullptr, *qrow = nullptr, *eptr = nullptr, *eocc = nullptr, *pptr = nullptr, *pent = nullptr, *poth = nullptr;
    int64_t *srow = nullptr, *svar = nullptr, *woff = nullptr, *optr = nullptr, *ovar = nullptr;
    int64_t nnz() const { return (int64_t)rows.size(); }
};

// The ONLY place that lays out the evaluator's vector block in HBM and its pinned staging buffer.  The block, in doubles:
//   [ g_L, g_U (m each) | x_L, x_U (n each) | lam (m), mU, mL (n each) | nu (m), ps (2 m), p (n) | jtl (ldn) | rown (Mp) | out (OUT) ]
// the bounds (ev_write_bounds), the one upload of asm_slp_norms, the one upload of ev_stage_step, J' lambda, the row norms of J, the
// reduction kernels' results.  Offsets and len() use the problem's own m: a model without rows has empty row vectors, and the block
// still ends with the whole of `out`, whose widest reader takes TRIALS + 2 <= OUT doubles.
struct EvLayout {
    static constexpr int64_t OUT = 16, TRIALS = 8;      // TRIALS merit values and {phi0, D} of a line search; RN_COUNT norms; 3 of a step quality
    int64_t n = 0, m = 0, ldn = 0, Mp = 0;
    double* d = nullptr;            // the block (EvalState's pool owns it)
    int64_t off(int k) const {      // where vector k of the block starts; off(13) is the block's length
        const int64_t w[13] = {m, m, n, n, m, n, n, m, 2 * m, n, ldn, Mp, OUT};
        return k == 0 ? 0 : off(k - 1) + w[k - 1];
    }
    int64_t len() const { return off(13); }
    double *g_L() const { return d + off(0); }  double *g_U() const { return d + off(1); }  double *x_L() const { return d + off(2); }  double *x_U() const { return d + off(3); }
    double *lam() const { return d + off(4); }  double *mU() const { return d + off(5); }   double *mL() const { return d + off(6); }
    double *nu() const { return d + off(7); }   double *ps() const { return d + off(8); }   double *p() const { return d + off(9); }
    double *jtl() const { return d + off(10); } double *rown() const { return d + off(11); } double *out() const { return d + off(12); }
    // The staging buffer holds one image at a time from offset 0: an evaluation [ x (n) | df (n) | E (m) | f ] (asm_eval_constraints: without
    // df), second derivatives [ x (n) | lam (m) | v (n) ] (asm_eval_data_gradient: without v), the image of lam | mU | mL or of nu | ps | p,
    // a read-back of `out`.  stage_len() is the maximum over these users.
    int64_t st_df() const { return n; }     int64_t st_E(bool df) const { return df ? 2 * n : n; }  int64_t st_f(bool df) const { return st_E(df) + m; }
    int64_t st_lam() const { return n; }    int64_t st_v() const { return n + m; }
    int64_t stage_len() const { return std::max({st_f(true) + 1, st_v() + n, nu() - lam(), jtl() - nu(), OUT}); }
};

// What runs an NLP block: nothing (the function store alone), the expression tape, the Ohm's-law kernel or the dense quadratic kernel.
// The kinds of the header map onto it below ("NLP block kinds"); the rest of the file reads what asm_eval_setup stored in EvalState.
enum class NlpFamily { NONE, EXPR, OHM, DENSE };

// The host-side form of an expression block after validation (expr_prepare): node references absolute, the slots of the VAR nodes
// (rows: Jacobian value from j0; terms: position in the per-variable gradient list)
struct ExprHost {
    int64_t R = 0, T = 0, L = 0;
    std::vector<int64_t> ptr, jptr, a, b, slot, gptr, cptr;   // cptr [n_dpar+1]: the CONST nodes grouped by dpar index (empty: no CONST node)
    std::vector<int32_t> op;
};

// Everything asm_eval_setup makes or that is made lazily after it, in one pool and with one lifetime: until the next asm_eval_setup or
// asm_sublp_setup.  The handle holds a pointer that is null while there is no evaluator (ev_of): no ready flag, no list of fields to reset.
struct EvalState {
    // What the block's kind means, derived once (nlp_setup): the family; whether second derivatives are announced (hs_check: every kind but
    // 1 and 2); whether derivatives with respect to the block's data exist (data_kind_check: kinds 3, 4 and 5); whether anything depends
    // on the data - a tape with a CONST node, a kernel with derivative entries and data - or every data derivative is zero, no launch
    NlpFamily family = NlpFamily::NONE;
    bool has_hess = true, has_data = false, data_dep = false;
    // the flattened function store, the NLP block (nlp_rows rows whatever the family) and its tape (asm_eval_kernels.hip.h), results in HBM
    int64_t nlp_rows = 0, fn_nnz = 0;
    FnStore F{};
    ExprTape X{};
    double *d_dpar = nullptr, *d_x = nullptr, *d_xt = nullptr, *d_df = nullptr, *d_E = nullptr, *d_Et = nullptr, *d_f = nullptr;
    EvLayout L;                     // reduction inputs (bounds, lambda, multipliers, nu, slacks, p) and results
    double* h_stage = nullptr;      // pinned staging, L.stage_len() doubles
    // NLP-block data (dpar): its length, and the range [dirty_lo, dirty_hi) asm_eval_set_data has written since asm_eval_setup (empty: the
    // device holds the setup values); expression tapes with constants: the data-gradient occurrence list (asm_eval_data_gradient)
    int64_t n_dpar = 0, dirty_lo = 0, dirty_hi = 0;
    int64_t *d_ipar = nullptr, *d_cptr = nullptr;
    double *d_cocc = nullptr, *d_lam = nullptr, *d_dgrad = nullptr, *h_dgrad = nullptr;
    // Hessian of the Lagrangian (asm_eval_hessian_*): made by the first of those calls after asm_eval_setup (hs_prepare) from the store and
    // the tape in HBM.  The pattern and the lists are hs_sh's (null: not prepared): the handle's own (hs_own), or for a batch slot that
    // asm_batch_hessian_* prepared the batch's; hs_H holds those lists with this handle's four node arrays and hocc; the workspace is in `mem`
    std::unique_ptr<HsShared> hs_own;
    const HsShared* hs_sh = nullptr;
    ExprHess hs_H{};
    double *d_hs_lam = nullptr, *d_hs_v = nullptr, *d_hs_vals = nullptr, *d_hs_out = nullptr, *h_hs = nullptr;
    void hs_forget() { hs_H = ExprHess{}; hs_sh = nullptr; }      // its lists are about to go; the workspace stays in `mem`
    // cross derivatives with respect to the data (asm_eval_data_cross and the sensitivity entries), made by the first call (cx_prepare).
    // With R = nlp_rows: d_cx_in = [lam (R) | cx_cap directions of n_dpar], d_cx_out = cx_cap columns [u (n) | w (R)], h_cx the pinned
    // staging of x, lam, one direction and one column.  The tape sweeps one direction at a time in cx_C's node arrays (cx_cap stays 1);
    // the kernels take 1 or KKM_CW columns, the Ohm's-law one with d_cx_occ = cx_cap x [4][nl] occurrences.  d_cx_vptr / d_cx_vnode: per
    // variable its VAR nodes (tape) or where its occurrences live in a column's (Ohm's law)
    ExprCross cx_C{};
    int64_t *d_cx_vptr = nullptr, *d_cx_vnode = nullptr;
    double *d_cx_in = nullptr, *d_cx_out = nullptr, *h_cx = nullptr, *d_cx_occ = nullptr;
    int64_t cx_cap = 0;
    // transposed cross derivatives (asm_eval_data_cross_t and the adjoint entries; ct_prepare): d_ct_in = [lam (R) | ct_cap columns
    // [vx (n) | vl (R)]], d_ct_out = ct_cap columns of n_dpar, h_ct the pinned staging of x, both and the read-back; ct_cap is 1 or
    // KKM_CW.  The tape runs in cx_C's node arrays and d_cocc.
    int64_t ct_cap = 0;
    double *d_ct_in = nullptr, *d_ct_out = nullptr, *h_ct = nullptr;
    bool ohm_vars_ok = true;        // Ohm's law with derivatives: every variable the block names is inside [0, n) (nlp_setup; refused by the data entries)
    KktBufs kk;                     // KKT solve on a working set (asm_kkt_solve and the multi entries)
    KktCounters kkm;                // test seam: the counters of the last multi call
    RangeBufs rg;                   // validity ranges (asm_sensitivity_range_multi)
    BufPool mem;                    // declared last: it goes first, while the fields it nulls are alive
};

// ---- NLP block kinds.  The ONLY place that knows what a kind of the header (ASM_NLP_*) means and what its family launches, with which
// grid and in which workspace.  The entries stage, check and read back the same way for every kind; where the kinds differ they call a
// function of this section or read the four facts nlp_setup stored (family, has_hess, has_data, data_dep), never the kind.  Kinds 4 and
// 5 are kinds 1 and 2 - same parameters, size checks and launches for values and Jacobian - that also announce their derivative entries:
// the Hessian and, in closed form, the derivatives with respect to their own data.  A new kind adds its case to nlp_family, nlp_setup's
// facts, nlp_check_sizes and nlp_rows_launch, and per derivative entry it announces to nlp_hess_lists / nlp_hess_launch,
// nlp_data_grad_launch, cx_prepare / nlp_cross_launch, nlp_cross_t_launch.  The caller has set the device; the launches go to `s`.
inline bool nlp_is_ohm(int kind) { return kind == ASM_NLP_ACOPF_OHM || kind == ASM_NLP_ACOPF_OHM_HESS; }
inline bool nlp_is_dense(int kind) { return kind == ASM_NLP_DENSE_QUADRATIC || kind == ASM_NLP_DENSE_QUADRATIC_HESS; }
inline bool nlp_block_derivs(int kind) { return kind == ASM_NLP_ACOPF_OHM_HESS || kind == ASM_NLP_DENSE_QUADRATIC_HESS; }
inline NlpFamily nlp_family(int kind) {
    return kind == ASM_NLP_EXPR ? NlpFamily::EXPR : nlp_is_ohm(kind) ? NlpFamily::OHM : nlp_is_dense(kind) ? NlpFamily::DENSE : NlpFamily::NONE;
}
// the parameter sizes of the kernel families (a tape's checks are expr_prepare's)
void nlp_check_sizes(int kind, int64_t n, int64_t nlp_rows, int64_t nlp_nnz, int64_t n_ipar, int64_t n_dpar) {
    if (nlp_is_ohm(kind) && (nlp_rows % 4 != 0 || nlp_nnz != 5 * nlp_rows || n_ipar != 7 + 2 * (nlp_rows / 4) || n_dpar != 8 * (nlp_rows / 4)))
        throw std::invalid_argument("asm_eval_setup: ACOPF block parameter sizes");
    if (nlp_is_dense(kind) && (nlp_nnz != nlp_rows * n || n_dpar != 2 * nlp_rows * n)) throw std::invalid_argument("asm_eval_setup: dense block parameter sizes");
}
// The block's part of asm_eval_setup, after F, nlp_rows, n_dpar and the parameters: the four facts, the tape (xh: what expr_prepare made
// of ipar) with its workspace, and what the data gradient needs - a batch calls that inside fibers and must not allocate there
void nlp_setup(EvalState& e, int kind, const ExprHost& xh, const int64_t* ipar) {
    BufPool& P = e.mem;
    const int64_t n = e.F.n, nd = e.n_dpar;
    e.family = nlp_family(kind);
    e.has_hess = kind != ASM_NLP_ACOPF_OHM && kind != ASM_NLP_DENSE_QUADRATIC;     // (their twins with second derivatives: kinds 4 and 5)
    e.has_data = e.family == NlpFamily::EXPR || nlp_block_derivs(kind);
    e.data_dep = e.family == NlpFamily::EXPR ? !xh.cptr.empty() : nlp_block_derivs(kind) && nd > 0;
    if (e.family == NlpFamily::EXPR) {
        ExprTape& X = e.X;
        X.R = xh.R; X.T = xh.T; X.L = xh.L; X.n = n;
        P.upload(X.ptr, xh.ptr.data(), (int64_t)xh.ptr.size()); P.upload(X.jptr, xh.jptr.data(), (int64_t)xh.jptr.size());
        P.upload(X.a, xh.a.data(), xh.L); P.upload(X.b, xh.b.data(), xh.L); P.upload(X.slot, xh.slot.data(), xh.L);
        P.upload(X.op, xh.op.data(), xh.L); P.upload(X.gptr, xh.gptr.data(), (int64_t)xh.gptr.size());
        X.cst = e.d_dpar;
        // workspace, sized here once: node values of 8 trial points, one set of adjoints, term values of 8 points, term adjoints
        P.zeroed(X.val, 8 * xh.L); P.zeroed(X.adj, xh.L);
        P.zeroed(X.tval, 8 * xh.T); P.zeroed(X.gocc, xh.gptr[n]);
        if (e.data_dep) {           // the data gradient's occurrence list
            P.upload(e.d_cptr, xh.cptr.data(), nd + 1);
            P.zeroed(e.d_cocc, xh.cptr[nd]);
        }
    }
    if (e.family == NlpFamily::EXPR ? e.data_dep : e.has_data) {       // the data gradient's multipliers of the rows and result
        P.zeroed(e.d_lam, e.nlp_rows); P.zeroed(e.d_dgrad, nd);
        P.alloc(e.h_dgrad, nd, BufPool::PINNED);
    }
    if (e.family == NlpFamily::OHM && e.has_data) {
        const int64_t nl = e.nlp_rows / 4;
        bool ok = ipar && ipar[0] == nl;
        for (int64_t l = 0; ok && l < 2 * nl; ++l) {
            const int64_t b = ipar[7 + l];
            ok = ipar[1] + b >= 0 && ipar[1] + b < n && ipar[2] + b >= 0 && ipar[2] + b < n;
        }
        e.ohm_vars_ok = ok;
    }
}

// Rows of the function store and of the block at the point xd: values into Ed, with `full` the Jacobian values into dE.  nt > 1 (values
// only): the trial points of a batched line search, xd / Ed advancing by ldx / ldE per point.  Two functions because asm_eval_functions
// launches the store's objective between them
void fn_rows_launch(const EvalState& e, hipStream_t s, const double* xd, double* Ed, double* dE, int full, unsigned nt = 1, int64_t ldx = 0, int64_t ldE = 0) {
    asmb::launch(k_fn_rows, dim3(asmb::blocks(e.F.n_rows).x, nt), dim3(256), s, e.F, xd, Ed, dE, full, ldx, ldE);
}
void nlp_rows_launch(const EvalState& e, hipStream_t s, const double* xd, double* Ed, double* dE, int full, unsigned nt = 1, int64_t ldx = 0, int64_t ldE = 0) {
    const int64_t R = e.nlp_rows, r0 = e.F.n_rows;
    switch (e.family) {
    case NlpFamily::NONE: break;
    case NlpFamily::EXPR: asmb::launch(k_nlp_expr_rows, dim3(asmb::blocks(R).x, nt), dim3(256), s, e.X, xd, Ed, dE, r0, e.fn_nnz, full, ldx, ldE); break;
    case NlpFamily::OHM: asmb::launch(k_nlp_acopf_ohm, dim3(asmb::blocks(R / 4).x, nt), dim3(256), s, e.d_ipar, e.d_dpar, xd, Ed, dE, r0, e.fn_nnz, full, ldx, ldE); break;
    case NlpFamily::DENSE: asmb::launch(k_nlp_dense_quadratic, dim3(asmb::blocks(R, 4).x, nt), dim3(256), s, e.d_dpar, R, e.F.n, xd, Ed, dE, r0, e.fn_nnz, full, ldx, ldE); break;
    }
}
// whether the block's objective replaces the store's objective row (a tape with terms), and its value into fd, with `full` its gradient into d_df
bool nlp_has_objective(const EvalState& e) { return e.family == NlpFamily::EXPR && e.X.T > 0; }
void nlp_objective_launch(const EvalState& e, hipStream_t s, const double* xd, double* fd, int full, unsigned nt, int64_t ldx) {
    if (!nlp_has_objective(e)) return;
    asmb::launch(k_nlp_expr_terms, dim3(asmb::blocks(e.X.T).x, nt), dim3(256), s, e.X, xd, full, ldx);
    asmb::launch(k_nlp_expr_objective, dim3(nt), dim3(64), s, e.X, e.F.objective_scale, fd);
    if (full) asmb::launch(k_nlp_expr_gradient, asmb::blocks(e.F.n), dim3(256), s, e.X, e.F.objective_scale, e.d_df);
}

template <class T>
std::vector<T> hs_download(const T* dev, int64_t count) {      // (a blocking copy: not inside a batch fiber)
    std::vector<T> v((size_t)std::max<int64_t>(count, 0));
    if (count > 0) HIPCHK(asmb::copy(v.data(), dev, count * sizeof(T), hipMemcpyDeviceToHost));
    return v;
}
// the interaction set P(last node) of the row or term with nodes [k0, k1) (absolute references), as pairs (j, i), j <= i, sorted by (j, i):
// the union over the nodes the last one depends on of what each op adds (the header's rule; POW / ATAN2 cover their operands' sets)
void hs_row_pairs(const int32_t* op, const int64_t* a, const int64_t* b, int64_t k0, int64_t k1, std::vector<std::vector<int64_t>>& L, std::vector<char>& reach,
                  std::vector<std::pair<int64_t, int64_t>>& P) {
    const int64_t len = k1 - k0;
    if ((int64_t)L.size() < len) L.resize(len);
    reach.assign(len, 0);
    reach[len - 1] = 1;
    for (int64_t q = len - 1; q >= 0; --q) {
        const int32_t o = op[k0 + q];
        if (!reach[q] || o == ASM_OP_CONST || o == ASM_OP_VAR) continue;
        reach[a[k0 + q] - k0] = 1;
        if ((o >= ASM_OP_ADD && o <= ASM_OP_DIV) || o >= ASM_OP_POW) reach[b[k0 + q] - k0] = 1;
    }
    P.clear();
    auto cross = [&P](const std::vector<int64_t>& A, const std::vector<int64_t>& B) {
        for (int64_t i : A)
            for (int64_t j : B) P.emplace_back(std::min(i, j), std::max(i, j));
    };
    for (int64_t q = 0; q < len; ++q) {
        const int64_t k = k0 + q;
        const int32_t o = op[k];
        std::vector<int64_t>& Lq = L[q];
        Lq.clear();
        if (o == ASM_OP_CONST) continue;
        if (o == ASM_OP_VAR) { Lq.push_back(a[k]); continue; }
        const std::vector<int64_t>& La = L[a[k] - k0];
        const bool binary = (o >= ASM_OP_ADD && o <= ASM_OP_DIV) || o >= ASM_OP_POW;
        if (!binary) Lq = La;
        else {
            const std::vector<int64_t>& Lb = L[b[k] - k0];
            Lq.resize(La.size() + Lb.size());
            Lq.erase(std::set_union(La.begin(), La.end(), Lb.begin(), Lb.end(), Lq.begin()), Lq.end());
        }
        if (!reach[q]) continue;
        switch (o) {
            case ASM_OP_ADD: case ASM_OP_SUB: case ASM_OP_NEG: case ASM_OP_MIN: case ASM_OP_MAX: break;
            case ASM_OP_MUL: cross(La, L[b[k] - k0]); break;
            case ASM_OP_DIV: cross(La, L[b[k] - k0]); cross(L[b[k] - k0], L[b[k] - k0]); break;
            case ASM_OP_POWI: if (b[k] != 1) cross(La, La); break;
            case ASM_OP_POW: case ASM_OP_ATAN2: cross(Lq, Lq); break;
            default: cross(La, La); break;       // every other unary op
        }
    }
    std::sort(P.begin(), P.end());
    P.erase(std::unique(P.begin(), P.end()), P.end());
}
// The block's second derivatives for hs_build: the tape's seed threads (srow, svar, woff over wnodes workspace nodes) with their
// occurrence lists (optr, ovar), the key i * n + j, i >= j, of every occurrence in list order (okey), where a listed occurrence lives
// (oslot; empty: in place), and the keys of entries the launch writes itself, without occurrences (own)
struct HsBlockLists {
    std::vector<int64_t> srow, svar, woff, optr{0}, ovar, okey, oslot, own;
    int64_t wnodes = 0;
};
HsBlockLists nlp_hess_lists(const EvalState& e) {
    HsBlockLists B;
    const int64_t n = e.F.n;
    switch (e.family) {
    case NlpFamily::NONE: break;
    case NlpFamily::EXPR: {
        // per row / term its interaction set, one seed thread per smaller index j with its occurrence list (i ascending)
        const ExprTape& X = e.X;
        const std::vector<int64_t> ptr = hs_download(X.ptr, X.R + X.T + 1), ta = hs_download(X.a, X.L), tb = hs_download(X.b, X.L);
        const std::vector<int32_t> top = hs_download(X.op, X.L);
        std::vector<std::vector<int64_t>> L;
        std::vector<char> reach;
        std::vector<std::pair<int64_t, int64_t>> P;
        for (int64_t t = 0; t < X.R + X.T; ++t) {
            hs_row_pairs(top.data(), ta.data(), tb.data(), ptr[t], ptr[t + 1], L, reach, P);
            for (size_t q = 0; q < P.size(); ++q) {
                if (q == 0 || P[q].first != P[q - 1].first) {
                    if (q) B.optr.push_back((int64_t)B.ovar.size());
                    B.srow.push_back(t); B.svar.push_back(P[q].first); B.woff.push_back(B.wnodes);
                    B.wnodes += ptr[t + 1] - ptr[t];
                }
                B.ovar.push_back(P[q].second);
                B.okey.push_back(P[q].second * n + P[q].first);
            }
            if (!P.empty()) B.optr.push_back((int64_t)B.ovar.size());
        }
        break;
    }
    case NlpFamily::OHM: {
        // ten occurrences per branch, listed by branch ascending and inside a branch in the order k_nlp_ohm_hess documents; occurrence q
        // of branch l is at hocc[q * nl + l]
        if (!e.has_hess) break;
        const int64_t nl = e.nlp_rows / 4;
        const std::vector<int64_t> ip = hs_download(e.d_ipar, 7 + 2 * nl);
        const int64_t va0 = ip[1], vm0 = ip[2];
        for (int64_t l = 0; l < nl; ++l) {
            const int64_t fb = ip[7 + l], tb = ip[7 + nl + l];
            const int64_t vf = vm0 + fb, vt = vm0 + tb, af = va0 + fb, at = va0 + tb;
            if (ip[0] != nl || std::min({vf, vt, af, at}) < 0 || std::max({vf, vt, af, at}) >= n)
                throw std::invalid_argument("asm_eval_hessian: the Ohm's-law block names a variable outside [0, n)");
            if (fb == tb) throw std::invalid_argument("asm_eval_hessian: branch " + std::to_string(l) + " of the Ohm's-law block joins a bus to itself");
            const int64_t pr[10][2] = {{vf, vf}, {vt, vt}, {vf, vt}, {vf, af}, {vf, at}, {vt, af}, {vt, at}, {af, af}, {at, at}, {af, at}};
            for (int64_t q = 0; q < 10; ++q) {
                B.okey.push_back(std::max(pr[q][0], pr[q][1]) * n + std::min(pr[q][0], pr[q][1]));
                B.oslot.push_back(q * nl + l);
            }
        }
        break;
    }
    case NlpFamily::DENSE:      // the n diagonal entries, written by k_nlp_dense_hess itself
        if (e.has_hess)
            for (int64_t j = 0; j < n; ++j) B.own.push_back(j * n + j);
        break;
    }
    return B;
}
// the block's values at (d_xt, lam) into vals, its nblk entries of the pattern: the occurrences into hs_H.hocc and their sums by the lists
// of L, or the entries in place.  (ipar / dpar read live: asm_eval_set_data and a scenario's table row take effect with nothing cached)
void nlp_hess_launch(const EvalState& e, hipStream_t s, const HsShared& L, const double* lam, double wobj, int64_t nblk, double* vals) {
    if (e.family == NlpFamily::DENSE && e.has_hess) asmb::launch(k_nlp_dense_hess, asmb::blocks(e.F.n), dim3(256), s, e.d_dpar, e.nlp_rows, e.F.n, lam, vals);
    if (e.family == NlpFamily::EXPR && e.hs_H.S > 0) asmb::launch(k_nlp_expr_hess, asmb::blocks(e.hs_H.S), dim3(256), s, e.X, e.hs_H, e.d_xt, lam, wobj);
    else if (e.family == NlpFamily::OHM && e.has_hess && L.nocc > 0) asmb::launch(k_nlp_ohm_hess, asmb::blocks(e.nlp_rows / 4), dim3(256), s, e.d_ipar, e.d_dpar, e.d_xt, lam, e.hs_H.hocc);
    else return;      // no occurrences to sum
    asmb::launch(k_nlp_expr_hess_gather, asmb::blocks(nblk), dim3(256), s, L.eptr, L.eocc, e.hs_H.hocc, nblk, vals);
}

// d_dgrad[c] = d(f - lam' g) / d dpar[c] at (d_xt, d_lam).  This and the launches below: for a block whose data_dep holds
void nlp_expr_data_gather(const EvalState& e, hipStream_t s, double* out) {      // out[c] = the sum of constant c's occurrences in d_cocc
    asmb::launch(k_nlp_expr_data_gather, asmb::blocks(e.n_dpar), dim3(256), s, e.d_cptr, e.d_cocc, e.n_dpar, out);
}
void nlp_data_grad_launch(const EvalState& e, hipStream_t s) {
    const int64_t R = e.nlp_rows, n = e.F.n;
    if (e.family == NlpFamily::EXPR) {
        asmb::launch(k_nlp_expr_const_adj, asmb::blocks(R + e.X.T), dim3(256), s, e.X, e.d_xt, e.d_lam, e.F.objective_scale, e.d_cocc);
        nlp_expr_data_gather(e, s, e.d_dgrad);
    } else if (e.family == NlpFamily::OHM) asmb::launch(k_nlp_ohm_data_grad, asmb::blocks(R / 4), dim3(256), s, e.d_ipar, e.d_xt, e.d_lam, e.d_dgrad);
    else asmb::launch(k_nlp_dense_data_grad, asmb::blocks(R * n), dim3(256), s, R, n, e.d_xt, e.d_lam, e.d_dgrad);
}

// The lists and the workspace of the cross derivatives, at the first call that needs them and again when the kernels' columns grow: 1
// for asm_eval_data_cross, KKM_CW from the first multi call on (the narrower buffers stay in the pool; a tape keeps its one column).
// Blocking copies: not inside a batch fiber.  Tape: the VAR nodes of every variable in (row, then term) order, node descending inside
// a row or term, and the sweep's node arrays.  Ohm's law: per variable its occurrences of k_nlp_ohm_cross, branch ascending and inside a
// branch in slot order (vm_f, vm_t, va_f, va_t; a branch from a bus to itself lists both occurrences of a variable, in that order)
void cx_prepare(EvalState& e, int64_t cap) {
    if (e.family == NlpFamily::EXPR) cap = 1;
    if (e.cx_cap >= cap) return;
    BufPool& M = e.mem;
    const int64_t n = e.F.n, R = e.nlp_rows, nl = R / 4, nd = e.n_dpar;
    if (!e.d_cx_vptr && e.family != NlpFamily::DENSE) {
        std::vector<std::pair<int64_t, int64_t>> occ;      // (variable, what its list names) in list order
        if (e.family == NlpFamily::EXPR) {
            const ExprTape& X = e.X;
            const std::vector<int64_t> ptr = hs_download(X.ptr, X.R + X.T + 1), ta = hs_download(X.a, X.L);
            const std::vector<int32_t> top = hs_download(X.op, X.L);
            for (int64_t t = 0; t < X.R + X.T; ++t)
                for (int64_t k = ptr[t + 1] - 1; k >= ptr[t]; --k)
                    if (top[k] == ASM_OP_VAR) occ.emplace_back(ta[k], k);
        } else {
            const std::vector<int64_t> ip = hs_download(e.d_ipar, 7 + 2 * nl);
            const int64_t base[4] = {ip[2], ip[2], ip[1], ip[1]};      // vm0, vm0, va0, va0
            for (int64_t l = 0; l < nl; ++l)
                for (int q = 0; q < 4; ++q) occ.emplace_back(base[q] + ip[7 + (q & 1) * nl + l], q * nl + l);
        }
        std::vector<int64_t> vptr(n + 1, 0), vnode(occ.size());
        for (const auto& o : occ) ++vptr[o.first + 1];
        for (int64_t j = 0; j < n; ++j) vptr[j + 1] += vptr[j];
        std::vector<int64_t> fill(vptr.begin(), vptr.end() - 1);
        for (const auto& o : occ) vnode[fill[o.first]++] = o.second;
        M.upload(e.d_cx_vptr, vptr.data(), n + 1); M.upload(e.d_cx_vnode, vnode.data(), (int64_t)vnode.size());
    }
    if (e.family == NlpFamily::EXPR) {      // (cx_cap was 0: once) the sweep's node arrays
        ExprCross& C = e.cx_C;
        const int64_t L = e.X.L;
        C.vptr = e.d_cx_vptr; C.vnode = e.d_cx_vnode;
        M.zeroed(C.val, L); M.zeroed(C.tval, L); M.zeroed(C.adj, L); M.zeroed(C.tadj, L); M.zeroed(C.vocc, L);
    }
    if (e.family == NlpFamily::OHM) M.zeroed(e.d_cx_occ, cap * 4 * nl);
    M.zeroed(e.d_cx_in, R + cap * nd); M.zeroed(e.d_cx_out, cap * (n + R));
    if (!e.h_cx) M.alloc(e.h_cx, 2 * (n + R) + nd, BufPool::PINNED);
    e.cx_cap = cap;
}
// the workspace of the transposed cross derivatives for `cap` columns: 1 for asm_eval_data_cross_t and asm_solution_adjoint, KKM_CW from
// the first multi call on (the narrower ones stay in the pool).  A tape borrows the node arrays of the cross sweep (cx_prepare)
void ct_prepare(EvalState& e, int64_t cap) {
    if (e.ct_cap >= cap) return;
    if (e.family == NlpFamily::EXPR) cx_prepare(e, 1);
    const int64_t n = e.F.n, R = e.nlp_rows, nd = e.n_dpar;
    BufPool& M = e.mem;
    M.zeroed(e.d_ct_in, R + cap * (n + R)); M.zeroed(e.d_ct_out, cap * nd);
    M.alloc(e.h_ct, n + R + cap * (n + R + nd), BufPool::PINNED);
    e.ct_cap = cap;
}
// ---- The launch sites of the KKT column family and of the SLP-EQP trial step (asm_kkt_kernels.hip.h, asm_eqp_kernels.hip.h): one function per
// launch of a kernel of the two headers.  Each computes its grid from the sizes it is given and the pitches held here, launches, and returns
// the workgroups (x times y) it asked for.  The drivers (KktFace, the KktOps back ends, kkt_stage_rhs, kkt_columns, nlp_cross_launch,
// asm_eqp_trial) and the test hook asm_test_kkt_stages go through these; nothing else launches a kernel of the two headers.
struct KktSites {
    hipStream_t s;
    int64_t ldn, ldT;      // pitch of the blocks over the variables / over the working rows
    unsigned gred;         // workgroups per column of the reductions over the variables: min(ceil(ldn / 256), KK_MAXWG)
    static constexpr int LA = 4, LAT = 8;      // lanes per working row / per variable of the sparse products ("KKT solve: the sparse form")
    KktSites(hipStream_t st, int64_t ldn_, int64_t ldT_) : s(st), ldn(ldn_), ldT(ldT_), gred((unsigned)std::min<int64_t>(asmb::blocks(ldn_).x, KK_MAXWG)) {}
    static unsigned wg(const dim3& g) { return g.x * g.y; }
    dim3 over_vars(int cols) const { return dim3(asmb::blocks(ldn).x, (unsigned)cols); }
    static dim3 over_rows(int64_t nWg, int cols) { return dim3(asmb::blocks(nWg).x, (unsigned)cols); }
    unsigned gather(const double* J, const int* wrow, const double* mask, int64_t nW, int64_t nWg, double* Aw) const {
        const dim3 g(asmb::blocks(ldn).x, (unsigned)nWg);
        asmb::launch(k_kkt_gather, g, dim3(256), s, J, ldn, wrow, mask, nW, Aw);
        return wg(g);
    }
    unsigned gather_t(const double* J, const int* wrow, const double* mask, int64_t nW, int64_t nWp, double* AT) const {
        const dim3 g((unsigned)((ldn + 63) / 64), (unsigned)((nWp + 63) / 64));
        asmb::launch(k_kktm_gather_t, g, dim3(256), s, J, ldn, wrow, mask, nW, nWp, AT, ldT);
        return wg(g);
    }
    // cols <= KKM_CW columns of pitch ldn: the template by the number of columns
    unsigned hess_product(const int64_t* pptr, const int64_t* pent, const int64_t* poth, const double* values, const double* v, int64_t n, int cols, double* out) const {
        const dim3 g = asmb::blocks(n);
        if (cols <= 8) asmb::launch(k_kktm_hess_product<8>, g, dim3(256), s, pptr, pent, poth, values, v, ldn, n, cols, out);
        else if (cols <= 16) asmb::launch(k_kktm_hess_product<16>, g, dim3(256), s, pptr, pent, poth, values, v, ldn, n, cols, out);
        else if (cols <= 32) asmb::launch(k_kktm_hess_product<32>, g, dim3(256), s, pptr, pent, poth, values, v, ldn, n, cols, out);
        else asmb::launch(k_kktm_hess_product<64>, g, dim3(256), s, pptr, pent, poth, values, v, ldn, n, cols, out);
        return wg(g);
    }
    unsigned axpby(double sa, const double* a, double sb, const double* b, const double* mask, const double* scal, double* out, int cols) const {
        const dim3 g = over_vars(cols);
        asmb::launch(k_kktm_axpby, g, dim3(256), s, sa, a, sb, b, mask, ldn, ldn, scal, out);
        return wg(g);
    }
    unsigned axpby_rows(double sa, const double* a, double sb, const double* b, int64_t nW, int64_t nWg, double* out, int cols) const {
        const dim3 g = over_rows(nWg, cols);
        asmb::launch(k_kktm_axpby, g, dim3(256), s, sa, a, sb, b, (const double*)nullptr, nW, ldT, (const double*)nullptr, out);
        return wg(g);
    }
    unsigned scatter(const double* y, const int* wrow, int64_t nW, int64_t nWg, double* out, int64_t ldo, int cols) const {
        const dim3 g = over_rows(nWg, cols);
        asmb::launch(k_kktm_scatter, g, dim3(256), s, y, ldT, wrow, nW, out, ldo);
        return wg(g);
    }
    unsigned cross_rhs(const double* cx, int64_t n, int64_t n_fn, const int* wrow, int64_t nW, double* ru, double* rww) const {
        const dim3 g = asmb::blocks(std::max(n, nW));
        asmb::launch(k_kktm_cross_rhs, g, dim3(256), s, cx, n, n_fn, wrow, nW, ru, rww);
        return wg(g);
    }
    unsigned cross_rhs_cols(const double* cx, int64_t ldc, int64_t n, int64_t n_fn, const int* wrow, int64_t nW, double* ru, double* rww, int cols) const {
        const dim3 g(asmb::blocks(std::max(n, nW)).x, (unsigned)cols);
        asmb::launch(k_kktm_cross_rhs_cols, g, dim3(256), s, cx, ldc, n, n_fn, wrow, nW, ru, ldn, rww, ldT);
        return wg(g);
    }
    unsigned bound_rhs(const int* rows, const double* delta, const int* wrow, int64_t nW, double* ru, double* rww, int cols) const {
        const dim3 g(asmb::blocks(std::max(ldn, ldT)).x, (unsigned)cols);
        asmb::launch(k_kktm_bound_rhs, g, dim3(256), s, rows, delta, wrow, nW, ru, ldn, rww, ldT);
        return wg(g);
    }
    unsigned var_unit(const int* vars, const double* mask, double* E, int cols) const {
        const dim3 g = over_vars(cols);
        asmb::launch(k_kktm_var_unit, g, dim3(256), s, vars, mask, E, ldn);
        return wg(g);
    }
    // J: the dense J of the solve, or nullptr in the sparse form (rww is then cleared for var_col)
    unsigned var_rhs(const int* vars, const double* delta, const double* mask, const double* hcol, int64_t n, const double* J, const int* wrow, int64_t nW, double* ru, double* rww,
                     int cols) const {
        const dim3 g(asmb::blocks(std::max(ldn, ldT)).x, (unsigned)cols);
        asmb::launch(k_kktm_var_rhs, g, dim3(256), s, vars, delta, mask, hcol, n, J, wrow, nW, ru, ldn, rww, ldT);
        return wg(g);
    }
    unsigned var_col(const int* vars, const double* delta, const double* mask, const int* cptr, const int* row, const int* pos, const double* val, const int* wpos, double* rww,
                     int cols) const {
        const dim3 g(1, (unsigned)cols);
        asmb::launch(k_kkts_var_col, g, dim3(256), s, vars, delta, mask, cptr, row, pos, val, wpos, rww, ldT);
        return wg(g);
    }
    unsigned var_dx(const int* vars, const double* delta, const double* mask, int cols, double* dx) const {
        const dim3 g = asmb::blocks(cols);
        asmb::launch(k_kktm_var_dx, g, dim3(256), s, vars, delta, mask, cols, dx, ldn);
        return wg(g);
    }
    unsigned gz_mask(const double* gz, const double* mask, int64_t n, double* gzb, double* cmask, int cols) const {
        const dim3 g = over_vars(cols);
        asmb::launch(k_kktm_gz_mask, g, dim3(256), s, gz, mask, n, ldn, gzb, cmask);
        return wg(g);
    }
    unsigned cg_p(const double* scal, const double* g_, double* p, int cols) const {
        const dim3 g = over_vars(cols);
        asmb::launch(k_kktm_cg_p, g, dim3(256), s, scal, g_, p, ldn, ldn);
        return wg(g);
    }
    unsigned normal(double* scal, const double* radius, double share, double* dx0, int cols) const {
        const dim3 g((unsigned)cols);
        asmb::launch(k_kktm_normal, g, dim3(1024), s, scal, radius, share, dx0, ldn, ldn);
        return wg(g);
    }
    unsigned cg_curv(bool trust, const KktMulti& R, const double* p, const double* hp_raw, const double* mask, const double* d, double* hp, int cols) const {
        const dim3 g(gred, (unsigned)cols);
        if (trust) asmb::launch(k_kktm_cg_curv<true>, g, dim3(256), s, R, p, hp_raw, mask, d, hp, ldn, ldn);
        else asmb::launch(k_kktm_cg_curv<false>, g, dim3(256), s, R, p, hp_raw, mask, d, hp, ldn, ldn);
        return wg(g);
    }
    unsigned cg_step(const double* scal, const double* p, const double* hp, double* d, double* r, int cols) const {
        const dim3 g = over_vars(cols);
        asmb::launch(k_kktm_cg_step, g, dim3(256), s, scal, p, hp, d, r, ldn, ldn);
        return wg(g);
    }
    unsigned cg_dir(const KktMulti& R, const double* r, int init, double rtol, unsigned pub, int trust, int cols) const {
        const dim3 g(gred, (unsigned)cols);
        asmb::launch(k_kktm_cg_dir, g, dim3(256), s, R, r, ldn, ldn, init, rtol, pub, trust);
        return wg(g);
    }
    unsigned finish(double* scal, const double* hdx, const double* ru, const double* jtl, const double* mask, int64_t n, const double* adx, const double* rww, int64_t nW,
                    double* dz, const double* dx, int cols) const {
        const dim3 g((unsigned)cols);
        asmb::launch(k_kktm_finish, g, dim3(1024), s, scal, hdx, ru, jtl, mask, n, ldn, adx, rww, nW, ldT, dz, dx);
        return wg(g);
    }
    unsigned kkts_vals(const double* dE, const int64_t* perm, const int64_t* ustart, int64_t nu, double* vals) const {
        const dim3 g((unsigned)std::min<int64_t>((nu + 255) / 256, 4096));
        asmb::launch(k_kkts_vals, g, dim3(256), s, dE, perm, ustart, nu, vals);
        return wg(g);
    }
    unsigned kkts_wpos(const int* wrow, int64_t nW, int64_t M, int* wpos) const {
        const dim3 g(1);
        asmb::launch(k_kkts_wpos, g, dim3(1024), s, wrow, nW, std::max<int64_t>(M, 1), wpos);
        return wg(g);
    }
    unsigned kkts_mul_a(const int* ptr, const int* col, const double* val, const int* wrow, const double* mask, const double* v, int64_t nW, int64_t nWg, double* t, int cols) const {
        const dim3 g(asmb::blocks(nWg * LA).x, (unsigned)cols);
        asmb::launch(k_kkts_mul_a<LA>, g, dim3(256), s, ptr, col, val, wrow, mask, v, ldn, nW, t, ldT);
        return wg(g);
    }
    unsigned kkts_mul_at(const int* cptr, const int* row, const int* pos, const double* val, const int* wpos, const double* mask, const double* y, int64_t n, double* v,
                         int cols) const {
        const dim3 g(asmb::blocks(ldn * LAT).x, (unsigned)cols);
        asmb::launch(k_kkts_mul_at<LAT>, g, dim3(256), s, cptr, row, pos, val, wpos, mask, y, ldT, n, ldn, v, ldn);
        return wg(g);
    }
    // (the two kernels of the trial step use neither pitch)
    unsigned eqp_face(const EqpFace& P, const KktRed& R, int* rows, int* bnd, int* side, double* rw, int* counts) const {
        const dim3 g((unsigned)std::min<int64_t>(asmb::blocks(std::max(P.n, P.m)).x, KK_MAXWG));
        asmb::launch(k_eqp_face, g, dim3(256), s, P, R, rows, bnd, side, rw, counts);
        return wg(g);
    }
    unsigned eqp_trial(const double* dx, const double* x, const double* x_L, const double* x_U, int64_t n, const KktRed& R, double* d, double* out) const {
        const dim3 g((unsigned)std::min<int64_t>(asmb::blocks(n).x, KK_MAXWG));
        asmb::launch(k_eqp_trial, g, dim3(256), s, dx, x, x_L, x_U, n, R, d, out);
        return wg(g);
    }
};
// where kkt_stage_rhs wants the cross derivatives of a chunk: column c as the right-hand sides b_ru + c ldn and, on the working rows, rww + c ldT
struct CxRhs { const int* wrow; int64_t nW; double* b_ru; int64_t ldn; double* rww; int64_t ldT; };
// Cross derivatives (u, w) of `cols` <= cx_cap directions at d_xt, with the block's multipliers in d_cx_in: u = d/dc (grad_x L) . dc,
// w = (dg/dc) . dc, L = f - lambda' g.  hd: the directions in pinned memory (pitch n_dpar), uploaded here; null: one direction, already
// behind the multipliers.  to: every column on into the right-hand sides of a KKT solve; null: it stays in d_cx_out = [u (n) | w (R)].
// The kernels take the columns at once (grid.y = column): one upload, one launch and a gather (Ohm's law) or two launches (dense).  The
// tape has one column: per direction its upload, its launch pair and its hand-over, no synchronisation between them.  A column's answer
// depends on its own direction only
void nlp_cross_launch(const EvalState& e, hipStream_t s, int cols, const double* hd, const CxRhs* to) {
    const int64_t n = e.F.n, R = e.nlp_rows, r0 = e.F.n_rows, nd = e.n_dpar, ldo = n + R, nl = R / 4;
    const double* lam = e.d_cx_in;
    double* dc = e.d_cx_in + R;
    const unsigned nc = (unsigned)cols;
    if (e.family == NlpFamily::EXPR) {
        for (int c = 0; c < cols; ++c) {
            if (hd) HIPCHK(asmb::copy_async(dc, hd + (int64_t)c * nd, nd * sizeof(double), hipMemcpyHostToDevice, s));
            asmb::launch(k_nlp_expr_cross, asmb::blocks(R + e.X.T), dim3(256), s, e.X, e.cx_C, e.d_xt, dc, lam, e.F.objective_scale, e.d_cx_out + n);
            asmb::launch(k_nlp_expr_cross_gather, asmb::blocks(n), dim3(256), s, e.cx_C, n, e.d_cx_out);
            if (to) KktSites(s, to->ldn, to->ldT).cross_rhs(e.d_cx_out, n, r0, to->wrow, to->nW, to->b_ru + (int64_t)c * to->ldn, to->rww + (int64_t)c * to->ldT);
        }
        return;
    }
    if (hd) HIPCHK(asmb::copy_async(dc, hd, (int64_t)cols * nd * sizeof(double), hipMemcpyHostToDevice, s));
    if (e.family == NlpFamily::OHM) {
        asmb::launch(k_nlp_ohm_cross, dim3(asmb::blocks(nl).x, nc), dim3(256), s, e.d_ipar, e.d_xt, dc, nd, lam, e.d_cx_occ, e.d_cx_out, n, ldo);
        asmb::launch(k_nlp_block_cross_gather, dim3(asmb::blocks(n).x, nc), dim3(256), s, e.d_cx_vptr, e.d_cx_vnode, e.d_cx_occ, 4 * nl, n, e.d_cx_out, ldo);
    } else {
        asmb::launch(k_nlp_dense_cross_w, dim3(asmb::blocks(R, 4).x, nc), dim3(256), s, dc, nd, R, n, e.d_xt, e.d_cx_out, ldo);
        asmb::launch(k_nlp_dense_cross_u, dim3(asmb::blocks(n).x, nc), dim3(256), s, dc, nd, R, n, e.d_xt, lam, e.d_cx_out, ldo);
    }
    if (to) KktSites(s, to->ldn, to->ldT).cross_rhs_cols(e.d_cx_out, ldo, n, r0, to->wrow, to->nW, to->b_ru, to->rww, cols);
}
// Transposed cross derivatives of `cols` <= ct_cap weight columns [vx (n) | vl (R)] at d_ct_in + R, at d_xt and with the block's
// multipliers in d_ct_in: column c of d_ct_out (pitch n_dpar).  The kernels take the columns at once (grid.y = column), the tape one
// launch pair per column
void nlp_cross_t_launch(const EvalState& e, hipStream_t s, int cols) {
    const int64_t n = e.F.n, R = e.nlp_rows, nd = e.n_dpar, ldv = n + R;
    const double *lam = e.d_ct_in, *dv = e.d_ct_in + R;
    if (e.family == NlpFamily::OHM) asmb::launch(k_nlp_ohm_cross_t, dim3(asmb::blocks(R / 4).x, (unsigned)cols), dim3(256), s, e.d_ipar, e.d_xt, lam, dv, ldv, n, e.d_ct_out, nd);
    if (e.family == NlpFamily::DENSE) asmb::launch(k_nlp_dense_cross_t, dim3(asmb::blocks(R * n).x, (unsigned)cols), dim3(256), s, R, n, e.d_xt, lam, dv, ldv, e.d_ct_out, nd);
    for (int c = 0; e.family == NlpFamily::EXPR && c < cols; ++c) {
        const double* v = dv + (int64_t)c * ldv;
        asmb::launch(k_nlp_expr_cross_t, asmb::blocks(R + e.X.T), dim3(256), s, e.X, e.cx_C, e.d_xt, v, lam, v + n, e.F.objective_scale, e.d_cocc);
        nlp_expr_data_gather(e, s, e.d_ct_out + (int64_t)c * nd);
    }
}

// Pitches and lengths of the buffers of the null-space form that do not depend on the null-space dimension, for an LP with nE hard equality
// rows and nI inequality rows (do_setup allocates by them; Solver::nsv places the work vectors).  theta~ = [n-part (ldn) | I-part (nIp)], a row
// of Gt = [Zt | GI'] has the same shape (pitch ldg).  Work vectors: five n-sized, three M-sized, two E-sized, then six more of n entries
// (10 .. 13 hold k <= n entries, 14 = e, 15).  kcap: rows reserved for a basis of k rows (Solver::ns_reserve).
struct NsLayout {
    int64_t ldn, Mp, nE, nI, nEp, nIp, ldg;
    NsLayout(int64_t ln, int64_t lm, int64_t ne, int64_t ni)
        : ldn(ln), Mp(lm), nE(ne), nI(ni), nEp(round_up(ne, 32)), nIp(round_up(std::max<int64_t>(ni, 1), 32)), ldg(ln + nIp) {}
    int64_t th_len() const { return ldg; }
    int64_t nsv_len() const { return 11 * ldn + 3 * Mp + 2 * nEp; }
    int64_t nsv_off(int which) const {
        if (which < 5) return (int64_t)which * ldn;
        if (which < 8) return 5 * ldn + (int64_t)(which - 5) * Mp;
        if (which < 10) return 5 * ldn + 3 * Mp + (int64_t)(which - 8) * nEp;
        return 5 * ldn + 3 * Mp + 2 * nEp + (int64_t)(which - 10) * ldn;
    }
    static int kcap(int k) { return (int)round_up(k + k / 4 + 64, 64); }
};

// The buffers of the null-space form sized by the null-space dimension, in a pool of their own: made by the first LP that uses the form and
// re-made when the dimension outgrows them (Solver::ns_reserve).  NsForm holds a pointer that is null until then.
struct NsK {
    int cap = 0, ccap = 0, Zk = 0;  // rows reserved (NsLayout::kcap); most constraints of a reduced active-set solve; rows of the previous LP's basis still in G
    double *R = nullptr, *X = nullptr, *G = nullptr, *N0 = nullptr, *Np = nullptr, *ZT = nullptr, *q = nullptr;   // right-hand-side blocks, Gt = [Zt | GI'], N, its split-K slices, Zt'
    int *J = nullptr, *qi = nullptr;
    FacBuf fN, fC;                  // factors of the k x k reduced matrix (per iteration) and of the Gram matrix of the active constraints in reduced coordinates
    // The ONLY place that lays out the work areas qi, q of the reduced active-set solve: sel | bpos | rpos | cnt  and  Csel | d, lam, v, w, u |
    // pbar | tbar | u0 | qh | 64 spare (u0, qh adjacent: one fill clears both).  Yields the vectors (null while qi, q are) and both lengths.
    struct Work { NsEq Q; int64_t ilen = 0, dlen = 0; };
    Work work(const NsLayout& L) const {
        Work W;
        auto I = [&](int64_t len) { int* p = qi ? qi + W.ilen : nullptr; W.ilen += len; return p; };
        auto D = [&](int64_t len) { double* p = q ? q + W.dlen : nullptr; W.dlen += len; return p; };
        NsEq& Q = W.Q; Q.ldc = fN.ld;
        Q.sel = I(ccap); Q.bpos = I(L.ldn); Q.rpos = I(L.nIp); Q.cnt = I(16);
        Q.Csel = D(ccap * Q.ldc); Q.d = D(ccap); Q.lam = D(ccap); Q.v = D(ccap); Q.w = D(ccap); Q.u = D(ccap);
        Q.pbar = D(L.ldn); Q.tbar = D(L.Mp); Q.u0 = D(Q.ldc); Q.qh = D(Q.ldc + 64);
        return W;
    }
    BufPool mem;                    // declared last, as in EvalState
};
// The null-space form of the interior-point Newton system (asm_ns_kernels.hip.h; oracle: class NullSpace): what do_setup makes for an LP
// skeleton that qualifies (sparse pattern, enough hard equality rows, small null space).  The handle's pointer is null when it does not.
struct NsForm {
    const NsLayout L;
    std::vector<int> eidx_h;        // host copy of Eidx: the equality rows in their reverse Cuthill-McKee order
    int *Eidx = nullptr, *Epos = nullptr, *Iidx = nullptr, *Ipos = nullptr, *cnt = nullptr, *S0pairs = nullptr;
    int64_t npairs = 0;             // structural non-zeros of the lower triangle of S0, listed in S0pairs (banded S0 only)
    FacBuf f0;                      // factor of S0 = A_EF A_EF' (per LP)
    double *Lt = nullptr, *th = nullptr, *Fm = nullptr, *v = nullptr, *Yt = nullptr;     // Yt: made by the first cold basis selection (Solver::ns_setup)
    std::unique_ptr<NsK> k;
    BufPool mem;                    // declared last, as in EvalState
    explicit NsForm(const NsLayout& l) : L(l) {}
};

// environment knobs of a handle, read once in asm_create (README.md lists them)
struct HandleKnobs {
    int timing = 1;                 // ASM_HIP_TIMING: 0, 1 or 2, the initial asm_handle::timing
    bool verbose = false;           // ASM_HIP_VERBOSE=1: solver diagnostics on stderr
    bool spin_read = true;          // ASM_HIP_SPIN=0: asmb::copy_async + asmb::sync instead (14.5 us per read-back instead of 6.7 us)
    int panel_wgs = 0;              // ASM_PANEL_WGS: grid bound of the panel kernels on the whole device (0: by the device's CU count)
    bool ns_defer = true;           // ASM_NS_DEFER=0: the step of a null-space iteration is taken on the host
    bool ns_side = true;            // ASM_NS_SIDE=0: the factor-independent head of a null-space iteration stays on the handle's stream (Solver::ns_iter_setup)
    int ns_s0side = 2;              // ASM_NS_S0SIDE: what of the null-space set-up runs on the side stream beside the factorisation of a banded S0 (Solver::ns_factor_S0) -
                                    // 0 nothing; 1 the previous basis' right-hand sides, the wide-block inverses and the transposed copy; 2 the forward substitution as well
    bool ns_fold = true;            // ASM_NS_FOLD=0: k_ns_add and k_ns_dp of a null-space Newton solve are launches of their own (k above ASM_SMALL_USE)
    double ns_rerr = NS_RERR;       // ASM_NS_RERR: accuracy bound of the reduced solves of a null-space iteration (test knob - a tiny bound
                                    // sends every LP through the fall-back to the row form)
};
HandleKnobs read_knobs() {
    HandleKnobs k;
    if (const char* v = std::getenv("ASM_HIP_TIMING")) if (v[0] >= '0' && v[0] <= '2') k.timing = v[0] - '0';
    if (const char* v = std::getenv("ASM_HIP_VERBOSE")) k.verbose = v[0] == '1';
    if (const char* v = std::getenv("ASM_HIP_SPIN")) k.spin_read = v[0] != '0';
    if (const char* v = std::getenv("ASM_PANEL_WGS")) k.panel_wgs = std::max(1, std::atoi(v));
    if (const char* v = std::getenv("ASM_NS_DEFER")) k.ns_defer = v[0] != '0';
    if (const char* v = std::getenv("ASM_NS_SIDE")) k.ns_side = v[0] != '0';
    if (const char* v = std::getenv("ASM_NS_S0SIDE")) if (v[0] >= '0' && v[0] <= '2') k.ns_s0side = v[0] - '0';
    if (const char* v = std::getenv("ASM_NS_FOLD")) k.ns_fold = v[0] != '0';
    if (const char* v = std::getenv("ASM_NS_RERR")) k.ns_rerr = std::atof(v);
    return k;
}

// The LP skeleton: everything asm_sublp_setup makes (do_setup) and everything that is valid only for it - the uploaded inputs, the retained
// working sets, the test hooks' factor - in one pool and with one lifetime: until the next asm_sublp_setup.  The handle holds a pointer that is
// null while there is no skeleton (sk_of): no ready flag, no list of fields to reset; every field starts from its initialiser here.
struct Skeleton {
    std::unique_ptr<NsForm> nsf;    // the null-space form with its own pools (null: the skeleton does not qualify)
    // ---- problem (subproblem.jl:51-215) ----
    int64_t n = 0, m = 0, nnz = 0, nadj = 0, M = 0, Mp = 0, ldn = 0, ns = 0;
    vec c_lb, c_ub, v_lb, v_ub;
    std::vector<int> kind;          // 0 EQ, 2 range, +1 lower only, -1 upper only
    std::vector<int64_t> adj;       // rows with two distinct finite bounds
    std::vector<int> rtype;         // LP row types (M)
    std::vector<int> srow;          // slack -> LP row
    vec scoef;                      // slack coefficient (+1 / -1)
    std::vector<int64_t> sown;      // slack -> original row (for p_slack)
    std::vector<int> nslack;        // slacks per original row (1 or 2)

    // ---- assembly plan ----
    int64_t nu = 0;
    bool dense_fast = false;
    int64_t *d_perm = nullptr, *d_ustart = nullptr, *d_uoff = nullptr, *d_adjoff = nullptr;

    // ---- device buffers ----
    double *d_dE = nullptr, *d_J = nullptr, *d_Ah = nullptr;
    double *d_c = nullptr, *d_rho = nullptr, *d_theta = nullptr, *d_diag = nullptr, *d_diag0 = nullptr;
    double *d_vecN = nullptr, *d_vecM = nullptr, *d_vecM2 = nullptr, *d_partial = nullptr;
    double *d_wpart = nullptr, *d_wt = nullptr;
    // factor of the Newton systems of the row and column forms and of the active-set Gram matrices (Mp x Mp); its band is set by the build
    // that fills it (0 = dense)
    FacBuf main_fac;
    // column form: transposed copy of Ah (n x ldT), its chunk flags, work vectors
    bool col_capable = false, ahT_valid = false, nzT_valid = false;
    int64_t ldT = 0;
    double nzT_fraction = 1.0;
    double *d_AhT = nullptr, *d_cdinv = nullptr, *d_cth = nullptr, *d_cu = nullptr, *d_ct = nullptr, *d_cv = nullptr, *d_cw = nullptr;
    unsigned char* d_nzT = nullptr;
    // reduced row form: dropped-row index list, its diagonal, gathered work vectors, s_ii
    int* d_idxI = nullptr;
    double *d_rdI = nullptr, *d_rce = nullptr, *d_rze = nullptr, *d_sdiag = nullptr;
    unsigned char* d_nz = nullptr;  // (row tile, k-chunk) non-zero flags of Ah; second half: flags of a gathered row set
    int64_t nz_half = 0;
    // sparse copy of the fixed Jacobian pattern for the matrix-vector products (sparse patterns only)
    bool sp_ok = false, spv_Ah_valid = false, spv_J_valid = false;
    int64_t sp_nnz = 0;
    int *d_sp_ptr = nullptr, *d_sp_col = nullptr, *d_sc_ptr = nullptr, *d_sc_row = nullptr, *d_sc_pos = nullptr;
    int64_t* d_sp_off = nullptr;
    double *d_spv_Ah = nullptr, *d_spv_J = nullptr;
    std::vector<int> sp_ptr_h, sp_col_h;      // host copy of the CSR pattern (sp_ok): the row orders made after the set-up read it (KktFace)
    bool nz_valid = false;
    int nz_T = 0, nz_pitch = 0;
    double nz_fraction = 1.0;       // executed share of the (tile pair, k-chunk) products of the Schur build
    double nz_frac_cache[2] = {-1.0, -1.0};   // ... cached: all rows / the equality rows (the pattern is fixed)
    // all M rows in reverse Cuthill-McKee order (sparse patterns whose bandwidth is below M / 2): the Gram matrices of row subsets taken in
    // that order are banded with half-bandwidth <= row_band
    int row_band = 0;
    int *d_rowperm = nullptr, *d_rowpos = nullptr, *d_rowpairs = nullptr, *d_cpos = nullptr;      // position -> row, row -> position, structural pairs (row_i, row_j), pos_i >= pos_j
    int64_t n_rowpairs = 0;
    std::vector<int> row_perm_h;    // host copy: rows by position
    int col_band = 0;               // the same for the n columns (column form of the restoration-phase Newton system)
    int *d_colperm = nullptr, *d_colpos = nullptr, *d_colpairs = nullptr;
    int64_t n_colpairs = 0;
    double* d_AhTg = nullptr;       // transposed copy of a dense Ah for the products Ah'y (ldn rows of pitch Mp; made once per LP)
    bool ahTg_valid = false;
    double* d_redpart = nullptr;    // partial results / arrival counter of the multi-workgroup interior-point reductions
    unsigned* d_redcnt = nullptr;
    FacBuf test_fac;                // the kernel hooks' own factor buffer (asm_test_set_factor layout 1), made by test_load_S
    double* d_ipm_snap = nullptr;   // best-iterate safeguard: copy of the iterate at the end of the best interior-point stage so far
    double* d_ipm = nullptr;        // arena of the device-resident interior-point state
    int* d_ipm_i = nullptr;
    double* d_as = nullptr;         // arena of the device-resident active-set machinery (asm_as_kernels.hip.h)
    int* d_as_i = nullptr;
    int* h_ascnt = nullptr;         // pinned read-back of its counters / scalars
    double* h_asscal = nullptr;
    // anchored primal face method (face_primal_anchored), a null-space active-set method of its own: made for every skeleton, in `mem` - no part of NsForm
    double *d_Zbuf = nullptr, *d_nsu = nullptr, *d_nsdots = nullptr, *h_nsdots = nullptr;
    std::vector<int64_t> j_row_h, j_col_h;   // j_str as asm_sublp_setup received it (the expression block's pattern is checked against it)
    bool J_valid = false;                              // the dense J in HBM matches the dE in HBM
    int64_t nsp = 0;
    double* h_scal = nullptr;       // pinned scalar read-back; host-mapped: the reduction kernels store the block there themselves (scal_publish)
    double* d_hscal = nullptr;      // its device address
    unsigned* h_seq = nullptr;      // sequence word the host spins on (host-mapped), d_hseq its device address
    unsigned* d_hseq = nullptr;
    unsigned scal_seq = 0;          // last sequence number handed to a publishing kernel
    int* d_idx = nullptr;
    double* h_pin = nullptr;        // pinned staging (max(ldn, Mp) doubles) x 2
    double* d_dl = nullptr;         // the answer of an LP packed on the device (k_as_pack) and its pinned host image: one device-to-host copy per LP instead of eight
    double* h_dl = nullptr;
    double* h_up = nullptr;         // pinned staging of the LP vectors an LP uploads (3 ldn + Mp + 3 nsp doubles, zero beyond the vectors' lengths)
    int64_t pin_len = 0;

    // ---- host copies of the evaluation results (slp.jl:8-21) ----
    bool inputs_ready = false;
    bool inputs_from_eval = false;  // the inputs came from asm_eval_functions: the evaluator's x, E and gradient in HBM are those of x_k
    vec df, E, x_k;
    double f = 0.0;

    // ---- warm start (retained active set per phase; GLPK keeps its basis, slp.jl:38-40) ----
    ActiveSet warm[2];
    SolveHint hint[2] = {SolveHint(false), SolveHint(true)};
    ActiveSet last;
    unsigned *d_pflags = nullptr, *d_ptmo = nullptr;      // flags and time-out word of the Cholesky panel kernels
    BufPool mem;                    // declared last, as in EvalState
};

// The limited-memory Hessian of a handle (include/asm_hip.h, "Limited-memory Hessian").  The type and the memory survive a set-up; the
// store is made at the first use after asm_sublp_setup (lm_store) and goes with the skeleton or the evaluator (drop): no ready flag.
static_assert(LM_PMAX == ASM_LM_MAX && 2 * LM_PMAX <= 64, "the store's most pairs are the header's");
struct LmState {
    int type = ASM_HESS_EXACT, memory = 10;
    bool pending = false;           // between asm_lm_begin and asm_lm_end
    LmStore S{};                    // R == nullptr: not made
    double *xs = nullptr, *gs = nullptr, *s = nullptr, *y = nullptr, *jtl = nullptr;      // the saved point and gradient, the new pair, J' lambda (ldn)
    double *part_dot = nullptr, *part = nullptr;      // partial sums of the pair's three dots (3 per workgroup) and of T = V [S; Y]' (KKM_CW columns)
    double *vb = nullptr, *ob = nullptr;              // asm_lm_product: a chunk of V and of OUT (made by its first call)
    int ndot = 0, nwg = 0;          // workgroups of k_lm_pair_dots (`per` variables each) and of k_lm_psi_v
    int64_t per = 0, bytes = 0;
    BufPool mem;                    // declared last, as in EvalState
    void drop() { mem.release(); S = LmStore{}; pending = false; bytes = 0; }
};

}  // namespace

struct asm_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // look-ahead stream of the Cholesky (next panel's block chain runs beside the trailing update)
    std::vector<hipEvent_t> la_events;
    // side stream of the null-space iterations (default priority): the launches that do not depend on the k x k factor run beside its build and
    // factorisation (Solver::ns_iter_setup); fork / join events, made with the first fork
    hipStream_t stream_ns = nullptr;
    hipEvent_t ns_fork = nullptr, ns_join = nullptr;
    // events of the set-up's side sequence beside the factorisation of S0 (Solver::ns_factor_S0): fork, join, then one per wide block; made
    // once per handle as the list grows, like la_events
    std::vector<hipEvent_t> s0_events;
    std::string err;
    // owners of the device / pinned buffers, one per lifetime: the LP skeleton with the null-space form inside it (until the next set-up; null:
    // no set-up yet, or the last one failed), the device evaluator (until the next asm_eval_setup or set-up; null: none).  What follows
    // them survives a set-up.
    std::unique_ptr<Skeleton> sk;
    std::unique_ptr<EvalState> ev;
    LmState lm;
    int test_band = 0;              // band of the matrices the kernel hooks load (test hook asm_test_set_band; 0 = dense)
    // test hook asm_test_set_factor: where the kernel hooks factor (0: the main factor, 1: a factor buffer of their own made by
    // ns_alloc_factor with this band hint) and the guard settings they factor with (k_diag_prepare mode / rel / absv, chol threshold)
    int test_layout = 0, test_band_hint = 0, test_mode = 0;
    double test_rel = 0.0, test_abs = 0.0, test_thr = 1e-14;
    int64_t stats_pcg = 0;          // conjugate-gradient steps since creation (verbose diagnostics)
    asm_solve_stats stats;

    // ---- kernel timing ----
    asm_kernel_stats kstats;
    std::vector<TimedRegion> regions;
    std::vector<hipEvent_t> event_pool;
    bool batch_slot = false;        // slot of an asm_batch: the stream belongs to the batch, no look-ahead stream, no event timing
    int panel_wgs = 240;            // grid bound of the Cholesky panel kernels: every workgroup must be able to become resident (a batch slot: its group's share)
    int panel_wgs_dev = 240;        // the bound of the whole device (ASM_PANEL_WGS) the shares of a batch's groups are taken from
    int num_cus = 256;              // compute units of the device (hipDeviceProp_t::multiProcessorCount)
    bool test_no_polish = false;    // test hook: the active-set attempts of an LP all fail (asm_test_no_polish)
    unsigned panel_epoch = 0;
    int timing = 1;                 // HIP-event timing: 0 off, 1 the dominant kernel only (every k_syrk launch), 2 every kernel family
    HandleKnobs knobs;
};

namespace {

// after host -> device copies whose source must stay untouched until they have run: in a scenario batch the payload was copied when the
// operation was recorded, nothing to wait for
inline void h2d_done(asm_handle* h) {
    if (!asmb::in_fiber()) HIPCHK(asmb::sync(h->stream));
}
// the handle's evaluator for entry `who`
EvalState& ev_of(const asm_handle* h, const char* who) {
    if (!h->ev) throw std::logic_error(std::string(who) + ": asm_eval_setup first");
    return *h->ev;
}
// the handle's LP skeleton, or std::logic_error(what) while there is none.  An evaluator implies a skeleton: do_eval_setup needs one, do_setup drops both
Skeleton& sk_of(const asm_handle* h, const char* what) {
    if (!h->sk) throw std::logic_error(what);
    return *h->sk;
}
// the reductions' copy of the handle's bounds into the block of L
void ev_write_bounds(const asm_handle* h, const EvLayout& L) {
    HIPCHK(asmb::copy(L.g_L(), h->sk->c_lb.data(), h->sk->m * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(asmb::copy(L.g_U(), h->sk->c_ub.data(), h->sk->m * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(asmb::copy(L.x_L(), h->sk->v_lb.data(), h->sk->n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(asmb::copy(L.x_U(), h->sk->v_ub.data(), h->sk->n * sizeof(double), hipMemcpyHostToDevice));
}

// buffers of one Cholesky factor of order <= N (pitch = N rounded up to 32) with the block inverses of the substitution kernels, from `pool`
void ns_alloc_factor(asm_handle* h, BufPool& pool, FacBuf& f, int64_t N, int band_hint = 0) {
    f.ld = round_up(std::max<int64_t>(N, 1), 32);
    f.wb = (f.ld <= 1024 || f.ld > 1536) ? 1024 : 512;      // one wide block (= the whole inverse) when the factor fits into it
    // a narrow band: the explicit inverse of a wide diagonal block is dense whatever the band, its cost grows with the square of the block
    // width - half the width is a quarter of the inverse (case300-sized S0, band 268 of 2 100: 16 % of a scenario batch's kernel time at 1024)
    if (band_hint > 0 && band_hint <= 512 && f.ld > 1024) f.wb = 512;
    pool.zeroed(f.S, f.ld * f.ld, h->stream);
    pool.zeroed(f.Linv, (f.ld / ASM_NB + 1) * ASM_NB * ASM_NB, h->stream);
    pool.zeroed(f.Binv, (f.ld / f.wb + 1) * (int64_t)f.wb * f.wb, h->stream);
    pool.zeroed(f.BinvT, (f.ld / f.wb + 1) * (int64_t)f.wb * f.wb, h->stream);
}

// =====================================================================================================
// device helpers
// =====================================================================================================
// The Cholesky / substitution launches work on the factor passed to them: matrix (lower triangle, pitch ld), inverses of its 64-wide diagonal
// blocks, explicit inverses of its wide diagonal blocks and their transposes (FacBuf).
struct Dev {
    asm_handle* h;
    explicit Dev(asm_handle* hh) : h(hh) {}
    Skeleton& sk() const { return *h->sk; }         // the entry has checked that there is one (sk_of); kernel statistics and timing need none
    // first row that the columns [.., c1) of a banded matrix / factor cannot reach (the order Ms when the matrix is dense)
    static int rowlim(const FacBuf& f, int Ms, int c1) { return f.band > 0 ? (int)std::min<int64_t>(Ms, round_up((int64_t)c1 + f.band, 64)) : Ms; }

    hipEvent_t get_event() {
        if (!h->event_pool.empty()) {
            hipEvent_t e = h->event_pool.back();
            h->event_pool.pop_back();
            return e;
        }
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        return e;
    }
    int begin(int kind, double flops, double bytes, hipStream_t on = nullptr) {
        h->kstats.flops[kind] += flops;
        h->kstats.bytes[kind] += bytes;
        h->kstats.calls[kind] += 1;
        if (h->timing < 2 && !(h->timing == 1 && (kind == ASM_K_SYRK_KERNEL || kind == ASM_K_PANEL_KERNEL))) return -1;
        TimedRegion r;
        r.a = get_event();
        r.b = get_event();
        r.kind = kind;
        r.stream = on ? on : h->stream;
        HIPCHK(hipEventRecord(r.a, r.stream));
        h->regions.push_back(r);
        return (int)h->regions.size() - 1;
    }
    void end(int id) {
        if (id < 0) return;
        HIPCHK(hipEventRecord(h->regions[id].b, h->regions[id].stream));
    }
    void resolve_timing() {
        if (h->regions.empty()) return;
        HIPCHK(asmb::sync(h->stream));
        HIPCHK(asmb::sync(h->stream2));
        // (stream_ns is not synchronised: no timed region is ever on it.  Its sequences - ns_iter_setup, ns_factor_S0 - are off under family
        // timing (timing == 2) and the kinds timed at level 1, ASM_K_SYRK_KERNEL and ASM_K_PANEL_KERNEL, are not launched there; a timed
        // launch on the side stream would need a synchronisation here before its events are read)
        for (auto& r : h->regions) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, r.a, r.b));
            h->kstats.ms[r.kind] += ms;
            h->event_pool.push_back(r.a);
            h->event_pool.push_back(r.b);
        }
        h->regions.clear();
    }

    void h2d(double* dst, const double* src, int64_t cnt, int64_t padded) {
        double* st = sk().h_pin;
        std::memcpy(st, src, cnt * sizeof(double));
        for (int64_t i = cnt; i < padded; ++i) st[i] = 0.0;
        HIPCHK(asmb::copy_async(dst, st, padded * sizeof(double), hipMemcpyHostToDevice, h->stream));
        h2d_done(h);   // staging buffer is reused by the next call
    }
    void d2h(double* dst, const double* src, int64_t cnt) {
        double* st = sk().h_pin + sk().pin_len;
        HIPCHK(asmb::copy_async(st, src, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(asmb::sync(h->stream));
        std::memcpy(dst, st, cnt * sizeof(double));
    }

    // out[M] = A x   (A = Ah or J, M rows)
    // gathered pattern values of A (d_Ah or d_J) for the sparse products, nullptr when the pattern is dense
    const double* sparse_vals(const double* A) {
        if (!sk().sp_ok) return nullptr;
        double* v = nullptr;
        bool* valid = nullptr;
        if (A == sk().d_Ah) { v = sk().d_spv_Ah; valid = &sk().spv_Ah_valid; }
        else if (A == sk().d_J) { v = sk().d_spv_J; valid = &sk().spv_J_valid; }
        else return nullptr;
        if (!*valid) {
            asmb::launch(k_sp_gather, asmb::blocks(sk().sp_nnz), dim3(256), h->stream, A, sk().d_sp_off, v, sk().sp_nnz);
            *valid = true;
        }
        return v;
    }
    void launch_gemv_n(const double* A, const double* x, double* out) {
        if (sk().M == 0) return;                         // LP without rows
        if (const double* v = sparse_vals(A)) {
            int id = begin(ASM_K_GEMV, 2.0 * sk().sp_nnz, 20.0 * sk().sp_nnz + 12.0 * sk().M);
            asmb::launch(k_spmv_n, asmb::blocks(sk().M), dim3(256), h->stream, sk().d_sp_ptr, sk().d_sp_col, v, x, out, sk().M);
            end(id);
            return;
        }
        int id = begin(ASM_K_GEMV, 2.0 * sk().M * sk().n, 8.0 * sk().M * sk().ldn);
        asmb::launch(k_gemv_n, asmb::blocks(sk().M, 4), dim3(256), h->stream, A, sk().ldn, x, out, sk().M, sk().ldn);
        end(id);
    }
    // the row chunks of the two-stage column reductions over the M rows (k_gemv_t_stage1/2, k_col_relmax_stage1/2): R chunks of `chunk` rows,
    // the last one shorter
    void col_chunks(int64_t& R, int64_t& chunk) const {
        R = std::min<int64_t>((sk().M + 31) / 32, ASM_TMAXCHUNKS);
        chunk = (sk().M + R - 1) / R;
        R = (sk().M + chunk - 1) / chunk;
    }
    // out[ldn] = A'y; returns the route taken: GemvT_Csc the CSC copy of a sparse pattern, GemvT_Copy the transposed copy of a dense Ah,
    // GemvT_TwoStage the two-stage column reduction, GemvT_None an LP without rows
    enum { GemvT_None = -1, GemvT_Csc = 0, GemvT_Copy = 1, GemvT_TwoStage = 2 };
    int launch_gemv_t(const double* A, const double* y, double* out) {
        if (sk().M == 0) {                               // LP without rows: A'y = 0
            HIPCHK(asmb::fill_async(out, 0, sk().ldn * sizeof(double), h->stream));
            return GemvT_None;
        }
        if (const double* v = sparse_vals(A)) {
            int id = begin(ASM_K_GEMV, 2.0 * sk().sp_nnz, 24.0 * sk().sp_nnz + 12.0 * sk().n);
            asmb::launch(k_spmv_t, asmb::blocks(sk().ldn * 8), dim3(256), h->stream, sk().d_sc_ptr, sk().d_sc_row, sk().d_sc_pos, v, y, out, sk().n, sk().ldn);
            end(id);
            return GemvT_Csc;
        }
        if (A == sk().d_Ah && (int64_t)sk().ldn * sk().Mp <= ((int64_t)1 << 27)) {
            // dense LP matrix of moderate size: through a transposed copy (made once per LP), one row-wise launch
            if (!sk().d_AhTg) sk().mem.zeroed(sk().d_AhTg, sk().ldn * sk().Mp, h->stream);
            if (!sk().ahTg_valid) {
                asmb::launch(k_transpose_dense, dim3((unsigned)((sk().n + 63) / 64), (unsigned)((sk().M + 63) / 64)), dim3(256), h->stream, sk().d_Ah, sk().ldn, sk().M, sk().n, sk().d_AhTg,
                             sk().Mp, (int64_t)-1);
                sk().ahTg_valid = true;
            }
            int id = begin(ASM_K_GEMV, 2.0 * sk().M * sk().n, 8.0 * sk().M * sk().ldn);
            asmb::launch(k_gemv_n_exact, asmb::blocks(sk().ldn, 4), dim3(256), h->stream, sk().d_AhTg, sk().Mp, y, out, sk().ldn, sk().M);
            end(id);
            return GemvT_Copy;
        }
        int64_t R, chunk;
        col_chunks(R, chunk);
        int id = begin(ASM_K_GEMV, 2.0 * sk().M * sk().n, 8.0 * sk().M * sk().ldn);
        asmb::launch(k_gemv_t_stage1, dim3((unsigned)((sk().ldn + 255) / 256), (unsigned)R), dim3(256), h->stream, A, sk().ldn, y, sk().d_partial, sk().M, sk().ldn, chunk);
        asmb::launch(k_gemv_t_stage2, asmb::blocks(sk().ldn), dim3(256), h->stream, sk().d_partial, out, R, sk().ldn);
        end(id);
        return GemvT_TwoStage;
    }
    // out[M] = A x   (host vectors)
    void gemv_n(const double* A, const double* x, double* out) {
        h2d(sk().d_vecN, x, sk().n, sk().ldn);
        launch_gemv_n(A, sk().d_vecN, sk().d_vecM);
        d2h(out, sk().d_vecM, sk().M);
    }
    // out[n] = A' y; returns launch_gemv_t's route
    int gemv_t(const double* A, const double* y, double* out) {
        h2d(sk().d_vecM, y, sk().M, sk().Mp);
        const int route = launch_gemv_t(A, sk().d_vecM, sk().d_vecN);
        d2h(out, sk().d_vecN, sk().n);
        return route;
    }

    // device-pointer variants (the IPM keeps its vectors in HBM)
    void gemv_n_dev(const double* A, const double* x, double* out) { launch_gemv_n(A, x, out); }
    void gemv_t_dev(const double* A, const double* y, double* out) { launch_gemv_t(A, y, out); }
    // Which chunk flags a Schur build skips by: Pattern = the fixed flags of all rows (tile_flags; of all columns for the transposed copy,
    // ensure_AhT), used when they fit the build; PerCall = made here for the row list, their executed share cached in `cache_slot` (>= 0)
    enum class NzFlags { Pattern, PerCall };
    // S[0:Ms,0:Ms] (lower, pitch ldS) = A[idx,:] diag(theta) A[idx,:]' + diag   with A = Ah, or with cols = true its transposed copy AhT
    // (column form: K = AhT diag(dinv) AhT' + diag(th)); idx == nullptr: the first Ms rows; everything already on the device
    void schur_syrk(bool cols, const int* idx_dev, int Ms, const double* theta_dev, const double* diag_dev, double* S, int64_t ldS, NzFlags flags,
                    int cache_slot = -1) {
        if (cols) ensure_AhT();
        const double* A = cols ? sk().d_AhT : sk().d_Ah;
        const int64_t ld = cols ? sk().ldT : sk().ldn;
        const int T = pick_tile(Ms);
        int nch = (int)(ld / ASM_KC);
        const unsigned char* nz = nullptr;
        double frac = 1.0;
        if (flags == NzFlags::PerCall) {
            const int TS = 32 * T, nt = (Ms + TS - 1) / TS;
            if (sk().nz_valid && nt > 0) {
                unsigned char* nz2 = sk().d_nz + sk().nz_half;
                launch_tile_flags(A, ld, Ms, T, nch, nz2, nch, idx_dev);
                frac = executed_fraction(nz2, nt, nch, cache_slot);
                nz = nz2;
            }
        } else if (cols) {
            if (sk().nzT_valid) { nz = sk().d_nzT; frac = sk().nzT_fraction; }
        } else {
            nch = sk().nz_pitch;
            if (sk().nz_valid && idx_dev == nullptr && Ms == (int)sk().M && T == sk().nz_T) { nz = sk().d_nz; frac = sk().nz_fraction; }
        }
        int id = begin(ASM_K_SYRK, frac * (double)Ms * (Ms + 1) * ld, 8.0 * (Ms * (double)ld + 0.5 * Ms * (double)Ms));
        launch_syrk(h->stream, T, A, ld, idx_dev, 0, Ms, (int)ld, theta_dev, diag_dev, S, ldS, 0, 0, -1, nz, nch, frac);
        end(id);
    }
    // The main factor's Schur matrix of a row list (reduced row form, active-set partitions): with the rows in the handle's banded order
    // (row_band > 0) built from the structural pairs - cpos maps a row to its place in the list - else gathered through idx
    void schur_rows(const int* idx_dev, const int* cpos_dev, int Ms, const double* theta_dev, const double* diag_dev) {
        if (sk().row_band > 0) schur_banded_dev(cpos_dev, Ms, theta_dev, diag_dev);
        else schur_syrk(false, idx_dev, Ms, theta_dev, diag_dev, sk().main_fac.S, sk().main_fac.ld, NzFlags::PerCall);
    }
    // clears the lower band of a banded factor's first Ms rows before an entry-by-entry build: the band plus what the blocked factorisation
    // reads beyond it (an outer panel of CHOL_NBO columns, tile rounding)
    void zero_band(const FacBuf& f, int Ms, int band) {
        const int64_t wz = std::min<int64_t>(round_up(band + 1, 64) + CHOL_NBO + 128, f.ld);
        asmb::launch(k_ns_zero_band, dim3((unsigned)((wz + 255) / 256), (unsigned)Ms), dim3(256), h->stream, f.S, f.ld, Ms, (int)wz);
    }
    // S[0:Ms,0:Ms] (lower) = Ah[idx,:] diag(theta) Ah[idx,:]' + diag for a row list in the handle's reverse Cuthill-McKee order
    // (Skeleton::row_band): banded, built entry by entry from the structural pairs - cpos maps a row to its place in the list (-1: not
    // in it).  The factorisation and the substitutions that follow stop at the band (the main factor's band).
    void schur_banded_dev(const int* cpos_dev, int Ms, const double* theta_dev, const double* diag_dev) {
        FacBuf& f = sk().main_fac;
        zero_band(f, Ms, sk().row_band);
        asmb::launch(k_schur_sparse, asmb::blocks(sk().n_rowpairs), dim3(256), h->stream, sk().d_rowpairs, sk().n_rowpairs, cpos_dev, sk().d_sp_ptr, sk().d_sp_col, sparse_vals(sk().d_Ah),
                     theta_dev, diag_dev, f.S, f.ld, nullptr);
    }
    // K = diag + Ah' diag(dinv) Ah (n x n, lower) with the COLUMNS in their reverse Cuthill-McKee order (Skeleton::col_band): the column form
    // of the restoration-phase Newton system, banded and built from the structural column pairs; `diag_place` is indexed by position
    void schur_banded_cols_dev(const double* dinv_dev, const double* diag_place) {
        FacBuf& f = sk().main_fac;
        const int n = (int)sk().n;
        zero_band(f, n, sk().col_band);
        asmb::launch(k_schur_sparse, asmb::blocks(sk().n_colpairs), dim3(256), h->stream, sk().d_colpairs, sk().n_colpairs, sk().d_colpos, sk().d_sc_ptr, sk().d_sc_row, sparse_vals(sk().d_Ah),
                     dinv_dev, diag_place, f.S, f.ld, sk().d_sc_pos);
    }
    // S0 = A_EF diag(Fm) A_EF' of the null-space form (equality rows in their reverse Cuthill-McKee order, Fm in F.Fm) into F.f0.S
    void ns_build_S0() {
        NsForm& F = *sk().nsf;
        const int nE = (int)F.L.nE;
        if (F.f0.band > 0) {
            // banded S0: the band is cleared (the last factor filled it) and the ~20 structural entries per row are written as merged
            // sparse dot products of the two rows - the dense rank-K build spends 3 ms on the zeros at n = 11 192
            zero_band(F.f0, nE, F.f0.band);
            asmb::launch(k_ns_s0_sparse, asmb::blocks(F.npairs), dim3(256), h->stream, F.S0pairs, F.npairs, sk().d_sp_ptr, sk().d_sp_col, sparse_vals(sk().d_Ah), F.Eidx, F.Fm, F.f0.S, F.f0.ld);
        } else {
            // S0 = A_EF A_EF' (the share of its chunk products cached per handle: the equality rows are fixed)
            schur_syrk(false, F.Eidx, nE, F.Fm, nullptr, F.f0.S, F.f0.ld, NzFlags::PerCall, 1);
        }
    }
    // C = (C0) -/+ A B'  on the matrix cores (k_gemm_nt); K a multiple of 32.  on: the stream (null: the handle's)
    void gemm_nt(const double* A, int64_t lda, const double* B, int64_t ldb, const double* C0, int64_t ldc0, double* C, int64_t ldc, int Ma, int Mb, int K, int mode,
                 hipStream_t on = nullptr) {
        if (Ma <= 0 || Mb <= 0) return;
        hipStream_t s = on ? on : h->stream;
        int id = begin(ASM_K_TRSV, 2.0 * Ma * (double)Mb * K, 8.0 * ((double)(Ma + Mb) * K + (double)Ma * Mb), s);
        // 64 x 64 tiles leave CUs idle when there are few right-hand sides: 32-row tiles then (same sums, same order)
        const int64_t t64 = (int64_t)((Mb + 63) / 64) * ((Ma + 63) / 64);
        // ... and 96 columns per workgroup when 32 x 64 tiles overshoot one workgroup per CU and 32 x 96 tiles do not
        const int64_t t3264 = (int64_t)((Mb + 63) / 64) * ((Ma + 31) / 32), t3296 = (int64_t)((Mb + 95) / 96) * ((Ma + 31) / 32);
        if (t64 < 2 * (int64_t)h->num_cus && Ma > 32 && t3264 > h->num_cus && t3296 <= h->num_cus)
            asmb::launch(k_gemm_nt32w, dim3((unsigned)((Mb + 95) / 96), (unsigned)((Ma + 31) / 32)), dim3(256), s, A, lda, B, ldb, C0, ldc0, C, ldc, Ma, Mb, K, mode);
        else if (t64 < 2 * (int64_t)h->num_cus && Ma > 32)
            asmb::launch(k_gemm_nt32, dim3((unsigned)((Mb + 63) / 64), (unsigned)((Ma + 31) / 32)), dim3(256), s, A, lda, B, ldb, C0, ldc0, C, ldc, Ma, Mb, K, mode);
        else
            asmb::launch(k_gemm_nt, dim3((unsigned)((Mb + 63) / 64), (unsigned)((Ma + 63) / 64)), dim3(256), s, A, lda, B, ldb, C0, ldc0, C, ldc, Ma, Mb, K, mode);
        end(id);
    }
    // Rows of R (nrhs x ldr, zero beyond column Ms) are right-hand sides of  L x = r  (forward) and then  L' x = z  (backward) with the
    // factor f (its matrix and wide-block inverses) and its transposed copy Lt (same pitch).  Right-looking block substitution over the
    // wide blocks: the block's solution is a product with the explicit inverse of the diagonal block, then ONE update of all the
    // remaining columns  R[:, rest] -= X_blk L[rest, blk]'  (K = the block width, every tile of the remainder in parallel) - both on the
    // matrix cores.  Forward: R -> X.  Backward (if Lt): X -> R.  The solution ends in R (backward) or X (forward only).
    void trsm_rows(const FacBuf& f, double* R, double* X, int64_t ldr, int nrhs, int Ms, const double* Lt) {
        const int nB = (Ms + f.wb - 1) / f.wb;
        for (int B = 0; B < nB; ++B) trsm_rows_fwd_step(f, R, X, ldr, nrhs, Ms, B);
        if (Lt) trsm_rows_bwd(f, R, X, ldr, nrhs, Ms, Lt);
    }
    // step B of the forward half: it needs the inverse of wide block B, column block B of the factor and step B - 1 - not the rest of the
    // factor, so it can follow a banded factorisation one wide block behind (Solver::ns_factor_S0).  on: the stream (null: the handle's)
    void trsm_rows_fwd_step(const FacBuf& f, double* R, double* X, int64_t ldr, int nrhs, int Ms, int B, hipStream_t on = nullptr) {
        const int WB = f.wb;
        const int b0 = B * WB, wv = std::min(WB, Ms - b0), b1 = b0 + wv, Kb = (int)round_up(wv, 32);
        gemm_nt(R + b0, ldr, f.Binv + (int64_t)B * WB * WB, WB, nullptr, 0, X + b0, ldr, nrhs, wv, Kb, 0, on);
        if (b1 < Ms) gemm_nt(X + b0, ldr, f.S + (int64_t)b1 * f.ld + b0, f.ld, R + b1, ldr, R + b1, ldr, nrhs, rowlim(f, Ms, b1) - b1, Kb, 1, on);
    }
    // the backward half: X -> R
    void trsm_rows_bwd(const FacBuf& f, double* R, double* X, int64_t ldr, int nrhs, int Ms, const double* Lt) {
        const int WB = f.wb;
        const int nB = (Ms + WB - 1) / WB;
        for (int B = nB - 1; B >= 0; --B) {
            const int b0 = B * WB, wv = std::min(WB, Ms - b0), Kb = (int)round_up(wv, 32);
            gemm_nt(X + b0, ldr, f.BinvT + (int64_t)B * WB * WB, WB, nullptr, 0, R + b0, ldr, nrhs, wv, Kb, 0);
            // rows of L in this block reach back `band` columns at most
            const int c0 = f.band > 0 ? std::max(0, (b0 - f.band) / 64 * 64) : 0;
            if (b0 > 0) gemm_nt(R + b0, ldr, Lt + (int64_t)c0 * f.ld + b0, f.ld, X + c0, ldr, X + c0, ldr, nrhs, b0 - c0, Kb, 1);
        }
    }
    // out[i] = sum_j Ah_ij^2 thinv_j   (sparse patterns only)
    void schur_diag(const double* thinv_dev, double* out_dev) {
        launch_sdiag_csr(sk().d_sp_ptr, sk().d_sp_col, sparse_vals(sk().d_Ah), thinv_dev, out_dev, sk().M);
    }
    unsigned launch_sdiag_csr(const int* ptr, const int* col, const double* vals, const double* thinv_dev, double* out_dev, int64_t M) {
        const dim3 g = asmb::blocks(M);
        asmb::launch(k_ipm_sdiag_csr, g, dim3(256), h->stream, ptr, col, vals, thinv_dev, out_dev, M);
        return g.x;
    }
    // transposed copy of Ah and its chunk flags (column form of the restoration-phase Newton system), once per LP
    void ensure_AhT() {
        if (sk().ahT_valid) return;
        asmb::launch(k_transpose_dense, dim3((unsigned)((sk().n + 63) / 64), (unsigned)((sk().M + 63) / 64)), dim3(256), h->stream, sk().d_Ah, sk().ldn, sk().M, sk().n, sk().d_AhT, sk().ldT,
                     (int64_t)-1);
        sk().nzT_valid = false;
        const int nch = (int)(sk().ldT / ASM_KC);
        if (!sk().dense_fast && nch <= ASM_MAXCHUNKS && sk().nnz * 8 <= sk().M * sk().n) {
            const int T = pick_tile(sk().n), TS = 32 * T;
            const int nt = (int)((sk().n + TS - 1) / TS);
            launch_tile_flags(sk().d_AhT, sk().ldT, sk().n, T, nch, sk().d_nzT, nch, nullptr);
            sk().nzT_fraction = executed_fraction(sk().d_nzT, nt, nch);
            sk().nzT_valid = true;
        }
        sk().ahT_valid = true;
    }
    // per (row tile, k-chunk) non-zero flags of Ah for the chunk-skipping Schur build (sparse Jacobians only)
    void tile_flags() {
        sk().nz_valid = false;
        if (sk().M == 0) return;
        const int nch = (int)(sk().ldn / ASM_KC);
        if (sk().dense_fast || nch > ASM_MAXCHUNKS || sk().nnz * 8 > sk().M * sk().n) return;     // dense pattern: nothing to skip
        if (sk().row_band > 0) return;      // banded row order: the full-row Schur matrix is built from its structural entries, not by k_syrk
        sk().nz_T = pick_tile(sk().M);
        const int TS = 32 * sk().nz_T;
        const int nt = (int)((sk().M + TS - 1) / TS);
        sk().nz_pitch = nch;
        launch_tile_flags(sk().d_Ah, sk().ldn, sk().M, sk().nz_T, nch, sk().d_nz, sk().nz_pitch, nullptr);
        sk().nz_valid = true;
        sk().nz_fraction = executed_fraction(sk().d_nz, nt, nch, 0);
    }
    // nz[t][c] (pitch nzpitch) = tile t (32 T rows of the list idx, or of the first Ms rows) of A has a non-zero in k-chunk c < nch
    void launch_tile_flags(const double* A, int64_t ld, int64_t Ms, int T, int nch, unsigned char* nz, int nzpitch, const int* idx_dev) {
        const int TS = 32 * T, nt = (int)((Ms + TS - 1) / TS);
        asmb::launch(k_tile_nzflags, dim3((unsigned)nt, (unsigned)((nch + 7) / 8)), dim3(256), h->stream, A, ld, Ms, TS, nch, nz, nzpitch, idx_dev);
    }
    // fraction of (tile pair, chunk) products actually executed: keeps the flop accounting of the roofline honest
    double executed_fraction(const unsigned char* d_flags, int nt, int nch, int cache_slot = -1) {
        if (h->timing == 0) return sk().nz_valid ? sk().nz_fraction : 1.0;      // only the flop accounting needs it: no read-back when timing is off
        // the flags follow the fixed pattern of the Jacobian: for the row sets that recur every LP (all rows; the equality rows of the
        // null-space form) the share is computed once per handle - the read-back and the O(nt^2 nch) host loop cost milliseconds per LP
        if (cache_slot >= 0 && sk().nz_frac_cache[cache_slot] >= 0.0) return sk().nz_frac_cache[cache_slot];
        const double fr_ = executed_fraction_now(d_flags, nt, nch);
        if (cache_slot >= 0) sk().nz_frac_cache[cache_slot] = fr_;
        return fr_;
    }
    double executed_fraction_now(const unsigned char* d_flags, int nt, int nch) {
        std::vector<unsigned char> fl((size_t)nt * nch);
        HIPCHK(asmb::copy_async(fl.data(), d_flags, fl.size(), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(asmb::sync(h->stream));
        double act = 0.0, tot = 0.0;
        for (int a = 0; a < nt; ++a)
            for (int b = 0; b <= a; ++b) {
                const unsigned char *fa = &fl[(size_t)a * nch], *fb = &fl[(size_t)b * nch];
                int cnt = 0;
                for (int c = 0; c < nch; ++c) cnt += fa[c] & fb[c];
                act += cnt;
                tot += nch;
            }
        return tot > 0 ? act / tot : 1.0;
    }
    // v[0:len] = val
    unsigned launch_ns_fill(double* v, double val, int64_t len) { const dim3 g = asmb::blocks(len); asmb::launch(k_ns_fill, g, dim3(256), h->stream, v, val, len); return g.x; }
    void chol_solve_dev(const FacBuf& f, const double* rhs_dev, double* out_dev, int Ms) {
        // the substitution runs in place in the caller's output buffer (w), z in d_vecM
        if (f.small && Ms <= ASM_SMALL_USE) {       // small systems: one workgroup, factor + inverses of its 64-wide diagonal blocks
            asmb::launch(k_small_solve, dim3(1), dim3(1024), h->stream, f.S, f.ld, f.Linv, Ms, rhs_dev, out_dev);
            return;
        }
        // a system of one wide block only READS its right-hand side (forward diagonal product); with more blocks the panel updates work in place
        const bool one_block = Ms <= f.wb;
        if (out_dev != rhs_dev && !one_block) HIPCHK(asmb::copy_async(out_dev, rhs_dev, Ms * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        int id = begin(ASM_K_TRSV, 2.0 * Ms * (double)Ms, 8.0 * Ms * (double)Ms);
        solve_launches(f, Ms, out_dev, one_block ? rhs_dev : out_dev);
        end(id);
    }
    // dd = (L L')^-1 rhs and du += dd (the refinement sweep of a null-space reduced solve).  A system of one wide block adds in its backward
    // diagonal product (k_wtrsv_bwd_diag_add: the lane that stores dd[i] also stores du[i] + dd[i]); every other system, and every system with
    // ASM_NS_FOLD=0, is chol_solve_dev followed by k_ns_add - the same values either way
    void chol_solve_add_dev(const FacBuf& f, const double* rhs_dev, double* dd_dev, double* du_dev, int Ms) {
        const bool small = f.small && Ms <= ASM_SMALL_USE;
        if (!h->knobs.ns_fold || small || Ms > f.wb) {
            chol_solve_dev(f, rhs_dev, dd_dev, Ms);
            asmb::launch(k_ns_add, asmb::blocks(Ms), dim3(256), h->stream, du_dev, dd_dev, du_dev, (int64_t)Ms);
            return;
        }
        int id = begin(ASM_K_TRSV, 2.0 * Ms * (double)Ms, 8.0 * Ms * (double)Ms);
        double* z = sk().d_vecM;
        if (f.wb == 1024) {
            asmb::launch((k_wtrsv_fwd_diag<1024>), dim3(1024 / 4), dim3(256), h->stream, f.Binv, 0, Ms, rhs_dev, z);
            asmb::launch((k_wtrsv_bwd_diag_add<1024>), dim3(1024 / 4), dim3(256), h->stream, f.BinvT, 0, Ms, z, dd_dev, Ms, du_dev);
        } else {
            asmb::launch((k_wtrsv_fwd_diag<512>), dim3(512 / 4), dim3(256), h->stream, f.Binv, 0, Ms, rhs_dev, z);
            asmb::launch((k_wtrsv_bwd_diag_add<512>), dim3(512 / 4), dim3(256), h->stream, f.BinvT, 0, Ms, z, dd_dev, Ms, du_dev);
        }
        end(id);
    }

    static int pick_tile(int64_t Ms) { return Ms >= 3072 ? 4 : (Ms >= 768 ? 2 : 1); }

    void launch_syrk(hipStream_t s, int T, const double* A, int64_t ld, const int* idx, int64_t row0, int Ms, int K, const double* theta,
                     const double* diag, double* S, int64_t ldS, int64_t srow0, int mode, int MsB = -1,
                     const unsigned char* nz = nullptr, int nzpitch = 0, double nzfrac = -1.0, int nsplit = 1, int64_t ksplit = 0) {
        int TS = 32 * T;
        int64_t nt = (Ms + TS - 1) / TS;
        int ntj = 0;
        int64_t blocks = (nt * (nt + 1) / 2 + 7) / 8 * 8;      // triangular: eight equal runs of the tile curve, one per XCD label (tri_tile_xcd)
        if (MsB >= 0) {                       // rectangular: all row tiles x the column tiles covering MsB columns
            ntj = (int)((MsB + TS - 1) / TS);
            blocks = nt * ntj;
        } else {
            MsB = Ms;
        }
        if (blocks <= 0) return;
        if (nz && ntj == 0) blocks = (nt * (nt + 1) / 2 + 511) / 512 * 512;      // sparse build: runs of 64 tile pairs dealt to the XCD labels (tri_tile_xcd)
        // per-launch timing of the MFMA kernel itself (algorithmic flops: Ms*MsB*K over the stored triangle/rectangle)
        double fl = (MsB == Ms && ntj == 0) ? (double)Ms * (Ms + 1) * K : 2.0 * ((double)Ms * MsB - 0.5 * (double)MsB * MsB) * K;
        if (nz) fl *= nzfrac >= 0.0 ? nzfrac : sk().nz_fraction;
        // timed on the stream it is launched on (HIP events see only their own stream)
        int kid = begin(ASM_K_SYRK_KERNEL, fl, 8.0 * ((double)(Ms + MsB) * K + (double)Ms * MsB), s);
        struct EndGuard { Dev* d; int id; ~EndGuard() { d->end(id); } } guard_{this, kid};
        if (T == 4 && mode == 1 && !nz && !idx && !theta && K % (2 * ASM_UPD_KC) == 0)      // Cholesky updates: their own kernel
            asmb::launch(k_syrk_upd, dim3((unsigned)blocks), dim3(256), s, A, ld, row0, Ms, K, S, ldS, srow0, MsB, ntj);
        else if (T == 4 && mode == 1 && !nz && K % 16 == 0)      // 16-wide k-chunks, two workgroups per CU
            asmb::launch((k_syrk<4, 8, 16, 4>), dim3((unsigned)blocks, (unsigned)nsplit), dim3(512), s, A, ld, idx, row0, Ms, K, theta, diag, S, ldS, srow0, mode, MsB, ntj, nz,
                         nzpitch, ksplit);
        else if (T == 4)
            asmb::launch((k_syrk<4, 8, 32, 2>), dim3((unsigned)blocks, (unsigned)nsplit), dim3(512), s, A, ld, idx, row0, Ms, K, theta, diag, S, ldS, srow0, mode, MsB, ntj, nz,
                         nzpitch, ksplit);
        else if (T == 2)
            asmb::launch((k_syrk<2, 4, 32, 1>), dim3((unsigned)blocks, (unsigned)nsplit), dim3(256), s, A, ld, idx, row0, Ms, K, theta, diag, S, ldS, srow0, mode, MsB, ntj, nz,
                         nzpitch, ksplit);
        else
            asmb::launch((k_syrk<1, 4, 32, 1>), dim3((unsigned)blocks, (unsigned)nsplit), dim3(256), s, A, ld, idx, row0, Ms, K, theta, diag, S, ldS, srow0, mode, MsB, ntj, nz,
                         nzpitch, ksplit);
    }

    void diag_prepare(const FacBuf& f, int Ms, int mode, double rel, double absv, double* diag0 = nullptr) {
        asmb::launch(k_diag_prepare, dim3(1), dim3(1024), h->stream, f.S, f.ld, Ms, diag0 ? diag0 : sk().d_diag0, mode, rel, absv);
    }
    // The k x k matrix of a null-space iteration, fN.S (lower) = G diag(theta) G' with its diagonal regularised (S_ii += rel S_ii + absv, the
    // plain diagonal kept in diag0), and its unregularised copy N0 (pitch fN.ld; mirrored into the upper triangle for the small systems).
    // G is k x K (pitch K).  nsplit > 1: split-K, the slices summed into `parts` (nsplit copies, fN.ld^2 doubles apart) and added in a fixed
    // order while the copy is made.  Everything up to the factorisation.
    void ns_newton_matrix(const double* G, int64_t K, const double* theta, int k, int nsplit, double* parts, const FacBuf& fN, double* N0, double* diag0, double rel,
                          double absv) {
        int id = begin(ASM_K_SYRK, (double)k * (k + 1) * K, 8.0 * (k * (double)K + 0.5 * k * (double)k));
        const int T = pick_tile(k);
        if (nsplit > 1) {
            const int64_t pstride = fN.ld * fN.ld;
            launch_syrk(h->stream, T, G, K, nullptr, 0, k, (int)K, theta, nullptr, parts, fN.ld, 0, 0, -1, nullptr, 0, -1.0, nsplit, pstride);
            end(id);
            asmb::launch(k_ns_reduce_lower, dim3((unsigned)((k + 255) / 256), (unsigned)k), dim3(256), h->stream, parts, nsplit, pstride, fN.ld, fN.S, N0, k,
                         k <= ASM_SMALL_USE ? 1 : 0, diag0, rel, absv);      // (+ k_diag_prepare, mode 0)
        } else {
            launch_syrk(h->stream, T, G, K, nullptr, 0, k, (int)K, theta, nullptr, fN.S, fN.ld, 0, 0);
            end(id);
            asmb::launch(k_ns_copy_lower, dim3((unsigned)((k + 255) / 256), (unsigned)k), dim3(256), h->stream, fN.S, fN.ld, N0, fN.ld, k, k <= ASM_SMALL_USE ? 1 : 0);
            diag_prepare(fN, k, 0, rel, absv, diag0);
        }
    }
    // explicit inverses (and their transposed copies) of the wide blocks B0 .. B1-1 on stream `on` (null: the handle's).  A block's launches
    // read its own rows of the factor and its own 64 x 64 block inverses and write its own Binv / BinvT (BinvT is the levels' scratch first)
    template <int WB>
    void trtri_launches(const FacBuf& f, int Ms, int B0, int B1, hipStream_t on = nullptr) {
        constexpr int WSUB = WB / ASM_NB;
        hipStream_t s = on ? on : h->stream;
        if (B1 <= B0) return;
        const unsigned nW = (unsigned)(B1 - B0);
        asmb::launch((k_trtri_init<WB>), dim3(nW, WSUB * WSUB), dim3(256), s, f.Linv, Ms, f.Binv, B0);
        for (int hh = 1; hh < WSUB; hh *= 2)
            for (int stage = 0; stage < 2; ++stage)
                asmb::launch((k_trtri_level<WB>), dim3(nW, (unsigned)(WSUB / (2 * hh)), (unsigned)(hh * hh)), dim3(256), s, f.S, f.ld, Ms, f.Binv, f.BinvT, hh, stage, B0);
        asmb::launch((k_transpose_wb<WB>), dim3(nW, WSUB * WSUB), dim3(256), s, f.Binv, f.BinvT, B0);
    }
    void trtri_blocks(const FacBuf& f, int Ms, int B0, int B1, hipStream_t on = nullptr) {
        if (f.wb == 1024) trtri_launches<1024>(f, Ms, B0, B1, on); else trtri_launches<512>(f, Ms, B0, B1, on);
    }
    // called by chol_launches_band after each panel launch: columns < I1 of the factor (and their 64 x 64 block inverses) are final, which
    // completes the first `done` wide blocks
    using PanelDone = std::function<void(int I1, int done)>;
    // want_inverse = false: the caller only solves against the factor and the factor is a "small" one (one-workgroup solves): the
    // explicit inverses of the wide blocks are not built
    // progress (only for a factor that band_panels_ok accepts): told after every panel launch how far the factor is final; its owner makes
    // the explicit inverses of the wide blocks as they complete (trtri_blocks), none are launched here
    void chol(const FacBuf& f, int Ms, double thr = 1e-14, bool want_inverse = true, const PanelDone* progress = nullptr) {
        if (Ms <= 0) return;
        if (progress && !band_panels_ok(f, Ms)) throw std::logic_error("Dev::chol: panel progress is reported by the band-panel factorisation only");
        // a banded factor (band b) costs about Ms (b + 64)^2 flops and touches Ms (b + 64) entries, not Ms^3 / 3 and Ms^2 / 2
        const double bw = f.band > 0 ? (double)std::min<int64_t>(Ms, (int64_t)f.band + 64) : (double)Ms;
        int id = begin(ASM_K_CHOL, f.band > 0 ? (double)Ms * bw * bw : (double)Ms * Ms * Ms / 3.0, 8.0 * 1.5 * Ms * bw);
        const bool skip_inv = !want_inverse && f.small && Ms <= ASM_SMALL_USE;
        // a factor of ONE wide block gets its explicit inverse inside the panel launches (helper workgroups of k_chol_panel_inv)
        const bool panel_inv = !skip_inv && Ms <= f.wb && f.band == 0 && f.Binv && f.BinvT && panel_inv_grid(Ms) <= h->panel_wgs;
        if (progress) chol_launches_band(f, Ms, thr, progress); else chol_launches(f, Ms, thr, panel_inv);
        if (skip_inv || panel_inv || progress) {
            end(id);
            h->stats.nfact += 1;
            return;
        }
        // explicit inverses of the wide diagonal blocks by divide and conquer over the 64-wide sub-blocks: diagonal
        // blocks from the panel kernels, then log2 levels of two launches each (the scratch T uses the buffer of the
        // transposed copy, which is written afterwards)
        trtri_blocks(f, Ms, 0, (Ms + f.wb - 1) / f.wb);
        end(id);
        h->stats.nfact += 1;
    }
    // the largest grid of the k_chol_panel_inv launches of a factor of one wide block (Ms <= wb <= CHOL_NBO: the inner panels of chol_chain's
    // only outer panel): G row-tile workgroups + one helper per 64 x 64 tile of the block rows a launch finishes.  All of them must be resident
    // within the handle's budget (a batch slot: its group's share); at most ASM_PNL_WT + ASM_PNL_NS * ASM_PNL_WT = 176, 144 for Ms <= 1024
    int panel_inv_grid(int Ms) const {
        const int T = (Ms + ASM_NB - 1) / ASM_NB;
        int grid = 0;
        for (int I0 = 0, I1 = 0; I0 < Ms; I0 = I1) {
            I1 = (Ms - I0 <= CHOL_NBI + 2 * ASM_NB) ? Ms : std::min(I0 + CHOL_NBI, Ms);
            const int nrt = (Ms - I0 + ASM_NB - 1) / ASM_NB, nst = (I1 - I0 + ASM_NB - 1) / ASM_NB;
            grid = std::max(grid, std::max(1, std::min(nrt, h->panel_wgs)) + nst * T);
        }
        return grid;
    }
    // block chain of one outer panel [K0, K1): 64-wide potrf / panel solve steps whose rank-64 updates stay inside a
    // 512-wide inner panel; the rest of the outer panel is updated once per inner panel with K = 512.  Launched on stream s; panel_inv: the
    // panel launches also make the explicit inverse of the factor's one wide block
    void chol_chain(const FacBuf& f, int Ms, double thr, int K0, int K1, hipStream_t s, bool panel_inv, bool beside_updates = false) {
        for (int I0 = K0, Inext = K0; I0 < K1; I0 = Inext) {
            // a remainder of at most two 64-wide steps joins the last inner panel (k = 519: one launch of nine steps instead of a panel launch, an
            // in-panel update and a second panel launch for the last seven columns)
            const int I1 = (K1 - I0 <= CHOL_NBI + 2 * ASM_NB) ? K1 : std::min(I0 + CHOL_NBI, K1);
            Inext = I1;
            const int Mi = rowlim(f, Ms, I1);           // banded factor: the rows below are out of this inner panel's reach
            {      // (scope of the panel launch's timing region: it ends before the update of the rest of the outer panel)
                // the <= 8 steps of this inner panel in one dataflow launch (k_chol_panel): row tiles are owned by workgroups,
                // diagonal-block factors and the panel tiles other workgroups need travel through release / acquire flags
                const int nrt = (Mi - I0 + ASM_NB - 1) / ASM_NB;
                // grid: one workgroup per row tile while they all fit (77 KB of LDS: two per CU); measured: fewer workgroups with several
                // tiles each lengthen every step (M = 11192: 16.7 ms with one tile per workgroup, 21.1 ms with three)
                const int G = std::max(1, std::min(nrt, h->panel_wgs));
                h->panel_epoch += 1;              // flags are "set" when they hold this launch's epoch: no reset between launches
                if (h->panel_epoch == 0) h->panel_epoch = 1;
                // algorithmic flops of the launch: per 64-wide step the factor + inverse of the diagonal block, the panel solve of the rows below
                // and the rank-64 update of the panel's remaining columns
                double pfl = 0.0;
                for (int k0 = I0; k0 < std::min(I1, Ms); k0 += ASM_NB) {
                    const double r = std::max(0, Mi - (k0 + ASM_NB)), w = std::max(0, std::min(I1, Mi) - (k0 + ASM_NB));
                    pfl += 2.0 / 3.0 * ASM_NB * ASM_NB * ASM_NB + 2.0 * r * ASM_NB * ASM_NB + 2.0 * ASM_NB * (r * w - 0.5 * w * w);
                }
                int pid = begin(ASM_K_PANEL_KERNEL, pfl, 8.0 * 2.0 * (double)(Mi - I0) * (double)(std::min(I1, Mi) - I0), s);
                struct PEnd { Dev* d; int id; ~PEnd() { d->end(id); } } pend_{this, pid};
                // beside the trailing update the register-capped build must be used (its wavefronts have to fit into freed update slots)
                if (panel_inv && !beside_updates) {
                    // one wide block: its explicit inverse is made inside the launch by helper workgroups, one per 64 x 64 tile of the block
                    // rows this inner panel finishes (k_chol_panel_inv) - no k_trtri_* launches afterwards
                    const int nst = (std::min(I1, Ms) - I0 + ASM_NB - 1) / ASM_NB, T = (Ms + ASM_NB - 1) / ASM_NB;
                    asmb::launch_resident(k_chol_panel_inv, dim3((unsigned)(G + nst * T)), dim3(256), s, f.S, f.ld, I0, std::min(I1, Ms), Mi, sk().d_diag0, thr, f.Linv, sk().d_pflags,
                                          sk().d_ptmo, h->panel_epoch, f.Binv, f.BinvT, f.wb, G);
                } else if (beside_updates)
                    asmb::launch_resident(k_chol_panel, dim3((unsigned)G), dim3(256), s, f.S, f.ld, I0, std::min(I1, Ms), Mi, sk().d_diag0, thr, f.Linv, sk().d_pflags, sk().d_ptmo,
                                          h->panel_epoch);
                else
                    asmb::launch_resident(k_chol_panel_solo, dim3((unsigned)G), dim3(256), s, f.S, f.ld, I0, std::min(I1, Ms), Mi, sk().d_diag0, thr, f.Linv, sk().d_pflags, sk().d_ptmo,
                                          h->panel_epoch);
            }
            if (I1 < K1 && I1 < Mi) {
                int rem = Mi - I1;
                launch_syrk(s, pick_tile(rem), f.S + I0, f.ld, nullptr, I1, rem, I1 - I0, nullptr, nullptr, f.S, f.ld, I1, 1, std::min(K1 - I1, rem));
            }
        }
    }
    // Banded factor, every inner panel with its whole trailing update in ONE launch (k_chol_panel_band): no rank-K launches between the panels.
    // Possible when a panel and the band's reach fit ASM_PNL_NRT row tiles and the workgroups (one per row tile + one per trailing tile) are
    // all resident; a batch slot keeps the launch sequence (its panel launches are merged across scenarios).
    bool band_panels_ok(const FacBuf& f, int Ms) const {
        if (f.band <= 0 || h->batch_slot || Ms <= CHOL_NBI + 2 * ASM_NB) return false;
        const int nrt = (CHOL_NBI + 2 * ASM_NB + (int)round_up(f.band, 64) + ASM_NB - 1) / ASM_NB + 1;
        const int m = nrt - CHOL_NBI / ASM_NB;
        return nrt <= ASM_PNL_NRT && nrt + m * (m + 1) / 2 <= h->panel_wgs;
    }
    void chol_launches_band(const FacBuf& f, int Ms, double thr, const PanelDone* progress = nullptr) {
        for (int I0 = 0, I1 = 0; I0 < Ms; I0 = I1) {
            I1 = (Ms - I0 <= CHOL_NBI + 2 * ASM_NB) ? Ms : I0 + CHOL_NBI;
            const int Mi = rowlim(f, Ms, I1);
            const int nrt = (Mi - I0 + ASM_NB - 1) / ASM_NB, nst = (I1 - I0 + ASM_NB - 1) / ASM_NB, m = nrt - nst;
            h->panel_epoch += 1;
            if (h->panel_epoch == 0) h->panel_epoch = 1;
            double pfl = 0.0;
            for (int k0 = I0; k0 < I1; k0 += ASM_NB) {
                const double r = std::max(0, Mi - (k0 + ASM_NB));
                pfl += 2.0 / 3.0 * ASM_NB * ASM_NB * ASM_NB + 2.0 * r * ASM_NB * ASM_NB + 2.0 * ASM_NB * (0.5 * r * r);      // factor, panel solve, update of everything in reach
            }
            int pid = begin(ASM_K_PANEL_KERNEL, pfl, 8.0 * 2.0 * (double)(Mi - I0) * (double)(Mi - I0) * 0.5, h->stream);
            const int nhelp = (m * (m + 1) / 2 + ASM_BAND_TPH - 1) / ASM_BAND_TPH;      // helper workgroups: one per trailing tile
            asmb::launch_resident(k_chol_panel_band, dim3((unsigned)(nrt + nhelp)), dim3(256), h->stream, f.S, f.ld, I0, I1, Mi, sk().d_diag0, thr, f.Linv, sk().d_pflags, sk().d_ptmo,
                                  h->panel_epoch, nrt);
            end(pid);
            // the launch applied its whole trailing update and later launches write columns >= I1 only: a wide block is complete once I1 has
            // reached its end (the last one with the last launch, which may have absorbed a remainder)
            if (progress) (*progress)(I1, I1 >= Ms ? (Ms + f.wb - 1) / f.wb : I1 / f.wb);
        }
    }
    void chol_launches(const FacBuf& f, int Ms, double thr, bool panel_inv) {
        if (band_panels_ok(f, Ms)) { chol_launches_band(f, Ms, thr); return; }
        // Two-level right-looking blocking with look-ahead.  64-wide steps inside a 1024-wide outer panel touch only the
        // panel's own columns; the trailing matrix is read-modify-written once per outer panel (K = 1024), in two parts:
        // (a) the columns of the NEXT outer panel, (b) the rest.  The next panel's serial block chain then runs on a second
        // stream beside (b), so the latency-bound chain hides under the MFMA-bound update.
        const int NBO = CHOL_NBO;
        const int nP = (Ms + NBO - 1) / NBO;
        const bool la = nP > 2 && !h->batch_slot;      // (a batch slot records its launches for ONE stream)
        while ((int)h->la_events.size() < 2 * nP + 2) {
            hipEvent_t e;
            HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            h->la_events.push_back(e);
        }
        chol_chain(f, Ms, thr, 0, std::min(NBO, Ms), h->stream, panel_inv);
        for (int p = 0; p < nP; ++p) {
            const int K0 = p * NBO, K1 = std::min(K0 + NBO, Ms);
            if (K1 >= Ms) break;
            const int rem = rowlim(f, Ms, K1) - K1, wa = std::min(NBO, rem);   // next panel = first `wa` trailing columns (banded: `rem` stops where the panel's reach ends)
            hipEvent_t e_a = h->la_events[2 * p], e_c = h->la_events[2 * p + 1];
            // (a) rows >= K1, columns of the next outer panel
            launch_syrk(h->stream, pick_tile(rem), f.S + K0, f.ld, nullptr, K1, rem, K1 - K0, nullptr, nullptr, f.S, f.ld, K1, 1, wa);
            if (la) {
                HIPCHK(hipEventRecord(e_a, h->stream));
                HIPCHK(hipStreamWaitEvent(h->stream2, e_a, 0));
                chol_chain(f, Ms, thr, K1, std::min(K1 + NBO, Ms), h->stream2, panel_inv, true);     // next panel's chain beside (b)
                HIPCHK(hipEventRecord(e_c, h->stream2));
            }
            // (b) the rest of the trailing matrix
            const int rem2 = rem - wa;
            if (rem2 > 0)
                launch_syrk(h->stream, pick_tile(rem2), f.S + K0, f.ld, nullptr, K1 + wa, rem2, K1 - K0, nullptr, nullptr, f.S, f.ld, K1 + wa, 1);
            if (la) HIPCHK(hipStreamWaitEvent(h->stream, e_c, 0));
            else chol_chain(f, Ms, thr, K1, std::min(K1 + NBO, Ms), h->stream, panel_inv);
        }
    }
    // out = (L L')^-1 rhs   (compact vectors of length Ms)
    void chol_solve(const FacBuf& f, const double* rhs, double* out, int Ms) {
        h2d(sk().d_vecM2, rhs, Ms, Ms);
        int id = begin(ASM_K_TRSV, 2.0 * Ms * (double)Ms, 8.0 * Ms * (double)Ms);
        solve_launches(f, Ms, sk().d_vecM2, sk().d_vecM2);
        end(id);
        d2h(out, sk().d_vecM2, Ms);
    }
    // the substitution runs in w (a copy of the right-hand side, updated in place); the forward diagonal products read src: w, or the
    // right-hand side itself for a system of one wide block (no copy into w first)
    void solve_launches(const FacBuf& f, int Ms, double* w, const double* src) {
        if (f.wb == 1024) solve_launches_wb<1024>(f, Ms, w, src); else solve_launches_wb<512>(f, Ms, w, src);
    }
    template <int WB>
    void solve_launches_wb(const FacBuf& f, int Ms, double* w, const double* src) {
        // forward: w updated in place, z -> d_vecM ; backward: x -> w (w is dead by then)
        double* z = sk().d_vecM;
        const int nB = (Ms + WB - 1) / WB;
        for (int B = 0; B < nB; ++B) {
            int b1 = std::min((B + 1) * WB, Ms);
            asmb::launch((k_wtrsv_fwd_diag<WB>), dim3(WB / 4), dim3(256), h->stream, f.Binv, B, Ms, src, z);
            const int Me = rowlim(f, Ms, b1);
            int rem = Me - b1;
            if (rem > 0)
                asmb::launch((k_wtrsv_fwd_panel<WB>), dim3((unsigned)((rem + 4 * ASM_FWD_RPW - 1) / (4 * ASM_FWD_RPW))), dim3(256), h->stream, f.S, f.ld, B, Me, z, w);
        }
        for (int B = nB - 1; B >= 0; --B) {
            int b1 = std::min((B + 1) * WB, Ms);
            const int Me = rowlim(f, Ms, b1);
            int rem = Me - b1;
            int np = 0;
            if (rem > 0) {
                np = (rem + ASM_WBROWS - 1) / ASM_WBROWS;
                asmb::launch((k_wtrsv_bwd_panel<WB>), dim3((unsigned)np), dim3(256), h->stream, f.S, f.ld, B, Me, w, sk().d_wpart);
            }
            if (np > 0) {
                asmb::launch((k_wtrsv_bwd_reduce<WB>), dim3(WB / ASM_NB), dim3(256), h->stream, B, Ms, z, sk().d_wpart, np, sk().d_wt);
                asmb::launch((k_wtrsv_bwd_diag<WB>), dim3(WB / 4), dim3(256), h->stream, f.BinvT, B, Ms, sk().d_wt, w, WB);
            } else {
                // last wide block (the only one of a small system): nothing to subtract, the diagonal product reads z itself
                asmb::launch((k_wtrsv_bwd_diag<WB>), dim3(WB / 4), dim3(256), h->stream, f.BinvT, B, Ms, z + (int64_t)B * WB, w, Ms - B * WB);
            }
        }
    }
    void assemble() {
        if (sk().J_valid) return;                 // J in HBM already matches dE (one assembly per evaluation, shared by the norms and the LP)
        sk().J_valid = true;
        sk().spv_J_valid = false;
        int id = begin(ASM_K_ASSEMBLE, 0.0, 8.0 * sk().nnz + 8.0 * sk().nu + (sk().dense_fast ? 0.0 : 24.0 * sk().nu + 8.0 * sk().nnz));
        if (sk().dense_fast) {
            int64_t total = sk().m * sk().n;
            unsigned g = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
            asmb::launch(k_assemble_dense, dim3(g), dim3(256), h->stream, sk().d_dE, sk().d_J, sk().m, sk().n, sk().ldn);
        } else if (sk().nu > 0) {
            unsigned g = (unsigned)std::min<int64_t>((sk().nu + 255) / 256, 4096);
            asmb::launch(k_assemble, dim3(g), dim3(256), h->stream, sk().d_dE, sk().d_perm, sk().d_ustart, sk().d_uoff, sk().d_adjoff, sk().d_J, sk().nu);
        }
        end(id);
    }
    // rel[j] = max_i |J_ij| / max_k |J_ik|   (host, n) - matrix-based cap of the column scale
    void col_relmax(double* rel) {
        if (sk().M == 0) { std::fill(rel, rel + sk().n, 0.0); return; }
        int64_t R, chunk;
        col_chunks(R, chunk);
        if (sk().sp_ok) {                      // sparse pattern: the same maxima over the stored entries only
            const double* vJ = sparse_vals(sk().d_J);
            int id = begin(ASM_K_SCALE, 0.0, 8.0 * 3.0 * sk().sp_nnz);
            asmb::launch(k_sp_row_absmax, asmb::blocks(sk().M), dim3(256), h->stream, sk().d_sp_ptr, vJ, sk().d_rho, sk().M);
            asmb::launch(k_sp_col_relmax, asmb::blocks(sk().ldn), dim3(256), h->stream, sk().d_sc_ptr, sk().d_sc_row, sk().d_sc_pos, vJ, sk().d_rho, sk().d_vecN, sk().n, sk().ldn);
            end(id);
            d2h(rel, sk().d_vecN, sk().n);
            return;
        }
        int id = begin(ASM_K_SCALE, 0.0, 8.0 * 2.0 * sk().M * sk().ldn);
        asmb::launch(k_row_absmax, asmb::blocks(sk().M, 4), dim3(256), h->stream, sk().d_J, sk().ldn, sk().d_rho, sk().M, sk().ldn);
        asmb::launch(k_col_relmax_stage1, dim3((unsigned)((sk().ldn + 255) / 256), (unsigned)R), dim3(256), h->stream, sk().d_J, sk().ldn, sk().d_rho, sk().d_partial, sk().M, sk().ldn, chunk);
        asmb::launch(k_col_relmax_stage2, asmb::blocks(sk().ldn), dim3(256), h->stream, sk().d_partial, sk().d_vecN, R, sk().ldn);
        end(id);
        d2h(rel, sk().d_vecN, sk().n);
    }
    // Ah = diag(1/rho) J diag(c);  rho (host, M)
    void scale(const double* c, double* rho) {
        sk().spv_Ah_valid = false;
        sk().ahT_valid = false;
        sk().ahTg_valid = false;
        if (sk().M == 0) return;
        h2d(sk().d_c, c, sk().n, sk().ldn);
        if (sk().sp_ok) {
            const double* vJ = sparse_vals(sk().d_J);
            int id = begin(ASM_K_SCALE, 0.0, 8.0 * 4.0 * sk().sp_nnz);
            asmb::launch(k_sp_scale_rows, asmb::blocks(sk().M), dim3(256), h->stream, sk().d_sp_ptr, sk().d_sp_col, sk().d_sp_off, vJ, sk().d_c, sk().d_Ah, sk().d_spv_Ah, sk().d_rho, sk().M);
            end(id);
            sk().spv_Ah_valid = true;
            d2h(rho, sk().d_rho, sk().M);
            return;
        }
        int id = begin(ASM_K_SCALE, 0.0, 8.0 * 3.0 * sk().M * sk().ldn);
        asmb::launch(k_scale_rows, dim3((unsigned)sk().M), dim3(256), h->stream, sk().d_J, sk().d_c, sk().d_Ah, sk().d_rho, sk().n, sk().ldn);
        end(id);
        d2h(rho, sk().d_rho, sk().M);
    }
    // From the dE in HBM to the scaled LP matrix (oracle: scale_lp): assemble J, rel = col_relmax, the column scale
    // c_j = pow2_round(min(box half-width, 1 / rel_j)), Ah = diag(1 / rho) J diag(c).  rel, c (n) and rho (M) on the host.  `after(name)` runs
    // after each stage that ran.  The stages hook runs a subset (`stages`, ASM_SKS_* bits) and may scale by a c of its own (`c_use`).
    template <class After>
    void scaled_matrix(const double* lb, const double* ub, double* rel, double* c, double* rho, After&& after, unsigned stages = ASM_SKS_ASSEMBLE | ASM_SKS_COLSCALE | ASM_SKS_SCALE,
                       const double* c_use = nullptr) {
        if (stages & ASM_SKS_ASSEMBLE) {
            assemble();
            after("assemble");
        }
        if (stages & ASM_SKS_COLSCALE) {
            col_relmax(rel);
            after("relmax");
            for (int64_t j = 0; j < sk().n; ++j) {
                double c_mat = rel[j] > 0.0 ? 1.0 / rel[j] : 1.0;
                c[j] = pow2_round(std::min(std::max(ub[j], -lb[j]), c_mat));
            }
        }
        if (stages & ASM_SKS_SCALE) {
            scale(c_use ? c_use : c, rho);
            after("scale");
        }
    }
    // out[i] = ||J_i||_2 over the first m rows (device); from_pattern: from the CSR copy where the pattern is sparse (the same bits, k_sp_row_norms)
    void launch_row_norms(double* out, bool from_pattern) {
        const int64_t m = sk().m;
        if (m == 0) return;
        if (const double* vJ = from_pattern ? sparse_vals(sk().d_J) : nullptr)      // sparse pattern: from the CSR copy (13 k entries instead of a 75 MB dense sweep at case300 size)
            asmb::launch(k_sp_row_norms, asmb::blocks(m, 4), dim3(256), h->stream, sk().d_sp_ptr, sk().d_sp_col, vJ, out, m);
        else
            asmb::launch(k_row_norms, asmb::blocks(m, 4), dim3(256), h->stream, sk().d_J, sk().ldn, out, m, sk().ldn);
    }
};

// =====================================================================================================
// LP in scaled units (oracle/lp_solver.py: class LP / scale_lp)
// =====================================================================================================
struct SLP {
    int64_t n, M, ns;
    vec q, r, lb, ub, w, slo;
    const int* rtype;
    const int* srow;
    const double* scoef;
    double scale_q;
};

// Pitches and buffer lengths of the device-resident interior-point state for an LP of n columns, M rows and ns slack columns
// (do_setup allocates by them; Solver::ipm_bind places the vectors)
struct IpmLayout {
    int64_t ldn, Mp, nsp;
    IpmLayout(int64_t n, int64_t M, int64_t ns) : ldn(round_up(n, 32)), Mp(round_up(std::max<int64_t>(M, 1), 16)), nsp(round_up(std::max<int64_t>(ns, 1), 16)) {}
    int64_t arena_len() const { return 24 * ldn + 23 * Mp + 16 * nsp + 64; }
    int64_t snap_len() const { return 6 * ldn + 3 * Mp + 3 * nsp; }
    int64_t int_len() const { return 3 * Mp + nsp; }
};

// Pitches and lengths of the two arenas of the device-resident active-set machinery (asm_as_kernels.hip.h): do_setup allocates by them,
// Solver::as_bind places the vectors.  Doubles: 17 n-vectors, 17 M-vectors, 4 slack vectors, the scalar block.  Ints: six working sets
// (rowst | bst | sst each), ksoft | Hidx | hpos, Fidx | fpos, the counter block.
struct AsLayout {
    int64_t ldn, Mp, nsp;
    AsLayout(int64_t ln, int64_t lm, int64_t ls) : ldn(ln), Mp(lm), nsp(ls) {}
    explicit AsLayout(const IpmLayout& l) : ldn(l.ldn), Mp(l.Mp), nsp(l.nsp) {}
    int64_t dbl_len() const { return 17 * ldn + 17 * Mp + 4 * nsp + 64; }
    int64_t int_len() const { return 6 * (Mp + ldn + nsp) + 3 * Mp + 2 * ldn + 64; }
};

// Sequence number for the next publishing kernel (0 = the kernel does not publish: copy path)
unsigned pub_next(asm_handle* h) {
    if (!h->knobs.spin_read) return 0;
    h->sk->scal_seq += 1;
    if (h->sk->scal_seq == 0) h->sk->scal_seq = 1;
    return h->sk->scal_seq;
}

struct Solver {
    // out = A x for a k x ncols matrix of few, long rows (the basis Zt): one workgroup per row when that fills the chip better
    // (`on`: the stream of the launch; null: the handle's)
    unsigned gemv_rows(const double* A, int64_t ld, const double* x, double* out, int64_t rows, int64_t ncols, hipStream_t on = nullptr) {
        if (!on) on = h->stream;
        if (rows <= 2048 && ncols >= 2048) {
            asmb::launch(k_gemv_n_wide, dim3((unsigned)rows), dim3(256), on, A, ld, x, out, rows, ncols);
            return (unsigned)rows;
        }
        const dim3 g = asmb::blocks(rows, 4);
        asmb::launch(k_gemv_n, g, dim3(256), on, A, ld, x, out, rows, ncols);
        return g.x;
    }
    // workgroups of the interior-point reductions (k_ipm_measures / _steps / _muaff): 1024 elements per workgroup and sweep, at most IPM_RED_MAXWG
    unsigned red_grid() const { return (unsigned)std::min<int64_t>(IPM_RED_MAXWG, std::max<int64_t>(1, (std::max(std::max(lp.n, lp.M), lp.ns) + 4095) / 4096)); }
    static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    asm_handle* h;
    Dev dev;
    SLP lp;

    explicit Solver(asm_handle* hh) : h(hh), dev(hh) {}
    Skeleton& sk() const { return *h->sk; }

    void atv(const vec& y, vec& out) {
        out.resize(lp.n);
        dev.gemv_t(sk().d_Ah, y.data(), out.data());
    }

    // ---------------------------------------------------------------- interior point (oracle: class IPM)
    // Form of the Newton system of an iteration (oracle: IPM.run, one branch per form): null-space (normal phase,
    // many hard equality rows), column (restoration phase, dense or banded columns), reduced row (normal phase, large sparse problems),
    // full row in the handle's banded row order, full dense row.  The first three fall back to the next in this order.
    enum class NewtonForm { NullSpace, Column, ReducedRow, BandedRow, Row };
    struct IpmState {
        int64_t ncomp = 1;
        vec pinf_hist;
        bool usable[3] = {false, false, false};   // NullSpace, Column, ReducedRow: available for this LP (ipm_init), cleared on fall-back
        int col_iters = 0;
        int ns_iters = 0, ns_k = 0;
        bool ns_e_ready = false;  // the component e of the iterate outside pbar + null(A_EF) has been split off
        int iters = 0;
        int status = ASM_OTHER;
        double mu = 0, pinf = 0, dinf = 0, gap = 0, ymax = 0, rpmax = 0;
    } ip;

    // ---- device-resident IPM state (asm_ipm_kernels.hip.h) ---------------------------------------------------
    IpmPtrs P;
    IpmDir dirA, dirC;
    double *d_sres = nullptr, *d_corr = nullptr, *d_tN = nullptr, *d_pcg = nullptr;

    // where the interior-point state lives: the handle's arena (ipm_bind()), or buffers of a test hook's with the same pitches
    struct IpmArena {
        double* base = nullptr;       // IpmLayout::arena_len() doubles
        int* ibase = nullptr;         // rtype | rs0 | rs1 (pitch lm each) | srow
        double* snap = nullptr;       // best-iterate snapshot (IpmLayout::snap_len() doubles)
        int64_t ln = 0, lm = 0, ls = 0;
        double* hscal = nullptr; unsigned* hseq = nullptr; double* rpart = nullptr; unsigned* rcnt = nullptr;
    } arena;
    void ipm_bind() {
        IpmArena a;
        a.base = sk().d_ipm; a.ibase = sk().d_ipm_i; a.snap = sk().d_ipm_snap;
        a.ln = sk().ldn; a.lm = sk().Mp; a.ls = sk().nsp;
        a.hscal = sk().d_hscal; a.hseq = sk().d_hseq; a.rpart = sk().d_redpart; a.rcnt = sk().d_redcnt;
        ipm_bind(a);
    }
    // the ONLY place that lays the arena out
    void ipm_bind(const IpmArena& ar) {
        arena = ar;
        double* a = ar.base;
        const int64_t ln = ar.ln, lm = ar.lm, ls = ar.ls;
        auto N = [&]() { double* r_ = a; a += ln; return r_; };
        auto Mv = [&]() { double* r_ = a; a += lm; return r_; };
        auto Sv = [&]() { double* r_ = a; a += ls; return r_; };
        double *q = N(), *lb = N(), *ub = N();
        P.q = q; P.lb = lb; P.ub = ub;
        P.p = N(); P.tL = N(); P.tU = N(); P.muL = N(); P.muU = N(); P.aty = N(); P.rdp = N(); P.thp_inv = N();
        P.hp = N(); P.tmpn = N(); P.rcL = N(); P.rcU = N();
        dirA.dp = N(); dirA.dmuL = N(); dirA.dmuU = N(); dirC.dp = N(); dirC.dmuL = N(); dirC.dmuU = N();
        d_tN = N();
        double* r = Mv();
        P.r = r;
        P.g = Mv(); P.y = Mv(); P.pi = Mv(); P.act = Mv(); P.rp = Mv(); P.dS = Mv(); P.t1 = Mv(); P.rhs = Mv(); P.res = Mv(); P.rcg = Mv();
        dirA.dg = Mv(); dirA.dy = Mv(); dirA.dpi = Mv(); dirC.dg = Mv(); dirC.dy = Mv(); dirC.dpi = Mv();
        d_sres = Mv(); d_corr = Mv(); d_pcg = Mv();
        double *w = Sv(), *slo = Sv(), *scoef = Sv();
        P.w = w; P.slo = slo; P.scoef = scoef;
        P.s = Sv(); P.ts = Sv(); P.mus = Sv(); P.rds = Sv(); P.ths_inv = Sv(); P.hs = Sv(); P.rcs = Sv();
        dirA.ds = Sv(); dirA.dmus = Sv(); dirC.ds = Sv(); dirC.dmus = Sv();
        P.scal = a;
        P.hscal = ar.hscal; P.hseq = ar.hseq;
        P.rpart = ar.rpart; P.rcnt = ar.rcnt;
        P.rtype = ar.ibase; P.rs0 = ar.ibase + lm; P.rs1 = ar.ibase + 2 * lm; P.srow = ar.ibase + 3 * lm;
    }
    // the vectors of the arena in the order the test hooks report them (include/asm_hip.h, asm_test_ipm_stages)
    void ipm_vectors(const double* (&vs)[ASM_IPM_NVEC]) const {
        const double* v[ASM_IPM_NVEC] = {P.q, P.lb, P.ub, P.r, P.w, P.slo, P.scoef, P.p, P.s, P.g, P.y, P.tL, P.tU, P.muL, P.muU, P.ts, P.mus, P.pi, P.act, P.aty, P.rp,
                                         P.rdp, P.rds, P.thp_inv, P.ths_inv, P.dS, P.hp, P.hs, P.tmpn, P.t1, P.rhs, P.res, P.rcL, P.rcU, P.rcs, P.rcg,
                                         dirA.dp, dirA.ds, dirA.dg, dirA.dy, dirA.dmuL, dirA.dmuU, dirA.dmus, dirA.dpi,
                                         dirC.dp, dirC.ds, dirC.dg, dirC.dy, dirC.dmuL, dirC.dmuU, dirC.dmus, dirC.dpi,
                                         d_sres, d_corr, d_pcg, d_tN};
        for (int q = 0; q < ASM_IPM_NVEC; ++q) vs[q] = v[q];
    }
    // ---- launch sites of the stage kernels (asm_ipm_kernels.hip.h): the solver and the test hook asm_test_ipm_stages launch through these
    // members only; each returns the number of workgroups it launched
    unsigned launch_init_p(int origin) { const unsigned g = grid_all(); asmb::launch(k_ipm_init_p, dim3(g), dim3(256), h->stream, P, origin); return g; }
    unsigned launch_init_rest(double mu_factor) { const unsigned g = grid_all(); asmb::launch(k_ipm_init_rest, dim3(g), dim3(256), h->stream, P, mu_factor); return g; }
    unsigned launch_measures(unsigned pub) { const unsigned g = red_grid(); asmb::launch(k_ipm_measures, dim3(g), dim3(1024), h->stream, P, pub); return g; }
    unsigned launch_theta(double rho_p) { const unsigned g = grid_all(); asmb::launch(k_ipm_theta, dim3(g), dim3(256), h->stream, P, rho_p); return g; }
    unsigned launch_rhs1(const IpmDir& base, int mode, double tp, double td) {
        const unsigned g = grid_all();
        asmb::launch(k_ipm_rhs1, dim3(g), dim3(256), h->stream, P, base, mode, tp, td, MCC_BMIN, MCC_BMAX);
        return g;
    }
    unsigned launch_rhs2(double res) { const unsigned g = grid_all(); asmb::launch(k_ipm_rhs2, dim3(g), dim3(256), h->stream, P, res); return g; }
    unsigned launch_vec_mul(double* x, const double* a, int64_t len) { const dim3 g = asmb::blocks(len); asmb::launch(k_vec_mul, g, dim3(256), h->stream, x, a, len); return g.x; }
    unsigned launch_res(const double* dy, unsigned pub, int spec, double crel, double floor_) {
        asmb::launch(k_ipm_res, dim3(1), dim3(1024), h->stream, P, d_sres, dy, pub, spec, crel, floor_);
        return 1;
    }
    unsigned launch_pcg_start() { asmb::launch(k_pcg_start, dim3(1), dim3(1024), h->stream, P, d_corr, d_pcg); return 1; }
    unsigned launch_pcg_step1(double* x, unsigned pub) { asmb::launch(k_pcg_step1, dim3(1), dim3(1024), h->stream, P, d_sres, d_pcg, x, pub); return 1; }
    unsigned launch_pcg_step2() { asmb::launch(k_pcg_step2, dim3(1), dim3(1024), h->stream, P, d_corr, d_pcg); return 1; }
    unsigned launch_dir(const IpmDir& D) { const unsigned g = grid_all(); asmb::launch(k_ipm_dir, dim3(g), dim3(256), h->stream, P, D, d_tN); return g; }
    unsigned launch_steps(const IpmDir& D, unsigned pub) { const unsigned g = red_grid(); asmb::launch(k_ipm_steps, dim3(g), dim3(1024), h->stream, P, D, pub); return g; }
    unsigned launch_muaff(const IpmDir& A_, int sexp) { const unsigned g = red_grid(); asmb::launch(k_ipm_muaff, dim3(g), dim3(1024), h->stream, P, A_, sexp); return g; }
    unsigned launch_diradd(const IpmDir& D, const IpmDir& E) { const unsigned g = grid_all(); asmb::launch(k_ipm_diradd, dim3(g), dim3(256), h->stream, P, D, E); return g; }
    unsigned launch_update(const IpmDir& C, double al, double be) { const unsigned g = grid_all(); asmb::launch(k_ipm_update, dim3(g), dim3(256), h->stream, P, C, al, be); return g; }
    // best-iterate snapshot: dir 0 saves the iterate (and e, the null-space form's component, when given), 1 brings it back
    unsigned launch_snapshot(double* e, int dir) {
        const unsigned g = grid_all();
        asmb::launch(k_ipm_snapshot, dim3(g), dim3(256), h->stream, P, arena.snap, e, arena.ln, arena.lm, arena.ls, dir);
        return g;
    }
    unsigned launch_col_prep(double rho_p, double fixed, double* dinv, double* th) {
        const unsigned g = grid_all();
        asmb::launch(k_ipm_col_prep, dim3(g), dim3(256), h->stream, P, rho_p, fixed, dinv, th);
        return g;
    }
    unsigned launch_col_scale(const double* dinv, const double* r, double* u) { const dim3 g = asmb::blocks(lp.M); asmb::launch(k_col_scale, g, dim3(256), h->stream, dinv, r, u, lp.M); return g.x; }
    unsigned launch_col_finish(const double* dinv, const double* u, const double* w, double* out) {
        const dim3 g = asmb::blocks(lp.M);
        asmb::launch(k_col_finish, g, dim3(256), h->stream, dinv, u, w, out, lp.M);
        return g.x;
    }
    unsigned launch_red_gather(const int* idx, int cnt, const double* in, double* out) { const dim3 g = asmb::blocks(cnt); asmb::launch(k_red_gather, g, dim3(256), h->stream, idx, cnt, in, out); return g.x; }
    unsigned launch_red_scatter(const int* idx, int cnt, const double* ze, const int* didx, int ndrop, const double* ddrop, const double* in, double* out, int64_t len) {
        const dim3 g = asmb::blocks(len);
        asmb::launch(k_red_scatter, g, dim3(256), h->stream, idx, cnt, ze, didx, ndrop, ddrop, in, out);
        return g.x;
    }
    void up(const double* dst, const vec& v) {
        if (!v.empty()) HIPCHK(asmb::copy_async((void*)dst, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    void down(vec& v, const double* src, int64_t cnt) {
        v.resize(cnt);
        if (cnt) HIPCHK(asmb::copy_async(v.data(), src, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    // push the (scaled) LP data of `lp` to the device
    void ipm_upload_lp() {
        ipm_bind();
        P.n = lp.n; P.M = lp.M; P.ns = lp.ns; P.scale_q = lp.scale_q;
        if (!asmb::in_fiber() && sk().h_up) {
            // seven vectors as three copies from pinned staging (q | lb | ub and w | slo | scoef are neighbours in the arena): a copy from a
            // pageable std::vector is staged by the runtime and blocks the host for tens of microseconds each, twice per LP
            const int64_t ln = sk().ldn, lm = sk().Mp, ls = sk().nsp;
            double* st = sk().h_up;
            std::memcpy(st, lp.q.data(), lp.n * sizeof(double));
            std::memcpy(st + ln, lp.lb.data(), lp.n * sizeof(double));
            std::memcpy(st + 2 * ln, lp.ub.data(), lp.n * sizeof(double));
            std::memcpy(st + 3 * ln, lp.r.data(), lp.M * sizeof(double));
            HIPCHK(asmb::copy_async((void*)P.q, st, 3 * ln * sizeof(double), hipMemcpyHostToDevice, h->stream));
            HIPCHK(asmb::copy_async((void*)P.r, st + 3 * ln, lp.M * sizeof(double), hipMemcpyHostToDevice, h->stream));
            if (lp.ns) {
                double* ss = st + 3 * ln + lm;
                std::memcpy(ss, lp.w.data(), lp.ns * sizeof(double));
                std::memcpy(ss + ls, lp.slo.data(), lp.ns * sizeof(double));
                std::memcpy(ss + 2 * ls, sk().scoef.data(), lp.ns * sizeof(double));
                HIPCHK(asmb::copy_async((void*)P.w, ss, 3 * ls * sizeof(double), hipMemcpyHostToDevice, h->stream));
            }
            h2d_done(h);
            return;
        }
        up(P.q, lp.q); up(P.lb, lp.lb); up(P.ub, lp.ub); up(P.r, lp.r);
        up(P.w, lp.w); up(P.slo, lp.slo);
        vec sc(sk().scoef.begin(), sk().scoef.begin() + lp.ns);
        up(P.scoef, sc);
        h2d_done(h);
    }
    unsigned grid_all() const { return (unsigned)((std::max(std::max(lp.n, lp.M), std::max<int64_t>(lp.ns, 1)) + 255) / 256); }
    // The scalar block of the last reduction kernel on the host.  pub != 0: that kernel stored the block into host-mapped memory
    // and then the sequence word; spin on the word (the stream is in order: everything before that kernel has finished too).
    void read_scal(unsigned pub) {
        if (pub == 0) {
            HIPCHK(asmb::copy_async(sk().h_scal, P.scal, SC_COUNT * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(asmb::sync(h->stream));
            return;
        }
        if (asmb::in_fiber()) {      // scenario batch: the publishing kernel is recorded; the round that launches it ends before this fiber resumes
            asmb::flush_wait();
            if (__atomic_load_n(sk().h_seq, __ATOMIC_ACQUIRE) != pub) throw HipError("read_scal: the batch round ended without the publishing kernel's sequence word");
            return;
        }
        // hot spin for the common case (the kernel is next on an otherwise idle stream: 6.7 us), then yield, then sleep: with several
        // solver threads per process (scenario batches) the kernel may be queued behind other streams' work for milliseconds, and a
        // spinning thread would burn the CPU share the launching threads need
        const double t0 = now_ms();
        for (unsigned long spins = 1;; ++spins) {
            if (__atomic_load_n(sk().h_seq, __ATOMIC_ACQUIRE) == pub) return;
            if (spins < 20000) __builtin_ia32_pause();
            else if (spins < 20200) sched_yield();
            else { struct timespec ts = {0, 20000}; nanosleep(&ts, nullptr); }
            if (((spins < 20200 && (spins & 0xfffff) == 0) || (spins >= 20200 && (spins & 0x3ff) == 0)) && now_ms() - t0 > 30000.0) {
                HIPCHK(asmb::sync(h->stream));            // a device fault surfaces here
                if (__atomic_load_n(sk().h_seq, __ATOMIC_ACQUIRE) == pub) return;
                throw HipError("read_scal: the publishing kernel finished without setting its sequence word");
            }
        }
    }

    void ipm_init() {
        const int64_t n = lp.n, M = lp.M;
        IpmState fresh;
        ip = fresh;
        int64_t nfree = 0, nineq = 0;
        for (int64_t i = 0; i < M; ++i) nineq += lp.rtype[i] != 0;
        for (int64_t j = 0; j < n; ++j) nfree += lp.ub[j] > lp.lb[j];
        ip.ncomp = std::max<int64_t>(2 * nfree + lp.ns + nineq, 1);
        ip.usable[(int)NewtonForm::ReducedRow] = M >= RED_MIN_M && sk().sp_ok;
        ip.usable[(int)NewtonForm::NullSpace] = ns_lp && lp.ns == 0;      // basis made by solve_scaled before the warm attempt
        ip.ns_k = ns_k;
        ip.usable[(int)NewtonForm::Column] = sk().col_capable && lp.ns > 0 && M >= COL_MIN_M && (double)n <= COL_MAX_RATIO * (double)M;   // every row owns a slack (setup)
        ipm_upload_lp();
        P.ncomp = ip.ncomp;
        launch_init_p(lp.ns == 0 ? 1 : 0);
        dev.gemv_n_dev(sk().d_Ah, P.p, P.act);
        launch_init_rest(lp.ns == 0 ? IPM_MU0_NORMAL : 1.0);
    }

    void ipm_measures() {
        dev.gemv_n_dev(sk().d_Ah, P.p, P.act);
        dev.gemv_t_dev(sk().d_Ah, P.y, P.aty);
        const unsigned pub = pub_next(h);
        if (ns_live()) {
            // null-space form: the equality rows' multipliers are carried as 0, the dual residual that counts is Z'rdp (oracle: IPM.measures)
            launch_measures(0u);
            launch_ns_zt(P.rdp, nsv(12), ip.ns_k);
            launch_ns_dinf(nsv(12), ip.ns_k, pub);
        } else {
            launch_measures(pub);
        }
        read_scal(pub);
        ip.pinf = sk().h_scal[SC_PINF];
        ip.dinf = sk().h_scal[SC_DINF];
        ip.mu = sk().h_scal[SC_MU];
        ip.gap = ip.mu / lp.scale_q;
        ip.ymax = sk().h_scal[SC_YMAX];
        ip.rpmax = sk().h_scal[SC_RPMAX];
    }

    // rigorous primal-infeasibility certificate test (oracle: farkas_margin)
    double farkas_margin(const vec& y) {
        double ymax = 0.0;
        for (double v : y) ymax = std::max(ymax, std::fabs(v));
        ymax = std::max(ymax, 1e-300);
        vec yn(lp.M), rho;
        for (int64_t i = 0; i < lp.M; ++i) yn[i] = y[i] / ymax;
        atv(yn, rho);
        double cmax = -1.0, sl = 0.0;
        for (int64_t k = 0; k < lp.ns; ++k) {
            double coef = lp.scoef[k] * yn[lp.srow[k]];
            cmax = std::max(cmax, coef);
            sl += coef * lp.slo[k];
        }
        if (lp.ns && cmax > 1e-12) return -INF;
        double lhs = sl, ynr = 0.0;
        for (int64_t j = 0; j < lp.n; ++j) lhs += std::max(rho[j] * lp.lb[j], rho[j] * lp.ub[j]);
        for (int64_t i = 0; i < lp.M; ++i) ynr += yn[i] * lp.r[i];
        return ynr - lhs;
    }

    // ------------------------------------------------------------ null-space form (oracle: class NullSpace / IPM.run, null-space branch)
    bool ns_was_cold = false;
    bool ns_lp = false;       // this LP has a valid null-space basis (set up before the warm attempt: the active-set solves use it too)
    int ns_k = 0;
    SolveHint* cur_hint = nullptr;
    // non-owning view of the buffers of a null-space iteration: the form's (ns_bind()), or buffers of a test hook's with the pitches of NsLayout
    struct NsArena {
        double *v = nullptr, *th = nullptr, *G = nullptr, *N0 = nullptr, *partial = nullptr;      // work vectors, theta~, Gt, unregularised N, scratch of Zt' u
        const FacBuf* fN = nullptr;
        const int *sp_ptr = nullptr, *sp_col = nullptr, *sc_ptr = nullptr, *sc_row = nullptr, *sc_pos = nullptr;
        const double* vals = nullptr;     // values of the sparse pattern; null: the handle's gathered copy of Ah (Dev::sparse_vals)
        NsIdx X = {nullptr, nullptr, nullptr, nullptr, 0, 0};
        NsLayout L{0, 0, 0, 0};           // pitches, and the offsets of the work vectors in v (nsv)
    } ns_ar;
    // bound once per LP, like the interior-point arena: at the start of ns_setup (the k-sized buffers may be missing) and again after ns_reserve
    void ns_bind() {
        const NsForm& F = *sk().nsf;
        NsArena a;
        a.v = F.v; a.th = F.th; a.partial = sk().d_partial;
        if (F.k) { a.G = F.k->G; a.N0 = F.k->N0; a.fN = &F.k->fN; }
        a.sp_ptr = sk().d_sp_ptr; a.sp_col = sk().d_sp_col; a.sc_ptr = sk().d_sc_ptr; a.sc_row = sk().d_sc_row; a.sc_pos = sk().d_sc_pos;
        a.X = NsIdx{F.Eidx, F.Epos, F.Iidx, F.Ipos, (int)F.L.nE, (int)F.L.nI}; a.L = F.L;
        ns_bind(a);
    }
    void ns_bind(const NsArena& a) { ns_ar = a; }
    const NsArena& nsa() const { return ns_ar; }
    NsIdx nsX() const { return nsa().X; }
    const double* ns_vals() { const NsArena& a = nsa(); return a.vals ? a.vals : dev.sparse_vals(sk().d_Ah); }
    int ns_count_big(const FacBuf& f, int order) {      // dropped pivots of the factor just made in f
        int v = 0;
        asmb::launch(k_ns_count_big, dim3(1), dim3(1024), h->stream, f.S, f.ld, order, NS_BIG, sk().nsf->cnt);
        HIPCHK(asmb::copy_async(&v, sk().nsf->cnt, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(asmb::sync(h->stream));
        return v;
    }
    // buffers sized by the null-space dimension: right-hand-side blocks R, X (k x nEp), Gt = [Zt | GI'] (k x ldg), the k x k factor
    void ns_reserve(int k) {
        NsForm& F = *sk().nsf;
        if (F.k && k <= F.k->cap) return;
        if (F.k) {
            // the null space grew beyond what the first LP of the form reserved (fewer fixed columns than then): the k-sized buffers are
            // released and re-made; the carried basis goes with them
            if (h->knobs.verbose) std::fprintf(stderr, "[asm] null-space form: dimension %d exceeds the reserved %d - buffers re-allocated\n", k, F.k->cap);
            HIPCHK(asmb::sync(h->stream));
            F.k.reset();
        }
        auto K = std::make_unique<NsK>();
        BufPool& P = K->mem;
        const int cap = K->cap = NsLayout::kcap(k);
        P.zeroed(K->R, (int64_t)cap * F.L.nEp, h->stream); P.zeroed(K->X, (int64_t)cap * F.L.nEp, h->stream);
        P.zeroed(K->G, (int64_t)cap * F.L.ldg, h->stream);
        ns_alloc_factor(h, P, K->fN, cap); K->fN.small = true;
        P.zeroed(K->N0, K->fN.ld * K->fN.ld, h->stream);
        P.zeroed(K->Np, NS_MAX_SPLIT * K->fN.ld * K->fN.ld, h->stream);       // split-K slices of the reduced Newton matrix
        P.zeroed(K->ZT, F.L.ldn * K->fN.ld, h->stream);       // transposed copy of the basis rows (right operand of the orthonormalisation product)
        P.alloc(K->J, cap);
        // active-set solves in reduced coordinates: up to 2 cap constraints (an over-determined working set has more than k)
        K->ccap = (int)std::min<int64_t>(2 * cap, F.L.Mp);
        ns_alloc_factor(h, P, K->fC, K->ccap); K->fC.small = true;
        const NsK::Work W = K->work(F.L);
        P.alloc(K->qi, W.ilen); P.zeroed(K->q, W.dlen, h->stream);
        HIPCHK(asmb::sync(h->stream));
        F.k = std::move(K);
    }
    // In place  Zt = L^-1 Zt  with the k x k factor just made in K.fN.  When the factor fits into one wide block the explicit inverse of
    // that block IS L^-1: one transpose + one product on the matrix cores (the rows are n long); otherwise forward substitution per column.
    // (returns the workgroups of k_ns_ortho; 0 on the product branch)
    unsigned ns_ortho(int k) {
        const NsForm& F = *sk().nsf; const NsK& K = *F.k;
        if (k <= K.fN.wb) {
            const int kp = (int)round_up(k, 32);
            asmb::launch(k_transpose_dense, dim3((unsigned)((sk().ldn + 63) / 64), (unsigned)((k + 63) / 64)), dim3(256), h->stream, K.G, F.L.ldg, (int64_t)k, sk().ldn, K.ZT, K.fN.ld, (int64_t)-1);
            dev.gemm_nt(K.fN.Binv, K.fN.wb, K.ZT, K.fN.ld, nullptr, 0, K.G, F.L.ldg, k, (int)sk().ldn, kp, 0);
            return 0;
        }
        const dim3 g = asmb::blocks(sk().ldn);
        asmb::launch(k_ns_ortho, g, dim3(256), h->stream, K.fN.S, K.fN.ld, k, K.G, F.L.ldg, sk().ldn);
        return g.x;
    }
    // The k rows in K.G (an approximate or an outdated basis) projected onto null(A_EF) of THIS LP and orthonormalised with their own
    // Gram matrix (pivot guard `thr`, absolute), then GI' = (A_I Z)'.  Used as the second pass of ns_basis_from and, with the previous
    // LP's basis, as the whole set-up (oracle: NullSpace.__init__, warm_Z).  The factor of S0 must be current in F.f0.
    // head_done: how much of it the side sequence of ns_factor_S0 has made already for these k rows (0 nothing, 1 the right-hand sides in
    // K.R, 2 the forward half of the substitution as well)
    bool ns_reproject(int k, double thr, int head_done = 0) {
        const NsForm& F = *sk().nsf; const NsK& K = *F.k;
        const int nE = (int)F.L.nE, nEp = (int)F.L.nEp;
        const double* vals = dev.sparse_vals(sk().d_Ah);
        // second pass (oracle: NullSpace.basis_from): project the rows once more and orthonormalise with their own Gram matrix (~ I) -
        // the columns picked in index order can be badly conditioned, and the active-set solves need A_EF Z = 0 to 1e-13
        if (head_done < 1) launch_ns_rows_e(vals, k);
        if (head_done < 2)
            for (int B = 0, nB = (nE + F.f0.wb - 1) / F.f0.wb; B < nB; ++B) dev.trsm_rows_fwd_step(F.f0, K.R, K.X, nEp, k, nE, B);
        dev.trsm_rows_bwd(F.f0, K.R, K.X, nEp, k, nE, F.Lt);
        launch_ns_pj(vals, k, 1);
        launch_ns_gram(k);
        if (ns_factor_N(k, thr) > 0) return false;
        ns_ortho(k);
        launch_ns_gi(vals, k);
        return true;
    }
    // the launch sites of the basis set-up (vals = dev.sparse_vals(sk().d_Ah), made by the caller before its first launch); each returns the
    // workgroups of its grid (x)
    unsigned launch_ns_rows_e(const double* vals, int k, hipStream_t on = nullptr) {      // R = (A_EF Zt')' for the k rows in K.G
        const NsForm& F = *sk().nsf; const NsK& K = *F.k;
        const int nEp = (int)F.L.nEp;
        const dim3 g((unsigned)((nEp + 255) / 256), (unsigned)k);
        asmb::launch(k_ns_rows_e, g, dim3(256), on ? on : h->stream, sk().d_sp_ptr, sk().d_sp_col, vals, nsX(), F.Fm, K.G, F.L.ldg, K.R, (int64_t)nEp);
        return g.x;
    }
    unsigned launch_ns_pj(const double* vals, int k, int second_pass) {      // rows of the projector from W = K.R into K.G
        const NsForm& F = *sk().nsf; const NsK& K = *F.k;
        const dim3 g((unsigned)((sk().ldn + 255) / 256), (unsigned)k);
        asmb::launch(k_ns_pj, g, dim3(256), h->stream, sk().d_sc_ptr, sk().d_sc_row, sk().d_sc_pos, vals, nsX(), K.J, F.Fm, K.R, (int64_t)F.L.nEp, K.G, F.L.ldg, lp.n, sk().ldn, second_pass);
        return g.x;
    }
    void launch_ns_gram(int k) {      // lower triangle of Zt Zt' into K.fN.S
        const NsForm& F = *sk().nsf; const NsK& K = *F.k;
        dev.launch_syrk(h->stream, Dev::pick_tile(k), K.G, F.L.ldg, nullptr, 0, k, (int)sk().ldn, nullptr, nullptr, K.fN.S, K.fN.ld, 0, 0);
    }
    int ns_factor_N(int k, double thr) {      // guarded factor of the k x k matrix in K.fN (pivot reference 1); its dropped pivots
        const NsK& K = *sk().nsf->k;
        dev.launch_ns_fill(sk().d_diag0, 1.0, (int64_t)k);
        dev.chol(K.fN, k, thr);
        return ns_count_big(K.fN, k);
    }
    unsigned launch_ns_gi(const double* vals, int k) {      // GI' = (A_I Zt')' beside Zt
        const NsForm& F = *sk().nsf; const NsK& K = *F.k;
        const int nIp = (int)F.L.nIp;
        const dim3 g((unsigned)((nIp + 255) / 256), (unsigned)k);
        asmb::launch(k_ns_gi, g, dim3(256), h->stream, sk().d_sp_ptr, sk().d_sp_col, vals, nsX(), K.G, F.L.ldg, K.G + sk().ldn, nIp);
        return g.x;
    }
    unsigned launch_ns_rhs_cols(const double* vals, const int* J, int nrhs, double* R) {      // columns J (null: all) of A_EF as rows of R
        const NsForm& F = *sk().nsf;
        asmb::launch(k_ns_rhs_cols, dim3((unsigned)nrhs), dim3(256), h->stream, sk().d_sc_ptr, sk().d_sc_row, sk().d_sc_pos, vals, nsX(), J, F.Fm, R, (int64_t)F.L.nEp);
        return (unsigned)nrhs;
    }
    unsigned launch_ns_gather_t(int k) {      // lower triangle of P[J, J] into K.fN.S
        const NsForm& F = *sk().nsf; const NsK& K = *F.k;
        const dim3 g((unsigned)((k + 255) / 256), (unsigned)k);
        asmb::launch(k_ns_gather_t, g, dim3(256), h->stream, K.G, F.L.ldg, K.J, k, K.fN.S, K.fN.ld);
        return g.x;
    }
    unsigned launch_ns_set_diag(const FacBuf& T, int n, const double* dvec) {
        const dim3 g((unsigned)((n + 255) / 256), (unsigned)n);
        asmb::launch(k_ns_set_diag, g, dim3(256), h->stream, T.S, T.ld, n, dvec);
        return g.x;
    }
    unsigned launch_ns_diag(const FacBuf& T, int n, double* out) {
        const dim3 g = asmb::blocks(n);
        asmb::launch(k_ns_diag, g, dim3(256), h->stream, T.S, T.ld, n, out);
        return g.x;
    }
    // Orthonormal basis from the columns J of the projector P (oracle: NullSpace.basis_from): W = S0^-1 A_EF[:, J] by block
    // substitution with all k right-hand sides at once, P[J, :] = E_J' - W' A_EF, L_J L_J' = P[J, J] (guard: pivot <= NS_WARM_THR
    // -> not a basis), Zt = L_J^-1 P[J, :], GI' = (A_I Z)'.  The factor of S0 must be current in F.f0.
    bool ns_basis_from(const std::vector<int>& J) {
        const NsForm& F = *sk().nsf; const NsK& K = *F.k;
        const int k = (int)J.size(), nE = (int)F.L.nE, nEp = (int)F.L.nEp;
        const double* vals = dev.sparse_vals(sk().d_Ah);
        HIPCHK(asmb::copy_async(K.J, J.data(), k * sizeof(int), hipMemcpyHostToDevice, h->stream));
        h2d_done(h);
        launch_ns_rhs_cols(vals, K.J, k, K.R);
        dev.trsm_rows(F.f0, K.R, K.X, nEp, k, nE, F.Lt);
        launch_ns_pj(vals, k, 0);
        launch_ns_gather_t(k);
        if (ns_factor_N(k, NS_WARM_THR) > 0) return false;
        ns_ortho(k);
        return ns_reproject(k, NS_WARM_THR);
    }
    // Per LP (oracle: NullSpace.__init__): factor S0, null-space dimension, basis columns (retained ones, else a guarded Cholesky of
    // P in index order), orthonormal basis.  False: the LP keeps the row form.
    bool ns_setup() {
        ns_bind();
        NsForm& F = *sk().nsf;
        const int nE = (int)F.L.nE;
        const int64_t n = lp.n;
        int64_t nF = 0;
        for (int64_t j = 0; j < n; ++j) nF += lp.ub[j] > lp.lb[j];
        // A banded S0 on the band-panel path with more than one wide block: what does not need the whole factor runs on the side stream beside
        // its factorisation (ns_factor_S0).  Same exclusions as the side stream of the iterations (ns_iter_setup): not in a scenario batch,
        // not under family timing.
        S0Side side{h};
        side.level = (F.f0.band > 0 && dev.band_panels_ok(F.f0, nE) && nE > F.f0.wb && h->stream_ns && !h->batch_slot && !asmb::in_fiber() && h->timing != 2)
                         ? h->knobs.ns_s0side : 0;
        const int dropped = ns_factor_S0(&side);
        // joined here whatever follows: before ns_reserve (it may release the buffers the side sequence wrote), before the first launch that
        // reads the inverses, the transposed copy, K.R or K.X, and before every return (the guard joins when an exception leaves ns_factor_S0)
        side.join();
        ns_dropped = dropped;
        const int64_t k = nF - (nE - dropped);
        if (k < 1 || (double)k > 1.5 * NS_MAX_RATIO * (double)lp.M + 8.0) return false;
        ns_reserve((int)k);
        ns_bind();
        if (!side.level) ns_make_Lt();
        std::vector<int>& J = cur_hint->ns_J;
        bool have = false;
        ns_was_cold = false;
        ns_path = 0;
        ns_vlap("Lt");
        // (the side sequence worked on the Zk rows of the previous basis before k was known: used if k == Zk, scratch that the other paths overwrite if not)
        if (F.k->Zk == (int)k) have = ns_reproject((int)k, NS_ZWARM_THR, side.head_done);      // the previous LP's basis, one projection pass
        ns_vlap("reproject");
        F.k->Zk = 0;
        if (have) ns_path = 1;
        if (!have && (int64_t)J.size() == k) {
            bool free_all = true;
            for (int j : J) free_all = free_all && j >= 0 && j < n && lp.ub[j] > lp.lb[j];
            if (free_all) have = ns_basis_from(J);
            if (have) ns_path = 2;
        }
        if (!have) {
            ns_was_cold = true;
            have = ns_cold_select(k, J);
            if (have) ns_path = 3;
        }
        if (!have) { J.clear(); return false; }
        ns_k = (int)k;
        F.k->Zk = (int)k;
        return true;
    }
    int ns_dropped = 0, ns_path = 0;      // of the last ns_setup: dropped pivots of S0; what made the basis (1 the previous basis, 2 the retained columns, 3 the cold selection, 0 none)
    double ns_tv = 0.0;
    void ns_vlap(const char* what) {      // ASM_HIP_VERBOSE: time since the last lap of the set-up
        if (!h->knobs.verbose) return;
        HIPCHK(asmb::sync(h->stream));
        const double t = now_ms();
        std::fprintf(stderr, "[asm] ns set-up %-10s +%.2f ms\n", what, t - ns_tv);
        ns_tv = t;
    }
    // head of ns_setup: the mask of the free columns from the LP's bounds, S0 and its guarded factor in F.f0; returns its dropped pivots
    //
    // side (ns_setup, level > 0; S0 banded, band-panel path, nB > 1 wide blocks): the work that does not need the whole factor goes to the side
    // stream, beside the latency-bound panel chain that leaves most of the chip empty:
    //   handle's stream:  S0 build, diag_prepare, FORK | panel launch, panel launch, EV_0, panel launch, ... , EV_nB-1 | count + read-back
    //   side stream:      wait FORK, k_ns_rows_e (previous basis, Zk rows -> K.R) | wait EV_B: inverses of wide block B, then (level 2)
    //                     forward step B of the substitution (K.R -> K.X) | ... | transposed copy of the factor, JOIN
    // Hazards.  Columns < I1 of the factor and their 64 x 64 block inverses are final after the panel launch that ends at I1: it applies its
    // whole trailing update itself and later launches write columns >= I1 only - the side sequence reads nothing else of the factor.  A block's
    // inverse launches use that block's BinvT as scratch and end with its transposed copy, in this order on one stream; no other block's is
    // touched.  d_vecM, d_diag0 and the panel flags belong to the chain; the side sequence uses none of them.  k_ns_rows_e reads the sparse
    // values, Fm and K.G: all in place at the fork.  The rows are the PREVIOUS basis' (k is not known before the read-back): ns_setup uses
    // K.R / K.X only if this LP's k equals Zk.  Host order: each panel launch is issued first, then what its event releases - behind a
    // read-back the device follows the host launch by launch (ns_iter_setup).  The join is unconditional once the fork is recorded: nothing
    // of the side sequence is in flight when ns_reserve re-makes the buffers, when K.G is rewritten or when the next LP clears the band.
    // Residency.  k_chol_panel_band needs all its workgroups resident (they wait for each other's flags), and it now shares the chip with the
    // side kernels, the chip-wide k_ns_rows_e beside its first launch among them.  It still makes progress: no side kernel waits for anything
    // of a running panel launch (only for events recorded after finished ones), so every side workgroup ends by itself and frees its slot for
    // the panel workgroups not yet dispatched; the delay is a side kernel's duration (0.3 ms at most) against the bound of the panel waits, 2^22 polls (pnl_wait: hundreds of ms).
    struct S0Side {
        asm_handle* h;
        int level = 0;           // HandleKnobs::ns_s0side, or 0 where the sequence does not apply
        int head_done = 0;       // what ns_reproject finds done for the Zk rows of the previous basis (its head_done)
        bool forked = false, join_recorded = false, joined = false;
        hipEvent_t ev(int i) {      // 0 fork, 1 join, 2 + B wide block B
            while ((int)h->s0_events.size() <= i) {
                hipEvent_t e;
                HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                h->s0_events.push_back(e);
            }
            return h->s0_events[i];
        }
        void fork() { HIPCHK(hipEventRecord(ev(0), h->stream)); forked = true; HIPCHK(hipStreamWaitEvent(h->stream_ns, ev(0), 0)); }
        void record_join() { HIPCHK(hipEventRecord(ev(1), h->stream_ns)); join_recorded = true; }
        void join() {
            if (!forked || joined) return;
            if (!join_recorded) record_join();
            HIPCHK(hipStreamWaitEvent(h->stream, h->s0_events[1], 0));
            joined = true;
        }
        ~S0Side() {      // an exception between fork and join: the handle's stream still waits for what the side stream was given
            if (!forked || joined || h->s0_events.size() < 2) return;
            if (!join_recorded) (void)hipEventRecord(h->s0_events[1], h->stream_ns);
            (void)hipStreamWaitEvent(h->stream, h->s0_events[1], 0);
        }
    };
    int ns_factor_S0(S0Side* side = nullptr) {
        NsForm& F = *sk().nsf;
        const int nE = (int)F.L.nE;
        const int64_t n = lp.n;
        {
            vec own(asmb::in_fiber() ? sk().ldn : 0);
            double* fm = asmb::in_fiber() ? own.data() : sk().h_pin;      // (pinned staging: the copy does not go through the runtime's pageable path)
            for (int64_t j = 0; j < sk().ldn; ++j) fm[j] = (j < n && lp.ub[j] > lp.lb[j]) ? 1.0 : 0.0;
            HIPCHK(asmb::copy_async(F.Fm, fm, sk().ldn * sizeof(double), hipMemcpyHostToDevice, h->stream));
            h2d_done(h);
        }
        ns_tv = now_ms();
        dev.ns_build_S0();
        ns_vlap("S0 build");
        dev.diag_prepare(F.f0, nE, 1, 0.0, 0.0);
        if (!side || !side->level) {
            dev.chol(F.f0, nE, 1e-10);
            ns_vlap("S0 factor");
            return ns_count_big(F.f0, nE);
        }
        hipStream_t ss = h->stream_ns;
        const int nEp = (int)F.L.nEp, nB = (nE + F.f0.wb - 1) / F.f0.wb;
        const int Zk = F.k ? F.k->Zk : 0;      // rows of the previous basis (0: none)
        const double* vals = Zk > 0 ? dev.sparse_vals(sk().d_Ah) : nullptr;
        side->ev(1 + nB);      // (the whole event list before the first launch)
        side->fork();
        int made = 0;          // wide blocks whose side launches are issued
        bool first = true;
        const Dev::PanelDone progress = [&](int, int done) {
            if (first && Zk > 0) launch_ns_rows_e(vals, Zk, ss);
            first = false;
            if (done <= made) return;
            HIPCHK(hipEventRecord(side->ev(2 + done - 1), h->stream));
            HIPCHK(hipStreamWaitEvent(ss, side->ev(2 + done - 1), 0));
            for (; made < done; ++made) {
                dev.trtri_blocks(F.f0, nE, made, made + 1, ss);
                if (side->level >= 2 && Zk > 0) dev.trsm_rows_fwd_step(F.f0, F.k->R, F.k->X, nEp, Zk, nE, made, ss);
            }
        };
        dev.chol(F.f0, nE, 1e-10, true, &progress);
        if (made != nB) throw std::logic_error("ns_factor_S0: the factorisation did not report every wide block");
        ns_make_Lt(ss);
        side->record_join();
        side->head_done = Zk > 0 ? (side->level >= 2 ? 2 : 1) : 0;
        ns_vlap("S0 factor");
        return ns_count_big(F.f0, nE);
    }
    void ns_make_Lt(hipStream_t on = nullptr) {      // transposed copy of the factor of S0 (inside its band)
        NsForm& F = *sk().nsf;
        const int nE = (int)F.L.nE;
        asmb::launch(k_transpose_dense, dim3((unsigned)((nE + 63) / 64), (unsigned)((nE + 63) / 64)), dim3(256), on ? on : h->stream, F.f0.S, F.f0.ld, (int64_t)nE, (int64_t)nE,
                     F.Lt, F.f0.ld, (int64_t)(F.f0.band > 0 ? F.f0.band : nE));
    }
    // the two buffers of the cold selection (ldn rows of nEp each): made by the first LP that needs them
    void ns_cold_buffers() {
        NsForm& F = *sk().nsf;
        const int nEp = (int)F.L.nEp;
        if (!F.Yt) F.mem.zeroed(F.Yt, (int64_t)sk().ldn * nEp + (int64_t)sk().ldn * nEp, h->stream);
    }
    // cold selection: Y = L0^-1 A_EF for ALL columns (forward substitution only), T = I_F - Y'Y in the main factor,
    // guarded Cholesky of T in index order with the absolute thresholds NS_SEL_THR in turn until exactly k columns are kept
    bool ns_cold_select(int64_t k, std::vector<int>& J) {
        NsForm& F = *sk().nsf;
        const int nE = (int)F.L.nE, nEp = (int)F.L.nEp;
        const int64_t n = lp.n;
        bool have = false;
        ns_cold_buffers();
        double* Yr = F.Yt;                                  // right-hand sides, then garbage
        double* Yt = F.Yt + (int64_t)sk().ldn * nEp;   // L0^-1 a_j as rows
        const double* vals = dev.sparse_vals(sk().d_Ah);
        launch_ns_rhs_cols(vals, nullptr, (int)n, Yr);
        dev.trsm_rows(F.f0, Yr, Yt, nEp, (int)n, nE, nullptr);
        std::vector<double> dg(n);
        FacBuf& T = sk().main_fac;
        T.band = 0;
        for (int a = 0; a < 4 && !have; ++a) {
            launch_ns_set_diag(T, (int)n, F.Fm);
            dev.launch_syrk(h->stream, Dev::pick_tile(n), Yt, nEp, nullptr, 0, (int)n, nEp, nullptr, nullptr, T.S, T.ld, 0, 1);
            dev.launch_ns_fill(sk().d_diag0, 1.0, n);
            dev.chol(T, (int)n, NS_SEL_THR[a]);
            launch_ns_diag(T, (int)n, sk().d_vecN);
            HIPCHK(asmb::copy_async(dg.data(), sk().d_vecN, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(asmb::sync(h->stream));
            std::vector<int> Jc;
            for (int64_t j = 0; j < n; ++j)
                if (dg[j] < NS_BIG) Jc.push_back((int)j);
            if ((int64_t)Jc.size() != k) continue;
            if (ns_basis_from(Jc)) { J = Jc; have = true; }
        }
        return have;
    }
    double* nsv(int which) const { return ns_ar.v + ns_ar.L.nsv_off(which); }      // work vectors: 0..4 n-sized, 5..7 M-sized, 8..9 E-sized, 10..13 k-sized (k <= n), 14..15 n-sized (14 = e)
    // oracle: ns_applicable
    bool ns_applicable() const {
        if (!sk().nsf || lp.ns != 0) return false;
        int64_t nE = 0, nF = 0;
        for (int64_t i = 0; i < lp.M; ++i) nE += lp.rtype[i] == 0;
        for (int64_t j = 0; j < lp.n; ++j) nF += lp.ub[j] > lp.lb[j];
        return nE >= NS_MIN_E && (double)(nF - nE) <= NS_MAX_RATIO * (double)lp.M;
    }
    NsEq nsq() const { return sk().nsf->k->work(sk().nsf->L).Q; }
    // dense products with the gathered constraint matrix Csel (nact rows of pitch ldc)
    void nsq_gemv_n(const NsEq& Q, int nact, const double* x, double* out) {
        asmb::launch(k_gemv_n, asmb::blocks(nact, 4), dim3(256), h->stream, Q.Csel, Q.ldc, x, out, (int64_t)nact, Q.ldc);
    }
    void nsq_gemv_t(const NsEq& Q, int nact, const double* y, double* out) {
        int64_t R = std::min<int64_t>((nact + 31) / 32, ASM_TMAXCHUNKS);
        int64_t chunk = (nact + R - 1) / R;
        R = (nact + chunk - 1) / chunk;
        asmb::launch(k_gemv_t_stage1, dim3((unsigned)((Q.ldc + 255) / 256), (unsigned)R), dim3(256), h->stream, Q.Csel, Q.ldc, y, sk().d_partial, (int64_t)nact, Q.ldc, chunk);
        asmb::launch(k_gemv_t_stage2, asmb::blocks(Q.ldc), dim3(256), h->stream, sk().d_partial, out, R, Q.ldc);
    }
    // per LP (oracle: eqp_ns, the part that does not depend on the working set): pbar, A pbar, u0 = Z'(p_ref - pbar), Z'q
    void ns_lp_vectors() {
        const NsForm& F = *sk().nsf; const NsK& K = *F.k;
        const int k = ns_k, nE = (int)F.L.nE;
        const int64_t ldn = sk().ldn;
        const NsIdx X = nsX();
        const NsEq Q = nsq();
        const unsigned gN = (unsigned)((ldn + 255) / 256), gE = (unsigned)((nE + 255) / 256);
        double *pfix = nsv(0), *x = nsv(1), *vz = nsv(2), *yM = nsv(5), *aM = nsv(6), *rE = nsv(8), *tE = nsv(9);
        asmb::launch(k_nseq_pfix, dim3(gN), dim3(256), h->stream, A, pfix, ldn);
        dev.gemv_n_dev(sk().d_Ah, pfix, aM);
        asmb::launch(k_nseq_be, dim3(gE), dim3(256), h->stream, A, X, aM, rE);
        dev.chol_solve_dev(F.f0, rE, tE, nE);
        launch_ns_rowvec_e(tE, yM);
        dev.gemv_t_dev(sk().d_Ah, yM, x);
        asmb::launch(k_nseq_pbar, dim3(gN), dim3(256), h->stream, A, pfix, x, d_zero, Q.pbar, vz, ldn);
        dev.gemv_n_dev(sk().d_Ah, Q.pbar, Q.tbar);
        HIPCHK(asmb::fill_async(Q.u0, 0, 2 * Q.ldc * sizeof(double), h->stream));      // u0 and qh (contiguous)
        gemv_rows((const double*)K.G, F.L.ldg, (const double*)vz, Q.u0, (int64_t)k, ldn);
        gemv_rows((const double*)K.G, F.L.ldg, (const double*)A.q, Q.qh, (int64_t)k, ldn);
    }
    // Equality-constrained solve on the working set `cur` in reduced coordinates (oracle: eqp_ns).  Leaves p, y, t = Ah p, tN = Ah' y
    // for the tail kernel like as_solve.  False: more active constraints than the buffers hold (the caller uses as_solve).
    bool as_solve_ns(const AsSets& cur) {
        const NsForm& F = *sk().nsf; const NsK& K = *F.k;
        const int k = ns_k, nE = (int)F.L.nE;
        const int64_t M = lp.M, n = lp.n, ldn = sk().ldn;
        const NsIdx X = nsX();
        const NsEq Q = nsq();
        const unsigned gM = (unsigned)((M + 255) / 256), gN = (unsigned)((ldn + 255) / 256);
        asmb::launch(k_nseq_setup, dim3(1), dim3(1024), h->stream, A, cur, X, Q, ldn);
        int cnt[2] = {0, 0};
        HIPCHK(asmb::copy_async(cnt, Q.cnt, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(asmb::sync(h->stream));
        const int nact = cnt[1];
        if (nact > NS_CMAX * k || nact > K.ccap) return false;             // oracle: eqp_ns returns None - the polish attempt ends (eqp_loop)
        const unsigned gC = (unsigned)((Q.ldc + 255) / 256), gA = (unsigned)((nact + 255) / 256);
        double *t1 = nsv(12), *t2 = nsv(13);
        HIPCHK(asmb::copy_async(Q.u, Q.u0, Q.ldc * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(asmb::fill_async(Q.lam, 0, (size_t)K.ccap * sizeof(double), h->stream));
        if (nact > 0) {
            asmb::launch(k_nseq_gather, dim3(gC, (unsigned)nact), dim3(256), h->stream, A, cur, X, Q, K.G, F.L.ldg, k, ldn);
            const FacBuf& C = K.fC;
            dev.launch_syrk(h->stream, Dev::pick_tile(nact), Q.Csel, Q.ldc, nullptr, 0, nact, (int)Q.ldc, nullptr, nullptr, C.S, C.ld, 0, 0);
            dev.diag_prepare(C, nact, 1, 0.0, 0.0);
            dev.chol(C, nact, 1e-10, false);
            for (int sw = 0; sw < 3; ++sw) {
                nsq_gemv_n(Q, nact, Q.u, Q.v);                                                                           // C u
                asmb::launch(k_nseq_sub, dim3(gA), dim3(256), h->stream, Q.d, Q.v, Q.v, (int64_t)nact);
                dev.chol_solve_dev(C, Q.v, Q.w, nact);
                nsq_gemv_t(Q, nact, Q.w, t1);
                launch_ns_add(Q.u, t1, Q.u, Q.ldc);
                nsq_gemv_t(Q, nact, Q.lam, t1);                                                                          // C' lam
                asmb::launch(k_nseq_sub, dim3(gC), dim3(256), h->stream, Q.qh, t1, t2, Q.ldc);
                nsq_gemv_n(Q, nact, t2, Q.v);
                dev.chol_solve_dev(C, Q.v, Q.w, nact);
                launch_ns_add(Q.lam, Q.w, Q.lam, (int64_t)nact);
            }
        }
        double *zu = nsv(3), *atw = nsv(4), *wN = nsv(2), *yM = nsv(5), *aM = nsv(6), *rE = nsv(8), *tE = nsv(9);
        ns_gemv_t_dense(Q.u, k, zu);
        asmb::launch(k_nseq_p, asmb::blocks(n), dim3(256), h->stream, A, cur, Q, zu, ldn);
        asmb::launch(k_nseq_yi, dim3(gM), dim3(256), h->stream, A, X, Q, yM);
        dev.gemv_t_dev(sk().d_Ah, yM, atw);
        asmb::launch(k_nseq_w, dim3(gN), dim3(256), h->stream, A, Q, atw, wN, ldn);
        dev.gemv_n_dev(sk().d_Ah, wN, aM);
        launch_ns_gather_e(aM, 1.0, rE);
        dev.chol_solve_dev(F.f0, rE, tE, nE);
        asmb::launch(k_nseq_y, dim3(gM), dim3(256), h->stream, A, X, yM, tE);
        dev.gemv_n_dev(sk().d_Ah, A.p, A.t);
        dev.gemv_t_dev(sk().d_Ah, A.y, A.tN);
        h->stats.eqp += 1;
        return true;
    }
    bool usable(NewtonForm f) const { return ip.usable[(int)f]; }      // (NullSpace, Column, ReducedRow)
    bool ns_live() const { return usable(NewtonForm::NullSpace); }
    // least-squares multipliers of the equality rows for the current iterate (oracle: IPM.ns_finish_y); P.rdp is the dual residual of the last
    // measures (with the equality multipliers as they stand: 0, or the values recovered at the end of the previous stage)
    void ns_finish_y() {
        const NsForm& F = *sk().nsf;
        const int nE = (int)F.L.nE;
        double *aM = nsv(6), *rE = nsv(8), *tE = nsv(9);
        dev.gemv_n_dev(sk().d_Ah, P.rdp, aM);
        launch_ns_gather_e(aM, 1.0, rE);
        dev.chol_solve_dev(F.f0, rE, tE, nE);
        // P.rdp already contains -A_E'y_E of the multipliers recovered at the end of an earlier stage: the solve gives the correction
        launch_ns_scatter_e(tE, P.y, 1);
    }
    // ---- launch sites of the kernels of a null-space iteration (asm_ns_kernels.hip.h): the solver and the test hook asm_test_ns_stages launch
    // through these members only; each carries its launch's grid and returns the number of workgroups it launched
    unsigned launch_theta_ns(double rho_p) {
        const NsArena& a = nsa();
        const unsigned g = std::max(grid_all(), (unsigned)((std::max<int64_t>(a.L.ldn, a.L.nIp) + 255) / 256));
        asmb::launch(k_ipm_theta_ns, dim3(g), dim3(256), h->stream, P, rho_p, a.X, a.th, a.L.ldn, (int)a.L.nIp);
        return g;
    }
    unsigned launch_ns_update(const IpmDir& C, double al, double be, double es) {
        const unsigned g = grid_all();
        asmb::launch(k_ns_update, dim3(g), dim3(256), h->stream, P, C, al, be, nsv(14), es, nsa().L.ldn);
        return g;
    }
    unsigned launch_ns_update_dev(const IpmDir& C, double eta, double rerr) {
        const unsigned g = grid_all();
        asmb::launch(k_ns_update_dev, dim3(g), dim3(256), h->stream, P, C, eta, nsv(14), nsa().L.ldn, rerr);
        return g;
    }
    unsigned launch_ns_dinf(const double* zr, int k, unsigned pub) { asmb::launch(k_ns_dinf, dim3(1), dim3(1024), h->stream, P, zr, k, pub); return 1; }
    // out[k] = Zt x   (x of ldn entries)
    unsigned launch_ns_zt(const double* x, double* out, int k, hipStream_t on = nullptr) { const NsArena& a = nsa(); return gemv_rows((const double*)a.G, a.L.ldg, x, out, (int64_t)k, a.L.ldn, on); }
    unsigned launch_ns_e0(const double* pbar, double* d0) {
        const NsArena& a = nsa();
        const unsigned gN = (unsigned)((a.L.ldn + 255) / 256);
        asmb::launch(k_ns_e0, dim3(gN), dim3(256), h->stream, P, pbar, d0, a.L.ldn);
        return gN;
    }
    unsigned launch_ns_e1(const double* d0, const double* zz, double* e) {
        const NsArena& a = nsa();
        const unsigned gN = (unsigned)((a.L.ldn + 255) / 256);
        asmb::launch(k_ns_e1, dim3(gN), dim3(256), h->stream, P, d0, zz, e, a.L.ldn);
        return gN;
    }
    // dpbar = -e, SC_NSERR = 0, yM = D_I^-1 (Ah dpbar)
    unsigned launch_ns_spmvn_wm_neg(const double* vals, hipStream_t on = nullptr) {
        const NsArena& a = nsa();
        const unsigned gM = (unsigned)((lp.M + 255) / 256), gN = (unsigned)((a.L.ldn + 255) / 256), g = std::max(gM, gN);
        asmb::launch(k_ns_spmvn_wm_neg, dim3(g), dim3(256), on ? on : h->stream, a.sp_ptr, a.sp_col, vals, nsv(14), nsv(0), a.L.ldn, P.scal + SC_NSERR, a.X, (const double*)(a.th + a.L.ldn), nsv(5), lp.M);
        return g;
    }
    // K dpbar = Th dpbar + Ah' yM
    unsigned launch_ns_spmvt_kx(const double* vals, hipStream_t on = nullptr) {
        const NsArena& a = nsa();
        const dim3 g = asmb::blocks(a.L.ldn * 8);
        asmb::launch(k_ns_spmvt_kx, g, dim3(256), on ? on : h->stream, a.sc_ptr, a.sc_row, a.sc_pos, vals, nsv(5), (const double*)a.th, nsv(0), nsv(1), lp.n, a.L.ldn);
        return g.x;
    }
    unsigned launch_ns_rhs1_bi(const IpmDir& base, int mode, double res, hipStream_t on = nullptr) {
        const NsArena& a = nsa();
        const unsigned g = grid_all();
        asmb::launch(k_ns_rhs1_bi, dim3(g), dim3(256), on ? on : h->stream, P, base, mode, a.X, (const double*)(a.th + a.L.ldn), res, nsv(7), nsv(5));
        return g;
    }
    unsigned launch_ns_spmvt_ht(const double* vals, double res, hipStream_t on = nullptr) {
        const NsArena& a = nsa();
        const dim3 g = asmb::blocks(a.L.ldn * 8);
        asmb::launch(k_ns_spmvt_ht, g, dim3(256), on ? on : h->stream, a.sc_ptr, a.sc_row, a.sc_pos, vals, nsv(5), (const double*)a.th, P.hp, nsv(1), res, nsv(2), nsv(3), lp.n, a.L.ldn);
        return g.x;
    }
    unsigned launch_ns_reduced_solve(int k, const double* ru, double* du) {
        const NsArena& a = nsa();
        asmb::launch(k_ns_reduced_solve, dim3(1), dim3(1024), h->stream, a.fN->S, a.fN->ld, a.fN->Linv, a.N0, k, ru, du, P.scal + SC_NSERR);
        return 1;
    }
    unsigned launch_ns_symv_res(int k, const double* x, const double* rhs, double* out) {
        const NsArena& a = nsa();
        const dim3 g = asmb::blocks(k, 4);
        asmb::launch(k_ns_symv_res, g, dim3(256), h->stream, a.N0, a.fN->ld, k, x, rhs, out);
        return g.x;
    }
    unsigned launch_ns_add(const double* a_, const double* b_, double* x, int64_t len) {
        const unsigned g = (unsigned)((len + 255) / 256);
        asmb::launch(k_ns_add, dim3(g), dim3(256), h->stream, a_, b_, x, len);
        return g;
    }
    unsigned launch_ns_relres(const double* r, const double* rhs, int k) { asmb::launch(k_ns_relres, dim3(1), dim3(1024), h->stream, r, rhs, k, P.scal + SC_NSERR); return 1; }
    unsigned launch_ns_gemv_t_small_dp(int k, const double* du, const IpmDir& D, double res) {
        const NsArena& a = nsa();
        const unsigned gN = (unsigned)((a.L.ldn + 255) / 256);
        asmb::launch(k_gemv_t_small_dp, dim3(gN), dim3(256), h->stream, a.G, a.L.ldg, k, du, P, D, (const double*)a.th, nsv(0), res, a.L.ldn);
        return gN;
    }
    unsigned launch_ns_dp(const IpmDir& D, double res, const double* zu) {
        const NsArena& a = nsa();
        const unsigned gN = (unsigned)((a.L.ldn + 255) / 256);
        asmb::launch(k_ns_dp, dim3(gN), dim3(256), h->stream, P, D, (const double*)a.th, nsv(0), res, zu, a.L.ldn);
        return gN;
    }
    unsigned launch_ns_spmvn_rows(const double* vals, const IpmDir& D) {
        const NsArena& a = nsa();
        const unsigned gM = (unsigned)((lp.M + 255) / 256);
        asmb::launch(k_ns_spmvn_rows, dim3(gM), dim3(256), h->stream, a.sp_ptr, a.sp_col, vals, P, D, a.X, (const double*)(a.th + a.L.ldn), nsv(7), nsv(5));
        return gM;
    }
    unsigned launch_ns_gather_e(const double* r, double scale, double* out) {
        const NsIdx X = nsX();
        const unsigned gE = (unsigned)((X.nE + 255) / 256);
        asmb::launch(k_ns_gather_e, dim3(gE), dim3(256), h->stream, X, r, scale, out);
        return gE;
    }
    unsigned launch_ns_scatter_e(const double* tE, double* out, int add) {
        const NsIdx X = nsX();
        const unsigned gE = (unsigned)((X.nE + 255) / 256);
        asmb::launch(k_ns_scatter_e, dim3(gE), dim3(256), h->stream, X, tE, out, add);
        return gE;
    }
    unsigned launch_ns_rowvec_e(const double* tE, double* yM) {
        const unsigned gM = (unsigned)((lp.M + 255) / 256);
        asmb::launch(k_ns_rowvec_e, dim3(gM), dim3(256), h->stream, nsX(), tE, yM, lp.M);
        return gM;
    }
    // Per iteration (oracle: IPM.run, null-space branch): reduced matrix N = Zt Th Zt' + GI' D_I^-1 GI (an unregularised copy is kept for the
    // refinement sweep), its factor, dpbar = A_EF' S0^-1 (-rp_E) and K dpbar (shared by predictor and corrector)
    void ns_iter_setup() {
        const NsForm& F = *sk().nsf; const NsK& K = *F.k;
        const int k = ip.ns_k;
        // (theta~ was formed with the interior-point theta: k_ipm_theta_ns in ipm_run)
        // the k range (free columns + inequality rows, 19 000 at n = 11 192) is long and the matrix small (k = 519: 45 tiles of 64 x 64):
        // split-K fills the chip; the slices are added in a fixed order while the unregularised copy N0 is made
        // (measured at k = 519, k range 19 000: 32 x 32 tiles x 8 slices 1.19 ms per iteration, 64 x 64 x 8 1.21, 32 x 32 x 4 1.21, unsplit 1.40)
        const int T = Dev::pick_tile(k);
        const int64_t ntile = ((k + 32 * T - 1) / (32 * T));
        int nsplit = (int)std::min<int64_t>(NS_MAX_SPLIT, std::max<int64_t>(1, 1224 / std::max<int64_t>(1, ntile * (ntile + 1) / 2)));
        nsplit = (int)std::min<int64_t>(nsplit, std::max<int64_t>(1, F.L.ldg / 512));
        // The head of the iteration - dpbar, K dpbar and the affine solve's right-hand sides down to ru - reads the iterate, theta~ and the sparse
        // values only and writes work vectors 0, 1, 2, 3, 5, 7, 10, the complementarity right-hand sides and SC_NSERR; the build and the
        // factorisation write Np, the factor with its inverses, N0, d_diag0 and the panel flags.  Nothing is shared: the head runs on the side
        // stream beside them (the chip is nearly empty during the factorisation) and ns_newton(0) joins it before its first reduced solve.
        // Not in a scenario batch (a slot records for one stream) and not under family timing (events of one stream).
        ns_head_side = h->knobs.ns_side && h->stream_ns && !h->batch_slot && !asmb::in_fiber() && h->timing != 2;
        const double* vals = ns_vals();
        if (ns_head_side) {
            ns_split_e_once(k);      // (e is read by the head)
            if (!h->ns_fork) {
                HIPCHK(hipEventCreateWithFlags(&h->ns_fork, hipEventDisableTiming));
                HIPCHK(hipEventCreateWithFlags(&h->ns_join, hipEventDisableTiming));
            }
            HIPCHK(hipEventRecord(h->ns_fork, h->stream));
        }
        dev.ns_newton_matrix(K.G, F.L.ldg, F.th, k, nsplit, K.Np, K.fN, K.N0, sk().d_diag0, 1e-13, 1e-30);
        dev.chol(K.fN, k, 1e-14, false);
        if (ns_head_side) {
            // issued AFTER the build and the factorisation: behind a read-back the device follows the host launch by launch, and five launches
            // issued first kept the build waiting for the host (traced: k_syrk started 57 us after k_ipm_theta_ns instead of 6)
            HIPCHK(hipStreamWaitEvent(h->stream_ns, h->ns_fork, 0));
            launch_ns_spmvn_wm_neg(vals, h->stream_ns);
            launch_ns_spmvt_kx(vals, h->stream_ns);
            ns_newton_head(0, dirA, vals, h->stream_ns);
            HIPCHK(hipEventRecord(h->ns_join, h->stream_ns));
            return;
        }
        ns_split_e_once(k);
        // (fused launches: negation + clearing of the residual measure; sparse product + its row- / column-wise kernel)
        launch_ns_spmvn_wm_neg(vals);
        launch_ns_spmvt_kx(vals);
    }
    bool ns_head_side = false;      // this iteration's head went to the side stream: ns_newton(0) joins it instead of launching its own
    // dpbar = -e: the component of the iterate outside pbar + null(A_EF), split off once per LP and shrunk by (1 - a) with every step
    void ns_split_e_once(int k) {
        if (ip.ns_e_ready) return;
        ip.ns_e_ready = true;
        ns_split_e(k, nsq().pbar);
    }
    // e = (I - Z Zt) Fm (p - pbar)  (work vectors: d0 = 2, Z Zt d0 = 3, Zt d0 = 12, e = 14)
    void ns_split_e(int k, const double* pbar) {
        double *d0 = nsv(2), *zz = nsv(3), *tk = nsv(12);
        launch_ns_e0(pbar, d0);
        launch_ns_zt(d0, tk, k);
        ns_gemv_t_dense(tk, k, zz);
        launch_ns_e1(d0, zz, nsv(14));
    }
    // One Newton solve in null-space form (oracle: IPM.run, solve_ns): mode 0 affine, 1 Mehrotra corrector on `base`.  The relative residual of
    // the reduced solve (after its refinement sweep) is accumulated in SC_NSERR.
    // Work vectors: dpbar = 0, K dpbar = 1, h~ = 2, v = 3, yM = 5, bI = 7, ru = 10, du = 11, rr = 12, dd = 13.
    // head_issued: ns_iter_setup has put the three launches of the head (ns_newton_head) on the side stream - the handle's stream waits for them here
    void ns_newton(int mode, const IpmDir& base, IpmDir& D, bool head_issued = false) {
        const int k = ip.ns_k;
        const double res = 1.0;
        const double* vals = ns_vals();
        if (head_issued) HIPCHK(hipStreamWaitEvent(h->stream, h->ns_join, 0));
        else ns_newton_head(mode, base, vals, nullptr);
        ns_reduced_solve(k);
        ns_direction(k, D, res);
        launch_ns_spmvn_rows(vals, D);
    }
    // the right-hand sides of a Newton solve down to ru = Zt v: nothing here reads the factor (`on`: the stream of the launches; null: the handle's)
    void ns_newton_head(int mode, const IpmDir& base, const double* vals, hipStream_t on) {
        const double res = 1.0;
        launch_ns_rhs1_bi(base, mode, res, on);
        launch_ns_spmvt_ht(vals, res, on);
        launch_ns_zt(nsv(3), nsv(10), ip.ns_k, on);
    }
    // du = N^-1 ru with one refinement sweep on the unregularised N0; SC_NSERR = max(SC_NSERR, relative residual)
    unsigned ns_reduced_solve(int k) {
        double *ru = nsv(10), *du = nsv(11), *rr = nsv(12), *dd = nsv(13);
        // solve, refinement sweep on the unregularised matrix and the residual check in ONE one-workgroup launch
        if (k <= ASM_SMALL_USE) return launch_ns_reduced_solve(k, ru, du);
        const FacBuf& fN = *nsa().fN;
        dev.chol_solve_dev(fN, ru, du, k);
        const unsigned g = launch_ns_symv_res(k, du, ru, rr);
        dev.chol_solve_add_dev(fN, rr, dd, du, k);      // dd = N^-1 rr, du += dd
        launch_ns_symv_res(k, du, ru, rr);
        launch_ns_relres(rr, ru, k);
        return g;
    }
    // dp = res dpbar + Z du with the bound multipliers' directions
    unsigned ns_direction(int k, const IpmDir& D, double res) {
        double *v = nsv(3), *du = nsv(11);
        if (k <= ASM_SMALL_USE) return launch_ns_gemv_t_small_dp(k, du, D, res);
        if (h->knobs.ns_fold) return ns_gemv_t_dense(du, k, v, &D, res);      // k_ns_dp inside the second stage of the product
        ns_gemv_t_dense(du, k, v);
        return launch_ns_dp(D, res, v);
    }
    // out[n] = Zt' u   (Zt dense, k rows of pitch ldg).  dp_of != null (k above ASM_SMALL_USE): the second stage also forms that direction's dp
    // and bound multipliers from its sums (k_gemv_t_stage2_dp, on launch_ns_dp's grid - the grid returned)
    unsigned ns_gemv_t_dense(const double* u, int k, double* out, const IpmDir* dp_of = nullptr, double res = 1.0) {
        const NsArena& a = nsa();
        if (k <= ASM_SMALL_USE) {
            const dim3 g = asmb::blocks(a.L.ldn);
            asmb::launch(k_gemv_t_small, g, dim3(256), h->stream, a.G, a.L.ldg, k, u, out, a.L.ldn);
            return g.x;
        }
        int64_t R = std::min<int64_t>((k + 31) / 32, ASM_TMAXCHUNKS);
        int64_t chunk = (k + R - 1) / R;
        R = (k + chunk - 1) / chunk;
        const unsigned gx = (unsigned)((a.L.ldn + 255) / 256);
        asmb::launch(k_gemv_t_stage1, dim3(gx, (unsigned)R), dim3(256), h->stream, a.G, a.L.ldg, u, a.partial, (int64_t)k, a.L.ldn, chunk);
        if (dp_of) {
            asmb::launch(k_gemv_t_stage2_dp, dim3(gx), dim3(256), h->stream, a.partial, out, R, P, *dp_of, (const double*)a.th, nsv(0), res, a.L.ldn);
            return gx;
        }
        asmb::launch(k_gemv_t_stage2, asmb::blocks(a.L.ldn), dim3(256), h->stream, a.partial, out, R, a.L.ldn);
        return gx * (unsigned)R;
    }

    NewtonForm form = NewtonForm::Row;      // form of the current factorisation
    // reduced row form: the rows kept in the factor (in the order of the factorisations) and the rows left to a diagonal preconditioner,
    // chosen from host copies of the slack terms dS and of the Schur diagonal
    struct ReducedRows {
        std::vector<int> kept, diag;
        vec dS, sdiag;
    } red;
    int cg_max = 0;           // most CG steps any solve of the current iteration needed
    bool cg_fail = false;     // a solve of the current iteration left its CG loop without reaching the tolerance
    // out = in through the main factor of a row (column) list: gather in[idx[0:cnt]], solve, scatter back; k_red_scatter gives the
    // ndrop rows didx outside the list out = in / ddrop (pure permutations: none).  The scatter covers `len` rows.
    void solve_list(const int* idx, int cnt, const int* didx, int ndrop, const double* ddrop, const double* in, double* out, int64_t len) {
        launch_red_gather(idx, cnt, in, sk().d_rce);
        dev.chol_solve_dev(sk().main_fac, sk().d_rce, sk().d_rze, cnt);
        launch_red_scatter(idx, cnt, sk().d_rze, didx, ndrop, ddrop, in, out, len);
    }
    // out = (approximate) S^-1 in : the Cholesky factor of S (row forms) or Sherman-Morrison-Woodbury through the factor of K (column form)
    void precond(const double* in, double* out) {
        const int M = (int)lp.M, n = (int)lp.n;
        switch (form) {
        case NewtonForm::ReducedRow:
            solve_list(sk().d_idx, (int)red.kept.size(), sk().d_idxI, (int)red.diag.size(), sk().d_rdI, in, out, M);
            return;
        case NewtonForm::BandedRow:      // rows in the handle's banded order
            solve_list(sk().d_rowperm, M, sk().d_rowperm, 0, sk().d_rze, in, out, M);
            return;
        case NewtonForm::Column:
            launch_col_scale(sk().d_cdinv, in, sk().d_cu);                                                                 // u = D^-1 r
            dev.gemv_t_dev(sk().d_Ah, sk().d_cu, sk().d_ct);                                                                 // Ah' u
            if (sk().col_band > 0) solve_list(sk().d_colperm, n, sk().d_colperm, 0, sk().d_rze, sk().d_ct, sk().d_cv, n);         // K^-1 (columns in banded order)
            else dev.chol_solve_dev(sk().main_fac, sk().d_ct, sk().d_cv, n);                                                 // K^-1
            dev.gemv_n_dev(sk().d_Ah, sk().d_cv, sk().d_cw);                                                                 // Ah v
            launch_col_finish(sk().d_cdinv, sk().d_cu, sk().d_cw, out);
            return;
        default:      // Row (the null-space form solves in ns_newton)
            dev.chol_solve_dev(sk().main_fac, in, out, M);
        }
    }
    // one Newton solve with the current factor (oracle: IPM.run.solve); mode 0 affine, 1 Mehrotra corrector built on
    // `base`, 2 Gondzio centrality corrector for `base` at the trial steps (tp, td)
    // spec = 0: as the oracle states it.  spec = 1 / 2 (first / later solve of an iteration, only with the factor of S itself as preconditioner):
    // the residual check is not waited for - its verdict travels in scal[SC_SPEC] with the next block the iteration reads (ipm_run redoes the
    // iteration's solves with spec = 0 when one of them missed its tolerance: one host round trip per solve less in the common case).
    void ipm_solve(int mode, const IpmDir& base, IpmDir& D, double tp = 0.0, double td = 0.0, int spec = 0) {
        launch_rhs1(base, mode, tp, td);
        dev.gemv_n_dev(sk().d_Ah, P.tmpn, P.t1);
        launch_rhs2(mode == 2 ? 0.0 : 1.0);
        precond(P.rhs, D.dy);
        if (spec) {
            dev.gemv_t_dev(sk().d_Ah, D.dy, d_tN);
            launch_vec_mul(d_tN, P.thp_inv, lp.n);
            dev.gemv_n_dev(sk().d_Ah, d_tN, d_sres);
            launch_res(D.dy, 0u, spec, 1e-10, PCG_KAPPA * ip.rpmax);
        } else {
            // preconditioned CG on the unregularised Schur system, the Cholesky factor as preconditioner (oracle: IPM.run.solve).
            // The residual of this system is exactly the primal residual the step leaves behind, hence the tolerance.
            auto applyS = [&](const double* v) {          // d_sres = Ah Th^-1 Ah' v
                dev.gemv_t_dev(sk().d_Ah, v, d_tN);
                launch_vec_mul(d_tN, P.thp_inv, lp.n);
                dev.gemv_n_dev(sk().d_Ah, d_tN, d_sres);
            };
            applyS(D.dy);
            unsigned pub = pub_next(h);
            launch_res(D.dy, pub, 0, 0.0, 0.0);
            read_scal(pub);
            // the approximate preconditioners (column and reduced row form) get the tighter floor (oracle: IPM.run.solve)
            const bool approx = form == NewtonForm::Column || form == NewtonForm::ReducedRow;
            const double tol = std::max((approx ? 1e-13 : 1e-10) * sk().h_scal[SC_RMAX], PCG_KAPPA * ip.rpmax);
            if (sk().h_scal[SC_EMAX] > tol) {
                precond(P.res, d_corr);
                launch_pcg_start();
                bool converged = false;
                for (int it = 0; it < PCG_MAXIT; ++it) {
                    applyS(d_pcg);
                    pub = pub_next(h);
                    launch_pcg_step1(D.dy, pub);
                    read_scal(pub);
                    h->stats_pcg += 1;
                    cg_max = std::max(cg_max, it + 1);
                    if (sk().h_scal[SC_STOP] != 0.0) break;
                    if (sk().h_scal[SC_EMAX] <= tol) { converged = true; break; }
                    precond(P.res, d_corr);
                    launch_pcg_step2();
                }
                if (!converged) cg_fail = true;
            }
        }
        dev.gemv_t_dev(sk().d_Ah, D.dy, d_tN);
        launch_dir(D);
    }

    // reduced row form (oracle: IPM.run): inequality rows whose slack term dominates their Schur diagonal stay out of the factor and get a
    // diagonal preconditioner.  Reads both vectors back.  False: too few such rows, or no row left for the factor.
    bool red_select() {
        dev.schur_diag(P.thp_inv, sk().d_sdiag);
        down(red.dS, P.dS, lp.M);
        down(red.sdiag, sk().d_sdiag, lp.M);
        HIPCHK(asmb::sync(h->stream));
        red.kept.clear(); red.diag.clear();
        for (int64_t q = 0; q < lp.M; ++q) {                 // kept rows in the order of the factorisations
            const int64_t i = sk().row_band > 0 ? sk().row_perm_h[q] : q;
            if (red.dS[i] > RED_TAU * red.sdiag[i]) red.diag.push_back((int)i);
            else red.kept.push_back((int)i);
        }
        return (double)red.diag.size() >= RED_MIN_FRAC * (double)lp.M && !red.kept.empty();
    }
    // the form of this iteration's Newton system, first usable in the order of NewtonForm (oracle: IPM.run)
    NewtonForm choose_form() {
        if (usable(NewtonForm::NullSpace)) return NewtonForm::NullSpace;
        if (usable(NewtonForm::Column)) return NewtonForm::Column;
        if (usable(NewtonForm::ReducedRow) && red_select()) return NewtonForm::ReducedRow;
        return sk().row_band > 0 ? NewtonForm::BandedRow : NewtonForm::Row;
    }
    // The Newton matrix of the current form and its factor (oracle: IPM.run).  Column form: K = Th + Ah' D^-1 Ah (n x n) while its
    // Sherman-Morrison-Woodbury preconditioner keeps the CG short; row forms: S = Ah Th^-1 Ah' + D (kept rows, or M x M); all three in
    // the main factor, whose band is that of the handle's column or row order (0: none).
    void newton_factor() {
        if (form == NewtonForm::NullSpace) {      // null-space form (oracle: IPM.run): set up once per LP, k x k factorisation per iteration
            ip.ns_iters += 1;
            ns_iter_setup();
            return;
        }
        const int M = (int)lp.M, n = (int)lp.n;
        FacBuf& f = sk().main_fac;
        f.band = form == NewtonForm::Column ? sk().col_band : sk().row_band;
        int dim = M;
        switch (form) {
        case NewtonForm::Column:
            ip.col_iters += 1;
            dim = n;
            launch_col_prep(IPM_RHO_P, COL_FIXED, sk().d_cdinv, sk().d_cth);
            if (sk().col_band > 0) {
                // columns in their banded order: K built from the structural column pairs, factor and substitutions stop at the band
                launch_red_gather(sk().d_colperm, (int)lp.n, sk().d_cth, sk().d_diag);
                dev.schur_banded_cols_dev(sk().d_cdinv, sk().d_diag);
            } else {
                dev.schur_syrk(true, nullptr, n, sk().d_cdinv, sk().d_cth, f.S, f.ld, Dev::NzFlags::Pattern);
            }
            break;
        case NewtonForm::ReducedRow: {
            // the kept rows with their slack terms; the others' diagonal (Schur diagonal + slack term) for the preconditioner
            dim = (int)red.kept.size();
            const int nd = (int)red.diag.size();
            vec dE_(dim), dI_(nd);
            for (int a = 0; a < dim; ++a) dE_[a] = red.dS[red.kept[a]];
            for (int b = 0; b < nd; ++b) dI_[b] = red.sdiag[red.diag[b]] + red.dS[red.diag[b]];
            HIPCHK(asmb::copy_async(sk().d_idx, red.kept.data(), dim * sizeof(int), hipMemcpyHostToDevice, h->stream));
            HIPCHK(asmb::copy_async(sk().d_idxI, red.diag.data(), nd * sizeof(int), hipMemcpyHostToDevice, h->stream));
            HIPCHK(asmb::copy_async(sk().d_diag, dE_.data(), dim * sizeof(double), hipMemcpyHostToDevice, h->stream));
            HIPCHK(asmb::copy_async(sk().d_rdI, dI_.data(), nd * sizeof(double), hipMemcpyHostToDevice, h->stream));
            std::vector<int> cp;
            if (sk().row_band > 0) {      // place of every row in the list (-1: not in it)
                cp.assign(lp.M, -1);
                for (int a = 0; a < dim; ++a) cp[red.kept[a]] = a;
                HIPCHK(asmb::copy_async(sk().d_cpos, cp.data(), lp.M * sizeof(int), hipMemcpyHostToDevice, h->stream));
            }
            h2d_done(h);      // the host vectors go out of scope
            dev.schur_rows(sk().d_idx, sk().d_cpos, dim, P.thp_inv, sk().d_diag);
            break;
        }
        case NewtonForm::BandedRow:
            // full row form, rows in the banded order: S is built entry by entry, factor and substitutions stop at the band
            launch_red_gather(sk().d_rowperm, M, P.dS, sk().d_diag);
            dev.schur_banded_dev(sk().d_rowpos, M, P.thp_inv, sk().d_diag);
            break;
        default:      // Row
            dev.schur_syrk(false, nullptr, M, P.thp_inv, P.dS, f.S, f.ld, Dev::NzFlags::Pattern);
        }
        dev.diag_prepare(f, dim, 0, 1e-13, 1e-30);
        dev.chol(f, dim);
    }
    // A form that lost its accuracy (or whose preconditioner needs too many CG steps) is not used again in this LP: the next iteration -
    // this one again when its step was not applied - takes the next usable form (oracle: IPM.run).  The null-space form first recovers
    // the equality rows' multipliers.
    void drop_form(NewtonForm f) {
        if (f == NewtonForm::NullSpace) ns_finish_y();
        ip.usable[(int)f] = false;
    }

    int btag = 100;      // alignment tags of a scenario batch grow in program order inside one LP (asm_batch.hip.h)
    int ipm_run(double tol, int max_more) {
        int done = 0;
        // null-space iterations apply their step on the device (k_ns_update_dev) and are checked with the NEXT measures: one read-back per
        // iteration.  ns_pending: the last iteration was one of those and its accuracy check is still owed
        const bool ns_defer = h->knobs.ns_defer;
        bool ns_pending = false;
        while (true) {
            asmb::barrier(btag);                 // scenario batch: iterations of different scenarios run in lockstep (min-PC-first)
            ipm_measures();
            if (ns_pending) {
                ns_pending = false;
                if (h->knobs.verbose) std::fprintf(stderr, "[asm]     ap %.3e ad %.3e (null-space step, applied on the device)\n", sk().h_scal[SC_AP], sk().h_scal[SC_AD]);
                if (sk().h_scal[SC_NSERR] > h->knobs.ns_rerr) {
                    // the reduced system lost its accuracy and the device left the iterate alone: redo the iteration in row form
                    // (oracle: IPM.run) - measured again below as the row form measures it
                    drop_form(NewtonForm::NullSpace);
                    continue;
                }
            }
            if (h->knobs.verbose) std::fprintf(stderr, "[asm] ipm %3d pinf %.3e dinf %.3e gap %.3e\n", ip.iters, ip.pinf, ip.dinf, ip.gap);
            if (ip.pinf <= tol && ip.gap <= tol && (ip.dinf <= tol || (ip.gap <= IPM_GAP_DONE * tol && ip.dinf <= IPM_DINF_FLOOR))) {
                if (ns_live()) ns_finish_y();
                return ip.status = ASM_OPTIMAL;
            }
            if (ip.iters >= 3 && ip.ymax > 1e3 * lp.scale_q) {
                if (ns_live()) ns_finish_y();
                vec y;
                down(y, P.y, lp.M);
                HIPCHK(asmb::sync(h->stream));
                if (farkas_margin(y) > 1e-9) return ip.status = ASM_INFEASIBLE;
            }
            if (done >= max_more) { if (ns_live()) ns_finish_y(); return ip.status = ASM_OTHER; }
            // jammed: complementarity collapsed but the primal residual no longer decreases (oracle: IPM.run)
            ip.pinf_hist.push_back(ip.pinf);
            if (ip.iters >= 10 && ip.pinf > JAM_PINF && ip.gap <= 1e-2 * ip.pinf && ip.pinf > 0.5 * ip.pinf_hist[ip.pinf_hist.size() - 4]) {
                if (ns_live()) ns_finish_y();
                return ip.status = ASM_OTHER;
            }
            if (ns_live())      // null-space form: its theta~ in the same launch (ns_iter_setup)
                launch_theta_ns(IPM_RHO_P);
            else
                launch_theta(IPM_RHO_P);
            form = choose_form();
            newton_factor();
            const bool ns = form == NewtonForm::NullSpace;
            ip.iters += 1;
            done += 1;
            double ap = 0.0, ad = 0.0;
            // the solves of the iteration; deferred = the residual checks of the solves are not waited for one by one (ipm_solve, spec):
            // false when one of them missed its tolerance - the solves are then redone as the oracle states them (same iterate, same
            // factor: every vector they write is written again)
            auto solves = [&](const bool deferred) -> bool {
                cg_max = 0;
                cg_fail = false;
                if (ns) ns_newton(0, dirA, dirA, ns_head_side); else ipm_solve(0, dirA, dirA, 0.0, 0.0, deferred ? 1 : 0);
                launch_steps(dirA, 0u);
                launch_muaff(dirA, IPM_SIG_EXP);
                if (ns) ns_newton(1, dirA, dirC); else ipm_solve(1, dirA, dirC, 0.0, 0.0, deferred ? 2 : 0);
                if (ns && ns_defer) {       // step lengths stay on the device (k_ns_update_dev below)
                    launch_steps(dirC, 0u);
                    return true;
                }
                unsigned pub = pub_next(h);
                launch_steps(dirC, pub);
                read_scal(pub);
                if (deferred && sk().h_scal[SC_SPEC] != 0.0) return false;
                ap = sk().h_scal[SC_AP]; ad = sk().h_scal[SC_AD];
                // Gondzio multiple centrality correctors (oracle: IPM.run): dirA is free again and receives the candidate
                for (int kc = 0; kc < (ns ? 0 : IPM_MCC); ++kc) {      // (no correctors in null-space form: a Newton solve costs more than the factorisation there)
                    if (std::min(ap, ad) >= 0.9) break;
                    const double tp = std::min(1.0, ap + MCC_DELTA), td = std::min(1.0, ad + MCC_DELTA);
                    ipm_solve(2, dirC, dirA, tp, td, deferred ? 2 : 0);
                    launch_diradd(dirA, dirC);
                    pub = pub_next(h);
                    launch_steps(dirA, pub);
                    read_scal(pub);
                    if (deferred && sk().h_scal[SC_SPEC] != 0.0) return false;
                    const double ap2 = sk().h_scal[SC_AP], ad2 = sk().h_scal[SC_AD];
                    if (!(ap2 >= ap && ad2 >= ad && ap2 + ad2 >= ap + ad + MCC_GAMMA * MCC_DELTA)) break;
                    std::swap(dirA, dirC);
                    ap = ap2; ad = ad2;
                }
                return true;
            };
            const bool approx = form == NewtonForm::Column || form == NewtonForm::ReducedRow;
            const bool defer = !ns && !approx;      // the factor of S itself is the preconditioner
            if (!(defer && solves(true))) solves(false);
            const double eta = ip.mu >= 1.0 ? IPM_ETA0 : std::min(std::max(IPM_ETA0, 1.0 - ip.mu / lp.scale_q), 0.999999);
            if (ns && ns_defer) {
                launch_ns_update_dev(dirC, eta, h->knobs.ns_rerr);
                ns_pending = true;
                continue;
            }
            if (h->knobs.verbose) std::fprintf(stderr, "[asm]     ap %.3e ad %.3e  cg steps so far %lld\n", ap, ad, (long long)h->stats_pcg);
            // the reduced system lost its accuracy, or the preconditioner of the column / reduced row form did: redo the iteration in the
            // next form (oracle: IPM.run)
            if (ns ? sk().h_scal[SC_NSERR] > h->knobs.ns_rerr : approx && cg_fail) {
                drop_form(form);
                continue;
            }
            if (ns)
                launch_ns_update(dirC, std::min(1.0, eta * ap), std::min(1.0, eta * ad), 1.0 - std::min(1.0, eta * ap));
            else
                launch_update(dirC, std::min(1.0, eta * ap), std::min(1.0, eta * ad));
            if (approx && cg_max > (form == NewtonForm::Column ? COL_MAX_CG : RED_MAX_CG)) drop_form(form);
        }
    }

    // ---------------------------------------------------------------- active-set machinery (device resident)
    // The working sets, index lists and every O(M+n) vector of the equality-constrained solves live in HBM
    // (asm_as_kernels.hip.h); the host reads back one block of counters / scalars after the set-up kernel (the size of the
    // gathered Schur system fixes the launch grids) and one after the tail kernel of a solve.
    struct EqpOut {
        vec p, s, y, act, z;   // act = Ah p + E s ; z = q - Ah' y
    };
    AsPtrs A;
    AsSets S_[6];              // 0..2: rotation of the correction loop; 3: partition of the iterate; 4: primal working set; 5: dual
    double *d_pref = nullptr, *d_zero = nullptr;
    double *d_p0 = nullptr, *d_s0 = nullptr, *d_y0 = nullptr, *d_act0 = nullptr, *d_z0 = nullptr;      // projection of the iterate
    double *d_pa = nullptr, *d_sa = nullptr, *d_acta = nullptr;                                          // anchor of the primal method
    double *d_pf = nullptr, *d_sf = nullptr, *d_actf = nullptr, *d_yf = nullptr, *d_zf = nullptr;       // least-norm point (scratch) / multipliers
    int final_sets = 0;
    int as_nH = 0, as_nF = 0;

    // where the active-set state lives: the handle's arenas (as_bind()), or buffers of a test hook's with the pitches of an AsLayout
    struct AsArena {
        double* base = nullptr;       // AsLayout::dbl_len() doubles
        int* ibase = nullptr;         // AsLayout::int_len() ints
        const int* rperm = nullptr;   // the row order of the factorisations, or null
        int64_t ln = 0, lm = 0, ls = 0;
    } as_arena;
    void as_bind() {
        AsArena a;
        a.base = sk().d_as; a.ibase = sk().d_as_i; a.rperm = sk().row_band > 0 ? sk().d_rowperm : nullptr;
        a.ln = sk().ldn; a.lm = sk().Mp; a.ls = sk().nsp;
        as_bind(a);
    }
    // the ONLY place that lays the two arenas out (the LP vectors are those of the interior-point arena: ipm_bind comes first)
    void as_bind(const AsArena& ar) {
        as_arena = ar;
        const int64_t ln = ar.ln, lm = ar.lm, ls = ar.ls;
        double* a = ar.base;
        auto N = [&]() { double* r_ = a; a += ln; return r_; };
        auto Mv = [&]() { double* r_ = a; a += lm; return r_; };
        auto Sv = [&]() { double* r_ = a; a += ls; return r_; };
        A.q = P.q; A.lb = P.lb; A.ub = P.ub; A.r = P.r; A.w = P.w; A.slo = P.slo; A.scoef = P.scoef;
        A.rtype = P.rtype; A.srow = P.srow; A.rs0 = P.rs0; A.rs1 = P.rs1;
        A.n = lp.n; A.M = lp.M; A.ns = lp.ns; A.scale_q = lp.scale_q;
        A.Fmask = N(); A.p = N(); A.z = N(); A.pB = N(); A.pF = N(); A.cF = N(); A.rd = N(); A.tN = N(); A.xfull = N(); A.nu = N();
        d_pref = N(); d_zero = N(); d_p0 = N(); d_z0 = N(); d_pa = N(); d_pf = N(); d_zf = N();
        A.Hmask = Mv(); A.sl = Mv(); A.y = Mv(); A.act = Mv(); A.t = Mv(); A.bH = Mv(); A.v = Mv(); A.u = Mv(); A.yH = Mv();
        A.yfull = Mv(); A.uacc = Mv(); A.ax = Mv();
        d_y0 = Mv(); d_act0 = Mv(); d_acta = Mv(); d_actf = Mv(); d_yf = Mv();
        A.s = Sv(); d_s0 = Sv(); d_sa = Sv(); d_sf = Sv();
        A.scal = a;
        int* ia = ar.ibase;
        auto Ni = [&]() { int* r_ = ia; ia += ln; return r_; };
        auto Mi = [&]() { int* r_ = ia; ia += lm; return r_; };
        auto Si = [&]() { int* r_ = ia; ia += ls; return r_; };
        for (int k = 0; k < 6; ++k) { S_[k].rowst = Mi(); S_[k].bst = Ni(); S_[k].sst = Si(); }
        A.ksoft = Mi(); A.Hidx = Mi(); A.hpos = Mi(); A.Fidx = Ni(); A.fpos = Ni();
        A.rperm = ar.rperm;
        A.cnt = ia;
    }
    // ---- launch sites of the active-set kernels (asm_as_kernels.hip.h): the solver and the test hook asm_test_as_stages launch through these
    // members only; each returns the number of workgroups it launched
    unsigned as_grid_m1() const { return (unsigned)((lp.M + 255) / 256 + 1); }
    unsigned as_grid_n() const { return (unsigned)((lp.n + 255) / 256); }
    unsigned launch_as_sl() { const unsigned g = as_grid_m1(); asmb::launch(k_as_sl, dim3(g), dim3(256), h->stream, A); return g; }
    unsigned launch_as_sl_values() { const unsigned g = as_grid_m1(); asmb::launch(k_as_sl_values, dim3(g), dim3(256), h->stream, A); return g; }
    unsigned launch_as_clip0(const double* src, double* out) { const dim3 g = asmb::blocks(lp.n); asmb::launch(k_as_clip0, g, dim3(256), h->stream, A.lb, A.ub, src, out, lp.n); return g.x; }
    unsigned launch_as_smax(const double* src, double* dst) { const dim3 g = asmb::blocks(lp.ns); asmb::launch(k_as_smax, g, dim3(256), h->stream, src, A.slo, dst, lp.ns); return g.x; }
    unsigned launch_as_copy_sets(const AsSets& dst, const AsSets& src) {
        const unsigned g = grid_all();
        asmb::launch(k_as_copy_sets, dim3(g), dim3(256), h->stream, dst, src, lp.M, lp.n, lp.ns);
        return g;
    }
    unsigned launch_as_pack(const AsSets& S, double* dst) {
        const unsigned g = grid_all();
        asmb::launch(k_as_pack, dim3(g), dim3(256), h->stream, A.p, A.z, A.y, A.act, A.s, S, lp.n, lp.M, lp.ns, dst);
        return g;
    }
    unsigned launch_as_identify(const AsSets& S) { const unsigned g = grid_all(); asmb::launch(k_as_identify, dim3(g), dim3(256), h->stream, P, S); return g; }
    unsigned launch_as_setup(const AsSets& cur, const double* p_ref) {
        asmb::launch(k_as_setup, dim3(1), dim3(1024), h->stream, A, cur, p_ref, as_arena.ln, as_arena.lm);
        return 1;
    }
    unsigned launch_as_rhs(const double* y_ref) { const unsigned g = grid_all(); asmb::launch(k_as_rhs, dim3(g), dim3(256), h->stream, A, y_ref); return g; }
    // (grids over the nH hard rows: the count the host read back after k_as_setup)
    unsigned launch_as_res_p(int nH) { const dim3 g = asmb::blocks(nH); asmb::launch(k_as_res_p, g, dim3(256), h->stream, A); return g.x; }
    unsigned launch_as_gather_h(int nH) { const dim3 g = asmb::blocks(nH); asmb::launch(k_as_gather_h, g, dim3(256), h->stream, A); return g.x; }
    unsigned launch_as_add_yh(int nH) { const dim3 g = asmb::blocks(nH); asmb::launch(k_as_add_yh, g, dim3(256), h->stream, A); return g.x; }
    unsigned launch_as_scatter_h(const double* src, int accumulate) {
        const unsigned g = as_grid_m1();
        asmb::launch(k_as_scatter_h, dim3(g), dim3(256), h->stream, A, src, accumulate);
        return g;
    }
    unsigned launch_as_add_f() { const unsigned g = as_grid_n(); asmb::launch(k_as_add_f, dim3(g), dim3(256), h->stream, A); return g; }
    unsigned launch_as_rd() { const unsigned g = as_grid_n(); asmb::launch(k_as_rd, dim3(g), dim3(256), h->stream, A); return g; }
    unsigned launch_as_merge(int with_y) { const unsigned g = grid_all(); asmb::launch(k_as_merge, dim3(g), dim3(256), h->stream, A, with_y); return g; }
    unsigned launch_as_finish(const AsSets& cur, const AsSets& nx, const AsSets& prev, int have_prev, double tol_p, double tol_d) {
        asmb::launch(k_as_finish, dim3(1), dim3(1024), h->stream, A, cur, nx, prev, have_prev, tol_p, tol_d);
        return 1;
    }
    unsigned launch_face_primal_finish(const AsSets& W, const AsSets& part, double tol_p, double tol_m, int check_only) {
        asmb::launch(k_face_primal_finish, dim3(1), dim3(1024), h->stream, A, W, part, tol_p, tol_m, check_only);
        return 1;
    }
    unsigned launch_face_ns_combine(const double* p0, const double* Zbuf, int64_t ldz, const double* u, int k, double* p) {
        const unsigned g = as_grid_n();
        asmb::launch(k_face_ns_combine, dim3(g), dim3(256), h->stream, p0, Zbuf, ldz, u, k, p, lp.n);
        return g;
    }
    unsigned launch_face_ns_step(const AsSets& W, double* pa, double* sa, double* acta, double tol_p) {
        asmb::launch(k_face_ns_step, dim3(1), dim3(1024), h->stream, A, W, pa, sa, acta, tol_p);
        return 1;
    }
    unsigned launch_face_ns_unmark(const AsSets& W, int fam, int64_t e) { asmb::launch(k_face_ns_unmark, dim3(1), dim3(64), h->stream, A, W, fam, e); return 1; }
    unsigned launch_face_ns_col(const double* Ah, int64_t ld, int fam, int64_t e, const double* p0, const double* t0) {
        asmb::launch(k_face_ns_col, dim3(1), dim3(1024), h->stream, A, Ah, ld, fam, e, p0, t0);
        return 1;
    }
    unsigned launch_face_ns_z(double* z) { const unsigned g = as_grid_n(); asmb::launch(k_face_ns_z, dim3(g), dim3(256), h->stream, A, z); return g; }
    unsigned launch_face_dual_finish(const AsSets& D, double tol_m) { asmb::launch(k_face_dual_finish, dim3(1), dim3(1024), h->stream, A, D, tol_m); return 1; }
    unsigned launch_face_kkt(const AsSets& D) { asmb::launch(k_face_kkt, dim3(1), dim3(1024), h->stream, A, D); return 1; }
    // per LP: reference point of the unique-optimum polish (0 clipped into the box), slack offsets of the rows
    void as_begin_lp() {
        as_bind();
        launch_as_sl();
        launch_as_clip0(nullptr, d_zero);
    }
    void as_read() {
        HIPCHK(asmb::copy_async(sk().h_ascnt, A.cnt, AC_COUNT * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(asmb::copy_async(sk().h_asscal, A.scal, AS_COUNT * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(asmb::sync(h->stream));
    }
    void as_copy_sets(int dst, int src) {
        launch_as_copy_sets(S_[dst], S_[src]);
    }
    void as_upload_sets(const ActiveSet& as, int dst) {
        std::vector<int> buf((size_t)(lp.M + lp.n + lp.ns));
        for (int64_t i = 0; i < lp.M; ++i) buf[i] = as.rowst[i];
        for (int64_t j = 0; j < lp.n; ++j) buf[lp.M + j] = as.bst[j];
        for (int64_t k = 0; k < lp.ns; ++k) buf[lp.M + lp.n + k] = as.sst[k];
        if (lp.M) HIPCHK(asmb::copy_async(S_[dst].rowst, buf.data(), lp.M * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(asmb::copy_async(S_[dst].bst, buf.data() + lp.M, lp.n * sizeof(int), hipMemcpyHostToDevice, h->stream));
        if (lp.ns) HIPCHK(asmb::copy_async(S_[dst].sst, buf.data() + lp.M + lp.n, lp.ns * sizeof(int), hipMemcpyHostToDevice, h->stream));
        h2d_done(h);
    }
    void dcopy(double* dst, const double* src, int64_t cnt) {
        if (cnt > 0) HIPCHK(asmb::copy_async(dst, src, cnt * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    }
    // final answer of the LP (device -> host): p, s, y, z, act and the working set `final_sets`
    void as_download(EqpOut& o, ActiveSet& as) {
        const int64_t n = lp.n, M = lp.M, ns = lp.ns;
        if (!asmb::in_fiber() && sk().d_dl) {
            // outside a batch: packed on the device, one copy into pinned memory (eight copies into pageable vectors cost the host tens of
            // microseconds each, with the GPU idle in between)
            launch_as_pack(S_[final_sets], sk().d_dl);
            const size_t bytes = (size_t)(2 * n + 2 * M + ns) * sizeof(double) + (size_t)(M + n + ns) * sizeof(int);
            HIPCHK(asmb::copy_async(sk().h_dl, sk().d_dl, bytes, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(asmb::sync(h->stream));
            const double* st = sk().h_dl;
            o.p.assign(st, st + n); o.z.assign(st + n, st + 2 * n); o.y.assign(st + 2 * n, st + 2 * n + M); o.act.assign(st + 2 * n + M, st + 2 * n + 2 * M);
            o.s.assign(st + 2 * n + 2 * M, st + 2 * n + 2 * M + ns);
            const int* bi = reinterpret_cast<const int*>(st + 2 * n + 2 * M + ns);
            as.rowst.resize(M); as.bst.resize(n); as.sst.resize(ns);
            for (int64_t i = 0; i < M; ++i) as.rowst[i] = (int8_t)bi[i];
            for (int64_t j = 0; j < n; ++j) as.bst[j] = (int8_t)bi[M + j];
            for (int64_t k = 0; k < ns; ++k) as.sst[k] = (int8_t)bi[M + n + k];
            as.valid = true;
            return;
        }
        down(o.p, A.p, n); down(o.z, A.z, n); down(o.y, A.y, M); down(o.act, A.act, M); down(o.s, A.s, ns);
        std::vector<int> buf((size_t)(M + n + ns));
        if (M) HIPCHK(asmb::copy_async(buf.data(), S_[final_sets].rowst, M * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(asmb::copy_async(buf.data() + M, S_[final_sets].bst, n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        if (ns) HIPCHK(asmb::copy_async(buf.data() + M + n, S_[final_sets].sst, ns * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(asmb::sync(h->stream));
        as.rowst.resize(M); as.bst.resize(n); as.sst.resize(ns);
        for (int64_t i = 0; i < M; ++i) as.rowst[i] = (int8_t)buf[i];
        for (int64_t j = 0; j < n; ++j) as.bst[j] = (int8_t)buf[M + j];
        for (int64_t k = 0; k < ns; ++k) as.sst[k] = (int8_t)buf[M + n + k];
        as.valid = true;
    }
    void identify_dev(int dst) {
        launch_as_identify(S_[dst]);
    }

    // Equality-constrained solve on the working set `cur` (oracle: eqp / _face_primal_solve / face_dual's solve).
    //   mode 0: both projections from (p_ref, y_ref), 4 refinement sweeps              (eqp)
    //   mode 1: primal least-norm point only (p_ref = 0), 3 sweeps, the multipliers of that problem accumulated in uacc
    //   mode 2: basic least-squares multipliers only (y_ref = 0), 4 sweeps
    // Leaves t = Ah p and tN = Ah' y (mode 1: tN = Ah' u_full) for the tail kernel.
    bool part_factor = false;   // the main factor is the factor of the partition's Schur matrix (face_polish re-uses it for the rounds on the same sets)
    void as_solve(const AsSets& cur, const double* p_ref, const double* y_ref, int mode, bool reuse_factor = false) {
        launch_as_setup(cur, p_ref);
        HIPCHK(asmb::copy_async(sk().h_ascnt, A.cnt, AC_COUNT * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(asmb::sync(h->stream));
        const int nH = sk().h_ascnt[AC_NH], nF = sk().h_ascnt[AC_NF];
        const bool any_soft = sk().h_ascnt[AC_ANYSOFT] != 0;
        as_nH = nH; as_nF = nF;
        if (nH > 0) {
            dev.gemv_n_dev(sk().d_Ah, A.pB, A.t);
            if (any_soft) dev.gemv_t_dev(sk().d_Ah, A.y, A.tN);
            launch_as_rhs(y_ref);
        }
        if (nH > 0 && nF > 0) {
            if (!(reuse_factor && part_factor)) {
                sk().main_fac.band = sk().row_band;
                dev.schur_rows(A.Hidx, A.hpos, nH, A.Fmask, nullptr);        // (Hidx is in the banded row order when there is one: k_as_setup)
                dev.diag_prepare(sk().main_fac, nH, 1, 0.0, 0.0);
                dev.chol(sk().main_fac, nH, 1e-10);
                part_factor = false;
            }
            const int sweeps = mode == 1 ? 3 : 4;
            for (int it = 0; it < sweeps; ++it) {
                if (mode != 2) {
                    dev.gemv_n_dev(sk().d_Ah, A.pF, A.t);                                                  // A_HF pF
                    launch_as_res_p(nH);
                    dev.chol_solve_dev(sk().main_fac, A.v, A.u, nH);
                    launch_as_scatter_h(A.u, mode == 1 ? 1 : 0);
                    dev.gemv_t_dev(sk().d_Ah, A.yfull, A.tN);                                              // A_HF' u
                    launch_as_add_f();
                }
                if (mode != 1) {
                    launch_as_scatter_h(A.yH, 0);
                    dev.gemv_t_dev(sk().d_Ah, A.yfull, A.tN);                                              // A_HF' yH
                    launch_as_rd();
                    dev.gemv_n_dev(sk().d_Ah, A.rd, A.t);                                                  // A_HF rd
                    launch_as_gather_h(nH);
                    dev.chol_solve_dev(sk().main_fac, A.v, A.u, nH);
                    launch_as_add_yh(nH);
                }
            }
        }
        if (nH > 0) launch_as_merge(mode != 1 ? 1 : 0);
        dev.gemv_n_dev(sk().d_Ah, A.p, A.t);
        if (mode == 1) {
            launch_as_scatter_h(A.uacc, 0);
            dev.gemv_t_dev(sk().d_Ah, A.yfull, A.tN);
        } else {
            dev.gemv_t_dev(sk().d_Ah, A.y, A.tN);
        }
        h->stats.eqp += 1;
    }

    // oracle: eqp_loop - solve, LP optimality test, bulk correction of the working set, at most `rounds` corrections.
    // Starts from the sets in S_[0]; on return `final_sets` is the buffer holding the last working set.
    bool eqp_loop(const double* p_ref, const double* y_ref, int rounds) {
        if (h->test_no_polish) return false;      // test hook (asm_test_no_polish): every active-set attempt fails -> the last resort decides
        int cur = 0, nx = 1, prev = 2;
        bool have_prev = false;
        double pr_last = -1.0;
        double t_round = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
        for (int k = 0; k <= rounds; ++k) {
            asmb::barrier(btag + 60 + k);
            if (ns_lp && p_ref == d_zero && y_ref == nullptr) {
                if (!as_solve_ns(S_[cur])) return false;
            } else {
                as_solve(S_[cur], p_ref, y_ref, 0);
            }
            launch_as_finish(S_[cur], S_[nx], S_[prev], have_prev ? 1 : 0, TOL_P, TOL_D);
            as_read();
            const double pr = sk().h_asscal[AS_PR], du = sk().h_asscal[AS_DU];
            h->stats.kkt_pr = pr;
            h->stats.kkt_du = du;
            final_sets = cur;
            if (h->knobs.verbose) {
                const double t_now = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
                std::fprintf(stderr, "[asm] eqp round %d: pr %.3e du %.3e changes %d  (%.2f ms)\n", k, pr, du, sk().h_ascnt[AC_NCHG], t_now - t_round);
                t_round = t_now;
            }
            if (pr <= TOL_P && du <= TOL_D) return true;
            if (k == rounds) break;
            // oracle: EQP_RUNAWAY - a correction that made the primal residual 1000 times worse has left the neighbourhood of the partition
            if (pr_last >= 0.0 && pr > EQP_RUNAWAY * std::max(pr_last, TOL_P)) break;
            pr_last = pr;
            if (sk().h_ascnt[AC_NCHG] == 0 || (have_prev && sk().h_ascnt[AC_NDIFF] == 0)) break;
            // oracle: EQP_MAXCHG - a correction that moves more than 3 % of all constraints at once has run away: the next solve is not made
            if ((double)sk().h_ascnt[AC_NCHG] > std::max((double)EQP_MINCHG, EQP_MAXCHG * (double)(lp.n + lp.M + lp.ns))) break;
            const int old_prev = prev;
            prev = cur; cur = nx; nx = old_prev;
            have_prev = true;
            final_sets = cur;
        }
        return false;
    }

    // bordered Cholesky of the small matrix Z'Z (host)
    struct SmallChol {
        std::vector<vec> T, L;
        bool factor_row(size_t k) {                 // row k of L from rows 0..k-1 and T[k]
            vec l(k + 1, 0.0);
            for (size_t a = 0; a < k; ++a) {
                double v = T[k][a];
                for (size_t b = 0; b < a; ++b) v -= l[b] * L[a][b];
                l[a] = v / L[a][a];
            }
            double d2 = T[k][k];
            for (size_t b = 0; b < k; ++b) d2 -= l[b] * l[b];
            if (!(d2 > 1e-14 * T[k][k])) return false;
            l[k] = std::sqrt(d2);
            L.push_back(l);
            return true;
        }
        bool append(const vec& trow) {              // trow: products with the members so far, then the diagonal entry
            const size_t k = T.size();
            for (size_t a = 0; a < k; ++a) T[a].push_back(trow[a]);
            T.push_back(trow);
            if (factor_row(k)) return true;
            T.pop_back();
            for (size_t a = 0; a < k; ++a) T[a].pop_back();
            return false;
        }
        bool remove_swap(size_t j) {                // member j leaves, the last member takes its slot
            const size_t last = T.size() - 1;
            if (j != last) {
                std::swap(T[j], T[last]);
                for (auto& r_ : T) std::swap(r_[j], r_[last]);
            }
            T.pop_back();
            for (auto& r_ : T) r_.pop_back();
            L.clear();
            for (size_t k = 0; k < T.size(); ++k)
                if (!factor_row(k)) return false;
            return true;
        }
        vec solve(const vec& g) const {
            const size_t k = L.size();
            vec x(g.begin(), g.begin() + k);
            for (size_t a = 0; a < k; ++a) {
                for (size_t b = 0; b < a; ++b) x[a] -= L[a][b] * x[b];
                x[a] /= L[a][a];
            }
            for (size_t a = k; a-- > 0;) {
                for (size_t b = a + 1; b < k; ++b) x[a] -= L[b][a] * x[b];
                x[a] /= L[a][a];
            }
            return x;
        }
    };

    bool face_primal_anchored() {
        const int64_t n = lp.n, M = lp.M, ns = lp.ns, ldz = sk().ldn;
        as_copy_sets(4, 3);
        as_solve(S_[4], nullptr, nullptr, 1);            // p0 = least-norm point of the partition; its factor, Hidx, Fmask stay
        const int nH0 = as_nH;
        double *p0 = d_pf, *t0 = d_actf;
        dcopy(p0, A.p, n); dcopy(t0, A.t, M);
        dcopy(d_pa, d_p0, n); dcopy(d_sa, d_s0, ns); dcopy(d_acta, d_act0, M);
        std::vector<std::pair<int, int64_t>> members;
        vec g, sign, u;
        SmallChol sc;
        for (int st = 0; st < FACE_STEPS; ++st) {
            const int k = (int)members.size();
            if (k > 0) {
                HIPCHK(asmb::copy_async(sk().d_nsu, u.data(), k * sizeof(double), hipMemcpyHostToDevice, h->stream));
                launch_face_ns_combine(p0, sk().d_Zbuf, ldz, sk().d_nsu, k, A.p);
            } else {
                dcopy(A.p, p0, n);
            }
            dev.gemv_n_dev(sk().d_Ah, A.p, A.t);
            launch_face_ns_step(S_[4], d_pa, d_sa, d_acta, TOL_P);
            as_read();                                    // (the host copy of u is no longer needed by the device after this)
            const int nviol = sk().h_ascnt[AC_NVIOL];
            if (h->knobs.verbose && (st < 5 || st % 20 == 0 || nviol == 0))
                std::fprintf(stderr, "[asm] face primal anchored %d: members %d viol %d hres %.2e\n", st, k, nviol, sk().h_asscal[AS_HARDRES]);
            if (sk().h_asscal[AS_HARDRES] > TOL_P) return false;
            if (nviol == 0) {
                int jw = -1;
                double worst = FACE_TOL_M;
                for (int j = 0; j < k; ++j)
                    if (-sign[j] * u[j] > worst) { worst = -sign[j] * u[j]; jw = j; }
                if (jw < 0) return true;                  // feasible, every multiplier has the right sign: THE least-norm point
                launch_face_ns_unmark(S_[4], members[jw].first, members[jw].second);
                dcopy(d_pa, A.p, n); dcopy(d_sa, A.s, ns); dcopy(d_acta, A.act, M);
                const int last = k - 1;
                if (jw != last) {
                    dcopy(sk().d_Zbuf + (int64_t)jw * ldz, sk().d_Zbuf + (int64_t)last * ldz, ldz);
                    members[jw] = members[last]; g[jw] = g[last]; sign[jw] = sign[last];
                }
                members.pop_back(); g.pop_back(); sign.pop_back();
                if (!sc.remove_swap((size_t)jw)) return false;
                u = sc.solve(g);
                continue;
            }
            const int fam = sk().h_ascnt[AC_NCHG];
            const int64_t e = sk().h_ascnt[AC_NDIFF];
            if (fam < 0) return false;                    // no blocking inequality could be named (a ratio that is not a number): k_face_ns_step
            launch_face_ns_col(sk().d_Ah, sk().ldn, fam, e, p0, t0);
            if (nH0 > 0) {
                dev.gemv_n_dev(sk().d_Ah, A.rd, A.t);
                launch_as_gather_h(nH0);
                dev.chol_solve_dev(sk().main_fac, A.v, A.u, nH0);
                launch_as_scatter_h(A.u, 0);
                dev.gemv_t_dev(sk().d_Ah, A.yfull, A.tN);
            } else {
                HIPCHK(asmb::fill_async(A.tN, 0, sk().ldn * sizeof(double), h->stream));
            }
            double* znew = sk().d_Zbuf + (int64_t)k * ldz;
            launch_face_ns_z(znew);
            asmb::launch(k_gemv_n, asmb::blocks(k + 1, 4), dim3(256), h->stream, sk().d_Zbuf, ldz, znew, sk().d_nsdots, (int64_t)(k + 1), ldz);
            HIPCHK(asmb::copy_async(sk().h_nsdots, sk().d_nsdots, (k + 1) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(asmb::copy_async(sk().h_asscal, A.scal, AS_COUNT * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(asmb::sync(h->stream));
            const double zz = sk().h_nsdots[k], cc = sk().h_asscal[AS_PR];
            if (!(zz > 1e-10 * cc)) return false;        // dependent on the working set although it blocks
            vec trow(sk().h_nsdots, sk().h_nsdots + k + 1);
            if (!sc.append(trow)) return false;
            members.emplace_back(fam, e);
            g.push_back(sk().h_asscal[AS_EQRES]);
            sign.push_back(fam == 0 ? (double)lp.rtype[e] : (fam == 1 ? -lp.scoef[e] : (fam == 2 ? 1.0 : -1.0)));
            u = sc.solve(g);
            h->stats.eqp += 1;
        }
        return false;
    }

    // oracle: face_polish - canonical pair of a non-unique optimum on the partition in S_[3].
    // Returns 2 ('face': least-norm point + basic multipliers), 1 ('ref': projection of the iterate), 0 (partition not optimal).
    int face_polish() {
        if (h->test_no_polish) return 0;
        const int64_t n = lp.n, M = lp.M, ns = lp.ns;
        launch_as_clip0(P.p, d_pref);
        as_solve(S_[3], d_pref, P.y, 0);
        launch_as_finish(S_[3], S_[1], S_[2], 0, TOL_P, TOL_D);
        as_read();
        h->stats.kkt_pr = sk().h_asscal[AS_PR];
        h->stats.kkt_du = sk().h_asscal[AS_DU];
        if (h->knobs.verbose) std::fprintf(stderr, "[asm] face polish: projection of the iterate on its partition pr %.3e du %.3e\n", sk().h_asscal[AS_PR], sk().h_asscal[AS_DU]);
        if (!(sk().h_asscal[AS_PR] <= TOL_P && sk().h_asscal[AS_DU] <= TOL_D)) return 0;
        dcopy(d_p0, A.p, n); dcopy(d_s0, A.s, ns); dcopy(d_y0, A.y, M); dcopy(d_act0, A.act, M); dcopy(d_z0, A.z, n);
        part_factor = true;            // the main factor belongs to the partition: the first dual / primal round below re-use it
        // ---- dual: basic least-squares multipliers on the partition, sign repair (oracle: face_dual; independent of the primal
        // stage, run first so that its round 0 and the primal round 0 share the factorisation of the projection above)
        bool okd = false;
        as_copy_sets(5, 3);
        for (int r = 0; r < FACE_BULK; ++r) {
            as_solve(S_[5], nullptr, nullptr, 2, r == 0);
            launch_face_dual_finish(S_[5], FACE_TOL_M);
            as_read();
            if (h->knobs.verbose) std::fprintf(stderr, "[asm] face dual %d: nH %d nF %d viol %d\n", r, as_nH, as_nF, sk().h_ascnt[AC_NVIOL]);
            if (sk().h_ascnt[AC_NVIOL] == 0) { okd = true; break; }
        }
        if (okd) { dcopy(d_yf, A.y, M); dcopy(d_zf, A.z, n); }
        // ---- primal: bulk rounds
        bool okp = false;
        if (okd) {
            as_copy_sets(4, 3);
            for (int r = 0; r < FACE_BULK; ++r) {
                as_solve(S_[4], nullptr, nullptr, 1, r == 0);
                launch_face_primal_finish(S_[4], S_[3], TOL_P, FACE_TOL_M, 0);
                as_read();
                if (h->knobs.verbose) std::fprintf(stderr, "[asm] face primal bulk %d: nH %d nF %d viol %d rel %d hres %.2e\n", r, as_nH, as_nF, sk().h_ascnt[AC_NVIOL], sk().h_ascnt[AC_NREL], sk().h_asscal[AS_HARDRES]);
                if (sk().h_asscal[AS_HARDRES] > TOL_P) break;            // over-determined working set
                if (sk().h_ascnt[AC_NVIOL] > 0) continue;
                if (sk().h_ascnt[AC_NREL] == 0) { okp = true; break; }
            }
            // ---- primal: anchored method in the null space of the partition (oracle: _face_primal_anchored) - one factorisation,
            // one solve with it per added constraint, the k x k matrix Z'Z of the added constraints on the host
            if (!okp && face_primal_anchored()) {
                // the answer is the least-norm point of the FINAL working set, computed like any other (fresh factorisation)
                as_solve(S_[4], nullptr, nullptr, 1);
                launch_face_primal_finish(S_[4], S_[3], TOL_P, FACE_TOL_M, 1);
                as_read();
                okp = sk().h_asscal[AS_HARDRES] <= TOL_P && sk().h_ascnt[AC_NVIOL] == 0;
            }
        }
        part_factor = false;
        if (okp && okd) {
            dcopy(A.y, d_yf, M); dcopy(A.z, d_zf, n);      // (p, s, act) are the primal stage's last solve; y, z come from the dual stage
            launch_face_kkt(S_[5]);
            as_read();
            h->stats.kkt_pr = sk().h_asscal[AS_PR];
            h->stats.kkt_du = sk().h_asscal[AS_DU];
            if (h->knobs.verbose) std::fprintf(stderr, "[asm] face kkt pr %.2e du %.2e\n", sk().h_asscal[AS_PR], sk().h_asscal[AS_DU]);
            if (sk().h_asscal[AS_PR] <= TOL_P && sk().h_asscal[AS_DU] <= TOL_D) { final_sets = 4; return 2; }
        }
        dcopy(A.p, d_p0, n); dcopy(A.s, d_s0, ns); dcopy(A.y, d_y0, M); dcopy(A.act, d_act0, M); dcopy(A.z, d_z0, n);
        final_sets = 3;
        return 1;
    }


    // oracle: phase1_infeasible - elastic LP over the same rows/box; its optimal multipliers are a Farkas
    // certificate of the original LP, verified rigorously before INFEASIBLE is reported.
    bool phase1_infeasible() {
        SLP saved = lp;
        IpmState saved_ip = ip;
        lp.ns = sk().ns;
        std::fill(lp.q.begin(), lp.q.end(), 0.0);
        lp.w.assign(lp.ns, 1.0);
        lp.slo.assign(lp.ns, 0.0);
        lp.scale_q = 1.0;
        ipm_init();
        ipm_run(1e-8, IPM_MAXIT);
        vec y1;
        down(y1, P.y, lp.M);
        HIPCHK(asmb::sync(h->stream));
        int its = ip.iters;
        lp = saved;
        ip = saved_ip;
        ipm_upload_lp();              // the original LP again (the interrupted iterate is not resumed after phase 1)
        h->stats.ipm_iters += its;
        return farkas_margin(y1) > 1e-9;
    }

    // oracle: solve_scaled
    double t_warm = 0, t_ipm = 0, t_polish = 0;
    bool snap_e = false;      // the snapshot of the best iterate holds the null-space form's component e
    void stats_measures() { h->stats.ipm_pinf = ip.pinf; h->stats.ipm_dinf = ip.dinf; h->stats.ipm_gap = ip.gap; }
    // best-iterate safeguard, second half (oracle: solve_scaled): the snapshot comes back, is measured and its partition identified
    void restore_best() {
        launch_snapshot(snap_e ? nsv(14) : (double*)nullptr, 1);
        ipm_measures();
        stats_measures();
        h->stats.restored = 1;
        identify_dev(3);
    }
    int solve_scaled(const ActiveSet* warm, SolveHint& hint) {
        int st = solve_scaled_impl(warm, hint);
        if (h->knobs.verbose) std::fprintf(stderr, "[asm] phases: warm %.2f ms, ipm %.2f ms (%d its), polish %.2f ms, path %d\n", t_warm, t_ipm, ip.iters, t_polish, h->stats.path);
        return st;
    }
    int solve_scaled_impl(const ActiveSet* warm, SolveHint& hint) {
        const int64_t n = lp.n, M = lp.M, ns = lp.ns;
        h->stats.path = -1;
        h->stats.polished = 1;
        h->stats.restored = 0;
        cur_hint = &hint;
        btag = 30;
        asmb::barrier(btag);
        ipm_upload_lp();
        as_begin_lp();
        // null-space basis of the equality rows (oracle: solve_scaled): made first, the active-set solves of the warm attempt and of the
        // polish go through it as well as the interior-point iterations
        ns_lp = false;
        h->stats.ns_dim = 0;
        h->stats.ns_cold = 0;
        h->stats.ns_path = 0;
        if (ns_applicable()) {
            const size_t had = hint.ns_J.size();
            const double t0 = now_ms();
            ns_lp = ns_setup();
            if (ns_lp) ns_lp_vectors();
            h->stats.ns_dim = ns_lp ? ns_k : 0;
            h->stats.ns_cold = (ns_lp && (had == 0 || ns_was_cold)) ? 1 : 0;
            h->stats.ns_path = ns_lp ? ns_path : 0;
            if (h->knobs.verbose) {
                HIPCHK(asmb::sync(h->stream));
                std::fprintf(stderr, "[asm] null-space set-up: %s, k = %d, %s basis columns, %.2f ms\n", ns_lp ? "ok" : "not usable", ns_k, ns_was_cold ? "fresh" : "retained", now_ms() - t0);
            }
        }
        if (warm && warm->valid && (int64_t)warm->rowst.size() == M && (int64_t)warm->bst.size() == n && (int64_t)warm->sst.size() == ns) {
            // attempt when the last two LPs ended on the same sets or the back-off has run out (oracle: solve_scaled)
            if (!hint.stable && hint.warm_skip > 0) {
                hint.warm_skip -= 1;
            } else {
                double t0 = now_ms();
                btag = 40 - 60;
                as_upload_sets(*warm, 0);
                bool okw = eqp_loop(d_zero, nullptr, 1);
                t_warm += now_ms() - t0;
                if (okw) { hint.warm_fail = 0; hint.warm_skip = 0; h->stats.path = 0; return ASM_OPTIMAL; }
                hint.warm_fail = std::min(hint.warm_fail + 1, WARM_BACKOFF_MAX);
                hint.warm_skip = (1 << hint.warm_fail) - 1;
                hint.stable = false;
            }
        }
        const bool prefer_ref = hint.prefer_ref;
        btag = 90;
        asmb::barrier(btag);
        ipm_init();
        const double tols[3] = {IPM_TOL0, 0.1 * IPM_TOL0, 1e-12};      // oracle: IPM_STAGES
        const int more[3] = {IPM_MAXIT, 6, 6};
        bool have_sets = false;
        double best_m = INF, m_last = INF;
        bool have_snap = false;
        for (int stage = 0; stage < 3; ++stage) {
            double t0 = now_ms();
            btag = 100 + 100 * stage;
            int st = ipm_run(tols[stage], more[stage]);
            asmb::barrier(btag + 50);
            t_ipm += now_ms() - t0;
            h->stats.ipm_iters = ip.iters;
            h->stats.col_iters = ip.col_iters;
            h->stats.ns_iters = ip.ns_iters;
            stats_measures();
            if (st == ASM_INFEASIBLE) { h->stats.path = 6; return ASM_INFEASIBLE; }
            {
                // best-iterate safeguard, first half (oracle: solve_scaled): the iterate at the end of the best stage so far is kept
                m_last = std::max(ip.pinf, std::max(ip.dinf, ip.gap));
                double* e_ns = ip.ns_e_ready ? nsv(14) : nullptr;      // (set only by iterations in null-space form)
                if (m_last < best_m) {
                    launch_snapshot(e_ns, 0);
                    best_m = m_last; have_snap = true; snap_e = e_ns != nullptr;
                }
            }
            if (st == ASM_OTHER && stage == 0) {
                // the IPM is only the identifier: a jammed / slow run that is already close is still handed to
                // the active-set solve, whose LP optimality test decides (oracle: solve_scaled)
                if (ip.pinf <= 1e-3 && ip.dinf <= 1e-3 && ip.gap <= 1e-4) {
                    identify_dev(3);
                    have_sets = true;
                    as_copy_sets(0, 3);
                    if (eqp_loop(d_zero, nullptr, 3)) { h->stats.path = 8; return ASM_OPTIMAL; }
                }
                if (lp.ns == 0 && phase1_infeasible()) { h->stats.path = 7; return ASM_INFEASIBLE; }
                break;
            }
            double t1 = now_ms();
            identify_dev(3);
            if (h->knobs.verbose) { HIPCHK(asmb::sync(h->stream)); std::fprintf(stderr, "[asm] stage %d identify %.2f ms\n", stage, now_ms() - t1); }
            have_sets = true;
            bool tried_ln = false;
            if (ns_lp) {
                // the least-norm polish in reduced coordinates costs two solves with the factor of S0: tried first whatever the last LP
                // needed (oracle: solve_scaled)
                as_copy_sets(0, 3);
                const bool okn = eqp_loop(d_zero, nullptr, 2);
                if (okn) { t_polish += now_ms() - t1; hint.prefer_ref = false; h->stats.path = 1 + stage; return ASM_OPTIMAL; }
                tried_ln = true;
            }
            if (prefer_ref) {
                // non-unique optimum expected: the canonical pair as soon as the partition passes the LP optimality test
                // (oracle: solve_scaled)
                const int how = face_polish();
                t_polish += now_ms() - t1;
                if (how == 2) { h->stats.path = 4; return ASM_OPTIMAL; }
                if (how == 1) { h->stats.path = 9; return ASM_OPTIMAL; }
                continue;
            }
            if (tried_ln) { t_polish += now_ms() - t1; continue; }
            as_copy_sets(0, 3);
            bool okp = eqp_loop(d_zero, nullptr, 2);
            t_polish += now_ms() - t1;
            if (okp) { h->stats.path = 1 + stage; return ASM_OPTIMAL; }
        }
        btag = 400;
        asmb::barrier(btag);
        if (have_snap && have_sets && m_last > IPM_DEGRADE * best_m) {
            // best-iterate safeguard, second half (oracle: solve_scaled): no stage ended in a successful polish and the last one ended IPM_DEGRADE
            // times worse than the best - the best iterate comes back, the final attempts run on it and on the partition identified from it
            restore_best();
            if (h->knobs.verbose) std::fprintf(stderr, "[asm] last stage ended %.1e against %.1e at best: best iterate restored (pinf %.3e dinf %.3e gap %.3e)\n", m_last, best_m, ip.pinf, ip.dinf, ip.gap);
        }
        if (have_sets) {
            double t1 = now_ms();
            // non-unique optimum: canonical (least-norm) pair of the optimal faces the partition describes (oracle: face_polish)
            const int how = prefer_ref ? 0 : face_polish();
            t_polish += now_ms() - t1;
            if (how == 2) { hint.prefer_ref = true; h->stats.path = 4; return ASM_OPTIMAL; }
            if (how == 1) { hint.prefer_ref = true; h->stats.path = 9; return ASM_OPTIMAL; }
            // the partition is not optimal as it stands: bulk corrections from the iterate's projection
            as_copy_sets(0, 3);
            bool okr = eqp_loop(d_pref, P.y, 2);
            if (okr) {
                // the corrected working set passes the LP optimality test, i.e. it describes a face of optimal points: return that
                // face's canonical pair (a function of the discrete set) rather than the projection of the iterate onto it
                // (oracle: solve_scaled).  face_polish leaves the projection in place when its own stages do not succeed.
                hint.prefer_ref = true;
                if (final_sets != 3) as_copy_sets(3, final_sets);
                const int eqp_sets = final_sets;
                const int how2 = face_polish();
                if (how2 == 0) final_sets = eqp_sets;
                h->stats.path = how2 == 2 ? 4 : 9;
                return ASM_OPTIMAL;
            }
            hint.prefer_ref = false;
            if (prefer_ref && !ns_lp) {                     // the least-norm polish has not been tried on this LP yet
                as_copy_sets(0, 3);
                if (eqp_loop(d_zero, nullptr, 2)) { h->stats.path = 3; return ASM_OPTIMAL; }
            }
        }
        // last resort (oracle: solve_scaled, 'ipm-conv'): an iterate converged to IPM_ACCEPT in all three measures is an optimal point of the
        // LP to that accuracy; it is handed out through the active-set arena (clipped into the box, partition of the last identification)
        bool conv = have_sets && ip.pinf <= IPM_ACCEPT && ip.dinf <= IPM_ACCEPT_DUAL && ip.gap <= IPM_ACCEPT;
        if (!conv && have_sets && have_snap && best_m <= IPM_ACCEPT) {
            // ... or the best stage end did (the last iterations drifted out of the acceptance, but by less than IPM_DEGRADE): that iterate then
            restore_best();
            conv = true;
        }
        if (conv) {
            launch_as_clip0(P.p, A.p);
            dcopy(A.y, P.y, lp.M);
            if (lp.ns) {
                launch_as_smax(P.s, A.s);
                launch_as_sl_values();      // the tail kernel must not recompute slacks from a stale working set
            }
            dev.gemv_n_dev(sk().d_Ah, A.p, A.t);
            dev.gemv_t_dev(sk().d_Ah, A.y, A.tN);
            launch_as_finish(S_[3], S_[1], S_[2], 0, TOL_P, TOL_D);
            as_read();
            final_sets = 3;
            h->stats.path = 10;
            return ASM_OPTIMAL;
        }
        // no active-set solve passed the LP optimality test: the interior iterate is not returned as a solution
        // (status OTHER; the SLP caller stops with a warning, slp_line_search.jl:127-133)
        h->stats.path = 5;
        h->stats.polished = 0;
        return ASM_OTHER;
    }

};

// =====================================================================================================
// formulation + extraction (subproblem.jl:229-542)
// =====================================================================================================
int row_kind(double lb, double ub) {
    if (lb == ub) return 0;
    if (lb != -INF && ub != INF && lb < ub) return 2;
    if (lb != -INF) return 1;
    if (ub != INF) return -1;
    return 9;
}

// the orthonormal basis of the previous LP is no longer resident (no form, or no k-sized buffers yet: nothing to forget)
void ns_forget_basis(Skeleton& K) { if (K.nsf && K.nsf->k) K.nsf->k->Zk = 0; }

// forgets the retained working sets and adaptive hints of both phases and the resident null-space basis; keep_ns_J: the basis columns of
// the null-space form stay
void reset_warm(Skeleton& K, bool keep_ns_J) {
    std::vector<int> J;
    if (keep_ns_J) J.swap(K.hint[0].ns_J);
    K.warm[0] = ActiveSet(); K.warm[1] = ActiveSet();
    K.hint[0] = SolveHint(false); K.hint[1] = SolveHint(true);
    K.hint[0].ns_J.swap(J);
    ns_forget_basis(K);
}

void check_panel_timeout(asm_handle* h) {
    unsigned tmo = 0;
    HIPCHK(asmb::copy(&tmo, h->sk->d_ptmo, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (tmo != 0) {
        HIPCHK(asmb::fill(h->sk->d_ptmo, 0, sizeof(unsigned)));      // reported once: the handle stays usable
        throw HipError("k_chol_panel: a workgroup timed out waiting for a producer (grid not resident?)");
    }
}

void do_setup(asm_handle* h, int64_t n, int64_t m, int64_t nnz, const int64_t* j_row, const int64_t* j_col, const double* c_lb,
              const double* c_ub, const double* v_lb, const double* v_ub) {
    if (n <= 0 || m < 0 || nnz < 0 || (nnz > 0 && (!j_row || !j_col)) || (m > 0 && (!c_lb || !c_ub)) || !v_lb || !v_ub)
        throw std::invalid_argument("asm_sublp_setup: bad dimensions or null pointer");
    HIPCHK(hipSetDevice(h->device));
    h->lm.drop();
    h->ev.reset(); h->sk.reset();   // released before anything is allocated; the new skeleton is built here and installed last: a failure leaves none
    auto sk = std::make_unique<Skeleton>();
    Skeleton& K = *sk;
    K.n = n; K.m = m; K.nnz = nnz;
    K.j_row_h.assign(j_row, j_row + nnz); K.j_col_h.assign(j_col, j_col + nnz);
    K.c_lb.assign(c_lb, c_lb + m); K.c_ub.assign(c_ub, c_ub + m);
    K.v_lb.assign(v_lb, v_lb + n); K.v_ub.assign(v_ub, v_ub + n);
    K.kind.resize(m);
    for (int64_t i = 0; i < m; ++i) {
        K.kind[i] = row_kind(c_lb[i], c_ub[i]);
        if (K.kind[i] == 9) throw Unsupported("free constraint row (c_lb=-Inf, c_ub=+Inf) is not representable");
        if (K.kind[i] == 2) K.adj.push_back(i);
    }
    K.nadj = (int64_t)K.adj.size();
    K.M = m + K.nadj;
    K.Mp = IpmLayout(n, K.M, 0).Mp;
    K.ldn = IpmLayout(n, K.M, 0).ldn;    // multiple of the SYRK k-chunk (ASM_KC)
    K.rtype.assign(K.M, 0);
    for (int64_t i = 0; i < m; ++i) K.rtype[i] = K.kind[i] == 0 ? 0 : (K.kind[i] == -1 ? -1 : 1);
    for (int64_t k = 0; k < K.nadj; ++k) K.rtype[m + k] = -1;
    // slack layout (subproblem.jl:83-112): one per row, two when both bounds are finite
    K.nslack.assign(m, 1);
    std::vector<int64_t> adjpos(m, -1);
    for (int64_t k = 0; k < K.nadj; ++k) adjpos[K.adj[k]] = k;
    for (int64_t i = 0; i < m; ++i) {
        K.nslack[i] = (c_lb[i] > -INF && c_ub[i] < INF) ? 2 : 1;
        int kd = K.kind[i];
        if (kd == 0) { K.srow.push_back((int)i); K.scoef.push_back(1.0); K.srow.push_back((int)i); K.scoef.push_back(-1.0); K.sown.push_back(i); K.sown.push_back(i); }
        else if (kd == 2) { K.srow.push_back((int)i); K.scoef.push_back(1.0); K.srow.push_back((int)(m + adjpos[i])); K.scoef.push_back(-1.0); K.sown.push_back(i); K.sown.push_back(i); }
        else if (kd == 1) { K.srow.push_back((int)i); K.scoef.push_back(1.0); K.sown.push_back(i); }
        else { K.srow.push_back((int)i); K.scoef.push_back(-1.0); K.sown.push_back(i); }
    }
    K.ns = (int64_t)K.srow.size();

    // assembly plan: stable sort of the COO entries by (row, col)
    for (int64_t k = 0; k < nnz; ++k)
        if (j_row[k] < 1 || j_row[k] > m || j_col[k] < 1 || j_col[k] > n) throw std::invalid_argument("j_row/j_col out of range (1-based)");
    bool dense = (nnz == m * n) && K.nadj == 0 && nnz > 0;
    if (dense)
        for (int64_t k = 0; k < nnz && dense; ++k) dense = (j_row[k] - 1) * n + (j_col[k] - 1) == k;
    K.dense_fast = dense;
    std::vector<int64_t> perm(nnz), ustart, uoff, adjoff;
    std::iota(perm.begin(), perm.end(), 0);
    if (!dense) {
        std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) {
            int64_t ka = (j_row[a] - 1) * n + (j_col[a] - 1), kb = (j_row[b] - 1) * n + (j_col[b] - 1);
            return ka < kb;
        });
        int64_t prev = -1;
        for (int64_t t = 0; t < nnz; ++t) {
            int64_t k = perm[t];
            int64_t r = j_row[k] - 1, c = j_col[k] - 1, key = r * n + c;
            if (key != prev) {
                ustart.push_back(t);
                uoff.push_back(r * K.ldn + c);
                adjoff.push_back(adjpos[r] >= 0 ? (m + adjpos[r]) * K.ldn + c : -1);
                prev = key;
            }
        }
        ustart.push_back(nnz);
    }
    K.nu = dense ? nnz : (int64_t)uoff.size();
    // sparse pattern (CSR + CSC) of the LP matrix rows [0, M): the unique Jacobian entries plus the copies of the range
    // rows; used by the matrix-vector products when the fill is below 1/16
    std::vector<int> sp_ptr, sp_col, sc_ptr, sc_row, sc_pos;
    std::vector<int64_t> sp_off;
    {
        int64_t nadjent = 0;
        for (int64_t v : adjoff) nadjent += v >= 0;
        const int64_t nnzS = (int64_t)uoff.size() + nadjent;
        if (!dense && nnzS > 0 && nnzS * 16 <= K.M * n && nnzS < (int64_t)1 << 30) {
            sp_off.reserve(nnzS);
            for (int64_t v : uoff) sp_off.push_back(v);                 // sorted by (row, col), rows < m
            for (int64_t v : adjoff) if (v >= 0) sp_off.push_back(v);   // rows m.., same order
            sp_ptr.assign(K.M + 1, 0);
            sp_col.resize(nnzS);
            for (int64_t k = 0; k < nnzS; ++k) {
                sp_ptr[sp_off[k] / K.ldn + 1] += 1;
                sp_col[k] = (int)(sp_off[k] % K.ldn);
            }
            for (int64_t i = 0; i < K.M; ++i) sp_ptr[i + 1] += sp_ptr[i];
            csc_from_csr(sp_ptr, sp_col, n, sc_ptr, sc_row, sc_pos);
            K.sp_nnz = nnzS;
        }
    }

    BufPool& P = K.mem;
    const hipStream_t s = h->stream;
    P.alloc(K.d_dE, nnz);
    P.zeroed(K.d_J, K.Mp * K.ldn, s);
    P.zeroed(K.d_Ah, K.Mp * K.ldn, s);
    FacBuf& F = K.main_fac;
    F.ld = K.Mp;
    P.alloc(F.S, K.Mp * K.Mp);
    P.alloc(K.d_c, K.ldn); P.alloc(K.d_rho, K.Mp); P.alloc(K.d_theta, K.ldn);
    P.alloc(K.d_diag, K.Mp); P.alloc(K.d_diag0, K.Mp);
    P.zeroed(K.d_vecN, K.ldn, s); P.zeroed(K.d_vecM, K.Mp, s); P.alloc(K.d_vecM2, K.Mp);
    P.alloc(K.d_partial, (int64_t)ASM_TMAXCHUNKS * K.ldn);
    P.alloc(K.d_idx, K.Mp);
    P.alloc(F.Linv, (K.Mp / ASM_NB + 1) * ASM_NB * ASM_NB);
    P.zeroed(K.d_pflags, ASM_PNL_FLAGS, s);
    P.zeroed(K.d_ptmo, 4, s);
    F.wb = K.M > 1536 ? 1024 : 512;      // wide-block width of the triangular solves (k_wtrsv_*<WB>)
    if (K.M >= RED_MIN_M) {
        P.alloc(K.d_idxI, K.Mp); P.alloc(K.d_rdI, K.Mp); P.alloc(K.d_rce, K.Mp); P.alloc(K.d_rze, K.Mp); P.alloc(K.d_sdiag, K.Mp);
    }
    // column form of the restoration-phase Newton system (every row owns a slack column there): n x n instead of M x M
    K.col_capable = K.M >= COL_MIN_M && (double)n <= COL_MAX_RATIO * (double)K.M && n <= K.Mp;
    if (K.col_capable) {
        K.ldT = round_up(K.M, 32);
        P.zeroed(K.d_AhT, n * K.ldT, s);
        P.zeroed(K.d_cdinv, K.ldT, s); P.zeroed(K.d_cth, K.ldn, s); P.zeroed(K.d_cu, K.Mp, s); P.zeroed(K.d_ct, K.ldn, s);
        P.zeroed(K.d_cv, K.ldn, s); P.zeroed(K.d_cw, K.Mp, s);
        P.alloc(K.d_nzT, (n / 32 + 2) * (K.ldT / ASM_KC + 1));
    }
    P.alloc(F.Binv, (K.Mp / F.wb + 1) * (int64_t)F.wb * F.wb);
    P.alloc(F.BinvT, (K.Mp / F.wb + 1) * (int64_t)F.wb * F.wb);
    P.alloc(K.d_wpart, (K.Mp / ASM_WBROWS + 2) * (int64_t)1024);
    P.alloc(K.d_wt, 1024);
    K.nz_half = (K.Mp / 32 + 1) * (K.ldn / ASM_KC + 1);
    P.alloc(K.d_nz, 2 * K.nz_half);
    if (K.sp_nnz > 0) {
        P.upload(K.d_sp_ptr, sp_ptr.data(), K.M + 1); P.upload(K.d_sp_col, sp_col.data(), K.sp_nnz); P.upload(K.d_sp_off, sp_off.data(), K.sp_nnz);
        P.upload(K.d_sc_ptr, sc_ptr.data(), n + 1); P.upload(K.d_sc_row, sc_row.data(), K.sp_nnz); P.upload(K.d_sc_pos, sc_pos.data(), K.sp_nnz);
        P.alloc(K.d_spv_Ah, K.sp_nnz); P.alloc(K.d_spv_J, K.sp_nnz);
        K.sp_ptr_h = sp_ptr; K.sp_col_h = sp_col;
        K.sp_ok = true;
    }
    const IpmLayout lay(n, K.M, K.ns);
    K.nsp = lay.nsp;
    {
        P.zeroed(K.d_ipm, lay.arena_len(), s);
        P.alloc(K.d_ipm_snap, lay.snap_len());
        std::vector<int> iv(lay.int_len(), -1);
        for (int64_t i = 0; i < K.M; ++i) iv[i] = K.rtype[i];
        for (int64_t k = 0; k < K.ns; ++k) {
            int r_ = K.srow[k];
            if (iv[K.Mp + r_] < 0) iv[K.Mp + r_] = (int)k; else iv[2 * K.Mp + r_] = (int)k;
            iv[3 * K.Mp + k] = r_;
        }
        P.upload(K.d_ipm_i, iv.data(), (int64_t)iv.size());
        P.alloc(K.d_redpart, IPM_RED_MAXWG * IPM_RED_SLOTS);
        P.zeroed(K.d_redcnt, 4, s);
        P.alloc(K.h_scal, 64, BufPool::MAPPED, &K.d_hscal);
        P.alloc(K.h_seq, 16, BufPool::MAPPED, &K.d_hseq);
        *K.h_seq = 0;
        const AsLayout alay(K.ldn, K.Mp, K.nsp);
        P.zeroed(K.d_as, alay.dbl_len(), s);
        P.zeroed(K.d_as_i, alay.int_len(), s);
        P.alloc(K.h_ascnt, 64, BufPool::PINNED);
        P.alloc(K.h_asscal, 64, BufPool::PINNED);
        P.zeroed(K.d_Zbuf, (int64_t)(FACE_STEPS + 1) * K.ldn, s);
        P.alloc(K.d_nsu, FACE_STEPS + 8);
        P.alloc(K.d_nsdots, FACE_STEPS + 8);
        P.alloc(K.h_nsdots, FACE_STEPS + 8, BufPool::PINNED);
    }
    // null-space form of the normal-phase Newton system: static part (index lists, factor of S0, work vectors); the buffers sized by the
    // null-space dimension k are allocated by the first LP that uses the form (Solver::ns_reserve)
    {
        int nE = 0;
        for (int64_t i = 0; i < K.M; ++i) nE += K.rtype[i] == 0;
        if (K.sp_ok && nE >= NS_MIN_E && (double)(n - nE) <= NS_MAX_RATIO * (double)K.M && n <= K.Mp && K.M < (int64_t)1 << 30) {
            K.nsf = std::make_unique<NsForm>(NsLayout(K.ldn, K.Mp, nE, K.M - nE));
            NsForm& F = *K.nsf;
            BufPool& Q = F.mem;
            std::vector<int> epos, iidx, ipos, s0_pairs;
            int s0_band = 0;
            ns_index_lists(K.rtype.data(), K.M, sp_ptr, sp_col, K.ldn, F.eidx_h, epos, iidx, ipos, &s0_band, &s0_pairs);
            Q.upload(F.Eidx, F.eidx_h.data(), nE, true); Q.upload(F.Epos, epos.data(), K.M, true);
            Q.upload(F.Iidx, iidx.data(), F.L.nI, true); Q.upload(F.Ipos, ipos.data(), K.M, true);
            Q.zeroed(F.cnt, 16);
            const int f0_band = 2 * (int64_t)s0_band >= nE ? 0 : std::max(s0_band, 1);
            ns_alloc_factor(h, Q, F.f0, F.L.nEp, f0_band);
            F.f0.band = f0_band;
            if (F.f0.band > 0) {                // S0 is then built entry by entry from its structural pattern (k_ns_s0_sparse)
                F.npairs = (int64_t)s0_pairs.size() / 2;
                Q.upload(F.S0pairs, s0_pairs.data(), (int64_t)s0_pairs.size(), true);
            }
            Q.zeroed(F.Lt, F.L.nEp * F.L.nEp, s);
            Q.zeroed(F.th, F.L.th_len(), s);
            Q.zeroed(F.Fm, K.ldn, s);
            Q.zeroed(F.v, F.L.nsv_len(), s);
        }
    }
    // row order of the factorisations (see Skeleton::row_band)
    if (K.sp_ok && K.M >= 256) {
        std::vector<int> all(K.M), pairs_pos;
        for (int64_t i = 0; i < K.M; ++i) all[i] = (int)i;
        int bw = 0;
        const std::vector<int> ord = rcm_order(all, sp_ptr, sp_col, K.ldn, &bw, &pairs_pos);
        if (2 * (int64_t)bw < K.M) {
            K.row_band = std::max(bw, 1);
            K.row_perm_h = ord;
            std::vector<int> pos(K.M), pairs(pairs_pos.size());
            for (int64_t q = 0; q < K.M; ++q) pos[ord[q]] = (int)q;
            for (size_t t = 0; t < pairs_pos.size(); ++t) pairs[t] = ord[pairs_pos[t]];
            K.n_rowpairs = (int64_t)pairs.size() / 2;
            P.upload(K.d_rowperm, ord.data(), K.M); P.upload(K.d_rowpos, pos.data(), K.M); P.upload(K.d_rowpairs, pairs.data(), (int64_t)pairs.size());
            P.upload(K.d_cpos, pos.data(), K.M);      // place of every row in the current row list of the interior-point factor (rewritten per iteration)
            if (!K.d_rce) { P.alloc(K.d_rce, K.Mp); P.alloc(K.d_rze, K.Mp); }
        }
    }
    // column order of the column form (K = Th + A' D^-1 A couples two columns when they share a row)
    if (K.sp_ok && K.col_capable && n >= 256) {
        std::vector<int> all(n), pairs_pos;
        for (int64_t j = 0; j < n; ++j) all[j] = (int)j;
        int bw = 0;
        const std::vector<int> ord = rcm_order(all, sc_ptr, sc_row, K.Mp, &bw, &pairs_pos);
        if (2 * (int64_t)bw < n) {
            K.col_band = std::max(bw, 1);
            std::vector<int> pos(n), pairs(pairs_pos.size());
            for (int64_t q = 0; q < n; ++q) pos[ord[q]] = (int)q;
            for (size_t t = 0; t < pairs_pos.size(); ++t) pairs[t] = ord[pairs_pos[t]];
            K.n_colpairs = (int64_t)pairs.size() / 2;
            P.upload(K.d_colperm, ord.data(), n); P.upload(K.d_colpos, pos.data(), n); P.upload(K.d_colpairs, pairs.data(), (int64_t)pairs.size());
            if (!K.d_rce) { P.alloc(K.d_rce, K.Mp); P.alloc(K.d_rze, K.Mp); }
        }
    }
    K.pin_len = std::max(std::max(K.ldn, K.Mp), K.nsp);
    P.alloc(K.h_pin, 2 * K.pin_len, BufPool::PINNED);
    P.alloc(K.h_up, 3 * K.ldn + K.Mp + 3 * K.nsp + 16, BufPool::PINNED);
    std::memset(K.h_up, 0, (3 * K.ldn + K.Mp + 3 * K.nsp + 16) * sizeof(double));
    {
        const int64_t dl = 2 * K.ldn + 2 * K.Mp + K.nsp + (K.ldn + K.Mp + K.nsp + 1) / 2 + 16;
        P.alloc(K.d_dl, dl);
        P.alloc(K.h_dl, dl, BufPool::PINNED);
    }
    if (!dense) {
        P.upload(K.d_perm, perm.data(), nnz); P.upload(K.d_ustart, ustart.data(), K.nu + 1);
        P.upload(K.d_uoff, uoff.data(), K.nu); P.upload(K.d_adjoff, adjoff.data(), K.nu);
    }
    HIPCHK(asmb::sync(h->stream));
    std::memset(&h->stats, 0, sizeof(h->stats));
    h->sk = std::move(sk);
}

void do_upload(asm_handle* h, const double* dE, const double* df, double f, const double* E, const double* x_k) {
    Skeleton& K = sk_of(h, "asm_sublp_setup has not been called");
    if ((K.nnz > 0 && !dE) || !df || (K.m > 0 && !E) || !x_k) throw std::invalid_argument("asm_sublp_upload: null pointer");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(asmb::copy_async(K.d_dE, dE, K.nnz * sizeof(double), hipMemcpyHostToDevice, h->stream));
    h2d_done(h);
    K.J_valid = false;
    K.df.assign(df, df + K.n); K.E.assign(E, E + K.m); K.x_k.assign(x_k, x_k + K.n);
    K.f = f;
    K.inputs_ready = true;
    K.inputs_from_eval = false;
}

void do_set_bounds(asm_handle* h, const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub) {
    Skeleton& K = sk_of(h, "asm_sublp_set_bounds: asm_sublp_setup first");
    if ((K.m > 0 && (!c_lb || !c_ub)) || !v_lb || !v_ub) throw std::invalid_argument("asm_sublp_set_bounds: null pointer");
    for (int64_t i = 0; i < K.m; ++i)
        if (row_kind(c_lb[i], c_ub[i]) != K.kind[i])
            throw Unsupported("asm_sublp_set_bounds: the kind of a row changes - the LP skeleton is not representable (call asm_sublp_setup)");
    HIPCHK(hipSetDevice(h->device));
    K.c_lb.assign(c_lb, c_lb + K.m); K.c_ub.assign(c_ub, c_ub + K.m);
    K.v_lb.assign(v_lb, v_lb + K.n); K.v_ub.assign(v_ub, v_ub + K.n);
    if (h->ev) ev_write_bounds(h, h->ev->L);
    // the retained working sets and the basis Z belong to the old instance; the basis COLUMNS of the null-space form are kept - the
    // pattern is the same, and a set that no longer spans null(A_EF) is detected and re-selected by the next LP (Solver::ns_setup)
    K.last = ActiveSet();
    reset_warm(K, true);
    K.inputs_ready = false;
}

void do_set_ns_basis(asm_handle* h, const int32_t* J, int64_t k) {
    if (k < 0 || (k > 0 && !J)) throw std::invalid_argument("asm_sublp_set_ns_basis: bad argument");
    Skeleton& K = sk_of(h, "asm_sublp_set_ns_basis: asm_sublp_setup first");
    for (int64_t a = 0; a < k; ++a)
        if (J[a] < 0 || J[a] >= K.n) throw std::invalid_argument("asm_sublp_set_ns_basis: column out of range");
    K.hint[0].ns_J.assign(J, J + k);
    ns_forget_basis(K);
}

// the LP in caller units: min q'p + w's  s.t.  J_i p + E s (=,>=,<=) r_i (rows m.. = the extra `<=` rows of range constraints),
// lb <= p <= ub, s >= slo (slack columns only in the restoration phase; layout of create_model!, subproblem.jl:83-112)
struct LpRaw {
    vec q, r, lb, ub, w, slo;
    bool slacks = false;
};
struct LpSol {
    int status = ASM_OTHER;
    vec p, s, y, z;          // p exactly on its bound where bound-active; y per LP row; z = q - J'y (reduced costs)
    ActiveSet as;
};

// assemble J from the dE in HBM, scale, solve, unscale (oracle: solve_lp).  `slot`: which retained active set / hints to use.
void solve_raw(asm_handle* h, const LpRaw& L, int slot, LpSol& out) {
    Skeleton& K = *h->sk;
    const int64_t n = K.n, M = K.M;
    Solver sv(h);
    SLP& lp = sv.lp;
    std::memset(&h->stats, 0, sizeof(h->stats));
    lp.n = n; lp.M = M; lp.ns = L.slacks ? K.ns : 0;
    lp.rtype = K.rtype.data(); lp.srow = K.srow.data(); lp.scoef = K.scoef.data();
    h->stats.M = (int)M; h->stats.n = (int)n; h->stats.ns = (int)lp.ns;
    // Jacobian -> dense rows incl. range rows; scaled copy (column scale = min(box, matrix cap), oracle: scale_lp)
    vec c(n), rel(n), rho(M);
    const double tr0 = Solver::now_ms();
    auto lap = [&](const char* what) {
        if (!h->knobs.verbose) return;
        HIPCHK(asmb::sync(h->stream));
        static thread_local double last = 0.0;
        const double t = Solver::now_ms();
        std::fprintf(stderr, "[asm] solve_raw %-10s +%.2f ms\n", what, t - (last > tr0 ? last : tr0));
        last = t;
    };
    asmb::barrier(20);
    sv.dev.scaled_matrix(L.lb.data(), L.ub.data(), rel.data(), c.data(), rho.data(), lap);
    sv.dev.tile_flags();
    lap("flags");
    lp.q.resize(n); lp.lb.resize(n); lp.ub.resize(n); lp.r.resize(M); lp.w.resize(lp.ns); lp.slo.resize(lp.ns);
    double qmax = 0.0;
    for (int64_t j = 0; j < n; ++j) { lp.q[j] = L.q[j] * c[j]; qmax = std::max(qmax, std::fabs(lp.q[j])); }
    for (int64_t k = 0; k < lp.ns; ++k) { lp.w[k] = L.w[k] * rho[K.srow[k]]; qmax = std::max(qmax, std::fabs(lp.w[k])); }
    double kap = pow2_round(qmax);
    for (int64_t j = 0; j < n; ++j) { lp.q[j] /= kap; lp.lb[j] = L.lb[j] / c[j]; lp.ub[j] = L.ub[j] / c[j]; }
    for (int64_t k = 0; k < lp.ns; ++k) { lp.w[k] /= kap; lp.slo[k] = L.slo[k] / rho[K.srow[k]]; }
    for (int64_t i = 0; i < M; ++i) lp.r[i] = L.r[i] / rho[i];
    lp.scale_q = 1.0;
    for (double v : lp.q) lp.scale_q = std::max(lp.scale_q, std::fabs(v));
    for (double v : lp.w) lp.scale_q = std::max(lp.scale_q, std::fabs(v));

    Solver::EqpOut o;
    lap("host-lp");
    out.status = sv.solve_scaled(&K.warm[slot], K.hint[slot]);
    lap("solve");
    asmb::barrier(900);
    if (out.status == ASM_OPTIMAL) {
        sv.as_download(o, out.as);
        const ActiveSet& prev = K.warm[slot];
        K.hint[slot].stable = prev.valid && prev.rowst == out.as.rowst && prev.bst == out.as.bst && prev.sst == out.as.sst;
        K.warm[slot] = out.as;
        K.last = out.as;
        // unscale - bound-active components are exactly on their bound
        out.p.resize(n); out.z.resize(n); out.y.resize(M); out.s.resize(lp.ns);
        for (int64_t j = 0; j < n; ++j) {
            double pj = o.p[j] * c[j];
            pj = std::min(std::max(pj, L.lb[j]), L.ub[j]);
            if (out.as.bst[j] < 0) pj = L.lb[j];
            else if (out.as.bst[j] > 0) pj = L.ub[j];
            out.p[j] = pj;
            out.z[j] = o.z[j] * kap / c[j];                  // z = q - J'y  ==  kap * zhat / c
        }
        for (int64_t i = 0; i < M; ++i) {
            double yi = o.y[i] * kap / rho[i];
            // multipliers with the sign their row type admits (a simplex code returns sign-feasible duals)
            if (K.rtype[i] == 1) yi = std::max(yi, 0.0);
            else if (K.rtype[i] == -1) yi = std::min(yi, 0.0);
            out.y[i] = yi;
        }
        for (int64_t k = 0; k < lp.ns; ++k) out.s[k] = o.s[k] * rho[K.srow[k]];
    } else {
        K.last = ActiveSet();
    }
    lap("extract");
    sv.dev.resolve_timing();
    lap("timing");
    check_panel_timeout(h);
    lap("ptmo");
}

void do_solve(asm_handle* h, double delta, int feasibility, double* p_out, double* lambda, double* mult_x_U, double* mult_x_L,
              double* p_slack, int32_t* status) {
    const Skeleton& K = sk_of(h, "inputs have not been uploaded");
    if (!p_out || (K.m > 0 && (!lambda || !p_slack)) || !mult_x_U || !mult_x_L || !status) throw std::invalid_argument("asm_sublp_solve: null output pointer");
    if (!(delta >= 0.0)) throw std::invalid_argument("asm_sublp_solve: delta must be >= 0");
    if (!K.inputs_ready) throw std::logic_error("inputs have not been uploaded");
    HIPCHK(hipSetDevice(h->device));
    auto t0 = std::chrono::steady_clock::now();
    const int64_t n = K.n, m = K.m, M = K.M;
    const bool fr = feasibility != 0;
    LpRaw L;
    L.slacks = fr;
    // trust region intersected with the variable bounds (subproblem.jl:427-434)
    L.lb.resize(n); L.ub.resize(n);
    for (int64_t j = 0; j < n; ++j) {
        L.ub[j] = std::min(delta, K.v_ub[j] - K.x_k[j]);
        L.lb[j] = std::max(-delta, K.v_lb[j] - K.x_k[j]);
    }
    // feasibility-restoration shift (subproblem.jl:287-295) and slack lower bounds (:298-381)
    vec b(K.E);
    if (fr) {
        L.slo.reserve(K.ns);
        for (int64_t i = 0; i < m; ++i) {
            double v = 0.0;
            if (K.E[i] > K.c_ub[i]) v = K.c_ub[i] - K.E[i];
            else if (K.E[i] < K.c_lb[i]) v = K.c_lb[i] - K.E[i];
            b[i] -= std::fabs(v);
            if (K.nslack[i] == 2) {
                if (v < 0) { L.slo.push_back(0.0); L.slo.push_back(v); }
                else { L.slo.push_back(-v); L.slo.push_back(0.0); }
            } else {
                L.slo.push_back(-std::fabs(v));
            }
        }
    }
    // right-hand sides (subproblem.jl:461-484)
    L.r.resize(M);
    for (int64_t i = 0; i < m; ++i) L.r[i] = K.kind[i] == -1 ? K.c_ub[i] - b[i] : K.c_lb[i] - b[i];
    for (int64_t k = 0; k < K.nadj; ++k) L.r[m + k] = K.c_ub[K.adj[k]] - b[K.adj[k]];
    // objective (subproblem.jl:250-272 | 384-405)
    L.q.assign(n, 0.0);
    L.w.assign(fr ? K.ns : 0, 1.0);
    if (!fr) L.q = K.df;

    LpSol sol;
    solve_raw(h, L, fr ? 1 : 0, sol);
    *status = sol.status;
    for (int64_t j = 0; j < n; ++j) { p_out[j] = 0.0; mult_x_U[j] = 0.0; mult_x_L[j] = 0.0; }
    for (int64_t i = 0; i < m; ++i) { lambda[i] = 0.0; p_slack[2 * i] = 0.0; p_slack[2 * i + 1] = K.nslack[i] == 2 ? 0.0 : std::nan(""); }
    if (sol.status == ASM_OPTIMAL) {
        for (int64_t j = 0; j < n; ++j) p_out[j] = sol.p[j];                                    // subproblem.jl:502
        if (fr) {
            int64_t k = 0;
            for (int64_t i = 0; i < m; ++i)
                for (int t = 0; t < K.nslack[i]; ++t, ++k) p_slack[2 * i + t] = sol.s[k];       // :503-505
        }
        for (int64_t i = 0; i < m; ++i) lambda[i] = sol.y[i];                                   // :510-512
        for (int64_t k = 0; k < K.nadj; ++k) lambda[K.adj[k]] += sol.y[m + k];                // :513-515
        for (int64_t j = 0; j < n; ++j) {                                                       // :519-529
            bool fixed = L.ub[j] <= L.lb[j];
            double mL = sol.as.bst[j] < 0 ? std::max(sol.z[j], 0.0) : 0.0;
            double mU = sol.as.bst[j] > 0 ? std::min(sol.z[j], 0.0) : 0.0;
            if (fixed) { mU = std::min(sol.z[j], 0.0); mL = std::max(sol.z[j], 0.0); }      // a fixed column reports both halves of its reduced cost
            if (p_out[j] < K.v_ub[j] - K.x_k[j]) mU = 0.0;
            if (p_out[j] > K.v_lb[j] - K.x_k[j]) mL = 0.0;
            mult_x_L[j] = mL;
            mult_x_U[j] = mU;
        }
    }
    h->stats.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The LP itself, as an MOI optimizer receives it from the reference (subproblem.jl:250-484): for AsmHip.Optimizer
void do_lp_solve(asm_handle* h, const double* dE, const double* q, const double* r, const double* lb, const double* ub, int use_slacks,
                 const double* w, const double* slo, double* p, double* s, double* y, double* z, int32_t* bound_state, int32_t* status) {
    Skeleton& K = sk_of(h, "asm_lp_solve: asm_sublp_setup first");
    HIPCHK(hipSetDevice(h->device));
    auto t0 = std::chrono::steady_clock::now();
    const int64_t n = K.n, M = K.M;
    for (int64_t j = 0; j < n; ++j)
        if (!(lb[j] > -INF && ub[j] < INF && lb[j] <= ub[j])) throw std::invalid_argument("asm_lp_solve: every structural column needs a finite box (the trust region)");
    HIPCHK(asmb::copy_async(K.d_dE, dE, K.nnz * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(asmb::sync(h->stream));
    K.J_valid = false;
    LpRaw L;
    L.slacks = use_slacks != 0;
    L.q.assign(q, q + n); L.r.assign(r, r + M); L.lb.assign(lb, lb + n); L.ub.assign(ub, ub + n);
    if (L.slacks) { L.w.assign(w, w + K.ns); L.slo.assign(slo, slo + K.ns); }
    LpSol sol;
    solve_raw(h, L, L.slacks ? 1 : 0, sol);
    *status = sol.status;
    for (int64_t j = 0; j < n; ++j) { p[j] = 0.0; z[j] = 0.0; if (bound_state) bound_state[j] = 0; }
    for (int64_t i = 0; i < M; ++i) y[i] = 0.0;
    if (s) for (int64_t k = 0; k < K.ns; ++k) s[k] = L.slacks ? slo[k] : 0.0;
    if (sol.status == ASM_OPTIMAL) {
        for (int64_t j = 0; j < n; ++j) { p[j] = sol.p[j]; z[j] = sol.z[j]; if (bound_state) bound_state[j] = sol.as.bst[j]; }
        for (int64_t i = 0; i < M; ++i) y[i] = sol.y[i];
        if (s && L.slacks) for (int64_t k = 0; k < K.ns; ++k) s[k] = sol.s[k];
    }
    h->stats.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// what a batch slot threw in one step (in_slot): the exception unchanged, and where it happened for the message
struct SlotError { std::exception_ptr e; const char* step; int slot; };

// The one map from the exception being handled to an ASM_ERR_* code, its message into `err`.  The internals throw HipError or
// asmb::BatchError for a device failure, Unsupported for input the library cannot represent, std::invalid_argument for bad input and
// std::logic_error for a missing earlier call.
int error_code(std::string& err) {
    try {
        throw;
    } catch (const SlotError& s) {
        try { std::rethrow_exception(s.e); } catch (...) {
            const int rc = error_code(err);
            err = std::string(s.step) + " (slot " + std::to_string(s.slot) + "): " + err;
            return rc;
        }
    } catch (const HipError& e) { err = e.what(); return ASM_ERR_HIP; }
    catch (const asmb::BatchError& e) { err = e.what(); return ASM_ERR_HIP; }
    catch (const Unsupported& e) { err = e.what(); return ASM_ERR_UNSUPPORTED; }
    catch (const std::invalid_argument& e) { err = e.what(); return ASM_ERR_ARG; }
    catch (const std::logic_error& e) { err = e.what(); return ASM_ERR_STATE; }
    catch (const std::exception& e) { err = e.what(); return ASM_ERR_ARG; }
}

// the body of an entry on a handle or a batch: ASM_OK, or the code of what fn() throws (message in the owner's err)
template <class Owner, class F>
int guarded(Owner* o, F&& fn) {
    if (!o) return ASM_ERR_ARG;
    try { fn(); } catch (...) { return error_code(o->err); }
    return ASM_OK;
}

// one slot's part of batch step `step`: what it throws keeps its type, so the batch entry returns the per-handle entry's code
template <class F>
void in_slot(const char* step, int slot, F&& fn) {
    try { fn(); } catch (...) { throw SlotError{std::current_exception(), step, slot}; }
}

// kernels of one evaluation at the point in `xd`: values into Ed (m), objective into fd, optionally gradient / Jacobian values
// `ntrial` > 1 (values only): the trial points of a batched line search, xd / Ed / fd advancing by ldx / ldE / 1 per point
void ev_launch(asm_handle* h, const double* xd, double* Ed, double* fd, bool full, int ntrial = 1, int64_t ldx = 0, int64_t ldE = 0) {
    const EvalState& e = *h->ev;
    const FnStore& F = e.F;
    const unsigned nt = (unsigned)ntrial;
    fn_rows_launch(e, h->stream, xd, Ed, h->sk->d_dE, full ? 1 : 0, nt, ldx, ldE);
    if (!nlp_has_objective(e)) {
        asmb::launch(k_fn_objective, dim3(nt), dim3(256), h->stream, F, xd, fd, ldx);
        if (full) asmb::launch(k_fn_gradient, asmb::blocks(h->sk->n), dim3(256), h->stream, F, xd, e.d_df);
    }
    nlp_rows_launch(e, h->stream, xd, Ed, h->sk->d_dE, full ? 1 : 0, nt, ldx, ldE);
    nlp_objective_launch(e, h->stream, xd, fd, full ? 1 : 0, nt, ldx);
}
// the evaluation results and the bounds for the reduction kernels; norms: also what k_slp_norms alone reads
SlpVecs ev_vecs(const EvalState& e, bool norms = false) {
    const EvLayout& L = e.L;
    SlpVecs V{};
    V.g_L = L.g_L(); V.g_U = L.g_U(); V.x_L = L.x_L(); V.x_U = L.x_U();
    V.E = e.d_E; V.x = e.d_x; V.df = e.d_df; V.n = L.n; V.m = L.m;
    if (norms) { V.lam = L.lam(); V.mU = L.mU(); V.mL = L.mL(); V.jtl = L.jtl(); V.rown = L.rown(); }
    return V;
}
// nu | the slacks (2 per row, as asm_sublp_solve returns them) | p of a step into the block: one copy.  Returns the evaluator
const EvalState& ev_stage_step(asm_handle* h, const double* nu, const double* p_slack, const double* p) {
    const EvLayout& L = h->ev->L;
    double* st = h->ev->h_stage;    // the image of the block from nu on
    if (L.m) { std::memcpy(st, nu, L.m * sizeof(double)); std::memcpy(st + (L.ps() - L.nu()), p_slack, 2 * L.m * sizeof(double)); }
    std::memcpy(st + (L.p() - L.nu()), p, L.n * sizeof(double));
    HIPCHK(asmb::copy_async(L.nu(), st, (L.jtl() - L.nu()) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return *h->ev;
}
}  // namespace

// =========================================================================================================
// C ABI
// =========================================================================================================
extern "C" {

int asm_create(int device, asm_handle** out) {
    if (!out) return ASM_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return ASM_ERR_HIP;
    asm_handle* h = new (std::nothrow) asm_handle();
    if (!h) return ASM_ERR_ARG;
    h->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&h->stream) != hipSuccess ||
        hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, -1) != hipSuccess ||   // look-ahead chain: high priority
        hipStreamCreateWithFlags(&h->stream_ns, hipStreamNonBlocking) != hipSuccess) {         // side stream of the null-space iterations
        if (h->stream2) (void)hipStreamDestroy(h->stream2);
        if (h->stream) (void)hipStreamDestroy(h->stream);
        delete h;
        return ASM_ERR_HIP;
    }
    std::memset(&h->kstats, 0, sizeof(h->kstats));
    std::memset(&h->stats, 0, sizeof(h->stats));
    h->knobs = read_knobs();
    h->timing = h->knobs.timing;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 16) { h->num_cus = prop.multiProcessorCount; h->panel_wgs = 2 * prop.multiProcessorCount - 32; }
        if (h->knobs.panel_wgs > 0) h->panel_wgs = h->knobs.panel_wgs;
        h->panel_wgs_dev = h->panel_wgs;
    }
    *out = h;
    return ASM_OK;
}

int asm_destroy(asm_handle* h) {
    if (!h) return ASM_ERR_ARG;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)asmb::sync(h->stream);
    if (h->stream2) (void)asmb::sync(h->stream2);   // look-ahead chain may still be running after an exception
    if (h->stream_ns) (void)asmb::sync(h->stream_ns);   // ... and the head of a null-space iteration whose join was never reached
    for (auto& r : h->regions) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : h->event_pool) (void)hipEventDestroy(e);
    h->ev.reset(); h->sk.reset();
    for (auto e : h->la_events) (void)hipEventDestroy(e);
    for (auto e : h->s0_events) (void)hipEventDestroy(e);
    if (h->ns_fork) (void)hipEventDestroy(h->ns_fork);
    if (h->ns_join) (void)hipEventDestroy(h->ns_join);
    if (!h->batch_slot) {
        if (h->stream_ns) (void)hipStreamDestroy(h->stream_ns);
        if (h->stream2) (void)hipStreamDestroy(h->stream2);
        if (h->stream) (void)hipStreamDestroy(h->stream);
    }
    delete h;
    return ASM_OK;
}

const char* asm_last_error(const asm_handle* h) { return h ? h->err.c_str() : "null handle"; }

int asm_sublp_setup(asm_handle* h, int64_t n, int64_t m, int64_t nnz, const int64_t* j_row, const int64_t* j_col,
                    const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub) {
    return guarded(h, [&] { do_setup(h, n, m, nnz, j_row, j_col, c_lb, c_ub, v_lb, v_ub); });
}

int asm_sublp_set_bounds(asm_handle* h, const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub) {
    return guarded(h, [&] { do_set_bounds(h, c_lb, c_ub, v_lb, v_ub); });
}

int asm_sublp_upload(asm_handle* h, const double* dE, const double* df, double f, const double* E, const double* x_k) {
    return guarded(h, [&] { do_upload(h, dE, df, f, E, x_k); });
}

int asm_sublp_solve_resident(asm_handle* h, double delta, int feasibility, double* p, double* lambda, double* mult_x_U,
                             double* mult_x_L, double* p_slack, int32_t* status) {
    return guarded(h, [&] { do_solve(h, delta, feasibility, p, lambda, mult_x_U, mult_x_L, p_slack, status); });
}

int asm_sublp_solve(asm_handle* h, const double* dE, const double* df, double f, const double* E, const double* x_k, double delta,
                    int feasibility, double* p, double* lambda, double* mult_x_U, double* mult_x_L, double* p_slack,
                    int32_t* status) {
    return guarded(h, [&] {
        do_upload(h, dE, df, f, E, x_k);
        do_solve(h, delta, feasibility, p, lambda, mult_x_U, mult_x_L, p_slack, status);
    });
}

int asm_lp_solve(asm_handle* h, const double* dE, const double* q, const double* r, const double* lb, const double* ub, int use_slacks,
                 const double* w, const double* slo, double* p, double* s, double* y, double* z, int32_t* bound_state, int32_t* status) {
    return guarded(h, [&] {
        const Skeleton& K = sk_of(h, "asm_lp_solve: asm_sublp_setup first");
        if ((K.nnz > 0 && !dE) || !q || (K.M > 0 && (!r || !y)) || !lb || !ub || !p || !z || !status || (use_slacks && (!w || !slo)))
            throw std::invalid_argument("asm_lp_solve: null pointer");
        do_lp_solve(h, dE, q, r, lb, ub, use_slacks, w, slo, p, s, y, z, bound_state, status);
    });
}

int asm_sublp_active_set(const asm_handle* h, int32_t* row_state, int32_t* bound_state, int32_t* slack_state, int64_t* n_rows,
                         int64_t* n_slack) {
    if (!h) return ASM_ERR_ARG;
    if (!h->sk || !h->sk->last.valid) return ASM_ERR_STATE;
    const ActiveSet& last = h->sk->last;
    if (n_rows) *n_rows = (int64_t)last.rowst.size();
    if (n_slack) *n_slack = (int64_t)last.sst.size();
    if (row_state) for (size_t i = 0; i < last.rowst.size(); ++i) row_state[i] = last.rowst[i];
    if (bound_state) for (size_t i = 0; i < last.bst.size(); ++i) bound_state[i] = last.bst[i];
    if (slack_state) for (size_t i = 0; i < last.sst.size(); ++i) slack_state[i] = last.sst[i];
    return ASM_OK;
}

int asm_sublp_reset_warm(asm_handle* h) {
    if (!h) return ASM_ERR_ARG;
    if (h->sk) reset_warm(*h->sk, false);
    return ASM_OK;
}

int asm_sublp_ns_basis(const asm_handle* h, int32_t* J, int64_t* k) {
    if (!h || !k) return ASM_ERR_ARG;
    *k = h->sk ? (int64_t)h->sk->hint[0].ns_J.size() : 0;        // without a skeleton: as on a new handle
    if (J) for (int64_t a = 0; a < *k; ++a) J[a] = h->sk->hint[0].ns_J[a];
    return ASM_OK;
}

int asm_sublp_row_order(const asm_handle* h, int32_t* perm, int64_t* band, int32_t* e_rows, int64_t* n_e, int64_t* e_band) {
    if (!h || !band || !n_e || !e_band) return ASM_ERR_ARG;
    const NsForm* F = h->sk ? h->sk->nsf.get() : nullptr;
    *band = h->sk ? h->sk->row_band : 0;                          // without a skeleton: as on a new handle
    if (perm && *band > 0) std::copy(h->sk->row_perm_h.begin(), h->sk->row_perm_h.end(), perm);
    *n_e = F ? F->L.nE : 0;
    *e_band = F ? F->f0.band : 0;
    if (e_rows && F) std::copy(F->eidx_h.begin(), F->eidx_h.end(), e_rows);
    return ASM_OK;
}

int asm_sublp_last_stats(const asm_handle* h, asm_solve_stats* out) {
    if (!h || !out) return ASM_ERR_ARG;
    *out = h->stats;
    return ASM_OK;
}

int asm_kernel_stats_get(asm_handle* h, asm_kernel_stats* out) {
    if (!out) return ASM_ERR_ARG;
    return guarded(h, [&] {
        Dev d(h);
        d.resolve_timing();
        *out = h->kstats;
    });
}

int asm_kernel_timing(asm_handle* h, int level) {
    return guarded(h, [&] {
        if (level < 0 || level > 2) throw std::invalid_argument("asm_kernel_timing: level 0, 1 or 2");
        Dev d(h);
        d.resolve_timing();
        h->timing = h->batch_slot ? 0 : level;
    });
}

int asm_kernel_stats_reset(asm_handle* h) {
    return guarded(h, [&] {
        Dev d(h);
        d.resolve_timing();
        std::memset(&h->kstats, 0, sizeof(h->kstats));
    });
}

// --------------------------------------------------------------------------------- norms on the resident Jacobian
static void do_jac_row_norms(asm_handle* h, double* out_m) {
    if (!out_m) throw std::invalid_argument("asm_jac_row_norms: null pointer");
    const Skeleton& K = sk_of(h, "asm_jac_row_norms: no assembled Jacobian");
    if (!K.inputs_ready) throw std::logic_error("asm_jac_row_norms: no assembled Jacobian");
    HIPCHK(hipSetDevice(h->device));
    Dev d(h);
    d.assemble();
    if (K.m == 0) return;
    d.launch_row_norms(K.d_vecM, false);
    d.d2h(out_m, K.d_vecM, K.m);
}

int asm_jac_row_norms(asm_handle* h, double* out_m) {
    return guarded(h, [&] { do_jac_row_norms(h, out_m); });
}

int asm_kt_residuals(asm_handle* h, const double* df, const double* lambda, const double* mult_x_U, const double* mult_x_L, double* out) {
    return guarded(h, [&] {
        const Skeleton& K = sk_of(h, "asm_kt_residuals: no assembled Jacobian");
        if (!df || !mult_x_U || !mult_x_L || !out || (K.m > 0 && !lambda)) throw std::invalid_argument("asm_kt_residuals: null pointer");
        if (!K.inputs_ready) throw std::logic_error("asm_kt_residuals: no assembled Jacobian");
        HIPCHK(hipSetDevice(h->device));
        Dev d(h);
        d.assemble();
        const int64_t n = K.n, m = K.m;
        vec lam(K.M, 0.0), jtl(n), rn(std::max<int64_t>(m, 1));
        for (int64_t i = 0; i < m; ++i) lam[i] = lambda[i];
        d.gemv_t(K.d_J, lam.data(), jtl.data());
        if (m > 0) {
            d.launch_row_norms(K.d_vecM, false);
            d.d2h(rn.data(), K.d_vecM, m);
        }
        // common.jl:38-43
        double res = 0.0, ndf = 0.0;
        for (int64_t j = 0; j < n; ++j) {
            double v = df[j] - jtl[j] - mult_x_U[j] - mult_x_L[j];
            res += v * v;
            ndf += df[j] * df[j];
        }
        double scalar = std::max(1.0, std::sqrt(ndf));
        for (int64_t i = 0; i < m; ++i) scalar = std::max(scalar, std::fabs(lambda[i]) * rn[i]);
        *out = std::sqrt(res) / scalar;
    });
}

// --------------------------------------------------------------------------------- device-side evaluators (rows a2 / f3)
namespace {
// an expression block (include/asm_hip.h, "Expression block") validated into its host-side form xh
void expr_prepare(const asm_handle* h, ExprHost& xh, int64_t n_rows, int64_t fn_nnz, int64_t nlp_rows, int64_t nlp_nnz, const int64_t* ip, int64_t n_ipar,
                  int64_t n_dpar) {
    auto bad = [](const std::string& what) { throw std::invalid_argument("asm_eval_setup: expression block: " + what); };
    if (!ip || n_ipar < 3) bad("ipar too short");
    const int64_t R = ip[0], T = ip[1], L = ip[2], n = h->sk->n;
    if (R != nlp_rows) bad("ipar[0] (rows) differs from nlp_rows");
    if (R < 0 || T < 0 || L < 0 || L > (int64_t)1 << 40 || R + T > L) bad("bad row / term / node count");
    if (n_ipar != 3 + R + T + 1 + 3 * L) bad("ipar size differs from 3 + R + T + 1 + 3 L");
    const int64_t *ptr = ip + 3, *op = ptr + R + T + 1, *a = op + L, *b = a + L;
    if (ptr[0] != 0 || ptr[R + T] != L) bad("ptr must run from 0 to L");
    for (int64_t r = 0; r < R + T; ++r)
        if (ptr[r + 1] <= ptr[r]) bad("row / term " + std::to_string(r) + " has no nodes");
    xh.R = R; xh.T = T; xh.L = L;
    xh.ptr.assign(ptr, ptr + R + T + 1);
    xh.op.resize(L); xh.a.resize(L); xh.b.resize(L); xh.slot.assign(L, -1);
    for (int64_t r = 0; r < R + T; ++r) {
        const int64_t k0 = ptr[r];
        for (int64_t k = k0; k < ptr[r + 1]; ++k) {
            const int64_t o = op[k], ka = a[k], kb = b[k], loc = k - k0;
            const std::string at = "node " + std::to_string(loc) + " of " + (r < R ? "row " + std::to_string(r) : "term " + std::to_string(r - R));
            if (o < ASM_OP_CONST || o >= ASM_OP_COUNT) bad(at + ": unknown op " + std::to_string(o));
            int64_t aa = ka, bb = 0;
            if (o == ASM_OP_CONST) {
                if (ka < 0 || ka >= n_dpar) bad(at + ": constant index out of range");
            } else if (o == ASM_OP_VAR) {
                if (ka < 0 || ka >= n) bad(at + ": variable out of range");
            } else {
                if (ka < 0 || ka >= loc) bad(at + ": operand a is not an earlier node of its row");
                aa = k0 + ka;
                if ((o >= ASM_OP_ADD && o <= ASM_OP_DIV) || (o >= ASM_OP_POW && o <= ASM_OP_MAX)) {
                    if (kb < 0 || kb >= loc) bad(at + ": operand b is not an earlier node of its row");
                    bb = k0 + kb;
                } else if (o == ASM_OP_POWI) {
                    if (kb == 0 || kb < -ASM_EXPR_MAX_POWI || kb > ASM_EXPR_MAX_POWI) bad(at + ": POWI exponent must be a nonzero integer of magnitude <= 64");
                    bb = kb;
                }
            }
            xh.op[k] = (int32_t)o; xh.a[k] = aa; xh.b[k] = bb;
        }
    }
    // Jacobian pattern: each row's distinct variables ascending; it must be the block's part of j_str
    xh.jptr.assign(1, 0);
    std::vector<int64_t> vars;
    for (int64_t r = 0; r < R; ++r) {
        vars.clear();
        for (int64_t k = ptr[r]; k < ptr[r + 1]; ++k)
            if (op[k] == ASM_OP_VAR) vars.push_back(a[k]);
        std::sort(vars.begin(), vars.end());
        vars.erase(std::unique(vars.begin(), vars.end()), vars.end());
        const int64_t j0 = xh.jptr.back();
        if (j0 + (int64_t)vars.size() > nlp_nnz) bad("nlp_nnz is smaller than the pattern of the rows");
        for (size_t q = 0; q < vars.size(); ++q) {
            const int64_t e = fn_nnz + j0 + (int64_t)q;
            if (h->sk->j_row_h[e] != n_rows + r + 1 || h->sk->j_col_h[e] != vars[q] + 1)
                bad("j_str entry " + std::to_string(e + 1) + " differs from the pattern of row " + std::to_string(r) + " (its distinct variables, ascending)");
        }
        for (int64_t k = ptr[r]; k < ptr[r + 1]; ++k)
            if (op[k] == ASM_OP_VAR) xh.slot[k] = j0 + (std::lower_bound(vars.begin(), vars.end(), a[k]) - vars.begin());
        xh.jptr.push_back(j0 + (int64_t)vars.size());
    }
    if (xh.jptr.back() != nlp_nnz) bad("nlp_nnz differs from the size of the rows' pattern");
    // objective terms: the VAR nodes grouped by variable, in (term, node) order inside each group
    xh.gptr.assign(n + 1, 0);
    for (int64_t k = ptr[R]; k < L; ++k)
        if (op[k] == ASM_OP_VAR) ++xh.gptr[a[k] + 1];
    for (int64_t j = 0; j < n; ++j) xh.gptr[j + 1] += xh.gptr[j];
    std::vector<int64_t> fill(xh.gptr.begin(), xh.gptr.end() - 1);
    for (int64_t k = ptr[R]; k < L; ++k)
        if (op[k] == ASM_OP_VAR) xh.slot[k] = fill[a[k]]++;
    // data gradient: the CONST nodes of rows and terms grouped by dpar index, in node order inside each group
    int64_t n_const = 0;
    for (int64_t k = 0; k < L; ++k) n_const += op[k] == ASM_OP_CONST;
    if (n_const == 0) return;
    xh.cptr.assign(n_dpar + 1, 0);
    for (int64_t k = 0; k < L; ++k)
        if (op[k] == ASM_OP_CONST) ++xh.cptr[a[k] + 1];
    for (int64_t c = 0; c < n_dpar; ++c) xh.cptr[c + 1] += xh.cptr[c];
    std::vector<int64_t> cfill(xh.cptr.begin(), xh.cptr.end() - 1);
    for (int64_t k = 0; k < L; ++k)
        if (op[k] == ASM_OP_CONST) xh.slot[k] = cfill[a[k]]++;
}
}  // namespace

static void do_eval_setup(asm_handle* h, int64_t n_rows, const int64_t* aff_ptr, const int64_t* aff_var, const double* aff_coef, const int64_t* quad_ptr,
                          const int64_t* q_v1, const int64_t* q_v2, const double* q_coef, const double* constant, const int64_t* jac_off,
                          const int64_t* g_ptr, const int64_t* g_kind, const double* g_coef, const int64_t* g_other, double objective_scale, int nlp_kind,
                          int64_t nlp_rows, int64_t nlp_nnz, const int64_t* nlp_ipar, int64_t n_ipar, const double* nlp_dpar, int64_t n_dpar) {
    const Skeleton& K = sk_of(h, "asm_eval_setup: asm_sublp_setup first (it fixes n, m and the j_str order of dE)");
    if (n_rows < 0 || !aff_ptr || !quad_ptr || !constant || !jac_off || !g_ptr || nlp_kind < ASM_NLP_NONE || nlp_kind > ASM_NLP_DENSE_QUADRATIC_HESS)
        throw std::invalid_argument("asm_eval_setup: bad argument");
    const int64_t fn_nnz = jac_off[n_rows];
    if (n_rows + nlp_rows != K.m || fn_nnz + nlp_nnz != K.nnz)
        throw std::invalid_argument("asm_eval_setup: row / Jacobian-entry counts do not match asm_sublp_setup");
    nlp_check_sizes(nlp_kind, K.n, nlp_rows, nlp_nnz, n_ipar, n_dpar);
    ExprHost xh;
    if (nlp_family(nlp_kind) == NlpFamily::EXPR) expr_prepare(h, xh, n_rows, fn_nnz, nlp_rows, nlp_nnz, nlp_ipar, n_ipar, n_dpar);   // all checks before any state changes
    HIPCHK(hipSetDevice(h->device));
    h->lm.drop();
    h->ev.reset();                  // the old evaluator goes before the new one is made; a failure below leaves the handle without one
    auto e = std::make_unique<EvalState>();
    BufPool& P = e->mem;
    FnStore& F = e->F;
    F.n_rows = n_rows; F.n = K.n; F.objective_scale = objective_scale;
    const int64_t na = aff_ptr[n_rows + 1], nq = quad_ptr[n_rows + 1], ng = g_ptr[K.n];
    P.upload(F.aff_ptr, aff_ptr, n_rows + 2); P.upload(F.aff_var, aff_var, na); P.upload(F.aff_coef, aff_coef, na);
    P.upload(F.quad_ptr, quad_ptr, n_rows + 2); P.upload(F.q_v1, q_v1, nq); P.upload(F.q_v2, q_v2, nq); P.upload(F.q_coef, q_coef, nq);
    P.upload(F.constant, constant, n_rows + 1); P.upload(F.jac_off, jac_off, n_rows + 1);
    P.upload(F.g_ptr, g_ptr, K.n + 1); P.upload(F.g_kind, g_kind, ng); P.upload(F.g_coef, g_coef, ng); P.upload(F.g_other, g_other, ng);
    e->nlp_rows = nlp_rows; e->fn_nnz = fn_nnz; e->n_dpar = n_dpar;
    P.upload(e->d_ipar, nlp_ipar, n_ipar); P.upload(e->d_dpar, nlp_dpar, n_dpar);
    const int64_t n = K.n, m = K.m;      // (the pool makes an empty vector one element long)
    P.zeroed(e->d_x, n); P.zeroed(e->d_xt, 8 * round_up(n, 32)); P.zeroed(e->d_df, n); P.zeroed(e->d_E, m);
    P.zeroed(e->d_Et, 8 * round_up(std::max<int64_t>(m, 1), 32)); P.zeroed(e->d_f, 16);      // xt / Et / f[1..8]: eight trial points of the batched line search
    nlp_setup(*e, nlp_kind, xh, nlp_ipar);
    e->L = EvLayout{n, m, K.ldn, K.Mp};      // the reductions' block with the bounds in it, and the staging buffer
    P.zeroed(e->L.d, e->L.len());
    ev_write_bounds(h, e->L);
    P.alloc(e->h_stage, e->L.stage_len(), BufPool::PINNED);
    h->ev = std::move(e);
}

int asm_eval_setup(asm_handle* h, int64_t n_rows, const int64_t* aff_ptr, const int64_t* aff_var, const double* aff_coef, const int64_t* quad_ptr,
                   const int64_t* q_v1, const int64_t* q_v2, const double* q_coef, const double* constant, const int64_t* jac_off,
                   const int64_t* g_ptr, const int64_t* g_kind, const double* g_coef, const int64_t* g_other, double objective_scale, int nlp_kind,
                   int64_t nlp_rows, int64_t nlp_nnz, const int64_t* nlp_ipar, int64_t n_ipar, const double* nlp_dpar, int64_t n_dpar) {
    return guarded(h, [&] {
        do_eval_setup(h, n_rows, aff_ptr, aff_var, aff_coef, quad_ptr, q_v1, q_v2, q_coef, constant, jac_off, g_ptr, g_kind, g_coef, g_other, objective_scale,
                      nlp_kind, nlp_rows, nlp_nnz, nlp_ipar, n_ipar, nlp_dpar, n_dpar);
    });
}

// eval_functions! (slp.jl:186-191) on the device + what asm_sublp_upload does with the results: dE stays in HBM
static void do_eval_functions(asm_handle* h, const double* x, double* f, double* df, double* E) {
    EvalState& e = ev_of(h, "asm_eval_functions");
    if (!x || !f || !df || (h->sk->m > 0 && !E)) throw std::invalid_argument("asm_eval_functions: null pointer");
    HIPCHK(hipSetDevice(h->device));
    const int64_t n = h->sk->n, m = h->sk->m;
    double *st = e.h_stage, *s_df = st + e.L.st_df(), *s_E = st + e.L.st_E(true), *s_f = st + e.L.st_f(true);
    std::memcpy(st, x, n * sizeof(double));
    HIPCHK(asmb::copy_async(e.d_x, st, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    ev_launch(h, e.d_x, e.d_E, e.d_f, true);
    HIPCHK(asmb::copy_async(s_df, e.d_df, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (m) HIPCHK(asmb::copy_async(s_E, e.d_E, m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(asmb::copy_async(s_f, e.d_f, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(asmb::sync(h->stream));
    std::memcpy(df, s_df, n * sizeof(double));
    if (m) std::memcpy(E, s_E, m * sizeof(double));
    *f = *s_f;
    h->sk->df.assign(df, df + n); h->sk->E.assign(E, E + m); h->sk->x_k.assign(x, x + n);
    h->sk->f = *f;
    h->sk->inputs_ready = true;
    h->sk->inputs_from_eval = true;
    h->sk->J_valid = false;
}

int asm_eval_functions(asm_handle* h, const double* x, double* f, double* df, double* E) {
    return guarded(h, [&] { do_eval_functions(h, x, f, df, E); });
}

// dpar[offset, offset + count) := values on the device: every later evaluation reads it, nothing else changes
static void do_set_data(asm_handle* h, int64_t offset, int64_t count, const double* values) {
    EvalState& e = ev_of(h, "asm_eval_set_data");
    if (!values || offset < 0 || count < 0 || offset > e.n_dpar - count)
        throw std::invalid_argument("asm_eval_set_data: null pointer or a range outside [0, n_dpar = " + std::to_string(e.n_dpar) + ")");
    if (count == 0) return;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(asmb::copy_async(e.d_dpar + offset, values, count * sizeof(double), hipMemcpyHostToDevice, h->stream));
    h2d_done(h);
    if (e.dirty_hi == e.dirty_lo) { e.dirty_lo = offset; e.dirty_hi = offset + count; }
    else { e.dirty_lo = std::min(e.dirty_lo, offset); e.dirty_hi = std::max(e.dirty_hi, offset + count); }
}

// the kinds with data derivatives: expression blocks and the block kernels that announce their derivative entries (kinds 4 and 5)
static void data_kind_check(const EvalState& e, const char* who, const char* what) {
    if (!e.has_data) throw std::invalid_argument(std::string(who) + ": " + what + " exist for expression blocks (nlp_kind 3) only");
    if (!e.ohm_vars_ok) throw std::invalid_argument(std::string(who) + ": the Ohm's-law block names a variable outside [0, n)");
}
// out[c] = d(f - lambda' g) / d dpar[c] at x (nlp_data_grad_launch); the inputs of the next LP are not touched (x goes where
// asm_eval_constraints puts its trial point)
static void do_data_gradient(asm_handle* h, const double* x, const double* lambda, double* out) {
    EvalState& e = ev_of(h, "asm_eval_data_gradient");
    data_kind_check(e, "asm_eval_data_gradient", "data gradients");
    if (!x || (h->sk->m > 0 && !lambda) || (e.n_dpar > 0 && !out)) throw std::invalid_argument("asm_eval_data_gradient: null pointer");
    const int64_t n = h->sk->n, nd = e.n_dpar, R = e.nlp_rows;
    if (!e.data_dep) {          // nothing depends on the data
        for (int64_t c = 0; c < nd; ++c) out[c] = 0.0;
        return;
    }
    HIPCHK(hipSetDevice(h->device));
    double *st = e.h_stage, *s_lam = st + e.L.st_lam();
    std::memcpy(st, x, n * sizeof(double));
    HIPCHK(asmb::copy_async(e.d_xt, st, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (R > 0) {                // (a tape of objective terms alone has no rows)
        std::memcpy(s_lam, lambda + e.F.n_rows, R * sizeof(double));
        HIPCHK(asmb::copy_async(e.d_lam, s_lam, R * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    nlp_data_grad_launch(e, h->stream);
    HIPCHK(asmb::copy_async(e.h_dgrad, e.d_dgrad, nd * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(asmb::sync(h->stream));
    std::memcpy(out, e.h_dgrad, nd * sizeof(double));
}

// ---- Hessian of the Lagrangian (include/asm_hip.h, "Hessian of the Lagrangian")
namespace {
// pattern, seed threads, occurrence and product lists of h's store and tape (downloaded with blocking copies: not inside a batch fiber) into sh
void hs_build(const asm_handle* h, HsShared& sh) {
    HIPCHK(hipSetDevice(h->device));
    const FnStore& F = h->ev->F;
    const int64_t nr = F.n_rows, n = h->sk->n;
    // 1. function store: the objective row's quadratic terms (unless the block has the objective), then the rows' in row order
    const std::vector<int64_t> qptr = hs_download(F.quad_ptr, nr + 2);
    const std::vector<int64_t> q1 = hs_download(F.q_v1, qptr[nr + 1]), q2 = hs_download(F.q_v2, qptr[nr + 1]);
    std::vector<int64_t> rows, cols, qterm, qrow;
    auto store_row = [&](int64_t r, int64_t tag) {
        for (int64_t k = qptr[r]; k < qptr[r + 1]; ++k) { rows.push_back(q1[k] + 1); cols.push_back(q2[k] + 1); qterm.push_back(k); qrow.push_back(tag); }
    };
    if (!nlp_has_objective(*h->ev)) store_row(nr, -1);
    for (int64_t r = 0; r < nr; ++r) store_row(r, r);
    const int64_t nfn = (int64_t)rows.size();
    // 2. the block: its seed threads, occurrences and the entries its launch writes in place
    const HsBlockLists B = nlp_hess_lists(*h->ev);
    const int64_t S = (int64_t)B.srow.size(), nocc = (int64_t)B.okey.size();
    // the block's entries: the distinct pairs (i, j), i >= j, sorted by (i, j); every entry's occurrences in list order
    std::vector<int64_t> keys(B.okey);
    keys.insert(keys.end(), B.own.begin(), B.own.end());
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const int64_t nblk = (int64_t)keys.size();
    std::vector<int64_t> eptr(nblk + 1, 0), eocc(nocc), oent(nocc);
    for (int64_t o = 0; o < nocc; ++o) { oent[o] = std::lower_bound(keys.begin(), keys.end(), B.okey[o]) - keys.begin(); ++eptr[oent[o] + 1]; }
    for (int64_t e = 0; e < nblk; ++e) eptr[e + 1] += eptr[e];
    {
        std::vector<int64_t> fill(eptr.begin(), eptr.end() - 1);
        for (int64_t o = 0; o < nocc; ++o) eocc[fill[oent[o]]++] = B.oslot.empty() ? o : B.oslot[o];
    }
    for (int64_t e = 0; e < nblk; ++e) { rows.push_back(keys[e] / n + 1); cols.push_back(keys[e] % n + 1); }
    const int64_t nnz = nfn + nblk;
    // 3. product lists: per variable (entry, other variable) in entry order, an off-diagonal entry in both lists
    std::vector<int64_t> pptr(n + 1, 0);
    for (int64_t e = 0; e < nnz; ++e) {
        if (rows[e] < 1 || rows[e] > n || cols[e] < 1 || cols[e] > n) throw std::invalid_argument("asm_eval_hessian: a quadratic term names a variable outside [0, n)");
        ++pptr[rows[e]];
        if (rows[e] != cols[e]) ++pptr[cols[e]];
    }
    for (int64_t j = 0; j < n; ++j) pptr[j + 1] += pptr[j];
    std::vector<int64_t> pent(pptr[n]), poth(pptr[n]), fill(pptr.begin(), pptr.end() - 1);
    for (int64_t e = 0; e < nnz; ++e) {
        const int64_t r = rows[e] - 1, c = cols[e] - 1;
        pent[fill[r]] = e; poth[fill[r]++] = c;
        if (r != c) { pent[fill[c]] = e; poth[fill[c]++] = r; }
    }
    BufPool& M = sh.mem;
    M.upload(sh.qterm, qterm.data(), nfn); M.upload(sh.qrow, qrow.data(), nfn);
    M.upload(sh.eptr, eptr.data(), nblk + 1); M.upload(sh.eocc, eocc.data(), nocc);
    M.upload(sh.pptr, pptr.data(), n + 1); M.upload(sh.pent, pent.data(), pptr[n]); M.upload(sh.poth, poth.data(), pptr[n]);
    if (S > 0) {
        M.upload(sh.srow, B.srow.data(), S); M.upload(sh.svar, B.svar.data(), S); M.upload(sh.woff, B.woff.data(), S);
        M.upload(sh.optr, B.optr.data(), S + 1); M.upload(sh.ovar, B.ovar.data(), nocc);
    }
    sh.nfn = nfn; sh.wnodes = B.wnodes; sh.S = S; sh.nocc = nocc;
    sh.rows.swap(rows); sh.cols.swap(cols);
}
// the handle's own part on the lists of sh: the four node arrays, hocc and the value / product vectors.  Inside a batch fiber the clearing
// fills are recorded with the slot's other operations
void hs_attach(asm_handle* h, const HsShared* sh) {
    EvalState& e = *h->ev;
    BufPool& M = e.mem;
    const bool rec = asmb::in_fiber();
    auto zeroed = [&](double*& f, int64_t count) { if (rec) M.zeroed(f, count, h->stream); else M.zeroed(f, count); };
    ExprHess& H = e.hs_H;          // (empty: the state is new, or hs_forget cleared it)
    H.S = sh->S;
    if (sh->S > 0) {               // seed threads (a tape): their lists and four node arrays
        H.srow = sh->srow; H.svar = sh->svar; H.woff = sh->woff; H.optr = sh->optr; H.ovar = sh->ovar;
        zeroed(H.val, sh->wnodes); zeroed(H.tval, sh->wnodes); zeroed(H.adj, sh->wnodes); zeroed(H.tadj, sh->wnodes);
    }
    if (sh->nocc > 0) zeroed(H.hocc, sh->nocc);      // the occurrences the block's launch writes, whatever lists them (nlp_hess_lists)
    zeroed(e.d_hs_lam, h->sk->m); zeroed(e.d_hs_v, h->sk->n); zeroed(e.d_hs_vals, sh->nnz()); zeroed(e.d_hs_out, h->sk->n);
    M.alloc(e.h_hs, std::max(sh->nnz(), h->sk->n), BufPool::PINNED);
    e.hs_sh = sh;
}
// once per asm_eval_setup, at the first Hessian call of a handle
void hs_prepare(asm_handle* h) {
    if (h->ev->hs_sh) return;
    HIPCHK(hipSetDevice(h->device));
    auto own = std::make_unique<HsShared>();
    hs_build(h, *own);
    h->ev->hs_own = std::move(own);
    hs_attach(h, h->ev->hs_own.get());
}
void hs_check(const asm_handle* h, const char* who) {
    const EvalState& e = ev_of(h, who);
    if (!e.has_hess)
        throw std::invalid_argument(std::string(who) + ": second derivatives exist for the function store alone (nlp_kind 0) or with an expression block (nlp_kind 3)");
}
// the values at (x, obj_factor, lambda) into d_hs_vals; with v also H v into d_hs_out.  x goes where asm_eval_constraints puts its trial
// point: the inputs of the next LP are not touched
void hs_launch(asm_handle* h, const double* x, double obj_factor, const double* lambda, const double* v) {
    hs_prepare(h);
    HIPCHK(hipSetDevice(h->device));
    EvalState& e = *h->ev;
    const HsShared& L = *e.hs_sh;
    const int64_t n = h->sk->n, m = h->sk->m, nnz = L.nnz(), nfn = L.nfn;
    double *st = e.h_stage, *s_lam = st + e.L.st_lam(), *s_v = st + e.L.st_v();
    std::memcpy(st, x, n * sizeof(double));
    HIPCHK(asmb::copy_async(e.d_xt, st, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (m > 0) {
        std::memcpy(s_lam, lambda, m * sizeof(double));
        HIPCHK(asmb::copy_async(e.d_hs_lam, s_lam, m * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    if (v) {
        std::memcpy(s_v, v, n * sizeof(double));
        HIPCHK(asmb::copy_async(e.d_hs_v, s_v, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    const double wobj = obj_factor * e.F.objective_scale;
    if (nfn > 0) asmb::launch(k_fn_hessian, asmb::blocks(nfn), dim3(256), h->stream, L.qterm, L.qrow, e.F.q_coef, e.d_hs_lam, wobj, nfn, e.d_hs_vals);
    nlp_hess_launch(e, h->stream, L, e.d_hs_lam + e.F.n_rows, wobj, nnz - nfn, e.d_hs_vals + nfn);
    if (v) asmb::launch(k_hess_product, asmb::blocks(n), dim3(256), h->stream, L.pptr, L.pent, L.poth, e.d_hs_vals, e.d_hs_v, n, e.d_hs_out);
}
void hs_pattern(const HsShared& sh, int64_t* nnz, int64_t* rows, int64_t* cols) {
    *nnz = sh.nnz();
    if (rows) {
        std::copy(sh.rows.begin(), sh.rows.end(), rows);
        std::copy(sh.cols.begin(), sh.cols.end(), cols);
    }
}
void hs_read(asm_handle* h, const double* dev, int64_t count, double* out) {
    if (count > 0) HIPCHK(asmb::copy_async(h->ev->h_hs, dev, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(asmb::sync(h->stream));
    if (count > 0) std::memcpy(out, h->ev->h_hs, count * sizeof(double));
}
}  // namespace

static void do_hessian_structure(asm_handle* h, int64_t* nnz, int64_t* rows, int64_t* cols) {
    hs_check(h, "asm_eval_hessian_structure");
    if (!nnz || (rows == nullptr) != (cols == nullptr)) throw std::invalid_argument("asm_eval_hessian_structure: null pointer");
    hs_prepare(h);
    hs_pattern(*h->ev->hs_sh, nnz, rows, cols);
}
static void do_hessian_lagrangian(asm_handle* h, const double* x, double obj_factor, const double* lambda, double* values) {
    hs_check(h, "asm_eval_hessian_lagrangian");
    if (!x || (h->sk->m > 0 && !lambda)) throw std::invalid_argument("asm_eval_hessian_lagrangian: null pointer");
    hs_prepare(h);
    if (h->ev->hs_sh->nnz() > 0 && !values) throw std::invalid_argument("asm_eval_hessian_lagrangian: null pointer");
    hs_launch(h, x, obj_factor, lambda, nullptr);
    hs_read(h, h->ev->d_hs_vals, h->ev->hs_sh->nnz(), values);
}
static void do_hessian_product(asm_handle* h, const double* x, double obj_factor, const double* lambda, const double* v, double* out) {
    hs_check(h, "asm_eval_hessian_product");
    if (!x || !v || !out || (h->sk->m > 0 && !lambda)) throw std::invalid_argument("asm_eval_hessian_product: null pointer");
    hs_launch(h, x, obj_factor, lambda, v);
    hs_read(h, h->ev->d_hs_out, h->sk->n, out);
}

// ---- cross derivatives with respect to the data (include/asm_hip.h, "Cross derivatives of an expression block")
namespace {
void cx_check(const asm_handle* h, const char* who) { data_kind_check(ev_of(h, who), who, "cross derivatives"); }
}  // namespace
// u = d/dc (grad_x L) . dc, w = (dg/dc) . dc at (x, lambda), L = f - lambda' g (nlp_cross_launch on one direction); the inputs of
// the next LP are not touched (x goes where asm_eval_constraints puts its trial point)
static void do_data_cross(asm_handle* h, const double* x, const double* lambda, const double* dc, double* u, double* w) {
    cx_check(h, "asm_eval_data_cross");
    EvalState& e = *h->ev;
    if (!x || !u || (h->sk->m > 0 && (!lambda || !w)) || (e.n_dpar > 0 && !dc)) throw std::invalid_argument("asm_eval_data_cross: null pointer");
    const int64_t n = h->sk->n, m = h->sk->m, nd = e.n_dpar, R = e.nlp_rows;
    for (int64_t j = 0; j < n; ++j) u[j] = 0.0;
    for (int64_t i = 0; i < m; ++i) w[i] = 0.0;
    if (!e.data_dep) return;    // nothing depends on the data
    HIPCHK(hipSetDevice(h->device));
    cx_prepare(e, 1);
    double *st = e.h_cx, *back = st + n + R + nd;      // [x | lam | dc] up in two copies, [u | w] back
    std::memcpy(st, x, n * sizeof(double));
    if (R > 0) std::memcpy(st + n, lambda + e.F.n_rows, R * sizeof(double));
    std::memcpy(st + n + R, dc, nd * sizeof(double));
    HIPCHK(asmb::copy_async(e.d_xt, st, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(asmb::copy_async(e.d_cx_in, st + n, (R + nd) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    nlp_cross_launch(e, h->stream, 1, nullptr, nullptr);
    HIPCHK(asmb::copy_async(back, e.d_cx_out, (n + R) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(asmb::sync(h->stream));
    std::memcpy(u, back, n * sizeof(double));
    if (R > 0) std::memcpy(w + e.F.n_rows, back + n, R * sizeof(double));
}

// ---- transposed cross derivatives (include/asm_hip.h, "Transposed cross derivatives")
namespace {
// OUT [ncol x n_dpar]: row c = the transposed cross derivative at (x, lambda) for the weights (sx * VX[c], VL[c]) (VX ncol x n, VL ncol x m;
// sx = -1 turns an adjoint state's ax into the weight -ax, exactly), in chunks of `cap` columns.  x and the block's multipliers go up once;
// a chunk is one upload, its launches (nlp_cross_t_launch, no synchronisation between columns) and one read-back.  A column's answer
// depends on its own weights only.
void ct_columns(asm_handle* h, const double* x, const double* lambda, int64_t ncol, const double* VX, double sx, const double* VL, double* OUT, int64_t cap) {
    EvalState& e = *h->ev;
    const int64_t n = h->sk->n, m = h->sk->m, nd = e.n_dpar;
    if (!e.data_dep) {          // nothing depends on the data
        for (int64_t q = 0; q < ncol * nd; ++q) OUT[q] = 0.0;
        return;
    }
    HIPCHK(hipSetDevice(h->device));
    ct_prepare(e, cap);
    const hipStream_t s = h->stream;
    const int64_t R = e.nlp_rows, r0 = e.F.n_rows, ldv = n + R;
    double *st = e.h_ct, *s_in = st + n, *back = s_in + R + cap * ldv;
    std::memcpy(st, x, n * sizeof(double));
    if (R > 0) std::memcpy(s_in, lambda + r0, R * sizeof(double));
    HIPCHK(asmb::copy_async(e.d_xt, st, n * sizeof(double), hipMemcpyHostToDevice, s));
    if (R > 0) HIPCHK(asmb::copy_async(e.d_ct_in, s_in, R * sizeof(double), hipMemcpyHostToDevice, s));
    double* dv = e.d_ct_in + R;
    for (int64_t c0 = 0; c0 < ncol; c0 += cap) {
        const int cols = (int)std::min<int64_t>(cap, ncol - c0);
        for (int c = 0; c < cols; ++c) {
            double* sv = s_in + R + (int64_t)c * ldv;
            const double* vx = VX + (c0 + c) * n;
            for (int64_t j = 0; j < n; ++j) sv[j] = sx * vx[j];
            if (R > 0) std::memcpy(sv + n, VL + (c0 + c) * m + r0, R * sizeof(double));
        }
        HIPCHK(asmb::copy_async(dv, s_in + R, (int64_t)cols * ldv * sizeof(double), hipMemcpyHostToDevice, s));
        nlp_cross_t_launch(e, s, cols);
        HIPCHK(asmb::copy_async(back, e.d_ct_out, (int64_t)cols * nd * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(asmb::sync(s));
        std::memcpy(OUT + c0 * nd, back, (int64_t)cols * nd * sizeof(double));
    }
}
}  // namespace
// out[c] = d/d dpar[c] [ D_vx L + vl' g ] at (x, lambda), L = f - lambda' g; the inputs of the next LP are not touched (x goes where
// asm_eval_constraints puts its trial point)
static void do_data_cross_t(asm_handle* h, const double* x, const double* lambda, const double* vx, const double* vl, double* out) {
    cx_check(h, "asm_eval_data_cross_t");
    EvalState& e = *h->ev;
    if (!x || !vx || (h->sk->m > 0 && (!lambda || !vl)) || (e.n_dpar > 0 && !out)) throw std::invalid_argument("asm_eval_data_cross_t: null pointer");
    ct_columns(h, x, lambda, 1, vx, 1.0, vl, out, 1);
}

// ---- limited-memory Hessian (include/asm_hip.h, "Limited-memory Hessian"; kernels in asm_lm_kernels.hip.h)
namespace {
void lm_clear(asm_handle* h) {
    LmState& M = h->lm;
    M.pending = false;
    if (!M.S.R) return;
    const LmStore& L = M.S;
    const hipStream_t s = h->stream;
    const int64_t P = L.P;
    HIPCHK(asmb::fill_async(L.R, 0, 2 * P * L.ld * sizeof(double), s));
    HIPCHK(asmb::fill_async(L.ss, 0, P * P * sizeof(double), s));
    HIPCHK(asmb::fill_async(L.sy, 0, P * P * sizeof(double), s));
    HIPCHK(asmb::fill_async(L.W, 0, 4 * P * P * sizeof(double), s));
    asmb::launch(k_lm_clear, dim3(1), dim3(64), s, L);
}
// the handle's store, made empty at the first use after a set-up and sized from the handle's memory
LmState* lm_store(asm_handle* h, const char* who) {
    const Skeleton& K = sk_of(h, (std::string(who) + ": asm_sublp_setup first").c_str());
    LmState& M = h->lm;
    if (M.S.R) return &M;
    HIPCHK(hipSetDevice(h->device));
    BufPool& B = M.mem;
    LmStore& L = M.S;
    const int64_t n = K.n, ld = K.ldn, P = M.memory;
    M.nwg = (int)std::max<int64_t>((n + LM_CHUNK - 1) / LM_CHUNK, 1);
    M.ndot = (int)std::min<int64_t>(M.nwg, LM_DOTWG);
    M.per = (n + M.ndot - 1) / M.ndot;
    try {
        B.alloc(L.R, 2 * P * ld); B.alloc(L.ss, P * P); B.alloc(L.sy, P * P); B.alloc(L.W, 4 * P * P); B.alloc(L.sigma, 1); B.alloc(L.st, LM_WORDS);
        B.alloc(M.xs, n); B.alloc(M.gs, n); B.alloc(M.s, n); B.alloc(M.y, n); B.zeroed(M.jtl, ld, h->stream);
        B.alloc(M.part_dot, 3 * LM_DOTWG); B.alloc(M.part, (int64_t)KKM_CW * M.nwg * 2 * P);
        M.bytes = (2 * P * ld + 6 * P * P + 1 + 4 * n + ld + 3 * LM_DOTWG + (int64_t)KKM_CW * M.nwg * 2 * P) * (int64_t)sizeof(double) + LM_WORDS * (int64_t)sizeof(int);
        L.n = n; L.ld = ld; L.P = (int)P; L.pad = 0;
        lm_clear(h);
        HIPCHK(asmb::sync(h->stream));
    } catch (...) {
        M.drop();      // (a store is whole or not there: R != nullptr is the test above)
        throw;
    }
    return &M;
}
// the pair in M.s, M.y: the three dots, the skip rule, the rows, the Gram entries, Ws - five launches, nothing read back
void lm_push(asm_handle* h) {
    LmState& M = h->lm;
    const LmStore& L = M.S;
    const hipStream_t s = h->stream;
    asmb::launch(k_lm_pair_dots, dim3((unsigned)M.ndot), dim3(256), s, M.s, M.y, L.n, M.per, M.part_dot);
    asmb::launch(k_lm_pair_decide, dim3(1), dim3(64), s, L, M.part_dot, M.ndot);
    asmb::launch(k_lm_pair_store, asmb::blocks(L.n), dim3(256), s, L, M.s, M.y);
    asmb::launch(k_lm_pair_gram, dim3((unsigned)L.P), dim3(256), s, L);
    asmb::launch(k_lm_middle, dim3(1), dim3(256), s, L);
}
// OUT = V B for cols <= KKM_CW rows of V on the device (pitches ldv, ldo; V and OUT apart): two launches
void lm_product(asm_handle* h, const double* V, int64_t ldv, int cols, double* OUT, int64_t ldo) {
    LmState& M = *lm_store(h, "asm_lm_product");
    const LmStore& L = M.S;
    asmb::launch(k_lm_psi_v, dim3((unsigned)M.nwg, (unsigned)((cols + LM_COLS - 1) / LM_COLS)), dim3(256), h->stream, L, V, ldv, cols, M.part);
    asmb::launch(k_lm_apply, asmb::blocks(L.n), dim3(256), h->stream, L, V, ldv, cols, M.part, M.nwg, OUT, ldo);
}
// J' lambda into the store's own vector, by the route of asm_slp_norms: the Jacobian assembled from the last evaluation's values, lambda
// padded with zeros on the extra range rows
LmState* lm_jtl(asm_handle* h, const char* who, const double* lambda) {
    const std::string me(who);
    ev_of(h, who);
    if (!h->sk->inputs_ready || !h->sk->inputs_from_eval) throw std::logic_error(me + ": asm_eval_functions first");
    if (h->sk->m > 0 && !lambda) throw std::invalid_argument(me + ": null pointer");
    LmState& M = *lm_store(h, who);
    HIPCHK(hipSetDevice(h->device));
    Dev d(h);
    d.assemble();
    d.h2d(h->sk->d_vecM, lambda, h->sk->m, h->sk->Mp);
    d.launch_gemv_t(h->sk->d_J, h->sk->d_vecM, M.jtl);
    return &M;
}
void do_lm_begin(asm_handle* h, const double* lambda) {
    LmState& M = *lm_jtl(h, "asm_lm_begin", lambda);
    const EvalState& e = *h->ev;
    asmb::launch(k_lm_save, asmb::blocks(M.S.n), dim3(256), h->stream, e.d_x, e.d_df, M.jtl, M.S.n, M.xs, M.gs);
    M.pending = true;
    Dev(h).resolve_timing();
}
void do_lm_end(asm_handle* h, const double* lambda) {
    ev_of(h, "asm_lm_end");
    if (!h->lm.pending) return;
    LmState& M = *lm_jtl(h, "asm_lm_end", lambda);
    const EvalState& e = *h->ev;
    asmb::launch(k_lm_diff, asmb::blocks(M.S.n), dim3(256), h->stream, e.d_x, e.d_df, M.jtl, M.xs, M.gs, M.S.n, M.s, M.y);
    lm_push(h);
    M.pending = false;
    Dev(h).resolve_timing();
}
void do_lm_push_pair(asm_handle* h, const double* sv, const double* yv) {
    if (!sv || !yv) throw std::invalid_argument("asm_lm_push_pair: null pointer");
    LmState& M = *lm_store(h, "asm_lm_push_pair");
    HIPCHK(hipSetDevice(h->device));
    const int64_t n = M.S.n;
    HIPCHK(asmb::copy_async(M.s, sv, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(asmb::copy_async(M.y, yv, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(asmb::sync(h->stream));      // (the caller's arrays are free again)
    lm_push(h);
}
void do_lm_product(asm_handle* h, const double* V, int32_t nrhs, double* OUT) {
    if (nrhs < 1) throw std::invalid_argument("asm_lm_product: nrhs < 1");
    if (!V || !OUT) throw std::invalid_argument("asm_lm_product: null pointer");
    LmState& M = *lm_store(h, "asm_lm_product");
    HIPCHK(hipSetDevice(h->device));
    const int64_t n = M.S.n, ld = M.S.ld;
    if (!M.vb) {
        M.mem.zeroed(M.vb, (int64_t)KKM_CW * ld, h->stream);
        M.mem.zeroed(M.ob, (int64_t)KKM_CW * ld, h->stream);
        M.bytes += 2 * (int64_t)KKM_CW * ld * (int64_t)sizeof(double);
    }
    for (int32_t c0 = 0; c0 < nrhs; c0 += KKM_CW) {
        const int cols = (int)std::min<int32_t>(KKM_CW, nrhs - c0);
        HIPCHK(hipMemcpy2DAsync(M.vb, ld * sizeof(double), V + (int64_t)c0 * n, n * sizeof(double), n * sizeof(double), cols, hipMemcpyHostToDevice, h->stream));
        lm_product(h, M.vb, ld, cols, M.ob, ld);
        HIPCHK(hipMemcpy2DAsync(OUT + (int64_t)c0 * n, n * sizeof(double), M.ob, ld * sizeof(double), n * sizeof(double), cols, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(asmb::sync(h->stream));
    }
}
void do_lm_info(asm_handle* h, struct asm_lm_info* out) {
    if (!out) throw std::invalid_argument("asm_lm_info: null pointer");
    const LmState& M = h->lm;
    std::memset(out, 0, sizeof(*out));
    out->type = M.type; out->memory = M.memory; out->pending = M.pending ? 1 : 0; out->sigma = 1.0; out->bytes = M.bytes;
    if (!M.S.R) return;
    HIPCHK(hipSetDevice(h->device));
    int st[LM_WORDS];
    HIPCHK(asmb::sync(h->stream));
    HIPCHK(asmb::copy(st, M.S.st, sizeof(st), hipMemcpyDeviceToHost));
    HIPCHK(asmb::copy(&out->sigma, M.S.sigma, sizeof(double), hipMemcpyDeviceToHost));
    out->pairs = st[LM_COUNT]; out->pushed = st[LM_PUSHED]; out->skipped_zero = st[LM_SKIP_ZERO]; out->skipped_curvature = st[LM_SKIP_CURV];
}
void do_hessian_set_type(asm_handle* h, int32_t type, int32_t memory) {
    if (h->batch_slot) throw std::invalid_argument("asm_hessian_set_type: the type is chosen per handle, not for a slot of an asm_batch");
    if (type != ASM_HESS_EXACT && type != ASM_HESS_LM) throw std::invalid_argument("asm_hessian_set_type: type is neither ASM_HESS_EXACT nor ASM_HESS_LM");
    if (memory < 1 || memory > ASM_LM_MAX) throw std::invalid_argument("asm_hessian_set_type: memory outside 1 .. ASM_LM_MAX");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(asmb::sync(h->stream));
    h->lm.drop();
    h->lm.type = type;
    h->lm.memory = memory;
}
// what stands for H in the KKT entries of this handle: the limited-memory operator takes every nlp_kind, the exact one hs_check's
bool kkt_hess_lm(const asm_handle* h, const char* who) {
    if (h->lm.type != ASM_HESS_LM) { hs_check(h, who); return false; }
    ev_of(h, who);
    return true;
}
}  // namespace

// ---- the KKT solve on a working set (include/asm_hip.h, "The KKT solve on a working set" and "Many right-hand sides on one factor"): one
// set-up of the face (KktFace, steps 1 and 2), one driver of steps 3 to 6 on blocks of columns (kkt_columns) and, behind KktOps, the
// ways to multiply and solve: KktOneColumn for asm_kkt_solve and asm_solution_sensitivity, KktBlock for the multi entries, and KktSparse
// for both where the handle's form is ASM_KKT_SPARSE (asm_kkt_set_form).  The entry point and the form choose (kkt_run), not nrhs: a
// column's bits do not depend on the number of columns beside it.  A call is described by values: KktPoint, KktRhs, KktOut, KktInfoSink, KktTrust.
static_assert(KKM_CW == ASM_KKT_CHUNK && KKM_CW % 32 == 0 && KKM_SCAL > KKM_ITERS, "the chunk width of the header is the kernels'");
namespace {
// once per asm_eval_setup, at the first KKT solve: what steps 1 and 2 fill, sized for every working set the problem admits, and the
// per-column reduction state
void kk_prepare(asm_handle* h) {
    KktBufs& K = h->ev->kk;
    if (K.ready) return;
    HIPCHK(hipSetDevice(h->device));
    BufPool& M = h->ev->mem;
    const hipStream_t s = h->stream;
    const int64_t ldn = h->sk->ldn, Mp = std::max<int64_t>(h->sk->Mp, 32), CW = KKM_CW;
    K.capW = std::max<int64_t>(std::min(h->sk->m, h->sk->n), 1);
    K.ldT = round_up(K.capW, 32);
    M.alloc(K.dE, h->sk->nnz);
    ns_alloc_factor(h, M, K.fac, K.capW);
    M.zeroed(K.sets, ldn + (Mp + 1) / 2, s);
    M.alloc(K.h_sets, ldn + (Mp + 1) / 2, BufPool::PINNED);
    M.zeroed(K.dropped, 4, s);
    M.zeroed(K.part, CW * KK_MAXWG * KK_SLOTS, s);
    M.zeroed(K.scal, CW * KKM_SCAL + 16, s);
    M.zeroed(K.cnt, CW + 4, s);
    M.zeroed(K.act, CW, s);
    HIPCHK(asmb::sync(s));
    K.ready = true;
}
// what only the dense form needs, at its first call: the solve's own dense J, A = J[W, F] and its transposed copy (a handle that only
// ever runs the sparse form never makes them)
void kk_dense(asm_handle* h) {
    kk_prepare(h);
    KktBufs& K = h->ev->kk;
    if (K.dense_ready) return;
    HIPCHK(hipSetDevice(h->device));
    BufPool& M = h->ev->mem;
    const hipStream_t s = h->stream;
    const int64_t ldn = h->sk->ldn, Mp = std::max<int64_t>(h->sk->Mp, 32);
    M.zeroed(K.J, Mp * ldn, s);
    M.zeroed(K.Aw, K.capW * ldn, s);
    M.zeroed(K.AwT, ldn * K.ldT, s);
    K.dense_bytes += (Mp * ldn + K.capW * ldn + ldn * K.ldT) * (int64_t)sizeof(double);
    HIPCHK(asmb::sync(s));
    K.dense_ready = true;
}
// what only the sparse form needs, at its first call: the CSR values and the position list.  The pairs of any working set are a subset of
// the pairs of all m rows: the pair buffer of either row order (kk_pairs) is sized from those, and the order of all rows with its pairs
// stays on the host for the static order.  False: rcm_order declines the pattern (RCM_MAX_PAIRS) and the call runs the dense form.
bool kk_sparse(asm_handle* h) {
    kk_prepare(h);
    KktBufs& K = h->ev->kk;
    if (K.sparse_ready) return K.pairs_cap > 0;
    HIPCHK(hipSetDevice(h->device));
    BufPool& M = h->ev->mem;
    const hipStream_t s = h->stream;
    const Skeleton& S = *h->sk;
    K.sparse_ready = true;
    std::vector<int> all((size_t)S.m), prs;
    for (int64_t i = 0; i < S.m; ++i) all[i] = (int)i;
    int bw = 0;
    K.s_order = rcm_order(all, S.sp_ptr_h, S.sp_col_h, S.ldn, &bw, &prs);
    if (S.m > 0 && prs.empty()) return false;
    K.pairs_cap = std::max<int64_t>((int64_t)prs.size() / 2, 1);
    K.s_band = bw;
    K.s_npairs = (int64_t)prs.size() / 2;
    K.s_pairs_h.resize(prs.size());
    for (size_t k = 0; k < prs.size(); ++k) K.s_pairs_h[k] = K.s_order[prs[k]];      // (places in the order -> rows)
    K.s_place.assign((size_t)std::max<int64_t>(S.m, 1), -1);
    K.c_state.reserve((size_t)S.m);
    K.c_order.reserve((size_t)S.m);
    K.last_rows.reserve((size_t)S.m);
    M.zeroed(K.sp_vals, S.sp_nnz, s);
    M.alloc(K.wpos, std::max<int64_t>(S.M, 1));
    K.sparse_bytes += S.sp_nnz * (int64_t)sizeof(double) + std::max<int64_t>(S.M, 1) * (int64_t)sizeof(int);
    HIPCHK(asmb::sync(s));
    return true;
}
// the pair buffer of the row order in use, at the first sparse call in that order: 2 * pairs_cap ints either way.  Working-set order: every
// new working set uploads its own pairs (kk_order).  Static order: the row-index pairs of all rows, uploaded here, once
void kk_pairs(asm_handle* h, int order) {
    KktBufs& K = h->ev->kk;
    int*& buf = order == ASM_KKT_ORDER_STATIC ? K.s_pairs : K.pairs;
    if (buf) return;
    HIPCHK(hipSetDevice(h->device));
    h->ev->mem.alloc(buf, 2 * K.pairs_cap);
    K.sparse_bytes += 2 * K.pairs_cap * (int64_t)sizeof(int);
    if (order == ASM_KKT_ORDER_STATIC && K.s_npairs > 0) {
        HIPCHK(asmb::copy_async(buf, K.s_pairs_h.data(), K.s_pairs_h.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(asmb::sync(h->stream));
    }
}
// the work area of capacity cap (1 or KKM_CW), made at the first call that asks for it (for a slot of a scenario batch before its fiber
// starts: batch_kkt_prepare); the unmasked transposed working rows of the dense block products at the first dense call
KktWork* kk_work(asm_handle* h, int64_t cap, bool sparse = false) {
    kk_prepare(h);
    KktBufs& K = h->ev->kk;
    KktWork& W = cap == 1 ? K.one : K.blk;
    HIPCHK(hipSetDevice(h->device));
    BufPool& M = h->ev->mem;
    const hipStream_t s = h->stream;
    const int64_t ldn = h->sk->ldn, Mp = std::max<int64_t>(h->sk->Mp, 32), nd = std::max<int64_t>(h->ev->n_dpar, 1);
    if (cap > 1 && !sparse && !W.AfT) {
        M.zeroed(W.AfT, ldn * K.ldT, s);
        K.dense_bytes += ldn * K.ldT * (int64_t)sizeof(double);
        HIPCHK(asmb::sync(s));
    }
    if (W.cap != 0) return &W;
    M.zeroed(W.vec, 14 * cap * ldn, s);
    M.zeroed(W.row, 5 * cap * K.ldT, s);
    M.zeroed(W.dlf, cap * Mp, s);
    M.zeroed(W.rad, cap, s);
    if (cap > 1) M.zeroed(W.Lt, K.fac.ld * K.fac.ld, s);
    if (cap > 1) M.zeroed(W.bnd, cap + (cap + 1) / 2, s);
    M.alloc(W.stage, cap * (3 * ldn + K.ldT + Mp + KKM_SCAL + nd) + 64, BufPool::PINNED);
    HIPCHK(asmb::sync(s));
    W.cap = cap;
    return &W;
}
// what only a call with weights on the bound multipliers needs (asm_solution_adjoint_z*, KktRhs::with_gz), at its first such call - for a
// slot of a scenario batch before its fiber starts: the mask of B and, where the call will run the dense form, J[W, B] as a dense operand
void kk_gz(asm_handle* h) {
    kk_prepare(h);
    KktBufs& K = h->ev->kk;
    const bool sparse = K.form == ASM_KKT_SPARSE && h->sk->sp_ok && kk_sparse(h);
    if (K.cmask && (sparse || K.Ab)) return;
    HIPCHK(hipSetDevice(h->device));
    BufPool& M = h->ev->mem;
    const int64_t ldn = h->sk->ldn;
    if (!K.cmask) M.zeroed(K.cmask, ldn, h->stream);
    if (!sparse && !K.Ab) {
        M.zeroed(K.Ab, K.capW * ldn, h->stream);
        K.dense_bytes += K.capW * ldn * (int64_t)sizeof(double);
    }
    HIPCHK(asmb::sync(h->stream));
}
// the active-column word of the last k_kktm_cg_dir on the host: the kernel's own store into the host-mapped scalar block and the sequence
// word the host spins on, or (pub == 0, ASM_HIP_SPIN=0) a copy and a stream synchronisation
int kk_read_scal(asm_handle* h, unsigned pub) {
    if (pub == 0) {
        HIPCHK(asmb::copy_async(h->sk->h_scal, h->ev->kk.scal + KKM_CW * KKM_SCAL, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(asmb::sync(h->stream));
        return (int)h->sk->h_scal[0];
    }
    if (asmb::in_fiber()) {      // scenario batch: the publishing kernel is recorded; the round that launches it ends before this fiber resumes
        asmb::flush_wait();
        if (__atomic_load_n(h->sk->h_seq, __ATOMIC_ACQUIRE) != pub) throw HipError("asm_kkt_solve: the batch round ended without the publishing kernel's sequence word");
        return (int)h->sk->h_scal[0];
    }
    const double t0 = Solver::now_ms();
    for (unsigned long spins = 1;; ++spins) {
        if (__atomic_load_n(h->sk->h_seq, __ATOMIC_ACQUIRE) == pub) break;
        if (spins < 20000) __builtin_ia32_pause();
        else sched_yield();
        if ((spins & 0xffff) == 0 && Solver::now_ms() - t0 > 30000.0) {
            HIPCHK(asmb::sync(h->stream));            // a device fault surfaces here
            if (__atomic_load_n(h->sk->h_seq, __ATOMIC_ACQUIRE) == pub) break;
            throw HipError("asm_kkt_solve: the publishing kernel finished without setting its sequence word");
        }
    }
    return (int)h->sk->h_scal[0];
}

// The face of a call: its counts and limits, and on the device (h->ev->kk) the mask of F, the list of W, A = J[W, F] with its transposed copy
// and the factor of S = A A'.
struct KktFace {
    int64_t nF = 0, nW = 0, nWp = 0, max_iter = 0;      // |F|, |W|, |W| rounded up to 32
    // |W| rounded up to 64: what the grids over the working rows are sized from (every such kernel returns beyond the nW of its arguments), so
    // that the launches of scenarios whose working sets differ by a few rows have one shape and merge (Sched::same)
    int64_t nWg = 0;
    double rtol = 0.0;
    // the working rows (Mp entries, 0 beyond |W|): ascending in the dense form, in the reverse Cuthill-McKee order of their coupling graph in
    // the sparse form.  Everything that touches working rows goes through this list or its device copy.
    std::vector<int> wl;
    const double* mask = nullptr;                       // 1.0 on F, 0.0 on B and beyond n (ldn)
    const int* wrow = nullptr;                          // wl on the device
    bool sparse = false;                                // the form of this call (asm_kkt_set_form and the fallback rules)
    bool lm = false;                                    // the limited-memory operator stands for H (asm_hessian_set_type): step 1 is skipped
    // the checks every entry shares (`me` names the caller in the messages) and steps 1 and 2 of the method
    KktFace(asm_handle* h, Dev& dev, const std::string& me, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state,
            const asm_kkt_params* par, bool use_lm = false);
};
// Sparse form: puts f.wl into the reverse Cuthill-McKee order of the working rows' coupling graph and leaves the pairs of S and the position
// list on the device, the band and the counts in K.last.  The order, band and pairs of the last row_state are kept: an equal row_state
// reuses them (and what is on the device) - the structure of S over W does not depend on F.
void kk_order(asm_handle* h, KktFace& f, const int32_t* row_state) {
    KktBufs& K = h->ev->kk;
    const Skeleton& S = *h->sk;
    const int64_t m = S.m, nW = f.nW;
    kk_pairs(h, ASM_KKT_ORDER_WORKING_SET);
    const bool hit = K.c_valid && K.c_kind == ASM_KKT_ORDER_WORKING_SET && (int64_t)K.c_state.size() == m && std::equal(row_state, row_state + m, K.c_state.begin());
    if (!hit) {
        K.c_valid = false;      // (until the new order and both device lists are in place)
        K.c_kind = ASM_KKT_ORDER_WORKING_SET;
        const double t0 = Solver::now_ms();
        const std::vector<int> rows(f.wl.begin(), f.wl.begin() + nW);
        std::vector<int> prs;
        int bw = 0;
        K.c_order.clear();
        if (nW > 0) {
            const std::vector<int> ord = rcm_order(rows, S.sp_ptr_h, S.sp_col_h, S.ldn, &bw, &prs);
            if ((int64_t)prs.size() / 2 > K.pairs_cap || prs.empty()) throw HipError("asm_kkt: the pairs of a working set outgrow the pairs of all rows");
            K.c_order.resize((size_t)nW);
            for (int64_t q = 0; q < nW; ++q) K.c_order[q] = rows[ord[q]];
        }
        K.c_band = nW > 0 ? std::max(bw, 1) : 0;
        K.n_pairs = (int64_t)prs.size() / 2;
        K.c_state.assign(row_state, row_state + m);
        std::vector<int> wpos((size_t)std::max<int64_t>(S.M, 1), -1);
        for (int64_t q = 0; q < nW; ++q) wpos[K.c_order[q]] = (int)q;
        HIPCHK(asmb::copy_async(K.wpos, wpos.data(), wpos.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        if (!prs.empty()) HIPCHK(asmb::copy_async(K.pairs, prs.data(), prs.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(asmb::sync(h->stream));
        K.c_valid = true;
        K.last.order_ms = Solver::now_ms() - t0;
    }
    for (int64_t q = 0; q < nW; ++q) f.wl[q] = K.c_order[q];
    K.last.band = K.c_band;
    K.last.n_pairs = K.n_pairs;
    K.last.order_reused = hit ? 1 : 0;
}
// Sparse form, static order (asm_kkt_set_order): f.wl is the order of all rows (kk_sparse) filtered by row_state - the coupling graph of W is
// an induced subgraph of that of all rows and places only move closer, so the band is at most the all-rows band.  The band (the exact
// largest distance over the static pairs with both rows in W) and the pair count are the host's; the cache is the one of kk_order.  Nothing
// goes up and nothing is waited for: the caller makes the position list on the device from the uploaded f.wl where this returns false.
bool kk_order_static(asm_handle* h, KktFace& f, const int32_t* row_state) {
    KktBufs& K = h->ev->kk;
    const int64_t m = h->sk->m, nW = f.nW;
    const bool hit = K.c_valid && K.c_kind == ASM_KKT_ORDER_STATIC && (int64_t)K.c_state.size() == m && std::equal(row_state, row_state + m, K.c_state.begin());
    if (!hit) {
        K.c_valid = false;
        K.c_kind = ASM_KKT_ORDER_STATIC;
        const double t0 = Solver::now_ms();
        K.c_order.clear();
        for (int64_t p = 0; p < m; ++p) {
            const int r = K.s_order[p];
            K.s_place[r] = row_state[r] ? (int)K.c_order.size() : -1;
            if (row_state[r]) K.c_order.push_back(r);
        }
        int bw = 0;
        int64_t np = 0;
        for (int64_t t = 0; t < K.s_npairs; ++t) {
            const int pi = K.s_place[K.s_pairs_h[2 * t]], pj = K.s_place[K.s_pairs_h[2 * t + 1]];
            if (pi < 0 || pj < 0) continue;
            bw = std::max(bw, std::abs(pi - pj));
            ++np;
        }
        K.c_band = nW > 0 ? std::max(bw, 1) : 0;
        K.n_pairs = np;
        K.c_state.assign(row_state, row_state + m);
        K.last.order_ms = Solver::now_ms() - t0;      // (c_valid: once the caller has the position list launched)
    }
    for (int64_t q = 0; q < nW; ++q) f.wl[q] = K.c_order[q];
    K.last.band = K.c_band;
    K.last.n_pairs = K.n_pairs;
    K.last.order_reused = hit ? 1 : 0;
    return hit;
}
KktFace::KktFace(asm_handle* h, Dev& dev, const std::string& me, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state,
                 const asm_kkt_params* par, bool use_lm) {
    const int64_t n = h->sk->n, m = h->sk->m, ldn = h->sk->ldn;
    KktFace& f = *this;
    f.lm = use_lm;
    for (int64_t j = 0; j < n; ++j) {
        if (bound_state[j] < -1 || bound_state[j] > 1) throw std::invalid_argument(me + ": bound_state holds a value outside {-1, 0, +1}");
        f.nF += bound_state[j] == 0;
    }
    for (int64_t i = 0; i < m; ++i) {
        if (row_state[i] != 0 && row_state[i] != 1) throw std::invalid_argument(me + ": row_state holds a value outside {0, 1}");
        f.nW += row_state[i];
    }
    const int64_t nW = f.nW;
    if (nW > f.nF) throw std::invalid_argument(me + ": more working rows (" + std::to_string(nW) + ") than free variables (" + std::to_string(f.nF) + ")");
    if (par && (par->max_iter < 0 || !(par->rtol >= 0.0))) throw std::invalid_argument(me + ": max_iter < 0 or rtol not >= 0");
    f.max_iter = par ? par->max_iter : 2 * (f.nF - nW) + 20;
    f.rtol = par ? par->rtol : 1e-12;
    f.nWp = round_up(nW, 32);
    f.nWg = round_up(nW, 64);
    // (a slot of a scenario batch has both made before its fiber starts - batch_kkt_prepare: no allocation, no list building in a round)
    if (f.lm) lm_store(h, me.c_str());
    else hs_prepare(h);
    kk_prepare(h);
    KktBufs& K = h->ev->kk;
    // the form: sparse when asked for and possible - a sparse pattern that rcm_order accepts - else dense, which is not an error
    f.sparse = K.form == ASM_KKT_SPARSE && h->sk->sp_ok && kk_sparse(h);
    if (!f.sparse) kk_dense(h);
    const bool fixed = f.sparse && K.order == ASM_KKT_ORDER_STATIC;
    if (fixed) kk_pairs(h, ASM_KKT_ORDER_STATIC);
    K.order_used = fixed ? ASM_KKT_ORDER_STATIC : ASM_KKT_ORDER_WORKING_SET;
    HIPCHK(hipSetDevice(h->device));
    const hipStream_t s = h->stream;
    const int64_t Mp = std::max<int64_t>(h->sk->Mp, 32);
    K.last = {};
    K.last.form_requested = K.form;
    K.last.form_used = f.sparse ? ASM_KKT_SPARSE : ASM_KKT_DENSE;
    // 1. the Hessian values of f - lambda' g at x, once: they stay in d_hs_vals for every product of the call (x goes to d_ev_xt)
    // (the limited-memory operator has nothing to evaluate: x alone goes up)
    if (f.lm) {
        std::memcpy(h->ev->h_stage, x, n * sizeof(double));
        HIPCHK(asmb::copy_async(h->ev->d_xt, h->ev->h_stage, n * sizeof(double), hipMemcpyHostToDevice, s));
    } else {
        std::vector<double> nl((size_t)std::max<int64_t>(m, 1), 0.0);
        for (int64_t i = 0; i < m; ++i) nl[i] = -lambda[i];
        hs_launch(h, x, 1.0, nl.data(), nullptr);      // (copies nl into the pinned staging buffer before it returns)
    }
    // 2. the Jacobian at x: values into a buffer of the solve's own, assembled into its own dense J (the LP's dE and J stay) or, sparse
    // form, summed into the CSR list of the pattern: its first nu entries are the unique entries in k_assemble's order
    {
        // (the kernel families without second derivatives come here with the limited-memory operator only)
        fn_rows_launch(*h->ev, s, h->ev->d_xt, h->ev->d_Et, K.dE, 1);
        nlp_rows_launch(*h->ev, s, h->ev->d_xt, h->ev->d_Et, K.dE, 1);
        if (f.sparse) {
            KktSites(s, ldn, K.ldT).kkts_vals(K.dE, h->sk->d_perm, h->sk->d_ustart, h->sk->nu, K.sp_vals);
        } else if (h->sk->dense_fast) {
            const unsigned g = (unsigned)std::min<int64_t>((h->sk->m * h->sk->n + 255) / 256, 4096);
            asmb::launch(k_assemble_dense, dim3(g), dim3(256), s, K.dE, K.J, h->sk->m, h->sk->n, ldn);
        } else if (h->sk->nu > 0) {
            const unsigned g = (unsigned)std::min<int64_t>((h->sk->nu + 255) / 256, 4096);
            asmb::launch(k_assemble, dim3(g), dim3(256), s, K.dE, h->sk->d_perm, h->sk->d_ustart, h->sk->d_uoff, h->sk->d_adjoff, K.J, h->sk->nu);
        }
    }
    // the sets: the mask and the working-row list in one upload
    {
        double* st = K.h_sets;
        for (int64_t j = 0; j < ldn; ++j) st[j] = (j < n && bound_state[j] == 0) ? 1.0 : 0.0;
        f.wl.assign((size_t)Mp, 0);
        int64_t q = 0;
        for (int64_t i = 0; i < m; ++i)
            if (row_state[i]) f.wl[q++] = (int)i;
        const bool made = !f.sparse || (fixed ? kk_order_static(h, f, row_state) : (kk_order(h, f, row_state), true));
        K.last_rows.assign(f.wl.begin(), f.wl.begin() + f.nW);
        std::memcpy(st + ldn, f.wl.data(), Mp * sizeof(int));
        HIPCHK(asmb::copy_async(K.sets, st, ldn * sizeof(double) + Mp * sizeof(int), hipMemcpyHostToDevice, s));
        f.mask = K.sets;
        f.wrow = reinterpret_cast<const int*>(K.sets + ldn);
        if (!made) {      // static order, a new working set: the place of every LP row in it, from the list just uploaded
            KktSites(s, ldn, K.ldT).kkts_wpos(f.wrow, f.nW, h->sk->M, K.wpos);
            K.c_valid = true;
        }
    }
    // A = J[W, F] as a dense operand and its transposed copy with the k-padding cleared; S = A A' and its factor (Dev::chol leaves the
    // wide-block inverses too); the dropped pivots
    if (nW > 0 && f.sparse) {
        // S = A diag(mask) A' entry by entry from the structural pairs, after the band (or, a band too wide to use, the rows) is cleared;
        // the factor is shared with the dense form: what an earlier call may have left outside this call's band is cleared here
        const int band = K.last.band;
        K.fac.band = 2 * (int64_t)band >= nW ? 0 : band;
        if (K.fac_full_rows > 0) {
            HIPCHK(asmb::fill_async(K.fac.S, 0, K.fac_full_rows * K.fac.ld * sizeof(double), s));
            K.fac_full_rows = 0;
        }
        if (K.fac.band > 0) {
            K.fac_band_hw = std::max(K.fac_band_hw, K.fac.band);
            dev.zero_band(K.fac, (int)nW, K.fac_band_hw);
        } else {
            HIPCHK(asmb::fill_async(K.fac.S, 0, nW * K.fac.ld * sizeof(double), s));
            K.fac_full_rows = std::min<int64_t>(round_up(nW, 64), K.fac.ld);
        }
        // (static order: every structural pair of all rows through the position list, those with a row outside W skipped - one grid for
        // every working set and every scenario of a batch)
        if (fixed)
            asmb::launch(k_schur_sparse, asmb::blocks(K.s_npairs), dim3(256), s, (const int*)K.s_pairs, K.s_npairs, (const int*)K.wpos, (const int*)h->sk->d_sp_ptr,
                         (const int*)h->sk->d_sp_col, (const double*)K.sp_vals, f.mask, (const double*)nullptr, K.fac.S, K.fac.ld, (const int*)nullptr);
        else
            asmb::launch(k_ns_s0_sparse, asmb::blocks(K.n_pairs), dim3(256), s, (const int*)K.pairs, K.n_pairs, (const int*)h->sk->d_sp_ptr, (const int*)h->sk->d_sp_col,
                         (const double*)K.sp_vals, f.wrow, f.mask, K.fac.S, K.fac.ld);
        dev.diag_prepare(K.fac, (int)nW, 1, 0.0, 0.0);
        const int nfact = h->stats.nfact;
        dev.chol(K.fac, (int)nW, 1e-10);
        h->stats.nfact = nfact;
        asmb::launch(k_ns_count_big, dim3(1), dim3(1024), s, K.fac.S, K.fac.ld, (int)nW, NS_BIG, K.dropped);
    } else if (nW > 0) {
        const KktSites at(s, ldn, K.ldT);
        K.fac.band = 0;
        K.fac_full_rows = std::max(K.fac_full_rows, std::min<int64_t>(round_up(nW, 64), K.fac.ld));
        at.gather(K.J, f.wrow, f.mask, nW, f.nWg, K.Aw);
        at.gather_t(K.J, f.wrow, f.mask, nW, f.nWp, K.AwT);
        dev.launch_syrk(s, Dev::pick_tile(nW), K.Aw, ldn, nullptr, 0, (int)nW, (int)ldn, nullptr, nullptr, K.fac.S, K.fac.ld, 0, 0);
        dev.diag_prepare(K.fac, (int)nW, 1, 0.0, 0.0);
        const int nfact = h->stats.nfact;
        dev.chol(K.fac, (int)nW, 1e-10);
        h->stats.nfact = nfact;          // (the LP statistics count the LP's factorisations)
        asmb::launch(k_ns_count_big, dim3(1), dim3(1024), s, K.fac.S, K.fac.ld, (int)nW, NS_BIG, K.dropped);
    } else {
        HIPCHK(asmb::fill_async(K.dropped, 0, 4 * sizeof(int), s));
    }
}

// What the two paths do differently, on the first `cols` columns of blocks (rows of pitch ldn over the variables, ldT over the working rows).
struct KktOps {
    asm_handle* const h;
    Dev& dev;
    const KktFace& f;
    KktWork& w;
    const hipStream_t s;
    const int64_t n, ldn, ldT;
    const KktSites site;             // the launch sites of the family's own kernels
    double* const spare;             // a block over the working rows of the back end's own
    KktOps(asm_handle* hh, Dev& d, const KktFace& ff, KktWork& ww)
        : h(hh), dev(d), f(ff), w(ww), s(hh->stream), n(hh->sk->n), ldn(hh->sk->ldn), ldT(hh->ev->kk.ldT), site(hh->stream, hh->sk->ldn, hh->ev->kk.ldT),
          spare(ww.row + 2 * ww.cap * hh->ev->kk.ldT) {}
    virtual ~KktOps() = default;
    virtual void hess(const double* v, double* out, int cols) = 0;                  // OUT = H V from the values of step 1, or B V
    // what every back end's hess is: the limited-memory product where the face has it, else the exact kernels on the values of step 1 -
    // `one`: a single column of pitch n (k_hess_product), otherwise cols <= KKM_CW columns of pitch ldn
    void hess_product(const double* v, double* out, int cols, bool one) {
        if (f.lm) { lm_product(h, v, ldn, cols, out, ldn); return; }
        const HsShared& L = *h->ev->hs_sh;
        if (one) asmb::launch(k_hess_product, asmb::blocks(n), dim3(256), s, L.pptr, L.pent, L.poth, h->ev->d_hs_vals, v, n, out);
        else site.hess_product(L.pptr, L.pent, L.poth, h->ev->d_hs_vals, v, n, cols, out);
    }
    virtual void mul_A(const double* v, double* t, int cols) = 0;                   // T = V A'
    virtual void mul_AT(const double* y, double* v, int cols) = 0;                  // V = Y A
    // T = V J[W, B]', the product with the columns that mul_A masks out (the weights on z of the adjoint entries; kk_gz made K.cmask, K.Ab)
    virtual void mul_AB(const double* v, double* t, int cols) = 0;
    // S^-1 applied to the block b; t (b itself, or another block) is where the answer may go.  Returns where it is.
    virtual double* solve_S(const double* b, double* t, int cols) = 0;
    // JTL = J_W' dlam_W over all variables, those of B too, from dlam_W (dlw) or its scattered form over all rows (dlf, pitch Mp)
    virtual void jt_dlam(const double* dlw, const double* dlf, double* jtl, int cols) = 0;
};
// one column: matrix-vector kernels, the factor's own substitution (the one-workgroup small solve where the factor has it) from one
// buffer into another, J' dlam from the private dense J
struct KktOneColumn final : KktOps {
    using KktOps::KktOps;
    void hess(const double* v, double* out, int) override { hess_product(v, out, 1, true); }
    void mul_A(const double* v, double* t, int) override { asmb::launch(k_gemv_n, asmb::blocks(f.nWg, 4), dim3(256), s, h->ev->kk.Aw, ldn, v, t, f.nW, ldn); }
    void mul_AT(const double* y, double* v, int) override { asmb::launch(k_gemv_n_exact, asmb::blocks(ldn, 4), dim3(256), s, h->ev->kk.AwT, ldT, y, v, ldn, f.nW); }
    void mul_AB(const double* v, double* t, int) override {
        const KktBufs& K = h->ev->kk;
        site.gather(K.J, f.wrow, K.cmask, f.nW, f.nWg, K.Ab);
        asmb::launch(k_gemv_n, asmb::blocks(f.nWg, 4), dim3(256), s, K.Ab, ldn, v, t, f.nW, ldn);
    }
    double* solve_S(const double* b, double* t, int) override {
        double* const out = b == t ? spare : t;
        dev.chol_solve_dev(h->ev->kk.fac, b, out, (int)f.nW);
        return out;
    }
    void jt_dlam(const double*, const double* dlf, double* jtl, int) override {
        const int64_t m = h->sk->m;
        int64_t Rc = std::min<int64_t>((m + 31) / 32, ASM_TMAXCHUNKS);
        const int64_t chunk = (m + Rc - 1) / Rc;
        Rc = (m + chunk - 1) / chunk;
        asmb::launch(k_gemv_t_stage1, dim3((unsigned)((ldn + 255) / 256), (unsigned)Rc), dim3(256), s, h->ev->kk.J, ldn, dlf, h->sk->d_partial, m, ldn, chunk);
        asmb::launch(k_gemv_t_stage2, asmb::blocks(ldn), dim3(256), s, h->sk->d_partial, jtl, Rc, ldn);
    }
};
// a block of columns: k_gemm_nt products on the matrix cores (Dev::gemm_nt), Dev::trsm_rows in place with the factor's wide-block
// inverses and its transposed copy, one Hessian launch for all columns, J_W' dlam_W from the unmasked transposed working rows.  Its own
// operands are made here, once per call.
struct KktBlock final : KktOps {
    KktBlock(asm_handle* hh, Dev& d, const KktFace& ff, KktWork& ww) : KktOps(hh, d, ff, ww) {
        const KktBufs& K = h->ev->kk;
        const int64_t nW = f.nW;
        if (nW > 0) {
            site.gather_t(K.J, f.wrow, nullptr, nW, f.nWp, w.AfT);
            // (the rows of Lt up to |W| rounded up to 32 are cleared first: the k-padding beside the nW x nW square the transposition writes)
            HIPCHK(asmb::fill_async(w.Lt, 0, f.nWp * K.fac.ld * sizeof(double), s));
            asmb::launch(k_transpose_dense, dim3((unsigned)((nW + 63) / 64), (unsigned)((nW + 63) / 64)), dim3(256), s, K.fac.S, K.fac.ld, nW, nW, w.Lt, K.fac.ld, nW);
        }
        // the blocks over the working rows are zero beyond column nW (the k-padding of the products that read them)
        HIPCHK(asmb::fill_async(w.row, 0, 5 * w.cap * ldT * sizeof(double), s));
    }
    // (rows >= cols of V are read - they exist: the blocks have KKM_CW rows - not written)
    void hess(const double* v, double* out, int cols) override { hess_product(v, out, cols, false); }
    void mul_A(const double* v, double* t, int cols) override { dev.gemm_nt(v, ldn, h->ev->kk.Aw, ldn, nullptr, 0, t, ldT, cols, (int)f.nW, (int)ldn, 0); }
    void mul_AT(const double* y, double* v, int cols) override { dev.gemm_nt(y, ldT, h->ev->kk.AwT, ldT, nullptr, 0, v, ldn, cols, (int)ldn, (int)f.nWp, 0); }
    void mul_AB(const double* v, double* t, int cols) override {
        const KktBufs& K = h->ev->kk;
        site.gather(K.J, f.wrow, K.cmask, f.nW, f.nWg, K.Ab);
        dev.gemm_nt(v, ldn, K.Ab, ldn, nullptr, 0, t, ldT, cols, (int)f.nW, (int)ldn, 0);
    }
    double* solve_S(const double* b, double* t, int cols) override {
        if (b != t) HIPCHK(asmb::copy_async(t, b, (int64_t)cols * ldT * sizeof(double), hipMemcpyDeviceToDevice, s));
        dev.trsm_rows(h->ev->kk.fac, t, spare, ldT, cols, (int)f.nW, w.Lt);
        return t;
    }
    void jt_dlam(const double* dlw, const double*, double* jtl, int cols) override { dev.gemm_nt(dlw, ldT, w.AfT, ldT, nullptr, 0, jtl, ldn, cols, (int)ldn, (int)f.nWp, 0); }
};
// the sparse form, for both capacities: the products with A and A' from the CSR / CSC lists of the pattern and the values KktFace summed
// into them, for every number of columns (k_kkts_mul_a, k_kkts_mul_at: the column in blockIdx.y); J_W' dlam_W is the transposed product
// without the mask.  The Hessian products and the substitutions are those of the dense back end of the same capacity, on the banded factor:
// chol_solve_dev for one column, trsm_rows with a transposed copy of the band for a block.
struct KktSparse final : KktOps {
    KktSparse(asm_handle* hh, Dev& d, const KktFace& ff, KktWork& ww) : KktOps(hh, d, ff, ww) {
        if (w.cap == 1) return;
        const KktBufs& K = h->ev->kk;
        const int64_t nW = f.nW;
        if (nW > 0) {
            // (the rows of Lt up to |W| rounded up to 32 are cleared whole: whatever an earlier call, of either form, transposed into them goes)
            HIPCHK(asmb::fill_async(w.Lt, 0, f.nWp * K.fac.ld * sizeof(double), s));
            asmb::launch(k_transpose_dense, dim3((unsigned)((nW + 63) / 64), (unsigned)((nW + 63) / 64)), dim3(256), s, K.fac.S, K.fac.ld, nW, nW, w.Lt, K.fac.ld,
                         K.fac.band > 0 ? (int64_t)K.fac.band : nW);
        }
        HIPCHK(asmb::fill_async(w.row, 0, 5 * w.cap * ldT * sizeof(double), s));
    }
    void hess(const double* v, double* out, int cols) override { hess_product(v, out, cols, w.cap == 1); }
    void mul_A(const double* v, double* t, int cols) override {
        const Skeleton& S = *h->sk;
        site.kkts_mul_a(S.d_sp_ptr, S.d_sp_col, h->ev->kk.sp_vals, f.wrow, f.mask, v, f.nW, f.nWg, t, cols);
    }
    void at(const double* y, const double* mask, double* v, int cols) {
        const Skeleton& S = *h->sk;
        site.kkts_mul_at(S.d_sc_ptr, S.d_sc_row, S.d_sc_pos, h->ev->kk.sp_vals, h->ev->kk.wpos, mask, y, n, v, cols);
    }
    void mul_AT(const double* y, double* v, int cols) override { at(y, f.mask, v, cols); }
    void mul_AB(const double* v, double* t, int cols) override {
        const Skeleton& S = *h->sk;
        site.kkts_mul_a(S.d_sp_ptr, S.d_sp_col, h->ev->kk.sp_vals, f.wrow, h->ev->kk.cmask, v, f.nW, f.nWg, t, cols);
    }
    double* solve_S(const double* b, double* t, int cols) override {
        if (w.cap == 1) {
            double* const out = b == t ? spare : t;
            dev.chol_solve_dev(h->ev->kk.fac, b, out, (int)f.nW);
            return out;
        }
        if (b != t) HIPCHK(asmb::copy_async(t, b, (int64_t)cols * ldT * sizeof(double), hipMemcpyDeviceToDevice, s));
        dev.trsm_rows(h->ev->kk.fac, t, spare, ldT, cols, (int)f.nW, w.Lt);
        return t;
    }
    void jt_dlam(const double* dlw, const double*, double* jtl, int cols) override { at(dlw, nullptr, jtl, cols); }
};

// ---- what travels together through the KKT entries: plain values, nothing owned
// The point of a call and its sets.  at(): scenario sc's rows of arrays with a leading scenario dimension (no rows, no arrays over them)
struct KktPoint {
    const double *x = nullptr, *lambda = nullptr;
    const int32_t *row_state = nullptr, *bound_state = nullptr;
    KktPoint at(int64_t sc, int64_t n, int64_t m) const { return {x + sc * n, m > 0 ? lambda + sc * m : nullptr, m > 0 ? row_state + sc * m : nullptr, bound_state + sc * n}; }
};
// Where the columns' answers go, a row per column (DZ may be absent).  at(): the rows from column o on
struct KktOut {
    double *DX = nullptr, *DLAM = nullptr, *DZ = nullptr;
    KktOut at(int64_t o, int64_t n, int64_t m) const { return {DX + o * n, m > 0 ? DLAM + o * m : nullptr, DZ ? DZ + o * n : nullptr}; }
};
// What the columns of a call are - one of four, made by the constructor of its name:
//   given(RU, RW)        the rows of RU, RW are the right-hand sides (asm_kkt_solve(_multi), the step entries, the adjoint states)
//   data(DC)             the rows of DC are directions of the data: the cross-derivative sweep makes each column's right-hand sides on
//                        the device (asm_solution_sensitivity_multi)
//   bound(rows, delta)   a row in [0, m) per column: column c is ru = 0, rw[rows[c]] = -delta[c] (delta == nullptr: -1.0), made on the device
//                        by k_kktm_bound_rhs from 12 bytes per column - no n- or m-long vector is staged (asm_bound_sensitivity_multi)
//   var_bound(vars, delta)  a variable in [0, n) per column, whose bound moves by delta[c] (delta == nullptr: 1.0): column c is
//                        ru = delta H[:, j], rw = delta J[W, j], made on the device from 12 bytes per column (k_kktm_var_unit, one Hessian
//                        product of the back end, k_kktm_var_rhs and in the sparse form k_kkts_var_col), and dx[j] = delta after the finish
//                        step (k_kktm_var_dx); a variable outside B gives the zero column (asm_var_bound_sensitivity_multi)
// A given() call may carry weights on the bound multipliers, with_gz(GZ), a row of n per column (asm_solution_adjoint_z*): the staged
// columns are then corrected on the device to ru - H gz_B and rw - J[W, B] gz_B, gz_B = GZ on B and 0.0 on F.
struct KktRhs {
    enum Kind { GIVEN, DATA, BOUND, VAR_BOUND } kind;
    const double *RU = nullptr, *RW = nullptr, *DC = nullptr, *delta = nullptr, *GZ = nullptr;
    const int32_t* rows = nullptr;      // BOUND: rows; VAR_BOUND: variables
    static KktRhs given(const double* RU, const double* RW) { KktRhs r(GIVEN); r.RU = RU; r.RW = RW; return r; }
    static KktRhs data(const double* DC) { KktRhs r(DATA); r.DC = DC; return r; }
    static KktRhs bound(const int32_t* rows, const double* delta) { KktRhs r(BOUND); r.rows = rows; r.delta = delta; return r; }
    static KktRhs var_bound(const int32_t* vars, const double* delta) { KktRhs r(VAR_BOUND); r.rows = vars; r.delta = delta; return r; }
    KktRhs with_gz(const double* gz) const { KktRhs r = *this; r.GZ = gz; return r; }
    bool derivative() const { return kind != GIVEN; }      // a derivative entry: the exact Hessian whatever the handle's type
    // scenario sc's n_col columns of a batch call; dc_stride: doubles from one scenario's directions to the next, 0 when they are shared
    // (the rows and moves of BOUND, the variables and moves of VAR_BOUND always are)
    KktRhs at(int64_t sc, int64_t n_col, int64_t n, int64_t m, int64_t dc_stride) const {
        KktRhs r = *this;
        if (kind == GIVEN) { r.RU = RU + sc * n_col * n; r.RW = m > 0 ? RW + sc * n_col * m : nullptr; if (GZ) r.GZ = GZ + sc * n_col * n; }
        if (kind == DATA && DC) r.DC = DC + sc * dc_stride;
        return r;
    }
private:
    explicit KktRhs(Kind k) : kind(k) {}
};
// Where a column's info goes: asm_kkt_info, or asm_kkt_step_info with the fields of the trust-region step
struct KktInfoSink {
    asm_kkt_info* plain = nullptr;
    asm_kkt_step_info* step = nullptr;
    KktInfoSink(asm_kkt_info* p) : plain(p) {}
    KktInfoSink(asm_kkt_step_info* s) : step(s) {}
    bool null() const { return !plain && !step; }
};
// The trust-region step (asm_kkt_step, asm_kkt_step_multi): a radius per column, each > 0 (+inf: no region), and the share of it the
// normal step may use.  The same launches with the trust-region forms of k_kktm_cg_curv, k_kktm_cg_dir and k_kktm_finish, and
// k_kktm_normal once per chunk after the normal step.
struct KktTrust {
    bool on = false;
    const double* radius = nullptr;
    double share = 0.8;
    static KktTrust step(const double* radius, double share) { return {true, radius, share}; }
    void check(const std::string& me, int32_t nrhs) const {      // the refusals of the step entries, after those every entry shares
        if (!on) return;
        if (!radius) throw std::invalid_argument(me + ": null pointer");
        for (int32_t c = 0; c < nrhs; ++c)
            if (!(radius[c] > 0.0)) throw std::invalid_argument(me + ": a radius is not > 0");
        if (!(share > 0.0 && share <= 1.0)) throw std::invalid_argument(me + ": normal_share outside (0, 1]");
    }
};
// Step 3 for the chunk of `cols` columns from column c0 on: its right-hand sides into the blocks b_ru (over the variables) and rww (over
// the working rows), by the way of rhs.kind.  The staging area is [ru block | rw block | directions]; the first chunk of a DATA call
// uploads the multipliers of the cross-derivative sweep, once.
// VAR_BOUND, and GIVEN with weights on z, multiply on the device: by ops, into the blocks va, vb over the variables and ta over the
// working rows, free until step 4.
void kkt_stage_rhs(asm_handle* h, const KktFace& f, KktOps& ops, const KktRhs& rhs, const double* lambda, const KktTrust& tr, int64_t c0, int cols, double* b_ru, double* rww,
                   double* va, double* vb, double* ta) {
    KktWork& w = ops.w;
    const hipStream_t s = h->stream;
    const int64_t n = h->sk->n, m = h->sk->m, ldn = h->sk->ldn, ldT = h->ev->kk.ldT, cap = w.cap, nW = f.nW;
    double* st = w.stage;
    switch (rhs.kind) {
    case KktRhs::VAR_BOUND: {
        // [delta | vars] of the chunk's columns, one upload as for BOUND; the unit block, its Hessian product, the scaling and the column of J
        const KktBufs& K = h->ev->kk;
        const Skeleton& S = *h->sk;
        int* hr = reinterpret_cast<int*>(st + cols);
        const int* dv = reinterpret_cast<const int*>(w.bnd + cols);
        const double* dd = rhs.delta ? (const double*)w.bnd : (const double*)nullptr;
        if (rhs.delta) std::memcpy(st, rhs.delta + c0, cols * sizeof(double));
        for (int c = 0; c < cols; ++c) hr[c] = rhs.rows[c0 + c];
        HIPCHK(asmb::copy_async(w.bnd, st, cols * (sizeof(double) + sizeof(int)), hipMemcpyHostToDevice, s));
        ops.site.var_unit(dv, f.mask, vb, cols);
        ops.hess(vb, va, cols);
        ops.site.var_rhs(dv, dd, f.mask, va, n, f.sparse ? (const double*)nullptr : (const double*)K.J, f.wrow, nW, b_ru, rww, cols);
        if (f.sparse && nW > 0) ops.site.var_col(dv, dd, f.mask, S.d_sc_ptr, S.d_sc_row, S.d_sc_pos, K.sp_vals, K.wpos, rww, cols);
        return;
    }
    case KktRhs::BOUND: {
        // [delta | rows] of the chunk's columns in the (unused) staging rows of ru, one upload, one launch
        int* hr = reinterpret_cast<int*>(st + cols);
        int* dr = reinterpret_cast<int*>(w.bnd + cols);
        if (rhs.delta) std::memcpy(st, rhs.delta + c0, cols * sizeof(double));
        for (int c = 0; c < cols; ++c) hr[c] = rhs.rows[c0 + c];
        HIPCHK(asmb::copy_async(w.bnd, st, cols * (sizeof(double) + sizeof(int)), hipMemcpyHostToDevice, s));
        KktSites(s, ldn, ldT).bound_rhs(dr, rhs.delta ? (const double*)w.bnd : (const double*)nullptr, f.wrow, nW, b_ru, rww, cols);
        return;
    }
    case KktRhs::GIVEN: {
        for (int c = 0; c < cols; ++c) {
            const double *u = rhs.RU + (c0 + c) * n, *rw = rhs.RW ? rhs.RW + (c0 + c) * m : nullptr;
            double *du = st + (int64_t)c * ldn, *dw = st + cap * ldn + (int64_t)c * ldT;
            std::memcpy(du, u, n * sizeof(double));
            for (int64_t j = n; j < ldn; ++j) du[j] = 0.0;
            for (int64_t q = 0; q < ldT; ++q) dw[q] = q < nW ? rw[f.wl[q]] : 0.0;
        }
        HIPCHK(asmb::copy_async(b_ru, st, (int64_t)cols * ldn * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(asmb::copy_async(rww, st + cap * ldn, (int64_t)cols * ldT * sizeof(double), hipMemcpyHostToDevice, s));
        if (tr.on) {      // (the staging rows of the directions are free: no sensitivity entry has a radius)
            double* hr = st + cap * (ldn + ldT);
            std::memcpy(hr, tr.radius + c0, cols * sizeof(double));
            HIPCHK(asmb::copy_async(w.rad, hr, cols * sizeof(double), hipMemcpyHostToDevice, s));
        }
        if (rhs.GZ) {
            // the weights on z, staged where the chunk's results will come back (free until then): gz_B by the complementary mask, then
            // ru -= H gz_B (one Hessian product on the block) and rw -= J[W, B] gz_B (the one product with the columns of B)
            double* hg = st + cap * (ldn + ldT + std::max<int64_t>(h->ev->n_dpar, 1));
            for (int c = 0; c < cols; ++c) {
                double* dg = hg + (int64_t)c * ldn;
                std::memcpy(dg, rhs.GZ + (c0 + c) * n, n * sizeof(double));
                for (int64_t j = n; j < ldn; ++j) dg[j] = 0.0;
            }
            HIPCHK(asmb::copy_async(va, hg, (int64_t)cols * ldn * sizeof(double), hipMemcpyHostToDevice, s));
            ops.site.gz_mask(va, f.mask, n, vb, h->ev->kk.cmask, cols);
            ops.hess(vb, va, cols);
            ops.site.axpby(1.0, b_ru, -1.0, va, nullptr, nullptr, b_ru, cols);
            if (nW > 0) {
                ops.mul_AB(vb, ta, cols);
                ops.site.axpby_rows(1.0, rww, -1.0, ta, nW, f.nWg, rww, cols);
            }
        }
        return;
    }
    case KktRhs::DATA:
        break;
    }
    EvalState& e = *h->ev;
    if (!e.data_dep) {      // nothing depends on the data, u = w = 0
        HIPCHK(asmb::fill_async(b_ru, 0, cap * ldn * sizeof(double), s));
        HIPCHK(asmb::fill_async(rww, 0, cap * ldT * sizeof(double), s));
        return;
    }
    const int64_t nd = e.n_dpar, R = e.nlp_rows;
    if (c0 == 0) {          // the multipliers of the block's rows, once
        cx_prepare(e, KKM_CW);
        if (R > 0) {
            std::memcpy(e.h_cx, lambda + e.F.n_rows, R * sizeof(double));
            HIPCHK(asmb::copy_async(e.d_cx_in, e.h_cx, R * sizeof(double), hipMemcpyHostToDevice, s));
        }
    }
    // the chunk's directions in the staging rows - every direction has its own - and their cross derivatives into the chunk's right-hand sides
    double* hd = st + cap * (ldn + ldT);
    std::memcpy(hd, rhs.DC + c0 * nd, (int64_t)cols * nd * sizeof(double));
    const CxRhs to{f.wrow, nW, b_ru, ldn, rww, ldT};
    nlp_cross_launch(e, s, cols, hd, &to);
}
// Steps 3 to 6 for the nrhs columns that `rhs` describes, in chunks of the work area's capacity (lambda: the multipliers of the point, read
// by the cross-derivative sweeps).  The element-wise and reduction kernels are the k_kktm_* family whatever the capacity; every product
// and substitution is ops'.  The answers go to `out`, a column's info to `sink` - the one place below that writes it - with the fields
// of the step where `tr` is on.
void kkt_columns(asm_handle* h, const KktFace& f, KktOps& ops, int32_t nrhs, const KktRhs& rhs, const double* lambda, const KktOut& out, const KktInfoSink& sink,
                 const KktTrust& tr, KktCounters& cnt) {
    const KktBufs& K = h->ev->kk;
    KktWork& w = ops.w;
    const hipStream_t s = h->stream;
    const int64_t n = h->sk->n, m = h->sk->m, ldn = h->sk->ldn, Mp = std::max<int64_t>(h->sk->Mp, 32), ldT = K.ldT, cap = w.cap, nW = f.nW;
    const double* const mask = f.mask;
    auto vblock = [&](int k) { return w.vec + (int64_t)k * cap * ldn; };
    auto rblock = [&](int k) { return w.row + (int64_t)k * cap * ldT; };      // (block 2 is ops.spare)
    double *b_ru = vblock(0), *dx0 = vblock(1), *cd = vblock(2), *cr = vblock(3), *cp = vblock(4), *hraw = vblock(5), *hp = vblock(6), *tt = vblock(7), *ddx = vblock(8),
           *hdx = vblock(9), *qq = vblock(10), *jtl = vblock(11), *ddz = vblock(12), *cg = vblock(13);
    double *rww = rblock(0), *tw = rblock(1), *dlw = rblock(3), *adx = rblock(4);
    double* const dlf = w.dlf;
    double* const scal = K.scal;
    const KktMulti R{K.part, K.cnt, scal, K.act, h->sk->d_hscal, h->sk->d_hseq};
    const KktSites& at = ops.site;
    const bool run_cg = f.nF > nW, trust = tr.on;
    int dropped = 0;
    cnt = {};
    for (int64_t c0 = 0; c0 < nrhs; c0 += cap) {
        const int cols = (int)std::min<int64_t>(cap, nrhs - c0);
        double* st = w.stage;                                    // [ru block | rw block | directions], then the results
        double* back = st + cap * (ldn + ldT + std::max<int64_t>(h->ev->n_dpar, 1));
        auto axpby = [&](double sa, const double* a, double sb, const double* b, const double* sc, double* out) {
            at.axpby(sa, a, sb, b, mask, sc, out, cols);
        };
        auto axpby_rows = [&](double sa, const double* a, double sb, const double* b, double* out) {
            at.axpby_rows(sa, a, sb, b, nW, f.nWg, out, cols);
        };
        // tt = A' S^-1 b for a block b over the working rows (t: where the substitution may work)
        auto normal_back = [&](const double* b, double* t) { ops.mul_AT(ops.solve_S(b, t, cols), tt, cols); };
        // v -= A' S^-1 A v for the columns that sc leaves active (all of them when sc == nullptr)
        auto project = [&](double* v, const double* sc) {
            if (nW == 0) return;
            ops.mul_A(v, tw, cols);
            normal_back(tw, tw);
            axpby(1.0, v, -1.0, tt, sc, v);
        };
        // 3. the right-hand sides of the chunk
        kkt_stage_rhs(h, f, ops, rhs, lambda, tr, c0, cols, b_ru, rww, hraw, hp, tw);
        // particular solution dx0 = -A' S^-1 rw_W
        if (nW > 0) {
            normal_back(rww, tw);
            axpby(-1.0, tt, 0.0, nullptr, nullptr, dx0);
            // one refinement step of the normal-equation solve: dx0 -= A' S^-1 (A dx0 + rw_W)
            ops.mul_A(dx0, adx, cols);
            axpby_rows(1.0, adx, 1.0, rww, tw);
            normal_back(tw, tw);
            axpby(1.0, dx0, -1.0, tt, nullptr, dx0);
        } else {
            HIPCHK(asmb::fill_async(dx0, 0, cap * ldn * sizeof(double), s));
        }
        // the share of the normal step that the radius admits: theta, dx0 <- theta dx0, Dt^2
        if (trust) at.normal(scal, w.rad, tr.share, dx0, cols);
        // 4. projected conjugate gradients on null(A), the columns in lockstep: minimise 1/2 d'H_FF d + (ru_F + H_FF dx0)'d
        HIPCHK(asmb::fill_async(cd, 0, cap * ldn * sizeof(double), s));
        if (run_cg) {
            ops.hess(dx0, hraw, cols);
            axpby(1.0, b_ru, 1.0, hraw, nullptr, cr);
            HIPCHK(asmb::fill_async(cp, 0, cap * ldn * sizeof(double), s));
            // the residual is kept projected (r = g = P P r): it then has no large component in range(A') for the projection's rounding to act on
            project(cr, nullptr);
            project(cr, nullptr);
            unsigned pub = pub_next(h);
            at.cg_dir(R, cr, 1, f.rtol, pub, (int)trust, cols);
            int active = kk_read_scal(h, pub);
            for (int64_t it = 0; active > 0 && it < f.max_iter; ++it) {
                at.cg_p(scal, cr, cp, cols);
                ops.hess(cp, hraw, cols);
                at.cg_curv(trust, R, cp, hraw, mask, cd, hp, cols);
                at.cg_step(scal, cp, hp, cd, cr, cols);
                project(cr, scal);
                project(cr, scal);
                pub = pub_next(h);
                at.cg_dir(R, cr, 0, f.rtol, pub, (int)trust, cols);
                active = kk_read_scal(h, pub);
                cnt.rounds += 1;
            }
            cnt.last_active = active;
        }
        // 5., 6. the solutions, their multipliers and residuals
        axpby(1.0, dx0, 1.0, cd, nullptr, ddx);
        ops.hess(ddx, hdx, cols);
        HIPCHK(asmb::fill_async(dlf, 0, cap * Mp * sizeof(double), s));
        if (nW > 0) {
            axpby(1.0, hdx, 1.0, b_ru, nullptr, qq);
            ops.mul_A(qq, tw, cols);
            ops.solve_S(tw, dlw, cols);
            // one refinement step: dlam_W += S^-1 A (q - A' dlam_W)
            ops.mul_AT(dlw, tt, cols);
            axpby(1.0, qq, -1.0, tt, nullptr, cg);
            ops.mul_A(cg, tw, cols);
            axpby_rows(1.0, dlw, 1.0, ops.solve_S(tw, tw, cols), dlw);
            at.scatter(dlw, f.wrow, nW, f.nWg, dlf, Mp, cols);
            ops.mul_A(ddx, adx, cols);
            ops.jt_dlam(dlw, dlf, jtl, cols);
        } else {
            HIPCHK(asmb::fill_async(jtl, 0, cap * ldn * sizeof(double), s));
        }
        at.finish(scal, hdx, b_ru, jtl, mask, n, adx, rww, nW, ddz, trust ? (const double*)ddx : (const double*)nullptr, cols);
        // (a variable-bound column: the moved variable itself, dx[j] = delta; the chunk's [delta | vars] are still in w.bnd)
        if (rhs.kind == KktRhs::VAR_BOUND)
            at.var_dx(reinterpret_cast<const int*>(w.bnd + cols), rhs.delta ? (const double*)w.bnd : (const double*)nullptr, mask, cols, ddx);
        HIPCHK(asmb::copy_async(back, ddx, (int64_t)cols * ldn * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(asmb::copy_async(back + cap * ldn, ddz, (int64_t)cols * ldn * sizeof(double), hipMemcpyDeviceToHost, s));
        if (m > 0) HIPCHK(asmb::copy_async(back + 2 * cap * ldn, dlf, (int64_t)cols * Mp * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(asmb::copy_async(back + cap * (2 * ldn + Mp), scal, (int64_t)cols * KKM_SCAL * sizeof(double), hipMemcpyDeviceToHost, s));
        if (c0 == 0) HIPCHK(asmb::copy_async(back + cap * (2 * ldn + Mp + KKM_SCAL), K.dropped, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(asmb::sync(s));
        if (c0 == 0) dropped = *reinterpret_cast<const int*>(back + cap * (2 * ldn + Mp + KKM_SCAL));
        for (int c = 0; c < cols; ++c) {
            std::memcpy(out.DX + (c0 + c) * n, back + (int64_t)c * ldn, n * sizeof(double));
            if (out.DZ) std::memcpy(out.DZ + (c0 + c) * n, back + cap * ldn + (int64_t)c * ldn, n * sizeof(double));
            if (m > 0) std::memcpy(out.DLAM + (c0 + c) * m, back + 2 * cap * ldn + (int64_t)c * Mp, m * sizeof(double));
            const double* sc = back + cap * (2 * ldn + Mp) + (int64_t)c * KKM_SCAL;
            // (without an iteration - a vertex - the column's stop code and count are not written: solved, no iteration)
            const int stop = run_cg ? (int)sc[KK_STOP] : 1;
            auto shared_fields = [&](auto& o) {
                o.status = dropped > 0 ? 3 : (stop == 2 ? 2 : (stop == 0 ? 1 : 0));
                o.cg_iters = run_cg ? (int32_t)sc[KKM_ITERS] : 0; o.n_free = (int32_t)f.nF; o.n_rows = (int32_t)nW; o.dropped_pivots = dropped;
                o.res_stat = sc[KK_RSTAT]; o.res_feas = sc[KK_RFEAS];
            };
            if (sink.step) {
                asm_kkt_step_info& o = sink.step[c0 + c];
                shared_fields(o);
                o.boundary = run_cg ? (int32_t)sc[KKM_BND] : 0;
                o.theta = sc[KKM_THETA]; o.norm_normal = sc[KKM_NNORM]; o.norm_step = sc[KKM_NSTEP]; o.model = sc[KKM_MODEL];
            } else {
                shared_fields(sink.plain[c0 + c]);
            }
        }
    }
    ops.dev.resolve_timing();      // (a batch slot records no events - its timing level stays 0, as for its LPs: nothing to read inside a fiber)
}
// The refusals the entries of the family share, under the entry's name `who`: per handle (kkt_run) and, on the calling thread, for a
// scenario batch - which so refuses exactly what its fibers would.  out == nullptr: the adjoint entries, whose states are optional.
void kkt_check_args(const std::string& who, int64_t m, int64_t nd, int32_t nrhs, const KktPoint& p, const KktRhs& rhs, const KktOut* out, const KktInfoSink& sink,
                    int64_t n = 0) {      // (n: read for VAR_BOUND alone)
    if (nrhs < 1) throw std::invalid_argument(who + ": nrhs < 1");
    bool null = !p.x || !p.bound_state || sink.null() || (m > 0 && (!p.lambda || !p.row_state));
    if (out) null = null || !out->DX || (m > 0 && !out->DLAM);
    if (rhs.kind == KktRhs::GIVEN) null = null || !rhs.RU || (m > 0 && !rhs.RW);
    if (rhs.kind == KktRhs::DATA) null = null || (nd > 0 && !rhs.DC);
    if (rhs.kind == KktRhs::BOUND || rhs.kind == KktRhs::VAR_BOUND) null = null || !rhs.rows;
    if (null) throw std::invalid_argument(who + ": null pointer");
    if (rhs.kind == KktRhs::VAR_BOUND)
        for (int32_t c = 0; c < nrhs; ++c)
            if (rhs.rows[c] < 0 || rhs.rows[c] >= n) throw std::invalid_argument(who + ": a variable index outside [0, n)");
    if (rhs.kind == KktRhs::BOUND)
        for (int32_t c = 0; c < nrhs; ++c)
            if (rhs.rows[c] < 0 || rhs.rows[c] >= m) throw std::invalid_argument(who + ": a row index outside [0, m)");
}
// Every per-handle entry of the family, under its name `who`: its refusals, the face, the back end, the columns, the round counters.
// cap, the capacity of the work area - 1 (asm_kkt_solve, asm_kkt_step and what runs through them) or KKM_CW (the multi entries) - and
// the form choose the back end, here and nowhere else.  Only a call with cap == KKM_CW leaves its counters on the handle
// (asm_test_kkt_multi_rounds: the last multi call).  exact_only: a derivative entry with given columns (adjoint states, asm_solution_sensitivity).
void kkt_run(asm_handle* h, const char* who, int64_t cap, const KktPoint& p, int32_t nrhs, const KktRhs& rhs, const asm_kkt_params* par, const KktOut& out,
             const KktInfoSink& sink, const KktTrust& tr = KktTrust(), bool exact_only = false) {
    const std::string me(who);
    const bool exact = rhs.derivative() || exact_only;
    if (rhs.kind == KktRhs::DATA) cx_check(h, who);
    if (exact) hs_check(h, who);
    const bool lm = !exact && kkt_hess_lm(h, who);
    kkt_check_args(me, h->sk->m, h->ev->n_dpar, nrhs, p, rhs, &out, sink, h->sk->n);
    tr.check(me, nrhs);
    if (rhs.GZ) kk_gz(h);
    Dev dev(h);
    const KktFace f(h, dev, me, p.x, p.lambda, p.row_state, p.bound_state, par, lm);
    KktCounters own;
    KktCounters& cnt = cap == KKM_CW ? h->ev->kkm : own;
    auto columns = [&](KktOps&& ops) { kkt_columns(h, f, ops, nrhs, rhs, p.lambda, out, sink, tr, cnt); };
    if (f.sparse) columns(KktSparse(h, dev, f, *kk_work(h, cap, true)));
    else if (cap == 1) columns(KktOneColumn(h, dev, f, *kk_work(h, 1)));
    else columns(KktBlock(h, dev, f, *kk_work(h, cap)));
}
}  // namespace

// asm_kkt_solve; asm_solution_sensitivity comes here too (exact_only), with the column it made
static void do_kkt_solve(asm_handle* h, const KktPoint& p, const double* ru, const double* rw, const asm_kkt_params* par, const KktOut& out, asm_kkt_info* info,
                         bool exact_only = false) {
    kkt_run(h, "asm_kkt_solve", 1, p, 1, KktRhs::given(ru, rw), par, out, info, KktTrust(), exact_only);
}
static void do_solution_sensitivity(asm_handle* h, const KktPoint& p, const double* dc, const asm_kkt_params* par, const KktOut& out, asm_kkt_info* info) {
    cx_check(h, "asm_solution_sensitivity");
    if (!p.x || !p.bound_state || !out.DX || !info || (h->sk->m > 0 && (!p.lambda || !p.row_state || !out.DLAM)) || (h->ev->n_dpar > 0 && !dc))
        throw std::invalid_argument("asm_solution_sensitivity: null pointer");
    std::vector<double> u((size_t)std::max<int64_t>(h->sk->n, 1)), w((size_t)std::max<int64_t>(h->sk->m, 1));
    do_data_cross(h, p.x, p.lambda, dc, u.data(), w.data());
    do_kkt_solve(h, p, u.data(), w.data(), par, out, info, true);
}
// The multi entries under the name `who`, for the per-handle call and for a batch fiber: asm_kkt_solve_multi (KktRhs::given),
// asm_solution_sensitivity_multi (data), asm_bound_sensitivity_multi (bound) and asm_var_bound_sensitivity_multi (var_bound)
static void do_kkt_solve_multi(asm_handle* h, const char* who, const KktPoint& p, int32_t nrhs, const KktRhs& rhs, const asm_kkt_params* par, const KktOut& out,
                               asm_kkt_info* info) {
    kkt_run(h, who, KKM_CW, p, nrhs, rhs, par, out, info);
}
// ---- adjoint solution sensitivities (include/asm_hip.h, "Adjoint solution sensitivities"): per function the adjoint state (ax, al) =
// asm_kkt_solve(ru = -gx, rw = gl), then out = the transposed cross derivative for the weights (-ax, al) and dbound_i = -al_i on the working
// rows, 0.0 elsewhere.  A derivative entry: the exact Hessian whatever the handle's type.
namespace {
// the kinds the adjoint entries serve: those of asm_solution_sensitivity, and the function store alone (kind 0) - no data, an empty out,
// but the bound gradient and the adjoint state need no data derivative.  Kinds 1 and 2 end in the solve's hs_check.
void adjoint_check(const asm_handle* h, const char* who) {
    if (ev_of(h, who).family != NlpFamily::NONE) cx_check(h, who);
}
// the refusals of the adjoint entries, per handle and for a batch: those of the solve with the gradients as its columns, and OUT
void adjoint_check_args(const std::string& who, int64_t m, int64_t nd, int32_t nrhs, const KktPoint& p, const double* GX, const double* GL, const double* OUT,
                        asm_kkt_info* info) {
    kkt_check_args(who, m, nd, nrhs, p, KktRhs::given(GX, GL), nullptr, info);
    if (nd > 0 && !OUT) throw std::invalid_argument(who + ": null pointer");
}
// what the adjoint entries set up for ncol functions: ru = -GX, and buffers of their own for the adjoint states the caller does not take
struct AdjointSetup {
    std::vector<double> ru, sx, sl;
    KktOut state;      // AX and AL, the caller's or the buffers here
    AdjointSetup(int64_t ncol, int64_t n, int64_t m, const double* GX, double* AX, double* AL)
        : ru((size_t)std::max<int64_t>(ncol * n, 1)), sx(AX ? 0 : ru.size()), sl(AL ? 0 : (size_t)std::max<int64_t>(ncol * m, 1)),
          state{AX ? AX : sx.data(), AL ? AL : sl.data(), nullptr} {
        for (int64_t q = 0; q < ncol * n; ++q) ru[q] = -GX[q];
    }
};
void adjoint_dbound(const int32_t* row_state, int64_t m, int64_t ncol, const double* AL, double* DBOUND) {
    if (!DBOUND) return;
    for (int64_t c = 0; c < ncol; ++c)
        for (int64_t i = 0; i < m; ++i) DBOUND[c * m + i] = row_state[i] == 1 ? -AL[c * m + i] : 0.0;
}
// what follows the checks and the set-up in every adjoint entry, per handle and in a batch fiber: the states by the solve `who` of
// capacity cap on rhs = given(-GX, GL), exact whatever the handle's type, then the data derivatives and the bound gradients
void adjoint_multi(asm_handle* h, const char* who, int64_t cap, const KktPoint& p, int32_t nrhs, const KktRhs& rhs, const asm_kkt_params* par, double* OUT, double* DBOUND,
                   const KktOut& state, asm_kkt_info* info) {
    kkt_run(h, who, cap, p, nrhs, rhs, par, state, info, KktTrust(), true);
    ct_columns(h, p.x, p.lambda, nrhs, state.DX, -1.0, state.DLAM, OUT, cap);
    adjoint_dbound(p.row_state, h->sk->m, nrhs, state.DLAM, DBOUND);
}
// the same for the entries with weights on the bound multipliers (asm_solution_adjoint_z*): rhs carries GZ (KktRhs::with_gz; absent: the
// launches of adjoint_multi, nothing prepared with zeros), the solve also returns its dz, the transposed sweep takes vx = gz_B - ax, and
// dxbound_j = -dz_j on B, 0.0 on F
void adjoint_z_multi(asm_handle* h, const char* who, int64_t cap, const KktPoint& p, int32_t nrhs, const KktRhs& rhs, const asm_kkt_params* par, double* OUT, double* DBOUND,
                     double* DXBOUND, const KktOut& state, asm_kkt_info* info) {
    const int64_t n = h->sk->n;
    std::vector<double> dz((size_t)std::max<int64_t>(nrhs * n, 1));
    kkt_run(h, who, cap, p, nrhs, rhs, par, {state.DX, state.DLAM, dz.data()}, info, KktTrust(), true);
    if (rhs.GZ) {
        std::vector<double> vx(dz.size());
        for (int64_t c = 0; c < nrhs; ++c)
            for (int64_t j = 0; j < n; ++j) vx[c * n + j] = (p.bound_state[j] != 0 ? rhs.GZ[c * n + j] : 0.0) - state.DX[c * n + j];
        ct_columns(h, p.x, p.lambda, nrhs, vx.data(), 1.0, state.DLAM, OUT, cap);
    } else {
        ct_columns(h, p.x, p.lambda, nrhs, state.DX, -1.0, state.DLAM, OUT, cap);
    }
    adjoint_dbound(p.row_state, h->sk->m, nrhs, state.DLAM, DBOUND);
    if (DXBOUND)
        for (int64_t c = 0; c < nrhs; ++c)
            for (int64_t j = 0; j < n; ++j) DXBOUND[c * n + j] = p.bound_state[j] != 0 ? -dz[c * n + j] : 0.0;
}
}  // namespace
static void do_solution_adjoint_z(asm_handle* h, const KktPoint& p, const double* gx, const double* gl, const double* gz, const asm_kkt_params* par, double* out, double* dbound,
                                  double* dxbound, double* ax, double* al, asm_kkt_info* info) {
    adjoint_check(h, "asm_solution_adjoint_z");
    const int64_t n = h->sk->n, m = h->sk->m;
    adjoint_check_args("asm_solution_adjoint_z", m, h->ev->n_dpar, 1, p, gx, gl, out, info);
    const AdjointSetup A(1, n, m, gx, ax, al);
    adjoint_z_multi(h, "asm_kkt_solve", 1, p, 1, KktRhs::given(A.ru.data(), gl).with_gz(gz), par, out, dbound, dxbound, A.state, info);
}
static void do_solution_adjoint_z_multi(asm_handle* h, const KktPoint& p, int32_t nrhs, const double* GX, const double* GL, const double* GZ, const asm_kkt_params* par,
                                        double* OUT, double* DBOUND, double* DXBOUND, double* AX, double* AL, asm_kkt_info* info) {
    const char* who = "asm_solution_adjoint_z_multi";
    adjoint_check(h, who);
    hs_check(h, who);
    const int64_t n = h->sk->n, m = h->sk->m;
    adjoint_check_args(who, m, h->ev->n_dpar, nrhs, p, GX, GL, OUT, info);
    const AdjointSetup A(nrhs, n, m, GX, AX, AL);
    adjoint_z_multi(h, who, KKM_CW, p, nrhs, KktRhs::given(A.ru.data(), GL).with_gz(GZ), par, OUT, DBOUND, DXBOUND, A.state, info);
}
static void do_solution_adjoint(asm_handle* h, const KktPoint& p, const double* gx, const double* gl, const asm_kkt_params* par, double* out, double* dbound, double* ax,
                                double* al, asm_kkt_info* info) {
    adjoint_check(h, "asm_solution_adjoint");
    const int64_t n = h->sk->n, m = h->sk->m;
    adjoint_check_args("asm_solution_adjoint", m, h->ev->n_dpar, 1, p, gx, gl, out, info);
    const AdjointSetup A(1, n, m, gx, ax, al);
    adjoint_multi(h, "asm_kkt_solve", 1, p, 1, KktRhs::given(A.ru.data(), gl), par, out, dbound, A.state, info);
}
static void do_solution_adjoint_multi(asm_handle* h, const KktPoint& p, int32_t nrhs, const double* GX, const double* GL, const asm_kkt_params* par, double* OUT,
                                      double* DBOUND, double* AX, double* AL, asm_kkt_info* info) {
    const char* who = "asm_solution_adjoint_multi";
    adjoint_check(h, who);
    hs_check(h, who);
    const int64_t n = h->sk->n, m = h->sk->m;
    adjoint_check_args(who, m, h->ev->n_dpar, nrhs, p, GX, GL, OUT, info);
    const AdjointSetup A(nrhs, n, m, GX, AX, AL);
    adjoint_multi(h, who, KKM_CW, p, nrhs, KktRhs::given(A.ru.data(), GL), par, OUT, DBOUND, A.state, info);
}
// asm_kkt_step (one column) and asm_kkt_step_multi: the solve's entry with a radius per column and the share of the normal step
static void do_kkt_step(asm_handle* h, const char* who, bool multi, const KktPoint& p, int32_t nrhs, const KktRhs& rhs, const double* RADIUS,
                        const asm_kkt_step_params* par, const KktOut& out, asm_kkt_step_info* info) {
    const asm_kkt_params kp{par ? par->max_iter : 0, par ? par->rtol : 0.0};
    kkt_run(h, who, multi ? KKM_CW : 1, p, nrhs, rhs, par ? &kp : nullptr, out, info, KktTrust::step(RADIUS, par ? par->normal_share : KktTrust().share));
}

// eval_f + eval_g at a trial point (compute_alpha, slp_line_search.jl:222-244; step_quality, slp_trust_region.jl:213-251)
static void do_eval_constraints(asm_handle* h, const double* x, double* f, double* E) {
    EvalState& e = ev_of(h, "asm_eval_constraints");
    if (!x || !f || (h->sk->m > 0 && !E)) throw std::invalid_argument("asm_eval_constraints: null pointer");
    HIPCHK(hipSetDevice(h->device));
    const int64_t n = h->sk->n, m = h->sk->m;
    double *st = e.h_stage, *s_E = st + e.L.st_E(false), *s_f = st + e.L.st_f(false);
    std::memcpy(st, x, n * sizeof(double));
    HIPCHK(asmb::copy_async(e.d_xt, st, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    ev_launch(h, e.d_xt, e.d_Et, e.d_f + 1, false);
    if (m) HIPCHK(asmb::copy_async(s_E, e.d_Et, m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(asmb::copy_async(s_f, e.d_f + 1, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(asmb::sync(h->stream));
    if (m) std::memcpy(E, s_E, m * sizeof(double));
    *f = *s_f;
}

int asm_eval_constraints(asm_handle* h, const double* x, double* f, double* E) {
    return guarded(h, [&] { do_eval_constraints(h, x, f, E); });
}

int asm_eval_jacobian_values(asm_handle* h, double* dE_out) {
    return guarded(h, [&] {
        if (!dE_out) throw std::invalid_argument("asm_eval_jacobian_values: null pointer");
        const Skeleton& K = sk_of(h, "asm_eval_jacobian_values: asm_sublp_setup first");
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(asmb::copy(dE_out, K.d_dE, K.nnz * sizeof(double), hipMemcpyDeviceToHost));
    });
}

int asm_eval_set_data(asm_handle* h, int64_t offset, int64_t count, const double* values) {
    return guarded(h, [&] { do_set_data(h, offset, count, values); });
}

int asm_eval_data_gradient(asm_handle* h, const double* x, const double* lambda, double* out) {
    return guarded(h, [&] { do_data_gradient(h, x, lambda, out); });
}

int asm_eval_data_cross(asm_handle* h, const double* x, const double* lambda, const double* dc, double* u, double* w) {
    return guarded(h, [&] { do_data_cross(h, x, lambda, dc, u, w); });
}

int asm_kkt_solve(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, const double* ru, const double* rw,
                  const asm_kkt_params* par, double* dx, double* dlam, double* dz, asm_kkt_info* info) {
    return guarded(h, [&] { do_kkt_solve(h, {x, lambda, row_state, bound_state}, ru, rw, par, {dx, dlam, dz}, info); });
}

int asm_solution_sensitivity(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, const double* dc,
                             const asm_kkt_params* par, double* dx, double* dlam, double* dz, asm_kkt_info* info) {
    return guarded(h, [&] { do_solution_sensitivity(h, {x, lambda, row_state, bound_state}, dc, par, {dx, dlam, dz}, info); });
}

int asm_kkt_solve_multi(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs, const double* RU,
                        const double* RW, const asm_kkt_params* par, double* DX, double* DLAM, double* DZ, asm_kkt_info* info) {
    return guarded(h, [&] { do_kkt_solve_multi(h, "asm_kkt_solve_multi", {x, lambda, row_state, bound_state}, nrhs, KktRhs::given(RU, RW), par, {DX, DLAM, DZ}, info); });
}

int asm_solution_sensitivity_multi(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs, const double* DC,
                                   const asm_kkt_params* par, double* DX, double* DLAM, double* DZ, asm_kkt_info* info) {
    return guarded(h, [&] { do_kkt_solve_multi(h, "asm_solution_sensitivity_multi", {x, lambda, row_state, bound_state}, nrhs, KktRhs::data(DC), par, {DX, DLAM, DZ}, info); });
}

int asm_bound_sensitivity_multi(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs, const int32_t* rows,
                                const double* delta, const asm_kkt_params* par, double* DX, double* DLAM, double* DZ, asm_kkt_info* info) {
    return guarded(h, [&] {
        if (!rows) throw std::invalid_argument("asm_bound_sensitivity_multi: null pointer");
        do_kkt_solve_multi(h, "asm_bound_sensitivity_multi", {x, lambda, row_state, bound_state}, nrhs, KktRhs::bound(rows, delta), par, {DX, DLAM, DZ}, info);
    });
}

int asm_eval_data_cross_t(asm_handle* h, const double* x, const double* lambda, const double* vx, const double* vl, double* out) {
    return guarded(h, [&] { do_data_cross_t(h, x, lambda, vx, vl, out); });
}

int asm_solution_adjoint(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, const double* gx, const double* gl,
                         const asm_kkt_params* par, double* out, double* dbound, double* ax, double* al, asm_kkt_info* info) {
    return guarded(h, [&] { do_solution_adjoint(h, {x, lambda, row_state, bound_state}, gx, gl, par, out, dbound, ax, al, info); });
}

int asm_solution_adjoint_multi(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs, const double* GX,
                               const double* GL, const asm_kkt_params* par, double* OUT, double* DBOUND, double* AX, double* AL, asm_kkt_info* info) {
    return guarded(h, [&] { do_solution_adjoint_multi(h, {x, lambda, row_state, bound_state}, nrhs, GX, GL, par, OUT, DBOUND, AX, AL, info); });
}

// ---- Validity ranges (include/asm_hip.h, "Validity ranges"): how far a column (dx, dlam, dz) of the sensitivity entries may be followed
// before the working set changes.  The ONE place that launches asm_range_kernels.hip.h.
static_assert(RG_CW == ASM_KKT_CHUNK && RG_CW % RG_CPB == 0 && RG_CPB == 4 * RG_CPT, "the chunk width of the header is the kernels'");
static_assert(sizeof(RangeOut) == sizeof(asm_range_info) && offsetof(RangeOut, pos_hi) == offsetof(asm_range_info, pos_hi), "asm_range_info is the kernels' RangeOut");
// what the entry refuses without a launch, per handle and - on the calling thread - for a scenario batch (n_scen points)
static void rg_check_args(const std::string& me, int64_t n, int64_t m, int64_t n_scen, const double* x, const double* lambda, const double* z, const int32_t* row_state,
                          const int32_t* bound_state, int32_t nrhs, const double* DX, const double* DLAM, const double* DZ, const asm_range_info* out) {
    if (nrhs < 1) throw std::invalid_argument(me + ": nrhs < 1");
    if (!x || !z || !bound_state || !DX || !DZ || !out || (m > 0 && (!lambda || !row_state || !DLAM))) throw std::invalid_argument(me + ": null pointer");
    for (int64_t j = 0; j < n_scen * n; ++j)
        if (bound_state[j] < -1 || bound_state[j] > 1) throw std::invalid_argument(me + ": bound_state holds a value outside {-1, 0, +1}");
    for (int64_t i = 0; i < n_scen * m; ++i)
        if (row_state[i] != 0 && row_state[i] != 1) throw std::invalid_argument(me + ": row_state holds a value outside {0, 1}");
}
// once per asm_eval_setup, at the first call (for a slot of a scenario batch before its fiber starts)
static void rg_prepare(asm_handle* h) {
    RangeBufs& G = h->ev->rg;
    if (G.ready) return;
    HIPCHK(hipSetDevice(h->device));
    BufPool& M = h->ev->mem;
    const hipStream_t s = h->stream;
    const Skeleton& S = *h->sk;
    const int64_t ldn = S.ldn, Mp = std::max<int64_t>(S.Mp, 32), ni = (Mp + ldn + 1) / 2, per = 2 * ldn + Mp;
    G.n_row_wg = (S.m + RG_TILE - 1) / RG_TILE;
    G.n_var_wg = (S.n + RG_TILE - 1) / RG_TILE;
    const int64_t slots = G.n_row_wg + G.n_var_wg;
    M.alloc(G.dE, S.nnz);
    if (S.sp_ok) M.zeroed(G.vals, S.sp_nnz, s);
    else M.zeroed(G.J, Mp * ldn, s);
    M.zeroed(G.pt, Mp + ldn + ni, s);
    M.zeroed(G.cols, RG_CW * per, s);
    M.zeroed(G.part_t, slots * RG_CW * 2, s);
    M.zeroed(G.part_k, slots * RG_CW * 4, s);
    M.zeroed(G.cnt, RG_CW / RG_CPB + 2, s);
    M.zeroed(G.out, RG_CW, s);
    M.alloc(G.stage, std::max(Mp + ldn + ni, RG_CW * per) + RG_CW * (int64_t)(sizeof(RangeOut) / sizeof(double)), BufPool::PINNED);
    HIPCHK(asmb::sync(s));
    G.ready = true;
}
// The entry under the name `who`, for the per-handle call and for a batch fiber (the arguments are checked by the caller).  E and the
// Jacobian values at x by the evaluator's launches into buffers of the entry's own (d_xt, d_Et and RangeBufs: the LP's inputs stay), the
// values summed into the CSR list of the pattern or assembled into dense rows; then per chunk one upload, the two launches, one read-back.
static void rg_run(asm_handle* h, const double* x, const double* lambda, const double* z, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs,
                   const double* DX, const double* DLAM, const double* DZ, asm_range_info* out) {
    rg_prepare(h);
    HIPCHK(hipSetDevice(h->device));
    EvalState& e = *h->ev;
    RangeBufs& G = e.rg;
    const Skeleton& S = *h->sk;
    const hipStream_t s = h->stream;
    const int64_t n = S.n, m = S.m, ldn = S.ldn, Mp = std::max<int64_t>(S.Mp, 32);
    // the point: x where the evaluator's launches read it; [lam | z | row_state | bound_state] in one upload
    std::memcpy(e.h_stage, x, n * sizeof(double));
    HIPCHK(asmb::copy_async(e.d_xt, e.h_stage, n * sizeof(double), hipMemcpyHostToDevice, s));
    double* st = G.stage;
    int* sti = reinterpret_cast<int*>(st + Mp + ldn);
    for (int64_t i = 0; i < Mp; ++i) { st[i] = i < m ? lambda[i] : 0.0; sti[i] = i < m ? row_state[i] : 0; }
    for (int64_t j = 0; j < ldn; ++j) { st[Mp + j] = j < n ? z[j] : 0.0; sti[Mp + j] = j < n ? bound_state[j] : 0; }
    HIPCHK(asmb::copy_async(G.pt, st, (Mp + ldn) * sizeof(double) + (Mp + ldn) * sizeof(int), hipMemcpyHostToDevice, s));
    h2d_done(h);      // (the staging area is written again for the first chunk)
    fn_rows_launch(e, s, e.d_xt, e.d_Et, G.dE, 1);
    nlp_rows_launch(e, s, e.d_xt, e.d_Et, G.dE, 1);
    if (S.sp_ok) {
        asmb::launch(k_kkts_vals, dim3((unsigned)std::min<int64_t>((S.nu + 255) / 256, 4096)), dim3(256), s, G.dE, S.d_perm, S.d_ustart, S.nu, G.vals);
    } else if (S.dense_fast) {
        asmb::launch(k_assemble_dense, dim3((unsigned)std::min<int64_t>((m * n + 255) / 256, 4096)), dim3(256), s, G.dE, G.J, m, n, ldn);
    } else if (S.nu > 0) {
        asmb::launch(k_assemble, dim3((unsigned)std::min<int64_t>((S.nu + 255) / 256, 4096)), dim3(256), s, G.dE, S.d_perm, S.d_ustart, S.d_uoff, S.d_adjoff, G.J, S.nu);
    }
    const EvLayout& L = e.L;
    const RangePoint P{e.d_Et, L.g_L(), L.g_U(), G.pt, reinterpret_cast<const int*>(G.pt + Mp + ldn), e.d_xt, L.x_L(), L.x_U(), G.pt + Mp,
                       reinterpret_cast<const int*>(G.pt + Mp + ldn) + Mp, m, n};
    const RangeRed R{G.part_t, G.part_k, G.cnt};
    for (int32_t c0 = 0; c0 < nrhs; c0 += RG_CW) {
        const int cols = (int)std::min<int32_t>(RG_CW, nrhs - c0);
        // the chunk's columns, packed [DX (cols x ldn) | DZ (cols x ldn) | DLAM (cols x Mp)] with the padding cleared: one upload
        double *sx = st, *sz = sx + (int64_t)cols * ldn, *sl = sz + (int64_t)cols * ldn;
        for (int c = 0; c < cols; ++c) {
            std::memcpy(sx + (int64_t)c * ldn, DX + (int64_t)(c0 + c) * n, n * sizeof(double));
            std::memcpy(sz + (int64_t)c * ldn, DZ + (int64_t)(c0 + c) * n, n * sizeof(double));
            for (int64_t j = n; j < ldn; ++j) sx[(int64_t)c * ldn + j] = sz[(int64_t)c * ldn + j] = 0.0;
            if (m > 0) std::memcpy(sl + (int64_t)c * Mp, DLAM + (int64_t)(c0 + c) * m, m * sizeof(double));
            for (int64_t i = m; i < Mp; ++i) sl[(int64_t)c * Mp + i] = 0.0;
        }
        HIPCHK(asmb::copy_async(G.cols, st, (int64_t)cols * (2 * ldn + Mp) * sizeof(double), hipMemcpyHostToDevice, s));
        const double *dx = G.cols, *dz = dx + (int64_t)cols * ldn, *dl = dz + (int64_t)cols * ldn;
        const unsigned gy = (unsigned)((cols + RG_CPB - 1) / RG_CPB);
        if (S.sp_ok)
            asmb::launch(k_range_rows_sparse, dim3((unsigned)G.n_row_wg, gy), dim3(256), s, P, (const int*)S.d_sp_ptr, (const int*)S.d_sp_col, (const double*)G.vals, dx, ldn, dl, Mp, cols, R);
        else
            asmb::launch(k_range_rows_dense, dim3((unsigned)G.n_row_wg, gy), dim3(256), s, P, (const double*)G.J, dx, ldn, dl, Mp, cols, R);
        asmb::launch(k_range_vars, dim3((unsigned)G.n_var_wg, gy), dim3(256), s, P, dx, dz, ldn, cols, (int)G.n_row_wg, R, G.out);
        RangeOut* back = reinterpret_cast<RangeOut*>(st + std::max(Mp + ldn + (Mp + ldn + 1) / 2, RG_CW * (2 * ldn + Mp)));
        HIPCHK(asmb::copy_async(back, G.out, cols * sizeof(RangeOut), hipMemcpyDeviceToHost, s));
        HIPCHK(asmb::sync(s));
        std::memcpy(out + c0, back, cols * sizeof(RangeOut));
    }
}
static void do_sensitivity_range(asm_handle* h, const double* x, const double* lambda, const double* z, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs,
                                 const double* DX, const double* DLAM, const double* DZ, asm_range_info* out) {
    const char* who = "asm_sensitivity_range_multi";
    ev_of(h, who);
    rg_check_args(who, h->sk->n, h->sk->m, 1, x, lambda, z, row_state, bound_state, nrhs, DX, DLAM, DZ, out);
    rg_run(h, x, lambda, z, row_state, bound_state, nrhs, DX, DLAM, DZ, out);
}

int asm_sensitivity_range_multi(asm_handle* h, const double* x, const double* lambda, const double* z, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs,
                                const double* DX, const double* DLAM, const double* DZ, asm_range_info* out) {
    return guarded(h, [&] { do_sensitivity_range(h, x, lambda, z, row_state, bound_state, nrhs, DX, DLAM, DZ, out); });
}

int asm_var_bound_sensitivity_multi(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs,
                                    const int32_t* vars, const double* delta, const asm_kkt_params* par, double* DX, double* DLAM, double* DZ, asm_kkt_info* info) {
    return guarded(h, [&] {
        do_kkt_solve_multi(h, "asm_var_bound_sensitivity_multi", {x, lambda, row_state, bound_state}, nrhs, KktRhs::var_bound(vars, delta), par, {DX, DLAM, DZ}, info);
    });
}

int asm_solution_adjoint_z(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, const double* gx, const double* gl,
                           const double* gz, const asm_kkt_params* par, double* out, double* dbound, double* dxbound, double* ax, double* al, asm_kkt_info* info) {
    return guarded(h, [&] { do_solution_adjoint_z(h, {x, lambda, row_state, bound_state}, gx, gl, gz, par, out, dbound, dxbound, ax, al, info); });
}

int asm_solution_adjoint_z_multi(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs, const double* GX,
                                 const double* GL, const double* GZ, const asm_kkt_params* par, double* OUT, double* DBOUND, double* DXBOUND, double* AX, double* AL,
                                 asm_kkt_info* info) {
    return guarded(h, [&] { do_solution_adjoint_z_multi(h, {x, lambda, row_state, bound_state}, nrhs, GX, GL, GZ, par, OUT, DBOUND, DXBOUND, AX, AL, info); });
}

int asm_kkt_set_form(asm_handle* h, int32_t form) {
    return guarded(h, [&] {
        EvalState& e = ev_of(h, "asm_kkt_set_form");
        if (form != ASM_KKT_DENSE && form != ASM_KKT_SPARSE) throw std::invalid_argument("asm_kkt_set_form: form is neither ASM_KKT_DENSE nor ASM_KKT_SPARSE");
        e.kk.form = form;
    });
}
int asm_kkt_set_order(asm_handle* h, int32_t order) {
    return guarded(h, [&] {
        EvalState& e = ev_of(h, "asm_kkt_set_order");
        if (order != ASM_KKT_ORDER_WORKING_SET && order != ASM_KKT_ORDER_STATIC)
            throw std::invalid_argument("asm_kkt_set_order: order is neither ASM_KKT_ORDER_WORKING_SET nor ASM_KKT_ORDER_STATIC");
        e.kk.order = order;
    });
}
int asm_kkt_order_info(const asm_handle* h, struct asm_kkt_order_info* out) {
    if (!h || !out) return ASM_ERR_ARG;
    if (!h->ev) return ASM_ERR_STATE;
    const KktBufs& K = h->ev->kk;
    *out = {K.order, K.order_used, K.s_band, K.s_npairs};
    return ASM_OK;
}
int asm_kkt_row_order(const asm_handle* h, int32_t* rows, int64_t* nW) {
    if (!h || !nW) return ASM_ERR_ARG;
    if (!h->ev) return ASM_ERR_STATE;
    const std::vector<int>& L = h->ev->kk.last_rows;
    *nW = (int64_t)L.size();
    if (rows) std::copy(L.begin(), L.end(), rows);
    return ASM_OK;
}
int asm_kkt_form_info(const asm_handle* h, struct asm_kkt_form_info* out) {
    if (!h || !out) return ASM_ERR_ARG;
    if (!h->ev) return ASM_ERR_STATE;
    const KktBufs& K = h->ev->kk;
    *out = K.last;
    out->form_requested = K.form;
    out->dense_bytes = K.dense_bytes;
    out->sparse_bytes = K.sparse_bytes;
    return ASM_OK;
}
int asm_kkt_step(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, const double* ru, const double* rw,
                 double radius, const asm_kkt_step_params* par, double* dx, double* dlam, double* dz, asm_kkt_step_info* info) {
    return guarded(h, [&] { do_kkt_step(h, "asm_kkt_step", false, {x, lambda, row_state, bound_state}, 1, KktRhs::given(ru, rw), &radius, par, {dx, dlam, dz}, info); });
}

int asm_kkt_step_multi(asm_handle* h, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs, const double* RU,
                       const double* RW, const double* RADIUS, const asm_kkt_step_params* par, double* DX, double* DLAM, double* DZ, asm_kkt_step_info* info) {
    return guarded(h, [&] { do_kkt_step(h, "asm_kkt_step_multi", true, {x, lambda, row_state, bound_state}, nrhs, KktRhs::given(RU, RW), RADIUS, par, {DX, DLAM, DZ}, info); });
}

int asm_test_kkt_multi_rounds(const asm_handle* h, int64_t* rounds, int32_t* last_active) {
    if (!h || !rounds || !last_active) return ASM_ERR_ARG;
    *rounds = h->ev ? h->ev->kkm.rounds : 0;
    *last_active = h->ev ? h->ev->kkm.last_active : 0;
    return ASM_OK;
}

int asm_eval_hessian_structure(const asm_handle* ch, int64_t* nnz, int64_t* rows, int64_t* cols) {
    asm_handle* h = const_cast<asm_handle*>(ch);          // the pattern is made when it is first asked for
    return guarded(h, [&] { do_hessian_structure(h, nnz, rows, cols); });
}

int asm_eval_hessian_lagrangian(asm_handle* h, const double* x, double obj_factor, const double* lambda, double* values) {
    return guarded(h, [&] { do_hessian_lagrangian(h, x, obj_factor, lambda, values); });
}

int asm_eval_hessian_product(asm_handle* h, const double* x, double obj_factor, const double* lambda, const double* v, double* out) {
    return guarded(h, [&] { do_hessian_product(h, x, obj_factor, lambda, v, out); });
}

// --------------------------------------------------------------------------------- per-iteration reductions on the device (row f1)
// out[4] = { norm_violations(Inf), norm_violations(1), KT_residuals, norm_complementarity(Inf) }  (common.jl:35-98) from the
// evaluation results of the last asm_eval_functions and the Jacobian assembled from its dE (assembled once, shared with the LP)
static void do_slp_norms(asm_handle* h, const double* lambda, const double* mult_x_U, const double* mult_x_L, double* out4) {
    if (!h->ev || !h->sk->inputs_ready) throw std::logic_error("asm_slp_norms: asm_eval_functions first");
    if (!mult_x_U || !mult_x_L || !out4 || (h->sk->m > 0 && !lambda)) throw std::invalid_argument("asm_slp_norms: null pointer");
    HIPCHK(hipSetDevice(h->device));
    const int64_t n = h->sk->n, m = h->sk->m;
    Dev d(h);
    d.assemble();
    const EvLayout& L = h->ev->L;
    double *lam = L.lam(), *jtl = L.jtl(), *rown = L.rown(), *outd = L.out();
    double* st = h->ev->h_stage;    // the image of the block from lam on
    if (m) std::memcpy(st, lambda, m * sizeof(double));
    std::memcpy(st + (L.mU() - lam), mult_x_U, n * sizeof(double));
    std::memcpy(st + (L.mL() - lam), mult_x_L, n * sizeof(double));
    HIPCHK(asmb::copy_async(lam, st, (L.nu() - lam) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    // J' lambda over the first m rows: lambda padded with zeros on the extra range rows
    HIPCHK(asmb::fill_async(h->sk->d_vecM, 0, h->sk->Mp * sizeof(double), h->stream));
    if (m) HIPCHK(asmb::copy_async(h->sk->d_vecM, lam, m * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    d.launch_gemv_t(h->sk->d_J, h->sk->d_vecM, jtl);
    d.launch_row_norms(rown, true);
    asmb::launch(k_slp_norms, dim3(1), dim3(1024), h->stream, ev_vecs(*h->ev, true), outd);
    HIPCHK(asmb::copy_async(st, outd, RN_COUNT * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(asmb::sync(h->stream));
    for (int k = 0; k < RN_COUNT; ++k) out4[k] = st[k];
    d.resolve_timing();
}

int asm_slp_norms(asm_handle* h, const double* lambda, const double* mult_x_U, const double* mult_x_L, double* out4) {
    return guarded(h, [&] { do_slp_norms(h, lambda, mult_x_U, mult_x_L, out4); });
}

// compute_phi(x, alpha, p) (slp.jl:79-115; mode 0) and compute_derivative (slp.jl:122-147; mode 1) with the trial evaluation on the
// device.  p_slack: 2 entries per row as asm_sublp_solve returns them.
int asm_slp_merit(asm_handle* h, int mode, double alpha, const double* p, const double* nu, const double* p_slack, int feasibility, double prim_infeas,
                  double* out) {
    return guarded(h, [&] {
        if (!h->ev || !h->sk->inputs_ready) throw std::logic_error("asm_slp_merit: asm_eval_functions first");
        if (!p || !out || (h->sk->m > 0 && (!nu || !p_slack)) || mode < 0 || mode > 1) throw std::invalid_argument("asm_slp_merit: bad argument");
        HIPCHK(hipSetDevice(h->device));
        const EvalState& e = ev_stage_step(h, nu, p_slack, p);
        const EvLayout& L = e.L;
        const double *Et = e.d_E, *ft = e.d_f;
        if (mode == 0 && alpha != 0.0) {
            asmb::launch(k_axpy_out, asmb::blocks(h->sk->n), dim3(256), h->stream, e.d_x, alpha, L.p(), e.d_xt, h->sk->n);
            ev_launch(h, e.d_xt, e.d_Et, e.d_f + 1, false);
            Et = e.d_Et; ft = e.d_f + 1;
        }
        asmb::launch(k_slp_merit, dim3(1), dim3(1024), h->stream, ev_vecs(e), Et, L.nu(), L.ps(), L.p(), alpha, feasibility, prim_infeas, ft, mode, L.out(), TrialAlphas(),
                     (int64_t)0);
        HIPCHK(asmb::copy_async(e.h_stage, L.out(), sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(asmb::sync(h->stream));
        *out = e.h_stage[0];
    });
}

// compute_alpha's trial loop (slp_line_search.jl:222-244) on the step ev_stage_step uploaded: alpha = 1, tau, tau^2, ... until
//   phi(alpha) <= phi0 + eta alpha D      (accepted: *ok = 1)      or      alpha < min_alpha with the test still failing (*ok = 0).
// The trials are pure function evaluations, so they are launched eight at a time without waiting for the verdict of the earlier ones (one
// read-back per eight): same alpha, same merit values as asm_slp_merit per trial.  phi0_D_on_device: k_slp_merit launches of the caller's
// put phi0 and D into out[TRIALS], out[TRIALS + 1]; they come back with the first eight merit values and leave through phi0, D.
static void slp_trials(asm_handle* h, int feasibility, double prim_infeas, bool phi0_D_on_device, double& phi0, double& D, double eta, double tau, double min_alpha,
                       double* alpha_out, double* phi_out, int* trials_out, int* ok_out) {
    const EvalState& e = *h->ev;
    const EvLayout& L = e.L;
    const int64_t n = h->sk->n, m = h->sk->m;
    const SlpVecs V = ev_vecs(e);
    constexpr int CH = (int)EvLayout::TRIALS;
    static_assert(sizeof(TrialAlphas) == CH * sizeof(double), "one alpha per trial of a round");
    double* st = e.h_stage;
    double alpha = 1.0, a[CH];
    int trials = 0;
    *ok_out = -1;
    for (int round = 0; *ok_out < 0; ++round) {
        asmb::barrier(920);
        // eight trial points per set of launches (trial index in the grid): x + alpha_t p, the function values there, the merit values
        TrialAlphas al;
        for (int t = 0; t < CH; ++t) { a[t] = al.a[t] = alpha; alpha *= tau; }
        const int64_t ldx = round_up(n, 32), ldE = round_up(std::max<int64_t>(m, 1), 32);
        asmb::launch(k_axpy_trials, dim3((unsigned)((n + 255) / 256), CH), dim3(256), h->stream, e.d_x, al, L.p(), e.d_xt, n, ldx);
        ev_launch(h, e.d_xt, e.d_Et, e.d_f + 1, false, CH, ldx, ldE);
        asmb::launch(k_slp_merit, dim3(CH), dim3(1024), h->stream, V, e.d_Et, L.nu(), L.ps(), L.p(), 0.0, feasibility, prim_infeas, e.d_f + 1, 0, L.out(), al, ldE);
        const bool first = phi0_D_on_device && round == 0;
        HIPCHK(asmb::copy_async(st, L.out(), (CH + (first ? 2 : 0)) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(asmb::sync(h->stream));
        if (first) { phi0 = st[CH]; D = st[CH + 1]; }
        for (int t = 0; t < CH && *ok_out < 0; ++t) {
            trials += 1;
            *ok_out = !(st[t] > phi0 + eta * a[t] * D) ? 1 : a[t] < min_alpha ? 0 : -1;
            if (*ok_out >= 0) { *alpha_out = a[t]; if (phi_out) *phi_out = st[t]; }
        }
    }
    if (trials_out) *trials_out = trials;
}

// compute_alpha with phi0 and D given; nu, the slacks and p are uploaded once
int asm_slp_line_search(asm_handle* h, const double* p, const double* nu, const double* p_slack, int feasibility, double prim_infeas, double phi0,
                        double D, double eta, double tau, double min_alpha, double* alpha_out, double* phi_out, int* trials_out, int* ok_out) {
    return guarded(h, [&] {
        if (!h->ev || !h->sk->inputs_ready) throw std::logic_error("asm_slp_line_search: asm_eval_functions first");
        if (!p || !alpha_out || !ok_out || (h->sk->m > 0 && (!nu || !p_slack)) || !(tau > 0.0 && tau < 1.0))
            throw std::invalid_argument("asm_slp_line_search: bad argument");
        HIPCHK(hipSetDevice(h->device));
        ev_stage_step(h, nu, p_slack, p);
        slp_trials(h, feasibility, prim_infeas, false, phi0, D, eta, tau, min_alpha, alpha_out, phi_out, trials_out, ok_out);
    });
}

// The native SLP driver's step: compute_phi(x, 0, p), compute_derivative and compute_alpha in one upload and - when one of the first eight
// trial steps is accepted, i.e. nearly always - one read-back (asm_slp_merit twice + asm_slp_line_search: three uploads of nu | slacks | p and
// three read-backs).  The trial points do not depend on phi0 and D, only the acceptance test does: same launches per quantity, same values.
static void slp_merit_and_search(asm_handle* h, const double* p, const double* nu, const double* p_slack, int feasibility, double prim_infeas, double eta, double tau,
                                 double min_alpha, double* phi0_out, double* D_out, double* alpha_out, double* phi_out, int* trials_out, int* ok_out) {
    const EvalState& e = ev_stage_step(h, nu, p_slack, p);
    const EvLayout& L = e.L;
    for (int mode = 0; mode < 2; ++mode)
        asmb::launch(k_slp_merit, dim3(1), dim3(1024), h->stream, ev_vecs(e), e.d_E, L.nu(), L.ps(), L.p(), 0.0, feasibility, prim_infeas, e.d_f, mode,
                     L.out() + EvLayout::TRIALS + mode, TrialAlphas(), (int64_t)0);
    slp_trials(h, feasibility, prim_infeas, true, *phi0_out, *D_out, eta, tau, min_alpha, alpha_out, phi_out, trials_out, ok_out);
}

// step_quality's merit values (slp_trust_region.jl:213-216): out3 = { compute_derivative, compute_phi(x, 0, p), compute_phi(x, 1, p) } with one
// upload of nu | slacks | p, the trial point x + p evaluated on the device and one read-back (three asm_slp_merit calls: three uploads, three read-backs).  The
// same launches per quantity as asm_slp_merit makes (k_axpy_out + ev_launch at alpha = 1, the merit body of k_slp_merit): same values.
static void slp_tr_step_quality(asm_handle* h, const double* p, const double* nu, const double* p_slack, int feasibility, double prim_infeas, double* out3) {
    const EvalState& e = ev_stage_step(h, nu, p_slack, p);
    const EvLayout& L = e.L;
    asmb::launch(k_axpy_out, asmb::blocks(h->sk->n), dim3(256), h->stream, e.d_x, 1.0, L.p(), e.d_xt, h->sk->n);
    ev_launch(h, e.d_xt, e.d_Et, e.d_f + 1, false);
    asmb::launch(k_slp_tr_quality, dim3(3), dim3(1024), h->stream, ev_vecs(e), e.d_Et, L.nu(), L.ps(), L.p(), feasibility, prim_infeas, e.d_f, e.d_f + 1, L.out());
    HIPCHK(asmb::copy_async(e.h_stage, L.out(), 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(asmb::sync(h->stream));
    for (int k = 0; k < 3; ++k) out3[k] = e.h_stage[k];
}

int asm_slp_step_quality(asm_handle* h, const double* p, const double* nu, const double* p_slack, int feasibility, double prim_infeas, double* out3) {
    return guarded(h, [&] {
        if (!h->ev || !h->sk->inputs_ready) throw std::logic_error("asm_slp_step_quality: asm_eval_functions first");
        if (!p || !out3 || (h->sk->m > 0 && (!nu || !p_slack))) throw std::invalid_argument("asm_slp_step_quality: null pointer");
        HIPCHK(hipSetDevice(h->device));
        slp_tr_step_quality(h, p, nu, p_slack, feasibility, prim_infeas, out3);
    });
}

// ---- the SLP-EQP trial step (include/asm_hip.h, "SLP-EQP"): steps B to F of the method on the handle, after asm_eval_functions at x
namespace {
void eq_prepare(asm_handle* h) {
    kk_prepare(h);
    KktBufs& K = h->ev->kk;
    if (K.eq_i) return;
    HIPCHK(hipSetDevice(h->device));
    const int64_t n = h->sk->n, m = h->sk->m, ni = h->sk->M + 2 * n + 3 * m + 4, nd = m + 2 * n + EQP_SCAL;
    h->ev->mem.zeroed(K.eq_i, ni, h->stream);
    h->ev->mem.zeroed(K.eq_d, nd, h->stream);
    h->ev->mem.alloc(K.eq_h, (ni + 1) / 2 + nd + n + 8, BufPool::PINNED);
    HIPCHK(asmb::sync(h->stream));
}
}  // namespace
static void do_eqp_trial(asm_handle* h, const double* x, const double* lambda, const int32_t* lp_row_state, const int32_t* lp_bound_state, double radius, const double* nu,
                         double tol_active, const asm_kkt_step_params* par, double* d, double* lam_new, double* mult_x_U, double* mult_x_L, int32_t* row_state,
                         int32_t* bound_state, asm_eqp_info* info) {
    const char* const who = "asm_eqp_trial";
    const std::string me(who);
    (void)kkt_hess_lm(h, who);
    const int64_t n = h->sk->n, m = h->sk->m, M = h->sk->M;
    if (!x || !lp_bound_state || !d || !mult_x_U || !mult_x_L || !bound_state || !info || (m > 0 && (!lambda || !lp_row_state || !nu || !lam_new || !row_state)))
        throw std::invalid_argument(me + ": null pointer");
    if (!(tol_active >= 0.0)) throw std::invalid_argument(me + ": tol_active is not >= 0");
    if (!(radius > 0.0)) throw std::invalid_argument(me + ": a radius is not > 0");
    if (par && !(par->normal_share > 0.0 && par->normal_share <= 1.0)) throw std::invalid_argument(me + ": normal_share outside (0, 1]");
    if (par && (par->max_iter < 0 || !(par->rtol >= 0.0))) throw std::invalid_argument(me + ": max_iter < 0 or rtol not >= 0");
    for (int64_t j = 0; j < n; ++j)
        if (lp_bound_state[j] < -1 || lp_bound_state[j] > 1) throw std::invalid_argument(me + ": bound_state holds a value outside {-1, 0, +1}");
    for (int64_t i = 0; i < (m > 0 ? M : 0); ++i)
        if (lp_row_state[i] != 0 && lp_row_state[i] != 1) throw std::invalid_argument(me + ": row_state holds a value outside {0, 1}");
    // (inputs uploaded by asm_sublp_upload leave the evaluator's x, E and gradient in HBM where an earlier evaluation put them)
    if (!h->sk->inputs_ready || !h->sk->inputs_from_eval) throw std::logic_error(me + ": asm_eval_functions first");
    if (std::memcmp(x, h->sk->x_k.data(), n * sizeof(double)) != 0) throw std::logic_error(me + ": x is not the point of the last asm_eval_functions");
    eq_prepare(h);
    HIPCHK(hipSetDevice(h->device));
    std::memset(info, 0, sizeof(*info));
    for (int64_t j = 0; j < n; ++j) d[j] = mult_x_U[j] = mult_x_L[j] = 0.0;
    for (int64_t i = 0; i < m; ++i) lam_new[i] = 0.0;
    const KktBufs& K = h->ev->kk;
    const hipStream_t s = h->stream;
    const KktRed R{K.part, K.cnt, K.scal};
    const int64_t n_in = M + n + m, n_out = m + n + 4;      // (the side a working row sits at stays on the device: rw carries what the host needs of it)
    int *i_lp_rows = K.eq_i, *i_lp_bnd = i_lp_rows + M, *i_twin = i_lp_bnd + n, *i_rows = i_twin + m, *i_bnd = i_rows + m, *i_cnt = i_bnd + n, *i_side = i_cnt + 4;
    double *d_rw = K.eq_d, *d_dx = d_rw + m, *d_d = d_dx + n, *d_scal = d_d + n;
    // B. the face: the LP's states and the twin map go up; the working set with the two counts, rw and the gradient come back (three copies, one wait)
    int* hi = reinterpret_cast<int*>(K.eq_h);
    double* hd = K.eq_h + (n_in + n_out + 1) / 2;
    if (m > 0) std::memcpy(hi, lp_row_state, M * sizeof(int));
    std::memcpy(hi + M, lp_bound_state, n * sizeof(int));
    for (int64_t i = 0; i < m; ++i) hi[M + n + i] = -1;
    for (size_t a = 0; a < h->sk->adj.size(); ++a) hi[M + n + h->sk->adj[a]] = (int)a;
    HIPCHK(asmb::copy_async(i_lp_rows, hi, n_in * sizeof(int), hipMemcpyHostToDevice, s));
    const SlpVecs V = ev_vecs(*h->ev);
    const EqpFace P{V.E, V.g_L, V.g_U, V.x, V.x_L, V.x_U, i_lp_rows, i_lp_bnd, i_twin, n, m, tol_active};
    const KktSites at(s, h->sk->ldn, K.ldT);
    at.eqp_face(P, R, i_rows, i_bnd, i_side, d_rw, i_cnt);
    HIPCHK(asmb::copy_async(hi + n_in, i_rows, n_out * sizeof(int), hipMemcpyDeviceToHost, s));
    if (m > 0) HIPCHK(asmb::copy_async(hd, d_rw, m * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(asmb::copy_async(hd + m, h->ev->d_df, n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(asmb::sync(s));
    const int* o_rows = hi + n_in;
    const int *o_bnd = o_rows + m, *o_cnt = o_bnd + n;
    std::vector<int32_t> rs((size_t)std::max<int64_t>(m, 1), 0);
    for (int64_t i = 0; i < m; ++i) rs[i] = row_state[i] = o_rows[i];
    for (int64_t j = 0; j < n; ++j) bound_state[j] = o_bnd[j];
    info->n_rows = o_cnt[EQP_NW];
    info->n_free = o_cnt[EQP_NF];
    // C. more working rows than free variables
    if (info->n_rows > info->n_free) { info->skipped = 1; return; }
    // D. the trust-region step (asm_kkt_step): ru = grad f, rw_W = E_W - bound_W
    vec ru(hd + m, hd + m + n), rw(hd, hd + m), dx((size_t)n), dlam((size_t)std::max<int64_t>(m, 1)), dz((size_t)n);
    rw.resize((size_t)std::max<int64_t>(m, 1), 0.0);
    asm_kkt_step_info st;
    do_kkt_step(h, who, false, {x, lambda, rs.data(), bound_state}, 1, KktRhs::given(ru.data(), rw.data()), &radius, par, {dx.data(), dlam.data(), dz.data()}, &st);
    info->status = st.status; info->cg_iters = st.cg_iters; info->n_free = st.n_free; info->n_rows = st.n_rows; info->dropped_pivots = st.dropped_pivots;
    info->boundary = st.boundary; info->res_stat = st.res_stat; info->res_feas = st.res_feas; info->theta = st.theta; info->norm_normal = st.norm_normal;
    info->norm_step = st.norm_step; info->model = st.model;
    if (st.status == 3) { info->skipped = 2; return; }
    // E. the fraction to the box, d = t dx and its norms
    double* hx = K.eq_h;
    std::memcpy(hx, dx.data(), n * sizeof(double));
    HIPCHK(asmb::copy_async(d_dx, hx, n * sizeof(double), hipMemcpyHostToDevice, s));
    at.eqp_trial(d_dx, V.x, V.x_L, V.x_U, n, R, d_d, d_scal);
    HIPCHK(asmb::copy_async(hx + n, d_d, (n + EQP_SCAL) * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(asmb::sync(s));
    const double* sc = hx + 2 * n;
    info->t = sc[EQP_T]; info->norm_d = sc[EQP_NORM2]; info->norm_d_inf = sc[EQP_NORMINF];
    if (sc[EQP_NONZERO] == 0.0) { info->skipped = 3; return; }
    std::memcpy(d, hx + n, n * sizeof(double));
    // F. the merit function at x and at x + d (the launch set of asm_slp_step_quality outside restoration: the slacks are not read)
    vec ps((size_t)(2 * std::max<int64_t>(m, 1)), 0.0);
    double q[3];
    slp_tr_step_quality(h, d, nu, ps.data(), 0, 0.0, q);
    info->phi0 = q[1]; info->phi1 = q[2];
    for (int64_t i = 0; i < m; ++i) lam_new[i] = dlam[i];
    for (int64_t j = 0; j < n; ++j) {
        mult_x_U[j] = bound_state[j] == 1 ? dz[j] : 0.0;
        mult_x_L[j] = bound_state[j] == -1 ? dz[j] : 0.0;
    }
}

int asm_eqp_trial(asm_handle* h, const double* x, const double* lambda, const int32_t* lp_row_state, const int32_t* lp_bound_state, double radius, const double* nu,
                  double tol_active, const asm_kkt_step_params* par, double* d, double* lam_new, double* mult_x_U, double* mult_x_L, int32_t* row_state,
                  int32_t* bound_state, asm_eqp_info* info) {
    return guarded(h, [&] {
        do_eqp_trial(h, x, lambda, lp_row_state, lp_bound_state, radius, nu, tol_active, par, d, lam_new, mult_x_U, mult_x_L, row_state, bound_state, info);
    });
}

int asm_hessian_set_type(asm_handle* h, int32_t type, int32_t memory) {
    return guarded(h, [&] { do_hessian_set_type(h, type, memory); });
}
int asm_lm_reset(asm_handle* h) {
    return guarded(h, [&] {
        HIPCHK(hipSetDevice(h->device));
        lm_clear(h);
    });
}
int asm_lm_push_pair(asm_handle* h, const double* s, const double* y) {
    return guarded(h, [&] { do_lm_push_pair(h, s, y); });
}
int asm_lm_begin(asm_handle* h, const double* lambda) {
    return guarded(h, [&] { do_lm_begin(h, lambda); });
}
int asm_lm_end(asm_handle* h, const double* lambda) {
    return guarded(h, [&] { do_lm_end(h, lambda); });
}
int asm_lm_product(asm_handle* h, const double* V, int32_t nrhs, double* OUT) {
    return guarded(h, [&] { do_lm_product(h, V, nrhs, OUT); });
}
int asm_lm_info(asm_handle* h, struct asm_lm_info* out) {
    return guarded(h, [&] { do_lm_info(h, out); });
}

// --------------------------------------------------------------------------------- kernel test hooks
static void test_alloc(asm_handle* h, int64_t M, int64_t K) {
    // minimal "problem" so that the generic buffers exist: dense pattern M x K
    std::vector<int64_t> jr(1, 1), jc(1, 1);
    vec lo(M, 0.0), hi(M, 0.0), vl(K, -1.0), vu(K, 1.0);
    do_setup(h, K, M, 1, jr.data(), jc.data(), lo.data(), hi.data(), vl.data(), vu.data());
    h->sk->sp_ok = false;     // the hooks write arbitrary matrices into the buffers
}

// The kernel hooks that also run on the fibers of a scenario batch (asm_batch_test_run) have their body in an internal function test_*(h, record):
// the record's fields are the hook's parameters after h, the value is the hook's return code.  The hook itself only fills the record.
static int test_syrk(asm_handle* h, const asm_test_syrk_args& a_);
int asm_test_syrk(asm_handle* h, const double* A, int64_t M, int64_t K, const int32_t* idx, int64_t Ms, const double* theta,
                  const double* diag, double* S_out, int tile) {
    return test_syrk(h, asm_test_syrk_args{A, M, K, idx, Ms, theta, diag, S_out, tile});
}
static int test_syrk(asm_handle* h, const asm_test_syrk_args& a_) {
    const double *A = a_.A, *theta = a_.theta, *diag = a_.diag;
    const int64_t M = a_.M, K = a_.K, Ms = a_.Ms;
    const int32_t* idx = a_.idx;
    double* S_out = a_.S_out;
    const int tile = a_.tile;
    return guarded(h, [&] {
        test_alloc(h, M, K);
        Dev d(h);
        for (int64_t i = 0; i < M; ++i)
            HIPCHK(asmb::copy(h->sk->d_Ah + i * h->sk->ldn, A + i * K, K * sizeof(double), hipMemcpyHostToDevice));
        d.h2d(h->sk->d_theta, theta, K, h->sk->ldn);
        if (diag) d.h2d(h->sk->d_diag, diag, Ms, Ms);
        if (idx) HIPCHK(asmb::copy(h->sk->d_idx, idx, Ms * sizeof(int), hipMemcpyHostToDevice));
        const FacBuf& F = h->sk->main_fac;
        HIPCHK(asmb::fill(F.S, 0, F.ld * F.ld * sizeof(double)));
        d.launch_syrk(h->stream, tile > 0 ? tile : Dev::pick_tile(Ms), h->sk->d_Ah, h->sk->ldn, idx ? h->sk->d_idx : nullptr, 0, (int)Ms, (int)h->sk->ldn, h->sk->d_theta,
                      diag ? h->sk->d_diag : nullptr, F.S, F.ld, 0, 0);
        HIPCHK(asmb::sync(h->stream));
        for (int64_t i = 0; i < Ms; ++i)
            HIPCHK(asmb::copy(S_out + i * Ms, F.S + i * F.ld, Ms * sizeof(double), hipMemcpyDeviceToHost));
    });
}

// The chunk-skipping build on buffers of the caller's: S (ldS x ldS, pre-filled by the caller) gets A[rows] diag(theta) A[rows]' + diag in the lower
// triangle of its first Ms rows, launched as Dev::schur_syrk launches a PerCall build - k_tile_nzflags for the row list, then k_syrk with the
// chunk flags (use_flags = 0: the same launch without them, the dense sweep).  Returns the flags (nt x K / 32 bytes) and their executed share.
int asm_test_build_flagged(asm_handle* h, const double* A, int64_t M, int64_t K, const int32_t* idx, int64_t Ms, const double* theta, const double* diag, int tile,
                           int use_flags, double* S_inout, int64_t ldS, unsigned char* flags_out, double* fraction_out) {
    return guarded(h, [&] {
        if (!A || !theta || !S_inout || !flags_out || !fraction_out || M <= 0 || Ms <= 0 || K <= 0 || K % ASM_KC != 0 || K / ASM_KC > ASM_MAXCHUNKS || ldS < Ms ||
            (!idx && Ms > M) || !(tile == 0 || tile == 1 || tile == 2 || tile == 4))
            throw std::invalid_argument("asm_test_build_flagged: bad argument");
        if (idx) for (int64_t a = 0; a < Ms; ++a) if (idx[a] < 0 || idx[a] >= M) throw std::invalid_argument("asm_test_build_flagged: row index out of range");
        HIPCHK(hipSetDevice(h->device));
        Dev d(h);
        const int T = tile > 0 ? tile : Dev::pick_tile(Ms), TS = 32 * T, nt = (int)((Ms + TS - 1) / TS), nch = (int)(K / ASM_KC);
        double *dA = nullptr, *dth = nullptr, *ddg = nullptr, *dS = nullptr;
        int* didx = nullptr;
        unsigned char* dnz = nullptr;
        BufPool tmp;
        tmp.upload(dA, A, M * K); tmp.upload(dth, theta, K); tmp.upload(dS, S_inout, ldS * ldS);
        if (diag) tmp.upload(ddg, diag, Ms);
        if (idx) tmp.upload(didx, idx, Ms);
        tmp.zeroed(dnz, (int64_t)nt * nch);
        d.launch_tile_flags(dA, K, Ms, T, nch, dnz, nch, didx);
        const double frac = d.executed_fraction_now(dnz, nt, nch);
        d.launch_syrk(h->stream, T, dA, K, didx, 0, (int)Ms, (int)K, dth, ddg, dS, ldS, 0, 0, -1, use_flags ? dnz : nullptr, nch, frac);
        HIPCHK(asmb::sync(h->stream));
        HIPCHK(asmb::copy(S_inout, dS, ldS * ldS * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(asmb::copy(flags_out, dnz, (size_t)nt * nch, hipMemcpyDeviceToHost));
        *fraction_out = frac;
        d.resolve_timing();
    });
}

// The k x k matrix of a null-space iteration on buffers of the caller's, by the statements of the solver (Dev::ns_newton_matrix: split-K build
// + reduction for nsplit > 1, else the plain build, its copy and k_diag_prepare).  G is k x K; every output has the pitch ld = k rounded up to
// 32 and is pre-filled by the caller: parts (nsplit x ld x ld; untouched for nsplit = 1), S, N0 (ld x ld each), diag0 (ld).
static int test_build_split(asm_handle* h, const asm_test_build_split_args& a_);
int asm_test_build_split(asm_handle* h, const double* G, int64_t k, int64_t K, const double* theta, int nsplit, double rel, double absv, double* parts_inout,
                         double* S_inout, double* N0_inout, double* diag0_inout) {
    return test_build_split(h, asm_test_build_split_args{G, k, K, theta, nsplit, rel, absv, parts_inout, S_inout, N0_inout, diag0_inout});
}
static int test_build_split(asm_handle* h, const asm_test_build_split_args& a_) {
    const double *G = a_.G, *theta = a_.theta;
    const int64_t k = a_.k, K = a_.K;
    const int nsplit = a_.nsplit;
    const double rel = a_.rel, absv = a_.absv;
    double *parts_inout = a_.parts_inout, *S_inout = a_.S_inout, *N0_inout = a_.N0_inout, *diag0_inout = a_.diag0_inout;
    return guarded(h, [&] {
        if (!G || !theta || !parts_inout || !S_inout || !N0_inout || !diag0_inout || k <= 0 || K <= 0 || K % ASM_KC != 0 || nsplit < 1 || nsplit > NS_MAX_SPLIT)
            throw std::invalid_argument("asm_test_build_split: bad argument");
        HIPCHK(hipSetDevice(h->device));
        Dev d(h);
        FacBuf f;
        f.ld = round_up(k, 32);
        const int64_t sq = f.ld * f.ld;
        double *dG = nullptr, *dth = nullptr, *dP = nullptr, *dN0 = nullptr, *dd0 = nullptr;
        BufPool tmp;
        tmp.upload(dG, G, k * K); tmp.upload(dth, theta, K); tmp.upload(dP, parts_inout, nsplit * sq);
        tmp.upload(f.S, S_inout, sq); tmp.upload(dN0, N0_inout, sq); tmp.upload(dd0, diag0_inout, f.ld);
        d.ns_newton_matrix(dG, K, dth, (int)k, nsplit, dP, f, dN0, dd0, rel, absv);
        HIPCHK(asmb::sync(h->stream));
        HIPCHK(asmb::copy(parts_inout, dP, nsplit * sq * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(asmb::copy(S_inout, f.S, sq * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(asmb::copy(N0_inout, dN0, sq * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(asmb::copy(diag0_inout, dd0, f.ld * sizeof(double), hipMemcpyDeviceToHost));
        d.resolve_timing();
    });
}

// The builds of a set-up handle through the solver's dispatch.  The Jacobian is assembled from dE and scaled by rows only (unit column scale),
// the chunk flags made as at the start of an LP; then build `which`: 0 Dev::schur_syrk with Pattern flags over all rows; 1 the same on the
// transposed copy (column form, theta = M weights, diag = n); 2 Dev::schur_rows of the row list idx (diag by place); 3
// Dev::schur_banded_cols_dev (columns in their banded order, diag by place); 4 Dev::ns_build_S0 (theta = the n column weights); < 0 nothing.
// The matrix is built in the factor buffer the solver uses, loaded from S_inout before (ld x ld with ld = info[4], or info[7] for which = 4)
// and returned in it.  info: M, n, row_band, col_band, main pitch, nE, S0 band, S0 pitch, column form possible, row flags valid, column
// flags valid, sparse pattern.  Ah_out: the operand as it stands on the device (M x n); orders (position -> index; -1 without one).
int asm_test_build_dispatch(asm_handle* h, const double* dE, int which, const int32_t* idx, int64_t Ms, const double* theta, const double* diag, double* S_inout,
                            double* Ah_out, int64_t* info, int32_t* row_order, int32_t* col_order, int32_t* e_order) {
    return guarded(h, [&] {
        Skeleton& K = sk_of(h, "asm_test_build_dispatch: asm_sublp_setup first");
        if (!info || (K.nnz > 0 && !dE) || which > 4) throw std::invalid_argument("asm_test_build_dispatch: bad argument");
        HIPCHK(hipSetDevice(h->device));
        const int64_t M = K.M, n = K.n;
        Dev d(h);
        HIPCHK(asmb::copy(K.d_dE, dE, K.nnz * sizeof(double), hipMemcpyHostToDevice));
        K.J_valid = false;
        d.assemble();
        vec c(n, 1.0), rho(M);
        d.scale(c.data(), rho.data());
        d.tile_flags();
        NsForm* const ns = K.nsf.get();
        const int64_t out[12] = {M, n, K.row_band, K.col_band, K.main_fac.ld, ns ? ns->L.nE : 0, ns ? ns->f0.band : 0, ns ? ns->f0.ld : 0, K.col_capable ? 1 : 0,
                                 K.nz_valid ? 1 : 0, 0, K.sp_ok ? 1 : 0};
        for (int k = 0; k < 12; ++k) info[k] = out[k];
        if (Ah_out) for (int64_t i = 0; i < M; ++i) HIPCHK(asmb::copy(Ah_out + i * n, K.d_Ah + i * K.ldn, n * sizeof(double), hipMemcpyDeviceToHost));
        if (row_order) for (int64_t q = 0; q < M; ++q) row_order[q] = K.row_band > 0 ? K.row_perm_h[q] : -1;
        if (col_order) {
            if (K.col_band > 0) HIPCHK(asmb::copy(col_order, K.d_colperm, n * sizeof(int), hipMemcpyDeviceToHost));
            else for (int64_t q = 0; q < n; ++q) col_order[q] = -1;
        }
        if (e_order && ns) std::copy(ns->eidx_h.begin(), ns->eidx_h.end(), e_order);
        if (which < 0) return;
        const FacBuf& f = which == 4 && ns ? ns->f0 : K.main_fac;       // (which = 4 without the form is refused below)
        const int64_t nth = (which == 1 || which == 3) ? M : n, ndg = which == 0 ? M : ((which == 1 || which == 3) ? n : Ms);
        if (!theta || !S_inout || (which == 2 && (!idx || Ms <= 0 || Ms > M)) || ((which == 1 || which == 3) && (!K.col_capable || !diag)) ||
            (which == 3 && K.col_band <= 0) || (which == 4 && !ns) || ((which == 1 || which == 3) && n > f.ld) || (which == 0 && M == 0))
            throw std::invalid_argument("asm_test_build_dispatch: build not available on this handle");
        double *dth = nullptr, *ddg = nullptr;
        BufPool tmp;
        tmp.zeroed(dth, std::max(K.ldn, K.Mp) + 64);
        HIPCHK(asmb::copy(dth, theta, nth * sizeof(double), hipMemcpyHostToDevice));
        if (diag && which != 4) tmp.upload(ddg, diag, ndg);
        HIPCHK(asmb::copy(f.S, S_inout, f.ld * f.ld * sizeof(double), hipMemcpyHostToDevice));
        switch (which) {
        case 0: d.schur_syrk(false, nullptr, (int)M, dth, ddg, f.S, f.ld, Dev::NzFlags::Pattern); break;
        case 1: d.schur_syrk(true, nullptr, (int)n, dth, ddg, f.S, f.ld, Dev::NzFlags::Pattern); break;
        case 2: {
            for (int64_t a = 0; a < Ms; ++a) if (idx[a] < 0 || idx[a] >= M) throw std::invalid_argument("asm_test_build_dispatch: row index out of range");
            HIPCHK(asmb::copy(K.d_idx, idx, Ms * sizeof(int), hipMemcpyHostToDevice));
            if (K.row_band > 0) {      // place of every row in the list (-1: not in it), as the reduced row form makes it
                std::vector<int> cp(M, -1);
                for (int64_t a = 0; a < Ms; ++a) cp[idx[a]] = (int)a;
                HIPCHK(asmb::copy(K.d_cpos, cp.data(), M * sizeof(int), hipMemcpyHostToDevice));
            }
            d.schur_rows(K.d_idx, K.d_cpos, (int)Ms, dth, ddg);
            break;
        }
        case 3: d.schur_banded_cols_dev(dth, ddg); break;
        default:
            HIPCHK(asmb::copy(ns->Fm, dth, K.ldn * sizeof(double), hipMemcpyDeviceToDevice));
            d.ns_build_S0();
        }
        HIPCHK(asmb::sync(h->stream));
        info[10] = K.nzT_valid ? 1 : 0;
        HIPCHK(asmb::copy(S_inout, f.S, f.ld * f.ld * sizeof(double), hipMemcpyDeviceToHost));
        d.resolve_timing();
    });
}

// The interior-point stage kernels (asm_ipm_kernels.hip.h), one launch per stage, through the launch-site members of Solver and on an arena
// laid out by Solver::ipm_bind with the pitches of IpmLayout - see include/asm_hip.h.  Every offset and index a stage reads is checked here
// against the buffers before anything is launched.
static int test_ipm_stages(asm_handle* h, const asm_test_ipm_stages_args& a_);
int asm_test_ipm_stages(asm_handle* h, int64_t n, int64_t M, int64_t ns, int64_t ncomp, double scale_q, int64_t* layout_out, double* dbl_inout, int64_t ndbl,
                        const int32_t* ints, int64_t nint, double* snap_inout, double* rpart_inout, uint32_t* rcnt_inout, double* hscal_inout, uint32_t* hseq_inout,
                        const asm_ipm_stage* stages, int64_t nstages, uint32_t* grid_out) {
    return test_ipm_stages(h, asm_test_ipm_stages_args{n, M, ns, ncomp, scale_q, layout_out, dbl_inout, ndbl, ints, nint, snap_inout, rpart_inout, rcnt_inout,
                                                       hscal_inout, hseq_inout, stages, nstages, grid_out});
}
static int test_ipm_stages(asm_handle* h, const asm_test_ipm_stages_args& a_) {
    const int64_t n = a_.n, M = a_.M, ns = a_.ns, ncomp = a_.ncomp, ndbl = a_.ndbl, nint = a_.nint, nstages = a_.nstages;
    const double scale_q = a_.scale_q;
    int64_t* layout_out = a_.layout_out;
    double *dbl_inout = a_.dbl_inout, *snap_inout = a_.snap_inout, *rpart_inout = a_.rpart_inout, *hscal_inout = a_.hscal_inout;
    const int32_t* ints = a_.ints;
    uint32_t *rcnt_inout = a_.rcnt_inout, *hseq_inout = a_.hseq_inout, *grid_out = a_.grid_out;
    const asm_ipm_stage* stages = a_.stages;
    return guarded(h, [&] {
        const int64_t LIM = (int64_t)1 << 24;
        if (!layout_out || n < 1 || M < 0 || ns < 0 || n > LIM || M > LIM || ns > LIM || ncomp < 1 || (ns > 0 && M == 0) || nstages < 0)
            throw std::invalid_argument("asm_test_ipm_stages: bad size");
        HIPCHK(hipSetDevice(h->device));
        const IpmLayout lay(n, M, ns);
        Solver S(h);
        S.lp.n = n; S.lp.M = M; S.lp.ns = ns; S.lp.scale_q = scale_q;
        Solver::IpmArena ar;
        ar.ln = lay.ldn; ar.lm = lay.Mp; ar.ls = lay.nsp;
        // the layout, from the pointers ipm_bind sets on a base address that is never dereferenced
        ar.base = reinterpret_cast<double*>((uintptr_t)1 << 30);
        S.ipm_bind(ar);
        auto off = [&](const double* v) { return (int64_t)(((uintptr_t)v - (uintptr_t)ar.base) / sizeof(double)); };
        {
            const double* vs[ASM_IPM_NVEC];
            S.ipm_vectors(vs);
            const int64_t head[8] = {lay.ldn, lay.Mp, lay.nsp, lay.arena_len(), lay.snap_len(), lay.int_len(), SC_COUNT, off(S.P.scal)};
            for (int k = 0; k < 8; ++k) layout_out[k] = head[k];
            for (int k = 0; k < ASM_IPM_NVEC; ++k) layout_out[8 + k] = off(vs[k]);
            if (layout_out[7] + SC_COUNT > lay.arena_len()) throw std::logic_error("asm_test_ipm_stages: the arena is shorter than its layout");
        }
        if (!dbl_inout) return;      // layout query
        if (!ints || !snap_inout || !rpart_inout || !rcnt_inout || !hscal_inout || !hseq_inout || (nstages > 0 && (!stages || !grid_out)) || ndbl < lay.arena_len() ||
            nint < lay.int_len() || ndbl > ((int64_t)1 << 31) || nint > ((int64_t)1 << 31))
            throw std::invalid_argument("asm_test_ipm_stages: bad buffer");
        for (int64_t i = 0; i < M; ++i) {
            const int rt = ints[i], k0 = ints[lay.Mp + i], k1 = ints[2 * lay.Mp + i];
            if (rt < -1 || rt > 1 || k0 < -1 || k0 >= ns || k1 < -1 || k1 >= ns) throw std::invalid_argument("asm_test_ipm_stages: row type or slack index out of range");
        }
        for (int64_t k = 0; k < ns; ++k)
            if (ints[3 * lay.Mp + k] < 0 || ints[3 * lay.Mp + k] >= M) throw std::invalid_argument("asm_test_ipm_stages: slack row out of range");
        auto dspan = [&](int64_t off, int64_t len) {
            if (off < 0 || len < 0 || off + len > ndbl) throw std::invalid_argument("asm_test_ipm_stages: vector outside the double block");
        };
        auto ilist = [&](int64_t off, int64_t len, int64_t bound) {      // an index list with entries in [0, bound)
            if (off < 0 || len < 0 || off + len > nint) throw std::invalid_argument("asm_test_ipm_stages: list outside the int block");
            for (int64_t a = 0; a < len; ++a)
                if (ints[off + a] < 0 || ints[off + a] >= bound) throw std::invalid_argument("asm_test_ipm_stages: index out of range");
        };
        for (int64_t q = 0; q < nstages; ++q) {
            const asm_ipm_stage& st = stages[q];
            if (st.D < 0 || st.D > 1 || st.B < 0 || st.B > 1) throw std::invalid_argument("asm_test_ipm_stages: direction selector");
            switch (st.kind) {
            case ASM_IPM_VEC_MUL: dspan(st.x[0], st.len[0]); dspan(st.x[1], st.len[0]); break;
            case ASM_IPM_SNAPSHOT: if (st.with_e) dspan(st.x[0], lay.ldn); break;
            case ASM_IPM_COL_PREP: dspan(st.x[0], M); dspan(st.x[1], n); break;
            case ASM_IPM_COL_SCALE: dspan(st.x[0], M); dspan(st.x[1], M); dspan(st.x[2], M); break;
            case ASM_IPM_COL_FINISH: dspan(st.x[0], M); dspan(st.x[1], M); dspan(st.x[2], M); dspan(st.x[3], M); break;
            case ASM_IPM_SDIAG_CSR: {
                const int64_t R = st.len[0];
                if (R < 0 || st.ix[0] < 0 || st.ix[0] + R + 1 > nint) throw std::invalid_argument("asm_test_ipm_stages: row pointers outside the int block");
                for (int64_t i = 0; i < R; ++i) if (ints[st.ix[0] + i] > ints[st.ix[0] + i + 1]) throw std::invalid_argument("asm_test_ipm_stages: row pointers decrease");
                if (ints[st.ix[0]] < 0) throw std::invalid_argument("asm_test_ipm_stages: negative row pointer");
                const int64_t nnz = ints[st.ix[0] + R];
                ilist(st.ix[1], nnz, st.len[1]);
                dspan(st.x[0], nnz); dspan(st.x[1], st.len[1]); dspan(st.x[2], R);
                break;
            }
            case ASM_IPM_RED_GATHER: ilist(st.ix[0], st.len[0], st.len[1]); dspan(st.x[0], st.len[1]); dspan(st.x[1], st.len[0]); break;
            case ASM_IPM_RED_SCATTER:
                if (st.len[2] < std::max(st.len[0], st.len[1])) throw std::invalid_argument("asm_test_ipm_stages: the scatter covers fewer rows than its lists hold");
                ilist(st.ix[0], st.len[0], st.len[2]); ilist(st.ix[1], st.len[1], st.len[2]);
                dspan(st.x[0], st.len[0]); dspan(st.x[1], st.len[1]); dspan(st.x[2], st.len[2]); dspan(st.x[3], st.len[2]);
                break;
            default:
                if (st.kind < 0 || st.kind >= ASM_IPM_NKINDS) throw std::invalid_argument("asm_test_ipm_stages: unknown stage");
            }
        }
        double *dD = nullptr, *dSnap = nullptr, *dRp = nullptr, *hScal = nullptr, *dhScal = nullptr;
        int* dI = nullptr;
        unsigned *dCnt = nullptr, *hSeq = nullptr, *dhSeq = nullptr;
        BufPool tmp;
        tmp.upload(dD, dbl_inout, ndbl);
        tmp.upload(dI, (const int*)ints, nint);
        tmp.upload(dSnap, snap_inout, lay.snap_len());
        tmp.upload(dRp, rpart_inout, (int64_t)IPM_RED_MAXWG * IPM_RED_SLOTS);
        tmp.upload(dCnt, (const unsigned*)rcnt_inout, 1);
        tmp.alloc(hScal, 64, BufPool::MAPPED, &dhScal);
        tmp.alloc(hSeq, 16, BufPool::MAPPED, &dhSeq);
        std::memcpy(hScal, hscal_inout, SC_COUNT * sizeof(double));
        *hSeq = *hseq_inout;
        ar.base = dD; ar.ibase = dI; ar.snap = dSnap; ar.hscal = dhScal; ar.hseq = dhSeq; ar.rpart = dRp; ar.rcnt = dCnt;
        S.ipm_bind(ar);
        S.P.n = n; S.P.M = M; S.P.ns = ns; S.P.ncomp = ncomp; S.P.scale_q = scale_q;
        for (int64_t q = 0; q < nstages; ++q) {      // one after the other on the handle's stream, no host synchronisation in between
            const asm_ipm_stage& st = stages[q];
            IpmDir& D = st.D ? S.dirC : S.dirA;
            IpmDir& B = st.B ? S.dirC : S.dirA;
            unsigned g = 0;
            switch (st.kind) {
            case ASM_IPM_INIT_P: g = S.launch_init_p(st.origin); break;
            case ASM_IPM_INIT_REST: g = S.launch_init_rest(st.mu_factor); break;
            case ASM_IPM_MEASURES: g = S.launch_measures(st.pub); break;
            case ASM_IPM_THETA: g = S.launch_theta(st.rho_p); break;
            case ASM_IPM_RHS1: g = S.launch_rhs1(B, st.mode, st.tp, st.td); break;
            case ASM_IPM_RHS2: g = S.launch_rhs2(st.res); break;
            case ASM_IPM_VEC_MUL: g = S.launch_vec_mul(dD + st.x[0], dD + st.x[1], st.len[0]); break;
            case ASM_IPM_RES: g = S.launch_res(D.dy, st.pub, st.spec, st.crel, st.floor_); break;
            case ASM_IPM_PCG_START: g = S.launch_pcg_start(); break;
            case ASM_IPM_PCG_STEP1: g = S.launch_pcg_step1(D.dy, st.pub); break;
            case ASM_IPM_PCG_STEP2: g = S.launch_pcg_step2(); break;
            case ASM_IPM_DIR: g = S.launch_dir(D); break;
            case ASM_IPM_STEPS: g = S.launch_steps(D, st.pub); break;
            case ASM_IPM_MUAFF: g = S.launch_muaff(D, st.sexp); break;
            case ASM_IPM_DIRADD: g = S.launch_diradd(D, B); break;
            case ASM_IPM_UPDATE: g = S.launch_update(D, st.al, st.be); break;
            case ASM_IPM_SNAPSHOT: g = S.launch_snapshot(st.with_e ? dD + st.x[0] : nullptr, st.dir); break;
            case ASM_IPM_COL_PREP: g = S.launch_col_prep(st.rho_p, st.fixed, dD + st.x[0], dD + st.x[1]); break;
            case ASM_IPM_COL_SCALE: g = S.launch_col_scale(dD + st.x[0], dD + st.x[1], dD + st.x[2]); break;
            case ASM_IPM_COL_FINISH: g = S.launch_col_finish(dD + st.x[0], dD + st.x[1], dD + st.x[2], dD + st.x[3]); break;
            case ASM_IPM_SDIAG_CSR: g = S.dev.launch_sdiag_csr(dI + st.ix[0], dI + st.ix[1], dD + st.x[0], dD + st.x[1], dD + st.x[2], st.len[0]); break;
            case ASM_IPM_RED_GATHER: g = S.launch_red_gather(dI + st.ix[0], (int)st.len[0], dD + st.x[0], dD + st.x[1]); break;
            default:
                g = S.launch_red_scatter(dI + st.ix[0], (int)st.len[0], dD + st.x[0], dI + st.ix[1], (int)st.len[1], dD + st.x[1], dD + st.x[2], dD + st.x[3], st.len[2]);
            }
            grid_out[q] = g;
        }
        HIPCHK(asmb::sync(h->stream));
        HIPCHK(asmb::copy(dbl_inout, dD, ndbl * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(asmb::copy(snap_inout, dSnap, lay.snap_len() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(asmb::copy(rpart_inout, dRp, (size_t)IPM_RED_MAXWG * IPM_RED_SLOTS * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(asmb::copy(rcnt_inout, dCnt, sizeof(unsigned), hipMemcpyDeviceToHost));
        std::memcpy(hscal_inout, hScal, SC_COUNT * sizeof(double));
        *hseq_inout = *hSeq;
    });
}

// The active-set and optimal-face kernels (asm_as_kernels.hip.h), one launch per stage, through the launch-site members of Solver and on arenas
// laid out by Solver::as_bind with the pitches of AsLayout - see include/asm_hip.h.  Every offset, set number, family / index pair and every
// index the caller's lists hold is checked here against the buffers before anything is launched.
static int test_as_stages(asm_handle* h, const asm_test_as_stages_args& a_);
int asm_test_as_stages(asm_handle* h, int64_t n, int64_t M, int64_t ns, double scale_q, int64_t* layout_out, double* dbl_inout, int64_t ndbl, int32_t* int_inout,
                       int64_t nint, const double* Ah, int64_t ah_rows, const asm_as_stage* stages, int64_t nstages, uint32_t* grid_out) {
    return test_as_stages(h, asm_test_as_stages_args{n, M, ns, scale_q, layout_out, dbl_inout, ndbl, int_inout, nint, Ah, ah_rows, stages, nstages, grid_out});
}
static int test_as_stages(asm_handle* h, const asm_test_as_stages_args& a_) {
    const int64_t n = a_.n, M = a_.M, ns = a_.ns, ndbl = a_.ndbl, nint = a_.nint, ah_rows = a_.ah_rows, nstages = a_.nstages;
    const double scale_q = a_.scale_q;
    int64_t* layout_out = a_.layout_out;
    double* dbl_inout = a_.dbl_inout;
    int32_t* int_inout = a_.int_inout;
    const double* Ah = a_.Ah;
    const asm_as_stage* stages = a_.stages;
    uint32_t* grid_out = a_.grid_out;
    return guarded(h, [&] {
        const int64_t LIM = (int64_t)1 << 24;
        if (!layout_out || n < 1 || M < 0 || ns < 0 || n > LIM || M > LIM || ns > LIM || (ns > 0 && M == 0) || nstages < 0)
            throw std::invalid_argument("asm_test_as_stages: bad size");
        HIPCHK(hipSetDevice(h->device));
        const AsLayout lay{IpmLayout(n, M, ns)};
        const int64_t ln = lay.ldn, lm = lay.Mp, ls = lay.nsp;
        Solver S(h);
        S.lp.n = n; S.lp.M = M; S.lp.ns = ns; S.lp.scale_q = scale_q;
        IpmPtrs& P = S.P;
        P = IpmPtrs();
        // the LP vectors and the interior-point iterate k_as_identify reads follow the solver's two arenas
        auto place_lp = [&](double* d, int* iv) {
            double* a = d + lay.dbl_len();
            auto N = [&]() { double* r_ = a; a += ln; return r_; };
            auto Mv = [&]() { double* r_ = a; a += lm; return r_; };
            auto Sv = [&]() { double* r_ = a; a += ls; return r_; };
            P.q = N(); P.lb = N(); P.ub = N(); P.r = Mv(); P.w = Sv(); P.slo = Sv(); P.scoef = Sv();
            P.p = N(); P.tL = N(); P.tU = N(); P.muL = N(); P.muU = N(); P.g = Mv(); P.pi = Mv(); P.y = Mv(); P.ts = Sv(); P.mus = Sv(); P.s = Sv();
            int* ia = iv + lay.int_len();
            P.rtype = ia; P.rs0 = ia + lm; P.rs1 = ia + 2 * lm; P.srow = ia + 3 * lm;
            P.n = n; P.M = M; P.ns = ns; P.scale_q = scale_q;
            Solver::AsArena ar;
            ar.base = d; ar.ibase = iv; ar.rperm = ia + 3 * lm + ls; ar.ln = ln; ar.lm = lm; ar.ls = ls;
            S.as_bind(ar);
        };
        const int64_t dbl_total = lay.dbl_len() + 8 * ln + 4 * lm + 6 * ls, int_total = lay.int_len() + 4 * lm + ls;
        // the layout, from the pointers as_bind sets on host blocks of the full lengths
        std::vector<double> hostd((size_t)dbl_total);
        std::vector<int> hosti((size_t)int_total);
        double* const fd = hostd.data();
        int* const fi = hosti.data();
        place_lp(fd, fi);
        {
            auto off = [&](const double* v) { return (int64_t)(v - fd); };
            auto ioff = [&](const int* v) { return (int64_t)(v - fi); };
            const AsPtrs& A = S.A;
            const double* vs[ASM_AS_NVEC] = {A.Fmask, A.p, A.z, A.pB, A.pF, A.cF, A.rd, A.tN, A.xfull, A.nu, A.Hmask, A.sl, A.y, A.act, A.t, A.bH, A.v, A.u, A.yH, A.yfull, A.uacc,
                                             A.ax, A.s, S.d_pref, S.d_zero, S.d_p0, S.d_z0, S.d_pa, S.d_pf, S.d_zf, S.d_y0, S.d_act0, S.d_acta, S.d_actf, S.d_yf, S.d_s0, S.d_sa,
                                             S.d_sf, P.q, P.lb, P.ub, P.r, P.w, P.slo, P.scoef, P.p, P.tL, P.tU, P.muL, P.muU, P.g, P.pi, P.y, P.ts, P.mus, P.s};
            const int* is[ASM_AS_NIVEC] = {S.S_[0].rowst, S.S_[0].bst, S.S_[0].sst, S.S_[1].rowst, S.S_[1].bst, S.S_[1].sst, S.S_[2].rowst, S.S_[2].bst, S.S_[2].sst,
                                           S.S_[3].rowst, S.S_[3].bst, S.S_[3].sst, S.S_[4].rowst, S.S_[4].bst, S.S_[4].sst, S.S_[5].rowst, S.S_[5].bst, S.S_[5].sst,
                                           A.ksoft, A.Hidx, A.hpos, A.Fidx, A.fpos, P.rtype, P.rs0, P.rs1, P.srow, A.rperm};
            const int64_t head[9] = {ln, lm, ls, dbl_total, int_total, off(A.scal), AS_COUNT, ioff(A.cnt), AC_COUNT};
            for (int k = 0; k < 9; ++k) layout_out[k] = head[k];
            for (int k = 0; k < ASM_AS_NVEC; ++k) layout_out[9 + k] = off(vs[k]);
            for (int k = 0; k < ASM_AS_NIVEC; ++k) layout_out[9 + ASM_AS_NVEC + k] = ioff(is[k]);
            if (head[5] + AS_COUNT > lay.dbl_len() || head[7] + AC_COUNT > lay.int_len()) throw std::logic_error("asm_test_as_stages: an arena is shorter than its layout");
        }
        if (!dbl_inout) return;      // layout query
        if (!int_inout || (nstages > 0 && (!stages || !grid_out)) || ndbl < dbl_total || nint < int_total || ndbl > ((int64_t)1 << 31) || nint > ((int64_t)1 << 31))
            throw std::invalid_argument("asm_test_as_stages: bad buffer");
        const int32_t* iv = int_inout;
        auto ioff = [&](const int* v) { return (int64_t)(v - fi); };
        const int64_t o_rt = ioff(P.rtype), o_rs0 = ioff(P.rs0), o_rs1 = ioff(P.rs1), o_srow = ioff(P.srow), o_rperm = ioff(S.A.rperm), o_ksoft = ioff(S.A.ksoft),
                      o_hidx = ioff(S.A.Hidx), o_hpos = ioff(S.A.hpos), o_cnt = ioff(S.A.cnt);
        for (int64_t i = 0; i < M; ++i) {
            const int rt = iv[o_rt + i], k0 = iv[o_rs0 + i], k1 = iv[o_rs1 + i], rp = iv[o_rperm + i];
            if (rt < -1 || rt > 1 || k0 < -1 || k0 >= ns || k1 < -1 || k1 >= ns) throw std::invalid_argument("asm_test_as_stages: row type or slack index out of range");
            if (rp < 0 || rp >= M) throw std::invalid_argument("asm_test_as_stages: row order out of range");
        }
        for (int64_t k = 0; k < ns; ++k)
            if (iv[o_srow + k] < 0 || iv[o_srow + k] >= M) throw std::invalid_argument("asm_test_as_stages: slack row out of range");
        auto dspan = [&](int64_t off, int64_t len, bool nullable = false) {
            if (nullable && off == -1) return;
            if (off < 0 || len < 0 || off + len > ndbl) throw std::invalid_argument("asm_test_as_stages: vector outside the double block");
        };
        auto setno = [&](const asm_as_stage& st, int cnt) {
            for (int a = 0; a < cnt; ++a)
                if (st.set[a] < 0 || st.set[a] > 5) throw std::invalid_argument("asm_test_as_stages: set number");
        };
        auto fam_e = [&](const asm_as_stage& st) {
            const int64_t lim = st.fam == 0 ? M : (st.fam == 1 ? ns : n);
            if (st.fam < 0 || st.fam > 3 || st.e < 0 || st.e >= lim) throw std::invalid_argument("asm_test_as_stages: family / index out of range");
        };
        // lists a kernel reads that an earlier k_as_setup (ksoft: or k_face_ns_step / k_as_sl_values) of the same call did not write are the caller's
        bool own_lists = false, own_ksoft = false, need_ah = false;
        auto lists_ok = [&](bool hidx, bool hpos) {
            if (own_lists) return;
            const int nH = iv[o_cnt + AC_NH];
            if (nH < 0 || nH > M) throw std::invalid_argument("asm_test_as_stages: hard-row count out of range");
            if (hidx) for (int64_t a = 0; a < nH; ++a)
                if (iv[o_hidx + a] < 0 || iv[o_hidx + a] >= M) throw std::invalid_argument("asm_test_as_stages: hard-row list out of range");
            if (hpos) for (int64_t i = 0; i < M; ++i)
                if (iv[o_hpos + i] < -1 || iv[o_hpos + i] >= lm) throw std::invalid_argument("asm_test_as_stages: hard-row position out of range");
        };
        auto ksoft_ok = [&]() {
            if (own_ksoft) return;
            for (int64_t i = 0; i < M; ++i)
                if (iv[o_ksoft + i] < -1 || iv[o_ksoft + i] >= ns) throw std::invalid_argument("asm_test_as_stages: basic-slack index out of range");
        };
        for (int64_t q = 0; q < nstages; ++q) {
            const asm_as_stage& st = stages[q];
            switch (st.kind) {
            case ASM_AS_IDENTIFY: setno(st, 1); break;
            case ASM_AS_CLIP0: dspan(st.x[0], n, true); dspan(st.x[1], n); break;
            case ASM_AS_SL: break;
            case ASM_AS_SL_VALUES: own_ksoft = true; break;
            case ASM_AS_SMAX: dspan(st.x[0], ns); dspan(st.x[1], ns); break;
            case ASM_AS_SETUP: setno(st, 1); dspan(st.x[0], n, true); own_lists = own_ksoft = true; break;
            case ASM_AS_RHS: dspan(st.x[0], M, true); lists_ok(true, false); break;
            case ASM_AS_RES_P: case ASM_AS_GATHER_H: case ASM_AS_ADD_YH:
                if (st.k < 0 || st.k > M) throw std::invalid_argument("asm_test_as_stages: host count of hard rows");
                lists_ok(true, false);
                break;
            case ASM_AS_SCATTER_H: dspan(st.x[0], lm); lists_ok(false, true); break;
            case ASM_AS_ADD_F: case ASM_AS_RD: break;
            case ASM_AS_MERGE: lists_ok(false, true); break;
            case ASM_AS_FINISH: setno(st, 3); ksoft_ok(); break;
            case ASM_FACE_PRIMAL_FINISH: setno(st, 2); ksoft_ok(); lists_ok(false, true); break;
            case ASM_FACE_NS_COMBINE:
                if (st.k < 0 || st.k > 4096) throw std::invalid_argument("asm_test_as_stages: member count");
                dspan(st.x[0], n); dspan(st.x[1], (int64_t)st.k * ln); dspan(st.x[2], st.k); dspan(st.x[3], n);
                break;
            case ASM_FACE_NS_STEP: setno(st, 1); dspan(st.x[0], n); dspan(st.x[1], ns); dspan(st.x[2], M); own_ksoft = true; break;
            case ASM_FACE_NS_COL:
                fam_e(st); dspan(st.x[0], n); dspan(st.x[1], M);
                if (!Ah || ah_rows < M) throw std::invalid_argument("asm_test_as_stages: the matrix has fewer rows than the LP");
                need_ah = true;
                break;
            case ASM_FACE_NS_Z: dspan(st.x[0], n); break;
            case ASM_FACE_NS_UNMARK: setno(st, 1); fam_e(st); break;
            case ASM_FACE_DUAL_FINISH: setno(st, 1); lists_ok(false, true); break;
            case ASM_FACE_KKT: setno(st, 1); break;
            case ASM_AS_PACK: setno(st, 1); dspan(st.x[0], 2 * n + 2 * M + ns + (M + n + ns + 1) / 2); break;
            case ASM_AS_COPY_SETS: setno(st, 2); break;
            default: throw std::invalid_argument("asm_test_as_stages: unknown stage");
            }
        }
        double *dD = nullptr, *dAh = nullptr;
        int* dI = nullptr;
        BufPool tmp;
        tmp.upload(dD, dbl_inout, ndbl);
        tmp.upload(dI, (const int*)int_inout, nint);
        if (need_ah) tmp.upload(dAh, Ah, ah_rows * ln);
        place_lp(dD, dI);
        const int* const rperm = S.A.rperm;
        auto X = [&](int64_t off) { return off < 0 ? nullptr : dD + off; };
        for (int64_t q = 0; q < nstages; ++q) {      // one after the other on the handle's stream, no host synchronisation in between
            const asm_as_stage& st = stages[q];
            auto SS = [&](int v) -> const AsSets& { return S.S_[v < 0 || v > 5 ? 0 : v]; };      // (the numbers a stage uses were checked above)
            const AsSets &s0 = SS(st.set[0]), &s1 = SS(st.set[1]), &s2 = SS(st.set[2]);
            S.A.rperm = st.rperm ? rperm : nullptr;
            unsigned g = 0;
            switch (st.kind) {
            case ASM_AS_IDENTIFY: g = S.launch_as_identify(s0); break;
            case ASM_AS_CLIP0: g = S.launch_as_clip0(X(st.x[0]), X(st.x[1])); break;
            case ASM_AS_SL: g = S.launch_as_sl(); break;
            case ASM_AS_SL_VALUES: g = S.launch_as_sl_values(); break;
            case ASM_AS_SMAX: g = S.launch_as_smax(X(st.x[0]), X(st.x[1])); break;
            case ASM_AS_SETUP: g = S.launch_as_setup(s0, X(st.x[0])); break;
            case ASM_AS_RHS: g = S.launch_as_rhs(X(st.x[0])); break;
            case ASM_AS_RES_P: g = S.launch_as_res_p(st.k); break;
            case ASM_AS_SCATTER_H: g = S.launch_as_scatter_h(X(st.x[0]), st.accumulate); break;
            case ASM_AS_ADD_F: g = S.launch_as_add_f(); break;
            case ASM_AS_RD: g = S.launch_as_rd(); break;
            case ASM_AS_GATHER_H: g = S.launch_as_gather_h(st.k); break;
            case ASM_AS_ADD_YH: g = S.launch_as_add_yh(st.k); break;
            case ASM_AS_MERGE: g = S.launch_as_merge(st.with_y); break;
            case ASM_AS_FINISH: g = S.launch_as_finish(s0, s1, s2, st.have_prev, st.tol_p, st.tol_d); break;
            case ASM_FACE_PRIMAL_FINISH: g = S.launch_face_primal_finish(s0, s1, st.tol_p, st.tol_m, st.check_only); break;
            case ASM_FACE_NS_COMBINE: g = S.launch_face_ns_combine(X(st.x[0]), X(st.x[1]), ln, X(st.x[2]), st.k, X(st.x[3])); break;
            case ASM_FACE_NS_STEP: g = S.launch_face_ns_step(s0, X(st.x[0]), X(st.x[1]), X(st.x[2]), st.tol_p); break;
            case ASM_FACE_NS_COL: g = S.launch_face_ns_col(dAh, ln, st.fam, st.e, X(st.x[0]), X(st.x[1])); break;
            case ASM_FACE_NS_Z: g = S.launch_face_ns_z(X(st.x[0])); break;
            case ASM_FACE_NS_UNMARK: g = S.launch_face_ns_unmark(s0, st.fam, st.e); break;
            case ASM_FACE_DUAL_FINISH: g = S.launch_face_dual_finish(s0, st.tol_m); break;
            case ASM_FACE_KKT: g = S.launch_face_kkt(s0); break;
            case ASM_AS_PACK: g = S.launch_as_pack(s0, X(st.x[0])); break;
            default: g = S.launch_as_copy_sets(s0, s1);
            }
            grid_out[q] = g;
        }
        HIPCHK(asmb::sync(h->stream));
        HIPCHK(asmb::copy(dbl_inout, dD, ndbl * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(asmb::copy(int_inout, dI, nint * sizeof(int), hipMemcpyDeviceToHost));
    });
}

// The kernels of the KKT column family and of the SLP-EQP trial step (asm_kkt_kernels.hip.h, asm_eqp_kernels.hip.h), one launch per stage,
// through the launch sites the drivers use (KktSites) and on blocks of the hook's own with the solver's pitches - see include/asm_hip.h.
// Every size, offset and index is checked here before anything is launched.
static int test_kkt_stages(asm_handle* h, const asm_test_kkt_stages_args& a_);
int asm_test_kkt_stages(asm_handle* h, int64_t n, int64_t M, int64_t nW, int64_t capW, int32_t cols, int64_t* layout_out, double* dbl_inout, int64_t ndbl,
                        int32_t* int_inout, int64_t nint, const int64_t* i64, int64_t ni64, uint32_t* cnt_inout, uint32_t* act_inout, double* hscal_inout,
                        uint32_t* hseq_inout, const asm_kkt_stage* stages, int64_t nstages, uint32_t* grid_out) {
    return test_kkt_stages(h, asm_test_kkt_stages_args{n, M, nW, capW, cols, layout_out, dbl_inout, ndbl, int_inout, nint, i64, ni64, cnt_inout, act_inout, hscal_inout,
                                                       hseq_inout, stages, nstages, grid_out});
}
static int test_kkt_stages(asm_handle* h, const asm_test_kkt_stages_args& a_) {
    const int64_t n = a_.n, M = a_.M, nW = a_.nW, capW = a_.capW, ndbl = a_.ndbl, nint = a_.nint, ni64 = a_.ni64, nstages = a_.nstages;
    const int32_t cols = a_.cols;
    int64_t* layout_out = a_.layout_out;
    double *dbl_inout = a_.dbl_inout, *hscal_inout = a_.hscal_inout;
    int32_t* int_inout = a_.int_inout;
    const int64_t* i64 = a_.i64;
    uint32_t *cnt_inout = a_.cnt_inout, *act_inout = a_.act_inout, *hseq_inout = a_.hseq_inout, *grid_out = a_.grid_out;
    const asm_kkt_stage* stages = a_.stages;
    return guarded(h, [&] {
        const int64_t LIM = (int64_t)1 << 20, CW = KKM_CW;
        if (!layout_out || n < 1 || n > LIM || M < 0 || M > LIM || nW < 0 || nW > capW || capW > LIM || (nW > 0 && M == 0) || cols < 1 || cols > CW || nstages < 0)
            throw std::invalid_argument("asm_test_kkt_stages: bad size");
        const int64_t ldn = IpmLayout(n, M, 0).ldn, Mp = std::max<int64_t>(IpmLayout(n, M, 0).Mp, 32), ldT = round_up(std::max<int64_t>(capW, 1), 32);
        const int64_t nWp = round_up(nW, 32), nWg = round_up(nW, 64);
        const int64_t o_vec = 0, o_row = o_vec + 14 * CW * ldn, o_dlf = o_row + 5 * CW * ldT, o_mask = o_dlf + CW * Mp, o_rad = o_mask + ldn, o_scal = o_rad + CW,
                      o_part = o_scal + CW * KKM_SCAL + 16, dbl_total = o_part + CW * KK_MAXWG * KK_SLOTS;
        const int64_t io_wrow = 0, io_wpos = Mp, io_rows = 2 * Mp, io_counts = io_rows + CW, int_total = io_counts + 4;
        {
            const int64_t lay[ASM_KKT_LAYOUT_LEN] = {ldn, ldT, Mp, nWp, nWg, dbl_total, int_total, o_vec, o_row, o_dlf, o_mask, o_rad, o_scal, o_part,
                                                     io_wrow, io_wpos, io_rows, io_counts, KKM_SCAL, KK_MAXWG * KK_SLOTS};
            for (int k = 0; k < ASM_KKT_LAYOUT_LEN; ++k) layout_out[k] = lay[k];
        }
        if (!dbl_inout) return;      // layout query
        if (!int_inout || !cnt_inout || !act_inout || !hscal_inout || !hseq_inout || (nstages > 0 && (!stages || !grid_out)) || ndbl < dbl_total || nint < int_total ||
            ndbl > ((int64_t)1 << 31) || nint > ((int64_t)1 << 31) || ni64 < 0 || ni64 > ((int64_t)1 << 31) || (ni64 > 0 && !i64))
            throw std::invalid_argument("asm_test_kkt_stages: bad buffer");
        const int32_t* iv = int_inout;
        auto bad = [](const char* what) { throw std::invalid_argument(std::string("asm_test_kkt_stages: ") + what); };
        auto dspan = [&](int64_t off, int64_t len, bool nullable = false) {
            if (nullable && off == -1) return;
            if (off < 0 || len < 0 || off > ndbl || len > ndbl - off) bad("vector outside the double block");
        };
        auto ilist = [&](int64_t off, int64_t len, int64_t lo, int64_t hi) {      // an int list with entries in [lo, hi)
            if (off < 0 || len < 0 || off > nint || len > nint - off) bad("list outside the int block");
            for (int64_t a = 0; a < len; ++a)
                if (iv[off + a] < lo || iv[off + a] >= hi) bad("index out of range");
        };
        auto iptr = [&](int64_t off, int64_t len) -> int64_t {                     // a pointer list of len + 1 entries: from >= 0, not decreasing; its last entry
            ilist(off, len + 1, 0, (int64_t)1 << 31);
            for (int64_t a = 0; a < len; ++a)
                if (iv[off + a] > iv[off + a + 1]) bad("pointer list decreases");
            return iv[off + len];
        };
        auto llist = [&](int64_t off, int64_t len, int64_t lo, int64_t hi) {
            if (off < 0 || len < 0 || off > ni64 || len > ni64 - off) bad("list outside the 64-bit block");
            for (int64_t a = 0; a < len; ++a)
                if (i64[off + a] < lo || i64[off + a] >= hi) bad("index out of range");
        };
        auto lptr = [&](int64_t off, int64_t len) -> int64_t {
            llist(off, len + 1, 0, (int64_t)1 << 31);
            for (int64_t a = 0; a < len; ++a)
                if (i64[off + a] > i64[off + a + 1]) bad("pointer list decreases");
            return i64[off + len];
        };
        ilist(io_wrow, nW, 0, M);
        ilist(io_rows, cols, 0, std::max<int64_t>(M, 1));
        const int64_t vb = (int64_t)cols * ldn, rb = (int64_t)cols * ldT;      // the first `cols` rows of a block over the variables / the working rows
        bool own_wpos = false;
        for (int64_t q = 0; q < nstages; ++q) {
            const asm_kkt_stage& st = stages[q];
            const int64_t* x = st.x;
            for (int a = 0; a < 3; ++a)
                if (st.len[a] < 0 || st.len[a] > ((int64_t)1 << 24)) bad("length out of range");
            switch (st.kind) {
            case ASM_KKT_GATHER: case ASM_KKT_GATHER_T:
                if (st.len[0] < M) bad("the matrix has fewer rows than the LP");
                dspan(x[0], st.len[0] * ldn); dspan(x[1], st.kind == ASM_KKT_GATHER ? nW * ldn : ldn * ldT);
                break;
            case ASM_KKT_HESS_PRODUCT: {
                const int64_t nnz = lptr(st.lx[0], n);
                llist(st.lx[1], nnz, 0, st.len[0]); llist(st.lx[2], nnz, 0, n);
                dspan(x[0], CW * ldn); dspan(x[1], vb); dspan(x[2], st.len[0]);
                break;
            }
            case ASM_KKT_AXPBY: { const int64_t b = st.flag[2] ? rb : vb; dspan(x[0], b); dspan(x[1], b, true); dspan(x[2], b); break; }
            case ASM_KKT_SCATTER: dspan(x[0], rb); dspan(x[1], (int64_t)cols * Mp); break;
            case ASM_KKT_CROSS_RHS: case ASM_KKT_CROSS_RHS_COLS: {
                const bool one = st.kind == ASM_KKT_CROSS_RHS;
                if (st.len[0] < 0 || st.len[0] > M) bad("function rows outside [0, M]");
                const int64_t lc = n + M - st.len[0];
                if (!one && st.len[1] < lc) bad("pitch of the cross derivatives");
                dspan(x[0], one ? lc : (int64_t)cols * st.len[1]); dspan(x[1], one ? n : vb); dspan(x[2], one ? nW : rb);
                break;
            }
            case ASM_KKT_BOUND_RHS: dspan(x[0], cols, true); dspan(x[1], vb); dspan(x[2], rb); break;
            case ASM_KKT_CG_P: dspan(x[0], vb); dspan(x[1], vb); break;
            case ASM_KKT_NORMAL: case ASM_KKT_CG_DIR: dspan(x[0], vb); break;
            case ASM_KKT_CG_CURV: case ASM_KKT_CG_STEP: dspan(x[0], vb); dspan(x[1], vb); dspan(x[2], vb); dspan(x[3], vb); break;
            case ASM_KKT_FINISH: dspan(x[0], vb); dspan(x[1], vb); dspan(x[2], vb); dspan(x[3], rb); dspan(x[4], rb); dspan(x[5], vb); dspan(x[6], vb, true); break;
            case ASM_KKTS_VALS: {
                const int64_t ndup = lptr(st.lx[1], st.len[0]);
                llist(st.lx[0], ndup, 0, st.len[1]);
                dspan(x[0], st.len[1]); dspan(x[1], st.len[0]);
                break;
            }
            case ASM_KKTS_WPOS: own_wpos = true; break;
            case ASM_KKTS_MUL_A: {
                const int64_t nnz = iptr(st.ix[0], M);
                ilist(st.ix[1], nnz, 0, n);
                dspan(x[0], nnz); dspan(x[1], vb); dspan(x[2], rb);
                break;
            }
            case ASM_KKTS_MUL_AT: {
                const int64_t nnz = iptr(st.ix[0], n);
                ilist(st.ix[1], nnz, 0, M); ilist(st.ix[2], nnz, 0, st.len[0]);
                if (!own_wpos) ilist(io_wpos, M, -1, nW);
                dspan(x[0], st.len[0]); dspan(x[1], rb); dspan(x[2], vb);
                break;
            }
            case ASM_EQP_FACE: {
                const int64_t ne = st.len[0], me = st.len[1], na = st.len[2];
                if (ne < 0 || me < 0 || na < 0 || ne > LIM || me > LIM || na > me || std::max(ne, me) < 1) bad("sizes of the face");
                dspan(x[0], me); dspan(x[1], me); dspan(x[2], me); dspan(x[3], ne); dspan(x[4], ne); dspan(x[5], ne); dspan(x[6], me);
                ilist(st.ix[0], me + na, 0, 2); ilist(st.ix[1], ne, -1, 2); ilist(st.ix[2], me, -1, na);
                const int64_t lo = (int64_t)INT32_MIN, hi = (int64_t)INT32_MAX + 1;
                ilist(st.ix[3], me, lo, hi); ilist(st.ix[4], ne, lo, hi); ilist(st.ix[5], me, lo, hi); ilist(st.ix[6], EQP_COUNTS, lo, hi);
                break;
            }
            case ASM_EQP_TRIAL:
                if (st.len[0] < 1 || st.len[0] > LIM) bad("size of the trial step");
                for (int a = 0; a < 5; ++a) dspan(x[a], st.len[0]);
                dspan(x[5], EQP_SCAL);
                break;
            default: bad("unknown stage");
            }
        }
        HIPCHK(hipSetDevice(h->device));
        double *dD = nullptr, *hScal = nullptr, *dhScal = nullptr;
        int* dI = nullptr;
        int64_t* dL = nullptr;
        unsigned *dCnt = nullptr, *dAct = nullptr, *hSeq = nullptr, *dhSeq = nullptr;
        BufPool tmp;
        tmp.upload(dD, dbl_inout, ndbl);
        tmp.upload(dI, (const int*)int_inout, nint);
        tmp.upload(dL, i64, ni64);
        tmp.upload(dCnt, (const unsigned*)cnt_inout, CW + 1);
        tmp.upload(dAct, (const unsigned*)act_inout, CW);
        tmp.alloc(hScal, 64, BufPool::MAPPED, &dhScal);
        tmp.alloc(hSeq, 16, BufPool::MAPPED, &dhSeq);
        hScal[0] = hscal_inout[0];
        *hSeq = *hseq_inout;
        const KktSites at(h->stream, ldn, ldT);
        double* const scal = dD + o_scal;
        const KktMulti R{dD + o_part, dCnt, scal, dAct, dhScal, dhSeq};
        const KktRed R0{dD + o_part, dCnt, scal};
        const double* const mask = dD + o_mask;
        const int *wrow = dI + io_wrow, *rows = dI + io_rows;
        int* const wpos = dI + io_wpos;
        auto X = [&](int64_t off) { return off < 0 ? nullptr : dD + off; };
        for (int64_t q = 0; q < nstages; ++q) {      // one after the other on the handle's stream, no host synchronisation in between
            const asm_kkt_stage& st = stages[q];
            const int64_t* x = st.x;
            const double* const m_or_null = st.flag[0] ? mask : nullptr;
            unsigned g = 0;
            switch (st.kind) {
            case ASM_KKT_GATHER: g = at.gather(X(x[0]), wrow, mask, nW, nWg, X(x[1])); break;
            case ASM_KKT_GATHER_T: g = at.gather_t(X(x[0]), wrow, m_or_null, nW, nWp, X(x[1])); break;
            case ASM_KKT_HESS_PRODUCT: g = at.hess_product(dL + st.lx[0], dL + st.lx[1], dL + st.lx[2], X(x[2]), X(x[0]), n, cols, X(x[1])); break;
            case ASM_KKT_AXPBY:
                if (st.flag[2]) g = at.axpby_rows(st.s[0], X(x[0]), st.s[1], X(x[1]), nW, nWg, X(x[2]), cols);
                else g = at.axpby(st.s[0], X(x[0]), st.s[1], X(x[1]), m_or_null, st.flag[1] ? scal : nullptr, X(x[2]), cols);
                break;
            case ASM_KKT_SCATTER: g = at.scatter(X(x[0]), wrow, nW, nWg, X(x[1]), Mp, cols); break;
            case ASM_KKT_CROSS_RHS: g = at.cross_rhs(X(x[0]), n, st.len[0], wrow, nW, X(x[1]), X(x[2])); break;
            case ASM_KKT_CROSS_RHS_COLS: g = at.cross_rhs_cols(X(x[0]), st.len[1], n, st.len[0], wrow, nW, X(x[1]), X(x[2]), cols); break;
            case ASM_KKT_BOUND_RHS: g = at.bound_rhs(rows, X(x[0]), wrow, nW, X(x[1]), X(x[2]), cols); break;
            case ASM_KKT_CG_P: g = at.cg_p(scal, X(x[0]), X(x[1]), cols); break;
            case ASM_KKT_NORMAL: g = at.normal(scal, dD + o_rad, st.s[0], X(x[0]), cols); break;
            case ASM_KKT_CG_CURV: g = at.cg_curv(st.flag[0] != 0, R, X(x[0]), X(x[1]), mask, X(x[2]), X(x[3]), cols); break;
            case ASM_KKT_CG_STEP: g = at.cg_step(scal, X(x[0]), X(x[1]), X(x[2]), X(x[3]), cols); break;
            case ASM_KKT_CG_DIR: g = at.cg_dir(R, X(x[0]), st.flag[0], st.s[0], st.pub, st.flag[1], cols); break;
            case ASM_KKT_FINISH: g = at.finish(scal, X(x[0]), X(x[1]), X(x[2]), mask, n, X(x[3]), X(x[4]), nW, X(x[5]), X(x[6]), cols); break;
            case ASM_KKTS_VALS: g = at.kkts_vals(X(x[0]), dL + st.lx[0], dL + st.lx[1], st.len[0], X(x[1])); break;
            case ASM_KKTS_WPOS: g = at.kkts_wpos(wrow, nW, M, wpos); break;
            case ASM_KKTS_MUL_A: g = at.kkts_mul_a(dI + st.ix[0], dI + st.ix[1], X(x[0]), wrow, mask, X(x[1]), nW, nWg, X(x[2]), cols); break;
            case ASM_KKTS_MUL_AT: g = at.kkts_mul_at(dI + st.ix[0], dI + st.ix[1], dI + st.ix[2], X(x[0]), wpos, m_or_null, X(x[1]), n, X(x[2]), cols); break;
            case ASM_EQP_FACE: {
                const EqpFace P{X(x[0]), X(x[1]), X(x[2]), X(x[3]), X(x[4]), X(x[5]), dI + st.ix[0], dI + st.ix[1], dI + st.ix[2], st.len[0], st.len[1], st.s[0]};
                g = at.eqp_face(P, R0, dI + st.ix[3], dI + st.ix[4], dI + st.ix[5], X(x[6]), dI + st.ix[6]);
                break;
            }
            default: g = at.eqp_trial(X(x[0]), X(x[1]), X(x[2]), X(x[3]), st.len[0], R0, X(x[4]), X(x[5]));
            }
            grid_out[q] = g;
        }
        HIPCHK(asmb::sync(h->stream));
        HIPCHK(asmb::copy(dbl_inout, dD, ndbl * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(asmb::copy(int_inout, dI, nint * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(asmb::copy(cnt_inout, dCnt, (CW + 1) * sizeof(unsigned), hipMemcpyDeviceToHost));
        HIPCHK(asmb::copy(act_inout, dAct, CW * sizeof(unsigned), hipMemcpyDeviceToHost));
        hscal_inout[0] = hScal[0];
        *hseq_inout = *hSeq;
    });
}

// The kernels of a null-space interior-point iteration and of ns_finish_y (asm_ns_kernels.hip.h), one launch site per stage, through the
// launch-site members of Solver / Dev and on buffers of the caller's laid out with the pitches of IpmLayout and NsLayout - see
// include/asm_hip.h.  The CSC view and the index lists are made by the routines do_setup uses; the factor is what Dev::chol leaves in a buffer
// of ns_alloc_factor.  Every size, offset and index is checked here before anything is launched.
static int test_ns_stages(asm_handle* h, const asm_test_ns_stages_args& a_);
int asm_test_ns_stages(asm_handle* h, int64_t n, int64_t M, int64_t k, double scale_q, const int32_t* rtype, const int32_t* ptr, const int32_t* col, const double* vals,
                       const double* Nreg, const double* N0, int64_t* layout_out, int32_t* idx_out, double* dbl_inout, int64_t ndbl, double* hscal_inout,
                       uint32_t* hseq_inout, const asm_ns_stage* stages, int64_t nstages, uint32_t* grid_out) {
    return test_ns_stages(h, asm_test_ns_stages_args{n, M, k, scale_q, rtype, ptr, col, vals, Nreg, N0, layout_out, idx_out, dbl_inout, ndbl, hscal_inout, hseq_inout,
                                                     stages, nstages, grid_out});
}
static int test_ns_stages(asm_handle* h, const asm_test_ns_stages_args& a_) {
    const int64_t n = a_.n, M = a_.M, k = a_.k, ndbl = a_.ndbl, nstages = a_.nstages;
    const double scale_q = a_.scale_q;
    const int32_t *rtype = a_.rtype, *ptr = a_.ptr, *col = a_.col;
    const double *vals = a_.vals, *Nreg = a_.Nreg, *N0 = a_.N0;
    int64_t* layout_out = a_.layout_out;
    int32_t* idx_out = a_.idx_out;
    double *dbl_inout = a_.dbl_inout, *hscal_inout = a_.hscal_inout;
    uint32_t *hseq_inout = a_.hseq_inout, *grid_out = a_.grid_out;
    const asm_ns_stage* stages = a_.stages;
    return guarded(h, [&] {
        const int64_t LIM = (int64_t)1 << 20;
        if (!layout_out || !rtype || n < 1 || M < 1 || n > LIM || M > LIM || k < 1 || k > n || k > ASM_SMALL_MAX || nstages < 0)
            throw std::invalid_argument("asm_test_ns_stages: bad size");
        int64_t nE = 0;
        for (int64_t i = 0; i < M; ++i) {
            if (rtype[i] < -1 || rtype[i] > 1) throw std::invalid_argument("asm_test_ns_stages: row type out of range");
            nE += rtype[i] == 0;
        }
        HIPCHK(hipSetDevice(h->device));
        const IpmLayout lay(n, M, 0);
        const NsLayout nl(lay.ldn, lay.Mp, nE, M - nE);
        Solver S(h);
        S.lp.n = n; S.lp.M = M; S.lp.ns = 0; S.lp.scale_q = scale_q;
        Solver::IpmArena ar;
        ar.ln = lay.ldn; ar.lm = lay.Mp; ar.ls = lay.nsp;
        ar.base = reinterpret_cast<double*>((uintptr_t)1 << 30);      // the layout, from pointers that are never dereferenced
        S.ipm_bind(ar);
        // the factor buffer as ns_alloc_factor sizes it for order k
        const int64_t fld = round_up(k, 32), linv_len = (fld / ASM_NB + 1) * ASM_NB * ASM_NB, g_rows = k + 1;
        const int64_t o_th = lay.arena_len(), o_v = o_th + nl.th_len(), o_G = o_v + nl.nsv_len(), o_S = o_G + g_rows * nl.ldg, o_Linv = o_S + fld * fld,
                      o_N0 = o_Linv + linv_len, o_part = o_N0 + fld * fld, o_end = o_part + (int64_t)ASM_TMAXCHUNKS * lay.ldn;
        {
            const double* vs[ASM_IPM_NVEC];
            S.ipm_vectors(vs);
            const int64_t head[ASM_NS_LAYOUT_HEAD] = {lay.ldn, lay.Mp, nl.nEp, nl.nIp, nl.ldg, fld, nE, M - nE, o_end, SC_COUNT,
                                                      (int64_t)(S.P.scal - ar.base), o_th, o_G, g_rows, o_S, o_Linv, linv_len, o_N0, o_part, ASM_SMALL_USE};
            for (int q = 0; q < ASM_NS_LAYOUT_HEAD; ++q) layout_out[q] = head[q];
            for (int q = 0; q < 16; ++q) layout_out[ASM_NS_LAYOUT_HEAD + q] = o_v + nl.nsv_off(q);
            for (int q = 0; q < ASM_IPM_NVEC; ++q) layout_out[ASM_NS_LAYOUT_HEAD + 16 + q] = (int64_t)(vs[q] - ar.base);
        }
        if (!dbl_inout) return;      // layout query
        if (!ptr || !col || !vals || !Nreg || !N0 || !idx_out || !hscal_inout || !hseq_inout || (nstages > 0 && (!stages || !grid_out)) || ndbl < o_end ||
            ndbl > ((int64_t)1 << 28))
            throw std::invalid_argument("asm_test_ns_stages: bad buffer");
        if (nE < 1) throw std::invalid_argument("asm_test_ns_stages: the null-space form needs an equality row");
        if (ptr[0] != 0) throw std::invalid_argument("asm_test_ns_stages: row pointers do not start at 0");
        for (int64_t i = 0; i < M; ++i)
            if (ptr[i] > ptr[i + 1]) throw std::invalid_argument("asm_test_ns_stages: row pointers decrease");
        const int64_t nnz = ptr[M];
        if (nnz > ((int64_t)1 << 26)) throw std::invalid_argument("asm_test_ns_stages: too many entries");
        for (int64_t e = 0; e < nnz; ++e)
            if (col[e] < 0 || col[e] >= n) throw std::invalid_argument("asm_test_ns_stages: column index out of range");
        auto dspan = [&](int64_t off, int64_t len) {
            if (off < 0 || len < 0 || off + len > ndbl) throw std::invalid_argument("asm_test_ns_stages: vector outside the double block");
        };
        bool factored = false;
        for (int64_t q = 0; q < nstages; ++q) {
            const asm_ns_stage& st = stages[q];
            if (st.D < 0 || st.D > 1 || st.B < 0 || st.B > 1 || st.mode < 0 || st.mode > 1) throw std::invalid_argument("asm_test_ns_stages: direction selector or mode");
            switch (st.kind) {
            case ASM_NS_FACTOR: factored = true; break;
            case ASM_NS_REDUCED_SOLVE: case ASM_NS_NEWTON:
                if (!factored) throw std::invalid_argument("asm_test_ns_stages: a solve before ASM_NS_FACTOR");
                break;
            case ASM_NS_CHOL_SOLVE:
                if (!factored) throw std::invalid_argument("asm_test_ns_stages: a solve before ASM_NS_FACTOR");
                dspan(st.x[0], k); dspan(st.x[1], k);
                break;
            case ASM_NS_E0: dspan(st.x[0], lay.ldn); break;
            case ASM_NS_ZT: dspan(st.x[0], lay.ldn); dspan(st.x[1], k); break;
            case ASM_NS_GEMV_T: dspan(st.x[0], k); dspan(st.x[1], lay.ldn); break;
            case ASM_NS_SYMV_RES: dspan(st.x[0], k); dspan(st.x[1], k); dspan(st.x[2], k); break;
            case ASM_NS_ADD: dspan(st.x[0], st.len); dspan(st.x[1], st.len); dspan(st.x[2], st.len); break;
            case ASM_NS_RELRES: dspan(st.x[0], k); dspan(st.x[1], k); break;
            case ASM_NS_DP: dspan(st.x[0], lay.ldn); break;
            case ASM_NS_DINF: dspan(st.x[0], k); break;
            case ASM_NS_GATHER_E: dspan(st.x[0], M); dspan(st.x[1], nE); break;
            case ASM_NS_SCATTER_E: dspan(st.x[0], nE); dspan(st.x[1], M); break;
            case ASM_NS_ROWVEC_E: dspan(st.x[0], nE); dspan(st.x[1], M); break;
            case ASM_NS_FILL: dspan(st.x[0], st.len); break;
            default:
                if (st.kind < 0 || st.kind >= ASM_NS_NKINDS) throw std::invalid_argument("asm_test_ns_stages: unknown stage");
            }
        }
        // CSC view and index lists, by the routines of do_setup
        std::vector<int> sp_ptr(ptr, ptr + M + 1), sp_col(col, col + nnz), sc_ptr, sc_row, sc_pos, eidx, epos, iidx, ipos;
        csc_from_csr(sp_ptr, sp_col, n, sc_ptr, sc_row, sc_pos);
        ns_index_lists((const int*)rtype, M, sp_ptr, sp_col, lay.ldn, eidx, epos, iidx, ipos, nullptr, nullptr);
        {
            int32_t* o = idx_out;
            auto put = [&](const std::vector<int>& v) { for (int x : v) *o++ = x; };
            put(sc_ptr); put(sc_row); put(sc_pos); put(eidx); put(epos); put(iidx); put(ipos);
        }
        // the generic buffers the factorisation and the wide substitutions use (pivot reference, flags, scratch), for order k
        test_alloc(h, round_up(k, 64), 16);
        std::vector<int> iv(lay.int_len(), -1);
        for (int64_t i = 0; i < lay.Mp; ++i) iv[i] = i < M ? rtype[i] : 0;
        iv[3 * lay.Mp] = 0;
        // N0 as ns_newton_matrix stores it (lower triangle; mirrored for the one-workgroup solve), N into the lower triangle of the factor buffer
        for (int64_t i = 0; i < k; ++i)
            for (int64_t j = 0; j <= i; ++j) {
                dbl_inout[o_N0 + i * fld + j] = N0[i * k + j];
                if (k <= ASM_SMALL_USE) dbl_inout[o_N0 + j * fld + i] = N0[i * k + j];
            }
        std::vector<double> dg0(k);
        for (int64_t i = 0; i < k; ++i) dg0[i] = N0[i * k + i];
        double *dD = nullptr, *dV = nullptr, *hScal = nullptr, *dhScal = nullptr;
        int *dI = nullptr, *dPtr = nullptr, *dCol = nullptr, *dCp = nullptr, *dCr = nullptr, *dCq = nullptr, *dE = nullptr, *dEp = nullptr, *dIi = nullptr, *dIp = nullptr;
        unsigned *hSeq = nullptr, *dhSeq = nullptr;
        BufPool tmp;
        FacBuf fN;
        ns_alloc_factor(h, tmp, fN, k);
        fN.small = true;
        if (fN.ld != fld) throw std::logic_error("asm_test_ns_stages: factor pitch");
        tmp.upload(dD, dbl_inout, ndbl);
        tmp.upload(dI, iv.data(), (int64_t)iv.size());
        tmp.upload(dPtr, sp_ptr.data(), M + 1); tmp.upload(dCol, sp_col.data(), std::max<int64_t>(nnz, 1)); tmp.upload(dV, vals, std::max<int64_t>(nnz, 1));
        tmp.upload(dCp, sc_ptr.data(), n + 1); tmp.upload(dCr, sc_row.data(), std::max<int64_t>(nnz, 1)); tmp.upload(dCq, sc_pos.data(), std::max<int64_t>(nnz, 1));
        iidx.push_back(0);      // (never empty: an LP without inequality rows)
        tmp.upload(dE, eidx.data(), nE); tmp.upload(dEp, epos.data(), M); tmp.upload(dIi, iidx.data(), (int64_t)iidx.size()); tmp.upload(dIp, ipos.data(), M);
        tmp.alloc(hScal, 64, BufPool::MAPPED, &dhScal);
        tmp.alloc(hSeq, 16, BufPool::MAPPED, &dhSeq);
        std::memcpy(hScal, hscal_inout, SC_COUNT * sizeof(double));
        *hSeq = *hseq_inout;
        HIPCHK(asmb::copy(h->sk->d_diag0, dg0.data(), k * sizeof(double), hipMemcpyHostToDevice));
        for (int64_t i = 0; i < k; ++i)
            HIPCHK(asmb::copy(fN.S + i * fld, Nreg + i * k, (i + 1) * sizeof(double), hipMemcpyHostToDevice));
        ar.base = dD; ar.ibase = dI; ar.hscal = dhScal; ar.hseq = dhSeq;
        S.ipm_bind(ar);
        S.P.n = n; S.P.M = M; S.P.ns = 0; S.P.ncomp = std::max<int64_t>(1, 2 * n + (M - nE)); S.P.scale_q = scale_q;
        Solver::NsArena na;
        na.v = dD + o_v; na.th = dD + o_th; na.G = dD + o_G; na.N0 = dD + o_N0; na.partial = dD + o_part;
        na.sp_ptr = dPtr; na.sp_col = dCol; na.sc_ptr = dCp; na.sc_row = dCr; na.sc_pos = dCq; na.vals = dV;
        na.X.Eidx = dE; na.X.Epos = dEp; na.X.Iidx = dIi; na.X.Ipos = dIp; na.X.nE = (int)nE; na.X.nI = (int)(M - nE);
        na.fN = &fN; na.L = nl;
        S.ns_bind(na);
        S.ip.ns_k = (int)k;
        const int kk = (int)k;
        for (int64_t q = 0; q < nstages; ++q) {      // one after the other on the handle's stream, no host synchronisation in between
            const asm_ns_stage& st = stages[q];
            IpmDir& D = st.D ? S.dirC : S.dirA;
            IpmDir& B = st.B ? S.dirC : S.dirA;
            auto X = [&](int a) { return dD + st.x[a]; };
            unsigned g = 0;
            switch (st.kind) {
            case ASM_NS_THETA: g = S.launch_theta_ns(st.rho_p); break;
            case ASM_NS_FACTOR: S.dev.chol(fN, kk, 1e-14, false); break;
            case ASM_NS_E0: g = S.launch_ns_e0(X(0), S.nsv(2)); break;
            case ASM_NS_ZT: g = S.launch_ns_zt(X(0), X(1), kk); break;
            case ASM_NS_GEMV_T: g = S.ns_gemv_t_dense(X(0), kk, X(1)); break;
            case ASM_NS_E1: g = S.launch_ns_e1(S.nsv(2), S.nsv(3), S.nsv(14)); break;
            case ASM_NS_WM_NEG: g = S.launch_ns_spmvn_wm_neg(S.ns_vals()); break;
            case ASM_NS_KX: g = S.launch_ns_spmvt_kx(S.ns_vals()); break;
            case ASM_NS_RHS1_BI: g = S.launch_ns_rhs1_bi(B, st.mode, st.res); break;
            case ASM_NS_HT: g = S.launch_ns_spmvt_ht(S.ns_vals(), st.res); break;
            case ASM_NS_RU: g = S.launch_ns_zt(S.nsv(3), S.nsv(10), kk); break;
            case ASM_NS_REDUCED_SOLVE: g = S.ns_reduced_solve(kk); break;
            case ASM_NS_DIRECTION: g = S.ns_direction(kk, D, st.res); break;
            case ASM_NS_ROWS: g = S.launch_ns_spmvn_rows(S.ns_vals(), D); break;
            case ASM_NS_NEWTON: S.ns_newton(st.mode, B, D); break;
            case ASM_NS_CHOL_SOLVE: S.dev.chol_solve_dev(fN, X(0), X(1), kk); g = kk <= ASM_SMALL_USE ? 1u : 0u; break;
            case ASM_NS_SYMV_RES: g = S.launch_ns_symv_res(kk, X(0), X(1), X(2)); break;
            case ASM_NS_ADD: g = S.launch_ns_add(X(0), X(1), X(2), st.len); break;
            case ASM_NS_RELRES: g = S.launch_ns_relres(X(0), X(1), kk); break;
            case ASM_NS_DP: g = S.launch_ns_dp(D, st.res, X(0)); break;
            case ASM_NS_UPDATE: g = S.launch_ns_update(D, st.al, st.be, st.es); break;
            case ASM_NS_UPDATE_DEV: g = S.launch_ns_update_dev(D, st.eta, st.rerr); break;
            case ASM_NS_DINF: g = S.launch_ns_dinf(X(0), kk, st.pub); break;
            case ASM_NS_GATHER_E: g = S.launch_ns_gather_e(X(0), st.scale, X(1)); break;
            case ASM_NS_SCATTER_E: g = S.launch_ns_scatter_e(X(0), X(1), st.add); break;
            case ASM_NS_ROWVEC_E: g = S.launch_ns_rowvec_e(X(0), X(1)); break;
            default: g = S.dev.launch_ns_fill(X(0), st.val, st.len);
            }
            grid_out[q] = g;
        }
        HIPCHK(asmb::sync(h->stream));
        if (factored) {      // the factor and the inverses of its 64-wide diagonal blocks, as the factorisation left them
            HIPCHK(asmb::copy(dD + o_S, fN.S, fld * fld * sizeof(double), hipMemcpyDeviceToDevice));
            HIPCHK(asmb::copy(dD + o_Linv, fN.Linv, linv_len * sizeof(double), hipMemcpyDeviceToDevice));
        }
        HIPCHK(asmb::copy(dbl_inout, dD, ndbl * sizeof(double), hipMemcpyDeviceToHost));
        std::memcpy(hscal_inout, hScal, SC_COUNT * sizeof(double));
        *hseq_inout = *hSeq;
        S.dev.resolve_timing();
        check_panel_timeout(h);
    });
}

// The basis set-up of the null-space form (Solver::ns_setup and its members), one launch site per stage, on a handle asm_sublp_setup has set
// up and whose skeleton has the form - see include/asm_hip.h.  The stages run on the form's own buffers (sk().nsf), which the caller loads and
// gets back whole; the Jacobian is assembled and scaled as asm_test_build_dispatch does it.  Every size, index and stage order is checked
// before anything is launched.
static int test_ns_setup_stages(asm_handle* h, const asm_test_ns_setup_stages_args& a_);
int asm_test_ns_setup_stages(asm_handle* h, const double* dE, const double* fm, int64_t k, int64_t k_reserve, const int32_t* J, int64_t* layout_out, int32_t* idx_out,
                             double* G_inout, double* R_inout, double* X_inout, double* SN_inout, double* Y_inout, double* T_inout, double* d_inout, double* f0_out,
                             double* Lt_out, int32_t Zk, const int32_t* hint_J, int64_t nhint, const asm_nss_stage* stages, int64_t nstages, uint32_t* grid_out,
                             int32_t* res_out, int32_t* setup_out) {
    return test_ns_setup_stages(h, asm_test_ns_setup_stages_args{dE, fm, k, k_reserve, J, layout_out, idx_out, G_inout, R_inout, X_inout, SN_inout, Y_inout, T_inout,
                                                                 d_inout, f0_out, Lt_out, Zk, hint_J, nhint, stages, nstages, grid_out, res_out, setup_out});
}
static int test_ns_setup_stages(asm_handle* h, const asm_test_ns_setup_stages_args& a_) {
    const double *dE = a_.dE, *fm = a_.fm;
    const int64_t k = a_.k, k_reserve = a_.k_reserve, nhint = a_.nhint, nstages = a_.nstages;
    const int32_t *J = a_.J, *hint_J = a_.hint_J;
    int64_t* layout_out = a_.layout_out;
    int32_t *idx_out = a_.idx_out, *res_out = a_.res_out, *setup_out = a_.setup_out;
    double *G_inout = a_.G_inout, *R_inout = a_.R_inout, *X_inout = a_.X_inout, *SN_inout = a_.SN_inout, *Y_inout = a_.Y_inout, *T_inout = a_.T_inout;
    double *d_inout = a_.d_inout, *f0_out = a_.f0_out, *Lt_out = a_.Lt_out;
    const int32_t Zk = a_.Zk;
    const asm_nss_stage* stages = a_.stages;
    uint32_t* grid_out = a_.grid_out;
    return guarded(h, [&] {
        Skeleton& K = sk_of(h, "asm_test_ns_setup_stages: asm_sublp_setup first");
        NsForm* const ns = K.nsf.get();
        const int64_t n = K.n, M = K.M;
        if (!ns || !layout_out || !fm || (K.nnz > 0 && !dE) || nstages < 0 || k < 1 || k > n || k_reserve < k ||
            (double)k_reserve > 1.5 * NS_MAX_RATIO * (double)M + 8.0)
            throw std::invalid_argument("asm_test_ns_setup_stages: no null-space form on this handle, or a bad size");
        for (int64_t j = 0; j < n; ++j)
            if (fm[j] != 0.0 && fm[j] != 1.0) throw std::invalid_argument("asm_test_ns_setup_stages: fm is 0 or 1");
        if (J)
            for (int64_t c = 0; c < k; ++c)
                if (J[c] < 0 || J[c] >= n) throw std::invalid_argument("asm_test_ns_setup_stages: column index out of range");
        if (nhint < 0 || nhint > n || (nhint > 0 && !hint_J)) throw std::invalid_argument("asm_test_ns_setup_stages: bad list of retained columns");
        for (int64_t c = 0; c < nhint; ++c)
            if (hint_J[c] < 0 || hint_J[c] >= n) throw std::invalid_argument("asm_test_ns_setup_stages: column index out of range");
        const NsLayout& L = ns->L;
        const int cap = NsLayout::kcap((int)k_reserve);
        if (Zk < 0 || Zk > cap) throw std::invalid_argument("asm_test_ns_setup_stages: rows of the previous basis");
        const int64_t Tld = K.main_fac.ld;
        bool s0 = false, facN = false, needY = Y_inout != nullptr;
        for (int64_t q = 0; q < nstages; ++q) {
            if (!stages || !grid_out || !res_out) throw std::invalid_argument("asm_test_ns_setup_stages: bad buffer");
            const asm_nss_stage& st = stages[q];
            if (st.kind < 0 || st.kind >= ASM_NSS_NKINDS) throw std::invalid_argument("asm_test_ns_setup_stages: unknown stage");
            if (st.flag < 0 || (st.flag > 1 && st.kind != ASM_NSS_COUNT_BIG)) throw std::invalid_argument("asm_test_ns_setup_stages: stage flag");
            switch (st.kind) {
            case ASM_NSS_S0_FACTOR: s0 = true; break;
            case ASM_NSS_RHS_COLS:
                if (st.flag == 0 && !J) throw std::invalid_argument("asm_test_ns_setup_stages: the stage needs the column list");
                if (st.flag == 1) needY = true;
                break;
            case ASM_NSS_TRSM:
                if (!s0) throw std::invalid_argument("asm_test_ns_setup_stages: a substitution before ASM_NSS_S0_FACTOR");
                if (st.flag == 0) needY = true;
                break;
            case ASM_NSS_PJ:
                if (st.flag == 0 && !J) throw std::invalid_argument("asm_test_ns_setup_stages: the stage needs the column list");
                break;
            case ASM_NSS_GATHER_T:
                if (!J) throw std::invalid_argument("asm_test_ns_setup_stages: the stage needs the column list");
                break;
            case ASM_NSS_FACTOR_N: facN = true; break;
            case ASM_NSS_ORTHO:
                if (!facN) throw std::invalid_argument("asm_test_ns_setup_stages: ASM_NSS_ORTHO before ASM_NSS_FACTOR_N");
                break;
            case ASM_NSS_COUNT_BIG:
                if (st.flag > Tld) throw std::invalid_argument("asm_test_ns_setup_stages: order beyond the main factor");
                break;
            case ASM_NSS_REPROJECT:
                if (!s0) throw std::invalid_argument("asm_test_ns_setup_stages: a substitution before ASM_NSS_S0_FACTOR");
                break;
            case ASM_NSS_BASIS_FROM:
                if (!s0) throw std::invalid_argument("asm_test_ns_setup_stages: a substitution before ASM_NSS_S0_FACTOR");
                if (!J) throw std::invalid_argument("asm_test_ns_setup_stages: the stage needs the column list");
                break;
            case ASM_NSS_SETUP:
                if (!setup_out) throw std::invalid_argument("asm_test_ns_setup_stages: bad buffer");
                break;
            default: break;      // ROWS_E, GRAM, GI, SET_DIAG, DIAG: nothing beyond the sizes
            }
        }
        HIPCHK(hipSetDevice(h->device));
        Solver S(h);
        S.lp.n = n; S.lp.M = M; S.lp.ns = 0; S.lp.scale_q = 1.0;
        S.lp.lb.assign(n, 0.0); S.lp.ub.assign(fm, fm + n);
        // an earlier LP of the skeleton with k_reserve basis rows has made the k-sized buffers (another reservation is dropped first)
        if (ns->k && ns->k->cap != cap) { HIPCHK(asmb::sync(h->stream)); ns->k.reset(); }
        S.ns_bind();
        S.ns_reserve((int)k_reserve);
        S.ns_bind();
        if (ns->k->cap != cap) throw std::logic_error("asm_test_ns_setup_stages: reservation");
        if (needY) S.ns_cold_buffers();
        {
            const int64_t out[ASM_NSS_LAYOUT_LEN] = {K.ldn, L.nEp, L.nIp, L.ldg, L.nE, L.nI, ns->f0.band, ns->f0.ld, cap, ns->k->fN.ld, ns->k->fN.wb, n, M, Tld, K.Mp, 0};
            for (int q = 0; q < ASM_NSS_LAYOUT_LEN; ++q) layout_out[q] = out[q];
            if (idx_out) {
                std::copy(ns->eidx_h.begin(), ns->eidx_h.end(), idx_out);
                HIPCHK(asmb::copy(idx_out + L.nE, ns->Iidx, L.nI * sizeof(int), hipMemcpyDeviceToHost));
            }
        }
        if (!stages) return;      // layout query
        if (ns->f0.ld != L.nEp) throw std::logic_error("asm_test_ns_setup_stages: pitch of the factor of S0");
        HIPCHK(asmb::copy(K.d_dE, dE, K.nnz * sizeof(double), hipMemcpyHostToDevice));
        K.J_valid = false;
        S.dev.assemble();
        {
            vec c(n, 1.0), rho(M);
            S.dev.scale(c.data(), rho.data());
        }
        S.dev.tile_flags();
        auto NK = [&]() -> NsK& { return *ns->k; };      // (never kept across ASM_NSS_SETUP: ns_reserve may re-make the buffers)
        const int64_t fld = NK().fN.ld, ylen = 2 * K.ldn * L.nEp;
        {
            vec f(K.ldn, 0.0);
            std::copy(fm, fm + n, f.begin());
            HIPCHK(asmb::copy(ns->Fm, f.data(), K.ldn * sizeof(double), hipMemcpyHostToDevice));
        }
        if (J) HIPCHK(asmb::copy(NK().J, J, k * sizeof(int), hipMemcpyHostToDevice));
        if (G_inout) HIPCHK(asmb::copy(NK().G, G_inout, cap * L.ldg * sizeof(double), hipMemcpyHostToDevice));
        if (R_inout) HIPCHK(asmb::copy(NK().R, R_inout, cap * L.nEp * sizeof(double), hipMemcpyHostToDevice));
        if (X_inout) HIPCHK(asmb::copy(NK().X, X_inout, cap * L.nEp * sizeof(double), hipMemcpyHostToDevice));
        if (SN_inout) HIPCHK(asmb::copy(NK().fN.S, SN_inout, fld * fld * sizeof(double), hipMemcpyHostToDevice));
        if (Y_inout) HIPCHK(asmb::copy(ns->Yt, Y_inout, ylen * sizeof(double), hipMemcpyHostToDevice));
        if (T_inout) HIPCHK(asmb::copy(K.main_fac.S, T_inout, Tld * Tld * sizeof(double), hipMemcpyHostToDevice));
        if (d_inout) HIPCHK(asmb::copy(K.d_vecN, d_inout, K.ldn * sizeof(double), hipMemcpyHostToDevice));
        const int kk = (int)k, nn = (int)n;
        SolveHint hint(false);
        for (int64_t q = 0; q < nstages; ++q) {      // one after the other on the handle's stream; the host waits only where the solver does
            const asm_nss_stage& st = stages[q];
            const double* vals = S.dev.sparse_vals(K.d_Ah);
            unsigned g = 0;
            int res = 0;
            switch (st.kind) {
            case ASM_NSS_S0_FACTOR: res = S.ns_factor_S0(); S.ns_make_Lt(); break;
            case ASM_NSS_RHS_COLS: g = st.flag ? S.launch_ns_rhs_cols(vals, nullptr, nn, ns->Yt) : S.launch_ns_rhs_cols(vals, NK().J, kk, NK().R); break;
            case ASM_NSS_ROWS_E: g = S.launch_ns_rows_e(vals, kk); break;
            case ASM_NSS_TRSM:
                if (st.flag) S.dev.trsm_rows(ns->f0, NK().R, NK().X, L.nEp, kk, (int)L.nE, ns->Lt);
                else S.dev.trsm_rows(ns->f0, ns->Yt, ns->Yt + K.ldn * L.nEp, L.nEp, nn, (int)L.nE, nullptr);
                break;
            case ASM_NSS_PJ: g = S.launch_ns_pj(vals, kk, st.flag); break;
            case ASM_NSS_GATHER_T: g = S.launch_ns_gather_t(kk); break;
            case ASM_NSS_GRAM: S.launch_ns_gram(kk); break;
            case ASM_NSS_FACTOR_N: res = S.ns_factor_N(kk, st.thr); break;
            case ASM_NSS_ORTHO: g = S.ns_ortho(kk); break;
            case ASM_NSS_GI: g = S.launch_ns_gi(vals, kk); break;
            case ASM_NSS_SET_DIAG: g = S.launch_ns_set_diag(K.main_fac, nn, st.flag ? nullptr : ns->Fm); break;
            case ASM_NSS_DIAG: g = S.launch_ns_diag(K.main_fac, nn, K.d_vecN); break;
            case ASM_NSS_COUNT_BIG: res = S.ns_count_big(K.main_fac, st.flag); g = 1; break;
            case ASM_NSS_REPROJECT: res = S.ns_reproject(kk, st.thr) ? 1 : 0; g = (unsigned)((L.nEp + 255) / 256); break;
            case ASM_NSS_BASIS_FROM: res = S.ns_basis_from(std::vector<int>(J, J + k)) ? 1 : 0; g = (unsigned)kk; break;
            default: {
                hint.ns_J.assign(hint_J, hint_J + nhint);
                S.cur_hint = &hint;
                NK().Zk = Zk;
                res = S.ns_setup() ? 1 : 0;
                setup_out[0] = S.ns_path; setup_out[1] = res ? S.ns_k : 0; setup_out[2] = S.ns_dropped; setup_out[3] = (int32_t)hint.ns_J.size();
                std::copy(hint.ns_J.begin(), hint.ns_J.end(), setup_out + 4);
                if (NK().cap != cap) throw std::logic_error("asm_test_ns_setup_stages: the LP's null space is larger than k_reserve allows for");
            }
            }
            grid_out[q] = g;
            res_out[q] = res;
        }
        HIPCHK(asmb::sync(h->stream));
        if (G_inout) HIPCHK(asmb::copy(G_inout, NK().G, cap * L.ldg * sizeof(double), hipMemcpyDeviceToHost));
        if (R_inout) HIPCHK(asmb::copy(R_inout, NK().R, cap * L.nEp * sizeof(double), hipMemcpyDeviceToHost));
        if (X_inout) HIPCHK(asmb::copy(X_inout, NK().X, cap * L.nEp * sizeof(double), hipMemcpyDeviceToHost));
        if (SN_inout) HIPCHK(asmb::copy(SN_inout, NK().fN.S, fld * fld * sizeof(double), hipMemcpyDeviceToHost));
        if (Y_inout) {
            HIPCHK(asmb::copy(Y_inout, ns->Yt, ylen * sizeof(double), hipMemcpyDeviceToHost));
            // the padding of the rows L0^-1 a_j is an operand of T in the cold selection and no launch writes it: the solver relies on the
            // zeros it is made with, so whatever the caller loaded there does not outlive the call
            vec y(Y_inout + K.ldn * L.nEp, Y_inout + ylen);
            for (int64_t j = 0; j < K.ldn; ++j) std::fill(y.begin() + j * L.nEp + L.nE, y.begin() + (j + 1) * L.nEp, 0.0);
            HIPCHK(asmb::copy(ns->Yt + K.ldn * L.nEp, y.data(), y.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        if (T_inout) HIPCHK(asmb::copy(T_inout, K.main_fac.S, Tld * Tld * sizeof(double), hipMemcpyDeviceToHost));
        if (d_inout) HIPCHK(asmb::copy(d_inout, K.d_vecN, K.ldn * sizeof(double), hipMemcpyDeviceToHost));
        if (f0_out) HIPCHK(asmb::copy(f0_out, ns->f0.S, L.nEp * L.nEp * sizeof(double), hipMemcpyDeviceToHost));
        if (Lt_out) HIPCHK(asmb::copy(Lt_out, ns->Lt, L.nEp * L.nEp * sizeof(double), hipMemcpyDeviceToHost));
        ns->k->Zk = 0;      // the basis rows in G are the caller's: no later LP on this skeleton takes them for its predecessor's
        S.dev.resolve_timing();
        check_panel_timeout(h);
    });
}

// S[a,b] -= sum_k P[a,k] P[b,k] for a >= b (and b < MsB when MsB >= 0): the Cholesky update as the factorisation launches it
// (k_syrk_upd for tile 4, the generic kernel otherwise), with an offset origin inside a larger matrix (srow0) like a trailing update
static int test_syrk_update(asm_handle* h, const asm_test_syrk_update_args& a_);
int asm_test_syrk_update(asm_handle* h, const double* Pm, int64_t Ms, int64_t K, int64_t MsB, int64_t srow0, double* S_inout, int tile) {
    return test_syrk_update(h, asm_test_syrk_update_args{Pm, Ms, K, MsB, srow0, S_inout, tile});
}
static int test_syrk_update(asm_handle* h, const asm_test_syrk_update_args& a_) {
    const double* Pm = a_.P;
    const int64_t Ms = a_.Ms, K = a_.K, MsB = a_.MsB, srow0 = a_.srow0;
    double* S_inout = a_.S_inout;
    const int tile = a_.tile;
    return guarded(h, [&] {
        if (K % 64 != 0) throw HipError("asm_test_syrk_update: K must be a multiple of 64 (panel widths)");
        const int64_t N = srow0 + Ms;
        test_alloc(h, N, std::max<int64_t>(K, 16));
        Dev d(h);
        HIPCHK(asmb::fill(h->sk->d_Ah, 0, h->sk->Mp * h->sk->ldn * sizeof(double)));
        for (int64_t i = 0; i < Ms; ++i)
            HIPCHK(asmb::copy(h->sk->d_Ah + (srow0 + i) * h->sk->ldn, Pm + i * K, K * sizeof(double), hipMemcpyHostToDevice));
        const FacBuf& F = h->sk->main_fac;
        for (int64_t i = 0; i < Ms; ++i)
            HIPCHK(asmb::copy(F.S + (srow0 + i) * F.ld + srow0, S_inout + i * Ms, Ms * sizeof(double), hipMemcpyHostToDevice));
        d.launch_syrk(h->stream, tile > 0 ? tile : Dev::pick_tile(Ms), h->sk->d_Ah, h->sk->ldn, nullptr, srow0, (int)Ms, (int)K, nullptr, nullptr, F.S, F.ld, srow0, 1, (int)MsB);
        HIPCHK(asmb::sync(h->stream));
        for (int64_t i = 0; i < Ms; ++i)
            HIPCHK(asmb::copy(S_inout + i * Ms, F.S + (srow0 + i) * F.ld + srow0, Ms * sizeof(double), hipMemcpyDeviceToHost));
        d.resolve_timing();
    });
}

// S into the buffers the hooks factor in (asm_test_set_factor): the main factor, or a factor buffer of the null-space form's kind, made for
// this order (released with the other null-space buffers at the next set-up); either has the band of asm_test_set_band
static void test_load_S(asm_handle* h, const double* S, int64_t N) {
    test_alloc(h, N, 16);
    FacBuf* f = &h->sk->main_fac;
    if (h->test_layout == 1) {
        ns_alloc_factor(h, h->sk->mem, h->sk->test_fac, N, h->test_band_hint);
        HIPCHK(asmb::sync(h->stream));          // (the buffers are cleared on the stream)
        f = &h->sk->test_fac;
    }
    f->band = h->test_band;
    for (int64_t i = 0; i < N; ++i)
        HIPCHK(asmb::copy(f->S + i * f->ld, S + i * N, N * sizeof(double), hipMemcpyHostToDevice));
}
// factorisation of the loaded matrix with the hooks' guard settings, in the buffers it was loaded into; returns that factor
static const FacBuf& test_factor(asm_handle* h, Dev& d, int64_t N) {
    const FacBuf& f = h->test_layout == 1 ? h->sk->test_fac : h->sk->main_fac;
    d.diag_prepare(f, (int)N, h->test_mode, h->test_rel, h->test_abs);
    d.chol(f, (int)N, h->test_thr);
    return f;
}

int asm_test_set_factor(asm_handle* h, int layout, int band_hint, int mode, double rel, double absv, double thr) {
    return guarded(h, [&] {
        if (layout < 0 || layout > 1 || band_hint < 0 || mode < 0 || mode > 1 || !(rel >= 0.0) || !(absv >= 0.0) || !(thr >= 0.0))
            throw std::invalid_argument("asm_test_set_factor: bad argument");
        h->test_layout = layout; h->test_band_hint = band_hint; h->test_mode = mode;
        h->test_rel = rel; h->test_abs = absv; h->test_thr = thr;
    });
}

static int test_cholesky(asm_handle* h, const asm_test_cholesky_args& a_);
int asm_test_cholesky(asm_handle* h, const double* S, int64_t N, double* L_out) { return test_cholesky(h, asm_test_cholesky_args{S, N, L_out}); }
static int test_cholesky(asm_handle* h, const asm_test_cholesky_args& a_) {
    const double* S = a_.S;
    const int64_t N = a_.N;
    double* L_out = a_.L_out;
    return guarded(h, [&] {
        test_load_S(h, S, N);
        Dev d(h);
        const FacBuf& f = test_factor(h, d, N);
        HIPCHK(asmb::sync(h->stream));
        for (int64_t i = 0; i < N; ++i) {
            HIPCHK(asmb::copy(L_out + i * N, f.S + i * f.ld, N * sizeof(double), hipMemcpyDeviceToHost));
            for (int64_t j = i + 1; j < N; ++j) L_out[i * N + j] = 0.0;
        }
        d.resolve_timing();
        check_panel_timeout(h);
    });
}

// The bounded wait of the panel kernel with a producer that never publishes: the probe's workgroups must give up (the first after the
// full bound, the others at their next look at the timeout word), the host must report ASM_ERR_HIP once, and the handle must stay usable.
// the matrices the following kernel hooks load are banded with this half-bandwidth (0 = dense again): their factorisation and
// substitutions then stop at the band, as for the S0 of the null-space form
int asm_test_set_band(asm_handle* h, int band) {
    return guarded(h, [&] {
        if (band < 0) throw std::invalid_argument("asm_test_set_band: bad argument");
        h->test_band = band;
    });
}

// every active-set attempt of the following LPs fails (on != 0): the LP solve ends on its last resort, the converged interior iterate
int asm_test_no_polish(asm_handle* h, int on) {
    return guarded(h, [&] { h->test_no_polish = on != 0; });
}

int asm_test_panel_timeout(asm_handle* h, int workgroups) {
    return guarded(h, [&] {
        if (workgroups < 1 || workgroups > 64) throw std::invalid_argument("asm_test_panel_timeout: 1..64 workgroups");
        test_alloc(h, 64, 16);
        h->panel_epoch += 1;
        if (h->panel_epoch == 0) h->panel_epoch = 1;
        asmb::launch(k_pnl_wait_probe, dim3((unsigned)workgroups), dim3(256), h->stream, h->sk->d_pflags, h->panel_epoch, h->sk->d_ptmo);
        HIPCHK(asmb::sync(h->stream));
        check_panel_timeout(h);
    });
}

static int test_chol_solve(asm_handle* h, const asm_test_chol_solve_args& a_);
int asm_test_chol_solve(asm_handle* h, const double* S, int64_t N, const double* b, double* x) { return test_chol_solve(h, asm_test_chol_solve_args{S, N, b, x}); }
static int test_chol_solve(asm_handle* h, const asm_test_chol_solve_args& a_) {
    const double *S = a_.S, *b = a_.b;
    const int64_t N = a_.N;
    double* x = a_.x;
    return guarded(h, [&] {
        test_load_S(h, S, N);
        Dev d(h);
        const FacBuf& f = test_factor(h, d, N);
        d.chol_solve(f, b, x, (int)N);
        d.resolve_timing();
    });
}

static int test_gemm_nt(asm_handle* h, const asm_test_gemm_nt_args& a_);
int asm_test_gemm_nt(asm_handle* h, const double* A, const double* B, const double* C0, int64_t Ma, int64_t Mb, int64_t K, int mode, double* C_out) {
    return test_gemm_nt(h, asm_test_gemm_nt_args{A, B, C0, Ma, Mb, K, mode, C_out});
}
static int test_gemm_nt(asm_handle* h, const asm_test_gemm_nt_args& a_) {
    const double *A = a_.A, *B = a_.B, *C0 = a_.C0;
    const int64_t Ma = a_.Ma, Mb = a_.Mb, K = a_.K;
    const int mode = a_.mode;
    double* C_out = a_.C_out;
    return guarded(h, [&] {
        if (Ma <= 0 || Mb <= 0 || K <= 0 || K % 32 != 0 || !A || !B || !C_out || (mode != 0 && !C0)) throw std::invalid_argument("asm_test_gemm_nt: bad argument");
        HIPCHK(hipSetDevice(h->device));
        double *dA = nullptr, *dB = nullptr, *dC = nullptr;
        BufPool tmp;
        tmp.upload(dA, A, Ma * K); tmp.upload(dB, B, Mb * K);
        if (mode != 0) tmp.upload(dC, C0, Ma * Mb);
        else tmp.alloc(dC, Ma * Mb);
        const char* var = std::getenv("ASM_TEST_GEMM");      // tile variant under test: 32 (32 x 64), 32w (32 x 96), default 64 x 64
        if (var && std::string(var) == "32w")
            asmb::launch(k_gemm_nt32w, dim3((unsigned)((Mb + 95) / 96), (unsigned)((Ma + 31) / 32)), dim3(256), h->stream, dA, K, dB, K, (mode != 0 ? dC : nullptr), Mb, dC, Mb,
                         (int)Ma, (int)Mb, (int)K, mode);
        else if (var && std::string(var) == "32")
            asmb::launch(k_gemm_nt32, dim3((unsigned)((Mb + 63) / 64), (unsigned)((Ma + 31) / 32)), dim3(256), h->stream, dA, K, dB, K, (mode != 0 ? dC : nullptr), Mb, dC, Mb,
                         (int)Ma, (int)Mb, (int)K, mode);
        else
        asmb::launch(k_gemm_nt, dim3((unsigned)((Mb + 63) / 64), (unsigned)((Ma + 63) / 64)), dim3(256), h->stream, dA, K, dB, K, (mode != 0 ? dC : nullptr), Mb, dC, Mb, (int)Ma,
                     (int)Mb, (int)K, mode);
        HIPCHK(asmb::sync(h->stream));
        HIPCHK(asmb::copy(C_out, dC, Ma * Mb * sizeof(double), hipMemcpyDeviceToHost));
    });
}

static int test_trsm_rows(asm_handle* h, const asm_test_trsm_rows_args& a_);
int asm_test_trsm_rows(asm_handle* h, const double* S, int64_t N, const double* R, int64_t nrhs, int backward, double* X_out) {
    return test_trsm_rows(h, asm_test_trsm_rows_args{S, N, R, nrhs, backward, X_out});
}
static int test_trsm_rows(asm_handle* h, const asm_test_trsm_rows_args& a_) {
    const double *S = a_.S, *R = a_.R;
    const int64_t N = a_.N, nrhs = a_.nrhs;
    const int backward = a_.backward;
    double* X_out = a_.X_out;
    return guarded(h, [&] {
        if (N <= 0 || nrhs <= 0 || !S || !R || !X_out) throw std::invalid_argument("asm_test_trsm_rows: bad argument");
        test_load_S(h, S, N);
        Dev d(h);
        const FacBuf& f = test_factor(h, d, N);
        const int64_t ldr = round_up(N, 32);
        double *dR = nullptr, *dX = nullptr, *dLt = nullptr;
        BufPool tmp;
        tmp.zeroed(dR, nrhs * ldr); tmp.zeroed(dX, nrhs * ldr); tmp.zeroed(dLt, f.ld * f.ld);
        for (int64_t r = 0; r < nrhs; ++r) HIPCHK(asmb::copy(dR + r * ldr, R + r * N, N * sizeof(double), hipMemcpyHostToDevice));
        asmb::launch(k_transpose_dense, dim3((unsigned)((N + 63) / 64), (unsigned)((N + 63) / 64)), dim3(256), h->stream, f.S, f.ld, N, N, dLt, f.ld, (int64_t)-1);
        d.trsm_rows(f, dR, dX, ldr, (int)nrhs, (int)N, backward ? dLt : nullptr);
        HIPCHK(asmb::sync(h->stream));
        const double* out = backward ? dR : dX;
        for (int64_t r = 0; r < nrhs; ++r) HIPCHK(asmb::copy(X_out + r * N, out + r * ldr, N * sizeof(double), hipMemcpyDeviceToHost));
        d.resolve_timing();
    });
}

static int test_gemv(asm_handle* h, const asm_test_gemv_args& a_);
int asm_test_gemv(asm_handle* h, const double* A, int64_t M, int64_t K, const double* x, const double* y, double* Ax, double* ATy) {
    return test_gemv(h, asm_test_gemv_args{A, M, K, x, y, Ax, ATy});
}
static int test_gemv(asm_handle* h, const asm_test_gemv_args& a_) {
    const double *A = a_.A, *x = a_.x, *y = a_.y;
    const int64_t M = a_.M, K = a_.K;
    double *Ax = a_.Ax, *ATy = a_.ATy;
    return guarded(h, [&] {
        test_alloc(h, M, K);
        Dev d(h);
        for (int64_t i = 0; i < M; ++i)
            HIPCHK(asmb::copy(h->sk->d_Ah + i * h->sk->ldn, A + i * K, K * sizeof(double), hipMemcpyHostToDevice));
        d.gemv_n(h->sk->d_Ah, x, Ax);
        d.gemv_t(h->sk->d_Ah, y, ATy);
        d.resolve_timing();
    });
}

int asm_test_mfma_peak(asm_handle* h, int iters, int waves_per_simd, double* tflops) {
    return guarded(h, [&] {
        if (!tflops || iters <= 0 || waves_per_simd < 1 || waves_per_simd > 8) throw std::invalid_argument("asm_test_mfma_peak: bad argument");
        HIPCHK(hipSetDevice(h->device));
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, h->device));
        int blocks = prop.multiProcessorCount * waves_per_simd;          // 256-thread blocks: 4 wavefronts = one per SIMD
        double* d_out = nullptr;
        BufPool tmp;
        tmp.alloc(d_out, 8);
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        asmb::launch(k_mfma_f64_peak<4>, dim3(blocks), dim3(256), h->stream, d_out, iters / 10 + 1);   // warm-up
        HIPCHK(hipEventRecord(e0, h->stream));
        asmb::launch(k_mfma_f64_peak<4>, dim3(blocks), dim3(256), h->stream, d_out, iters);
        HIPCHK(hipEventRecord(e1, h->stream));
        HIPCHK(asmb::sync(h->stream));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        double flops = (double)blocks * 4.0 * (double)iters * 4.0 * 2.0 * 16 * 16 * 4;
        *tflops = flops / (ms * 1e-3) / 1e12;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    });
}

int asm_test_assemble(asm_handle* h, const double* dE, double* J_out) {
    return guarded(h, [&] {
        Skeleton& K = sk_of(h, "setup first");
        HIPCHK(asmb::copy(K.d_dE, dE, K.nnz * sizeof(double), hipMemcpyHostToDevice));
        K.J_valid = false;
        Dev d(h);
        d.assemble();
        HIPCHK(asmb::sync(h->stream));
        for (int64_t i = 0; i < K.M; ++i)
            HIPCHK(asmb::copy(J_out + i * K.n, K.d_J + i * K.ldn, K.n * sizeof(double), hipMemcpyDeviceToHost));
        d.resolve_timing();
    });
}

static int test_skeleton_stages(asm_handle* h, const asm_test_skeleton_stages_args& a_);
int asm_test_skeleton_stages(asm_handle* h, uint32_t stages, const double* dE, const double* lb, const double* ub, const double* c_in,
                             const double* x, const double* y, int64_t* info_out, double* J_out, double* rmax_out, double* rel_out,
                             double* c_out, double* rho_out, double* Ah_out, double* spvAh_out, double* Jx_out, double* JTy_out, double* Ahx_out,
                             double* AhTy_out, int32_t* route_out, double* norms_out, double* spnorms_out) {
    return test_skeleton_stages(h, asm_test_skeleton_stages_args{stages, dE, lb, ub, c_in, x, y, info_out, J_out, rmax_out, rel_out, c_out, rho_out, Ah_out, spvAh_out,
                                                                 Jx_out, JTy_out, Ahx_out, AhTy_out, route_out, norms_out, spnorms_out});
}
static int test_skeleton_stages(asm_handle* h, const asm_test_skeleton_stages_args& a_) {
    const uint32_t stages = a_.stages;
    const double *dE = a_.dE, *lb = a_.lb, *ub = a_.ub, *c_in = a_.c_in, *x = a_.x, *y = a_.y;
    int64_t* info_out = a_.info_out;
    double *J_out = a_.J_out, *rmax_out = a_.rmax_out, *rel_out = a_.rel_out, *c_out = a_.c_out, *rho_out = a_.rho_out, *Ah_out = a_.Ah_out;
    double *spvAh_out = a_.spvAh_out, *Jx_out = a_.Jx_out, *JTy_out = a_.JTy_out, *Ahx_out = a_.Ahx_out, *AhTy_out = a_.AhTy_out;
    int32_t* route_out = a_.route_out;
    double *norms_out = a_.norms_out, *spnorms_out = a_.spnorms_out;
    return guarded(h, [&] {
        Skeleton& K = sk_of(h, "asm_test_skeleton_stages: asm_sublp_setup first");
        const int64_t n = K.n, m = K.m, M = K.M;
        const bool bad = (stages & ~(uint32_t)ASM_SKS_ALL) || !info_out
            || ((stages & ASM_SKS_ASSEMBLE) && ((K.nnz > 0 && !dE) || !J_out))
            || ((stages & ASM_SKS_COLSCALE) && (!lb || !ub || !rel_out || !c_out || (M > 0 && !rmax_out)))
            || ((stages & ASM_SKS_SCALE) && ((!c_in && !(stages & ASM_SKS_COLSCALE)) || !Ah_out || (M > 0 && !rho_out)))
            || ((stages & ASM_SKS_PRODUCTS) && (!x || !JTy_out || !AhTy_out || !route_out || (M > 0 && (!y || !Jx_out || !Ahx_out))))
            || ((stages & ASM_SKS_NORMS) && m > 0 && !norms_out);
        if (bad) throw std::invalid_argument("asm_test_skeleton_stages: unknown stage or null pointer");
        HIPCHK(hipSetDevice(h->device));
        Dev d(h);
        int64_t R = 0, chunk = 0;
        if (M > 0) d.col_chunks(R, chunk);
        const int64_t info[ASM_SKS_INFO_LEN] = {n, m, M, K.Mp, K.ldn, K.sp_ok ? 1 : 0, K.sp_nnz, K.dense_fast ? 1 : 0, R, chunk};
        std::copy(info, info + ASM_SKS_INFO_LEN, info_out);
        auto image = [&](double* out, const double* src, int64_t len) {
            HIPCHK(asmb::sync(h->stream));
            HIPCHK(asmb::copy(out, src, len * sizeof(double), hipMemcpyDeviceToHost));
        };
        if (stages & ASM_SKS_ASSEMBLE) {
            HIPCHK(asmb::copy(K.d_dE, dE, K.nnz * sizeof(double), hipMemcpyHostToDevice));
            K.J_valid = false;
            K.inputs_ready = false;
        }
        vec rel(n), c(n), rho(M);
        d.scaled_matrix(lb, ub, rel.data(), c.data(), rho.data(), [&](const char* what) {
            if (what[0] == 'a') image(J_out, K.d_J, K.Mp * K.ldn);
            if (what[0] == 'r' && M > 0) image(rmax_out, K.d_rho, M);      // the row maxima are in d_rho until the scale puts rho there
            if (what[0] == 's') {
                image(Ah_out, K.d_Ah, K.Mp * K.ldn);
                if (K.sp_ok && spvAh_out) image(spvAh_out, K.d_spv_Ah, K.sp_nnz);
            }
        }, stages & (ASM_SKS_ASSEMBLE | ASM_SKS_COLSCALE | ASM_SKS_SCALE), c_in);
        if (stages & ASM_SKS_COLSCALE) { std::copy(rel.begin(), rel.end(), rel_out); std::copy(c.begin(), c.end(), c_out); }
        if (stages & ASM_SKS_SCALE) std::copy(rho.begin(), rho.end(), rho_out);
        if (stages & ASM_SKS_PRODUCTS) {
            const double none = 0.0;      // an LP without rows: y is empty, A x has no entries
            if (M > 0) d.gemv_n(K.d_J, x, Jx_out);
            route_out[0] = d.gemv_t(K.d_J, M > 0 ? y : &none, JTy_out);
            if (M > 0) d.gemv_n(K.d_Ah, x, Ahx_out);
            route_out[1] = d.gemv_t(K.d_Ah, M > 0 ? y : &none, AhTy_out);
        }
        if ((stages & ASM_SKS_NORMS) && m > 0) {
            d.launch_row_norms(K.d_vecM, false);
            d.d2h(norms_out, K.d_vecM, m);
            if (K.sp_ok && spnorms_out) {
                d.launch_row_norms(K.d_vecM2, true);
                d.d2h(spnorms_out, K.d_vecM2, m);
            }
        }
        d.resolve_timing();
    });
}

// asmb::copy_async (H2D, D2D, D2H) and asmb::fill_async at the caller's offsets inside two device buffers with a 64-byte margin on each side
static int test_copy_fill(asm_handle* h, const asm_test_copy_fill_args& a) {
    return guarded(h, [&] {
        auto inside = [&](int64_t off) { return off >= 0 && off <= a.span - a.bytes; };
        const bool h2d = a.ops & ASM_CF_H2D, d2d = a.ops & ASM_CF_D2D, fill = a.ops & ASM_CF_FILL, d2h = a.ops & ASM_CF_D2H;
        if ((a.ops & ~(uint32_t)ASM_CF_ALL) || a.span < 0 || a.span > ((int64_t)1 << 30) || a.bytes < 0 || a.bytes > a.span || !a.a_init || !a.b_init || !a.a_out ||
            !a.b_out || (h2d && (!a.host_src || !inside(a.dst_off))) || (d2d && (!inside(a.src_off) || !inside(a.dst_off))) || (fill && !inside(a.fill_off)) ||
            (d2h && (!a.host_out || !inside(a.src_off))))
            throw std::invalid_argument("asm_test_copy_fill: unknown operation, null pointer or a range outside the buffer");
        HIPCHK(hipSetDevice(h->device));
        const int64_t total = 64 + a.span + 64;
        char *dA = nullptr, *dB = nullptr;      // (hipMalloc aligns to 256 bytes: the working area at + 64 is 64-byte aligned)
        BufPool tmp;
        tmp.alloc(dA, total); tmp.alloc(dB, total);
        HIPCHK(asmb::copy(dA, a.a_init, total, hipMemcpyHostToDevice));
        HIPCHK(asmb::copy(dB, a.b_init, total, hipMemcpyHostToDevice));
        if (h2d) HIPCHK(asmb::copy_async(dA + 64 + a.dst_off, a.host_src, a.bytes, hipMemcpyHostToDevice, h->stream));
        if (d2d) HIPCHK(asmb::copy_async(dB + 64 + a.dst_off, dA + 64 + a.src_off, a.bytes, hipMemcpyDeviceToDevice, h->stream));
        if (fill) HIPCHK(asmb::fill_async(dB + 64 + a.fill_off, a.value, a.bytes, h->stream));
        if (d2h) HIPCHK(asmb::copy_async(a.host_out, dB + 64 + a.src_off, a.bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(asmb::sync(h->stream));
        HIPCHK(asmb::copy(a.a_out, dA, total, hipMemcpyDeviceToHost));
        HIPCHK(asmb::copy(a.b_out, dB, total, hipMemcpyDeviceToHost));
    });
}
int asm_test_copy_fill(asm_handle* h, uint32_t ops, int64_t span, int64_t bytes, int64_t dst_off, int64_t src_off, int64_t fill_off, int32_t value,
                       const uint8_t* a_init, const uint8_t* b_init, const uint8_t* host_src, uint8_t* host_out, uint8_t* a_out, uint8_t* b_out) {
    return test_copy_fill(h, asm_test_copy_fill_args{ops, span, bytes, dst_off, src_off, fill_off, value, a_init, b_init, host_src, host_out, a_out, b_out});
}

int asm_sublp_set_ns_basis(asm_handle* h, const int32_t* J, int64_t k) {
    return guarded(h, [&] { do_set_ns_basis(h, J, k); });
}

}  // extern "C"

// =========================================================================================================
// Native SLP driver (rows f2 of SURVEY.md section 8): run!(::SlpLS), slp_line_search.jl:78-215, on the device evaluator - the same
// sequence of library calls as activesetmethods_amd/slp.py (SlpLS.run with Parameters(device_eval=True)), statement by statement, so
// that a whole scenario solve is one C call and B of them can run as fibers of one host thread (asm_batch_slp_run).
// =========================================================================================================
namespace {

// the start point clamped into the variable bounds as the reference does it (slp_line_search.jl:96-104, slp_trust_region.jl:104-114): the
// upper clamp tests x_U > -Inf, sic
void clamp_start(int64_t n, const double* x0, const double* lb, const double* ub, double* x) {
    for (int64_t j = 0; j < n; ++j) {
        double v = x0[j];
        if (lb[j] > -INF) v = std::max(v, lb[j]);
        if (ub[j] > -INF) v = std::min(v, ub[j]);
        x[j] = v;
    }
}

// the state both drivers keep: iterate, the last LP's step and multipliers, status, counts and the caller's result record
struct SlpRun {
    asm_handle* h;
    const asm_slp_params& o;
    int64_t n, m;
    vec x, p, lam, mU, mL, ps, df, E, nu;
    double f = 0.0, phi = INF, prim_infeas = INF, dual_infeas = INF, compl_ = INF;
    bool fr = false;
    int iter = 1, ret = -5, lp_solves = 0, fr_solves = 0;
    asm_slp_result* res;

    SlpRun(asm_handle* hh, const asm_slp_params& par, asm_slp_result* r) : h(hh), o(par), n(hh->sk->n), m(hh->sk->m), res(r) {
        x.assign(n, 0.0); p.assign(n, 0.0); lam.assign(m, 0.0); mU.assign(n, 0.0); mL.assign(n, 0.0);
        ps.assign(2 * std::max<int64_t>(m, 1), 0.0); df.assign(n, 0.0); E.assign(std::max<int64_t>(m, 1), 0.0); nu.assign(m, 0.0);
    }
    bool feasible_enough() const { return prim_infeas <= o.tol_infeas; }
    double finite_or_zero(double v) const { return std::isfinite(v) ? v : 0.0; }
    void count_lp() {            // the LP just solved
        lp_solves += 1;
        if (fr) fr_solves += 1;
        if (res) {
            const int pth = h->stats.path;
            if (pth >= 0 && pth < 12) res->paths[pth] += 1;
            res->ipm_iters += h->stats.ipm_iters;
            res->ns_cold += h->stats.ns_cold;
        }
    }
    // the objective at the final point (slp_line_search.jl:208-214, slp_trust_region.jl:198) and the result record
    void finish(int tag, int ls_trials) {
        double f_end = 0.0;
        vec Et(std::max<int64_t>(m, 1));
        asmb::barrier(tag);
        do_eval_constraints(h, x.data(), &f_end, Et.data());
        if (res) {
            res->status = ret; res->iter = iter; res->lp_solves = lp_solves; res->restoration_solves = fr_solves; res->ls_trials = ls_trials;
            res->obj_val = f_end; res->prim_infeas = prim_infeas; res->dual_infeas = dual_infeas; res->compl_ = compl_;
        }
    }
    void outputs(double* x_out, double* lambda, double* mult_x_U, double* mult_x_L, double* g_out) const {
        if (x_out) std::memcpy(x_out, x.data(), n * sizeof(double));
        if (lambda && m) std::memcpy(lambda, lam.data(), m * sizeof(double));
        if (mult_x_U) std::memcpy(mult_x_U, mU.data(), n * sizeof(double));
        if (mult_x_L) std::memcpy(mult_x_L, mL.data(), n * sizeof(double));
        if (g_out && m) std::memcpy(g_out, E.data(), m * sizeof(double));
    }
};

struct SlpRunLS : SlpRun {
    double alpha = 1.0, D = 0.0;
    int ls_trials = 0;
    using SlpRun::SlpRun;

    void run(const double* x0) {
        clamp_start(n, x0, h->sk->v_lb.data(), h->sk->v_ub.data(), x.data());       // slp_line_search.jl:96-104
        while (true) {
            if (o.max_lp_solves > 0 && lp_solves >= o.max_lp_solves) break;
            asmb::next_cycle();
            asmb::barrier(10);
            do_eval_functions(h, x.data(), &f, df.data(), E.data());                                    // :109-110
            alpha = 0.0;
            double nrm[4];
            do_slp_norms(h, lam.data(), mU.data(), mL.data(), nrm);                                     // :113-118, the previous LP's multipliers
            prim_infeas = nrm[0]; dual_infeas = nrm[2]; compl_ = nrm[3];
            int32_t status = 0;
            do_solve(h, 1000.0, fr ? 1 : 0, p.data(), lam.data(), mU.data(), mL.data(), ps.data(), &status);   // :122-123
            count_lp();
            if (status != ASM_OPTIMAL && status != ASM_INFEASIBLE) {                                     // :127-133
                if (feasible_enough()) ret = 6;
                break;
            }
            if (status == ASM_INFEASIBLE) {                                                              // :135-147
                if (fr) { ret = feasible_enough() ? 6 : 2; break; }
                fr = true;
                continue;
            }
            for (int64_t i = 0; i < m; ++i) nu[i] = iter == 1 ? std::fabs(lam[i]) : std::max(nu[i], std::fabs(lam[i]));       // :251-261
            asmb::barrier(910);
            int trials = 0, ok = 0;
            double phi_a = 0.0;
            // compute_phi, compute_derivative, compute_alpha (:222-244) - as asm_slp_merit (modes 0, 1) + asm_slp_line_search, with one upload
            slp_merit_and_search(h, p.data(), nu.data(), ps.data(), fr ? 1 : 0, finite_or_zero(prim_infeas), o.eta, o.tau, o.min_alpha, &phi, &D, &alpha, &phi_a,
                                 &trials, &ok);
            ls_trials += trials;
            if (!ok && fr) ret = -3;
            const bool valid = ok != 0;
            if (iter >= o.max_iter) { ret = feasible_enough() ? 6 : -1; break; }                         // :160-166
            double pmax = 0.0;
            for (int64_t j = 0; j < n; ++j) pmax = std::max(pmax, std::fabs(p[j]));
            if ((feasible_enough() && compl_ <= o.tol_residual) || pmax <= o.tol_direction) {            // :168-182
                if (fr) { fr = false; iter += 1; continue; }
                if (dual_infeas <= o.tol_residual) { ret = 0; break; }
            }
            if (!valid) {                                                                                 // :184-199
                if (ret == -3) { ret = feasible_enough() ? 6 : 2; break; }
                fr = true;
                iter += 1;
                continue;
            }
            for (int64_t j = 0; j < n; ++j) x[j] = x[j] + alpha * p[j];                                  // :201-203
            iter += 1;
        }
        finish(990, ls_trials);
    }
};

void slp_run_ls(asm_handle* h, const asm_slp_params* par, const double* x0, double* x_out, double* lambda, double* mult_x_U, double* mult_x_L, double* g_out,
                asm_slp_result* res) {
    if (!h->ev) throw std::logic_error("asm_slp_run: asm_eval_setup first (the native driver evaluates on the device)");
    if (res) std::memset(res, 0, sizeof(*res));
    SlpRunLS r(h, *par, res);
    r.run(x0);
    r.outputs(x_out, lambda, mult_x_U, mult_x_L, g_out);
}

// run!(::SlpTR), slp_trust_region.jl:87-251 - statement by statement the library calls of SlpTR.run in activesetmethods_amd/slp.py with
// Parameters(device_eval=True).  One difference from the host driver: compute_nu's ||df||_2 is summed here in index order, NumPy's norm
// may round it differently in the last bit.  It only enters nu at iter 1 and through nu only the merit values and rho: iterates,
// multipliers, radius and counts stay bit-identical unless rho falls within an ulp of 0, 0.25 or 0.75.  The same holds for the 1-norm of
// the violations in the status-OTHER branch (device evaluator instead of the host's eval_g, a plain sum), which only decides ret 6 / -5.
struct SlpRunTR : SlpRun {
    vec rn;
    double Delta, Delta_max = 2.0, alpha1 = 0.1, alpha2 = 0.25;     // slp_trust_region.jl:62-65
    asm_slp_tr_info info{};
    int32_t lp_status = 0;          // the last LP solved: its status and whether it was a restoration LP
    bool lp_fr = false;
    virtual ~SlpRunTR() = default;
    // between the evaluation and the LP: nothing here (SlpRunEQP takes its step on the LP's working set)
    virtual void second_order_step() {}
    // before the accepted LP step changes x: nothing here (SlpRunEQP with the limited-memory Hessian saves the point of the next pair)
    virtual void before_lp_step() {}

    SlpRunTR(asm_handle* hh, const asm_slp_params& par, double tr_size, asm_slp_result* r)
        : SlpRun(hh, par, r), rn(std::max<int64_t>(m, 1), 0.0), Delta(tr_size) {}

    // slp.jl:54-66 (the base compute_nu!, not the Line-Search one)
    void compute_nu() {
        if (iter == 1) {
            double norm_df = 1.0;
            if (!fr) {
                double s = 0.0;
                for (int64_t j = 0; j < n; ++j) s += df[j] * df[j];
                norm_df = std::sqrt(s);
            }
            do_jac_row_norms(h, rn.data());
            for (int64_t i = 0; i < m; ++i) nu[i] = std::max(1.0, norm_df / std::max(1.0, rn[i]));
        } else {
            for (int64_t i = 0; i < m; ++i) nu[i] = std::max(nu[i], std::fabs(lam[i]));
        }
    }

    // step_quality (slp_trust_region.jl:213-251) as SlpTR.step_quality: the three merit values from one launch, the rest on the host
    double step_quality() {
        double q[3];
        slp_tr_step_quality(h, p.data(), nu.data(), ps.data(), fr ? 1 : 0, finite_or_zero(prim_infeas), q);
        phi = q[2] - q[1];
        const double phi_pre = q[0];
        if (std::fabs(phi_pre) > 0.0) {
            const double rho = phi / phi_pre, D0 = Delta;
            if (rho <= 0) Delta *= alpha1;
            else if (rho <= 0.25) Delta *= alpha2;
            else if (rho > 0.75) Delta = std::min(2 * Delta, Delta_max);
            if (Delta < D0) info.shrunk += 1;
            else if (Delta > D0) info.expanded += 1;
            return rho;
        }
        const double rho = -phi;
        if (std::fabs(phi) < 1.e-8) {
            if (fr) fr = false;
            else if (feasible_enough()) ret = (dual_infeas <= o.tol_residual && compl_ <= o.tol_residual) ? 0 : 6;
            else ret = 2;
        }
        return rho;
    }

    void run(const double* x0) {
        clamp_start(n, x0, h->sk->v_lb.data(), h->sk->v_ub.data(), x.data());       // slp_trust_region.jl:104-114
        while (true) {
            if (o.max_lp_solves > 0 && lp_solves >= o.max_lp_solves) break;
            asmb::next_cycle();
            asmb::barrier(11);
            do_eval_functions(h, x.data(), &f, df.data(), E.data());                                    // :120
            second_order_step();
            int32_t status = 0;
            do_solve(h, Delta, fr ? 1 : 0, p.data(), lam.data(), mU.data(), mL.data(), ps.data(), &status);
            count_lp();
            lp_status = status; lp_fr = fr;
            if (status != ASM_OPTIMAL && status != ASM_INFEASIBLE) {                                     // :130-136 (`slp.ret == -3`: a comparison, sic)
                double fc = 0.0, v1 = 0.0;
                vec Ec(std::max<int64_t>(m, 1));
                do_eval_constraints(h, x.data(), &fc, Ec.data());
                for (int64_t i = 0; i < m; ++i) v1 += std::max(0.0, std::max(Ec[i] - h->sk->c_ub[i], h->sk->c_lb[i] - Ec[i]));
                for (int64_t j = 0; j < n; ++j) v1 += std::max(0.0, std::max(x[j] - h->sk->v_ub[j], h->sk->v_lb[j] - x[j]));
                if (v1 <= o.tol_infeas) ret = 6;
                break;
            }
            if (status == ASM_INFEASIBLE) {                                                              // :137-150
                if (fr) { ret = feasible_enough() ? 6 : 2; break; }
                fr = true;
                continue;
            }
            asmb::barrier(930);
            compute_nu();                                                                                 // :152
            double nrm[4];
            do_slp_norms(h, lam.data(), mU.data(), mL.data(), nrm);                                     // :154-156, this LP's multipliers
            prim_infeas = nrm[0]; dual_infeas = nrm[2]; compl_ = nrm[3];
            double pmax = 0.0;
            for (int64_t j = 0; j < n; ++j) pmax = std::max(pmax, std::fabs(p[j]));
            if (feasible_enough() && compl_ <= o.tol_residual && pmax <= o.tol_direction) {               // :163-175
                if (fr) { fr = false; iter += 1; continue; }
                if (dual_infeas <= o.tol_residual) { ret = 0; break; }
            }
            if (iter >= o.max_iter) { ret = feasible_enough() ? 6 : -1; break; }                         // :178-184
            asmb::barrier(940);
            const double rho = step_quality();                                                            // :187-196
            if (ret == 0 || ret == 2 || ret == 6) break;
            if (rho >= 0) {
                before_lp_step();
                for (int64_t j = 0; j < n; ++j) x[j] = x[j] + p[j];
                info.accepted += 1;
            } else {
                info.rejected += 1;
            }
            iter += 1;
        }
        finish(995, 0);
        info.delta = Delta;
    }
};

// SLP-EQP (include/asm_hip.h, "SLP-EQP"): SlpRunTR with the trust-region step on the working set of the last LP between the evaluation
// and the LP - statement by statement SlpEQP.second_order_step of activesetmethods_amd/slp.py with Parameters(device_eval=True):
// asm_eqp_trial, and asm_eval_functions again after an accepted step.  iter, lp_solves and the LP's radius are not touched.
struct SlpRunEQP : SlpRunTR {
    const asm_slp_eqp_params& e;
    asm_slp_eqp_info eq{};
    std::vector<int32_t> rs, bs;
    vec d, lam_t, mU_t, mL_t;

    SlpRunEQP(asm_handle* hh, const asm_slp_params& par, double tr_size, const asm_slp_eqp_params& ep, asm_slp_result* r)
        : SlpRunTR(hh, par, tr_size, r), e(ep), rs(std::max<int64_t>(m, 1), 0), bs(n, 0), d(n, 0.0), lam_t(std::max<int64_t>(m, 1), 0.0), mU_t(n, 0.0), mL_t(n, 0.0),
          lm(hh->lm.type == ASM_HESS_LM) {
        eq.radius = ep.radius0;
    }

    // the limited-memory Hessian's pairs, where SlpEQP of slp.py makes them: begin before each of the two updates of x (none in
    // restoration), end after the evaluation that follows, both with the multipliers current there
    const bool lm;
    void before_lp_step() override {
        if (lm && !fr) do_lm_begin(h, lam.data());
    }
    void second_order_step() override {
        if (lm) do_lm_end(h, lam.data());
        // A. outside restoration, after a normal-phase LP that ended OPTIMAL (its active set is the handle's h->sk->last)
        if (fr || lp_solves == 0 || lp_status != ASM_OPTIMAL || lp_fr || !h->sk->last.valid || !e.enabled) return;
        eq.attempts += 1;
        asm_eqp_info t;
        const std::vector<int32_t> lp_rows(h->sk->last.rowst.begin(), h->sk->last.rowst.end()), lp_bnd(h->sk->last.bst.begin(), h->sk->last.bst.end());      // (as asm_sublp_active_set)
        do_eqp_trial(h, x.data(), lam.data(), lp_rows.data(), lp_bnd.data(), eq.radius, nu.data(), e.tol_active, nullptr, d.data(), lam_t.data(), mU_t.data(),
                     mL_t.data(), rs.data(), bs.data(), &t);                                            // B to F
        if (t.skipped) {
            if (t.skipped == 1) eq.skipped_rows += 1;
            else if (t.skipped == 2) eq.skipped_dependent += 1;
            else eq.skipped_zero += 1;
            if (t.skipped != 1) eq.cg_iters += t.cg_iters;
            return;
        }
        eq.cg_iters += t.cg_iters;
        eq.boundary += t.boundary != 0;
        if (t.phi1 < t.phi0) {                                                                           // F, G
            eq.accepted += 1;
            for (int64_t i = 0; i < m; ++i) lam[i] = lam_t[i];
            if (lm) do_lm_begin(h, lam.data());
            for (int64_t j = 0; j < n; ++j) { x[j] = x[j] + d[j]; mU[j] = mU_t[j]; mL[j] = mL_t[j]; }
            if (t.boundary != 0 && t.t == 1.0) eq.radius = std::min(2.0 * eq.radius, e.radius_max);
            do_eval_functions(h, x.data(), &f, df.data(), E.data());
            if (lm) do_lm_end(h, lam.data());
        } else {
            eq.rejected += 1;
            eq.radius = 0.5 * t.norm_d;
        }
    }
};

void check_tr_size(double tr_size, const char* what) {
    if (!std::isfinite(tr_size) || !(tr_size > 0.0)) throw std::invalid_argument(std::string(what) + ": tr_size must be finite and > 0");
}
void check_eqp_params(const asm_slp_eqp_params& ep, const char* what) {
    if (!std::isfinite(ep.radius0) || !(ep.radius0 > 0.0) || !(ep.radius_max > 0.0) || !(ep.tol_active >= 0.0))
        throw std::invalid_argument(std::string(what) + ": radius0 must be finite and > 0, radius_max > 0, tol_active >= 0");
}

void slp_run_tr(asm_handle* h, const asm_slp_params* par, double tr_size, const double* x0, double* x_out, double* lambda, double* mult_x_U, double* mult_x_L,
                double* g_out, asm_slp_result* res, asm_slp_tr_info* tr) {
    if (!h->ev) throw std::logic_error("asm_slp_run_tr: asm_eval_setup first (the native driver evaluates on the device)");
    if (res) std::memset(res, 0, sizeof(*res));
    SlpRunTR r(h, *par, tr_size, res);
    r.run(x0);
    r.outputs(x_out, lambda, mult_x_U, mult_x_L, g_out);
    if (tr) *tr = r.info;
}

void slp_run_eqp(asm_handle* h, const asm_slp_params* par, double tr_size, const asm_slp_eqp_params* ep, const double* x0, double* x_out, double* lambda,
                 double* mult_x_U, double* mult_x_L, double* g_out, asm_slp_result* res, asm_slp_tr_info* tr, asm_slp_eqp_info* eq) {
    (void)kkt_hess_lm(h, "asm_slp_run_eqp");
    if (res) std::memset(res, 0, sizeof(*res));
    SlpRunEQP r(h, *par, tr_size, *ep, res);
    r.run(x0);
    r.outputs(x_out, lambda, mult_x_U, mult_x_L, g_out);
    if (tr) *tr = r.info;
    if (eq) *eq = r.eq;
}

}  // namespace

// A batch is split into groups: each group = a contiguous range of slots, one stream, one scheduler, one host thread (group 0 runs on the
// calling thread).  While one group's round executes on the device the other groups' host threads merge and launch theirs: two groups
// hide the host side of the rounds (64 case300-sized scenarios on one GPU: 23 -> 32 solves/s).
struct BatchGroup {
    struct Stream { hipStream_t s = nullptr; Stream() { HIPCHK(hipStreamCreate(&s)); } ~Stream() { (void)hipStreamDestroy(s); } } stream;
    asmb::Sched sched;              // (after the stream: it leaves first)
    const int lo, hi;               // slots [lo, hi)
    BatchGroup(int device, int lo_, int hi_, int panel_wgs, bool verbose, bool time_panels) : sched(device, stream.s, panel_wgs, verbose, time_panels), lo(lo_), hi(hi_) {}
    ~BatchGroup() { (void)hipStreamSynchronize(stream.s); }
};
struct asm_batch {
    int device = 0;
    std::vector<asm_handle*> slots;
    std::vector<std::unique_ptr<BatchGroup>> groups;
    ~asm_batch() {                  // the groups' streams drain, the slots leave, then (as members) the groups
        (void)hipSetDevice(device);
        for (auto& g : groups) (void)hipStreamSynchronize(g->stream.s);
        for (asm_handle* h : slots) (void)asm_destroy(h);
    }
    std::string err;
    std::vector<int> J_ref;         // basis columns of the null-space form every scenario starts from (first cold selection of the batch)
    std::vector<double> dpar0;      // the NLP-block data of asm_batch_eval_setup (what a scenario start restores)
    std::vector<double> scen_tab;   // per-scenario data [scen_n x scen_cnt] for dpar[scen_off, scen_off + scen_cnt) (scen_cnt = 0: none)
    int64_t scen_n = 0, scen_off = 0, scen_cnt = 0;
    std::unique_ptr<HsShared> hs;   // pattern and lists of the Hessian of the Lagrangian, one copy for every slot (asm_batch_hessian_*); dropped by
                                    // asm_batch_eval_setup
    int kkt_form = ASM_KKT_DENSE, kkt_order = ASM_KKT_ORDER_WORKING_SET;      // asm_batch_kkt_set_form; asm_batch_eval_setup starts from these
    bool setup_done = false;
    asm_batch_stats stats;
    bool verbose = false;           // ASM_BATCH_VERBOSE=1: per-kernel merge statistics of every group at release
    bool count_kernels = false;     // test entry asm_test_batch_kernel_counting: the groups keep their per-kernel merge tables
    bool time_panels = true;        // HIP events around the groups' merged panel launches (off when ASM_HIP_TIMING=0, as for a handle)
};

namespace {
// run `work(slot)` as step `step` for every slot in [0, count): the slots of a group are fibers of the group's thread, launches merged across them
template <class W>
void run_fibers(asm_batch* b, int count, const char* step, W&& work) {
    if (b->groups.empty()) throw std::logic_error(std::string(step) + ": the batch has no group (asm_batch_set_groups failed)");
    const double t0 = asmb::Sched::now_ms();
    std::vector<std::exception_ptr> errs(b->groups.size());
    auto run_group = [&](size_t k) {
        try {
            HIPCHK(hipSetDevice(b->device));
            BatchGroup& g = *b->groups[k];
            g.sched.run_range(g.lo, std::min(g.hi, count), [&work, step](int s) { in_slot(step, s, [&] { work(s); }); });
        } catch (...) {
            errs[k] = std::current_exception();
        }
    };
    std::vector<std::thread> th;
    for (size_t k = 1; k < b->groups.size(); ++k)
        if (b->groups[k]->lo < count) th.emplace_back(run_group, k);
    run_group(0);
    for (auto& t : th) t.join();
    b->stats.wall_ms += asmb::Sched::now_ms() - t0;
    asm_batch_stats& st = b->stats;
    st.rounds = st.ops = st.launches = st.releases = st.blob_bytes = 0;
    st.emit_ms = st.wait_ms = st.host_ms = 0.0;
    st.panel_ms = st.panel_flops = st.panel_bytes = 0.0;
    st.panel_launches = st.panel_ops = 0;
    st.panel_grid_max = 0;
    for (asm_handle* sh : b->slots) { st.panel_flops += sh->kstats.flops[ASM_K_PANEL_KERNEL]; st.panel_bytes += sh->kstats.bytes[ASM_K_PANEL_KERNEL]; }
    for (auto& g : b->groups) {
        const asmb::Sched& S = g->sched;
        st.panel_ms += S.res_ms; st.panel_launches += (int64_t)S.res_launches; st.panel_ops += (int64_t)S.res_ops;
        st.panel_grid_max = std::max(st.panel_grid_max, (int64_t)S.res_grid_max);
        st.rounds += (int64_t)S.n_rounds; st.ops += (int64_t)S.n_ops; st.launches += (int64_t)S.n_launches; st.releases += (int64_t)S.n_releases;
        st.blob_bytes += (int64_t)S.blob_bytes; st.emit_ms += S.t_emit_ms; st.wait_ms += S.t_wait_ms; st.host_ms += S.t_host_ms;
    }
    // a BatchError out of a scheduler is a failed round: its slots stopped half way through a solve, so the batch needs asm_batch_setup
    // again (every other failure is one slot's own, a SlotError, and the batch works on).  The first group's error is the call's
    for (auto& e : errs)
        try { if (e) std::rethrow_exception(e); } catch (const asmb::BatchError&) { b->setup_done = false; } catch (...) {}
    for (auto& e : errs)
        if (e) std::rethrow_exception(e);
}
// scenario sc's NLP-block data on slot handle h before its start: row sc of the scenario table, or the setup values.  What the slot's
// earlier work wrote outside the range about to be written is restored first, so a result never depends on what the slot solved before.
void batch_scenario_data(asm_batch* b, asm_handle* h, int64_t sc) {
    const int64_t lo = h->ev->dirty_lo, hi = h->ev->dirty_hi;
    const bool covered = b->scen_cnt > 0 && lo >= b->scen_off && hi <= b->scen_off + b->scen_cnt;
    if (hi > lo && !covered) {
        do_set_data(h, lo, hi - lo, b->dpar0.data() + lo);
        h->ev->dirty_lo = h->ev->dirty_hi = 0;
    }
    if (b->scen_cnt > 0) do_set_data(h, b->scen_off, b->scen_cnt, b->scen_tab.data() + sc * b->scen_cnt);
}
// a batch call over n_scen scenarios with a scenario table of another height
void check_scen(const asm_batch* b, int64_t n_scen, const char* what) {
    if (b->scen_cnt > 0 && n_scen != b->scen_n)
        throw std::invalid_argument(std::string(what) + ": " + std::to_string(n_scen) + " scenarios, the scenario data table has " + std::to_string(b->scen_n));
}
// body(h, sc, slot) for every scenario sc in [0, n_scen) as step `step`: the first min(n_scen, slots) slots run as fibers and take the
// scenarios in index order.  What a scenario starts with - its data, its bounds, a new merge cycle - is the body's
template <class Body>
void for_each_scenario(asm_batch* b, int64_t n_scen, const char* step, Body&& body) {
    std::atomic<int64_t> next{0};
    run_fibers(b, (int)std::min<int64_t>(n_scen, (int64_t)b->slots.size()), step, [&](int s) {
        for (;;) {
            const int64_t sc = next.fetch_add(1);
            if (sc >= n_scen) break;
            body(b->slots[s], sc, s);
        }
    });
}
// forget the shared Hessian lists: the slots that use them go back to "not prepared" (their workspaces leave with their evaluator pools)
void batch_hs_drop(asm_batch* b) {
    for (asm_handle* h : b->slots)
        if (h->ev && h->ev->hs_sh && h->ev->hs_sh == b->hs.get()) h->ev->hs_forget();
    b->hs.reset();
}
// `n_groups` groups of (almost) equal size over the slots; the slots' launches go to their group's stream
void batch_make_groups(asm_batch* b, int n_groups) {
    HIPCHK(hipSetDevice(b->device));
    const int n = (int)b->slots.size();
    n_groups = std::max(1, std::min(n_groups, n));
    // the former groups leave first, each once its stream has drained: new streams made beside them do not get the hardware queues they
    // give back, and groups that share a queue run one after the other (64 case300-sized scenarios in 3 groups: 41 -> 30 solves/s)
    b->groups.clear();
    for (asm_handle* h : b->slots) h->stream = h->stream2 = nullptr;
    std::vector<std::unique_ptr<BatchGroup>> groups;      // (all of them or none: a batch with no group refuses to run)
    for (int k = 0; k < n_groups; ++k) {
        // the all-resident panel kernels of the groups run side by side: together they must fit the chip (workgroups are dealt to the XCDs
        // round-robin and each XCD places its share on its own - a consumer can become resident before its producer, and with the chip
        // full of spinning consumers the producer never would).  The slots size their panel grids to the same share: a resident launch
        // wider than the share would go out unmerged at its full grid
        const int share = std::max(16, b->slots[0]->panel_wgs_dev / n_groups);
        groups.push_back(std::make_unique<BatchGroup>(b->device, (int)((int64_t)n * k / n_groups), (int)((int64_t)n * (k + 1) / n_groups), share, b->verbose,
                                                      b->time_panels));
    }
    b->groups.swap(groups);
    for (auto& g : b->groups) g->sched.counting = b->verbose || b->count_kernels;
    for (auto& g : b->groups)
        for (int s = g->lo; s < g->hi; ++s) { b->slots[s]->stream = g->stream.s; b->slots[s]->stream2 = g->stream.s; b->slots[s]->panel_wgs = g->sched.panel_wgs; }
}
}  // namespace

extern "C" {

int asm_slp_run(asm_handle* h, const asm_slp_params* par, const double* x0, double* x, double* lambda, double* mult_x_U, double* mult_x_L, double* g,
                asm_slp_result* res) {
    return guarded(h, [&] {
        if (!par || !x0) throw std::invalid_argument("asm_slp_run: null pointer");
        slp_run_ls(h, par, x0, x, lambda, mult_x_U, mult_x_L, g, res);
    });
}

int asm_slp_run_tr(asm_handle* h, const asm_slp_params* par, double tr_size, const double* x0, double* x, double* lambda, double* mult_x_U, double* mult_x_L,
                   double* g, asm_slp_result* res, asm_slp_tr_info* tr) {
    return guarded(h, [&] {
        if (!par || !x0) throw std::invalid_argument("asm_slp_run_tr: null pointer");
        check_tr_size(tr_size, "asm_slp_run_tr");
        slp_run_tr(h, par, tr_size, x0, x, lambda, mult_x_U, mult_x_L, g, res, tr);
    });
}

int asm_slp_run_eqp(asm_handle* h, const asm_slp_params* par, double tr_size, const asm_slp_eqp_params* eqp_par, const double* x0, double* x, double* lambda,
                    double* mult_x_U, double* mult_x_L, double* g, asm_slp_result* res, asm_slp_tr_info* tr, asm_slp_eqp_info* eqp_info) {
    return guarded(h, [&] {
        if (!par || !eqp_par || !x0) throw std::invalid_argument("asm_slp_run_eqp: null pointer");
        check_tr_size(tr_size, "asm_slp_run_eqp");
        check_eqp_params(*eqp_par, "asm_slp_run_eqp");
        slp_run_eqp(h, par, tr_size, eqp_par, x0, x, lambda, mult_x_U, mult_x_L, g, res, tr, eqp_info);
    });
}

int asm_batch_create(int device, int n_slots, asm_batch** out) {
    if (!out || n_slots < 1 || n_slots > 4096) return ASM_ERR_ARG;
    *out = nullptr;
    asm_batch* b = new (std::nothrow) asm_batch();
    if (!b) return ASM_ERR_ARG;
    b->device = device;
    std::memset(&b->stats, 0, sizeof(b->stats));
    int rc = ASM_OK;
    if (hipSetDevice(device) != hipSuccess) { delete b; return ASM_ERR_HIP; }
    for (int s = 0; s < n_slots && rc == ASM_OK; ++s) {
        asm_handle* h = nullptr;
        rc = asm_create(device, &h);
        if (rc != ASM_OK) break;
        // the slot's launches are recorded and merged onto its group's stream: no streams of its own, no look-ahead stream, no event timing
        (void)hipStreamDestroy(h->stream_ns);
        (void)hipStreamDestroy(h->stream2);
        (void)hipStreamDestroy(h->stream);
        h->stream = nullptr; h->stream2 = nullptr; h->stream_ns = nullptr;
        h->batch_slot = true;
        h->timing = 0;
        b->slots.push_back(h);
    }
    if (rc == ASM_OK) {
        try {
            // measured on 64 case300-sized scenarios, one MI355X: 1 group 23.4 solves/s, 2 groups 31.0, 3 groups 35.3, 4 groups 21.5 (the
            // all-resident panel kernels of four streams crowd each other out of the compute units)
            int ng = n_slots >= 48 ? 3 : (n_slots >= 16 ? 2 : 1);
            if (const char* e = std::getenv("ASM_BATCH_GROUPS")) ng = std::max(1, std::atoi(e));
            if (const char* v = std::getenv("ASM_BATCH_VERBOSE")) b->verbose = v[0] == '1';
            b->time_panels = b->slots[0]->knobs.timing != 0;      // ASM_HIP_TIMING as the slots read it
            batch_make_groups(b, ng);
        } catch (...) { rc = error_code(b->err); }
    }
    if (rc != ASM_OK) { delete b; return rc; }
    *out = b;
    return ASM_OK;
}

int asm_batch_destroy(asm_batch* b) {
    if (!b) return ASM_ERR_ARG;
    delete b;
    return ASM_OK;
}

int asm_batch_set_groups(asm_batch* b, int n_groups) {
    return guarded(b, [&] {
        if (n_groups < 1) throw std::invalid_argument("asm_batch_set_groups: at least one group");
        batch_make_groups(b, n_groups);
    });
}
int asm_batch_groups(const asm_batch* b) { return b ? (int)b->groups.size() : 0; }

const char* asm_batch_last_error(const asm_batch* b) { return b ? b->err.c_str() : "null batch"; }
int asm_batch_slots(const asm_batch* b) { return b ? (int)b->slots.size() : 0; }
asm_handle* asm_batch_handle(asm_batch* b, int slot) { return (b && slot >= 0 && slot < (int)b->slots.size()) ? b->slots[slot] : nullptr; }

int asm_batch_setup(asm_batch* b, int64_t n, int64_t m, int64_t nnz, const int64_t* j_row, const int64_t* j_col, const double* c_lb, const double* c_ub,
                    const double* v_lb, const double* v_ub) {
    return guarded(b, [&] {
        batch_hs_drop(b);
        b->setup_done = false;      // while it holds every slot has a skeleton: the entries read slot 0's dimensions behind it
        for (size_t s = 0; s < b->slots.size(); ++s)
            in_slot("asm_sublp_setup", (int)s, [&] { do_setup(b->slots[s], n, m, nnz, j_row, j_col, c_lb, c_ub, v_lb, v_ub); });
        b->J_ref.clear();
        b->setup_done = true;
    });
}

int asm_batch_eval_setup(asm_batch* b, int64_t n_rows, const int64_t* aff_ptr, const int64_t* aff_var, const double* aff_coef, const int64_t* quad_ptr,
                         const int64_t* q_v1, const int64_t* q_v2, const double* q_coef, const double* constant, const int64_t* jac_off, const int64_t* g_ptr,
                         const int64_t* g_kind, const double* g_coef, const int64_t* g_other, double objective_scale, int nlp_kind, int64_t nlp_rows,
                         int64_t nlp_nnz, const int64_t* nlp_ipar, int64_t n_ipar, const double* nlp_dpar, int64_t n_dpar) {
    return guarded(b, [&] {
        if (!b->setup_done) throw std::logic_error("asm_batch_eval_setup: asm_batch_setup first");
        batch_hs_drop(b);
        for (size_t s = 0; s < b->slots.size(); ++s)
            in_slot("asm_eval_setup", (int)s, [&] {
                do_eval_setup(b->slots[s], n_rows, aff_ptr, aff_var, aff_coef, quad_ptr, q_v1, q_v2, q_coef, constant, jac_off, g_ptr, g_kind, g_coef, g_other,
                              objective_scale, nlp_kind, nlp_rows, nlp_nnz, nlp_ipar, n_ipar, nlp_dpar, n_dpar);
            });
        if (n_dpar > 0) b->dpar0.assign(nlp_dpar, nlp_dpar + n_dpar);
        else b->dpar0.clear();
        b->scen_tab.clear();
        b->scen_n = b->scen_off = b->scen_cnt = 0;
        b->kkt_form = ASM_KKT_DENSE;
        b->kkt_order = ASM_KKT_ORDER_WORKING_SET;
    });
}

int asm_batch_kkt_set_form(asm_batch* b, int32_t form, int32_t order) {
    return guarded(b, [&] {
        if (!b->setup_done || !b->slots[0]->ev) throw std::logic_error("asm_batch_kkt_set_form: asm_batch_eval_setup first");
        if ((form != ASM_KKT_DENSE && form != ASM_KKT_SPARSE) || (order != ASM_KKT_ORDER_WORKING_SET && order != ASM_KKT_ORDER_STATIC))
            throw std::invalid_argument("asm_batch_kkt_set_form: form is neither ASM_KKT_DENSE nor ASM_KKT_SPARSE, or order neither ASM_KKT_ORDER_WORKING_SET nor ASM_KKT_ORDER_STATIC");
        if (form == ASM_KKT_SPARSE && order != ASM_KKT_ORDER_STATIC)
            throw std::invalid_argument("asm_batch_kkt_set_form: the sparse form in the working-set order is per handle - it orders the rows on the host, uploads "
                                        "and synchronises at every new working set, which a round of the batch cannot; use ASM_KKT_ORDER_STATIC");
        b->kkt_form = form;
        b->kkt_order = order;
    });
}

int asm_batch_set_scenario_data(asm_batch* b, int64_t n_scen, int64_t offset, int64_t count, const double* table) {
    return guarded(b, [&] {
        if (!b->setup_done || !b->slots[0]->ev) throw std::logic_error("asm_batch_set_scenario_data: asm_batch_eval_setup first");
        if (count == 0) {
            b->scen_tab.clear();
            b->scen_n = b->scen_off = b->scen_cnt = 0;
            return;
        }
        const int64_t nd = (int64_t)b->dpar0.size();
        if (!table || n_scen < 1 || count < 0 || offset < 0 || offset > nd - count)
            throw std::invalid_argument("asm_batch_set_scenario_data: null table, no scenario or a range outside [0, n_dpar = " + std::to_string(nd) + ")");
        b->scen_tab.assign(table, table + n_scen * count);
        b->scen_n = n_scen; b->scen_off = offset; b->scen_cnt = count;
    });
}

int asm_batch_set_ns_basis(asm_batch* b, const int32_t* J, int64_t k) {
    return guarded(b, [&] {
        if (k < 0 || (k > 0 && !J)) throw std::invalid_argument("asm_batch_set_ns_basis: bad argument");
        if (!b->setup_done) throw std::logic_error("asm_batch_set_ns_basis: asm_batch_setup first");
        for (size_t s = 0; s < b->slots.size(); ++s) in_slot("asm_sublp_set_ns_basis", (int)s, [&] { do_set_ns_basis(b->slots[s], J, k); });
        b->J_ref.assign(J, J + k);
    });
}

// `count` LPs in lockstep, one per slot: asm_sublp_solve with a leading scenario dimension on every array
int asm_batch_sublp_solve(asm_batch* b, int count, const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub, const double* dE,
                          const double* df, const double* f, const double* E, const double* x_k, const double* delta, const int32_t* feasibility, double* p,
                          double* lambda, double* mult_x_U, double* mult_x_L, double* p_slack, int32_t* status) {
    return guarded(b, [&] {
        if (!b->setup_done) throw std::logic_error("asm_batch_sublp_solve: asm_batch_setup first");
        if (count < 1 || count > (int)b->slots.size() || !dE || !df || !f || !x_k || !delta || !feasibility || !p || !mult_x_U || !mult_x_L || !status)
            throw std::invalid_argument("asm_batch_sublp_solve: bad count or null pointer");
        const int64_t n = b->slots[0]->sk->n, m = b->slots[0]->sk->m, nnz = b->slots[0]->sk->nnz;
        if (m > 0 && (!E || !lambda || !p_slack)) throw std::invalid_argument("asm_batch_sublp_solve: null pointer");
        check_scen(b, count, "asm_batch_sublp_solve");
        HIPCHK(hipSetDevice(b->device));
        run_fibers(b, count, "asm_sublp_solve", [&](int s) {
            asm_handle* h = b->slots[s];
            if (c_lb && c_ub && v_lb && v_ub) do_set_bounds(h, c_lb + s * m, c_ub + s * m, v_lb + s * n, v_ub + s * n);
            if (h->ev) batch_scenario_data(b, h, s);
            asmb::next_cycle();
            do_upload(h, dE + s * nnz, df + s * n, f[s], E ? E + s * m : nullptr, x_k + s * n);
            do_solve(h, delta[s], feasibility[s], p + s * n, lambda ? lambda + s * m : nullptr, mult_x_U + s * n, mult_x_L + s * n,
                     p_slack ? p_slack + s * 2 * m : nullptr, status + s);
        });
    });
}

}  // extern "C"

namespace {
// n_scen complete SLP runs of one algorithm: the slots' fibers take the scenarios in index order; every array has a leading scenario dimension.
// run_one(h, sc) solves scenario sc on handle h (bounds and basis columns already set).
template <class RunOne>
void batch_slp_runs(asm_batch* b, const char* step, int64_t n_scen, const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub,
                    const double* x0, asm_slp_result* res, RunOne&& run_one) {
    const int64_t n = b->slots[0]->sk->n, m = b->slots[0]->sk->m;
    HIPCHK(hipSetDevice(b->device));
    if (b->J_ref.empty()) {
        // reference selection of the null-space basis columns: one LP of scenario 0 at its start point on slot 0 (cold selection); EVERY
        // scenario, 0 included, then starts from these columns - the results do not depend on the slot or on what it solved before
        asm_handle* h0 = b->slots[0];
        in_slot(step, 0, [&] {
            do_set_bounds(h0, c_lb, c_ub, v_lb, v_ub);
            batch_scenario_data(b, h0, 0);
            h0->sk->hint[0].ns_J.clear();
            vec xs(n), dfs(n), Es(std::max<int64_t>(m, 1)), pp(n), ll(std::max<int64_t>(m, 1)), uu(n), lo(n), sl(2 * std::max<int64_t>(m, 1));
            clamp_start(n, x0, v_lb, v_ub, xs.data());
            double f0 = 0.0;
            int32_t st0 = 0;
            do_eval_functions(h0, xs.data(), &f0, dfs.data(), Es.data());
            do_solve(h0, 1000.0, 0, pp.data(), ll.data(), uu.data(), lo.data(), sl.data(), &st0);
        });
        b->J_ref = h0->sk->hint[0].ns_J;
    }
    for_each_scenario(b, n_scen, step, [&](asm_handle* h, int64_t sc, int s) {
        do_set_bounds(h, c_lb + sc * m, c_ub + sc * m, v_lb + sc * n, v_ub + sc * n);
        batch_scenario_data(b, h, sc);
        // every scenario starts from the batch's reference basis columns (results do not depend on which slot solved what before)
        if (!b->J_ref.empty()) h->sk->hint[0].ns_J = b->J_ref;
        else h->sk->hint[0].ns_J.clear();
        run_one(h, sc);
        res[sc].slot = s;
    });
}
}  // namespace

extern "C" {

// n_scen complete SLP runs (Line Search)
int asm_batch_slp_run(asm_batch* b, int64_t n_scen, const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub, const double* x0,
                      const asm_slp_params* par, double* x, double* lambda, double* mult_x_U, double* mult_x_L, double* g, asm_slp_result* res) {
    return guarded(b, [&] {
        if (!b->setup_done) throw std::logic_error("asm_batch_slp_run: asm_batch_setup first");
        if (n_scen < 1 || !c_lb || !c_ub || !v_lb || !v_ub || !x0 || !par || !res) throw std::invalid_argument("asm_batch_slp_run: bad argument");
        check_scen(b, n_scen, "asm_batch_slp_run");
        const int64_t n = b->slots[0]->sk->n, m = b->slots[0]->sk->m;
        batch_slp_runs(b, "asm_slp_run", n_scen, c_lb, c_ub, v_lb, v_ub, x0, res, [&](asm_handle* h, int64_t sc) {
            slp_run_ls(h, par, x0 + sc * n, x ? x + sc * n : nullptr, lambda ? lambda + sc * m : nullptr, mult_x_U ? mult_x_U + sc * n : nullptr,
                       mult_x_L ? mult_x_L + sc * n : nullptr, g ? g + sc * m : nullptr, res + sc);
        });
    });
}

// n_scen complete SLP runs (Trust Region)
int asm_batch_slp_run_tr(asm_batch* b, int64_t n_scen, const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub, const double* x0,
                         const asm_slp_params* par, double tr_size, double* x, double* lambda, double* mult_x_U, double* mult_x_L, double* g,
                         asm_slp_result* res, asm_slp_tr_info* tr) {
    return guarded(b, [&] {
        if (!b->setup_done) throw std::logic_error("asm_batch_slp_run_tr: asm_batch_setup first");
        if (n_scen < 1 || !c_lb || !c_ub || !v_lb || !v_ub || !x0 || !par || !res) throw std::invalid_argument("asm_batch_slp_run_tr: bad argument");
        check_tr_size(tr_size, "asm_batch_slp_run_tr");
        check_scen(b, n_scen, "asm_batch_slp_run_tr");
        const int64_t n = b->slots[0]->sk->n, m = b->slots[0]->sk->m;
        batch_slp_runs(b, "asm_slp_run_tr", n_scen, c_lb, c_ub, v_lb, v_ub, x0, res, [&](asm_handle* h, int64_t sc) {
            slp_run_tr(h, par, tr_size, x0 + sc * n, x ? x + sc * n : nullptr, lambda ? lambda + sc * m : nullptr, mult_x_U ? mult_x_U + sc * n : nullptr,
                       mult_x_L ? mult_x_L + sc * n : nullptr, g ? g + sc * m : nullptr, res + sc, tr ? tr + sc : nullptr);
        });
    });
}

// asm_eval_data_gradient of n_scen scenarios (each with its data, as asm_batch_slp_run gives it), the slots taking them in index order
int asm_batch_data_gradient(asm_batch* b, int64_t n_scen, const double* x, const double* lambda, double* out) {
    return guarded(b, [&] {
        if (!b->setup_done || !b->slots[0]->ev) throw std::logic_error("asm_batch_data_gradient: asm_batch_eval_setup first");
        data_kind_check(*b->slots[0]->ev, "asm_batch_data_gradient", "data gradients");
        const int64_t n = b->slots[0]->sk->n, m = b->slots[0]->sk->m, nd = (int64_t)b->dpar0.size();
        if (n_scen < 1 || !x || (m > 0 && !lambda) || (nd > 0 && !out)) throw std::invalid_argument("asm_batch_data_gradient: bad argument");
        check_scen(b, n_scen, "asm_batch_data_gradient");
        HIPCHK(hipSetDevice(b->device));
        for_each_scenario(b, n_scen, "asm_eval_data_gradient", [&](asm_handle* h, int64_t sc, int) {
            batch_scenario_data(b, h, sc);
            asmb::next_cycle();
            do_data_gradient(h, x + sc * n, m > 0 ? lambda + sc * m : nullptr, out + sc * nd);
        });
    });
}

}  // extern "C"

namespace {
// what every asm_batch_hessian_* entry starts with: state and kind checks, then the shared pattern and lists - built once per
// asm_batch_eval_setup from slot 0's store and tape, on the calling thread (the build downloads with blocking copies)
void batch_hs_prepare(asm_batch* b, const char* who) {
    if (!b->setup_done || !b->slots[0]->ev) throw std::logic_error(std::string(who) + ": asm_batch_eval_setup first");
    hs_check(b->slots[0], who);
    if (b->hs) return;
    auto sh = std::make_unique<HsShared>();
    hs_build(b->slots[0], *sh);
    b->hs = std::move(sh);
}
// what the SLP-EQP step allocates or builds at its first call on a handle, for the first `count` slots and on the calling thread, before
// their fibers start: the Hessian workspace on the batch's shared lists, the KKT buffers, the one-column work area and the trial's
// state.  hipMalloc and the clearing fills stay out of the rounds; a slot that has them keeps them (until the next batch set-up).
// Every slot gets the batch's form and order (asm_batch_kkt_set_form) and what that form needs, nothing of the other.  The dense fallback
// of the sparse form is decided here, on slot 0, for all slots (they share the pattern): no sparse pattern, or one that rcm_order
// declines.  What a slot then holds besides the shared factor (ld^2 doubles, ld = min(m, n) rounded up) and the one-column work area, with
// ldn, Mp, ldT the padded n, m, min(m, n):
//   dense    (Mp ldn + min(m, n) ldn + ldn ldT) doubles: J, A and its transposed copy (asm_kkt_form_info: dense_bytes)
//   sparse   nnz doubles + (M + 2 pairs) ints: the CSR values, the position list, the row-index pairs of all rows (sparse_bytes), and on
//            the host the order of all rows (m ints), the pairs again and the cache of the last working set (3 m ints)
// The multi entries (asm_batch_kkt_solve and the two sensitivity entries, cap = KKM_CW) come here too: the work area of 64 columns
// - 14 ldn + 5 ldT + Mp doubles per column, the transposed factor (ld^2) and, dense form, the unmasked transposed working rows (ldn ldT) -
// instead of the one-column area and the trial's state, and with `cross` what the cross-derivative sweep of the slot's kind needs
// (cx_prepare downloads with blocking copies), under the conditions kkt_stage_rhs reads it for KktRhs::data; with `cross_t` the workspace of the transposed
// sweep (asm_batch_solution_adjoint), under the conditions ct_columns reads it.
void batch_kkt_prepare(asm_batch* b, int count, const char* step = "asm_slp_run_eqp", int64_t cap = 1, bool cross = false, bool cross_t = false) {
    bool sparse = b->kkt_form == ASM_KKT_SPARSE && b->slots[0]->sk->sp_ok;
    for (int s = 0; s < count; ++s)
        in_slot(step, s, [&] {
            asm_handle* h = b->slots[s];
            if (!h->ev->hs_sh) hs_attach(h, b->hs.get());
            h->ev->kk.form = b->kkt_form;
            h->ev->kk.order = b->kkt_order;
            sparse = sparse && kk_sparse(h);
            if (sparse) kk_pairs(h, ASM_KKT_ORDER_STATIC);
            else kk_dense(h);
            (void)kk_work(h, cap, sparse);
            if (cap == 1) eq_prepare(h);
            EvalState& e = *h->ev;
            if (!e.data_dep) return;       // (what kkt_stage_rhs and ct_columns ask before they read either workspace)
            HIPCHK(hipSetDevice(h->device));
            if (cross) cx_prepare(e, KKM_CW);
            if (cross_t) ct_prepare(e, KKM_CW);
        });
}
// The four multi entries on n_scen scenarios, the slots taking them in index order (for_each_scenario): per scenario do_kkt_solve_multi
// under the per-handle entry's name `step`, on the scenario's part of the point, of the columns `rhs` and of the outputs (KktPoint::at,
// KktRhs::at with dc_stride, KktOut::at) and with its data.  Everything that can be refused without a launch is refused here, on the
// calling thread - the arguments by the per-handle entry's own kkt_check_args under the batch entry's name `who` - and what a slot
// allocates or builds at its first call is made before the fibers start (batch_kkt_prepare).
void batch_kkt_multi(asm_batch* b, const char* who, const char* step, int64_t n_scen, const KktPoint& p, int32_t nrhs, const KktRhs& rhs, int64_t dc_stride,
                     const asm_kkt_params* par, const KktOut& out, asm_kkt_info* info) {
    const std::string me(who);
    const bool data = rhs.kind == KktRhs::DATA;
    // a model without second derivatives ends here, as in asm_batch_hessian_*, one without cross derivatives as in the per-handle entry
    batch_hs_prepare(b, who);
    if (data) cx_check(b->slots[0], who);
    const int64_t n = b->slots[0]->sk->n, m = b->slots[0]->sk->m, nd = (int64_t)b->dpar0.size();
    if (n_scen < 1 || nrhs < 1) throw std::invalid_argument(me + ": n_scen < 1 or nrhs < 1");
    kkt_check_args(me, m, nd, nrhs, p, rhs, &out, info, n);
    if (par && (par->max_iter < 0 || !(par->rtol >= 0.0))) throw std::invalid_argument(me + ": max_iter < 0 or rtol not >= 0");
    check_scen(b, n_scen, who);
    HIPCHK(hipSetDevice(b->device));
    batch_kkt_prepare(b, (int)std::min<int64_t>(n_scen, (int64_t)b->slots.size()), step, KKM_CW, data);
    for_each_scenario(b, n_scen, step, [&](asm_handle* h, int64_t sc, int) {
        batch_scenario_data(b, h, sc);
        asmb::next_cycle();
        const int64_t o = sc * nrhs;
        do_kkt_solve_multi(h, step, p.at(sc, n, m), nrhs, rhs.at(sc, nrhs, n, m, dc_stride), par, out.at(o, n, m), info + o);
    });
}
// asm_solution_adjoint_multi on n_scen scenarios, the slots taking them in index order: the checks as in batch_kkt_multi, the set-up of
// the adjoint entries (AdjointSetup) for the functions of all scenarios, the workspaces before the fibers start
// z: asm_batch_solution_adjoint_z - asm_solution_adjoint_z_multi per scenario, with the weights GZ (may be absent) and the variable-bound
// gradients DXBOUND; what a slot needs for the weights (kk_gz) is made before the fibers start, too
void batch_adjoint(asm_batch* b, int64_t n_scen, const KktPoint& p, int32_t nrhs, const double* GX, const double* GL, const asm_kkt_params* par, double* OUT,
                   double* DBOUND, double* AX, double* AL, asm_kkt_info* info, bool z = false, const double* GZ = nullptr, double* DXBOUND = nullptr) {
    const char *who = z ? "asm_batch_solution_adjoint_z" : "asm_batch_solution_adjoint", *step = z ? "asm_solution_adjoint_z_multi" : "asm_solution_adjoint_multi";
    const std::string me(who);
    batch_hs_prepare(b, who);
    adjoint_check(b->slots[0], who);
    const int64_t n = b->slots[0]->sk->n, m = b->slots[0]->sk->m, nd = b->slots[0]->ev->n_dpar;
    if (n_scen < 1 || nrhs < 1) throw std::invalid_argument(me + ": n_scen < 1 or nrhs < 1");
    adjoint_check_args(me, m, nd, nrhs, p, GX, GL, OUT, info);
    if (par && (par->max_iter < 0 || !(par->rtol >= 0.0))) throw std::invalid_argument(me + ": max_iter < 0 or rtol not >= 0");
    check_scen(b, n_scen, who);
    HIPCHK(hipSetDevice(b->device));
    const AdjointSetup A(n_scen * nrhs, n, m, GX, AX, AL);
    const KktRhs rhs = KktRhs::given(A.ru.data(), GL).with_gz(GZ);
    const int count = (int)std::min<int64_t>(n_scen, (int64_t)b->slots.size());
    batch_kkt_prepare(b, count, step, KKM_CW, false, true);
    for (int s = 0; GZ && s < count; ++s) in_slot(step, s, [&] { kk_gz(b->slots[s]); });
    for_each_scenario(b, n_scen, step, [&](asm_handle* h, int64_t sc, int) {
        batch_scenario_data(b, h, sc);
        asmb::next_cycle();
        const int64_t o = sc * nrhs;
        if (z)
            adjoint_z_multi(h, step, KKM_CW, p.at(sc, n, m), nrhs, rhs.at(sc, nrhs, n, m, 0), par, OUT + o * nd, DBOUND ? DBOUND + o * m : nullptr,
                            DXBOUND ? DXBOUND + o * n : nullptr, A.state.at(o, n, m), info + o);
        else
            adjoint_multi(h, step, KKM_CW, p.at(sc, n, m), nrhs, rhs.at(sc, nrhs, n, m, 0), par, OUT + o * nd, DBOUND ? DBOUND + o * m : nullptr, A.state.at(o, n, m), info + o);
    });
}
// asm_eval_hessian_lagrangian (v == nullptr: values [n_scen x nnz] into out) or asm_eval_hessian_product (out [n_scen x n]) of n_scen
// scenarios, each with its data, the slots taking them in index order.  A slot attaches its workspace to the shared lists when it takes
// its first scenario (a slot that a per-handle call prepared keeps its own lists: same pattern, same bits)
void batch_hessians(asm_batch* b, const char* who, int64_t n_scen, const double* x, const double* obj_factor, const double* lambda, const double* v,
                    double* out) {
    const int64_t n = b->slots[0]->sk->n, m = b->slots[0]->sk->m, nnz = b->hs->nnz(), len = v ? n : nnz;
    check_scen(b, n_scen, who);
    HIPCHK(hipSetDevice(b->device));
    for_each_scenario(b, n_scen, v ? "asm_eval_hessian_product" : "asm_eval_hessian_lagrangian", [&](asm_handle* h, int64_t sc, int) {
        if (!h->ev->hs_sh) hs_attach(h, b->hs.get());
        batch_scenario_data(b, h, sc);
        asmb::next_cycle();
        hs_launch(h, x + sc * n, obj_factor ? obj_factor[sc] : 1.0, m > 0 ? lambda + sc * m : nullptr, v ? v + sc * n : nullptr);
        hs_read(h, v ? h->ev->d_hs_out : h->ev->d_hs_vals, len, out + sc * len);
    });
}
}  // namespace

extern "C" {

int asm_batch_hessian_structure(asm_batch* b, int64_t* nnz, int64_t* rows, int64_t* cols) {
    return guarded(b, [&] {
        batch_hs_prepare(b, "asm_batch_hessian_structure");
        if (!nnz || (rows == nullptr) != (cols == nullptr)) throw std::invalid_argument("asm_batch_hessian_structure: null pointer");
        hs_pattern(*b->hs, nnz, rows, cols);
    });
}

int asm_batch_hessian_lagrangian(asm_batch* b, int64_t n_scen, const double* x, const double* obj_factor, const double* lambda, double* values) {
    return guarded(b, [&] {
        batch_hs_prepare(b, "asm_batch_hessian_lagrangian");
        if (n_scen < 1 || !x || (b->slots[0]->sk->m > 0 && !lambda) || (b->hs->nnz() > 0 && !values))
            throw std::invalid_argument("asm_batch_hessian_lagrangian: no scenario or a null pointer");
        batch_hessians(b, "asm_batch_hessian_lagrangian", n_scen, x, obj_factor, lambda, nullptr, values);
    });
}

int asm_batch_hessian_product(asm_batch* b, int64_t n_scen, const double* x, const double* obj_factor, const double* lambda, const double* v, double* out) {
    return guarded(b, [&] {
        batch_hs_prepare(b, "asm_batch_hessian_product");
        if (n_scen < 1 || !x || !v || !out || (b->slots[0]->sk->m > 0 && !lambda)) throw std::invalid_argument("asm_batch_hessian_product: no scenario or a null pointer");
        batch_hessians(b, "asm_batch_hessian_product", n_scen, x, obj_factor, lambda, v, out);
    });
}

// n_scen complete SLP runs (SLP-EQP): asm_slp_run_eqp per scenario, the KKT solves and trial steps of the slots merged like their LPs
int asm_batch_slp_run_eqp(asm_batch* b, int64_t n_scen, const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub, const double* x0,
                          const asm_slp_params* par, double tr_size, const asm_slp_eqp_params* eqp_par, double* x, double* lambda, double* mult_x_U,
                          double* mult_x_L, double* g, asm_slp_result* res, asm_slp_tr_info* tr, asm_slp_eqp_info* eqp_info) {
    return guarded(b, [&] {
        if (!b->setup_done) throw std::logic_error("asm_batch_slp_run_eqp: asm_batch_setup first");
        if (n_scen < 1 || !c_lb || !c_ub || !v_lb || !v_ub || !x0 || !par || !eqp_par || !res) throw std::invalid_argument("asm_batch_slp_run_eqp: bad argument");
        check_tr_size(tr_size, "asm_batch_slp_run_eqp");
        check_eqp_params(*eqp_par, "asm_batch_slp_run_eqp");
        check_scen(b, n_scen, "asm_batch_slp_run_eqp");
        // a model without second derivatives ends here, as in asm_slp_run_eqp, before any fiber starts; the lists are the batch's
        batch_hs_prepare(b, "asm_batch_slp_run_eqp");
        HIPCHK(hipSetDevice(b->device));
        if (eqp_par->enabled) batch_kkt_prepare(b, (int)std::min<int64_t>(n_scen, (int64_t)b->slots.size()));
        const int64_t n = b->slots[0]->sk->n, m = b->slots[0]->sk->m;
        // (asm_sublp_set_bounds at every scenario start forgets the slot's retained active sets and hints: no history for the step to read)
        batch_slp_runs(b, "asm_slp_run_eqp", n_scen, c_lb, c_ub, v_lb, v_ub, x0, res, [&](asm_handle* h, int64_t sc) {
            slp_run_eqp(h, par, tr_size, eqp_par, x0 + sc * n, x ? x + sc * n : nullptr, lambda ? lambda + sc * m : nullptr, mult_x_U ? mult_x_U + sc * n : nullptr,
                        mult_x_L ? mult_x_L + sc * n : nullptr, g ? g + sc * m : nullptr, res + sc, tr ? tr + sc : nullptr, eqp_info ? eqp_info + sc : nullptr);
        });
    });
}

// asm_kkt_solve_multi, asm_solution_sensitivity_multi, asm_bound_sensitivity_multi and asm_var_bound_sensitivity_multi of n_scen scenarios (include/asm_hip.h, "Scenario
// batches: KKT solves and sensitivities")
int asm_batch_kkt_solve(asm_batch* b, int64_t n_scen, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs,
                        const double* RU, const double* RW, const asm_kkt_params* par, double* DX, double* DLAM, double* DZ, asm_kkt_info* info) {
    return guarded(b, [&] {
        batch_kkt_multi(b, "asm_batch_kkt_solve", "asm_kkt_solve_multi", n_scen, {x, lambda, row_state, bound_state}, nrhs, KktRhs::given(RU, RW), 0, par, {DX, DLAM, DZ}, info);
    });
}

int asm_batch_solution_sensitivity(asm_batch* b, int64_t n_scen, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs,
                                   const double* DC, int32_t dc_per_scenario, const asm_kkt_params* par, double* DX, double* DLAM, double* DZ, asm_kkt_info* info) {
    return guarded(b, [&] {
        if (dc_per_scenario != 0 && dc_per_scenario != 1) throw std::invalid_argument("asm_batch_solution_sensitivity: dc_per_scenario is neither 0 nor 1");
        const int64_t stride = dc_per_scenario ? (int64_t)std::max<int32_t>(nrhs, 0) * (int64_t)b->dpar0.size() : 0;
        batch_kkt_multi(b, "asm_batch_solution_sensitivity", "asm_solution_sensitivity_multi", n_scen, {x, lambda, row_state, bound_state}, nrhs, KktRhs::data(DC), stride, par,
                        {DX, DLAM, DZ}, info);
    });
}

int asm_batch_solution_adjoint(asm_batch* b, int64_t n_scen, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs,
                               const double* GX, const double* GL, const asm_kkt_params* par, double* OUT, double* DBOUND, double* AX, double* AL, asm_kkt_info* info) {
    return guarded(b, [&] { batch_adjoint(b, n_scen, {x, lambda, row_state, bound_state}, nrhs, GX, GL, par, OUT, DBOUND, AX, AL, info); });
}

int asm_batch_solution_adjoint_z(asm_batch* b, int64_t n_scen, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs,
                                 const double* GX, const double* GL, const double* GZ, const asm_kkt_params* par, double* OUT, double* DBOUND, double* DXBOUND, double* AX,
                                 double* AL, asm_kkt_info* info) {
    return guarded(b, [&] { batch_adjoint(b, n_scen, {x, lambda, row_state, bound_state}, nrhs, GX, GL, par, OUT, DBOUND, AX, AL, info, true, GZ, DXBOUND); });
}

// asm_sensitivity_range_multi of n_scen scenarios, each with its bounds (as asm_batch_slp_run takes them) and its data, the slots taking them
// in index order.  Everything that can be refused without a launch is refused here, on the calling thread, by the per-handle entry's own
// rg_check_args; what a slot allocates at its first call is made before the fibers start (rg_prepare).
int asm_batch_sensitivity_range(asm_batch* b, int64_t n_scen, const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub, const double* x,
                                const double* lambda, const double* z, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs, const double* DX,
                                const double* DLAM, const double* DZ, asm_range_info* out) {
    return guarded(b, [&] {
        const char *who = "asm_batch_sensitivity_range", *step = "asm_sensitivity_range_multi";
        const std::string me(who);
        if (!b->setup_done || !b->slots[0]->ev) throw std::logic_error(me + ": asm_batch_eval_setup first");
        const int64_t n = b->slots[0]->sk->n, m = b->slots[0]->sk->m;
        if (n_scen < 1) throw std::invalid_argument(me + ": n_scen < 1");
        if (!v_lb || !v_ub || (m > 0 && (!c_lb || !c_ub))) throw std::invalid_argument(me + ": null pointer");
        rg_check_args(me, n, m, n_scen, x, lambda, z, row_state, bound_state, nrhs, DX, DLAM, DZ, out);
        check_scen(b, n_scen, who);
        HIPCHK(hipSetDevice(b->device));
        const int count = (int)std::min<int64_t>(n_scen, (int64_t)b->slots.size());
        for (int s = 0; s < count; ++s) in_slot(step, s, [&] { rg_prepare(b->slots[s]); });
        for_each_scenario(b, n_scen, step, [&](asm_handle* h, int64_t sc, int) {
            do_set_bounds(h, m > 0 ? c_lb + sc * m : nullptr, m > 0 ? c_ub + sc * m : nullptr, v_lb + sc * n, v_ub + sc * n);
            batch_scenario_data(b, h, sc);
            asmb::next_cycle();
            const int64_t o = sc * nrhs;
            rg_run(h, x + sc * n, m > 0 ? lambda + sc * m : nullptr, z + sc * n, m > 0 ? row_state + sc * m : nullptr, bound_state + sc * n, nrhs, DX + o * n,
                   m > 0 ? DLAM + o * m : nullptr, DZ + o * n, out + o);
        });
    });
}

int asm_batch_var_bound_sensitivity(asm_batch* b, int64_t n_scen, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs,
                                    const int32_t* vars, const double* delta, const asm_kkt_params* par, double* DX, double* DLAM, double* DZ, asm_kkt_info* info) {
    return guarded(b, [&] {
        batch_kkt_multi(b, "asm_batch_var_bound_sensitivity", "asm_var_bound_sensitivity_multi", n_scen, {x, lambda, row_state, bound_state}, nrhs,
                        KktRhs::var_bound(vars, delta), 0, par, {DX, DLAM, DZ}, info);
    });
}

int asm_batch_bound_sensitivity(asm_batch* b, int64_t n_scen, const double* x, const double* lambda, const int32_t* row_state, const int32_t* bound_state, int32_t nrhs,
                                const int32_t* rows, const double* delta, const asm_kkt_params* par, double* DX, double* DLAM, double* DZ, asm_kkt_info* info) {
    return guarded(b, [&] {
        batch_kkt_multi(b, "asm_batch_bound_sensitivity", "asm_bound_sensitivity_multi", n_scen, {x, lambda, row_state, bound_state}, nrhs, KktRhs::bound(rows, delta), 0, par,
                        {DX, DLAM, DZ}, info);
    });
}

int asm_batch_ns_basis(const asm_batch* b, int32_t* J, int64_t* k) {
    if (!b || !k) return ASM_ERR_ARG;
    *k = (int64_t)b->J_ref.size();
    if (J) for (size_t a = 0; a < b->J_ref.size(); ++a) J[a] = b->J_ref[a];
    return ASM_OK;
}

int asm_batch_get_stats(const asm_batch* b, asm_batch_stats* out) {
    if (!b || !out) return ASM_ERR_ARG;
    *out = b->stats;
    return ASM_OK;
}

}  // extern "C"

namespace {
// one family of asm_batch_test_run: the record's size and the hook's internal function on record `sc` of the caller's array
struct TestFamily { int64_t size; int (*run)(asm_handle*, const void* records, int64_t sc); };
template <class Rec, int (*Fn)(asm_handle*, const Rec&)>
constexpr TestFamily test_family() {
    return {(int64_t)sizeof(Rec), [](asm_handle* h, const void* records, int64_t sc) { return Fn(h, static_cast<const Rec*>(records)[sc]); }};
}
const TestFamily TEST_FAMILIES[ASM_TF_COUNT] = {      // in the order of the ASM_TF_* numbers
    test_family<asm_test_skeleton_stages_args, test_skeleton_stages>(), test_family<asm_test_ipm_stages_args, test_ipm_stages>(),
    test_family<asm_test_as_stages_args, test_as_stages>(), test_family<asm_test_ns_stages_args, test_ns_stages>(),
    test_family<asm_test_ns_setup_stages_args, test_ns_setup_stages>(), test_family<asm_test_kkt_stages_args, test_kkt_stages>(),
    test_family<asm_test_cholesky_args, test_cholesky>(), test_family<asm_test_chol_solve_args, test_chol_solve>(),
    test_family<asm_test_trsm_rows_args, test_trsm_rows>(), test_family<asm_test_gemm_nt_args, test_gemm_nt>(), test_family<asm_test_gemv_args, test_gemv>(),
    test_family<asm_test_syrk_args, test_syrk>(), test_family<asm_test_syrk_update_args, test_syrk_update>(),
    test_family<asm_test_build_split_args, test_build_split>(), test_family<asm_test_copy_fill_args, test_copy_fill>(),
};
}  // namespace

extern "C" {

int64_t asm_batch_test_record_size(int32_t family) { return family >= 0 && family < ASM_TF_COUNT ? TEST_FAMILIES[family].size : -1; }

int asm_batch_test_run(asm_batch* b, int32_t family, int64_t n_scen, const void* records, int32_t* status_out) {
    return guarded(b, [&] {
        if (family < 0 || family >= ASM_TF_COUNT || n_scen < 1 || !records || !status_out) throw std::invalid_argument("asm_batch_test_run: bad argument");
        HIPCHK(hipSetDevice(b->device));
        const TestFamily& F = TEST_FAMILIES[family];
        for_each_scenario(b, n_scen, "asm_batch_test_run", [&](asm_handle* h, int64_t sc, int) {
            asmb::next_cycle();
            status_out[sc] = F.run(h, records, sc);      // (the hook's own failure is the scenario's status; a cancelled fiber unwinds through it)
        });
    });
}

int asm_test_batch_panel_share(const asm_batch* b, int group) {
    return (b && group >= 0 && group < (int)b->groups.size()) ? b->groups[group]->sched.panel_wgs : -1;
}

int asm_test_batch_kernel_counting(asm_batch* b, int on) {
    return guarded(b, [&] {
        b->count_kernels = on != 0;
        for (auto& g : b->groups) { g->sched.counting = b->count_kernels || b->verbose; g->sched.per_kernel.clear(); }
    });
}

int asm_test_batch_kernel_table(asm_batch* b, asm_batch_kernel_row* rows, int64_t cap, int64_t* n_rows, int reset) {
    return guarded(b, [&] {
        if (!n_rows || cap < 0 || (cap > 0 && !rows)) throw std::invalid_argument("asm_test_batch_kernel_table: bad argument");
        std::map<std::pair<const void*, unsigned>, asmb::Sched::KernelCount> sum;
        for (auto& g : b->groups)
            for (auto& kv : g->sched.per_kernel) {
                asmb::Sched::KernelCount& c = sum[kv.first];
                c.ops += kv.second.ops; c.launches += kv.second.launches; c.nb_max = std::max(c.nb_max, kv.second.nb_max);
            }
        *n_rows = (int64_t)sum.size();
        int64_t i = 0;
        HIPCHK(hipSetDevice(b->device));
        for (auto& kv : sum) {
            if (i >= cap) break;
            asm_batch_kernel_row& r = rows[i++];
            const char* nm = hipKernelNameRefByPtr(kv.first.first, b->groups.empty() ? nullptr : b->groups[0]->stream.s);
            std::snprintf(r.name, sizeof(r.name), "%s", nm ? nm : "?");
            r.operations = (int64_t)kv.second.ops; r.launches = (int64_t)kv.second.launches;
            r.nb_max = (int32_t)kv.second.nb_max; r.gz = (int32_t)kv.first.second;
        }
        if (reset)
            for (auto& g : b->groups) g->sched.per_kernel.clear();
    });
}

}  // extern "C"

#ifdef ASM_UPD_PROF
extern "C" int asm_debug_upd_prof(unsigned long long* out8) {       // diagnostic build only: read and clear the k_syrk_upd phase sums
    unsigned long long z[8] = {0};
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_upd_prof), sizeof(z)) != hipSuccess) return 1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_upd_prof), z, sizeof(z)) != hipSuccess;
}
#endif
