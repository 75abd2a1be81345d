// Host side of the scenario batch (device side: asm_bt.hip.h).  SURVEY.md section 8 rows b / e; the reference has one model per
// optimizer and no batching (src/MOI_wrapper.jl:1093-1152), so this is the build's own design for BASELINE.json's scenario batch.
//
// B scenarios are solved by B *fibers* (user-level contexts) of ONE host thread.  Each fiber runs the ordinary single-scenario solver
// code on its own handle.  That code makes every stream operation through the functions at the end of this header:
//   asmb::launch / launch_resident(kernel, grid, block, stream, args...)      asmb::blocks(n, per) - the 1-D grid of ceil(n / per)
//   asmb::copy_async / fill_async(..., stream)      asmb::copy / fill(...)      asmb::sync(stream)      asmb::free(p)
// and what such a call does depends on where it is made:
//   * outside a fiber     it is the plain stream operation (kernel launch with bt.tab = nullptr, copy, fill, synchronise, free);
//   * inside a fiber      the operation is RECORDED (kernel, grid, packed arguments; copies become copy-kernel operations whose
//                         payload travels in the round's blob), and the fiber yields when it needs a result on the host
//                         (sync, copy, fill, free, read-backs) or reaches an alignment point (barrier).
// When every fiber is blocked the scheduler MERGES the recorded lists position by position: operations of different fibers that are
// the same kernel with the same grid become one launch with the scenario index in gridDim.z and an argument table in HBM (one H2D
// copy of all tables + payloads per round), on one stream; a completion word in host-mapped memory ends the round.  Scenarios that
// leave the common path simply stop matching: their operations are launched on their own, in order.  Results are bit-identical to
// the per-scenario path by construction (same kernels, same arguments, same grids).
// Alignment: fibers wait at barriers (tags in program order); the scheduler releases the group with the smallest (cycle, tag) first
// once nobody can run - min-PC-first reconvergence, as a SIMT machine treats a divergent loop.  Fibers, scheduler and these waits are
// host-only code in asm_fiber.h; this header is the recorder on top of them.
#pragma once
#include <cstdint>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "asm_bt.hip.h"
#include "asm_fiber.h"

// copy / fill operations of recorded streams (every asmb::copy_async / asmb::fill_async inside a fiber becomes one of these)
__global__ __launch_bounds__(256) void k_bcopy(AsmBt bt, char* dst, const char* src, int64_t bytes) {
    ASM_BARGS(bt, dst, src, bytes);
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const uintptr_t al = (uintptr_t)dst | (uintptr_t)src | (uintptr_t)bytes;
    if ((al & 15) == 0) {
        for (int64_t i = t0; i < bytes / 16; i += stride) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
    } else if ((al & 7) == 0) {
        for (int64_t i = t0; i < bytes / 8; i += stride) reinterpret_cast<uint64_t*>(dst)[i] = reinterpret_cast<const uint64_t*>(src)[i];
    } else if ((al & 3) == 0) {
        for (int64_t i = t0; i < bytes / 4; i += stride) reinterpret_cast<uint32_t*>(dst)[i] = reinterpret_cast<const uint32_t*>(src)[i];
    } else {
        for (int64_t i = t0; i < bytes; i += stride) dst[i] = src[i];
    }
}
__global__ __launch_bounds__(256) void k_bfill(AsmBt bt, char* dst, int value, int64_t bytes) {
    ASM_BARGS(bt, dst, value, bytes);
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const unsigned v = (unsigned)(value & 0xff) * 0x01010101u;
    const uintptr_t al = (uintptr_t)dst | (uintptr_t)bytes;
    if ((al & 15) == 0) {
        for (int64_t i = t0; i < bytes / 16; i += stride) reinterpret_cast<uint4*>(dst)[i] = make_uint4(v, v, v, v);
    } else if ((al & 3) == 0) {
        for (int64_t i = t0; i < bytes / 4; i += stride) reinterpret_cast<uint32_t*>(dst)[i] = v;
    } else {
        for (int64_t i = t0; i < bytes; i += stride) dst[i] = (char)value;
    }
}
// last operation of a round: everything before it on the stream has finished when the word arrives on the host
__global__ void k_bsignal(AsmBt bt, unsigned* word, unsigned value) {
    ASM_BARGS(bt, word, value);
    __threadfence_system();
    __hip_atomic_store(word, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

namespace asmb {

// ---- argument packing: the layout rule of asm_bget (natural alignment, declaration order, entry rounded up to 16 bytes)
template <class T>
constexpr size_t pk_align(size_t off) { return (off + alignof(T) - 1) & ~(alignof(T) - 1); }
template <class... KA>
constexpr size_t pk_size() {
    size_t off = 0;
    ((off = pk_align<KA>(off) + sizeof(KA)), ...);
    return (off + 15) & ~(size_t)15;
}
template <class... KA>
inline void pk_write(char* dst, const KA&... a) {
    size_t off = 0;
    ((off = pk_align<KA>(off), std::memcpy(dst + off, &a, sizeof(KA)), off += sizeof(KA)), ...);
}
template <class T>
inline T conv(T v) { return v; }

enum { OP_RESIDENT = 1 };      // every workgroup of the launch must be resident at once (dataflow panel kernels)

struct Op {
    const void* kfn;
    void (*thunk)(const void* kfn, dim3 g, dim3 b, unsigned sh, hipStream_t s, AsmBt bt);
    unsigned gx, gy, gz, bx, by, bz, shmem, flags;
    uint32_t arg_off, arg_size;            // packed arguments in the fiber's argument arena
    int32_t src_payload;                   // >= 0: H2D copy - argument `src` (offset 8) is patched to the payload's place in the round's blob
    uint32_t payload_bytes;
    void* h_dst;                           // != nullptr: D2H copy - argument `dst` (offset 0) is patched to a place in the out-staging buffer
    uint32_t out_bytes;
};

// what a fiber has recorded since its last flush
struct RecFiber : Fiber {
    using Fiber::Fiber;
    std::vector<Op> ops;
    std::vector<char> args, payload;
    // merge cursor / per-round scratch
    size_t cursor = 0;
    std::vector<uint32_t> out_off;
};

struct Sched : FiberSched {
    const int device;
    const hipStream_t stream;
    char *h_blob = nullptr, *d_blob = nullptr;
    size_t blob_cap = 0;
    char *h_out = nullptr, *d_out = nullptr;
    size_t out_cap = 0;
    unsigned *h_sig = nullptr, *d_sig = nullptr;
    unsigned round = 0;
    const int panel_wgs;
    // statistics (n_releases, t_host_ms: the scheduler's)
    uint64_t n_rounds = 0, n_ops = 0, n_launches = 0, blob_bytes = 0;
    double t_emit_ms = 0, t_wait_ms = 0;
    const bool verbose;                                     // ASM_BATCH_VERBOSE=1: per-kernel merge statistics when the scheduler leaves
    // HIP events around every merged launch of the dataflow panel kernels (OP_RESIDENT) on this group's stream: the family bench.py's roofline names
    const bool time_resident;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> res_events;
    std::vector<hipEvent_t> res_pool;
    double res_ms = 0.0;
    uint64_t res_launches = 0, res_ops = 0;
    uint64_t res_grid_max = 0;                              // most workgroups of one (merged) OP_RESIDENT launch
    hipEvent_t res_event() {
        if (!res_pool.empty()) { hipEvent_t e = res_pool.back(); res_pool.pop_back(); return e; }
        hipEvent_t e;
        chk(hipEventCreate(&e), "hipEventCreate");
        return e;
    }
    void resolve_resident() {                               // (the stream is idle: every round ends with a completion wait)
        for (auto& pr : res_events) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) res_ms += ms;
            res_pool.push_back(pr.first); res_pool.push_back(pr.second);
        }
        res_events.clear();
    }
    // per-kernel merge table, kept while `counting` is on (ASM_BATCH_VERBOSE=1, or the test entry asm_test_batch_kernel_counting)
    struct KernelCount { uint64_t ops = 0, launches = 0; unsigned nb_max = 0; };      // operations recorded, launches made, most scenarios of one launch
    bool counting = false;
    std::map<std::pair<const void*, unsigned>, KernelCount> per_kernel;   // (kernel, gridDim.z of one scenario) -> counts

    static void chk(hipError_t e, const char* what) {
        if (e != hipSuccess) throw BatchError(std::string(what) + ": " + hipGetErrorString(e));
    }
    void reserve_blob(size_t need) {
        if (need <= blob_cap) return;
        if (h_blob) (void)hipHostFree(h_blob);
        if (d_blob) (void)::hipFree(d_blob);
        h_blob = d_blob = nullptr, blob_cap = 0;      // (should an allocation below fail: nothing to free twice, nothing claimed)
        const size_t cap = std::max<size_t>(need * 2, (size_t)4 << 20);
        chk(hipHostMalloc((void**)&h_blob, cap), "hipHostMalloc(blob)");
        chk(hipMalloc((void**)&d_blob, cap), "hipMalloc(blob)");
        blob_cap = cap;
    }
    void reserve_out(size_t need) {
        if (need <= out_cap) return;
        if (h_out) (void)hipHostFree(h_out);
        h_out = nullptr, out_cap = 0;
        const size_t cap = std::max<size_t>(need * 2, (size_t)1 << 20);
        chk(hipHostMalloc((void**)&h_out, cap, hipHostMallocMapped), "hipHostMalloc(out)");
        chk(hipHostGetDevicePointer((void**)&d_out, h_out, 0), "hipHostGetDevicePointer(out)");
        out_cap = cap;
    }
    void free_buffers() {
        if (h_blob) (void)hipHostFree(h_blob);
        if (d_blob) (void)::hipFree(d_blob);
        if (h_out) (void)hipHostFree(h_out);
        if (h_sig) (void)hipHostFree(h_sig);
    }
    Sched(int dev, hipStream_t s, int pwgs, bool verbose_, bool time_resident_) : device(dev), stream(s), panel_wgs(pwgs), verbose(verbose_), time_resident(time_resident_), counting(verbose_) {
        try {
            chk(hipHostMalloc((void**)&h_sig, 64, hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc(sig)");
            chk(hipHostGetDevicePointer((void**)&d_sig, h_sig, 0), "hipHostGetDevicePointer(sig)");
            *h_sig = 0;
            reserve_blob((size_t)4 << 20);
            reserve_out((size_t)1 << 20);
        } catch (...) { free_buffers(); throw; }      // (no destructor runs for a constructor that throws)
    }
    ~Sched() override {
        if (verbose && !per_kernel.empty()) {
            std::map<const void*, std::pair<uint64_t, uint64_t>> by_kernel;      // kernel -> (operations, launches), every gz together
            for (auto& kv : per_kernel) { auto& pk = by_kernel[kv.first.first]; pk.first += kv.second.ops; pk.second += kv.second.launches; }
            std::vector<std::pair<uint64_t, const void*>> v;
            for (auto& kv : by_kernel) v.push_back({kv.second.second, kv.first});
            std::sort(v.rbegin(), v.rend());
            std::fprintf(stderr, "[asm batch] rounds %llu, launches by kernel (launches, operations, operations per launch):\n", (unsigned long long)n_rounds);
            for (size_t i = 0; i < v.size() && i < 40; ++i) {
                const auto& pk = by_kernel[v[i].second];
                const char* nm = hipKernelNameRefByPtr(v[i].second, stream);
                std::fprintf(stderr, "[asm batch]   %8llu %9llu %6.1f  %.60s\n", (unsigned long long)pk.second, (unsigned long long)pk.first, (double)pk.first / (double)pk.second, nm ? nm : "?");
            }
        }
        for (auto& pr : res_events) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        for (hipEvent_t e : res_pool) (void)hipEventDestroy(e);
        free_buffers();
    }
    void run_range(int lo, int hi, const std::function<void(int)>& body) {      // fiber s of [lo, hi) runs body(s)
        std::vector<std::unique_ptr<Fiber>> fl;
        for (int s = lo; s < hi; ++s) fl.push_back(std::make_unique<RecFiber>([&body, s] { body(s); }));
        if (!fl.empty()) run(std::move(fl));
    }

    static bool same(const Op& a, const Op& b) {
        return a.kfn == b.kfn && a.gx == b.gx && a.gy == b.gy && a.gz == b.gz && a.bx == b.bx && a.by == b.by && a.bz == b.bz && a.shmem == b.shmem &&
               a.arg_size == b.arg_size;
    }

    void flush(std::vector<Fiber*>& waiting) override {      // (every fiber of this scheduler is a RecFiber: run_range)
        std::vector<RecFiber*> fl(waiting.size());
        std::transform(waiting.begin(), waiting.end(), fl.begin(), [](Fiber* f) { return static_cast<RecFiber*>(f); });
        emit(fl);
    }
    // merge and launch the recorded operations of `fl`, wait for the round to finish, hand the read-backs to their destinations
    void emit(std::vector<RecFiber*>& fl) {
        const double t0 = now_ms();
        // ---- sizes: tables + payloads (blob), read-back staging (out)
        size_t need_blob = 0, need_out = 0;
        for (RecFiber* f : fl) {
            for (const Op& o : f->ops) {
                need_blob += o.arg_size + 16;
                if (o.src_payload >= 0) need_blob += ((size_t)o.payload_bytes + 15) & ~(size_t)15;
                if (o.h_dst) need_out += ((size_t)o.out_bytes + 15) & ~(size_t)15;
            }
            f->cursor = 0;
            f->out_off.assign(f->ops.size(), 0);
        }
        reserve_blob(need_blob + 64);
        reserve_out(need_out + 64);
        // ---- payloads first, then one table per merged launch
        size_t bo = 0, oo = 0;
        for (RecFiber* f : fl)
            for (size_t i = 0; i < f->ops.size(); ++i) {
                Op& o = f->ops[i];
                if (o.src_payload >= 0) {
                    std::memcpy(h_blob + bo, f->payload.data() + o.src_payload, o.payload_bytes);
                    const char* src = d_blob + bo;
                    std::memcpy(f->args.data() + o.arg_off + 8, &src, 8);
                    bo += ((size_t)o.payload_bytes + 15) & ~(size_t)15;
                }
                if (o.h_dst) {
                    char* dst = d_out + oo;
                    std::memcpy(f->args.data() + o.arg_off, &dst, 8);
                    f->out_off[i] = (uint32_t)oo;
                    oo += ((size_t)o.out_bytes + 15) & ~(size_t)15;
                }
            }
        struct Launch { const Op* op; size_t tab; unsigned nb; };
        std::vector<Launch> launches;
        std::vector<RecFiber*> group;
        for (;;) {
            RecFiber* lead = nullptr;                    // the least advanced fiber leads (keeps the cursors together)
            for (RecFiber* f : fl)
                if (f->cursor < f->ops.size() && (!lead || f->cursor < lead->cursor)) lead = f;
            if (!lead) break;
            const Op& X = lead->ops[lead->cursor];
            size_t cap = fl.size();
            if (X.flags & OP_RESIDENT) cap = std::max<size_t>(1, (size_t)panel_wgs / std::max(1u, X.gx * X.gy * X.gz));
            cap = std::min<size_t>(cap, 65535u / std::max(1u, X.gz));
            group.clear();
            for (RecFiber* f : fl)
                if (group.size() < cap && f->cursor < f->ops.size() && (f == lead || same(f->ops[f->cursor], X))) group.push_back(f);
            bo = (bo + 15) & ~(size_t)15;
            launches.push_back({&X, bo, (unsigned)group.size()});
            if (counting) {
                KernelCount& pk = per_kernel[{X.kfn, X.gz}];
                pk.ops += group.size(); pk.launches += 1; pk.nb_max = std::max(pk.nb_max, (unsigned)group.size());
            }
            for (RecFiber* f : group) {
                std::memcpy(h_blob + bo, f->args.data() + f->ops[f->cursor].arg_off, X.arg_size);
                bo += X.arg_size;
                f->cursor += 1;
            }
        }
        // ---- one copy of the blob, then the launches, then the completion word
        if (bo > 0) chk(::hipMemcpyAsync(d_blob, h_blob, bo, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(blob)");
        for (const Launch& L : launches) {
            const Op& X = *L.op;
            AsmBt bt{(const void*)(d_blob + L.tab), X.arg_size, X.gz};
            const bool timed = time_resident && (X.flags & OP_RESIDENT);
            if (X.flags & OP_RESIDENT) res_grid_max = std::max<uint64_t>(res_grid_max, (uint64_t)X.gx * X.gy * X.gz * L.nb);
            hipEvent_t ea = nullptr, eb = nullptr;
            if (timed) { ea = res_event(); eb = res_event(); chk(hipEventRecord(ea, stream), "hipEventRecord"); }
            X.thunk(X.kfn, dim3(X.gx, X.gy, X.gz * L.nb), dim3(X.bx, X.by, X.bz), X.shmem, stream, bt);
            if (timed) { chk(hipEventRecord(eb, stream), "hipEventRecord"); res_events.push_back({ea, eb}); res_launches += 1; res_ops += L.nb; }
        }
        round += 1;
        if (round == 0) round = 1;
        k_bsignal<<<dim3(1), dim3(1), 0, stream>>>(AsmBt{nullptr, 0, 1}, d_sig, round);
        chk(hipGetLastError(), "launch");
        const double t1 = now_ms();
        wait_round();
        const double t2 = now_ms();
        if (!res_events.empty()) resolve_resident();
        for (RecFiber* f : fl) {
            for (size_t i = 0; i < f->ops.size(); ++i)
                if (f->ops[i].h_dst) std::memcpy(f->ops[i].h_dst, h_out + f->out_off[i], f->ops[i].out_bytes);
            n_ops += f->ops.size();
            f->ops.clear(); f->args.clear(); f->payload.clear();
            f->pending = false;
        }
        n_rounds += 1;
        n_launches += launches.size() + 1;
        blob_bytes += bo;
        t_emit_ms += t1 - t0;
        t_wait_ms += t2 - t1;
    }
    void wait_round() {
        const double t0 = now_ms();
        for (unsigned long spins = 1;; ++spins) {
            if (__atomic_load_n(h_sig, __ATOMIC_ACQUIRE) == round) return;
            __builtin_ia32_pause();
            if ((spins & 0xfffff) == 0 && now_ms() - t0 > 60000.0) {
                chk(::hipStreamSynchronize(stream), "hipStreamSynchronize");      // a device fault surfaces here
                if (__atomic_load_n(h_sig, __ATOMIC_ACQUIRE) == round) return;
                throw BatchError("batch round: the stream finished without its completion word");
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------- what the solver code calls
template <class... KA>
void thunk(const void* kfn, dim3 g, dim3 b, unsigned sh, hipStream_t s, AsmBt bt) {
    auto k = reinterpret_cast<void (*)(AsmBt, KA...)>(const_cast<void*>(kfn));
    k<<<g, b, sh, s>>>(bt, KA{}...);
}

template <class... KA>
inline Op& record(RecFiber* f, void (*kern)(AsmBt, KA...), dim3 g, dim3 b, unsigned sh, unsigned flags, const KA&... a) {
    constexpr size_t sz = pk_size<KA...>();
    const size_t off = f->args.size();
    f->args.resize(off + sz);
    pk_write<KA...>(f->args.data() + off, a...);
    Op o;
    o.kfn = (const void*)kern;
    o.thunk = &thunk<KA...>;
    o.gx = g.x; o.gy = g.y; o.gz = g.z; o.bx = b.x; o.by = b.y; o.bz = b.z; o.shmem = sh; o.flags = flags;
    o.arg_off = (uint32_t)off; o.arg_size = (uint32_t)sz;
    o.src_payload = -1; o.payload_bytes = 0; o.h_dst = nullptr; o.out_bytes = 0;
    f->ops.push_back(o);
    f->pending = true;
    return f->ops.back();
}
// the fiber that records the calling thread's stream operations, nullptr outside a batch (a cancelled one records nothing and answers hipSuccess)
inline RecFiber* recording() { return static_cast<RecFiber*>(cur); }

// the grid of a one-dimensional launch: ceil(n / per) workgroups (n == 0 gives the zero grid that launch skips)
inline dim3 blocks(int64_t n, int64_t per = 256) { return dim3((unsigned)((n + per - 1) / per)); }

// kernel launch (no dynamic shared memory); the arguments are converted to the kernel's own parameter types.  A grid with a zero
// dimension launches nothing
template <class... KA, class... A>
inline void launch(void (*kern)(AsmBt, KA...), dim3 g, dim3 b, hipStream_t st, A&&... a) {
    static_assert(sizeof...(KA) == sizeof...(A), "kernel launch: argument count does not match the kernel's parameter list");
    if (g.x == 0 || g.y == 0 || g.z == 0) return;
    RecFiber* f = recording();
    if (!f) {
        kern<<<g, b, 0, st>>>(AsmBt{nullptr, 0, g.z}, conv<KA>(a)...);
        return;
    }
    if (!f->cancelled) record<KA...>(f, kern, g, b, 0u, 0u, conv<KA>(a)...);
}
// launch whose workgroups must all be resident at once (OP_RESIDENT): the merge keeps the joint grid inside Sched::panel_wgs
template <class... KA, class... A>
inline void launch_resident(void (*kern)(AsmBt, KA...), dim3 g, dim3 b, hipStream_t st, A&&... a) {
    static_assert(sizeof...(KA) == sizeof...(A), "kernel launch: argument count does not match the kernel's parameter list");
    RecFiber* f = recording();
    if (!f) {
        kern<<<g, b, 0, st>>>(AsmBt{nullptr, 0, g.z}, conv<KA>(a)...);
        return;
    }
    if (!f->cancelled) record<KA...>(f, kern, g, b, 0u, (unsigned)OP_RESIDENT, conv<KA>(a)...);
}

inline unsigned copy_grid(size_t bytes) { return (unsigned)std::min<size_t>(64, std::max<size_t>(1, (bytes + 16383) / 16384)); }

inline hipError_t copy_async(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
    RecFiber* f = recording();
    if (!f) {
        // outside a batch: device-to-device copies of the solver's vectors (4 - 150 KB, ~60 per LP) as a copy kernel of this library - the
        // runtime's blit path brackets each copy with its own barrier / signal packets
        if (kind == hipMemcpyDeviceToDevice && bytes > 0 && bytes <= ((size_t)64 << 20)) {
            k_bcopy<<<dim3((unsigned)std::min<size_t>(256, std::max<size_t>(1, (bytes + 16383) / 16384))), dim3(256), 0, st>>>(AsmBt{nullptr, 0, 1}, (char*)dst, (const char*)src, (int64_t)bytes);
            return hipGetLastError();
        }
        return ::hipMemcpyAsync(dst, src, bytes, kind, st);
    }
    if (bytes == 0 || f->cancelled) return hipSuccess;
    if (kind == hipMemcpyHostToDevice) {
        const size_t po = (f->payload.size() + 15) & ~(size_t)15;
        f->payload.resize(po + bytes);
        std::memcpy(f->payload.data() + po, src, bytes);
        Op& o = record<char*, const char*, int64_t>(f, k_bcopy, dim3(copy_grid(bytes)), dim3(256), 0, 0u, (char*)dst, (const char*)nullptr, (int64_t)bytes);
        o.src_payload = (int32_t)po;
        o.payload_bytes = (uint32_t)bytes;
    } else if (kind == hipMemcpyDeviceToHost) {
        Op& o = record<char*, const char*, int64_t>(f, k_bcopy, dim3(copy_grid(bytes)), dim3(256), 0, 0u, (char*)nullptr, (const char*)src, (int64_t)bytes);
        o.h_dst = dst;
        o.out_bytes = (uint32_t)bytes;
    } else if (kind == hipMemcpyDeviceToDevice) {
        record<char*, const char*, int64_t>(f, k_bcopy, dim3(copy_grid(bytes)), dim3(256), 0, 0u, (char*)dst, (const char*)src, (int64_t)bytes);
    } else {
        return hipErrorInvalidValue;
    }
    return hipSuccess;
}
inline hipError_t fill_async(void* dst, int value, size_t bytes, hipStream_t st) {
    RecFiber* f = recording();
    if (!f) {
        if (bytes > 0 && bytes <= ((size_t)64 << 20)) {
            k_bfill<<<dim3((unsigned)std::min<size_t>(256, std::max<size_t>(1, (bytes + 16383) / 16384))), dim3(256), 0, st>>>(AsmBt{nullptr, 0, 1}, (char*)dst, value, (int64_t)bytes);
            return hipGetLastError();
        }
        return ::hipMemsetAsync(dst, value, bytes, st);
    }
    if (bytes == 0 || f->cancelled) return hipSuccess;
    record<char*, int, int64_t>(f, k_bfill, dim3(copy_grid(bytes)), dim3(256), 0, 0u, (char*)dst, value, (int64_t)bytes);
    return hipSuccess;
}
// the host waits for the stream; inside a fiber: for everything the fiber has recorded
inline hipError_t sync(hipStream_t st) {
    if (!cur) return ::hipStreamSynchronize(st);
    flush_wait();
    return hipSuccess;
}
// synchronous copy / fill / free
inline hipError_t copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (!cur) return ::hipMemcpy(dst, src, bytes, kind);
    hipError_t e = copy_async(dst, src, bytes, kind, nullptr);
    flush_wait();
    return e;
}
inline hipError_t fill(void* dst, int value, size_t bytes) {
    if (!cur) return ::hipMemset(dst, value, bytes);
    hipError_t e = fill_async(dst, value, bytes, nullptr);
    flush_wait();
    return e;
}
inline hipError_t free(void* p) {
    flush_wait_nothrow();      // recorded operations may still use the buffer (destructors free: no throw from here)
    return ::hipFree(p);
}

}  // namespace asmb
