// Host-only core of the scenario batch (asm_batch.hip.h records and merges on top of it): fibers - user-level contexts of ONE host thread -
// and the scheduler that runs them.  No HIP here: it compiles as plain C++17, and tests/fiber_host.cpp drives it with a fake round.
//
// A fiber runs until it needs the results of what it has recorded (flush_wait) or reaches an alignment point (barrier).  When no fiber can
// run the scheduler hands the fibers that wait for a flush to its owner's flush() - the one thing it does not know - and makes them
// runnable; when nobody waits for a flush it releases the barrier group with the smallest (cycle, tag) - min-PC-first reconvergence, as a
// SIMT machine treats a divergent loop.
// Failures: a body that throws ends its own fiber only, the others run on, and run() rethrows the first such exception in index order.  A
// flush() that throws is a failed round: every fiber that has not ended is CANCELLED - resumed once to unwind its own frames, so that
// every destructor on its stack runs - and run() rethrows what flush() threw.
#pragma once
#include <sys/mman.h>
#include <time.h>
#include <ucontext.h>
#include <unistd.h>
#include <cstddef>
#include <cstdint>
#include <exception>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace asmb {

struct BatchError : std::runtime_error {
    explicit BatchError(const std::string& s) : std::runtime_error(s) {}
};

// A fiber's stack: 2 MB above one page without access, so that code which runs too deep stops there instead of writing into the stack
// of its neighbour (the stacks of one scheduler usually lie next to each other).  Owns the mapping; move-only.
struct FiberStack {
    static constexpr size_t SIZE = (size_t)2 << 20;
    char* base = nullptr;       // the guard page; the stack is [base + page, base + page + SIZE)
    size_t page = 0;
    FiberStack() : page((size_t)sysconf(_SC_PAGESIZE)) {
        void* p = mmap(nullptr, SIZE + page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_STACK, -1, 0);
        if (p == MAP_FAILED) throw BatchError("mmap of a fiber stack failed");
        if (mprotect(p, page, PROT_NONE) != 0) { munmap(p, SIZE + page); throw BatchError("mprotect of a fiber stack's guard page failed"); }
        base = (char*)p;
    }
    FiberStack(FiberStack&& o) noexcept : base(o.base), page(o.page) { o.base = nullptr; }
    FiberStack& operator=(FiberStack&& o) noexcept { std::swap(base, o.base); std::swap(page, o.page); return *this; }
    ~FiberStack() { if (base) munmap(base, SIZE + page); }
    void* sp() const { return base + page; }
};

struct FiberSched;

// (the recorder derives its fiber from this one: the scheduler owns fibers through the base, hence the virtual destructor)
struct Fiber {
    enum State { RUNNABLE, WAIT_FLUSH, WAIT_BARRIER, DONE };
    ucontext_t ctx;
    State state = RUNNABLE;
    long cycle = 0;
    int tag = 0;
    int index = 0;
    bool pending = false;       // the fiber has recorded what no flush has taken yet: set by whoever records, cleared by flush()
    bool cancelled = false;     // a round failed: the fiber unwinds at its next wait that may throw ...
    bool unwinding = false;     // ... and from then on every entry point does nothing (destructors call them)
    FiberSched* sched = nullptr;
    std::function<void()> body;
    std::exception_ptr err;
    explicit Fiber(std::function<void()> b) : body(std::move(b)) {}
    Fiber(const Fiber&) = delete;
    Fiber& operator=(const Fiber&) = delete;
    virtual ~Fiber() = default;
};

inline thread_local Fiber* cur = nullptr;      // per thread: every group of a batch has its own thread and scheduler

inline bool in_fiber() { return cur != nullptr; }

struct FiberSched {
    ucontext_t main_ctx;
    std::vector<FiberStack> stacks;            // kept from one run to the next: a run of no more fibers than an earlier one maps nothing
    uint64_t n_releases = 0;
    double t_host_ms = 0;

    FiberSched() = default;
    FiberSched(const FiberSched&) = delete;
    FiberSched& operator=(const FiberSched&) = delete;
    virtual ~FiberSched() = default;

    // every fiber of `fl` waits for the results of what it has recorded: get them (and clear the fibers' `pending`)
    virtual void flush(std::vector<Fiber*>& fl) = 0;

    static double now_ms() {
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
    }

    // run every fiber to completion (fiber i on stack i); the fibers are gone when this returns or throws
    void run(std::vector<std::unique_ptr<Fiber>> fibers) {
        while (stacks.size() < fibers.size()) stacks.emplace_back();
        for (size_t i = 0; i < fibers.size(); ++i) {
            Fiber* f = fibers[i].get();
            f->sched = this;
            f->index = (int)i;
            getcontext(&f->ctx);
            f->ctx.uc_stack.ss_sp = stacks[i].sp();
            f->ctx.uc_stack.ss_size = FiberStack::SIZE;
            f->ctx.uc_link = nullptr;
            const uintptr_t p = (uintptr_t)f;
            makecontext(&f->ctx, (void (*)())trampoline, 2, (unsigned)(p & 0xffffffffu), (unsigned)(p >> 32));
        }
        std::exception_ptr failed;
        try {
            loop(fibers);
        } catch (...) {
            failed = std::current_exception();
        }
        if (failed) {      // (outside the handler: the fibers throw and catch on their own stacks)
            for (auto& f : fibers) f->cancelled = f->state != Fiber::DONE;
            for (auto& f : fibers)
                if (f->cancelled) resume(f.get());
            std::rethrow_exception(failed);
        }
        for (auto& f : fibers)
            if (f->err) std::rethrow_exception(f->err);
    }

private:
    static void trampoline(unsigned lo, unsigned hi) {
        Fiber* f = reinterpret_cast<Fiber*>(((uintptr_t)hi << 32) | (uintptr_t)lo);
        try {
            if (!f->cancelled) f->body();
        } catch (...) {
            // whatever arrives from a cancelled fiber is its unwinding, however the frames on the way wrapped it
            if (!f->cancelled) f->err = std::current_exception();
        }
        f->state = Fiber::DONE;
        cur = nullptr;
        swapcontext(&f->ctx, &f->sched->main_ctx);      // never resumed
    }
    void resume(Fiber* f) {
        cur = f;
        f->state = Fiber::RUNNABLE;
        swapcontext(&main_ctx, &f->ctx);
        cur = nullptr;
    }
    void loop(std::vector<std::unique_ptr<Fiber>>& fibers) {
        std::vector<Fiber*> fl;
        for (;;) {
            bool any_live = false, progressed = false;
            for (auto& f : fibers) {
                if (f->state == Fiber::RUNNABLE) {
                    const double t0 = now_ms();
                    resume(f.get());
                    t_host_ms += now_ms() - t0;
                    progressed = true;
                }
                any_live = any_live || f->state != Fiber::DONE;
            }
            if (!any_live) break;
            fl.clear();
            for (auto& f : fibers)
                if (f->state == Fiber::WAIT_FLUSH) fl.push_back(f.get());
            if (!fl.empty()) {
                flush(fl);
                for (Fiber* f : fl) f->state = Fiber::RUNNABLE;
                continue;
            }
            // everybody waits at a barrier (or is done): release the group with the smallest (cycle, tag)
            Fiber* mn = nullptr;
            for (auto& f : fibers)
                if (f->state == Fiber::WAIT_BARRIER && (!mn || f->cycle < mn->cycle || (f->cycle == mn->cycle && f->tag < mn->tag))) mn = f.get();
            if (!mn) {
                if (!progressed) throw BatchError("batch scheduler: no fiber can run");
                continue;
            }
            for (auto& f : fibers)
                if (f->state == Fiber::WAIT_BARRIER && f->cycle == mn->cycle && f->tag == mn->tag) f->state = Fiber::RUNNABLE;
            n_releases += 1;
        }
        // a fiber that ended with recorded operations still pending (it should not, unless its body threw): flush them so that nothing is lost
        fl.clear();
        for (auto& f : fibers)
            if (f->pending) fl.push_back(f.get());
        if (!fl.empty()) flush(fl);
    }
};

// ---------------------------------------------------------------------------------------------- what the code on a fiber calls
inline void yield_to_scheduler(Fiber* f) {
    cur = nullptr;
    swapcontext(&f->ctx, &f->sched->main_ctx);
}
struct Cancelled {};      // what unwinds a cancelled fiber: private to this header, deliberately no std::exception
inline void wait_as(Fiber::State s) {
    Fiber* f = cur;
    if (!f || f->unwinding) return;
    if (!f->cancelled) { f->state = s; yield_to_scheduler(f); }
    if (f->cancelled) { f->unwinding = true; throw Cancelled{}; }
}
// the fiber needs the results of everything it has recorded
inline void flush_wait() { wait_as(Fiber::WAIT_FLUSH); }
// the same for a caller that must not throw (a destructor that frees a buffer): a fiber cancelled while it waits here goes on to its next
// flush_wait or barrier and unwinds from there
inline void flush_wait_nothrow() noexcept {
    Fiber* f = cur;
    if (!f || f->cancelled) return;
    f->state = Fiber::WAIT_FLUSH;
    yield_to_scheduler(f);
}
// alignment point `tag` (tags grow in program order inside one cycle); no-op outside a batch
inline void barrier(int tag) {
    if (cur && !cur->cancelled) cur->tag = tag;
    wait_as(Fiber::WAIT_BARRIER);
}
inline void next_cycle() {
    if (cur) cur->cycle += 1;
}

}  // namespace asmb
