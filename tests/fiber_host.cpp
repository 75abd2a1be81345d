// Drives the host-only fiber scheduler of the scenario batch (activesetmethods_amd/csrc/asm_fiber.h) with a fake round: no GPU, no HIP.
// One case per run: fiber_host order | body_throws | flush_throws | guard_page | two_threads | cancel_in_destructor.  Exit status 0 = passed.
// (tests/test_fiber_cpu.py builds it with -fsanitize=undefined and runs every case.)
#include "asm_fiber.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

using asmb::Fiber;

#define CHECK(c)                                                               \
    do {                                                                       \
        if (!(c)) {                                                            \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

// the fake round: logs the indices of the fibers of each flush ('*' = the fiber had something pending), throws in round `fail_round`
struct FlushFailed { int round; };
struct FakeSched : asmb::FiberSched {
    std::string log;
    int rounds = 0, fail_round = 0;
    void flush(std::vector<Fiber*>& fl) override {
        rounds += 1;
        log += "F[";
        for (size_t i = 0; i < fl.size(); ++i) log += (i ? "," : "") + std::to_string(fl[i]->index) + (fl[i]->pending ? "*" : "");
        log += "] ";
        if (rounds == fail_round) throw FlushFailed{rounds};
        for (Fiber* f : fl) f->pending = false;
    }
    void note(const std::string& s) { log += s + " "; }
    void run_bodies(std::vector<std::function<void()>> bodies) {
        std::vector<std::unique_ptr<Fiber>> fl;
        for (auto& b : bodies) fl.push_back(std::make_unique<Fiber>(std::move(b)));
        run(std::move(fl));
    }
};

// a local whose constructions and destructions are counted (per thread: case two_threads)
struct Counted {
    static thread_local int made, gone;
    Counted() { made += 1; }
    Counted(const Counted&) { made += 1; }
    ~Counted() { gone += 1; }
};
thread_local int Counted::made = 0, Counted::gone = 0;

static int me() { return asmb::cur->index; }

// ---- order: six fibers, different numbers of flush points, barriers in two cycles with tags 10 / 20 / 30
static void pass(FakeSched& S, int tag) {      // a barrier, and a note once it is behind the fiber
    asmb::barrier(tag);
    S.note("p" + std::to_string(me()) + "(" + std::to_string(asmb::cur->cycle) + "," + std::to_string(tag) + ")");
}
static void end(FakeSched& S) { S.note("e" + std::to_string(me())); }
static std::vector<std::function<void()>> order_bodies(FakeSched& S) {
    using namespace asmb;
    return {
        [&S] { next_cycle(); flush_wait(); pass(S, 10); flush_wait(); pass(S, 30); end(S); },
        [&S] { next_cycle(); flush_wait(); flush_wait(); pass(S, 10); pass(S, 30); end(S); },
        [&S] { next_cycle(); pass(S, 20); flush_wait(); pass(S, 30); end(S); },
        [&S] { next_cycle(); flush_wait(); next_cycle(); pass(S, 10); flush_wait(); end(S); },
        [&S] { next_cycle(); flush_wait(); flush_wait(); flush_wait(); pass(S, 20); end(S); },
        [&S] { next_cycle(); flush_wait(); end(S); },
    };
}
// By hand from the rule "flush before any release; release the smallest (cycle, tag), all fibers with that pair together; resume in index
// order".  Pass 1: 0 1 3 4 5 reach a flush point, 2 waits at (1,20).  Pass 2: 0 -> (1,10), 1 and 4 flush again, 3 -> (2,10), 5 ends.
// Pass 3: 1 -> (1,10), 4 flushes alone.  Pass 4: 4 -> (1,20); now 0 1 wait at (1,10), 2 4 at (1,20), 3 at (2,10) and nobody for a flush:
// (1,10) goes first, 0 flushes and joins 1 at (1,30); then (1,20): 2 flushes, 4 ends; then (1,30): 0 1 2 end; last (2,10): 3.
static const char* const ORDER_LOG =
    "F[0,1,3,4,5] e5 F[1,4] F[4] p0(1,10) p1(1,10) F[0] p2(1,20) p4(1,20) e4 F[2] p0(1,30) e0 p1(1,30) e1 p2(1,30) e2 p3(2,10) F[3] e3 ";
static void case_order() {
    FakeSched S;
    S.run_bodies(order_bodies(S));
    if (S.log != ORDER_LOG) std::fprintf(stderr, "got:  %s\nwant: %s\n", S.log.c_str(), ORDER_LOG);
    CHECK(S.log == ORDER_LOG);
    CHECK(S.n_releases == 4 && S.rounds == 6);
    CHECK(!asmb::in_fiber());
}
static void case_two_threads() {
    FakeSched S[2];
    std::thread th[2];
    for (int k = 0; k < 2; ++k)
        th[k] = std::thread([&S, k] {
            for (int rep = 0; rep < 50; ++rep) { S[k].log.clear(); S[k].run_bodies(order_bodies(S[k])); }
            CHECK(!asmb::in_fiber());
        });
    for (auto& t : th) t.join();
    for (int k = 0; k < 2; ++k) CHECK(S[k].log == ORDER_LOG);
}

// ---- one body throws: fiber 2 of 4, after a flush point, with something recorded and not flushed
static void case_body_throws() {
    FakeSched S;
    std::vector<std::function<void()>> bodies;
    for (int i = 0; i < 4; ++i)
        bodies.push_back([&S, i] {
            Counted c;
            asmb::flush_wait();
            if (i == 2) { asmb::cur->pending = true; throw std::invalid_argument("fiber 2 refuses"); }
            asmb::barrier(10);
            asmb::flush_wait();
            end(S);
        });
    bool caught = false;
    try {
        S.run_bodies(std::move(bodies));
    } catch (const std::invalid_argument& e) {
        caught = std::strcmp(e.what(), "fiber 2 refuses") == 0;
    }
    CHECK(caught);
    // the others ran to their last statement; the last flush is fiber 2's pending work
    CHECK(S.log == "F[0,1,2,3] F[0,1,3] e0 e1 e3 F[2*] ");
    CHECK(Counted::made == 4 && Counted::gone == 4);
    CHECK(!asmb::in_fiber());
}

// ---- the flush throws in its second round, with five fibers suspended at different depths
static int after = 0;           // statements after a yield point that must never run
static int inert_done = 0;
struct CallsEntryPoints {       // as a buffer pool whose destructor frees, which waits
    ~CallsEntryPoints() { asmb::flush_wait(); asmb::barrier(5); inert_done += 1; }
};
struct Wrapped { std::exception_ptr e; };
static void nested(int depth) {
    std::vector<Counted> v(3);
    if (depth > 0) { nested(depth - 1); return; }
    asmb::flush_wait();
    after += 1;
}
static void case_flush_throws() {
    FakeSched S;
    S.fail_round = 2;
    std::vector<std::function<void()>> bodies = {
        [] { Counted c; asmb::flush_wait(); asmb::flush_wait(); after += 1; },
        [] { Counted c; CallsEntryPoints d; asmb::flush_wait(); asmb::flush_wait(); after += 1; },
        [] { Counted c; asmb::flush_wait(); asmb::barrier(10); after += 1; },
        [] {
            try { Counted c; asmb::flush_wait(); asmb::barrier(10); after += 1; } catch (...) { throw Wrapped{std::current_exception()}; }
        },
        [] { Counted c; asmb::flush_wait(); nested(2); after += 1; },
    };
    bool caught = false;
    try {
        S.run_bodies(std::move(bodies));
    } catch (const FlushFailed& f) {
        caught = f.round == 2;
    }
    CHECK(caught);                                        // the flush's exception and no other (anything else leaves main uncaught)
    CHECK(S.log == "F[0,1,2,3,4] F[0,1,4] ");
    CHECK(Counted::made == 5 + 3 * 3 && Counted::gone == Counted::made);
    CHECK(inert_done == 1);
    CHECK(after == 0);
    CHECK(!asmb::in_fiber() && asmb::cur == nullptr);
    // the scheduler works on, on the stacks it has
    const size_t stacks = S.stacks.size();
    CHECK(stacks == 5);
    S.fail_round = 0;
    S.log.clear();
    std::vector<std::function<void()>> fresh;
    for (int i = 0; i < 5; ++i) fresh.push_back([&S] { Counted c; asmb::flush_wait(); asmb::barrier(10); end(S); });
    S.run_bodies(std::move(fresh));
    CHECK(S.log == "F[0,1,2,3,4] e0 e1 e2 e3 e4 ");
    CHECK(S.stacks.size() == stacks);
    CHECK(Counted::gone == Counted::made);
}

// ---- a fiber that waits inside a destructor when the round fails: the wait cannot throw there, the fiber unwinds at its next wait
static int between = 0;
struct Frees {
    ~Frees() { asmb::flush_wait_nothrow(); }
};
static void case_cancel_in_destructor() {
    FakeSched S;
    S.fail_round = 1;
    bool caught = false;
    try {
        S.run_bodies({[] { Counted c; { Frees f; } between += 1; asmb::flush_wait(); after += 1; },
                      [] { Counted c; asmb::flush_wait(); after += 1; }});
    } catch (const FlushFailed&) {
        caught = true;
    }
    CHECK(caught);
    CHECK(S.log == "F[0,1] ");
    CHECK(between == 1 && after == 0);
    CHECK(Counted::made == 2 && Counted::gone == 2);
    CHECK(!asmb::in_fiber());
}

// ---- guard page, read from /proc/self/maps without touching it
static void check_stack_mapping() {
    int local = 0;
    const uintptr_t at = (uintptr_t)&local, sp = (uintptr_t)asmb::cur->ctx.uc_stack.ss_sp;
    std::FILE* m = std::fopen("/proc/self/maps", "r");
    CHECK(m != nullptr);
    char line[512], perms[8];
    uintptr_t prev_end = 0;
    char prev_perms[8] = "";
    bool found = false;
    while (std::fgets(line, sizeof line, m)) {
        uint64_t lo = 0, hi = 0;
        if (std::sscanf(line, "%" SCNx64 "-%" SCNx64 " %7s", &lo, &hi, perms) != 3) continue;
        if (lo <= at && at < hi) {
            CHECK(lo == sp);                                              // the stack starts where the context says ...
            CHECK(hi - lo == asmb::FiberStack::SIZE);                     // ... is 2 MB long ...
            CHECK(asmb::cur->ctx.uc_stack.ss_size == asmb::FiberStack::SIZE);
            CHECK(prev_end == lo && std::strcmp(prev_perms, "---p") == 0);      // ... and the page directly below it has no access
            found = true;
            break;
        }
        prev_end = (uintptr_t)hi;
        std::strcpy(prev_perms, perms);
    }
    std::fclose(m);
    CHECK(found);
}
static void case_guard_page() {
    FakeSched S;
    int checked = 0;
    std::vector<std::function<void()>> bodies;
    for (int i = 0; i < 2; ++i) bodies.push_back([&checked] { asmb::flush_wait(); check_stack_mapping(); checked += 1; });
    S.run_bodies(std::move(bodies));
    CHECK(checked == 2);
}

int main(int argc, char** argv) {
    const std::string c = argc > 1 ? argv[1] : "";
    if (c == "order") case_order();
    else if (c == "body_throws") case_body_throws();
    else if (c == "flush_throws") case_flush_throws();
    else if (c == "guard_page") case_guard_page();
    else if (c == "two_threads") case_two_threads();
    else if (c == "cancel_in_destructor") case_cancel_in_destructor();
    else { std::fprintf(stderr, "unknown case '%s'\n", c.c_str()); return 2; }
    std::printf("%s: ok\n", c.c_str());
    return 0;
}
