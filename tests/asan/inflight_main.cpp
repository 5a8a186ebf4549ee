// The in-flight pipeline of raiko_amd/csrc/inflight.hpp as a program of its own: built by tests/test_inflight_host.py from
// the header alone (plain C++, no GPU toolchain), once with -fsanitize=thread and once with -fsanitize=address,undefined.
// The callbacks are fakes that count their calls and yield; a handle is a heap block of its own, so one that is never
// released is a leak the address sanitizer reports, and one released twice a double free.  Every scenario prints one line;
// a scenario that deadlocks prints none and the caller's time limit ends the program.  Prints "inflight_main ok" and
// returns 0 when every scenario held.
#include <atomic>
#include <cstdio>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "inflight.hpp"

namespace {

using Handle = int*;
using Pipe = rk::inflight::Pipeline<Handle>;
constexpr size_t NONE = (size_t)-1;

enum Where { NOWHERE, STAGE, PROVE, VERIFY };

// the callbacks of one run and what they saw
struct Fake {
    size_t n, n_devices, workers;
    std::vector<std::atomic<int>> staged, proven, released, verified, proven_on;   // per item
    std::atomic<int> inside{0};               // callbacks running now
    std::atomic<size_t> max_outstanding{0};   // the largest count a stage saw
    std::vector<std::string> text;            // per (device, worker + 1): what error_text gives
    Pipe* pipe = nullptr;
    // what goes wrong, and where
    Where fail_in = NOWHERE, throw_in = NOWHERE;
    size_t at = NONE;
    int code = 0;
    size_t at2 = NONE;                        // a second prove that fails, at the same time as the first
    int code2 = 0;
    std::atomic<int> failing_now{0};
    std::function<void(size_t d, size_t item)> before_prove;

    Fake(size_t items, size_t devs, size_t w)
        : n(items), n_devices(devs), workers(w), staged(items), proven(items), released(items), verified(items), proven_on(items),
          text(devs * (w + 1)) {
        for (size_t i = 0; i < n; i++) staged[i] = proven[i] = released[i] = verified[i] = 0, proven_on[i] = -1;
    }
    struct Inside {
        std::atomic<int>& c;
        explicit Inside(std::atomic<int>& x) : c(x) { c++; }
        ~Inside() { c--; }
    };
    int result(Where w, size_t d, int worker, size_t i) {
        std::this_thread::yield();
        if (throw_in == w && i == at) throw std::runtime_error("a callback that throws");
        const int st = fail_in == w && i == at ? code : fail_in == w && i == at2 ? code2 : 0;
        if (st != 0 && w != VERIFY) text[d * (workers + 1) + (size_t)(worker + 1)] = "item " + std::to_string(i) + " failed";
        if (st != 0 && at2 != NONE) {   // both failures are on their way before either is reported
            failing_now++;
            while (failing_now.load() < 2) std::this_thread::yield();
        }
        return st;
    }
    rk::inflight::Calls<Handle> calls() {
        rk::inflight::Calls<Handle> c;
        c.stage = [this](size_t d, size_t i, Handle* out) -> int {
            Inside in(inside);
            const size_t o = pipe->outstanding(d);
            size_t seen = max_outstanding.load();
            while (o > seen && !max_outstanding.compare_exchange_weak(seen, o)) {
            }
            const int st = result(STAGE, d, -1, i);
            if (st != 0) return st;
            staged[i]++;
            *out = new int((int)i);
            return 0;
        };
        c.prove = [this](size_t d, size_t w, size_t i, Handle& h) -> int {
            Inside in(inside);
            if (!h || *h != (int)i) return RK_ERR_INVALID;   // the handle is the one staged for this item
            if (before_prove) before_prove(d, i);
            const int st = result(PROVE, d, (int)w, i);
            if (st != 0) return st;
            proven[i]++;
            proven_on[i] = (int)d;
            return 0;
        };
        c.release = [this](size_t, Handle& h) {
            Inside in(inside);
            released[(size_t)*h]++;
            delete h;
            h = nullptr;
        };
        c.verify = [this](size_t i) -> int {
            Inside in(inside);
            const int v = result(VERIFY, 0, 0, i);
            verified[i]++;
            return v;
        };
        c.error_text = [this](size_t d, int w) { return text[d * (workers + 1) + (size_t)(w + 1)].c_str(); };
        return c;
    }
    // runs the items; afterwards no callback is running and every staged handle was released exactly once
    bool run(std::vector<int> owner, size_t bound, size_t verifiers, Pipe** out) {
        pipe = new Pipe(n, std::move(owner), n_devices, workers, bound, verifiers, calls());
        *out = pipe;
        pipe->run();
        bool ok = inside.load() == 0 && max_outstanding.load() <= bound;
        for (size_t i = 0; i < n; i++) ok = ok && staged[i] <= 1 && released[i] == staged[i] && proven[i] <= staged[i];
        for (auto& dv : pipe->devs) ok = ok && dv.ready.empty();
        return ok;
    }
    ~Fake() { delete pipe; }
};

bool report(const char* name, bool ok) {
    std::printf("scenario %s: %s\n", name, ok ? "ok" : "FAILED");
    std::fflush(stdout);
    return ok;
}

// every item staged, proven, released and verified exactly once
bool all_done_once(Fake& f, Pipe* p, bool verified) {
    bool ok = p->status == RK_OK && p->failed == NONE && p->detail.empty();
    size_t sum = 0;
    for (auto& dv : p->devs) sum += dv.proven;
    for (size_t i = 0; i < f.n; i++) ok = ok && f.staged[i] == 1 && f.proven[i] == 1 && f.released[i] == 1 && f.verified[i] == (verified ? 1 : 0);
    return ok && sum == f.n;
}

bool normal_run() {
    Fake f(7, 2, 2);
    Pipe* p;
    return f.run(std::vector<int>(7, -1), 3, 2, &p) && all_done_once(f, p, true);
}
bool more_workers_than_items() {
    Fake f(1, 2, 2);
    Pipe* p;
    return f.run({-1}, 3, 1, &p) && all_done_once(f, p, true);
}
// Items 0-3 are device 1's, 4-5 anyone's.  Device 1 holds three of its items (the bound) and proves none until the feeder
// of device 0 is done: device 0 finished while item 3 was nobody's yet.
bool pinned_items() {
    Fake f(6, 2, 2);
    Pipe* p;
    std::mutex once;
    int item3_unclaimed = -1;
    f.before_prove = [&](size_t d, size_t) {
        if (d != 1) return;
        for (;;) {
            std::unique_lock<std::mutex> l(f.pipe->mu);
            if (f.pipe->devs[0].feeder_done) break;
            l.unlock();
            std::this_thread::yield();
        }
        std::lock_guard<std::mutex> o(once);   // before any proof of device 1 returns and lets its feeder claim again
        if (item3_unclaimed < 0) {
            std::lock_guard<std::mutex> l(f.pipe->mu);
            item3_unclaimed = f.pipe->claimed[3] == 0;
        }
    };
    bool ok = f.run({1, 1, 1, 1, -1, -1}, 3, 1, &p) && all_done_once(f, p, true) && item3_unclaimed == 1;
    for (size_t i = 0; i < 4; i++) ok = ok && f.proven_on[i] == 1;
    return ok && p->devs[0].proven + p->devs[1].proven == 6 && p->devs[1].proven >= 4;
}
// status, index and text of the run come from the one event
bool one_failure(Where w, int code, int want_status) {
    Fake f(7, 2, 2);
    f.fail_in = w;
    f.at = 3;
    f.code = code;
    Pipe* p;
    const bool ok = f.run(std::vector<int>(7, -1), 3, 2, &p);
    const std::string text = w == VERIFY ? "seal failed verification (reason " + std::to_string(code) + ")" : "item 3 failed";
    return ok && p->status == want_status && p->failed == 3 && p->detail == text;
}
bool two_failures() {
    Fake f(8, 2, 2);
    f.fail_in = PROVE;
    f.at = 2;
    f.code = RK_ERR_CAPACITY;
    f.at2 = 5;
    f.code2 = RK_ERR_CALLBACK;
    Pipe* p;
    const bool ok = f.run(std::vector<int>(8, -1), 3, 0, &p);
    const bool first = p->status == RK_ERR_CAPACITY && p->failed == 2 && p->detail == "item 2 failed";
    const bool second = p->status == RK_ERR_CALLBACK && p->failed == 5 && p->detail == "item 5 failed";
    return ok && (first || second);
}
bool exception_in(Where w) {
    Fake f(7, 2, 2);
    f.throw_in = w;
    f.at = 3;
    Pipe* p;
    return f.run(std::vector<int>(7, -1), 3, 2, &p) && p->status == RK_ERR_INTERNAL;
}
bool verify_off() {
    Fake f(7, 2, 2);
    Pipe* p;
    const size_t nv = rk::inflight::verifier_threads(0, 2, 7, 64);
    return nv == 0 && f.run(std::vector<int>(7, -1), 3, nv, &p) && all_done_once(f, p, false);
}
// the checks and the rule that need no thread
bool options_and_counts() {
    using namespace rk::inflight;
    const int two[2] = {3, 1}, dup[2] = {2, 2};
    std::vector<int> out;
    bool ok = opts_ok(1, 0, 0, nullptr) && opts_ok(16, 16, 64, two) && !opts_ok(0, 0, 0, nullptr) && !opts_ok(17, 0, 0, nullptr) &&
              !opts_ok(1, -1, 0, nullptr) && !opts_ok(1, 17, 0, nullptr) && !opts_ok(1, 0, -1, nullptr) && !opts_ok(1, 0, 65, two) &&
              !opts_ok(1, 0, 2, nullptr);
    ok = ok && device_list(5, nullptr, 0, &out) && out == std::vector<int>{5};
    ok = ok && device_list(5, two, 2, &out) && out == std::vector<int>{1, 3} && !device_list(5, dup, 2, &out);
    // 1: up to four per device, a quarter of the hardware threads, at least one; more: that many, at most 16; never more than items
    ok = ok && verifier_threads(1, 2, 7, 8) == 2 && verifier_threads(1, 1, 100, 64) == 4 && verifier_threads(1, 8, 100, 256) == 16 &&
         verifier_threads(1, 1, 100, 0) == 1 && verifier_threads(5, 1, 100, 0) == 5 && verifier_threads(40, 1, 100, 8) == 16 &&
         verifier_threads(5, 1, 3, 8) == 3 && verifier_threads(0, 4, 100, 64) == 0;
    return ok;
}

}  // namespace

int main() {
    int bad = 0;
    bad += !report("options and counts", options_and_counts());
    bad += !report("normal run", normal_run());
    bad += !report("more workers than items", more_workers_than_items());
    bad += !report("pinned items", pinned_items());
    bad += !report("stage fails", one_failure(STAGE, RK_ERR_CAPACITY, RK_ERR_CAPACITY));
    bad += !report("prove fails", one_failure(PROVE, RK_ERR_CALLBACK, RK_ERR_CALLBACK));
    bad += !report("verify fails", one_failure(VERIFY, 9, RK_ERR_VERIFY));
    bad += !report("two failures at once", two_failures());
    bad += !report("stage throws", exception_in(STAGE));
    bad += !report("prove throws", exception_in(PROVE));
    bad += !report("verify throws", exception_in(VERIFY));
    bad += !report("verify off", verify_off());
    if (!bad) std::printf("inflight_main ok: 12 scenarios\n");
    return bad != 0;
}
