// Several proofs in flight per GPU: the one host-thread pipeline behind rk_prove_session (session.hip) and
// rk_p3_prove_shards (p3_shards.hip).  Per device one feeder thread claims items from the run-wide work queue -- one
// claim flag per item, shared by all devices, so a slower GPU or a short last item never stalls the others -- and stages
// them ahead of `workers` prover threads under a bound on the items a device holds; a few more host threads verify what
// is proven while the GPUs go on.  One mutex, one condition variable, and the first failure wins: its status, item and
// text are the run's.  What an item is, how it is staged, proven and verified is the caller's, behind plain callables.
// Standard C++ and the RK_* status codes only: no GPU runtime, so the machine runs (and is tested) without a GPU.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/raiko_hip.h"

namespace rk {
namespace inflight {

// the ranges of an options struct: proofs in flight per GPU, items staged ahead, and the optional device list
inline bool opts_ok(int per_gpu, int ahead, int n_devices, const int* devices) {
    return per_gpu >= 1 && per_gpu <= 16 && ahead >= 0 && ahead <= 16 && n_devices >= 0 && n_devices <= 64 && (n_devices == 0 || devices);
}
// the devices of a run in ascending order (the order their pools are locked in: no lock cycles); false on a duplicate
inline bool device_list(int device, const int* devices, int n_devices, std::vector<int>* out) {
    if (n_devices > 0) out->assign(devices, devices + n_devices);
    else out->assign(1, device);
    std::sort(out->begin(), out->end());
    return std::adjacent_find(out->begin(), out->end()) == out->end();
}
// host threads that verify.  request 0: none; 1: the library's choice; more: that many (at most 16).
// A segment seal takes ~7 ms of host time to verify whatever the segment size (50 query paths of Poseidon2): one thread
// keeps up with 2^20-cycle segments, smaller ones need more (2^16: 3.5 ms per proof)
inline size_t verifier_threads(int request, size_t n_devices, size_t n_items, unsigned hw_threads) {
    if (!request) return 0;
    const size_t nv = request == 1 ? std::min<size_t>(std::min<size_t>(16, 4 * n_devices), std::max<unsigned>(1, hw_threads / 4))
                                   : std::min<size_t>((size_t)request, 16);
    return std::min(nv, n_items);
}

// What the caller supplies.  `d` is the position of a device in the run's list, `worker` that of a prover thread of it.
template <class Handle>
struct Calls {
    // on the feeder thread of `d`: RK_OK and *out filled, or a status with nothing left behind
    std::function<int(size_t d, size_t item, Handle* out)> stage;
    std::function<int(size_t d, size_t worker, size_t item, Handle& h)> prove;
    // exactly once per staged handle, proven or not (after a failed run also for those no prover took)
    std::function<void(size_t d, Handle& h)> release;
    std::function<int(size_t item)> verify;                          // 0 or a reason
    std::function<const char*(size_t d, int worker)> error_text;     // of a failed stage (worker -1) or prove; may be empty
};

template <class Handle>
struct Pipeline {
    struct Item {
        size_t idx;
        Handle handle;
    };
    struct Dev {
        std::vector<Item> ready;     // claimed and staged, not yet taken by a prover
        size_t outstanding = 0;      // claimed, proof not finished
        size_t cursor = 0;
        size_t proven = 0;
        bool feeder_done = false;
    };
    const size_t n, workers, bound, n_verifiers;
    const std::vector<int> owner;    // per item: the device (position in the list) that alone may take it, or -1 for any
    Calls<Handle> calls;
    std::vector<Dev> devs;
    std::vector<char> claimed;
    std::vector<size_t> to_verify;   // proven items in the order they finished; verifiers take from verify_next
    size_t verify_next = 0;
    size_t provers_left = 0;
    std::mutex mu;
    std::condition_variable cv;
    int status = RK_OK;              // first failure
    size_t failed = (size_t)-1;
    std::string detail;

    // `bound` items per device are claimed and not yet proven at most, the one being staged included
    Pipeline(size_t n_items, std::vector<int> owner_of, size_t n_devices, size_t workers_per_device, size_t bound_per_device,
             size_t verifiers, Calls<Handle> c)
        : n(n_items), workers(workers_per_device), bound(bound_per_device), n_verifiers(verifiers), owner(std::move(owner_of)),
          calls(std::move(c)), devs(n_devices), claimed(n_items, 0) {
        for (Dev& dv : devs) dv.ready.reserve(bound);   // never more than `outstanding`: handing an item over cannot throw
        to_verify.reserve(n_verifiers ? n : 0);
    }

    void fail(int st, size_t idx, const char* text) {
        std::lock_guard<std::mutex> l(mu);
        if (status == RK_OK) {
            status = st;
            failed = idx;
            try {
                detail = text ? text : "";
            } catch (...) {
            }
        }
        cv.notify_all();
    }
    size_t outstanding(size_t d) {
        std::lock_guard<std::mutex> l(mu);
        return devs[d].outstanding;
    }

    // next unclaimed item device `d` may take, scanning from its cursor (mu held)
    bool claim(size_t d, size_t* out) {
        Dev& dv = devs[d];
        for (size_t i = dv.cursor; i < n; i++) {
            if (owner[i] >= 0 && (size_t)owner[i] != d) continue;
            const bool taken = claimed[i] != 0;
            claimed[i] = 1;
            if (i == dv.cursor) dv.cursor++;
            if (taken) continue;
            *out = i;
            return true;
        }
        return false;
    }

    // claims items for one device and stages them
    void feeder(size_t d) {
        Dev& dv = devs[d];
        for (;;) {
            size_t i = 0;
            {
                std::unique_lock<std::mutex> l(mu);
                cv.wait(l, [&] { return status != RK_OK || dv.outstanding < bound; });
                if (status != RK_OK || !claim(d, &i)) return;
                dv.outstanding++;
            }
            Handle h{};
            const int st = calls.stage(d, i, &h);
            if (st != RK_OK) {
                fail(st, i, calls.error_text ? calls.error_text(d, -1) : nullptr);
                return;
            }
            std::lock_guard<std::mutex> l(mu);
            dv.ready.push_back(Item{i, std::move(h)});
            cv.notify_all();
        }
    }
    void prover(size_t d, size_t w) {
        Dev& dv = devs[d];
        for (;;) {
            std::unique_lock<std::mutex> l(mu);
            cv.wait(l, [&] { return status != RK_OK || !dv.ready.empty() || dv.feeder_done; });
            if (status != RK_OK || dv.ready.empty()) return;
            Item it = std::move(dv.ready.front());
            dv.ready.erase(dv.ready.begin());
            l.unlock();
            int st;
            try {
                st = calls.prove(d, w, it.idx, it.handle);
            } catch (...) {
                calls.release(d, it.handle);
                throw;
            }
            calls.release(d, it.handle);
            l.lock();
            dv.outstanding--;
            if (st == RK_OK) dv.proven++;
            if (st == RK_OK && n_verifiers) to_verify.push_back(it.idx);   // host work: never on the thread that feeds the GPU
            cv.notify_all();
            l.unlock();
            if (st != RK_OK) {
                fail(st, it.idx, calls.error_text ? calls.error_text(d, (int)w) : nullptr);
                return;
            }
        }
    }
    void verifier() {
        for (;;) {
            size_t i;
            {
                std::unique_lock<std::mutex> l(mu);
                cv.wait(l, [&] { return verify_next < to_verify.size() || provers_left == 0 || status != RK_OK; });
                if (status != RK_OK || verify_next == to_verify.size()) return;   // failed, or all provers done and nothing left
                i = to_verify[verify_next++];
            }
            const int v = calls.verify(i);
            if (v != 0) {
                fail(RK_ERR_VERIFY, i, ("seal failed verification (reason " + std::to_string(v) + ")").c_str());
                return;
            }
        }
    }

    // A thread's loop with whatever a callback throws turned into the run's failure; the counters the other threads wait
    // on move all the same.
    template <class Loop>
    void guarded(const char* what, Loop loop) {
        try {
            loop();
        } catch (...) {
            fail(RK_ERR_INTERNAL, (size_t)-1, what);
        }
    }
    void feeder_thread(size_t d) {
        guarded("exception in a feeder thread", [&] { feeder(d); });
        std::lock_guard<std::mutex> l(mu);
        devs[d].feeder_done = true;
        cv.notify_all();
    }
    void prover_thread(size_t d, size_t w) {
        guarded("exception in a prover thread", [&] { prover(d, w); });
        std::lock_guard<std::mutex> l(mu);
        provers_left--;
        cv.notify_all();
    }

    // Runs the items to the end or to the first failure, joins every thread and returns the run's status.
    int run() {
        std::vector<std::thread> threads;
        threads.reserve(devs.size() * (1 + workers) + n_verifiers);
        provers_left = devs.size() * workers;
        try {
            for (size_t d = 0; d < devs.size(); d++) {
                threads.emplace_back([this, d] { feeder_thread(d); });
                for (size_t w = 0; w < workers; w++) threads.emplace_back([this, d, w] { prover_thread(d, w); });
            }
            for (size_t v = 0; v < n_verifiers; v++)
                threads.emplace_back([this] { guarded("exception in a verifier thread", [&] { verifier(); }); });
        } catch (...) {   // a thread that did not start: the ones that did see the failure and return
            fail(RK_ERR_INTERNAL, (size_t)-1, "could not start a thread");
        }
        for (auto& t : threads) t.join();
        for (size_t d = 0; d < devs.size(); d++) {   // a failed run leaves staged items nobody proved
            for (Item& it : devs[d].ready) calls.release(d, it.handle);
            devs[d].ready.clear();
        }
        return status;
    }
};

}  // namespace inflight
}  // namespace rk
