// rk_prove_session: all segments of a session, several in flight per GPU, over one or more GPUs.
//
// The reference proves a session's segments one after the other (`session.prove()`,
// provers/risc0/driver/src/bonsai.rs:271).  One proof is a chain of ~120 dependent launches with a
// host round trip at every Merkle root, so a lone proof leaves an MI355X partly idle; segments are
// independent, so this entry point runs `inflight` prover contexts per GPU (one HIP stream, scratch
// pool and host thread each).  Per GPU one more context + thread (the feeder) claims segments from
// the session-wide work queue -- one claim flag per segment, shared by all GPUs, so a slower GPU or a
// short last segment never stalls the others -- and stages host-resident traces up to
// `upload_ahead` segments ahead into a ring of device buffers: the PCIe upload of segment i+1 runs
// under the proof of segment i.  Seals land in the caller's host buffers (no inter-GPU traffic, no
// collective: a single-process host such as raiko's, core/src/interfaces.rs:187-193, needs none) and
// are verified (rk_verify_segment_ex, host code) by one more thread while the GPUs go on.
// Contexts and staging buffers are kept per device for the life of the process
// (rk_session_release frees them): the `Prover` trait of the reference has no `self`, a backend's
// state is process-global (lib/src/prover.rs:52-62).
// The threads, the work queue and the handling of failures are inflight.hpp's, shared with rk_p3_prove_shards; this
// file supplies what is a segment's: the staging ring, the pinning of device-resident segments, the calls.
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include <cstdlib>

#include "inflight.hpp"
#include "internal.hpp"

namespace {

// RK_TEST_LOGICAL_DEVICES=k (test switch): the session code sees k devices, logical device d running on physical GPU
// d mod (number of GPUs).  It lets the multi-device path -- one pool, one feeder and `inflight` provers per device, the
// session-wide claim flags, the pinning of device-resident segments -- run on a box with a single GPU; every pool
// still has its own contexts, streams, staging ring and lock, so nothing is shared that real devices would not share.
int logical_devices() {
    const char* e = std::getenv("RK_TEST_LOGICAL_DEVICES");
    if (!e || !*e) return 0;
    const int k = std::atoi(e);
    return k > 0 && k <= 64 ? k : 0;
}
int physical_of(int device, int n_gpus) { return logical_devices() > 0 && n_gpus > 0 ? device % n_gpus : device; }

struct RingSlot {
    void* group[3] = {nullptr, nullptr, nullptr};
    void* check = nullptr;
    size_t words[4] = {0, 0, 0, 0};
};

void free_slot(rk_ctx* up, RingSlot* s) {
    for (int g = 0; g < 3; g++) {
        if (s->group[g]) (void)rk_free(up, s->group[g]);
        s->group[g] = nullptr;
    }
    if (s->check) (void)rk_free(up, s->check);
    s->check = nullptr;
    for (auto& w : s->words) w = 0;
}

// slots[j].key: the parameter set prover j carries (empty: risc0's defaults)
struct DevicePool : rk::CtxPool {
    int device = 0;
    std::vector<RingSlot*> ring;
    std::string last_error;
    int physical = 0;       // the GPU behind it (= device unless RK_TEST_LOGICAL_DEVICES is set)
    size_t last_proven = 0; // segments this device proved in the last session it took part in
    bool ktime_on = false;  // applied to contexts created later
    void clear() {
        for (RingSlot* s : ring) {   // a ring has slots only where there is an uploader
            free_slot(uploader, s);
            delete s;
        }
        ring.clear();
        rk::CtxPool::clear();
    }
    ~DevicePool() { clear(); }
};

std::mutex g_mu;
// shared ownership: a session that looked its pool up keeps it alive even if rk_session_release
// drops it from the map before the session locks `busy`
std::map<int, std::shared_ptr<DevicePool>> g_pools;

// the ring slots of one device no segment of the running session holds (feeder takes, provers give back)
struct FreeSlots {
    std::mutex mu;
    std::deque<RingSlot*> slots;
};

bool needs_staging(const rk_segment& s) { return s.on_device == 0; }
bool hook_accum(const rk_segment& s) { return s.hooks && s.hooks->accumulate; }
bool hook_check(const rk_segment& s) { return s.hooks && (s.hooks->eval_check || s.hooks->program); }

// a host-resident segment into `slot`, on the uploader's stream; the check evaluations span 4 << blowup_log2 columns of rows
int stage_segment(rk_ctx* up, const rk_segment& seg, unsigned blowup_log2, RingSlot* slot) {
    const size_t rows = (size_t)1 << seg.po2;
    const size_t want[4] = {hook_accum(seg) ? 0 : rows * seg.taps.group_size[0], rows * seg.taps.group_size[1],
                            rows * seg.taps.group_size[2], hook_check(seg) ? 0 : (rows * 4) << blowup_log2};
    int st = RK_OK;
    if (want[0] != slot->words[0] || want[1] != slot->words[1] || want[2] != slot->words[2] || want[3] != slot->words[3]) {
        free_slot(up, slot);
        for (int g = 0; g < 3 && st == RK_OK; g++)
            if (want[g]) st = rk_alloc(up, want[g] * 4, &slot->group[g]);
        if (st == RK_OK && want[3]) st = rk_alloc(up, want[3] * 4, &slot->check);
        if (st == RK_OK)
            for (int k = 0; k < 4; k++) slot->words[k] = want[k];
    }
    for (int g = 0; g < 3 && st == RK_OK; g++) {
        if (!want[g]) continue;
        st = seg.group[g] ? rk_h2d(up, slot->group[g], seg.group[g], want[g] * 4) : RK_ERR_INVALID;
    }
    if (st == RK_OK && want[3]) st = seg.check ? rk_h2d(up, slot->check, seg.check, want[3] * 4) : RK_ERR_INVALID;
    if (st == RK_OK) st = rk_sync(up);  // the buffers change hands after this
    return st;
}

int prove_session(const rk_session_opts* opts, const rk_segment* segs, size_t n, uint32_t* const* h_seals,
                  const size_t* seal_capacity_words, size_t* seal_words, size_t* failed_index) {
    if (failed_index) *failed_index = (size_t)-1;
    if (!opts || (n && (!segs || !h_seals || !seal_capacity_words || !seal_words))) return RK_ERR_INVALID;
    if (!rk::inflight::opts_ok(opts->inflight, opts->upload_ahead, opts->n_devices, opts->devices)) return RK_ERR_INVALID;
    std::vector<int> devices;
    if (!rk::inflight::device_list(opts->device, opts->devices, opts->n_devices, &devices)) return RK_ERR_INVALID;
    if (n == 0) return RK_OK;
    int n_gpus = 0;
    if (hipGetDeviceCount(&n_gpus) != hipSuccess || n_gpus <= 0) return RK_ERR_NODEVICE;
    const int n_visible = logical_devices() > 0 ? logical_devices() : n_gpus;
    for (int d : devices)
        if (d < 0 || d >= n_visible) return RK_ERR_INVALID;

    std::vector<std::shared_ptr<DevicePool>> pools;
    {
        std::lock_guard<std::mutex> l(g_mu);
        for (int d : devices) {
            auto& sp = g_pools[d];
            if (!sp) {
                sp = std::make_shared<DevicePool>();
                sp->device = d;
            }
            sp->physical = physical_of(d, n_gpus);
            pools.push_back(sp);
        }
    }
    std::vector<std::unique_lock<std::mutex>> sessions;
    for (auto& p : pools) sessions.emplace_back(p->busy);

    std::vector<int> owner(n, -1);   // position in `devices` of the GPU a device-resident segment lives on (-1: host-resident, any GPU)
    bool any_host = false;
    for (size_t i = 0; i < n; i++) {
        if (segs[i].on_device > 2) return RK_ERR_INVALID;
        if (needs_staging(segs[i])) {
            any_host = true;
        } else if (devices.size() == 1) {
            owner[i] = 0;
        } else {  // device-resident input: only the GPU holding it can prove it
            hipPointerAttribute_t attr{};
            if (!segs[i].group[1] || hipPointerGetAttributes(&attr, segs[i].group[1]) != hipSuccess) {
                (void)hipGetLastError();
                return RK_ERR_INVALID;
            }
            // the device of the session that runs on the GPU holding the data (with logical test devices: the first)
            for (size_t d = 0; d < devices.size(); d++)
                if (owner[i] < 0 && physical_of(devices[d], n_gpus) == attr.device) owner[i] = (int)d;
            if (owner[i] < 0) {
                if (failed_index) *failed_index = i;
                return RK_ERR_INVALID;
            }
        }
    }
    const size_t workers = std::min<size_t>((size_t)opts->inflight, n);
    // the session's parameter set, and its key: empty for risc0's defaults, so that a fresh context is not configured again
    rk_params prm;
    rk::params_preset(&prm, RK_PRESET_RISC0);
    std::vector<uint32_t> key;
    if (opts->params) {
        key = rk::params_key(*opts->params);
        if (key.empty()) return RK_ERR_INVALID;
        if (key == rk::params_key(prm)) key.clear();
        prm = *opts->params;
    }
    rk_verify_opts vopts{};
    if (opts->verify_opts) vopts = *opts->verify_opts;
    if (opts->params && !vopts.params) vopts.params = opts->params;
    const rk_verify_opts* verify_opts = (opts->verify_opts || opts->params) ? &vopts : nullptr;
    // with nothing to hide behind (upload_ahead == 0) the ring still needs one slot per prover
    const size_t n_slots = (size_t)opts->upload_ahead + workers;
    std::vector<FreeSlots> free_slots(devices.size());
    for (size_t d = 0; d < devices.size(); d++) {
        DevicePool* pool = pools[d].get();
        const size_t had = pool->slots.size();
        RK_TRY(pool->ensure(pool->physical, workers, &prm, key));
        for (size_t j = had; pool->ktime_on && j < pool->slots.size(); j++) (void)rk_set_kernel_timing(pool->slots[j].ctx, 1);
        if (any_host) RK_TRY(pool->ensure_uploader(pool->physical));
        for (size_t k = 0; k < pool->ring.size() && k < n_slots; k++) free_slots[d].slots.push_back(pool->ring[k]);
    }

    rk::inflight::Calls<RingSlot*> calls;
    calls.stage = [&](size_t d, size_t i, RingSlot** out) -> int {
        if (!needs_staging(segs[i])) return RK_OK;
        RingSlot* slot = nullptr;
        {
            std::lock_guard<std::mutex> l(free_slots[d].mu);
            if (!free_slots[d].slots.empty()) {
                slot = free_slots[d].slots.front();
                free_slots[d].slots.pop_front();
            } else {  // fewer than n_slots segments hold one: the ring has room to grow
                auto fresh = std::make_unique<RingSlot>();
                pools[d]->ring.push_back(fresh.get());
                slot = fresh.release();
            }
        }
        *out = slot;   // after a failed upload nobody releases it: it stays the ring's, for a later session
        return stage_segment(pools[d]->uploader, segs[i], prm.blowup_log2, slot);
    };
    calls.prove = [&](size_t d, size_t w, size_t i, RingSlot*& slot) -> int {
        rk_segment seg = segs[i];
        if (slot) {
            seg.on_device = 2;  // the staged copy is ours: no second copy inside the prover
            for (int g = 0; g < 3; g++) seg.group[g] = (const uint32_t*)slot->group[g];
            seg.check = (const uint32_t*)slot->check;
        }
        return rk_prove_segment(pools[d]->slots[w].ctx, &seg, h_seals[i], seal_capacity_words[i], &seal_words[i]);
    };
    calls.release = [&](size_t d, RingSlot*& slot) {
        if (!slot) return;
        std::lock_guard<std::mutex> l(free_slots[d].mu);
        free_slots[d].slots.push_back(slot);
    };
    // rk_verify_segment_ex of every finished seal (~9 ms of host time at S20, against ~26 ms per proof)
    calls.verify = [&](size_t i) -> int { return rk_verify_segment_ex(&segs[i], verify_opts, h_seals[i], seal_words[i]); };
    calls.error_text = [&](size_t d, int w) { return rk_last_error(w < 0 ? pools[d]->uploader : pools[d]->slots[(size_t)w].ctx); };

    const size_t n_verifiers = rk::inflight::verifier_threads(opts->verify, devices.size(), n, std::thread::hardware_concurrency());
    rk::inflight::Pipeline<RingSlot*> run(n, std::move(owner), devices.size(), workers, n_slots, n_verifiers, std::move(calls));
    const int status = run.run();
    for (size_t d = 0; d < devices.size(); d++) pools[d]->last_proven = run.devs[d].proven;
    if (status != RK_OK) {
        if (failed_index) *failed_index = run.failed;
        std::lock_guard<std::mutex> l(g_mu);
        for (auto& p : pools) p->last_error = run.detail;
    }
    return status;
}

}  // namespace

extern "C" {

int rk_prove_session(const rk_session_opts* opts, const rk_segment* segs, size_t n, uint32_t* const* h_seals,
                     const size_t* seal_capacity_words, size_t* seal_words, size_t* failed_index) {
    RK_GUARD_BEGIN
    return prove_session(opts, segs, n, h_seals, seal_capacity_words, seal_words, failed_index);
    RK_GUARD_END
}

}  // extern "C"

// ---- sessions that grow while they run -------------------------------------------------------------
// A worker thread takes whatever has been submitted since its last look and proves it as one
// rk_prove_session batch (the device's contexts persist, so a batch costs nothing to start): the host can
// hand over segment k while its executor is still producing segment k + 1.
struct rk_stream {
    rk_session_opts opts{};
    std::vector<int> devices;
    rk_params params{};
    rk_verify_opts vopts{};
    struct Item {
        rk_segment seg;
        uint32_t* seal;
        size_t cap;
        size_t* words;
    };
    std::mutex mu;
    std::condition_variable cv;
    std::vector<Item> items;
    size_t next = 0;
    size_t done = 0;     // items [0, done) are finished: batches complete in submission order
    bool closed = false;
    int status = RK_OK;
    size_t failed = (size_t)-1;
    std::thread worker;

    void run() {
        for (;;) {
            size_t b0, b1;
            {
                std::unique_lock<std::mutex> l(mu);
                cv.wait(l, [&] { return closed || next < items.size(); });
                if (next >= items.size()) return;  // closed and drained
                b0 = next;
                b1 = items.size();
                next = b1;
                if (status != RK_OK) {             // after a failure the rest is only drained
                    done = b1;
                    cv.notify_all();
                    continue;
                }
            }
            const size_t n = b1 - b0;
            std::vector<rk_segment> segs(n);
            std::vector<uint32_t*> seals(n);
            std::vector<size_t> caps(n), words(n, 0);
            {
                std::lock_guard<std::mutex> l(mu);
                for (size_t i = 0; i < n; i++) {
                    segs[i] = items[b0 + i].seg;
                    seals[i] = items[b0 + i].seal;
                    caps[i] = items[b0 + i].cap;
                }
            }
            size_t bad = (size_t)-1;
            int st = RK_ERR_INTERNAL;
            try {
                st = prove_session(&opts, segs.data(), n, seals.data(), caps.data(), words.data(), &bad);
            } catch (...) {
            }
            std::lock_guard<std::mutex> l(mu);
            for (size_t i = 0; i < n; i++)
                if (items[b0 + i].words) *items[b0 + i].words = words[i];
            if (st != RK_OK && status == RK_OK) {
                status = st;
                failed = bad == (size_t)-1 ? bad : b0 + bad;
            }
            done = b1;
            cv.notify_all();
        }
    }
};

extern "C" {

int rk_stream_open(const rk_session_opts* opts, rk_stream** out) {
    RK_GUARD_BEGIN
    if (!opts || !out) return RK_ERR_INVALID;
    *out = nullptr;
    if (!rk::inflight::opts_ok(opts->inflight, opts->upload_ahead, opts->n_devices, opts->devices)) return RK_ERR_INVALID;
    std::unique_ptr<rk_stream> s(new rk_stream);
    s->opts = *opts;
    if (opts->n_devices > 0) {
        s->devices.assign(opts->devices, opts->devices + opts->n_devices);
        s->opts.devices = s->devices.data();
    }
    if (opts->params) {  // the blob is copied; tables it points at stay the caller's
        s->params = *opts->params;
        s->opts.params = &s->params;
    }
    if (opts->verify_opts) {
        s->vopts = *opts->verify_opts;
        s->opts.verify_opts = &s->vopts;
    }
    rk_stream* raw = s.get();
    s->worker = std::thread([raw] { raw->run(); });
    *out = s.release();
    return RK_OK;
    RK_GUARD_END
}

int rk_stream_submit(rk_stream* s, const rk_segment* seg, uint32_t* h_seal, size_t seal_capacity_words, size_t* seal_words) {
    RK_GUARD_BEGIN
    if (!s || !seg || !h_seal) return RK_ERR_INVALID;
    std::lock_guard<std::mutex> l(s->mu);
    if (s->closed) return RK_ERR_INVALID;
    s->items.push_back(rk_stream::Item{*seg, h_seal, seal_capacity_words, seal_words});
    s->cv.notify_all();
    return RK_OK;
    RK_GUARD_END
}

int rk_stream_wait(rk_stream* s, size_t max_pending, size_t* finished_prefix) {
    RK_GUARD_BEGIN
    if (!s) return RK_ERR_INVALID;
    std::unique_lock<std::mutex> l(s->mu);
    s->cv.wait(l, [&] { return s->status != RK_OK || s->items.size() - s->done <= max_pending; });
    if (finished_prefix) *finished_prefix = s->done;
    return s->status;
    RK_GUARD_END
}

int rk_stream_close(rk_stream* s, size_t* failed_index) {
    RK_GUARD_BEGIN
    if (failed_index) *failed_index = (size_t)-1;
    if (!s) return RK_ERR_INVALID;
    {
        std::lock_guard<std::mutex> l(s->mu);
        s->closed = true;
        s->cv.notify_all();
    }
    if (s->worker.joinable()) s->worker.join();
    const int st = s->status;
    if (failed_index) *failed_index = s->failed;
    delete s;
    return st;
    RK_GUARD_END
}

// the text is copied into storage of the calling thread: a later session cannot change it under the caller
const char* rk_session_last_error(int device) {
    thread_local std::string text;
    try {
        std::shared_ptr<DevicePool> p;
        {
            std::lock_guard<std::mutex> l(g_mu);
            auto it = g_pools.find(device);
            if (it != g_pools.end()) p = it->second;
        }
        if (!p) return "";
        std::lock_guard<std::mutex> l(g_mu);
        text = p->last_error;
        return text.c_str();
    } catch (...) {
        return "";
    }
}

static std::shared_ptr<DevicePool> pool_of(int device, bool create) {
    std::lock_guard<std::mutex> l(g_mu);
    auto it = g_pools.find(device);
    if (it != g_pools.end()) return it->second;
    if (!create) return nullptr;
    auto sp = std::make_shared<DevicePool>();
    sp->device = device;
    g_pools[device] = sp;
    return sp;
}
int rk_session_set_kernel_timing(int device, int enabled) {
    RK_GUARD_BEGIN
    if (device < 0) return RK_ERR_INVALID;
    auto p = pool_of(device, true);
    std::lock_guard<std::mutex> s(p->busy);
    p->ktime_on = enabled != 0;
    for (auto& slot : p->slots) RK_TRY(rk_set_kernel_timing(slot.ctx, enabled));
    return RK_OK;
    RK_GUARD_END
}
int rk_session_kernel_stats(int device, int kclass, rk_kernel_stat* out) {
    RK_GUARD_BEGIN
    if (!out || kclass < 0 || kclass >= RK_KCLASS_COUNT) return RK_ERR_INVALID;
    *out = rk_kernel_stat{0, 0.0, 0.0};
    auto p = pool_of(device, false);
    if (!p) return RK_OK;
    std::lock_guard<std::mutex> s(p->busy);
    for (auto& slot : p->slots) {
        rk_kernel_stat st{};
        RK_TRY(rk_kernel_stats(slot.ctx, kclass, &st));
        out->launches += st.launches;
        out->ms += st.ms;
        out->bytes += st.bytes;
    }
    return RK_OK;
    RK_GUARD_END
}

// segments `device` proved in the last session it took part in (a diagnosis of the work queue's balance)
int rk_session_last_proven(int device, size_t* count) {
    RK_GUARD_BEGIN
    if (!count) return RK_ERR_INVALID;
    *count = 0;
    auto p = pool_of(device, false);
    if (!p) return RK_OK;
    std::lock_guard<std::mutex> s(p->busy);
    *count = p->last_proven;
    return RK_OK;
    RK_GUARD_END
}

int rk_session_release(void) {
    RK_GUARD_BEGIN
    rk::p3_release_pools();
    rk::code_cache_release();
    std::map<int, std::shared_ptr<DevicePool>> pools;
    {
        std::lock_guard<std::mutex> l(g_mu);
        pools.swap(g_pools);
    }
    for (auto& kv : pools) {
        std::lock_guard<std::mutex> s(kv.second->busy);  // wait for a running session of this device
        kv.second->clear();
    }
    return RK_OK;
    RK_GUARD_END
}

}  // extern "C"
