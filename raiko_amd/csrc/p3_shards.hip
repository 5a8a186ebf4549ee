// rk_p3_prove_shards / rk_p3_prove_shards_key (include/raiko_hip.h): uni-stark proofs of many shards in flight on one or
// several devices.  Per device a pool of prover contexts and an uploader, kept between calls; one feeder thread per
// device stages the traces ahead of the provers, host threads verify what is proven.  The proofs themselves are
// rk_p3_prove's / rk_p3_prove_key's (p3.hip), the checks rk_p3_verify's / rk_p3_verify_key's (p3_verify.hip): nothing else
// of those files is reached from here.  A key (p3_host.hpp) is only read: its device, parameter set, shapes and root.
#include "internal.hpp"
#include "p3_air.hpp"
#include "p3_host.hpp"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

namespace {

struct ShardPool {
    struct Slot {   // a prover context and the parameter set it was configured with: they come and go together
        rk_ctx* ctx = nullptr;
        std::vector<uint32_t> key;
    };
    std::mutex busy;                 // one batch at a time per device
    std::vector<Slot> slots;
    rk_ctx* uploader = nullptr;      // stages host-resident traces ahead of the provers (its own stream)
    std::mutex up_mu;                // the uploader's allocator: the feeder allocates, the provers free
    void drop_slots() {
        for (Slot& s : slots) (void)rk_ctx_destroy(s.ctx);
        slots.clear();
    }
    ~ShardPool() {
        drop_slots();
        if (uploader) (void)rk_ctx_destroy(uploader);
    }
};
std::mutex g_shard_mu;
std::map<int, std::shared_ptr<ShardPool>> g_shard_pools;

std::vector<uint32_t> params_key(const rk_params& p) {
    std::vector<uint32_t> k = {p.ext_w, p.root_2_27, p.coset_shift, p.p2_width, p.p2_m4, p.p2_pad_free, p.queries, p.blowup_log2,
                               p.fri_fold_log2, p.fri_min_degree, p.pow_bits};
    rk::Sys sys;
    auto any = std::make_unique<p2::Any>();
    if (rk::resolve_params(&p, &sys, any.get()) != RK_OK) return {};
    k.insert(k.end(), any->rc_ext(), any->rc_ext() + 8 * any->cells());
    k.insert(k.end(), any->rc_int(), any->rc_int() + any->rounds_partial());
    k.insert(k.end(), any->diag(), any->diag() + any->cells());
    return k;
}

// the keys of a keyed run against their slots' devices, each other, the parameter set and every shard's shapes: all of it
// from host data, before a context exists.  keys[d] belongs to devices[d].
int check_keys(const std::vector<int>& devices, const std::vector<const rk_p3_key*>& keys, const rk_params& par,
               const rk_p3_shard* shards, size_t n, size_t* failed_index) {
    rk::Sys sys;
    auto any = std::make_unique<p2::Any>();
    if (rk::resolve_params(&par, &sys, any.get()) != RK_OK) return RK_ERR_INVALID;
    const std::vector<uint32_t> tab = rk::p2_chip_tab(*any);
    const rk_p3_key* first = keys.empty() ? nullptr : keys[0];
    for (size_t d = 0; d < keys.size(); d++) {
        const rk_p3_key* k = keys[d];
        if (!k || k->device != devices[d]) return RK_ERR_INVALID;
        if (!k->same_commitment_params(par, tab)) return RK_ERR_INVALID;
        if (k->has_root() != first->has_root() || !std::equal(k->root, k->root + 8, first->root)) return RK_ERR_INVALID;
    }
    for (size_t i = 0; i < n; i++)
        for (const rk_p3_key* k : keys) {
            const rk_p3_shard& sh = shards[i];
            bool ok = sh.tables && sh.n_tables == k->tables.size();
            for (uint32_t t = 0; ok && t < sh.n_tables; t++) {
                const rk_p3_key::Table& kt = k->tables[t];
                ok = sh.tables[t].air && rk_air_prep_width(sh.tables[t].air) == kt.prep_width &&
                     (!kt.prep_width || sh.tables[t].log_height == kt.log_height);
            }
            if (!ok) {
                if (failed_index) *failed_index = i;
                return RK_ERR_INVALID;
            }
        }
    return RK_OK;
}

// caller_keys NULL: rk_p3_prove_shards; otherwise one key per device in the caller's order (rk_p3_prove_shards_key)
int p3_prove_shards(const rk_p3_session_opts* opts, const rk_p3_key* const* caller_keys, rk_p3_shard* shards, size_t n,
                    size_t* failed_index) {
    if (failed_index) *failed_index = (size_t)-1;
    if (!opts || (n && !shards) || opts->batch < 1 || opts->batch > 16) return RK_ERR_INVALID;
    if (opts->n_devices < 0 || opts->n_devices > 64 || (opts->n_devices > 0 && !opts->devices)) return RK_ERR_INVALID;
    if (n == 0) return RK_OK;
    for (size_t i = 0; !caller_keys && i < n; i++)   // no key: tables with preprocessed columns are rk_p3_prove_shards_key's
        for (uint32_t t = 0; shards[i].tables && t < shards[i].n_tables; t++)
            if (rk_air_prep_width(shards[i].tables[t].air)) {
                if (failed_index) *failed_index = i;
                return RK_ERR_INVALID;
            }
    std::vector<int> devices;
    if (opts->n_devices > 0) devices.assign(opts->devices, opts->devices + opts->n_devices);
    else devices.push_back(opts->device);
    std::vector<const rk_p3_key*> dev_keys;   // the pools are sorted by device: each key travels with its device
    if (caller_keys) {
        std::vector<size_t> order(devices.size());
        for (size_t d = 0; d < order.size(); d++) order[d] = d;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return devices[a] < devices[b]; });
        for (size_t d : order) dev_keys.push_back(caller_keys[d]);
    }
    std::sort(devices.begin(), devices.end());   // pools are locked in ascending order
    if (std::adjacent_find(devices.begin(), devices.end()) != devices.end()) return RK_ERR_INVALID;
    int n_gpus = 0;
    if (hipGetDeviceCount(&n_gpus) != hipSuccess || n_gpus <= 0) return RK_ERR_NODEVICE;
    for (int d : devices)
        if (d < 0 || d >= n_gpus) return RK_ERR_INVALID;
    rk_params par;
    rk::params_preset(&par, RK_PRESET_SP1);
    if (opts->params) par = *opts->params;
    const std::vector<uint32_t> key = params_key(par);
    if (key.empty()) return RK_ERR_INVALID;
    for (size_t i = 0; i < n; i++)
        if (!shards[i].h_proof || (shards[i].n_init && !shards[i].init_words)) return RK_ERR_INVALID;
    if (caller_keys) RK_TRY(check_keys(devices, dev_keys, par, shards, n, failed_index));
    const uint32_t* prep_root = caller_keys && dev_keys[0]->has_root() ? dev_keys[0]->root : nullptr;

    std::vector<std::shared_ptr<ShardPool>> pools;
    {
        std::lock_guard<std::mutex> l(g_shard_mu);
        for (int d : devices) {
            auto& sp = g_shard_pools[d];
            if (!sp) sp = std::make_shared<ShardPool>();
            pools.push_back(sp);
        }
    }
    std::vector<std::unique_lock<std::mutex>> held;
    for (auto& p : pools) held.emplace_back(p->busy);
    const size_t per_dev = std::min<size_t>((size_t)opts->batch, n);
    for (size_t d = 0; d < devices.size(); d++) {
        ShardPool& pool = *pools[d];
        while (pool.slots.size() < per_dev) {
            rk_ctx* c = nullptr;
            RK_TRY(rk_ctx_create(devices[d], nullptr, &c));
            pool.slots.push_back(ShardPool::Slot{c, {}});
        }
        for (size_t j = 0; j < per_dev; j++) {
            ShardPool::Slot& slot = pool.slots[j];
            if (slot.key == key) continue;
            RK_TRY(rk_set_params(slot.ctx, &par));
            slot.key = key;
        }
        if (!pool.uploader) RK_TRY(rk_ctx_create(devices[d], nullptr, &pool.uploader));
    }
    std::atomic<size_t> next{0};
    std::mutex mu;
    std::condition_variable cv;
    std::deque<size_t> to_verify;      // proven shards waiting for a verifier thread
    size_t workers_left = 0;
    int status = RK_OK;
    size_t failed = (size_t)-1;
    auto fail = [&](int st, size_t i) {
        std::lock_guard<std::mutex> l(mu);
        if (status == RK_OK) {
            status = st;
            failed = i;
        }
        cv.notify_all();
    };
    // One feeder per device claims shards from the common queue and, for traces in host memory, uploads them into device
    // buffers AHEAD of the provers (a single thread per device keeps the PCIe link busy with one stream of copies, and a
    // proof never waits for its own upload); the provers then see on_device tables.  At most `per_dev + 1` staged shards
    // per device.
    struct Staged {
        size_t idx = 0;
        std::vector<rk_p3_table> tables;
        std::vector<void*> bufs;
    };
    struct DevQueue {
        std::deque<std::unique_ptr<Staged>> ready;
        size_t outstanding = 0;     // staged or being proven
        bool feeder_done = false;
    };
    std::vector<DevQueue> dq(devices.size());
    auto release = [&](ShardPool& pool, Staged& st) {
        std::lock_guard<std::mutex> l(pool.up_mu);
        for (void* b : st.bufs) (void)rk_free(pool.uploader, b);
        st.bufs.clear();
    };
    auto feeder = [&](size_t d) {
        ShardPool& pool = *pools[d];
        for (;;) {
            {
                std::unique_lock<std::mutex> l(mu);
                cv.wait(l, [&] { return status != RK_OK || dq[d].outstanding < per_dev + 1; });
                if (status != RK_OK) break;
            }
            const size_t i = next.fetch_add(1);
            if (i >= n) break;
            auto st = std::make_unique<Staged>();
            st->idx = i;
            const rk_p3_shard& sh = shards[i];
            int rc = sh.tables && sh.n_tables ? RK_OK : RK_ERR_INVALID;
            if (rc == RK_OK) st->tables.assign(sh.tables, sh.tables + sh.n_tables);
            for (uint32_t t = 0; rc == RK_OK && t < sh.n_tables; t++) {
                rk_p3_table& tb = st->tables[t];
                if (tb.on_device || !tb.trace || tb.log_height < 1 || tb.log_height > ntt::LAMBDA || tb.width == 0) continue;   // the prover refuses what is malformed
                const size_t bytes = ((size_t)tb.width << tb.log_height) * 4;
                void* buf = nullptr;
                {
                    std::lock_guard<std::mutex> l(pool.up_mu);
                    rc = rk_alloc(pool.uploader, bytes, &buf);
                }
                if (rc != RK_OK) break;
                st->bufs.push_back(buf);
                rc = rk_h2d(pool.uploader, buf, tb.trace, bytes);      // copy + wait on the uploader's own stream
                tb.trace = (const uint32_t*)buf;
                tb.on_device = 1;
            }
            if (rc != RK_OK) {
                release(pool, *st);
                fail(rc, i);
                break;
            }
            std::lock_guard<std::mutex> l(mu);
            dq[d].outstanding++;
            dq[d].ready.push_back(std::move(st));
            cv.notify_all();
        }
        std::lock_guard<std::mutex> l(mu);
        dq[d].feeder_done = true;
        cv.notify_all();
    };
    auto worker = [&](rk_ctx* ctx, size_t d) {
        ShardPool& pool = *pools[d];
        for (;;) {
            std::unique_ptr<Staged> st;
            {
                std::unique_lock<std::mutex> l(mu);
                cv.wait(l, [&] { return status != RK_OK || !dq[d].ready.empty() || dq[d].feeder_done; });
                if (status != RK_OK || dq[d].ready.empty()) break;
                st = std::move(dq[d].ready.front());
                dq[d].ready.pop_front();
            }
            const size_t i = st->idx;
            rk_p3_shard& sh = shards[i];
            int rc = RK_ERR_INTERNAL;
            try {
                rc = caller_keys ? rk_p3_prove_key(ctx, dev_keys[d], st->tables.data(), sh.n_tables, sh.init_words, sh.n_init, sh.h_proof,
                                                   sh.capacity_words, &sh.proof_words)
                                 : rk_p3_prove(ctx, st->tables.data(), sh.n_tables, sh.init_words, sh.n_init, sh.h_proof, sh.capacity_words,
                                               &sh.proof_words);
            } catch (...) {
            }
            release(pool, *st);
            {
                std::lock_guard<std::mutex> l(mu);
                dq[d].outstanding--;
                cv.notify_all();
            }
            if (rc != RK_OK) {
                fail(rc, i);
                break;
            }
            if (opts->verify) {   // host work (~40 ms for 100 queries): never on the thread that feeds the GPU
                std::lock_guard<std::mutex> l(mu);
                to_verify.push_back(i);
                cv.notify_all();
            }
        }
        std::lock_guard<std::mutex> l(mu);
        workers_left--;
        cv.notify_all();
    };
    auto verifier = [&]() {
        for (;;) {
            size_t i;
            {
                std::unique_lock<std::mutex> l(mu);
                cv.wait(l, [&] { return !to_verify.empty() || workers_left == 0 || status != RK_OK; });
                if (status != RK_OK || to_verify.empty()) return;
                i = to_verify.front();
                to_verify.pop_front();
            }
            int v = RK_ERR_INTERNAL;
            try {
                const rk_p3_shard& sh = shards[i];
                v = caller_keys ? rk_p3_verify_key(&par, sh.tables, sh.n_tables, prep_root, sh.init_words, sh.n_init, sh.h_proof, sh.proof_words)
                                : rk_p3_verify(&par, sh.tables, sh.n_tables, sh.init_words, sh.n_init, sh.h_proof, sh.proof_words);
            } catch (...) {
            }
            if (v != 0) {
                fail(RK_ERR_VERIFY, i);
                return;
            }
        }
    };
    std::vector<std::thread> threads;
    workers_left = devices.size() * per_dev;
    for (size_t d = 0; d < devices.size(); d++) {
        threads.emplace_back(feeder, d);
        for (size_t j = 0; j < per_dev; j++) threads.emplace_back(worker, pools[d]->slots[j].ctx, d);
    }
    if (opts->verify) {
        const unsigned hw = std::thread::hardware_concurrency();
        size_t nv = std::min<size_t>(std::min<size_t>(16, 4 * devices.size()), std::max<unsigned>(1, hw / 4));
        nv = std::min(nv, n);
        for (size_t v = 0; v < nv; v++) threads.emplace_back(verifier);
    }
    for (auto& t : threads) t.join();
    for (size_t d = 0; d < devices.size(); d++)     // a failed run leaves staged shards nobody proved
        for (auto& st : dq[d].ready) release(*pools[d], *st);
    if (failed_index) *failed_index = failed;
    return status;
}

}  // namespace

namespace rk {
void p3_release_pools() {
    std::map<int, std::shared_ptr<ShardPool>> pools;
    {
        std::lock_guard<std::mutex> l(g_shard_mu);
        pools.swap(g_shard_pools);
    }
    for (auto& kv : pools) {
        std::lock_guard<std::mutex> l(kv.second->busy);   // wait for a running batch
        kv.second->drop_slots();
    }
}
}  // namespace rk

extern "C" {

int rk_p3_prove_shards(const rk_p3_session_opts* opts, rk_p3_shard* shards, size_t n, size_t* failed_index) {
    RK_GUARD_BEGIN
    return p3_prove_shards(opts, nullptr, shards, n, failed_index);
    RK_GUARD_END
}
int rk_p3_prove_shards_key(const rk_p3_session_opts* opts, const rk_p3_key* const* keys, rk_p3_shard* shards, size_t n,
                           size_t* failed_index) {
    RK_GUARD_BEGIN
    return p3_prove_shards(opts, keys, shards, n, failed_index);
    RK_GUARD_END
}

}  // extern "C"
