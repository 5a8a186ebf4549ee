// rk_p3_prove_shards / rk_p3_prove_shards_key / rk_p3_prove_shards_claims (include/raiko_hip.h): uni-stark proofs of many shards in flight on one or
// several devices.  Per device a pool of prover contexts and an uploader, kept between calls; one feeder thread per
// device stages the traces ahead of the provers, host threads verify what is proven.  The proofs themselves are
// rk_p3_prove's / rk_p3_prove_key's (p3.hip), the checks rk_p3_verify's / rk_p3_verify_key's (p3_verify.hip): nothing else
// of those files is reached from here.  A key (p3_host.hpp) is only read: its device, parameter set, shapes and root.
// The threads, the work queue and the handling of failures are inflight.hpp's, shared with rk_prove_session.
#include "inflight.hpp"
#include "internal.hpp"
#include "p3_air.hpp"
#include "p3_host.hpp"

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

namespace {

struct ShardPool : rk::CtxPool {
    std::mutex up_mu;                // the uploader's allocator: the feeder allocates, the provers free
};
std::mutex g_shard_mu;
std::map<int, std::shared_ptr<ShardPool>> g_shard_pools;

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

// a shard whose host-resident traces were uploaded: its tables as the prover sees them (on_device) and the buffers behind
struct Staged {
    std::vector<rk_p3_table> tables;
    std::vector<void*> bufs;
};

// caller_keys NULL: rk_p3_prove_shards; otherwise one key per device in the caller's order (rk_p3_prove_shards_key)
// claims NULL: none; otherwise claims[i] / n_claims[i] are what shard i's verifier adds (rk_p3_prove_shards_claims)
int p3_prove_shards(const rk_p3_session_opts* opts, const rk_p3_key* const* caller_keys, rk_p3_shard* shards, size_t n,
                    size_t* failed_index, const rk_p3_claim* const* claims = nullptr, const uint32_t* n_claims = nullptr) {
    if (failed_index) *failed_index = (size_t)-1;
    if (claims && !n_claims) return RK_ERR_INVALID;
    if (!opts || (n && !shards) || !rk::inflight::opts_ok(opts->batch, 0, opts->n_devices, opts->devices)) return RK_ERR_INVALID;
    if (n == 0) return RK_OK;
    for (size_t i = 0; !caller_keys && i < n; i++)   // no key: tables with preprocessed columns are rk_p3_prove_shards_key's
        for (uint32_t t = 0; shards[i].tables && t < shards[i].n_tables; t++)
            if (rk_air_prep_width(shards[i].tables[t].air)) {
                if (failed_index) *failed_index = i;
                return RK_ERR_INVALID;
            }
    std::vector<int> devices;
    if (!rk::inflight::device_list(opts->device, opts->devices, opts->n_devices, &devices)) return RK_ERR_INVALID;
    std::vector<const rk_p3_key*> dev_keys;   // the pools are sorted by device: each key travels with its device
    for (size_t d = 0; caller_keys && d < devices.size(); d++)
        dev_keys.push_back(caller_keys[opts->n_devices > 0 ? std::find(opts->devices, opts->devices + opts->n_devices, devices[d]) - opts->devices : 0]);
    int n_gpus = 0;
    if (hipGetDeviceCount(&n_gpus) != hipSuccess || n_gpus <= 0) return RK_ERR_NODEVICE;
    for (int d : devices)
        if (d < 0 || d >= n_gpus) return RK_ERR_INVALID;
    rk_params par;
    rk::params_preset(&par, RK_PRESET_SP1);
    if (opts->params) par = *opts->params;
    const std::vector<uint32_t> key = rk::params_key(par);
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
        RK_TRY(pools[d]->ensure(devices[d], per_dev, &par, key));
        RK_TRY(pools[d]->ensure_uploader(devices[d]));
    }

    using Handle = std::unique_ptr<Staged>;
    rk::inflight::Calls<Handle> calls;
    auto release = [&](size_t d, Handle& st) {
        std::lock_guard<std::mutex> l(pools[d]->up_mu);
        for (void* b : st->bufs) (void)rk_free(pools[d]->uploader, b);
        st->bufs.clear();
    };
    calls.release = release;
    // For traces in host memory the feeder uploads them into device buffers AHEAD of the provers (a single thread per device
    // keeps the PCIe link busy with one stream of copies, and a proof never waits for its own upload); the provers then see
    // on_device tables.
    calls.stage = [&](size_t d, size_t i, Handle* out) -> int {
        ShardPool& pool = *pools[d];
        auto st = std::make_unique<Staged>();
        const rk_p3_shard& sh = shards[i];
        int rc = sh.tables && sh.n_tables ? RK_OK : RK_ERR_INVALID;
        if (rc == RK_OK) st->tables.assign(sh.tables, sh.tables + sh.n_tables);
        if (rc == RK_OK) st->bufs.reserve(sh.n_tables);   // a buffer is never allocated and then not recorded
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
        if (rc != RK_OK) release(d, st);
        else *out = std::move(st);
        return rc;
    };
    calls.prove = [&](size_t d, size_t w, size_t i, Handle& st) -> int {
        rk_ctx* ctx = pools[d]->slots[w].ctx;
        rk_p3_shard& sh = shards[i];
        return caller_keys ? rk_p3_prove_key(ctx, dev_keys[d], st->tables.data(), sh.n_tables, sh.init_words, sh.n_init, sh.h_proof,
                                             sh.capacity_words, &sh.proof_words)
                           : rk_p3_prove(ctx, st->tables.data(), sh.n_tables, sh.init_words, sh.n_init, sh.h_proof, sh.capacity_words,
                                         &sh.proof_words);
    };
    // host work (~40 ms for 100 queries)
    calls.verify = [&](size_t i) -> int {
        const rk_p3_shard& sh = shards[i];
        if (claims)   // a NULL root is the unkeyed check there
            return rk_p3_verify_claims(&par, sh.tables, sh.n_tables, prep_root, sh.init_words, sh.n_init, sh.h_proof, sh.proof_words, claims[i],
                                       n_claims[i]);
        return caller_keys ? rk_p3_verify_key(&par, sh.tables, sh.n_tables, prep_root, sh.init_words, sh.n_init, sh.h_proof, sh.proof_words)
                           : rk_p3_verify(&par, sh.tables, sh.n_tables, sh.init_words, sh.n_init, sh.h_proof, sh.proof_words);
    };
    // Any device may take any shard.  At most `per_dev + 1` shards per device are staged, being staged or being proven.
    const size_t n_verifiers = rk::inflight::verifier_threads(opts->verify ? 1 : 0, devices.size(), n, std::thread::hardware_concurrency());
    rk::inflight::Pipeline<Handle> run(n, std::vector<int>(n, -1), devices.size(), per_dev, per_dev + 1, n_verifiers, std::move(calls));
    const int status = run.run();
    if (failed_index) *failed_index = run.failed;
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
        kv.second->clear();
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
int rk_p3_prove_shards_claims(const rk_p3_session_opts* opts, const rk_p3_key* const* keys, rk_p3_shard* shards,
                              const rk_p3_claim* const* claims, const uint32_t* n_claims, size_t n, size_t* failed_index) {
    RK_GUARD_BEGIN
    return p3_prove_shards(opts, keys, shards, n, failed_index, claims, n_claims);
    RK_GUARD_END
}

}  // extern "C"
