// Internal declarations shared by the translation units of libraiko_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/raiko_hip.h"
#include "taps.hpp"
#include "bb.hpp"
#include "ntt_core.hpp"
#include "poseidon2_core.hpp"
#include "params.hpp"

struct rk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string last_error;

    // twiddle / power tables (one device allocation)
    uint32_t* d_tables = nullptr;
    ntt::Tables tb{};

    // the parameter set (rk_set_params): field / protocol values and the Poseidon2 instance -- host copy
    // for the transcript, device copy (the active Core's Consts) for the kernels
    rk::Sys sys{};
    p2::Any h_p2{};
    void* d_p2 = nullptr;

    // caching allocator (exact-size free lists) so steady-state proving never calls hipMalloc
    std::multimap<size_t, void*> free_list;
    std::unordered_map<void*, size_t> live;
    size_t pooled_bytes = 0;                         // bytes parked in free_list
    size_t pool_limit = (size_t)24 << 30;            // parked bytes above this: the cache is dropped (varying shapes); several contexts share one GPU

    // small staging area for per-call parameter uploads
    void* d_scratch = nullptr;
    size_t scratch_bytes = 0;
    // page-locked ring the small uploads are staged in (rk::upload): no wait per upload
    void* h_ring = nullptr;
    size_t h_ring_at = 0;
    bool h_ring_failed = false;

    rk_timing timing{};
    rk_p3_timing p3_timing{};
    std::vector<hipEvent_t> stage_events;            // pool behind the per-stage brackets of prove_segment

    // optional per-kernel-class timing (hipEvent pairs on the ctx stream, resolved lazily)
    bool ktime_on = false;
    struct KRec {
        hipEvent_t a, b;
        int cls;
        double bytes;
    };
    std::vector<KRec> krecs;
    size_t krec_used = 0;
    double k_ms[RK_KCLASS_COUNT] = {0};
    double k_bytes[RK_KCLASS_COUNT] = {0};
    uint64_t k_launches[RK_KCLASS_COUNT] = {0};
};

#define RK_HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);              \
            return RK_ERR_HIP;                                                                  \
        }                                                                                       \
    } while (0)
// extern "C" bodies never let a C++ exception cross the ABI ("never aborts")
#define RK_GUARD_BEGIN try {
#define RK_GUARD_END                                   \
    }                                                  \
    catch (const std::bad_alloc&) { return RK_ERR_NOMEM; } \
    catch (...) { return RK_ERR_INTERNAL; }
#define RK_TRY(expr)                \
    do {                            \
        int _s = (expr);            \
        if (_s != RK_OK) return _s; \
    } while (0)

static inline bool is_pow2(size_t n) { return n && !(n & (n - 1)); }
static inline unsigned log2u(size_t n) {
    unsigned k = 0;
    while (((size_t)1 << k) < n) k++;
    return k;
}

namespace rk {

// per-kernel-class timing (context.hip): bracket a launch; no-ops unless enabled
struct KTimer {
    rk_ctx* ctx;
    int idx;
    KTimer(rk_ctx* c, int cls, double algorithmic_bytes);
    ~KTimer();
};

// optional roctx ranges around the proof stages (context.hip): libroctx64 is looked up at run time and only
// when RK_ROCTX is set, so the library has no link-time dependency on it
bool trace_push(const char* name);
void trace_pop();

// memory (context.hip)
int dev_alloc(rk_ctx* ctx, size_t bytes, void** out);
int dev_free(rk_ctx* ctx, void* p);
int scratch(rk_ctx* ctx, size_t bytes, void** out);  // valid until the next scratch() call
// host -> device on the ctx stream without waiting: the bytes are staged in the context's page-locked ring, so the
// caller's buffer is free on return (large uploads fall back to copy + wait)
int upload(rk_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int post_launch(rk_ctx* ctx, const char* what);
// a kernel launch on the ctx stream, then post_launch: `what` names the kernel in the error
template <class... P, class... A>
inline int launch(rk_ctx* ctx, const char* what, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, A&&... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, ctx->stream, std::forward<A>(args)...);
    return post_launch(ctx, what);
}
// device -> host on the ctx stream, then wait for the stream: the one way transcript-sized data reaches the host
int d2h_sync(rk_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);

// dev_alloc'd block released with the scope, or caller-owned memory used in place (`adopt`: never freed here)
struct DevBuf {
    rk_ctx* ctx = nullptr;
    void* p = nullptr;
    bool borrowed = false;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : ctx(o.ctx), p(o.p), borrowed(o.borrowed) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        release();
        ctx = o.ctx;
        p = o.p;
        borrowed = o.borrowed;
        o.p = nullptr;
        return *this;
    }
    ~DevBuf() { release(); }
    int alloc(rk_ctx* c, size_t bytes) {
        release();
        ctx = c;
        return dev_alloc(c, bytes, &p);
    }
    void adopt(rk_ctx* c, void* ptr) {
        release();
        ctx = c;
        p = ptr;
        borrowed = true;
    }
    void release() {
        if (p && !borrowed) (void)dev_free(ctx, p);
        p = nullptr;
        borrowed = false;
    }
    uint32_t* u32() const { return (uint32_t*)p; }
};

// NTT (kernels_ntt.hip)
int ntt_reverse(rk_ctx* ctx, uint32_t* d_io, size_t size, size_t count, bool fuse_zk_shift);
int ntt_reverse_from(rk_ctx* ctx, uint32_t* d_dst, const uint32_t* d_src, size_t size, size_t count, bool fuse_zk_shift);
int ntt_forward(rk_ctx* ctx, uint32_t* d_out, const uint32_t* d_in, size_t in_size, size_t count,
                unsigned expand_bits);
int zk_shift(rk_ctx* ctx, uint32_t* d_io, size_t size, size_t count);
int bit_reverse(rk_ctx* ctx, uint32_t* d_io, size_t size, size_t count);

// hashing (kernels_hash.hip)
int hash_rows(rk_ctx* ctx, uint32_t* d_out, const uint32_t* d_matrix, size_t rows, size_t cols);
int hash_fold(rk_ctx* ctx, uint32_t* d_nodes, size_t output_size);
int merkle_build(rk_ctx* ctx, uint32_t* d_nodes, const uint32_t* d_matrix, size_t rows, size_t cols);
// smallest proof-of-work nonce for the transcript generator state h_cells (host, p2 width words)
int pow_grind(rk_ctx* ctx, const uint32_t* h_cells, unsigned bits, uint32_t* nonce);
int duplex_grind(rk_ctx* ctx, const uint32_t* h_state, const uint32_t* h_input, unsigned n_input, unsigned bits, uint32_t* witness);

// polynomial / elementwise (kernels_poly.hip)
int eltwise_add(rk_ctx* ctx, uint32_t* d_out, const uint32_t* a, const uint32_t* b, size_t n);
int eltwise_sum_ext(rk_ctx* ctx, uint32_t* d_out, const uint32_t* d_in, size_t count, size_t to_add);
int eltwise_zeroize(rk_ctx* ctx, uint32_t* d_io, size_t n);
int fri_fold(rk_ctx* ctx, uint32_t* d_out, const uint32_t* d_in, size_t out_count, const bb::Ext& mix);
int fri_fold_evals(rk_ctx* ctx, uint32_t* d_out_ext, const uint32_t* d_in_ext, size_t n_out, const bb::Ext& beta);
int gather_sample(rk_ctx* ctx, uint32_t* d_dst, const uint32_t* d_src, size_t idx, size_t size, size_t stride);
// rows: d_dst[q*cols + c] = d_matrix[c*rows + h_idx[q]]
int gather_rows(rk_ctx* ctx, uint32_t* d_dst, const uint32_t* d_matrix, size_t rows, size_t cols,
                const uint32_t* d_idx, size_t n_idx);
// digests: d_dst[i] = d_nodes[d_idx[i]]
int gather_digests(rk_ctx* ctx, uint32_t* d_dst, const uint32_t* d_nodes, const uint32_t* d_idx, size_t n_idx);
// openings of several trees in two launches: job k gathers rows idx[idx_off .. +n) of its column-major matrix to
// dst[dst_off ..) (n x cols) and, behind them, the digests idx[idx_off + n .. + n * path_len) of its node heap
struct GatherJob {
    const uint32_t* matrix;
    const uint32_t* nodes;
    uint64_t rows, cols, idx_off, dst_off;
    uint32_t n, path_len;
};
int gather_many(rk_ctx* ctx, uint32_t* d_dst, const uint32_t* d_idx, const GatherJob* d_jobs, const GatherJob* h_jobs, size_t n_jobs);
int ext_powers(rk_ctx* ctx, uint32_t* d_pw_ext, const bb::Ext& x, size_t n, bool bit_reversed);
// n_pts tables of n powers each, one launch: table j (at d_pw_ext + j * n * 4) holds h_pts[j]^k
int ext_powers_many(rk_ctx* ctx, uint32_t* d_pw_ext, const bb::Ext* h_pts, size_t n_pts, size_t n, bool bit_reversed);
int bit_reverse_ext(rk_ctx* ctx, uint32_t* d_io_ext, size_t size, size_t count);
// levels of a Merkle tree with <= 1024 parents, fused in one launch (kernels_hash.hip)
// every level from the one with top_output_size (<= HASH_FOLD_TOP_MAX, a power of two) parents up to the root
constexpr size_t HASH_FOLD_TOP_MAX = 4096;
int hash_fold_top(rk_ctx* ctx, uint32_t* d_nodes, size_t top_output_size);
// d_out_ext[e] = sum_k coeffs[which[e]*size + k] * pw[pw_sel[e]*size + k], one launch over several coefficient buffers:
// the evaluations are numbered through the sources in order, the first srcs[0].n of them read srcs[0].d_coeffs, ...
// h_which / h_sel (host, one word per evaluation) are arbitrary: repeats, any order
struct EvalSrc {
    const uint32_t* d_coeffs;
    size_t n;
};
int eval_dot(rk_ctx* ctx, uint32_t* d_out_ext, size_t size, const EvalSrc* srcs, size_t n_srcs, const uint32_t* h_which,
             const uint32_t* h_sel, const uint32_t* d_pw_ext);
// out[h_combos[i]*count + idx] += mix_start * mix^i * in[i*count + idx], the columns i numbered through the sources in
// order (srcs[g].n columns of `count` words at srcs[g].d_in, their combos at srcs[g].h_combos).
// fresh_combos != 0: instead of adding to `out`, every combo below fresh_combos is written once (zero where no column
// names it) and none may be named at or above it
struct MixSrc {
    const uint32_t* d_in;
    const uint32_t* h_combos;
    size_t n;
};
int mix_poly_coeffs(rk_ctx* ctx, uint32_t* d_out_ext, const bb::Ext& mix_start, const bb::Ext& mix, const MixSrc* srcs,
                    size_t n_srcs, size_t count, size_t fresh_combos);
int poly_divide(rk_ctx* ctx, uint32_t* d_poly_ext, size_t count, const bb::Ext& z, bb::Ext* h_rem);
// n_items polynomials of `count` ext coefficients at d_base_ext + h_offsets[i] (in ext elements), each divided
// by (x - h_z[i]) in one batch of launches; remainders to h_rems (may be null)
int poly_divide_many(rk_ctx* ctx, uint32_t* d_base_ext, size_t count, const size_t* h_offsets, const bb::Ext* h_z,
                     size_t n_items, bb::Ext* h_rems, uint32_t* d_rems = nullptr);  // d_rems: n_items x 4 words, no wait
int prefix_products(rk_ctx* ctx, uint32_t* d_io_ext, size_t count);
int scatter(rk_ctx* ctx, uint32_t* d_into, size_t into_words, const uint32_t* h_index, size_t n_cycles,
            const uint32_t* h_offsets, const uint32_t* h_values);
// circuit_program.hip: the step program behind rk_circuit_hooks.program / rk_verify_opts.program
int program_eval_check(const rk_program* prog, const rk_circuit_view* view, const uint32_t poly_mix[4], uint32_t* d_check);
int program_poly_ext(const rk_program* prog, uint32_t wm, const uint32_t poly_mix[4], const uint32_t* eval_u_ext, size_t n_taps,
                     const uint32_t* globals, uint32_t n_globals, const uint32_t* mix, uint32_t n_mix, uint32_t out_ext[4]);
// Plonky3 two-adic PCS steps on row-major matrices (kernels_pcs.hip)
// keep_cols != nullptr: *keep_cols receives the column-major natural-order evaluations (w columns of h << blow-up
// words, a dev_alloc'd block the caller frees) the rows were transposed from
int pcs_coset_lde_rows(rk_ctx* ctx, uint32_t* d_out, const uint32_t* d_in, size_t h, size_t w, uint32_t** keep_cols = nullptr);
// column-major w columns of H words (natural order) -> row-major H x w with row bitrev(j) = index j
int pcs_cols_to_rows_bitrev(rk_ctx* ctx, uint32_t* d_out, const uint32_t* d_cols, size_t H, size_t w);
// cols: d_lde is column-major in natural order (rk_matrix layout 2) instead of row-major with bit-reversed rows
int pcs_eval_at(rk_ctx* ctx, uint32_t* d_out_ext, const uint32_t* d_lde, size_t H, size_t w, const uint32_t* h_points, size_t n_points,
                bool cols = false);
int pcs_reduce_openings(rk_ctx* ctx, uint32_t* d_ro_ext, const uint32_t* d_lde, size_t H, size_t w, size_t n_points,
                        const uint32_t* h_points, const uint32_t* h_ys, const bb::Ext& alpha, uint64_t alpha_offset, bool cols = false);
int pcs_coset_lde_cols(rk_ctx* ctx, uint32_t* d_cols, const uint32_t* d_in, size_t h, size_t w);
// d_ext[idx[i]] -= delta[i]
int ext_sub_at(rk_ctx* ctx, uint32_t* d_ext, const uint32_t* h_idx, const bb::Ext* h_delta, size_t n);

// The contexts an entry point with several proofs in flight keeps per device between calls (session.hip and
// p3_shards.hip, each with a map of its own: their allocator caches and parameter sets differ).
struct CtxPool {
    struct Slot {   // a prover context and the parameter set it was configured with: they come and go together
        rk_ctx* ctx = nullptr;
        std::vector<uint32_t> key;
    };
    std::mutex busy;                 // one run at a time per device (an entry point may be entered from many threads)
    std::vector<Slot> slots;
    rk_ctx* uploader = nullptr;      // stages host-resident inputs ahead of the provers (its own stream)
    // at least n_workers contexts on `device`, the first n_workers carrying `params`: only those whose key differs are
    // configured again, so an equal set costs nothing next time
    int ensure(int device, size_t n_workers, const rk_params* params, const std::vector<uint32_t>& key) {
        while (slots.size() < n_workers) {
            slots.emplace_back();   // first the slot, then its context: a failed push_back would leak one
            const int st = rk_ctx_create(device, nullptr, &slots.back().ctx);
            if (st != RK_OK) {
                slots.pop_back();
                return st;
            }
        }
        for (size_t j = 0; j < n_workers; j++) {
            if (slots[j].key == key) continue;
            RK_TRY(rk_set_params(slots[j].ctx, params));
            slots[j].key = key;
        }
        return RK_OK;
    }
    int ensure_uploader(int device) { return uploader ? RK_OK : rk_ctx_create(device, nullptr, &uploader); }
    void clear() {
        for (Slot& s : slots) (void)rk_ctx_destroy(s.ctx);
        slots.clear();
        if (uploader) (void)rk_ctx_destroy(uploader);
        uploader = nullptr;
    }
    ~CtxPool() { clear(); }
};
// p3_shards.hip: the contexts rk_p3_prove_shards keeps per device (freed by rk_session_release)
void p3_release_pools();

// code_cache.hip: the committed code group of a segment, kept per device and looked up by content
struct CodeKey {
    uint32_t fp[4];                    // keyed fingerprint of the code input's words
    uint32_t po2, cols, blowup_log2, queries;
    uint32_t root27m, shiftm;          // the field parameters the transforms depend on
    uint32_t p2[8];                    // digest of the Poseidon2 instance
    bool operator==(const CodeKey& o) const { return std::memcmp(this, &o, sizeof(CodeKey)) == 0; }
};
struct CodeEntry {                     // what commit_group leaves behind for the code group; device memory of its own
    CodeKey key{};
    int device = 0;
    uint32_t* coeffs = nullptr;        // interpolated, zk-shifted, bit-reversed
    uint32_t* evaluated = nullptr;     // the LDE
    uint32_t* nodes = nullptr;         // the Merkle heap over its rows
    std::vector<uint32_t> top;         // MerkleDev::top
    hipEvent_t ready = nullptr;        // recorded on the building stream once the tree is complete
    size_t bytes = 0;
    CodeEntry() = default;
    CodeEntry(const CodeEntry&) = delete;
    CodeEntry& operator=(const CodeEntry&) = delete;
    ~CodeEntry();
};
// the cache of `device` is on, an input of `words` words can be fingerprinted and an entry of entry_bytes fits
bool code_cache_usable(int device, size_t words, size_t entry_bytes);
// fp = the fingerprint of d_src[0 .. words) (waits for the stream); *canonical: every word was < p
int code_fingerprint(rk_ctx* ctx, const uint32_t* d_src, size_t words, uint32_t fp[4], bool* canonical);
// the key of the code group committed from an input of fingerprint `fp` under the context's parameter set: the shape
// of the group and of its tree's cap, the field parameters of the transforms, the digest of the Poseidon2 instance
CodeKey code_key(const rk_ctx* ctx, uint32_t po2, uint32_t cols, uint32_t queries, const uint32_t fp[4]);
// the entry of `key` (a hit) or null (a miss)
std::shared_ptr<CodeEntry> code_cache_lookup(int device, const CodeKey& key);
// an entry with buffers of the given sizes, not yet in the cache; null when the device has no room for it
std::shared_ptr<CodeEntry> code_cache_new_entry(int device, const CodeKey& key, size_t coeff_bytes, size_t eval_bytes, size_t node_bytes);
// after `ready` was recorded; dropped when the key is already there (two contexts missed at once)
void code_cache_insert(const std::shared_ptr<CodeEntry>& e);
void code_cache_release();

}  // namespace rk
