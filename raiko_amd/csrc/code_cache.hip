// The committed code group, kept per device and looked up by content.
//
// The code (control) columns of a segment are a function of the circuit and of po2 alone -- risc0's verifier checks
// the code root against a fixed table of control IDs, one per po2 -- so their interpolation, zk shift, LDE and Merkle
// tree come out the same for every segment of one size.  prove_segment (prover.hip) fingerprints the code input it is
// given on the device, and when the device already holds the committed group of that input under the same parameters
// it borrows coefficients, LDE, tree and top layer instead of computing them again.
//
// Nothing here trusts an address or a caller's word: the fingerprint reads every word of the input on every call.  It
// is the bilinear form  sum_i m[i] * a[i mod 4096] * b[i / 4096]  over the extension field (p^4 ~ 2^123.6) with two
// tables of uniform extension elements drawn once per process; for two different inputs of canonical words the
// difference is a non-zero polynomial of degree 2 in the table entries, so they collide with probability <= 2 / p^4
// < 2^-122 (Schwartz-Zippel).  An input with a word >= p has no such bound (m and m + p agree mod p) and is committed
// the ordinary way, as is one longer than the b table covers.
//
// Entries are allocated with hipMalloc, not from a context's pool, and are reference-counted: a context may be
// destroyed, or the entry evicted, while other contexts still read it.  LRU by bytes.
#include "internal.hpp"

#include <cstdlib>
#include <list>
#include <mutex>
#include <random>

namespace rk {

namespace {

constexpr unsigned FP_CHUNK = 4096;            // words per entry of b; a has one entry per word of a chunk
constexpr unsigned FP_TPB = 256;
constexpr unsigned FP_PER_LANE = FP_CHUNK / FP_TPB;   // 16 words: 4 x uint4
constexpr size_t FP_MAX_CHUNKS = (size_t)1 << 16;     // b: 1 MiB, inputs of up to 2^28 words (1 GiB)
constexpr unsigned FP_MAX_BLOCKS = 1024;
constexpr unsigned FP_PART = 8;                // words per block in the partial buffer: ext sum, flag, padding

// part[8 b .. 8 b + 4) = sum over the chunks j of block b of (sum_k m[4096 j + k] * a[k]) * tb[j];  part[8 b + 4] != 0
// when one of its words was >= p.  Lane t holds a[4 (t + 256 q) + e] for q, e < 4 in registers for all its chunks.
__global__ __launch_bounds__(FP_TPB) void code_fingerprint_kernel(uint32_t* __restrict__ part, const uint32_t* __restrict__ m,
                                                                  size_t words, const uint32_t* __restrict__ ta,
                                                                  const uint32_t* __restrict__ tb, uint32_t wm, int vec) {
    const unsigned t = threadIdx.x;
    uint32_t a[FP_PER_LANE][4];
#pragma unroll
    for (unsigned q = 0; q < 4; q++)
#pragma unroll
        for (unsigned e = 0; e < 4; e++) {
            const uint4 v = ((const uint4*)ta)[4 * (t + FP_TPB * q) + e];
            a[4 * q + e][0] = v.x, a[4 * q + e][1] = v.y, a[4 * q + e][2] = v.z, a[4 * q + e][3] = v.w;
        }
    bb::Ext tot = bb::ext_zero();
    uint32_t bad = 0;
    const size_t chunks = (words + FP_CHUNK - 1) / FP_CHUNK;
    for (size_t j = blockIdx.x; j < chunks; j += gridDim.x) {
        const size_t base = j * FP_CHUNK;
        uint32_t w[FP_PER_LANE];
        if (vec && base + FP_CHUNK <= words) {
#pragma unroll
            for (unsigned q = 0; q < 4; q++) {
                const uint4 v = ((const uint4*)(m + base))[t + FP_TPB * q];
                w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
            }
        } else {  // the last, partial chunk, or an input that is not 16-byte aligned
#pragma unroll
            for (unsigned q = 0; q < 4; q++)
#pragma unroll
                for (unsigned e = 0; e < 4; e++) {
                    const size_t i = base + 4 * (t + FP_TPB * q) + e;
                    w[4 * q + e] = i < words ? m[i] : 0u;
                }
        }
        bb::Ext s;
#pragma unroll
        for (unsigned c = 0; c < 4; c++) {
            uint32_t acc = 0;
            // two products of values < p stay below 2^32 p, the range of one Montgomery reduction
#pragma unroll
            for (unsigned k = 0; k < FP_PER_LANE; k += 2)
                acc = bb::add(acc, bb::mont_reduce((uint64_t)w[k] * a[k][c] + (uint64_t)w[k + 1] * a[k + 1][c]));
            s.c[c] = acc;
        }
#pragma unroll
        for (unsigned k = 0; k < FP_PER_LANE; k++) bad |= w[k] >= bb::P ? 1u : 0u;
        const uint4 bv = ((const uint4*)tb)[j];
        tot = bb::add(tot, bb::mul(s, bb::Ext{{bv.x, bv.y, bv.z, bv.w}}, wm));
    }
    __shared__ uint32_t red[FP_TPB][5];
#pragma unroll
    for (unsigned c = 0; c < 4; c++) red[t][c] = tot.c[c];
    red[t][4] = bad;
    __syncthreads();
    for (unsigned h = FP_TPB / 2; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (unsigned c = 0; c < 4; c++) red[t][c] = bb::add(red[t][c], red[t + h][c]);
            red[t][4] |= red[t + h][4];
        }
        __syncthreads();
    }
    if (t < 5) part[(size_t)blockIdx.x * FP_PART + t] = red[0][t];
}

struct DevCache {
    std::mutex mu;
    std::list<std::shared_ptr<CodeEntry>> lru;  // front: used last
    size_t bytes = 0, max_bytes = 0;
    uint64_t hits = 0, misses = 0;
    uint32_t* d_tables = nullptr;  // a (FP_CHUNK ext) then b (FP_MAX_CHUNKS ext)
};

std::mutex g_mu;
// never destroyed: entries own device memory, and the HIP runtime may be gone when static destructors run
std::map<int, DevCache*>* g_caches = nullptr;

size_t default_bytes() {
    static const size_t v = [] {
        const char* e = std::getenv("RK_CODE_CACHE_BYTES");
        if (e && *e) return (size_t)std::strtoull(e, nullptr, 0);
        return (size_t)2 << 30;
    }();
    return v;
}

DevCache* cache_of(int device) {
    std::lock_guard<std::mutex> l(g_mu);
    if (!g_caches) g_caches = new std::map<int, DevCache*>();
    DevCache*& c = (*g_caches)[device];
    if (!c) {
        c = new DevCache();
        c->max_bytes = default_bytes();
    }
    return c;
}

// the key of the fingerprint: drawn once per process, the same on every device
const std::vector<uint32_t>& fp_tables() {
    static const std::vector<uint32_t> t = [] {
        std::random_device rd;
        std::seed_seq seq{rd(), rd(), rd(), rd(), rd(), rd(), rd(), rd()};
        std::mt19937_64 gen(seq);
        std::uniform_int_distribution<uint32_t> uni(0, bb::P - 1);
        std::vector<uint32_t> v((FP_CHUNK + FP_MAX_CHUNKS) * 4);
        for (uint32_t& x : v) x = uni(gen);
        return v;
    }();
    return t;
}

}  // namespace

CodeEntry::~CodeEntry() {
    // hipFree waits for the device: no kernel of a finished proof still reads the buffers (holders drop their
    // reference only after their last stream synchronisation)
    if (coeffs) (void)hipFree(coeffs);
    if (evaluated) (void)hipFree(evaluated);
    if (nodes) (void)hipFree(nodes);
    if (ready) (void)hipEventDestroy(ready);
}

bool code_cache_usable(int device, size_t words, size_t entry_bytes) {
    if (words == 0 || (words + FP_CHUNK - 1) / FP_CHUNK > FP_MAX_CHUNKS) return false;
    DevCache* c = cache_of(device);
    std::lock_guard<std::mutex> l(c->mu);
    return c->max_bytes != 0 && entry_bytes <= c->max_bytes;
}

int code_fingerprint(rk_ctx* ctx, const uint32_t* d_src, size_t words, uint32_t fp[4], bool* canonical) {
    DevCache* c = cache_of(ctx->device);
    const uint32_t* d_tables = nullptr;
    {
        std::lock_guard<std::mutex> l(c->mu);
        if (!c->d_tables) {
            const std::vector<uint32_t>& h = fp_tables();
            RK_HIP_TRY(ctx, hipMalloc((void**)&c->d_tables, h.size() * 4));
            if (hipMemcpy(c->d_tables, h.data(), h.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
                (void)hipFree(c->d_tables);
                c->d_tables = nullptr;
                ctx->last_error = "hipMemcpy of the fingerprint tables failed";
                return RK_ERR_HIP;
            }
        }
        d_tables = c->d_tables;
    }
    const size_t chunks = (words + FP_CHUNK - 1) / FP_CHUNK;
    const unsigned blocks = (unsigned)(chunks < FP_MAX_BLOCKS ? chunks : FP_MAX_BLOCKS);
    void* d_part = nullptr;
    RK_TRY(dev_alloc(ctx, (size_t)blocks * FP_PART * 4, &d_part));
    int st;
    {
        KTimer kt(ctx, RK_KCLASS_POLY, (double)words * 4);
        hipLaunchKernelGGL(code_fingerprint_kernel, dim3(blocks), dim3(FP_TPB), 0, ctx->stream, (uint32_t*)d_part, d_src, words, d_tables,
                           d_tables + (size_t)FP_CHUNK * 4, ctx->sys.wm, ((uintptr_t)d_src & 15) == 0 ? 1 : 0);
        st = post_launch(ctx, "code_fingerprint_kernel");
    }
    std::vector<uint32_t> h((size_t)blocks * FP_PART);
    if (st == RK_OK) {
        hipError_t e = hipMemcpyAsync(h.data(), d_part, h.size() * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            ctx->last_error = std::string("code fingerprint: ") + hipGetErrorString(e);
            st = RK_ERR_HIP;
        }
    }
    (void)dev_free(ctx, d_part);
    RK_TRY(st);
    bb::Ext sum = bb::ext_zero();
    uint32_t bad = 0;
    for (unsigned b = 0; b < blocks; b++) {
        const uint32_t* p = &h[(size_t)b * FP_PART];
        sum = bb::add(sum, bb::Ext{{p[0], p[1], p[2], p[3]}});
        bad |= p[4];
    }
    for (int i = 0; i < 4; i++) fp[i] = sum.c[i];
    *canonical = bad == 0;
    return RK_OK;
}

CodeKey code_key(const rk_ctx* ctx, uint32_t po2, uint32_t cols, uint32_t queries, const uint32_t fp[4]) {
    CodeKey key{};
    std::memcpy(key.fp, fp, sizeof key.fp);
    key.po2 = po2;
    key.cols = cols;
    key.blowup_log2 = ctx->sys.blowup_log2;
    key.queries = queries;  // the layer sent as the tree's cap depends on it
    key.root27m = ctx->sys.root27m;
    key.shiftm = ctx->sys.shiftm;
    const p2::Any& kc = ctx->h_p2;
    std::vector<uint32_t> inst{bb::encode((uint32_t)kc.kind), bb::encode(kc.pad_free ? 1u : 0u)};
    inst.insert(inst.end(), kc.rc_ext(), kc.rc_ext() + 8 * kc.cells());
    inst.insert(inst.end(), kc.rc_int(), kc.rc_int() + kc.rounds_partial());
    inst.insert(inst.end(), kc.diag(), kc.diag() + kc.cells());
    kc.hash_elems(inst.data(), inst.size(), key.p2);
    return key;
}

std::shared_ptr<CodeEntry> code_cache_lookup(int device, const CodeKey& key) {
    DevCache* c = cache_of(device);
    std::lock_guard<std::mutex> l(c->mu);
    for (auto it = c->lru.begin(); it != c->lru.end(); ++it) {
        if (!((*it)->key == key)) continue;
        c->lru.splice(c->lru.begin(), c->lru, it);
        c->hits++;
        return c->lru.front();
    }
    c->misses++;
    return nullptr;
}

std::shared_ptr<CodeEntry> code_cache_new_entry(int device, const CodeKey& key, size_t coeff_bytes, size_t eval_bytes, size_t node_bytes) {
    auto e = std::make_shared<CodeEntry>();
    e->key = key;
    e->device = device;
    e->bytes = coeff_bytes + eval_bytes + node_bytes;
    if (hipMalloc((void**)&e->coeffs, coeff_bytes) != hipSuccess || hipMalloc((void**)&e->evaluated, eval_bytes) != hipSuccess ||
        hipMalloc((void**)&e->nodes, node_bytes) != hipSuccess || hipEventCreateWithFlags(&e->ready, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();  // no room for an entry: the group is committed in the context's own buffers
        return nullptr;
    }
    return e;
}

void code_cache_insert(const std::shared_ptr<CodeEntry>& e) {
    DevCache* c = cache_of(e->device);
    std::vector<std::shared_ptr<CodeEntry>> evicted;  // freed after the lock is dropped: hipFree waits for the device
    {
        std::lock_guard<std::mutex> l(c->mu);
        if (c->max_bytes == 0 || e->bytes > c->max_bytes) return;
        for (const auto& o : c->lru)
            if (o->key == e->key) return;  // another context built the same group meanwhile: the first insert wins
        while (!c->lru.empty() && c->bytes + e->bytes > c->max_bytes) {
            c->bytes -= c->lru.back()->bytes;
            evicted.push_back(std::move(c->lru.back()));
            c->lru.pop_back();
        }
        c->lru.push_front(e);
        c->bytes += e->bytes;
    }
}

void code_cache_release() {
    std::vector<DevCache*> all;
    {
        std::lock_guard<std::mutex> l(g_mu);
        if (g_caches)
            for (auto& kv : *g_caches) all.push_back(kv.second);
    }
    for (DevCache* c : all) {
        std::list<std::shared_ptr<CodeEntry>> gone;
        std::lock_guard<std::mutex> l(c->mu);
        gone.swap(c->lru);
        c->bytes = 0;
        // the fingerprint tables (1 MiB) stay for the life of the process: a proof on a context of the caller's own may
        // be about to launch with them
    }
}

}  // namespace rk

extern "C" {

int rk_code_cache_configure(int device, size_t max_bytes) {
    RK_GUARD_BEGIN
    if (device < 0) return RK_ERR_INVALID;
    rk::DevCache* c = rk::cache_of(device);
    std::vector<std::shared_ptr<rk::CodeEntry>> evicted;
    std::lock_guard<std::mutex> l(c->mu);
    c->max_bytes = max_bytes;
    while (!c->lru.empty() && c->bytes > max_bytes) {
        c->bytes -= c->lru.back()->bytes;
        evicted.push_back(std::move(c->lru.back()));
        c->lru.pop_back();
    }
    return RK_OK;
    RK_GUARD_END
}

int rk_code_cache_stats(int device, uint64_t* hits, uint64_t* misses, uint64_t* bytes) {
    RK_GUARD_BEGIN
    if (device < 0) return RK_ERR_INVALID;
    rk::DevCache* c = rk::cache_of(device);
    std::lock_guard<std::mutex> l(c->mu);
    if (hits) *hits = c->hits;
    if (misses) *misses = c->misses;
    if (bytes) *bytes = c->bytes;
    return RK_OK;
    RK_GUARD_END
}

}  // extern "C"
