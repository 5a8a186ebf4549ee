// Poseidon2 row hashing and Merkle folds (Hal::hash_rows / Hal::hash_fold and
// MerkleTreeProver::new of risc0-zkp 1.0.1).  Integer-ALU-bound: one lane owns one
// sponge (24 state words in VGPRs), consecutive lanes own consecutive rows so every
// column load is a coalesced 256-byte wave access of the column-major matrix.
#include <algorithm>
#include <cstring>

#include "cell_perm.hpp"
#include "internal.hpp"

namespace {

constexpr int HASH_BLOCK = 256;
// levels with at most this many parents go cell-parallel (hash_fold_top): a cell-parallel permutation costs ~6x the
// lane-cycles of a lane-per-parent one, so it only pays where the level is latency-bound anyway
constexpr size_t CELLS_MAX_OUT = rk::HASH_FOLD_TOP_MAX;

// C = the configured p2::Core (width 24 or 16, external 4x4 block): one kernel instance per Core and sponge kind.
// PAD_FREE: the last partial block leaves the remaining rate cells as they are (Plonky3
// PaddingFreeSponge) instead of zero-padding them (risc0); an empty row then takes no permutation.
//
// A row ends with a partial block (zero-padded: also the one block of an empty row), which takes the full
// permutation, or with a whole block, of which only the digest is read.  The blocks before that only hand their
// capacity on, the next block overwrites the rate -- except before a padding-free partial block, which keeps rate
// cells of its predecessor: such a row takes the full permutation throughout.  Every path runs one loop and then
// one permutation, so that no 24-cell state has to be merged between two inlined permutations.
template <class C, bool PAD_FREE>
__global__ __launch_bounds__(HASH_BLOCK, 5) void hash_rows_kernel(uint32_t* __restrict__ out,
                                                               const uint32_t* __restrict__ matrix, size_t rows,
                                                               uint32_t cols, const typename C::Consts* __restrict__ kc) {
    size_t row = (size_t)blockIdx.x * HASH_BLOCK + threadIdx.x;
    if (row >= rows) return;
    const typename C::Consts& k = *kc;
    uint32_t s[C::CELLS];
#pragma unroll
    for (int i = 0; i < C::CELLS; i++) s[i] = 0;
    const uint32_t full = cols / C::RATE, rem = cols - full * C::RATE;
    // a column's address is a wave-uniform pointer plus the lane
    const uint32_t* src = matrix + (size_t)blockIdx.x * HASH_BLOCK;
    const unsigned lane = threadIdx.x;
    auto load_block = [&](uint32_t b) {
#pragma unroll
        for (int i = 0; i < C::RATE; i++) s[i] = (src + (size_t)(b * C::RATE + i) * rows)[lane];
    };
    if (rem != 0 || (cols == 0 && !PAD_FREE)) {
        for (uint32_t b = 0; b < full; b++) {
            load_block(b);
            if constexpr (PAD_FREE) C::permute(s, k);
            else C::template permute<C::RATE, p2::OUT>(s, k);
        }
#pragma unroll
        for (int i = 0; i < C::RATE; i++) {
            if ((uint32_t)i < rem) s[i] = (src + (size_t)(full * C::RATE + i) * rows)[lane];
            else if (!PAD_FREE) s[i] = 0u;
        }
        C::permute(s, k);
    } else if (full != 0) {
        for (uint32_t b = 0; b + 1 < full; b++) {
            load_block(b);
            C::template permute<C::RATE, p2::OUT>(s, k);
        }
        load_block(full - 1);
        C::template permute<0, p2::OUT>(s, k);
    }
    uint4* o = reinterpret_cast<uint4*>(out + (size_t)blockIdx.x * HASH_BLOCK * p2::OUT) + 2 * lane;
    o[0] = make_uint4(s[0], s[1], s[2], s[3]);
    o[1] = make_uint4(s[4], s[5], s[6], s[7]);
}

// nodes[out_size + i] = H(nodes[2*(out_size+i)] || nodes[2*(out_size+i)+1]): the two digests fill
// cells 0..15, the rest of a wider state is zero; the parent is the first 8 cells
template <class C>
__global__ __launch_bounds__(HASH_BLOCK) void hash_fold_kernel(uint32_t* __restrict__ nodes, size_t out_size,
                                                               const typename C::Consts* __restrict__ kc) {
    size_t i = (size_t)blockIdx.x * HASH_BLOCK + threadIdx.x;
    if (i >= out_size) return;
    const typename C::Consts& k = *kc;
    size_t idx = out_size + i;
    const uint4* in = reinterpret_cast<const uint4*>(nodes + 2 * idx * p2::OUT);
    uint4 a = in[0], b = in[1], c = in[2], d = in[3];
    uint32_t s[C::CELLS];
    s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w; s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
    s[8] = c.x; s[9] = c.y; s[10] = c.z; s[11] = c.w; s[12] = d.x; s[13] = d.y; s[14] = d.z; s[15] = d.w;
#pragma unroll
    for (int j = 16; j < C::CELLS; j++) s[j] = 0;
    C::template permute<0, p2::OUT, 16>(s, k);
    uint4* o = reinterpret_cast<uint4*>(nodes + idx * p2::OUT);
    o[0] = make_uint4(s[0], s[1], s[2], s[3]);
    o[1] = make_uint4(s[4], s[5], s[6], s[7]);
}

// `levels` (<= CELLS_MAX_LEVELS) levels of a tree in one launch: workgroup b owns the 2^levels nodes
// [b 2^levels, (b + 1) 2^levels) of the level with 2 first_out nodes and everything above them; a level lives
// in LDS (ping-pong) between steps and every parent also goes to its heap slot.  blockDim = 32 lanes per
// parent of the first step (at most 512: a workgroup then has at most two waves per SIMD).
constexpr unsigned CELLS_MAX_LEVELS = 5;
template <class C>
__global__ __launch_bounds__(512) void hash_fold_cells_kernel(uint32_t* __restrict__ nodes, unsigned first_out, unsigned levels,
                                                               const typename C::Consts* __restrict__ kc) {
    __shared__ uint32_t buf[2][(1u << CELLS_MAX_LEVELS) * p2::OUT];
    const typename C::Consts& k = *kc;
    const unsigned tid = threadIdx.x, b = blockIdx.x;
    const unsigned nhw = blockDim.x >> 5, h = tid >> 5, cell = tid & 31u;
    const unsigned in_cnt = 1u << levels;
    for (unsigned i = tid; i < in_cnt * p2::OUT; i += blockDim.x)
        buf[0][i] = nodes[((size_t)2 * first_out + (size_t)b * in_cnt) * p2::OUT + i];
    CellPerm<C> cp;
    cp.init(k, cell);
    __syncthreads();
    for (unsigned l = 0; l < levels; l++) {
        const unsigned cnt = in_cnt >> (l + 1);
        const size_t out_base = (size_t)(first_out >> l) + (size_t)b * cnt;
        const uint32_t* src = buf[l & 1];
        uint32_t* dst = buf[(l + 1) & 1];
        for (unsigned t0 = 0; t0 < cnt; t0 += nhw) {  // uniform trip count: idle half-waves redo parent 0 and drop it
            const unsigned t = t0 + h;
            const bool valid = t < cnt;
            const unsigned tt = valid ? t : 0u;
            uint32_t x = cell < 2 * p2::OUT ? src[2 * tt * p2::OUT + cell] : 0u;
            x = cp.permute(x, k);
            if (valid && cell < (unsigned)p2::OUT) {
                dst[t * p2::OUT + cell] = x;
                nodes[(out_base + t) * p2::OUT + cell] = x;
            }
        }
        __syncthreads();
    }
}

// Proof of work on the transcript: candidate w = base + lane.  digest = hash([w]) (one block of the
// sponge), the generator absorbs it (cells[0..8) += digest, permute) and the next four outputs,
// decoded and xor-ed, must be zero in their low `bits` bits -- exactly what Transcript::commit and
// p2::Rng::random_bits do with pool_used = 0.  The smallest hit of the launch wins (atomicMin).
template <class C>
__global__ __launch_bounds__(HASH_BLOCK) void pow_grind_kernel(uint32_t* __restrict__ best, const uint32_t* __restrict__ cells,
                                                               uint32_t base, uint32_t count, uint32_t mask,
                                                               const typename C::Consts* __restrict__ kc) {
    const uint32_t gid = blockIdx.x * HASH_BLOCK + threadIdx.x;
    if (gid >= count) return;
    const typename C::Consts& k = *kc;
    const uint32_t w = base + gid;
    uint32_t s[C::CELLS];
    s[0] = w;
#pragma unroll
    for (int i = 1; i < C::CELLS; i++) s[i] = 0;
    C::template permute<0, p2::OUT, 1>(s, k);
    uint32_t c[C::CELLS];
#pragma unroll
    for (int i = 0; i < C::CELLS; i++) c[i] = cells[i];
#pragma unroll
    for (int i = 0; i < p2::OUT; i++) c[i] = bb::add(c[i], s[i]);
    C::template permute<0, 4>(c, k);  // the four outputs random_bits draws
    const uint32_t v = bb::decode(c[0]) ^ bb::decode(c[1]) ^ bb::decode(c[2]) ^ bb::decode(c[3]);
    if ((v & mask) == 0) atomicMin(best, w);
}

// Plonky3 DuplexChallenger::grind (p3-challenger duplex_challenger.rs + grinding_challenger.rs, RECALLED): candidate
// w = base + lane is observed on a copy of the challenger -- it joins the buffered inputs, which overwrite the first
// cells of the sponge state, and whether the push fills the rate or the following sample forces it, exactly one
// permutation runs before sample_bits pops the last rate cell of the new state.  Smallest hit wins.
template <class C>
__global__ __launch_bounds__(HASH_BLOCK) void duplex_grind_kernel(uint32_t* __restrict__ best, const uint32_t* __restrict__ state,
                                                                  unsigned n_input, uint32_t base, uint32_t count, uint32_t mask,
                                                                  const typename C::Consts* __restrict__ kc) {
    const uint32_t gid = blockIdx.x * HASH_BLOCK + threadIdx.x;
    if (gid >= count) return;
    const uint32_t w = base + gid;
    uint32_t s[C::CELLS];
#pragma unroll
    for (int i = 0; i < C::CELLS; i++) s[i] = (unsigned)i == n_input ? bb::mul(w, bb::R2) : state[i];  // state already holds the buffered inputs
    C::template permute<(C::RATE - 1) / 4 * 4, 4>(s, *kc);  // the block of the last rate cell
    if ((bb::decode(s[C::RATE - 1]) & mask) == 0) atomicMin(best, w);
}

// run F<Core> for the context's Poseidon2 instance
#define RK_P2_DISPATCH(ctx, CALL)                         \
    switch ((ctx)->h_p2.kind) {                           \
        case 0: { using C = p2::K0; CALL; } break;        \
        case 1: { using C = p2::K1; CALL; } break;        \
        case 2: { using C = p2::K2; CALL; } break;        \
        default: { using C = p2::K3; CALL; } break;       \
    }

}  // namespace

namespace rk {

int hash_rows(rk_ctx* ctx, uint32_t* d_out, const uint32_t* d_matrix, size_t rows, size_t cols) {
    if (rows == 0) return RK_ERR_INVALID;
    size_t blocks = (rows + HASH_BLOCK - 1) / HASH_BLOCK;
    if (blocks > 0x7fffffffu || cols > 0x7fffffffu) return RK_ERR_INVALID;
    KTimer kt(ctx, RK_KCLASS_HASH_ROWS, (double)rows * cols * 4 + (double)rows * 32);
    if (ctx->h_p2.pad_free) {
        RK_P2_DISPATCH(ctx, hipLaunchKernelGGL((hash_rows_kernel<C, true>), dim3((unsigned)blocks), dim3(HASH_BLOCK), 0, ctx->stream,
                                               d_out, d_matrix, rows, (uint32_t)cols, (const typename C::Consts*)ctx->d_p2));
    } else {
        RK_P2_DISPATCH(ctx, hipLaunchKernelGGL((hash_rows_kernel<C, false>), dim3((unsigned)blocks), dim3(HASH_BLOCK), 0, ctx->stream,
                                               d_out, d_matrix, rows, (uint32_t)cols, (const typename C::Consts*)ctx->d_p2));
    }
    return post_launch(ctx, "hash_rows_kernel");
}

int hash_fold(rk_ctx* ctx, uint32_t* d_nodes, size_t output_size) {
    if (output_size == 0) return RK_ERR_INVALID;
    size_t blocks = (output_size + HASH_BLOCK - 1) / HASH_BLOCK;
    if (blocks > 0x7fffffffu) return RK_ERR_INVALID;
    KTimer kt(ctx, RK_KCLASS_HASH_FOLD, (double)output_size * 96);
    RK_P2_DISPATCH(ctx, hipLaunchKernelGGL(hash_fold_kernel<C>, dim3((unsigned)blocks), dim3(HASH_BLOCK), 0, ctx->stream, d_nodes,
                                           output_size, (const typename C::Consts*)ctx->d_p2));
    return post_launch(ctx, "hash_fold_kernel");
}

int merkle_build(rk_ctx* ctx, uint32_t* d_nodes, const uint32_t* d_matrix, size_t rows, size_t cols) {
    if (!is_pow2(rows)) return RK_ERR_INVALID;
    RK_TRY(hash_rows(ctx, d_nodes + rows * p2::OUT, d_matrix, rows, cols));
    size_t layer = rows / 2;
    for (; layer > CELLS_MAX_OUT; layer /= 2) RK_TRY(hash_fold(ctx, d_nodes, layer));
    if (layer >= 1) RK_TRY(hash_fold_top(ctx, d_nodes, layer));
    return RK_OK;
}

int pow_grind(rk_ctx* ctx, const uint32_t* h_cells, unsigned bits, uint32_t* nonce) {
    if (bits == 0 || bits > 24 || !h_cells || !nonce) return RK_ERR_INVALID;
    const unsigned width = (unsigned)ctx->h_p2.cells();
    void* d = nullptr;
    RK_TRY(scratch(ctx, (p2::MAX_CELLS + 4) * 4, &d));
    uint32_t* d_cells = (uint32_t*)d;
    uint32_t* d_best = d_cells + p2::MAX_CELLS;
    uint32_t host[p2::MAX_CELLS + 1] = {0};
    std::memcpy(host, h_cells, width * 4);
    host[p2::MAX_CELLS] = 0xffffffffu;
    RK_HIP_TRY(ctx, hipMemcpyAsync(d, host, sizeof host, hipMemcpyHostToDevice, ctx->stream));
    RK_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // `host` is a stack buffer
    // 2^(bits + 2) candidates per launch: four hits expected, so one launch almost always; candidates run
    // up to p (a nonce is a field element), far beyond what 24 bits need
    const uint64_t batch = (uint64_t)1 << (bits + 2 < 16 ? 16 : bits + 2);
    const uint32_t mask = (uint32_t)(((uint64_t)1 << bits) - 1);
    for (uint64_t base = 0; base < bb::P; base += batch) {
        const uint32_t count = (uint32_t)std::min<uint64_t>(batch, bb::P - base);
        const unsigned blocks = (count + HASH_BLOCK - 1) / HASH_BLOCK;
        RK_P2_DISPATCH(ctx, hipLaunchKernelGGL(pow_grind_kernel<C>, dim3(blocks), dim3(HASH_BLOCK), 0, ctx->stream, d_best, d_cells,
                                               (uint32_t)base, count, mask, (const typename C::Consts*)ctx->d_p2));
        RK_TRY(post_launch(ctx, "pow_grind_kernel"));
        uint32_t best = 0;
        RK_HIP_TRY(ctx, hipMemcpyAsync(&best, d_best, 4, hipMemcpyDeviceToHost, ctx->stream));
        RK_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (best != 0xffffffffu) {
            *nonce = best;
            return RK_OK;
        }
    }
    return RK_ERR_INTERNAL;
}

int duplex_grind(rk_ctx* ctx, const uint32_t* h_state, const uint32_t* h_input, unsigned n_input, unsigned bits, uint32_t* witness) {
    const unsigned width = (unsigned)ctx->h_p2.cells(), rate = width - p2::OUT;
    if (bits == 0 || bits > 24 || !h_state || !witness || n_input >= rate || (n_input && !h_input)) return RK_ERR_INVALID;
    uint32_t host[p2::MAX_CELLS + 1] = {0};
    std::memcpy(host, h_state, width * 4);
    if (n_input) std::memcpy(host, h_input, n_input * 4);  // duplexing overwrites the first cells with the buffered inputs
    for (unsigned i = 0; i < width; i++)
        if (host[i] >= bb::P) return RK_ERR_INVALID;
    host[p2::MAX_CELLS] = 0xffffffffu;
    void* d = nullptr;
    RK_TRY(scratch(ctx, sizeof host, &d));
    uint32_t* d_cells = (uint32_t*)d;
    uint32_t* d_best = d_cells + p2::MAX_CELLS;
    RK_TRY(upload(ctx, d, host, sizeof host));
    const uint64_t batch = (uint64_t)1 << (bits + 2 < 16 ? 16 : bits + 2);
    const uint32_t mask = (uint32_t)(((uint64_t)1 << bits) - 1);
    for (uint64_t base = 0; base < bb::P; base += batch) {
        const uint32_t count = (uint32_t)std::min<uint64_t>(batch, bb::P - base);
        const unsigned blocks = (count + HASH_BLOCK - 1) / HASH_BLOCK;
        RK_P2_DISPATCH(ctx, hipLaunchKernelGGL(duplex_grind_kernel<C>, dim3(blocks), dim3(HASH_BLOCK), 0, ctx->stream, d_best, d_cells,
                                               n_input, (uint32_t)base, count, mask, (const typename C::Consts*)ctx->d_p2));
        RK_TRY(post_launch(ctx, "duplex_grind_kernel"));
        uint32_t best = 0;
        RK_HIP_TRY(ctx, hipMemcpyAsync(&best, d_best, 4, hipMemcpyDeviceToHost, ctx->stream));
        RK_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (best != 0xffffffffu) {
            *witness = best;
            return RK_OK;
        }
    }
    return RK_ERR_INTERNAL;
}

// every level from the one with `top_output_size` parents up to the root, cell-parallel, a few levels per launch
int hash_fold_top(rk_ctx* ctx, uint32_t* d_nodes, size_t top_output_size) {
    if (!is_pow2(top_output_size) || top_output_size > CELLS_MAX_OUT) return RK_ERR_INVALID;
    unsigned remaining = 1;  // levels left, the root's included
    for (size_t n = top_output_size; n > 1; n >>= 1) remaining++;
    unsigned first_out = (unsigned)top_output_size;
    while (remaining) {
        // the last launch is one workgroup: four levels keep it at one wave per SIMD (eight parents first); the
        // launches below it take up to five levels each, split evenly
        unsigned m = std::min(remaining, 4u);
        if (remaining > 4) {
            const unsigned rest = remaining - 4, k = (rest + 4) / 5;
            m = (rest + k - 1) / k;
        }
        const unsigned blocks = (2 * first_out) >> m;
        const unsigned threads = std::max(64u, 32u << (m - 1));  // m <= CELLS_MAX_LEVELS: at most 512
        KTimer kt(ctx, RK_KCLASS_HASH_FOLD, (double)blocks * ((1u << m) - 1) * 96);
        RK_P2_DISPATCH(ctx, hipLaunchKernelGGL(hash_fold_cells_kernel<C>, dim3(blocks), dim3(threads), 0, ctx->stream, d_nodes,
                                               first_out, m, (const typename C::Consts*)ctx->d_p2));
        RK_TRY(post_launch(ctx, "hash_fold_cells_kernel"));
        first_out >>= m;
        remaining -= m;
    }
    return RK_OK;
}

}  // namespace rk

extern "C" {

int rk_hash_rows(rk_ctx* ctx, uint32_t* d_out, const uint32_t* d_matrix, size_t rows, size_t cols) {
    RK_GUARD_BEGIN
    if (!ctx || !d_out || (!d_matrix && cols)) return RK_ERR_INVALID;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return rk::hash_rows(ctx, d_out, d_matrix, rows, cols);
    RK_GUARD_END
}
int rk_hash_fold(rk_ctx* ctx, uint32_t* d_nodes, size_t input_size, size_t output_size) {
    RK_GUARD_BEGIN
    if (!ctx || !d_nodes || input_size != 2 * output_size) return RK_ERR_INVALID;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return rk::hash_fold(ctx, d_nodes, output_size);
    RK_GUARD_END
}
int rk_pow_grind(rk_ctx* ctx, const uint32_t* sponge_cells, uint32_t bits, uint32_t* nonce) {
    RK_GUARD_BEGIN
    if (!ctx || !sponge_cells || !nonce) return RK_ERR_INVALID;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return rk::pow_grind(ctx, sponge_cells, bits, nonce);
    RK_GUARD_END
}
int rk_duplex_grind(rk_ctx* ctx, const uint32_t* sponge_state, const uint32_t* input_buffer, uint32_t n_input, uint32_t bits,
                    uint32_t* witness) {
    RK_GUARD_BEGIN
    if (!ctx || !sponge_state || !witness) return RK_ERR_INVALID;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return rk::duplex_grind(ctx, sponge_state, input_buffer, n_input, bits, witness);
    RK_GUARD_END
}
int rk_merkle_build(rk_ctx* ctx, uint32_t* d_nodes, const uint32_t* d_matrix, size_t rows, size_t cols) {
    RK_GUARD_BEGIN
    if (!ctx || !d_nodes || !d_matrix) return RK_ERR_INVALID;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return rk::merkle_build(ctx, d_nodes, d_matrix, rows, cols);
    RK_GUARD_END
}

}  // extern "C"
