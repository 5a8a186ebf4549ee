// The Keccak-256 padding table (rk_keccak_pad_*, include/raiko_hip.h) under the sponge table: its AIR written by the library
// as a step list, the padded blocks and its rows written on the GPU.  Layout, kernel bodies and step writer: keccak_pad.hpp.
#include "internal.hpp"
#include "keccak_pad.hpp"

#include <memory>

namespace {

// The blocks kernel: one thread per 32-bit word slot of d_blocks, a wavefront reading 64 consecutive words of a message
// and storing 64 consecutive words.  A thread finds its message by bisection of d_first (a wavefront spans at most three
// blocks, so nearly always one message).  No LDS, no atomics, no cross-lane traffic.
constexpr unsigned KP_BLOCKS_THREADS = 256;
__global__ void __launch_bounds__(KP_BLOCKS_THREADS) keccak_pad_blocks_kernel(kc::KeccakPadArgs a) {
    kc::keccak_pad_block_word(a, (size_t)blockIdx.x * KP_BLOCKS_THREADS + threadIdx.x);
}

// The rows kernel: one wavefront per block slot, KP_WAVES slots per block, a grid over the ceil(rows / 34) slots.  A row is
// 167 words: three stores of consecutive words by the whole wavefront (the last masked to 39 lanes), 34 rows a slot; what
// a row holds is wave-uniform but for the column, and d_first is bisected once a slot.  Padding slots write zero rows, the
// slot the table's end cuts stops at `rows`.  No LDS, no atomics, no cross-lane traffic.  (A wavefront per ROW was
// measured first: every wavefront then waits for its own bisection before its three stores, 98 us at 4096 one-block
// messages against 60 us at one message)
constexpr unsigned KP_WAVES = 4;
__global__ void __launch_bounds__(64 * KP_WAVES) keccak_pad_rows_kernel(kc::KeccakPadArgs a, size_t slots) {
    const size_t slot = (size_t)blockIdx.x * KP_WAVES + (threadIdx.x >> 6);
    if (slot >= slots) return;
    kc::keccak_pad_lane(a, slot, threadIdx.x & 63u);
}

// The digests kernel: 16 threads a message, each one word of D on the message's last row.
constexpr unsigned KP_DIGEST_THREADS = 256;
__global__ void __launch_bounds__(KP_DIGEST_THREADS)
keccak_pad_digests_kernel(const uint64_t* __restrict__ digests, const uint32_t* __restrict__ first, size_t n_msgs, size_t n_blocks, size_t rows,
                          uint32_t* __restrict__ trace) {
    kc::keccak_pad_digest_word(digests, first, n_msgs, n_blocks, rows, trace, (size_t)blockIdx.x * KP_DIGEST_THREADS + threadIdx.x);
}

bool pad_shape_ok(size_t n_msgs, size_t n_blocks, size_t rows) {
    if (n_msgs == 0 || n_msgs > n_blocks) return false;
    return !(rows & (rows - 1)) && rows <= ((size_t)1 << 24) && n_blocks <= rows / kc::KeccakPadLayout::ROWS;
}

}  // namespace

extern "C" {

uint32_t rk_keccak_pad_width(void) { return kc::KeccakPadLayout::WIDTH; }
uint32_t rk_keccak_pad_rows_per_block(void) { return kc::KeccakPadLayout::ROWS; }

int rk_keccak_pad_air(const rk_params* params, uint32_t bus, rk_air** out) {
    RK_GUARD_BEGIN
    if (!out) return RK_ERR_INVALID;
    *out = nullptr;
    rk_params def;
    rk::params_preset(&def, RK_PRESET_SP1);
    const rk_params& par = params ? *params : def;
    rk::Sys sys;
    auto k = std::make_unique<p2::Any>();
    RK_TRY(rk::resolve_params(&par, &sys, k.get()));
    if (bus >= bb::P - 8) return RK_ERR_INVALID;
    using L = kc::KeccakPadLayout;
    std::vector<rk_air_step> steps;
    kc::keccak_pad_steps(steps);
    // receives, the sponge's three sends: the block as (MSG, BLK, half of B) STEP[33] times on bus + 4, bus + 5 and (MSG,
    // NBLK, D) S_END times on bus + 6; sends: (MSG, IDX, W_LO, W_HI) R times on bus + 7, (MSG, LEN, D) S_END times on bus + 8
    std::vector<uint32_t> ix;
    for (uint32_t j = 0; j < 2; j++) {
        ix.insert(ix.end(), {1u, bus + 4 + j, 0u, L::step(33), 36u, L::MSG, L::BLK});
        for (uint32_t i = 0; i < 34; i++) ix.push_back(L::b(34 * j + i));
    }
    ix.insert(ix.end(), {1u, bus + 6, 0u, L::S_END, 18u, L::MSG, L::NBLK});
    for (uint32_t i = 0; i < 16; i++) ix.push_back(L::d(i));
    ix.insert(ix.end(), {0u, bus + 7, 0u, L::R, 4u, L::MSG, L::IDX, L::W_LO, L::W_HI});
    ix.insert(ix.end(), {0u, bus + 8, 0u, L::S_END, 18u, L::MSG, L::LEN});
    for (uint32_t i = 0; i < 16; i++) ix.push_back(L::d(i));
    return rk_air_create_lookup(steps.data(), steps.size(), L::WIDTH, 0, ix.data(), 5, ix.size(), par.ext_w, out);
    RK_GUARD_END
}

int rk_keccak_pad_trace(rk_ctx* ctx, const uint32_t* d_words, size_t n_words, const uint32_t* d_word_first, const uint32_t* d_lens,
                        const uint32_t* d_first, const uint32_t* d_msg_ids, size_t n_msgs, size_t n_blocks, size_t rows, uint32_t* d_trace,
                        uint64_t* d_blocks) {
    RK_GUARD_BEGIN
    using L = kc::KeccakPadLayout;
    if (!ctx || !d_words || !d_word_first || !d_lens || !d_first || !d_trace || !d_blocks || !pad_shape_ok(n_msgs, n_blocks, rows)) return RK_ERR_INVALID;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const kc::KeccakPadArgs a{d_words, d_word_first, d_lens, d_first, d_msg_ids, n_words, n_msgs, n_blocks, rows, reinterpret_cast<uint32_t*>(d_blocks), d_trace};
    const size_t slots = n_blocks * L::ROWS;
    hipLaunchKernelGGL(keccak_pad_blocks_kernel, dim3((unsigned)((slots + KP_BLOCKS_THREADS - 1) / KP_BLOCKS_THREADS)), dim3(KP_BLOCKS_THREADS), 0, ctx->stream, a);
    RK_TRY(rk::post_launch(ctx, "keccak_pad_blocks_kernel"));
    const size_t row_slots = (rows + L::ROWS - 1) / L::ROWS;   // the last one cut off by the table's end
    hipLaunchKernelGGL(keccak_pad_rows_kernel, dim3((unsigned)((row_slots + KP_WAVES - 1) / KP_WAVES)), dim3(64 * KP_WAVES), 0, ctx->stream, a, row_slots);
    return rk::post_launch(ctx, "keccak_pad_rows_kernel");
    RK_GUARD_END
}

int rk_keccak_pad_digests(rk_ctx* ctx, const uint64_t* d_digests, const uint32_t* d_first, size_t n_msgs, size_t n_blocks, size_t rows, uint32_t* d_trace) {
    RK_GUARD_BEGIN
    if (!ctx || !d_digests || !d_first || !d_trace || !pad_shape_ok(n_msgs, n_blocks, rows)) return RK_ERR_INVALID;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = 16 * n_msgs;
    hipLaunchKernelGGL(keccak_pad_digests_kernel, dim3((unsigned)((n + KP_DIGEST_THREADS - 1) / KP_DIGEST_THREADS)), dim3(KP_DIGEST_THREADS), 0, ctx->stream,
                       d_digests, d_first, n_msgs, n_blocks, rows, d_trace);
    return rk::post_launch(ctx, "keccak_pad_digests_kernel");
    RK_GUARD_END
}

}  // extern "C"
