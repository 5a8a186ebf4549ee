// The Keccak-256 sponge table (rk_keccak_sponge_*, include/raiko_hip.h) over the Keccak-f[1600] chip: its AIR written by the
// library as a step list, its rows written on the GPU by two kernels -- the states of every message's dependent chain of
// permutations first, then the rows, which no longer depend on each other.  Layout, lane body and step writer:
// keccak_sponge.hpp.
#include "internal.hpp"
#include "keccak_sponge.hpp"

#include <memory>

namespace {

// The states kernel: one wavefront per message, KS_CHAIN_WAVES messages per block.  Lane i < 25 holds lane i = x + 5 y of
// the state -- one 64-bit register pair, not 25 --; theta's column parities, pi's permuted read and chi's row neighbours
// come through cross-lane reads (__shfl: ds_bpermute_b32 twice per 64-bit value), rho rotates by a per-lane amount.
// Lanes 25..63 follow lane 0's indices and store nothing.  No LDS, no atomics; every shuffle runs under a wave-uniform
// condition.  Per block: xor the 17 rate lanes in, store the permutation's input, permute, store its output.
constexpr unsigned KS_CHAIN_WAVES = 4;
__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t from) { return (uint64_t)__shfl((unsigned long long)v, (int)from); }
__global__ void __launch_bounds__(64 * KS_CHAIN_WAVES)
keccak_sponge_chain_kernel(const uint64_t* __restrict__ blocks, const uint32_t* __restrict__ first, size_t n_msgs, size_t n_blocks,
                           uint64_t* __restrict__ states, uint64_t* __restrict__ outs, uint64_t* __restrict__ digests) {
    const size_t m = (size_t)blockIdx.x * KS_CHAIN_WAVES + (threadIdx.x >> 6);
    if (m >= n_msgs) return;   // the whole wavefront
    const uint32_t lane = threadIdx.x & 63u, i = lane < 25 ? lane : 0u, x = i % 5, row = i - x;
    const uint32_t up1 = (i + 5) % 25, up2 = (i + 10) % 25, up3 = (i + 15) % 25, up4 = (i + 20) % 25;
    const uint32_t left = (x + 4) % 5, right = (x + 1) % 5;             // row 0 holds every column's parity as well as any row
    const uint32_t from = kc::pi_from(i), chi1 = (x + 1) % 5 + row, chi2 = (x + 2) % 5 + row;
    uint32_t rot = 0;
#pragma unroll
    for (uint32_t k = 0; k < 25; k++) rot = from == k ? kc::ROT[k] : rot;
    const size_t begin = first[m], end = first[m + 1] < n_blocks ? first[m + 1] : n_blocks;
    uint64_t a = 0;
    for (size_t b = begin; b < end; b++) {
        if (lane < kc::KeccakSpongeLayout::RATE_LANES) a ^= blocks[kc::KeccakSpongeLayout::RATE_LANES * b + lane];
        if (lane < 25) states[25 * b + lane] = a;
#pragma unroll
        for (uint32_t r = 0; r < 24; r++) {
            const uint64_t c = a ^ shfl64(a, up1) ^ shfl64(a, up2) ^ shfl64(a, up3) ^ shfl64(a, up4);
            const uint64_t cr = shfl64(c, right);
            a ^= shfl64(c, left) ^ ((cr << 1) | (cr >> 63));
            const uint64_t t = shfl64(a, from);
            const uint64_t bb_ = (t << rot) | (t >> ((64u - rot) & 63u));
            a = bb_ ^ (~shfl64(bb_, chi1) & shfl64(bb_, chi2));
            if (lane == 0) a ^= kc::RC[r];
        }
        if (lane < 25) outs[25 * b + lane] = a;
    }
    if (lane < 4) digests[4 * m + lane] = a;
}

// The rows kernel: one wavefront per block slot, KS_WAVES slots per block, a grid over the slots -- the store pattern of
// keccak_chip_trace_kernel: lane z stores bit z of each 64-column bit group, the limb and flag groups leave as masked
// stores.  No LDS, no atomics, no cross-lane traffic.
constexpr unsigned KS_WAVES = 4;
__global__ void __launch_bounds__(64 * KS_WAVES) keccak_sponge_rows_kernel(kc::KeccakSpongeArgs a, size_t slots) {
    const size_t slot = (size_t)blockIdx.x * KS_WAVES + (threadIdx.x >> 6);
    if (slot >= slots) return;
    kc::keccak_sponge_lane(a, slot, threadIdx.x & 63u);
}

}  // namespace

extern "C" {

uint32_t rk_keccak_sponge_width(void) { return kc::KeccakSpongeLayout::WIDTH; }
uint32_t rk_keccak_sponge_rows_per_block(void) { return kc::KeccakSpongeLayout::ROWS; }

int rk_keccak_sponge_air(const rk_params* params, uint32_t bus, rk_air** out) {
    RK_GUARD_BEGIN
    if (!out) return RK_ERR_INVALID;
    *out = nullptr;
    rk_params def;
    rk::params_preset(&def, RK_PRESET_SP1);
    const rk_params& par = params ? *params : def;
    rk::Sys sys;
    auto k = std::make_unique<p2::Any>();
    RK_TRY(rk::resolve_params(&par, &sys, k.get()));
    if (bus >= bb::P - 6) return RK_ERR_INVALID;
    using L = kc::KeccakSpongeLayout;
    std::vector<rk_air_step> steps;
    kc::keccak_sponge_steps(steps);
    // sends: (PID, half of V) to the chip, S_IN times on bus, bus + 1 and S_OUT times on bus + 2, bus + 3; the block as
    // (MSG, BLK, half of its 68 limbs) S_MSG times on bus + 4, bus + 5; (MSG, NBLK, the 16 digest limbs) S_DIG times on bus + 6
    std::vector<uint32_t> ix;
    for (uint32_t j = 0; j < 4; j++) {
        ix.insert(ix.end(), {0u, bus + j, 0u, j < 2 ? L::S_IN : L::S_OUT, 51u, L::PID});
        for (uint32_t i = 0; i < 50; i++) ix.push_back(L::v(50 * (j & 1) + i));
    }
    for (uint32_t j = 0; j < 2; j++) {
        ix.insert(ix.end(), {0u, bus + 4 + j, 0u, L::S_MSG, 36u, L::MSG, L::BLK});
        for (uint32_t i = 0; i < 34; i++) ix.push_back(L::v(34 * j + i));
    }
    ix.insert(ix.end(), {0u, bus + 6, 0u, L::S_DIG, 18u, L::MSG, L::NBLK});
    for (uint32_t i = 0; i < 16; i++) ix.push_back(L::v(i));
    return rk_air_create_lookup(steps.data(), steps.size(), L::WIDTH, 0, ix.data(), 7, ix.size(), par.ext_w, out);
    RK_GUARD_END
}

int rk_keccak_sponge_trace(rk_ctx* ctx, const uint64_t* d_blocks, const uint32_t* d_first, const uint32_t* d_msg_ids, size_t n_msgs, size_t n_blocks,
                           size_t rows, uint32_t* d_trace, uint64_t* d_states, uint64_t* d_outs, uint64_t* d_digests) {
    RK_GUARD_BEGIN
    using L = kc::KeccakSpongeLayout;
    if (!ctx || !d_blocks || !d_first || !d_trace || !d_states || !d_outs || !d_digests || n_msgs == 0 || n_blocks == 0 || n_msgs > n_blocks) return RK_ERR_INVALID;
    if (rows < 2 || (rows & (rows - 1)) || rows > ((size_t)1 << 24) || n_blocks > rows / L::ROWS) return RK_ERR_INVALID;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(keccak_sponge_chain_kernel, dim3((unsigned)((n_msgs + KS_CHAIN_WAVES - 1) / KS_CHAIN_WAVES)), dim3(64 * KS_CHAIN_WAVES), 0,
                       ctx->stream, d_blocks, d_first, n_msgs, n_blocks, d_states, d_outs, d_digests);
    RK_TRY(rk::post_launch(ctx, "keccak_sponge_chain_kernel"));
    const size_t slots = (rows + L::ROWS - 1) / L::ROWS;   // the last one cut off by the table's end
    const kc::KeccakSpongeArgs a{d_blocks, d_first, d_msg_ids, d_states, d_outs, n_msgs, n_blocks, rows, d_trace};
    hipLaunchKernelGGL(keccak_sponge_rows_kernel, dim3((unsigned)((slots + KS_WAVES - 1) / KS_WAVES)), dim3(64 * KS_WAVES), 0, ctx->stream, a, slots);
    return rk::post_launch(ctx, "keccak_sponge_rows_kernel");
    RK_GUARD_END
}

}  // extern "C"
