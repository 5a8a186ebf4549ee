// The Keccak-f[1600] chip (rk_keccak_chip_*, include/raiko_hip.h): the first precompile-shaped table -- its AIR written by
// the library as a step list and its rows written on the GPU.  Layout, constants, lane body and step writer: keccak_chip.hpp.
// The shape is p3-keccak-air's (reference Cargo.lock:5022, the crate itself outside the reference tree: RECALLED).
#include "internal.hpp"
#include "keccak_chip.hpp"

#include <memory>

namespace {

// One wavefront per permutation slot, KC_WAVES slots per block, a grid over the slots: the state is the same in every
// lane, lane z stores bit z of each 64-column bit group (one store of 64 consecutive words per group), the limb / flag /
// multiplicity groups leave as masked stores.  No LDS, no atomics, no cross-lane traffic: the kernel is its HBM writes.
constexpr unsigned KC_WAVES = 4;
__global__ void __launch_bounds__(64 * KC_WAVES) keccak_chip_trace_kernel(kc::KeccakChipArgs a, size_t slots) {
    const size_t slot = (size_t)blockIdx.x * KC_WAVES + (threadIdx.x >> 6);
    if (slot >= slots) return;
    kc::keccak_chip_lane(a, slot, threadIdx.x & 63u);
}

}  // namespace

extern "C" {

uint32_t rk_keccak_chip_width(void) { return kc::KeccakChipLayout::WIDTH; }

int rk_keccak_chip_air(const rk_params* params, uint32_t bus, rk_air** out) {
    RK_GUARD_BEGIN
    if (!out) return RK_ERR_INVALID;
    *out = nullptr;
    rk_params def;
    rk::params_preset(&def, RK_PRESET_SP1);
    const rk_params& par = params ? *params : def;
    rk::Sys sys;
    auto k = std::make_unique<p2::Any>();
    RK_TRY(rk::resolve_params(&par, &sys, k.get()));
    if (bus >= bb::P - 3) return RK_ERR_INVALID;
    using L = kc::KeccakChipLayout;
    std::vector<rk_air_step> steps;
    kc::keccak_chip_steps(steps);
    // receives (bus, bus + 1: ID, the two halves of A) M_IN times and (bus + 2, bus + 3: the same columns) M_OUT times
    std::vector<uint32_t> ix;
    for (uint32_t j = 0; j < 4; j++) {
        ix.insert(ix.end(), {1u, bus + j, 0u, j < 2 ? L::M_IN : L::M_OUT, 51u, L::ID});
        for (uint32_t i = 0; i < 50; i++) ix.push_back(L::a(50 * (j & 1) + i));
    }
    return rk_air_create_lookup(steps.data(), steps.size(), L::WIDTH, 0, ix.data(), 4, ix.size(), par.ext_w, out);
    RK_GUARD_END
}

int rk_keccak_chip_trace(rk_ctx* ctx, const uint64_t* d_states, const uint32_t* d_ids, const uint32_t* d_mult, size_t n, size_t rows,
                         uint32_t* d_trace, uint64_t* d_out) {
    RK_GUARD_BEGIN
    if (!ctx || !d_states || !d_trace || n == 0 || rows < 2 || (rows & (rows - 1)) || rows > ((size_t)1 << 24) || n > rows / 25) return RK_ERR_INVALID;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t slots = (rows + 24) / 25;   // the last one cut off by the table's end
    const kc::KeccakChipArgs a{d_states, d_ids, d_mult, n, rows, d_trace, d_out};
    hipLaunchKernelGGL(keccak_chip_trace_kernel, dim3((unsigned)((slots + KC_WAVES - 1) / KC_WAVES)), dim3(64 * KC_WAVES), 0, ctx->stream, a, slots);
    return rk::post_launch(ctx, "keccak_chip_trace_kernel");
    RK_GUARD_END
}

}  // extern "C"
