// The cell-parallel Poseidon2 permutation (CellPerm) and its DPP helpers: shared by kernels_hash.hip (the top levels of a
// Merkle tree) and fri_tables.hip (the Fiat-Shamir chain of the transcript table), where a run of dependent permutations
// is bound by the latency of one.
#pragma once
#include "internal.hpp"

namespace {

// ---- cell-parallel permutation: one 32-lane half-wave per permutation, one lane per cell --------------
// The levels near the root have too few parents to fill the chip, so a lane-per-permutation launch costs the
// latency of one permutation (~6.7 k dependent instructions, ~15 us) per level whatever its size.  Here the
// 24 (16) cells of one state sit in consecutive lanes, values canonical Montgomery residues:
//   * S-boxes run in all lanes at once (full rounds) or are kept by cell 0 only (partial rounds);
//   * external layer circ(2 M4, M4, ...): out = M4 (x_quad + X), X_j = sum over quads of cell j -- the quad
//     sums are two row rotations (DPP row_ror:4/8) and one exchange of the two 16-lane rows
//     (v_permlane16_swap, gfx950), the 4x4 product takes its operands by DPP quad broadcasts and
//     accumulates exactly in 64 bits (< 16 p), one REDC and one product by 2^64 bring it back;
//   * internal layer: the cell sum is a 5-step DPP reduction, then x_i = d_i x_i + S.
// ~40 dependent instructions per round instead of ~230, nothing goes through LDS.  Lanes beyond the width
// hold zero between layers so that they do not disturb the sums.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
constexpr int DPP_ROR1 = 0x121, DPP_ROR2 = 0x122, DPP_ROR4 = 0x124, DPP_ROR8 = 0x128;
constexpr int DPP_Q0 = 0x00, DPP_Q1 = 0x55, DPP_Q2 = 0xaa, DPP_Q3 = 0xff;
// lane i + lane (i ^ 16), both < p: the sum of the two rows of a half-wave, canonical
__device__ __forceinline__ uint32_t row_pair_sum(uint32_t v) {
    auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return bb::ucanon(r[0] + r[1]);
}
constexpr uint32_t R2_NQ = bb::R2 * (0u - bb::MPRIME);  // bb::umul_const companion of 2^64 mod p

template <class C>
struct CellPerm {
    static constexpr int W = C::CELLS;
    uint32_t m0, m1, m2, m3;  // this lane's row of the 4x4 block
    uint32_t diag;
    uint32_t rc[2 * p2::ROUNDS_HALF_FULL];  // rc - p of this cell, per full round
    unsigned cell;
    bool active;

    __device__ __forceinline__ void init(const typename C::Consts& k, unsigned cell_) {
        cell = cell_;
        active = cell < (unsigned)W;
        const unsigned j = cell & 3u;
        // rows of the block, one nibble per coefficient (see m_ext_redc)
        const uint32_t pk = C::M4_KIND == 0 ? (j == 0 ? 0x3175u : j == 1 ? 0x1164u : j == 2 ? 0x7531u : 0x6411u)
                                            : (j == 0 ? 0x1132u : j == 1 ? 0x1321u : j == 2 ? 0x3211u : 0x2113u);
        m0 = pk & 15u;
        m1 = (pk >> 4) & 15u;
        m2 = (pk >> 8) & 15u;
        m3 = pk >> 12;
        diag = active ? k.diag[cell] : 0u;
#pragma unroll
        for (int r = 0; r < 2 * p2::ROUNDS_HALF_FULL; r++) rc[r] = (active ? k.rc_ext[r * W + cell] : 0u) - bb::P;
    }
    __device__ __forceinline__ uint32_t ext(uint32_t x) const {
        uint32_t X = bb::ucanon(x + dpp_mov<DPP_ROR4>(x));
        X = bb::ucanon(X + dpp_mov<DPP_ROR8>(X));
        X = row_pair_sum(X);
        const uint32_t z = bb::ucanon(x + X);
        uint64_t w = (uint64_t)dpp_mov<DPP_Q0>(z) * m0;
        w += (uint64_t)dpp_mov<DPP_Q1>(z) * m1;
        w += (uint64_t)dpp_mov<DPP_Q2>(z) * m2;
        w += (uint64_t)dpp_mov<DPP_Q3>(z) * m3;
        // w < 16 p: REDC gives w / 2^32 (< p + 8), the product by 2^64 / 2^32 restores w mod p
        const uint32_t u = bb::ucanon(bb::umul_const(bb::uredc64(w), bb::R2, R2_NQ));
        return active ? u : 0u;
    }
    __device__ __forceinline__ uint32_t internal(uint32_t x, uint32_t rc_mp) const {
        const uint32_t y = bb::sbox7_add(x, rc_mp);
        x = cell == 0 ? y : x;
        uint32_t s = bb::ucanon(x + dpp_mov<DPP_ROR1>(x));
        s = bb::ucanon(s + dpp_mov<DPP_ROR2>(s));
        s = bb::ucanon(s + dpp_mov<DPP_ROR4>(s));
        s = bb::ucanon(s + dpp_mov<DPP_ROR8>(s));
        s = row_pair_sum(s);
        const uint32_t r = bb::add(bb::mul(x, diag), s);
        return active ? r : 0u;
    }
    // x: this lane's cell (canonical, zero beyond the width); every lane of the wave must be here
    __device__ __forceinline__ uint32_t permute(uint32_t x, const typename C::Consts& k) const {
        x = ext(x);
#pragma unroll
        for (int r = 0; r < p2::ROUNDS_HALF_FULL; r++) x = ext(bb::sbox7_add(x, rc[r]));
        // unrolled: the round constants are wave-uniform scalar loads, which a rolled loop would wait for one by one
#pragma unroll
        for (int r = 0; r < C::ROUNDS_PARTIAL; r++) x = internal(x, k.rc_int_mp[r]);
#pragma unroll
        for (int r = p2::ROUNDS_HALF_FULL; r < 2 * p2::ROUNDS_HALF_FULL; r++) x = ext(bb::sbox7_add(x, rc[r]));
        return x;
    }
};

}  // namespace
