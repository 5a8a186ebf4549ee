// The Keccak-f[1600] chip (rk_keccak_chip_*, include/raiko_hip.h), HIP-free: where its columns are (KeccakChipLayout), the
// round constants / rotation offsets / pi map, the lane body of the rows kernel (keccak_chip.hip; tests/emul runs the same
// code on the CPU one emulated lane at a time) and the step-list writer of its AIR.  The shape is p3-keccak-air's (pulled
// by the reference's Cargo.lock, outside the reference tree: RECALLED, parity unpinned; the columns are this project's).
#pragma once
#include <map>
#include <tuple>
#include <type_traits>
#include <vector>

#include "bb.hpp"
#include "../../include/raiko_hip.h"

namespace kc {

// ---- one row = one round; 25 rows = one permutation (rows 0..23 the rounds, row 24 the output row: a round with round
// constant 0 whose results nobody reads, there so that the output stands in the columns A the input stood in).
// Lane (x, y) of the state has index i = x + 5 y; a lane is four 16-bit limbs (little endian) or 64 bit columns.
struct KeccakChipLayout {
    static constexpr uint32_t ROWS = 25;
    RK_HD static constexpr uint32_t step(uint32_t r) { return r; }                          // STEP[25]: one-hot round flags
    RK_HD static constexpr uint32_t a(uint32_t j) { return 25 + j; }                        // A: the state entering the row, limb j = 4 i + limb
    RK_HD static constexpr uint32_t c(uint32_t x, uint32_t z) { return 125 + 64 * x + z; }  // C[5][64]: column parities
    RK_HD static constexpr uint32_t cp(uint32_t x, uint32_t z) { return 445 + 64 * x + z; } // C'[5][64]: after theta's rotation and xor
    RK_HD static constexpr uint32_t ap(uint32_t i, uint32_t z) { return 765 + 64 * i + z; } // A'[25][64]: the state after theta
    RK_HD static constexpr uint32_t app(uint32_t j) { return 2365 + j; }                    // A'': the state after rho, pi, chi, limb j
    RK_HD static constexpr uint32_t app00_bit(uint32_t z) { return 2465 + z; }              // the bits of A''[0][0]
    RK_HD static constexpr uint32_t appp00(uint32_t l) { return 2529 + l; }                 // A'''[0][0]: lane (0, 0) after iota, limbs
    static constexpr uint32_t ID = 2533, M = 2534, M_IN = 2535, M_OUT = 2536, WIDTH = 2537; // M_IN = M STEP[0], M_OUT = M STEP[24]
};

constexpr uint64_t RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
    0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800Aull, 0x800000008000000Aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
// rho: lane i = x + 5 y is rotated left by ROT[i]; pi moves it to lane y + 5 ((2 x + 3 y) mod 5)
constexpr uint32_t ROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
// the lane pi moves to place i: place (X, Y) takes lane (x, y) = ((X + 3 Y) mod 5, X)
RK_HD constexpr uint32_t pi_from(uint32_t i) { return (i % 5 + 3 * (i / 5)) % 5 + 5 * (i % 5); }

RK_HD uint64_t rol64(uint64_t v, uint32_t n) { return n ? (v << n) | (v >> (64 - n)) : v; }

// ---- the rows (rk_keccak_chip_trace): one wavefront per permutation slot, every lane carrying the same state; lane z
// takes bit z of a 64-column bit group, so every such group leaves as one store of 64 consecutive words
struct KeccakChipArgs {
    const uint64_t* states;   // n x 25 lanes
    const uint32_t* ids;      // n Montgomery words, or null: the slot's number
    const uint32_t* mult;     // n Montgomery words, or null: ones
    size_t n, rows;           // permutations; rows of the table (slots past n: the zero state with M = ID = 0)
    uint32_t* trace;          // rows x WIDTH Montgomery words
    uint64_t* out;            // null, or n x 25 lanes: the permutations' outputs
};
// s[i], i < 25, with an index the compiler does not know: a tree of selects over the five bits of i, so the state stays
// in registers and a lane needs five conditions, not twenty-five (they are loop-invariant and live in scalar registers)
RK_HD uint64_t pick(const uint64_t (&s)[25], uint32_t i) {
    uint64_t t[32];
#pragma unroll
    for (uint32_t k = 0; k < 32; k++) t[k] = k < 25 ? s[k] : 0;
#pragma unroll
    for (uint32_t b = 0; b < 5; b++) {
        const bool hi = (i >> b) & 1u;
#pragma unroll
        for (uint32_t k = 0; k < (16u >> b); k++) t[k] = hi ? t[2 * k + 1] : t[2 * k];
    }
    return t[0];
}
RK_HD uint32_t limb_word(uint64_t lane, uint32_t l) { return bb::encode((uint32_t)(lane >> (16 * l)) & 0xffffu); }
RK_HD uint32_t bit_word(uint64_t lane, uint32_t z) { return (lane >> z) & 1u ? bb::ONE : 0u; }
RK_HD uint64_t rc_of(uint32_t r) {   // 0 on the output row
    uint64_t w = 0;
#pragma unroll
    for (uint32_t k = 0; k < 24; k++) w = r == k ? RC[k] : w;
    return w;
}
// theta, rho, pi, chi of the state a: the column parities c, c' = c ^ c[x-1] ^ rol(c[x+1], 1), a' = a ^ c ^ c' and a'' (before iota)
RK_HD void round_values(const uint64_t (&a)[25], uint64_t (&c)[5], uint64_t (&cp)[5], uint64_t (&ap)[25], uint64_t (&app)[25]) {
#pragma unroll
    for (uint32_t x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
    for (uint32_t x = 0; x < 5; x++) cp[x] = c[x] ^ c[(x + 4) % 5] ^ rol64(c[(x + 1) % 5], 1);
#pragma unroll
    for (uint32_t i = 0; i < 25; i++) ap[i] = a[i] ^ c[i % 5] ^ cp[i % 5];
    uint64_t b[25];
#pragma unroll
    for (uint32_t i = 0; i < 25; i++) b[i] = rol64(ap[pi_from(i)], ROT[pi_from(i)]);
#pragma unroll
    for (uint32_t i = 0; i < 25; i++) app[i] = b[i] ^ (~b[(i + 1) % 5 + 5 * (i / 5)] & b[(i + 2) % 5 + 5 * (i / 5)]);
}
// lane `lane` (0..63) of the wavefront that writes permutation slot `slot`: its share of the slot's rows that lie in the table
RK_HD void keccak_chip_lane(const KeccakChipArgs& g, size_t slot, uint32_t lane) {
    using L = KeccakChipLayout;
    const bool real = slot < g.n;
    uint64_t a[25];
#pragma unroll
    for (uint32_t i = 0; i < 25; i++) a[i] = real ? g.states[25 * slot + i] : 0;
    const uint32_t id = real ? (g.ids ? g.ids[slot] : bb::encode((uint32_t)slot)) : 0u;
    const uint32_t m = real ? (g.mult ? g.mult[slot] : bb::ONE) : 0u;
#pragma unroll 1
    for (uint32_t r = 0; r < L::ROWS; r++) {
        const size_t at = L::ROWS * slot + r;
        if (at >= g.rows) break;   // the table's end cuts the last slot off
        uint32_t* row = g.trace + at * L::WIDTH;
        if (r == 24 && real && g.out && lane < 25) g.out[25 * slot + lane] = pick(a, lane);
        // STEP | A: columns 0..124
#pragma unroll
        for (uint32_t k = 0; k < 2; k++) {
            const uint32_t col = lane + 64 * k;
            if (col < 25) row[col] = col == r ? bb::ONE : 0u;
            else if (col < 125) row[col] = limb_word(pick(a, (col - 25) >> 2), (col - 25) & 3);
        }
        uint64_t c[5], cp[5], ap[25], app[25];
        round_values(a, c, cp, ap, app);
#pragma unroll
        for (uint32_t x = 0; x < 5; x++) row[L::c(x, lane)] = bit_word(c[x], lane);
#pragma unroll
        for (uint32_t x = 0; x < 5; x++) row[L::cp(x, lane)] = bit_word(cp[x], lane);
#pragma unroll
        for (uint32_t i = 0; i < 25; i++) row[L::ap(i, lane)] = bit_word(ap[i], lane);
#pragma unroll
        for (uint32_t k = 0; k < 2; k++) {
            const uint32_t j = lane + 64 * k;
            if (j < 100) row[L::app(j)] = limb_word(pick(app, j >> 2), j & 3);
        }
        row[L::app00_bit(lane)] = bit_word(app[0], lane);
        const uint64_t a3 = app[0] ^ rc_of(r);
        // A'''00 | ID | M | M_IN | M_OUT
        if (lane < 4) row[L::appp00(lane)] = limb_word(a3, lane);
        else if (lane < 8) row[L::ID + (lane - 4)] = lane == 4 ? id : lane == 5 || (lane == 6 && r == 0) || (lane == 7 && r == 24) ? m : 0u;
#pragma unroll
        for (uint32_t i = 0; i < 25; i++) a[i] = app[i];
        a[0] = a3;
    }
}

// ---- the AIR as a step list (rk_keccak_chip_air): a value is shared within one constraint only -- every constraint's
// sub-expressions stand right before its assert, so the evaluator keeps few values alive
struct StepGen {
    std::vector<rk_air_step>& steps;
    uint32_t nv = 0;
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, uint32_t> memo;
    uint32_t push(uint32_t op, uint32_t a = 0, uint32_t b = 0) {
        const auto key = std::make_tuple(op, a, b);
        auto it = memo.find(key);
        if (it != memo.end()) return it->second;
        steps.push_back(rk_air_step{op, a, b});
        memo.emplace(key, nv);
        return nv++;
    }
    void assert_zero(uint32_t v) {
        steps.push_back(rk_air_step{RK_AIR_ASSERT_ZERO, v, 0});
        memo.clear();
    }
    uint32_t add(uint32_t a, uint32_t b) { return push(RK_AIR_ADD, a, b); }
    uint32_t sub(uint32_t a, uint32_t b) { return push(RK_AIR_SUB, a, b); }
    uint32_t mul(uint32_t a, uint32_t b) { return push(RK_AIR_MUL, a, b); }
    uint32_t cst(uint32_t canon) { return push(RK_AIR_CONST, canon); }
    uint32_t col(uint32_t c) { return push(RK_AIR_LOCAL, c); }
    uint32_t nxt(uint32_t c) { return push(RK_AIR_NEXT, c); }
    uint32_t dbl(uint32_t a) { return add(a, a); }
    uint32_t xor2(uint32_t a, uint32_t b) { return sub(add(a, b), dbl(mul(a, b))); }   // a + b - 2 a b
    void assert_bool(uint32_t c) {
        const uint32_t v = col(c);
        assert_zero(mul(v, sub(v, cst(1))));
    }
};
// the sum of 2^k bit_k over 16 bit expressions, from the top
template <class F>
inline uint32_t limb_of_bits(StepGen& g, F&& bit) {
    uint32_t acc = bit(15);
    for (int k = 14; k >= 0; k--) {
        const uint32_t b = bit((uint32_t)k);
        acc = g.add(g.dbl(acc), b);
    }
    return acc;
}
inline void keccak_chip_steps(std::vector<rk_air_step>& steps) {
    using L = KeccakChipLayout;
    StepGen g{steps};
    // the flags: one-hot, STEP[0] on the first row, STEP[i] -> the next row's STEP[i + 1 mod 25]
    for (uint32_t r = 0; r < 25; r++) g.assert_bool(L::step(r));
    {
        uint32_t sum = g.col(L::step(0));
        for (uint32_t r = 1; r < 25; r++) sum = g.add(sum, g.col(L::step(r)));
        g.assert_zero(g.sub(sum, g.cst(1)));
    }
    g.assert_zero(g.mul(g.push(RK_AIR_IS_FIRST_ROW), g.sub(g.col(L::step(0)), g.cst(1))));
    for (uint32_t r = 0; r < 25; r++) g.assert_zero(g.mul(g.push(RK_AIR_IS_TRANSITION), g.sub(g.col(L::step(r)), g.nxt(L::step((r + 1) % 25)))));
    // the bit columns
    for (uint32_t x = 0; x < 5; x++)
        for (uint32_t z = 0; z < 64; z++) g.assert_bool(L::c(x, z));
    for (uint32_t i = 0; i < 25; i++)
        for (uint32_t z = 0; z < 64; z++) g.assert_bool(L::ap(i, z));
    for (uint32_t z = 0; z < 64; z++) g.assert_bool(L::app00_bit(z));
    // C'[x][z] = C[x][z] ^ C[x-1][z] ^ C[x+1][z-1]
    for (uint32_t x = 0; x < 5; x++)
        for (uint32_t z = 0; z < 64; z++) {
            const uint32_t v = g.xor2(g.xor2(g.col(L::c(x, z)), g.col(L::c((x + 4) % 5, z))), g.col(L::c((x + 1) % 5, (z + 63) % 64)));
            g.assert_zero(g.sub(g.col(L::cp(x, z)), v));
        }
    // every limb of A is recomposed from A' ^ C ^ C'
    for (uint32_t i = 0; i < 25; i++)
        for (uint32_t l = 0; l < 4; l++) {
            const uint32_t v = limb_of_bits(g, [&](uint32_t k) {
                const uint32_t z = 16 * l + k;
                return g.xor2(g.xor2(g.col(L::c(i % 5, z)), g.col(L::cp(i % 5, z))), g.col(L::ap(i, z)));
            });
            g.assert_zero(g.sub(g.col(L::a(4 * i + l)), v));
        }
    // C' is the parity of A''s columns: d = sum_y A'[y][x][z] - C'[x][z] is 0, 2 or 4
    for (uint32_t x = 0; x < 5; x++)
        for (uint32_t z = 0; z < 64; z++) {
            uint32_t d = g.col(L::ap(x, z));
            for (uint32_t y = 1; y < 5; y++) d = g.add(d, g.col(L::ap(x + 5 * y, z)));
            d = g.sub(d, g.col(L::cp(x, z)));
            g.assert_zero(g.mul(g.mul(d, g.sub(d, g.cst(2))), g.sub(d, g.cst(4))));
        }
    // every limb of A'' is recomposed from b ^ (~b1 & b2), b the rho / pi-permuted bits of A'
    auto b_bit = [&](uint32_t i, uint32_t z) { return g.col(L::ap(pi_from(i), (z + 64 - ROT[pi_from(i)]) % 64)); };
    for (uint32_t i = 0; i < 25; i++)
        for (uint32_t l = 0; l < 4; l++) {
            const uint32_t v = limb_of_bits(g, [&](uint32_t k) {
                const uint32_t z = 16 * l + k, i1 = (i + 1) % 5 + 5 * (i / 5), i2 = (i + 2) % 5 + 5 * (i / 5);
                return g.xor2(b_bit(i, z), g.mul(g.sub(g.cst(1), b_bit(i1, z)), b_bit(i2, z)));
            });
            g.assert_zero(g.sub(g.col(L::app(4 * i + l)), v));
        }
    // A''[0][0] from its bits; A'''[0][0] = that ^ rc, rc_z = sum_r STEP[r] RC[r]_z (0 on row 24)
    for (uint32_t l = 0; l < 4; l++) {
        const uint32_t v = limb_of_bits(g, [&](uint32_t k) { return g.col(L::app00_bit(16 * l + k)); });
        g.assert_zero(g.sub(g.col(L::app(l)), v));
    }
    for (uint32_t l = 0; l < 4; l++) {
        const uint32_t v = limb_of_bits(g, [&](uint32_t k) {
            const uint32_t z = 16 * l + k, bit = g.col(L::app00_bit(z));
            uint32_t rc = 0;
            bool any = false;
            for (uint32_t r = 0; r < 24; r++)
                if ((RC[r] >> z) & 1u) rc = any ? g.add(rc, g.col(L::step(r))) : g.col(L::step(r)), any = true;
            return any ? g.xor2(bit, rc) : bit;
        });
        g.assert_zero(g.sub(g.col(L::appp00(l)), v));
    }
    // unless this is an output row, the next row's A is this row's result, and ID and M go on
    auto carried = [&](uint32_t next_col, uint32_t this_col) {
        const uint32_t on = g.mul(g.push(RK_AIR_IS_TRANSITION), g.sub(g.cst(1), g.col(L::step(24))));
        g.assert_zero(g.mul(on, g.sub(g.nxt(next_col), g.col(this_col))));
    };
    for (uint32_t j = 0; j < 100; j++) carried(L::a(j), j < 4 ? L::appp00(j) : L::app(j));
    carried(L::ID, L::ID);
    carried(L::M, L::M);
    g.assert_zero(g.sub(g.col(L::M_IN), g.mul(g.col(L::M), g.col(L::step(0)))));
    g.assert_zero(g.sub(g.col(L::M_OUT), g.mul(g.col(L::M), g.col(L::step(24)))));
}

}  // namespace kc
