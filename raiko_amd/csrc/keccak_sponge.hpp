// The Keccak-256 sponge table over the Keccak-f[1600] chip (rk_keccak_sponge_*, include/raiko_hip.h), HIP-free: where its
// columns are (KeccakSpongeLayout), the lane body of the rows kernel (keccak_sponge.hip; tests/emul runs the same code on the
// CPU one emulated lane at a time) and the step-list writer of its AIR.  The table absorbs whole 136-byte blocks: padding
// lies with whoever sends them.  Constants, pick / limb_word / bit_word and StepGen are the chip's (keccak_chip.hpp).
#pragma once
#include "keccak_chip.hpp"

namespace kc {

// ---- three rows = one block (a group): the X row holds the block (V[0..67] its 68 rate limbs, V[68..99] = 0), the I row
// the state entering the permutation (PREV xor the block), the O row the permutation's output.  Everything the table
// sends stands in the one block V of 100 limb columns, on different rows of the group: a permutation's two ends alone
// are 200 limbs, and a table's interactions may read 120 distinct columns.  On EVERY row MB are the bits of V's rate
// lanes, PB those of PREV's and XR the limbs of their xor (unconditional constraints: an all-zero row satisfies them);
// only the X row's XR is read, by the transition to the I row, which so stays linear under its selectors.
struct KeccakSpongeLayout {
    static constexpr uint32_t ROWS = 3, RATE_LANES = 17, RATE_LIMBS = 68;
    RK_HD static constexpr uint32_t v(uint32_t j) { return j; }                               // V[100]: limb j = 4 lane + limb
    RK_HD static constexpr uint32_t prev(uint32_t j) { return 100 + j; }                      // PREV[100]: the state before this block, the same on a group's rows
    RK_HD static constexpr uint32_t mb(uint32_t i, uint32_t z) { return 200 + 64 * i + z; }   // MB[17][64]: the bits of V's rate lanes
    RK_HD static constexpr uint32_t pb(uint32_t i, uint32_t z) { return 1288 + 64 * i + z; }  // PB[17][64]: the bits of PREV's rate lanes
    RK_HD static constexpr uint32_t xr(uint32_t j) { return 2376 + j; }                       // XR[68]: sum_k 2^k (mb ^ pb), limbs
    // the flags and counters, constant over a group but for the kinds, NBLK and the multiplicities; all 0 on a padding row
    static constexpr uint32_t MSG = 2444, BLK = 2445, NBLK = 2446, PID = 2447;                // NBLK = BLK + REAL
    static constexpr uint32_t KX = 2448, KI = 2449, KO = 2450, REAL = 2451;                   // REAL = KX + KI + KO, boolean
    static constexpr uint32_t FIRST = 2452, LAST = 2453;                                      // of the block within its message
    static constexpr uint32_t S_IN = 2454, S_OUT = 2455, S_MSG = 2456, S_DIG = 2457;          // REAL KI, REAL KO, REAL KX, KO LAST
    static constexpr uint32_t FLAGS = MSG, N_FLAGS = 14, WIDTH = 2458;
};

// ---- the rows (rk_keccak_sponge_trace): one wavefront per block slot, every lane carrying the same values; lane z
// takes bit z of a 64-column bit group, so every such group leaves as one store of 64 consecutive words
struct KeccakSpongeArgs {
    const uint64_t* blocks;    // n_blocks x 17 lanes: the padded messages
    const uint32_t* first;     // n_msgs + 1: the first block of each message, then n_blocks
    const uint32_t* msg_ids;   // n_msgs Montgomery words, or null: the message's number
    const uint64_t* states;    // n_blocks x 25 lanes: the state entering each block's permutation
    const uint64_t* outs;      // n_blocks x 25 lanes: its output
    size_t n_msgs, n_blocks, rows;
    uint32_t* trace;           // rows x WIDTH Montgomery words
};
// the message of block `slot`: the last m with first[m] <= slot (first[0] = 0, first[n_msgs] = n_blocks > slot)
RK_HD size_t sponge_msg_of(const uint32_t* first, size_t n_msgs, size_t slot) {
    size_t lo = 0, hi = n_msgs;
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (first[mid] <= slot) lo = mid;
        else hi = mid;
    }
    return lo;
}
// lane `lane` (0..63) of the wavefront that writes block slot `slot`: its share of the slot's rows that lie in the table
RK_HD void keccak_sponge_lane(const KeccakSpongeArgs& g, size_t slot, uint32_t lane) {
    using L = KeccakSpongeLayout;
    const bool real = slot < g.n_blocks;
    size_t m = 0;
    uint32_t blk = 0;
    bool is_first = false, is_last = false;
    if (real) {
        m = sponge_msg_of(g.first, g.n_msgs, slot);
        blk = (uint32_t)(slot - g.first[m]);
        is_first = blk == 0;
        is_last = slot + 1 == g.first[m + 1];
    }
    const uint32_t msg = real ? (g.msg_ids ? g.msg_ids[m] : bb::encode((uint32_t)m)) : 0u;
    const uint32_t one = real ? bb::ONE : 0u;
    uint64_t prev[25];
#pragma unroll
    for (uint32_t i = 0; i < 25; i++) prev[i] = real && !is_first && slot > 0 ? g.outs[25 * (slot - 1) + i] : 0;
#pragma unroll 1
    for (uint32_t r = 0; r < L::ROWS; r++) {
        const size_t at = L::ROWS * slot + r;
        if (at >= g.rows) break;   // the table's end cuts the last slot off
        uint32_t* row = g.trace + at * L::WIDTH;
        // V: the block on the X row, the permutation's input on the I row, its output on the O row
        uint64_t v[25];
        const uint64_t* full = r == 1 ? g.states : g.outs;
#pragma unroll
        for (uint32_t i = 0; i < 25; i++) v[i] = !real ? 0 : r != 0 ? full[25 * slot + i] : i < L::RATE_LANES ? g.blocks[L::RATE_LANES * slot + i] : 0;
        // V | PREV: columns 0..199
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t col = lane + 64 * k;
            if (col < 100) row[col] = limb_word(pick(v, col >> 2), col & 3);
            else if (col < 200) row[col] = limb_word(pick(prev, (col - 100) >> 2), (col - 100) & 3);
        }
#pragma unroll
        for (uint32_t i = 0; i < L::RATE_LANES; i++) row[L::mb(i, lane)] = bit_word(v[i], lane);
#pragma unroll
        for (uint32_t i = 0; i < L::RATE_LANES; i++) row[L::pb(i, lane)] = bit_word(prev[i], lane);
        uint64_t x[25];
#pragma unroll
        for (uint32_t i = 0; i < 25; i++) x[i] = i < L::RATE_LANES ? v[i] ^ prev[i] : 0;
#pragma unroll
        for (uint32_t k = 0; k < 2; k++) {
            const uint32_t j = lane + 64 * k;
            if (j < L::RATE_LIMBS) row[L::xr(j)] = limb_word(pick(x, j >> 2), j & 3);
        }
        // MSG BLK NBLK PID | KX KI KO REAL | FIRST LAST | S_IN S_OUT S_MSG S_DIG
        if (lane < L::N_FLAGS) {
            const uint32_t c = L::FLAGS + lane;
            uint32_t w = 0;
            if (c == L::MSG) w = msg;
            else if (c == L::BLK) w = bb::encode(blk);
            else if (c == L::NBLK) w = real ? bb::encode(blk + 1) : 0u;
            else if (c == L::PID) w = real ? bb::encode((uint32_t)slot) : 0u;
            else if (c == L::KX || c == L::S_MSG) w = r == 0 ? one : 0u;
            else if (c == L::KI || c == L::S_IN) w = r == 1 ? one : 0u;
            else if (c == L::KO || c == L::S_OUT) w = r == 2 ? one : 0u;
            else if (c == L::REAL) w = one;
            else if (c == L::FIRST) w = is_first ? one : 0u;
            else if (c == L::LAST) w = is_last ? one : 0u;
            else if (c == L::S_DIG) w = r == 2 && is_last ? one : 0u;
            row[c] = w;
        }
    }
}

// ---- the AIR as a step list (rk_keccak_sponge_air).  Degree <= 3 throughout, selectors and IS_TRANSITION counted as 1.
inline void keccak_sponge_steps(std::vector<rk_air_step>& steps) {
    using L = KeccakSpongeLayout;
    StepGen g{steps};
    auto one_minus = [&](uint32_t v) { return g.sub(g.cst(1), v); };
    auto trans = [&]() { return g.push(RK_AIR_IS_TRANSITION); };
    // the kinds: boolean, at most one a row (REAL is their sum), X -> I -> O, and an X row only after an O row: REAL falls
    // once, the rows are whole real groups and then padding
    for (uint32_t c : {L::KX, L::KI, L::KO, L::REAL, L::FIRST, L::LAST}) g.assert_bool(c);
    g.assert_zero(g.sub(g.col(L::REAL), g.add(g.add(g.col(L::KX), g.col(L::KI)), g.col(L::KO))));
    g.assert_zero(g.mul(trans(), g.sub(g.col(L::KX), g.nxt(L::KI))));
    g.assert_zero(g.mul(trans(), g.sub(g.col(L::KI), g.nxt(L::KO))));
    g.assert_zero(g.mul(g.mul(trans(), g.nxt(L::KX)), one_minus(g.col(L::KO))));
    // the first row opens a message as block 0 with PID 0 (or is padding); a group the table's end cuts is not real
    g.assert_zero(g.mul(g.push(RK_AIR_IS_FIRST_ROW), g.add(g.col(L::KI), g.col(L::KO))));
    g.assert_zero(g.mul(g.push(RK_AIR_IS_FIRST_ROW), g.sub(g.col(L::FIRST), g.col(L::REAL))));
    g.assert_zero(g.mul(g.push(RK_AIR_IS_FIRST_ROW), g.col(L::PID)));
    g.assert_zero(g.mul(g.push(RK_AIR_IS_LAST_ROW), g.add(g.col(L::KX), g.col(L::KI))));
    // a padding row is zero (MB, PB, XR follow from V and PREV; the kinds from REAL)
    for (uint32_t c : {L::MSG, L::BLK, L::PID, L::FIRST, L::LAST})
        g.assert_zero(g.mul(one_minus(g.col(L::REAL)), g.col(c)));
    for (uint32_t j = 0; j < 100; j++) g.assert_zero(g.mul(one_minus(g.col(L::REAL)), g.col(L::v(j))));
    for (uint32_t j = 0; j < 100; j++) g.assert_zero(g.mul(one_minus(g.col(L::REAL)), g.col(L::prev(j))));
    // every multiplicity is forced: a real row cannot withhold a send
    g.assert_zero(g.sub(g.col(L::S_MSG), g.mul(g.col(L::REAL), g.col(L::KX))));
    g.assert_zero(g.sub(g.col(L::S_IN), g.mul(g.col(L::REAL), g.col(L::KI))));
    g.assert_zero(g.sub(g.col(L::S_OUT), g.mul(g.col(L::REAL), g.col(L::KO))));
    g.assert_zero(g.sub(g.col(L::S_DIG), g.mul(g.col(L::KO), g.col(L::LAST))));
    g.assert_zero(g.sub(g.col(L::NBLK), g.add(g.col(L::BLK), g.col(L::REAL))));
    // FIRST => BLK = 0 and PREV = 0 (BLK = 0 => FIRST by the transitions below: a block that continues has BLK >= 1)
    g.assert_zero(g.mul(g.col(L::FIRST), g.col(L::BLK)));
    for (uint32_t j = 0; j < 100; j++) g.assert_zero(g.mul(g.col(L::FIRST), g.col(L::prev(j))));
    // the bits: boolean, recomposed to the rate limbs of V and PREV; XR is their xor, limb by limb
    for (uint32_t i = 0; i < L::RATE_LANES; i++)
        for (uint32_t z = 0; z < 64; z++) g.assert_bool(L::mb(i, z));
    for (uint32_t i = 0; i < L::RATE_LANES; i++)
        for (uint32_t z = 0; z < 64; z++) g.assert_bool(L::pb(i, z));
    for (uint32_t j = 0; j < L::RATE_LIMBS; j++) {
        const uint32_t i = j >> 2, l = j & 3;
        g.assert_zero(g.sub(g.col(L::v(j)), limb_of_bits(g, [&](uint32_t k) { return g.col(L::mb(i, 16 * l + k)); })));
        g.assert_zero(g.sub(g.col(L::prev(j)), limb_of_bits(g, [&](uint32_t k) { return g.col(L::pb(i, 16 * l + k)); })));
        g.assert_zero(g.sub(g.col(L::xr(j)), limb_of_bits(g, [&](uint32_t k) { return g.xor2(g.col(L::mb(i, 16 * l + k)), g.col(L::pb(i, 16 * l + k))); })));
    }
    // the X row: a block has no capacity part; the I row after it: rate = XR, capacity = PREV's
    for (uint32_t j = L::RATE_LIMBS; j < 100; j++) g.assert_zero(g.mul(g.col(L::KX), g.col(L::v(j))));
    for (uint32_t j = 0; j < 100; j++)
        g.assert_zero(g.mul(g.mul(trans(), g.col(L::KX)), g.sub(g.nxt(L::v(j)), g.col(j < L::RATE_LIMBS ? L::xr(j) : L::prev(j)))));
    // within a group (after an X or an I row) PREV and the counters go on
    auto in_group = [&](uint32_t c) {
        g.assert_zero(g.mul(g.mul(trans(), g.add(g.col(L::KX), g.col(L::KI))), g.sub(g.nxt(c), g.col(c))));
    };
    for (uint32_t j = 0; j < 100; j++) in_group(L::prev(j));
    for (uint32_t c : {L::MSG, L::BLK, L::PID, L::FIRST, L::LAST}) in_group(c);
    // PID counts the groups
    g.assert_zero(g.mul(g.mul(trans(), g.nxt(L::KX)), g.sub(g.nxt(L::PID), g.add(g.col(L::PID), g.cst(1)))));
    // after an O row that is not LAST (KO - S_DIG): a real group of the same message, BLK + 1, its PREV this row's V; such
    // a row is not the table's last
    auto cont = [&]() { return g.sub(g.col(L::KO), g.col(L::S_DIG)); };
    g.assert_zero(g.mul(g.push(RK_AIR_IS_LAST_ROW), cont()));
    g.assert_zero(g.mul(g.mul(trans(), cont()), one_minus(g.nxt(L::KX))));
    g.assert_zero(g.mul(g.mul(trans(), cont()), g.sub(g.nxt(L::MSG), g.col(L::MSG))));
    g.assert_zero(g.mul(g.mul(trans(), cont()), g.sub(g.nxt(L::BLK), g.add(g.col(L::BLK), g.cst(1)))));
    g.assert_zero(g.mul(g.mul(trans(), cont()), g.nxt(L::FIRST)));
    for (uint32_t j = 0; j < 100; j++) g.assert_zero(g.mul(g.mul(trans(), cont()), g.sub(g.nxt(L::prev(j)), g.col(L::v(j)))));
    // after a LAST O row (S_DIG): a real group opens a message
    g.assert_zero(g.mul(g.mul(trans(), g.col(L::S_DIG)), g.sub(g.nxt(L::FIRST), g.nxt(L::KX))));
}

}  // namespace kc
