// The Keccak-256 padding table under the sponge table (rk_keccak_pad_*, include/raiko_hip.h), HIP-free: where its columns
// are (KeccakPadLayout), the bodies of its three kernels (keccak_pad.hip; tests/emul runs the same code on the CPU one
// emulated lane at a time) and the step-list writer of its AIR.  The table takes a message as 32-bit words and a byte
// length, places the words into 136-byte blocks, masks the last word's bytes past the length and adds 0x01 .. 0x80: it
// receives what the sponge table sends.  StepGen and limb_of_bits are the chip's (keccak_chip.hpp).
#pragma once
#include "keccak_chip.hpp"

namespace kc {

// ---- one row = one 32-bit word slot; 34 rows = one block.  B is a shift register of limbs: B[66], B[67] are the word
// PLACED on this row, next.B[j] = B[j + 2] within a block, so the block's 34th row (STEP[33]) holds the whole block in
// B[0..67] and the 68 block limbs the table receives never stand in more than 68 columns.  A row is DATA (a word before
// the one that holds byte position LEN), END (that word: exactly one a message) or AFTER; W is the word handed over by
// the sender, WB its bits, E the one-hot of LEN mod 4 on the END row.  All columns are 0 on a padding row.
struct KeccakPadLayout {
    static constexpr uint32_t ROWS = 34, BLOCK_LIMBS = 68;
    RK_HD static constexpr uint32_t b(uint32_t j) { return j; }             // B[68]: the shift register, limb j of the block on a STEP[33] row
    RK_HD static constexpr uint32_t step(uint32_t t) { return 68 + t; }     // STEP[34]: one-hot word position in the block
    static constexpr uint32_t W_LO = 102, W_HI = 103;                       // the sender's word; 0 where R = 0
    RK_HD static constexpr uint32_t wb(uint32_t z) { return 104 + z; }      // WB[32]: the bits of W
    RK_HD static constexpr uint32_t e(uint32_t k) { return 136 + k; }       // E[4]: one-hot of LEN mod 4 on the END row
    RK_HD static constexpr uint32_t d(uint32_t j) { return 140 + j; }       // D[16]: the digest's limbs on a message's last row, else 0
    static constexpr uint32_t MSG = 156, BLK = 157, NBLK = 158, IDX = 159, LEN = 160;   // NBLK = BLK + REAL; IDX the word's index in the message
    static constexpr uint32_t DATA = 161, END = 162, AFTER = 163, REAL = 164;           // REAL = DATA + END + AFTER, boolean
    static constexpr uint32_t R = 165, S_END = 166;                         // R = DATA + END - E[0]; S_END = STEP[33] (END + AFTER)
    static constexpr uint32_t FLAGS = MSG, N_FLAGS = 11, WIDTH = 167;
};

// ---- the padded blocks (rk_keccak_pad_trace, first launch): one thread per 32-bit word slot of d_blocks
struct KeccakPadArgs {
    const uint32_t* words;       // n_words: the messages' words back to back
    const uint32_t* word_first;  // n_msgs + 1: the first word of each message, then n_words
    const uint32_t* lens;        // n_msgs byte lengths
    const uint32_t* first;       // n_msgs + 1: the first block of each message, then n_blocks
    const uint32_t* msg_ids;     // n_msgs Montgomery words, or null: the message's number
    size_t n_words, n_msgs, n_blocks, rows;
    uint32_t* blocks;            // n_blocks x 34 words = n_blocks x 17 lanes (little endian): the padded messages
    uint32_t* trace;             // rows x WIDTH Montgomery words
};
// the message of block `blk`: the last m with first[m] <= blk (first[0] = 0, first[n_msgs] = n_blocks > blk)
RK_HD size_t pad_msg_of(const uint32_t* first, size_t n_msgs, size_t blk) {
    size_t lo = 0, hi = n_msgs;
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (first[mid] <= blk) lo = mid;
        else hi = mid;
    }
    return lo;
}
// where a block lies in its message, and what one of its word slots holds: the sender's word and the word placed
struct PadBlock {
    size_t m, word0;             // the message; the index in `words` of the block's first word slot
    uint32_t blk, len;
};
struct PadSlot {
    uint32_t idx, e, w, placed;
    bool data, end, last;        // last: the 34th slot of a block at or after END
};
RK_HD PadBlock pad_block(const KeccakPadArgs& g, size_t block) {
    PadBlock p;
    p.m = pad_msg_of(g.first, g.n_msgs, block);
    p.blk = (uint32_t)(block - g.first[p.m]);
    p.len = g.lens[p.m];
    p.word0 = (size_t)g.word_first[p.m] + (size_t)p.blk * KeccakPadLayout::ROWS;
    return p;
}
RK_HD PadSlot pad_slot(const KeccakPadArgs& g, const PadBlock& p, uint32_t t) {
    PadSlot s;
    s.idx = p.blk * KeccakPadLayout::ROWS + t;
    s.e = p.len & 3u;
    const uint32_t q = p.len >> 2;
    s.data = s.idx < q;
    s.end = s.idx == q;
    s.last = t == KeccakPadLayout::ROWS - 1 && !s.data;
    // the sender's word: on the DATA rows and on an END row that holds a message byte; never read past the words
    s.w = (s.data || (s.end && s.e != 0)) && p.word0 + t < g.n_words ? g.words[p.word0 + t] : 0u;
    // placed: DATA the word; END its bytes below e and 0x01 above them; AFTER 0; 0x80 into the block's last byte
    s.placed = s.data ? s.w : s.end ? (s.w & ((1u << (8 * s.e)) - 1u)) + (1u << (8 * s.e)) : 0u;
    if (s.last) s.placed += 0x80000000u;
    return s;
}
// thread `slot` of the blocks kernel: word slot % 34 of block slot / 34
RK_HD void keccak_pad_block_word(const KeccakPadArgs& g, size_t slot) {
    if (slot >= g.n_blocks * KeccakPadLayout::ROWS) return;
    const PadBlock p = pad_block(g, slot / KeccakPadLayout::ROWS);
    g.blocks[slot] = pad_slot(g, p, (uint32_t)(slot % KeccakPadLayout::ROWS)).placed;
}

// ---- the rows (rk_keccak_pad_trace, second launch): one wavefront per block slot, looping over the slot's 34 rows; lane l
// writes columns l, l + 64, l + 128 -- three stores of consecutive words a row.  Everything but the column is the same on
// all lanes, and the message is looked up once a block.  B is read back from the blocks the first launch wrote: B[j] on
// the row of word t is limb j + 2 t - 66 of the block, 0 before the block's start.
RK_HD void keccak_pad_lane(const KeccakPadArgs& g, size_t block, uint32_t lane) {
    using L = KeccakPadLayout;
    const bool real = block < g.n_blocks;
    PadBlock p{0, 0, 0, 0};
    uint32_t msg = 0;
    if (real) {
        p = pad_block(g, block);
        msg = g.msg_ids ? g.msg_ids[p.m] : bb::encode((uint32_t)p.m);
    }
    for (uint32_t t = 0; t < L::ROWS; t++) {
        const size_t at = L::ROWS * block + t;
        if (at >= g.rows) break;   // the table's end cuts the last slot off
        uint32_t* row = g.trace + at * L::WIDTH;
        if (!real) {               // a padding row
#pragma unroll
            for (uint32_t k = 0; k < 3; k++)
                if (lane + 64 * k < L::WIDTH) row[lane + 64 * k] = 0u;
            continue;
        }
        const PadSlot s = pad_slot(g, p, t);
        const bool after = !s.data && !s.end, sends = s.data || (s.end && s.e != 0);
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) {
            const uint32_t c = lane + 64 * k;
            if (c >= L::WIDTH) break;
            uint32_t v = 0;
            if (c < L::BLOCK_LIMBS) {
                const uint32_t j = c + 2 * t;   // limb j - 66 of the block
                v = j >= 66 ? bb::encode((g.blocks[block * L::ROWS + (j - 66) / 2] >> (16 * (j & 1u))) & 0xffffu) : 0u;
            } else if (c < L::W_LO) v = c - L::step(0) == t ? bb::ONE : 0u;
            else if (c == L::W_LO) v = bb::encode(s.w & 0xffffu);
            else if (c == L::W_HI) v = bb::encode(s.w >> 16);
            else if (c < L::e(0)) v = (s.w >> (c - L::wb(0))) & 1u ? bb::ONE : 0u;
            else if (c < L::d(0)) v = s.end && c - L::e(0) == s.e ? bb::ONE : 0u;
            else if (c < L::MSG) v = 0u;        // D: keccak_pad_digest_word, once the digests exist
            else if (c == L::MSG) v = msg;
            else if (c == L::BLK) v = bb::encode(p.blk);
            else if (c == L::NBLK) v = bb::encode(p.blk + 1);
            else if (c == L::IDX) v = bb::encode(s.idx);
            else if (c == L::LEN) v = bb::encode(p.len);
            else if (c == L::DATA) v = s.data ? bb::ONE : 0u;
            else if (c == L::END) v = s.end ? bb::ONE : 0u;
            else if (c == L::AFTER) v = after ? bb::ONE : 0u;
            else if (c == L::REAL) v = bb::ONE;
            else if (c == L::R) v = sends ? bb::ONE : 0u;
            else if (c == L::S_END) v = s.last ? bb::ONE : 0u;
            row[c] = v;
        }
    }
}

// ---- D (rk_keccak_pad_digests): thread i writes limb i % 16 of message i / 16's digest into the message's last row
RK_HD void keccak_pad_digest_word(const uint64_t* digests, const uint32_t* first, size_t n_msgs, size_t n_blocks, size_t rows, uint32_t* trace, size_t i) {
    using L = KeccakPadLayout;
    const size_t m = i / 16;
    const uint32_t j = (uint32_t)(i % 16);
    if (m >= n_msgs) return;
    const size_t end = first[m + 1];
    if (end == 0 || end > n_blocks || end * L::ROWS > rows) return;   // a malformed d_first writes nothing outside the table
    trace[(end * L::ROWS - 1) * L::WIDTH + L::d(j)] = limb_word(digests[4 * m + j / 4], j & 3u);
}

// ---- the AIR as a step list (rk_keccak_pad_air).  Degree <= 3 throughout, selectors and IS_TRANSITION counted as 1.
inline void keccak_pad_steps(std::vector<rk_air_step>& steps) {
    using L = KeccakPadLayout;
    StepGen g{steps};
    auto one_minus = [&](uint32_t v) { return g.sub(g.cst(1), v); };
    auto trans = [&]() { return g.push(RK_AIR_IS_TRANSITION); };
    auto first = [&]() { return g.push(RK_AIR_IS_FIRST_ROW); };
    // the phases: boolean, REAL their sum and boolean (at most one a row); REAL falls once
    for (uint32_t c : {L::DATA, L::END, L::AFTER, L::REAL}) g.assert_bool(c);
    g.assert_zero(g.sub(g.col(L::REAL), g.add(g.add(g.col(L::DATA), g.col(L::END)), g.col(L::AFTER))));
    g.assert_zero(g.mul(g.mul(trans(), g.nxt(L::REAL)), one_minus(g.col(L::REAL))));
    // STEP: boolean, one-hot on a real row and 0 on a padding row, STEP[0] on the first row, cyclic between real rows
    for (uint32_t t = 0; t < L::ROWS; t++) g.assert_bool(L::step(t));
    {
        uint32_t sum = g.col(L::step(0));
        for (uint32_t t = 1; t < L::ROWS; t++) sum = g.add(sum, g.col(L::step(t)));
        g.assert_zero(g.sub(sum, g.col(L::REAL)));
    }
    g.assert_zero(g.mul(first(), g.sub(g.col(L::step(0)), g.col(L::REAL))));
    for (uint32_t t = 0; t < L::ROWS; t++)
        g.assert_zero(g.mul(g.mul(trans(), g.nxt(L::REAL)), g.sub(g.col(L::step(t)), g.nxt(L::step((t + 1) % L::ROWS)))));
    // the multiplicities are forced: S_END = STEP[33] (END + AFTER) marks a message's last row, R = DATA + END - E[0] the
    // rows that carry a sender's word (an END row with LEN mod 4 = 0 holds no message byte); the blocks are received
    // STEP[33] times, which is REAL STEP[33]
    g.assert_zero(g.sub(g.col(L::S_END), g.mul(g.col(L::step(33)), g.add(g.col(L::END), g.col(L::AFTER)))));
    g.assert_zero(g.sub(g.col(L::R), g.sub(g.add(g.col(L::DATA), g.col(L::END)), g.col(L::e(0)))));
    g.assert_zero(g.sub(g.col(L::NBLK), g.add(g.col(L::BLK), g.col(L::REAL))));
    // E: boolean, one-hot on the END row, 0 elsewhere; there LEN = 4 IDX + e
    for (uint32_t k = 0; k < 4; k++) g.assert_bool(L::e(k));
    g.assert_zero(g.sub(g.col(L::END), g.add(g.add(g.col(L::e(0)), g.col(L::e(1))), g.add(g.col(L::e(2)), g.col(L::e(3))))));
    {
        const uint32_t idx4 = g.dbl(g.dbl(g.col(L::IDX)));
        const uint32_t e = g.add(g.add(g.col(L::e(1)), g.dbl(g.col(L::e(2)))), g.add(g.col(L::e(3)), g.dbl(g.col(L::e(3)))));
        g.assert_zero(g.sub(g.mul(g.col(L::END), g.sub(g.col(L::LEN), idx4)), e));
    }
    // W: its bits are boolean and recompose it on every row; W = 0 where no word is taken
    for (uint32_t z = 0; z < 32; z++) g.assert_bool(L::wb(z));
    g.assert_zero(g.sub(g.col(L::W_LO), limb_of_bits(g, [&](uint32_t k) { return g.col(L::wb(k)); })));
    g.assert_zero(g.sub(g.col(L::W_HI), limb_of_bits(g, [&](uint32_t k) { return g.col(L::wb(16 + k)); })));
    g.assert_zero(g.mul(one_minus(g.col(L::R)), g.col(L::W_LO)));
    g.assert_zero(g.mul(one_minus(g.col(L::R)), g.col(L::W_HI)));
    // the placed word.  DATA: W.  END: W's bytes below e, then 0x01 -- e = 0: 0x00000001; e = 1: byte 0 + 0x0100; e = 2:
    // the low limb + 0x00010000; e = 3: the low limb and byte 2 + 0x0100 above it.  AFTER: 0.  A message's last row adds
    // 0x80 to the block's last byte: the kept bytes above e are 0 and 0x01 + 0x80 = 0x81, so nothing carries
    auto byte_of = [&](uint32_t n) {
        uint32_t acc = g.col(L::wb(8 * n + 7));
        for (int k = 6; k >= 0; k--) acc = g.add(g.dbl(acc), g.col(L::wb(8 * n + (uint32_t)k)));
        return acc;
    };
    {
        const uint32_t lo = g.add(g.add(g.mul(g.add(g.col(L::DATA), g.add(g.col(L::e(2)), g.col(L::e(3)))), g.col(L::W_LO)), g.col(L::e(0))),
                                  g.mul(g.col(L::e(1)), g.add(byte_of(0), g.cst(0x100))));
        g.assert_zero(g.sub(g.col(L::b(66)), lo));
    }
    {
        const uint32_t hi = g.add(g.add(g.mul(g.col(L::DATA), g.col(L::W_HI)), g.col(L::e(2))),
                                  g.add(g.mul(g.col(L::e(3)), g.add(byte_of(2), g.cst(0x100))), g.mul(g.cst(0x8000), g.col(L::S_END))));
        g.assert_zero(g.sub(g.col(L::b(67)), hi));
    }
    // the shift register: empty at a block's start and on a padding row, shifted by one word after a real row that is not
    // the block's last (REAL - STEP[33]: such a row is followed by a real row, below)
    for (uint32_t j = 0; j < 66; j++) g.assert_zero(g.mul(g.col(L::step(0)), g.col(L::b(j))));
    for (uint32_t j = 0; j < 66; j++) g.assert_zero(g.mul(one_minus(g.col(L::REAL)), g.col(L::b(j))));
    for (uint32_t j = 0; j < 66; j++)
        g.assert_zero(g.mul(g.mul(trans(), g.sub(g.col(L::REAL), g.col(L::step(33)))), g.sub(g.nxt(L::b(j)), g.col(L::b(j + 2)))));
    // a padding row is zero (W, WB, E, R, S_END, NBLK, B[66], B[67], STEP and the phases follow from REAL = 0)
    for (uint32_t c : {L::MSG, L::BLK, L::IDX, L::LEN}) g.assert_zero(g.mul(one_minus(g.col(L::REAL)), g.col(c)));
    // D is read on a message's last row only, where the sponge's send binds it; 0 elsewhere
    for (uint32_t j = 0; j < 16; j++) g.assert_zero(g.mul(one_minus(g.col(L::S_END)), g.col(L::d(j))));
    // a message opens with IDX = 0, BLK = 0 and not AFTER: on the first row and after a message's last row
    for (uint32_t c : {L::IDX, L::BLK, L::AFTER}) {
        g.assert_zero(g.mul(first(), g.col(c)));
        g.assert_zero(g.mul(g.mul(trans(), g.col(L::S_END)), g.nxt(c)));
    }
    // a real row that is not its message's last (REAL - S_END) is followed by a real row of the same message: MSG and LEN
    // go on, IDX + 1, BLK + STEP[33], AFTER exactly after END or AFTER -- so DATA* END AFTER*, one END a message --; such
    // a row is not the table's last: a message the table's end cuts is not real
    auto cont = [&]() { return g.sub(g.col(L::REAL), g.col(L::S_END)); };
    g.assert_zero(g.mul(g.push(RK_AIR_IS_LAST_ROW), cont()));
    g.assert_zero(g.mul(g.mul(trans(), cont()), one_minus(g.nxt(L::REAL))));
    g.assert_zero(g.mul(g.mul(trans(), cont()), g.sub(g.nxt(L::MSG), g.col(L::MSG))));
    g.assert_zero(g.mul(g.mul(trans(), cont()), g.sub(g.nxt(L::LEN), g.col(L::LEN))));
    g.assert_zero(g.mul(g.mul(trans(), cont()), g.sub(g.nxt(L::IDX), g.add(g.col(L::IDX), g.cst(1)))));
    g.assert_zero(g.mul(g.mul(trans(), cont()), g.sub(g.nxt(L::BLK), g.add(g.col(L::BLK), g.col(L::step(33))))));
    g.assert_zero(g.mul(g.mul(trans(), cont()), g.sub(g.nxt(L::AFTER), g.add(g.col(L::END), g.col(L::AFTER)))));
}

}  // namespace kc
