// TEST INFRASTRUCTURE: the lane bodies of rk_fri_reduce_rows_device (p3k::fri_fold_lane with the X column, fri_path_lane,
// fri_reduce_term / fri_reduce_join / fri_reduce_row, chip_row; raiko_amd/csrc/p3_kernels.hpp) run on the CPU in the
// order of the launches of fri_tables.hip.  The reduce kernel's workgroup is emulated as it runs: FRI_REDUCE_TPB lanes in
// waves of 64, every scan step reading the sums the lanes `d` further down held before the step (a shuffle), the waves'
// totals and the round's running reduced opening passed through arrays that stand for LDS, the barriers where the
// kernel has them.  Buffers must arrive zeroed, as the library clears them.
#include <cstring>
#include <vector>

#include "p3_kernels.hpp"

namespace {

void reduce_workgroup(const p3k::FriReduceArgs& a, uint32_t q, uint32_t rd) {
    constexpr uint32_t TPB = p3k::FRI_REDUCE_TPB, WAVES = TPB / 64;
    bb::Ext wtot[2][WAVES], s_rop = bb::ext_zero();
    const p3k::FriReduceCtx cx = p3k::fri_reduce_begin(a, q, rd);
    bb::Ext rop = bb::ext_zero();            // the same in every lane
    for (uint32_t m = 0; m < a.M; m++) {
        const uint32_t* slot = a.slots + p3k::FRI_REDUCE_SLOT_WORDS * m;
        if (slot[0] != rd) continue;
        const uint32_t width = slot[1];
        bb::Ext carry[2] = {bb::ext_zero(), bb::ext_zero()};   // the same in every lane
        for (uint32_t base = 0; base < width; base += TPB) {
            std::vector<p3k::FriReduceLane> ln(TPB);
            for (uint32_t tid = 0; tid < TPB; tid++) {
                if (base + tid < width) {
                    p3k::fri_reduce_term(a, q, m, base + tid, ln[tid]);
                } else {
                    ln[tid].p = 0;
                    ln[tid].pw[0] = ln[tid].pw[1] = ln[tid].sum[0] = ln[tid].sum[1] = bb::ext_zero();
                }
            }
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const std::vector<p3k::FriReduceLane> old = ln;
                for (uint32_t tid = 0; tid < TPB; tid++)
                    if ((tid & 63u) >= d) p3k::fri_reduce_join(ln[tid], old[tid - d].sum[0], old[tid - d].sum[1]);
            }
            for (uint32_t w = 0; w < WAVES; w++) wtot[0][w] = ln[64 * w + 63].sum[0], wtot[1][w] = ln[64 * w + 63].sum[1];
            // barrier
            bb::Ext next_carry[2] = {carry[0], carry[1]};
            for (uint32_t tid = 0; tid < TPB; tid++) {
                const uint32_t wave = tid >> 6;
                bb::Ext before[2] = {carry[0], carry[1]}, all[2] = {carry[0], carry[1]};
                for (uint32_t w = 0; w < WAVES; w++)
                    for (int j = 0; j < 2; j++) {
                        if (w < wave) before[j] = bb::add(before[j], wtot[j][w]);
                        all[j] = bb::add(all[j], wtot[j][w]);
                    }
                next_carry[0] = all[0], next_carry[1] = all[1];
                p3k::fri_reduce_join(ln[tid], before[0], before[1]);
                if (base + tid < width) {
                    const bb::Ext after = p3k::fri_reduce_row(a, q, m, base + tid, cx, ln[tid], rop);
                    if (base + tid + 1 == width) s_rop = after;
                }
            }
            carry[0] = next_carry[0], carry[1] = next_carry[1];
            // barrier
        }
        rop = s_rop;
    }
}

}  // namespace

extern "C" {

// tab = rc_ext 128 | rc_int 13 | diag 16 (Montgomery words); slots = FRI_REDUCE_SLOT_WORDS words per slot, gen(log_n) filled
// in; chip_n = the chip table's padded height
int emul_fri_reduce_rows(uint32_t log_max, uint32_t blowup_log2, uint32_t queries, uint32_t gen_l, uint32_t wm, uint32_t shiftm,
                         const uint32_t* fold_pub, const uint32_t* fold_rec, const uint32_t* tab, int m4, uint32_t n_slots, const uint32_t* slots,
                         uint32_t rows_per_query, const uint32_t* reduce_pub, const uint32_t* in_rec, size_t per_record, uint32_t* fold,
                         uint32_t* path, uint32_t* reduce, uint32_t* chip, size_t chip_n) {
    p3k::FriArgs a{};
    a.L = log_max, a.R = log_max - blowup_log2, a.Q = queries;
    a.gen_l = gen_l, a.wm = wm, a.pub = fold_pub, a.rec = fold_rec;
    a.xcol = 1, a.shiftm = shiftm;
    std::vector<uint32_t> in(chip_n * 16, 0), mult(chip_n, 0);
    a.fold = fold, a.path = path, a.claims = nullptr, a.chip_in = in.data(), a.chip_mult = mult.data();
    p3k::P2ChipLayout L;
    L.W = 16, L.RP = 13, L.width = 314;
    for (uint32_t q = 0; q < a.Q; q++) p3k::fri_fold_lane(a, q);
    for (uint32_t t = 0; t < a.Q * a.R; t++) {
        if (m4) p3k::fri_path_lane<1>(a, t, tab, L);
        else p3k::fri_path_lane<0>(a, t, tab, L);
    }
    std::vector<uint32_t> apow(32 * 4);
    bb::Ext p = p3k::fri_load_ext(reduce_pub);
    for (int i = 0; i < 32; i++) {
        std::memcpy(&apow[4 * i], p.c, 16);
        p = bb::mul(p, p, wm);
    }
    p3k::FriReduceArgs r{};
    r.L = log_max, r.R = a.R, r.Q = queries, r.M = n_slots;
    r.rows_per_query = rows_per_query, r.wm = wm, r.shiftm = shiftm, r.gen_l = gen_l;
    r.per_record = per_record;
    r.slots = slots, r.pub = reduce_pub, r.rec = in_rec, r.apow = apow.data(), r.out = reduce;
    for (uint32_t blk = 0; blk < queries * a.R; blk++) reduce_workgroup(r, blk / a.R, blk % a.R);
    for (size_t row = 0; row < chip_n; row++) {
        if (m4) p3k::chip_row<16, 13, 1>(chip + row * L.width, in.data() + row * 16, mult[row], tab, L);
        else p3k::chip_row<16, 13, 0>(chip + row * L.width, in.data() + row * 16, mult[row], tab, L);
    }
    return 0;
}

}  // extern "C"
