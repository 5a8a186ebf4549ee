// TEST INFRASTRUCTURE: the lane bodies of rk_fri_chip_rows_device (p3k::fri_fold_lane / fri_path_lane / chip_row,
// raiko_amd/csrc/p3_kernels.hpp) run on the CPU one emulated lane at a time, in the order of the launches of
// fri_tables.hip: every fold lane, every path lane, every chip lane.  Buffers must arrive zeroed, as the library clears them.
#include <cstring>
#include <vector>

#include "p3_kernels.hpp"

extern "C" {

// tab = rc_ext 128 | rc_int 13 | diag 16 (Montgomery words); chip_n = the chip table's padded height
int emul_fri_chip_rows(uint32_t log_max, uint32_t blowup_log2, uint32_t queries, uint32_t gen_l, uint32_t wm, const uint32_t* pub,
                       const uint32_t* rec, const uint32_t* tab, int m4, uint32_t* fold, uint32_t* path, uint32_t* claims, uint32_t* chip,
                       size_t chip_n) {
    p3k::FriArgs a{};
    a.L = log_max, a.R = log_max - blowup_log2, a.Q = queries;
    a.gen_l = gen_l, a.wm = wm, a.pub = pub, a.rec = rec;
    std::vector<uint32_t> in(chip_n * 16, 0), mult(chip_n, 0);
    a.fold = fold, a.path = path, a.claims = claims, a.chip_in = in.data(), a.chip_mult = mult.data();
    p3k::P2ChipLayout L;
    L.W = 16, L.RP = 13, L.width = 314;
    for (uint32_t q = 0; q < a.Q; q++) p3k::fri_fold_lane(a, q);
    for (uint32_t t = 0; t < a.Q * a.R; t++) {
        if (m4) p3k::fri_path_lane<1>(a, t, tab, L);
        else p3k::fri_path_lane<0>(a, t, tab, L);
    }
    for (size_t r = 0; r < chip_n; r++) {
        if (m4) p3k::chip_row<16, 13, 1>(chip + r * L.width, in.data() + r * 16, mult[r], tab, L);
        else p3k::chip_row<16, 13, 0>(chip + r * L.width, in.data() + r * 16, mult[r], tab, L);
    }
    return 0;
}

}  // extern "C"
