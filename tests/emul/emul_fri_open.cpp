// TEST INFRASTRUCTURE: the three new lane bodies of rk_fri_open_rows_device (p3k::fri_open_sponge_lane, fri_open_fill_lane,
// fri_open_ipath_lane; raiko_amd/csrc/p3_kernels.hpp) and chip_row run on the CPU in the order of the launches of
// fri_tables.hip.  `reduce` arrives as the earlier kernels leave it -- the reduce table's own columns at the wider stride, the
// sponge columns zero --, chip_in / chip_mult with the commit-phase inputs (rows below chip_base) filled in; everything
// else must arrive zeroed, as the library clears it.
#include <vector>

#include "p3_kernels.hpp"

extern "C" {

// tab = rc_ext 128 | rc_int 13 | diag 16 (Montgomery words); slots, groups, rowinfo, levels: the words of p3_kernels.hpp
int emul_fri_open_rows(uint32_t log_max, uint32_t queries, uint32_t n_slots, uint32_t n_groups, uint32_t n_batches, uint32_t rows_per_query,
                       uint32_t stride, size_t per_record, size_t per_path, size_t chip_base, const uint32_t* slots, const uint32_t* groups,
                       const uint32_t* rowinfo, const uint32_t* levels, const uint32_t* rec, const uint32_t* paths, const uint32_t* tab, int m4,
                       uint32_t* reduce, uint32_t* ipath, uint32_t* chip_in, uint32_t* chip_mult, uint32_t* chip, size_t chip_n,
                       uint32_t* state, size_t state_n) {
    p3k::FriOpenArgs a{};
    a.L = log_max, a.Q = queries, a.M = n_slots, a.G = n_groups, a.NB = n_batches;
    a.rows_per_query = rows_per_query, a.stride = stride, a.sponge_at = stride - p3k::FRI_OPEN_SPONGE_COLS;
    a.per_record = per_record, a.per_path = per_path, a.chip_base = chip_base;
    a.slots = slots, a.groups = groups, a.rowinfo = rowinfo, a.levels = levels, a.rec = rec, a.paths = paths;
    std::vector<uint32_t> sin(state_n * 16, 0), smult(state_n, 0), dig((size_t)queries * n_groups * 8, 0);
    a.reduce = reduce, a.ipath = ipath, a.state_in = sin.data(), a.state_mult = smult.data(), a.chip_in = chip_in, a.chip_mult = chip_mult;
    a.digests = dig.data();
    p3k::P2ChipLayout L;
    L.W = 16, L.RP = 13, L.width = 314;
    for (uint32_t t = 0; t < queries * n_groups; t++) {
        if (m4) p3k::fri_open_sponge_lane<1>(a, t, tab, L);
        else p3k::fri_open_sponge_lane<0>(a, t, tab, L);
    }
    for (size_t r = 0; r < (size_t)queries * rows_per_query; r++) p3k::fri_open_fill_lane(a, r);
    for (uint32_t t = 0; t < queries * n_batches; t++) {
        if (m4) p3k::fri_open_ipath_lane<1>(a, t, tab, L);
        else p3k::fri_open_ipath_lane<0>(a, t, tab, L);
    }
    for (size_t row = 0; row < chip_n; row++) {
        if (m4) p3k::chip_row<16, 13, 1>(chip + row * L.width, chip_in + row * 16, chip_mult[row], tab, L);
        else p3k::chip_row<16, 13, 0>(chip + row * L.width, chip_in + row * 16, chip_mult[row], tab, L);
    }
    for (size_t row = 0; row < state_n; row++) {
        if (m4) p3k::chip_row<16, 13, 1>(state + row * L.width, sin.data() + row * 16, smult[row], tab, L);
        else p3k::chip_row<16, 13, 0>(state + row * L.width, sin.data() + row * 16, smult[row], tab, L);
    }
    return 0;
}

}  // extern "C"
