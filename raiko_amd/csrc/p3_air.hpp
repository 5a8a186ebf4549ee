// Shared by p3_air.hip (the AIR front end: rk_air_*, the lookup constraints, the Poseidon2 chip), fri_tables.hip (the rows
// of the FRI lookup tables) and p3.hip / p3_verify.hip (prover, verifier): what an rk_air holds and the Poseidon2 chip as
// the FRI tables feed it.  (The scoped device buffer all of them use is rk::DevBuf of internal.hpp.)
#pragma once
#include "internal.hpp"
#include "circuit_program.hpp"
#include "p3_kernels.hpp"

#include <vector>

struct rk_air {
    std::vector<rk_air_step> steps;
    std::vector<uint32_t> lookups;   // flat interactions (rk_air_create_lookup): constants as Montgomery words, columns as slots of `used`
    std::vector<uint32_t> used;      // the distinct columns the interactions read: c < width main trace, else preprocessed column c - width
    uint32_t n_lookups = 0, perm_width = 0, n_chal = 0;   // base columns of the permutation trace, words of the challenge vector
    uint32_t width = 0, n_public = 0;
    uint32_t prep_width = 0;         // preprocessed columns (rk_air_create_prep): committed once in an rk_p3_key, not part of the trace
    bool perm_reads_prep = false;    // an interaction names a preprocessed column: the permutation trace needs the key's rows
    rk_air_info info{};
    uint32_t sel_mask = 0;   // bit c: selector column c (is_first_row, is_last_row, is_transition) is named by the list
    rk_program* prog = nullptr;
};

namespace rk {

constexpr uint32_t NEXT_BACK = 0xffffffffu;  // a tap "one row ahead": back = -1 modulo any power-of-two domain

// the Poseidon2 chip of an instance: where its columns are, and the constants its lanes read
inline p3k::P2ChipLayout p2_chip_layout(const p2::Any& k) {
    p3k::P2ChipLayout L;
    L.W = (uint32_t)k.cells();
    L.RP = (uint32_t)k.rounds_partial();
    L.width = L.W + 16 * L.W + 2 * L.RP - 1 + L.W + 1;
    return L;
}
inline std::vector<uint32_t> p2_chip_tab(const p2::Any& k) {   // rc_ext | rc_int | diag: what p3k::chip_permute reads
    const p3k::P2ChipLayout L = p2_chip_layout(k);
    std::vector<uint32_t> tab(k.rc_ext(), k.rc_ext() + 8 * L.W);
    tab.insert(tab.end(), k.rc_int(), k.rc_int() + L.RP);
    tab.insert(tab.end(), k.diag(), k.diag() + L.W);
    return tab;
}
// rk_p2_chip_trace behind its argument checks (0 < n <= 2^24, the context's device current), reading the constants from
// d_tab: p2_chip_tab of the context's instance, uploaded by the caller (p3_air.hip)
int p2_chip_trace(rk_ctx* ctx, const uint32_t* d_tab, const p3k::P2ChipLayout& L, const uint32_t* d_in, const uint32_t* d_mult, size_t n, uint32_t* d_out);

}  // namespace rk
