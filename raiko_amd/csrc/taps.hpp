// Host-only shape checks of the C ABI: TapSet validation, the integer facts of a seal's shape that prover,
// verifier and bound share, and the seal-size bound.  No HIP dependency, so tests/asan/ can build exactly
// this code with -fsanitize=address on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/raiko_hip.h"

namespace rk {

constexpr unsigned MAX_PO2_PLUS_2 = 24;  // = ntt::LAMBDA: the 4x domain of the largest segment

// TapSet validation shared by the prover, the seal bound and the verifier: registers sorted by
// (group, offset) covering every column once, combo ids in range, combo_off strictly increasing
// from 0, backs of a combo increasing (as risc0-zkp taps.rs builds them) and <= 64.
inline int check_taps(const rk_taps& t) {
    if (!t.reg_group || !t.reg_offset || !t.reg_combo || !t.combo_off || !t.combo_backs) return RK_ERR_INVALID;
    if ((size_t)t.group_size[0] + t.group_size[1] + t.group_size[2] != t.n_regs) return RK_ERR_INVALID;
    if (t.n_combos == 0 || t.n_combos > (1u << 16)) return RK_ERR_INVALID;
    uint32_t r = 0;
    for (uint32_t g = 0; g < 3; g++)
        for (uint32_t o = 0; o < t.group_size[g]; o++, r++) {
            if (t.reg_group[r] != g || t.reg_offset[r] != o) return RK_ERR_INVALID;
            if (t.reg_combo[r] >= t.n_combos) return RK_ERR_INVALID;
        }
    if (t.combo_off[0] != 0) return RK_ERR_INVALID;
    for (uint32_t c = 0; c < t.n_combos; c++) {
        if (t.combo_off[c + 1] <= t.combo_off[c]) return RK_ERR_INVALID;
        if (t.combo_backs[t.combo_off[c]] > 64) return RK_ERR_INVALID;
        // backs of a combo are distinct (each is divided out once) and increasing, as TapSet builds them
        for (uint32_t b = t.combo_off[c] + 1; b < t.combo_off[c + 1]; b++)
            if (t.combo_backs[b] <= t.combo_backs[b - 1] || t.combo_backs[b] > 64) return RK_ERR_INVALID;
    }
    return RK_OK;
}

// the protocol shape of a segment proof (rk_params): risc0's by default
struct Shape {
    uint32_t queries = 50, blowup_log2 = 2, fold_log2 = 4, min_degree = 256, pow_bits = 0;
};
inline bool shape_ok(const Shape& s) {
    return s.queries >= 1 && s.queries <= RK_MAX_QUERIES && s.blowup_log2 >= 1 && s.blowup_log2 <= 4 && s.fold_log2 >= 1 &&
           s.fold_log2 <= 4 && s.min_degree >= 1 && !(s.min_degree & (s.min_degree - 1)) && s.pow_bits <= 24;
}

// ---- the integer facts of a seal's shape, stated once for MerkleDev / TreeVerifier, the prover's and the verifier's
// FRI loops and the bound below.  Tap sets are assumed to have passed check_taps.
inline size_t ceil_log2(size_t n) {
    size_t k = 0;
    while (((size_t)1 << k) < n) k++;
    return k;
}
inline size_t combo_taps(const rk_taps& t, size_t c) { return t.combo_off[c + 1] - t.combo_off[c]; }
inline size_t reg_taps(const rk_taps& t, uint32_t r) { return combo_taps(t, t.reg_combo[r]); }
inline size_t total_taps(const rk_taps& t) {
    size_t n = 0;
    for (uint32_t r = 0; r < t.n_regs; r++) n += reg_taps(t, r);
    return n;
}
inline uint32_t max_back(const rk_taps& t) {
    uint32_t m = 0;
    for (uint32_t b = 0; b < t.combo_off[t.n_combos]; b++)
        if (t.combo_backs[b] > m) m = t.combo_backs[b];
    return m;
}
// MerkleTreeParams: the layer sent as a tree's cap is the largest i < layers with 2^i <= queries (0: the root alone)
inline size_t merkle_top_layer(size_t rows, size_t queries) {
    const size_t layers = ceil_log2(rows);
    size_t top_layer = 0;
    for (size_t i = 1; i < layers; i++) {
        if (((size_t)1 << i) > queries) break;
        top_layer = i;
    }
    return top_layer;
}
// fri_prove's loop: per_round(size, domain) for every round that commits a polynomial of `size` coefficients on its
// `domain` = size << blow-up points and folds it; returns the degree of the final polynomial
template <class F>
inline size_t fri_walk(size_t n, const Shape& sh, F&& per_round) {
    const size_t fold = (size_t)1 << sh.fold_log2;
    size_t size = n;
    while (size > sh.min_degree && size >= fold) {
        per_round(size, size << sh.blowup_log2);
        size /= fold;
    }
    return size;
}

// upper bound on the seal words of a segment under a protocol shape; 0 for one rk_prove_segment would reject
inline size_t seal_bound_words(const rk_segment* seg, const Shape& sh = Shape()) {
    if (!seg || !shape_ok(sh) || seg->po2 < 1 || seg->po2 + sh.blowup_log2 > MAX_PO2_PLUS_2) return 0;
    const rk_taps& t = seg->taps;
    if (check_taps(t) != RK_OK) return 0;
    const size_t queries = sh.queries, fold = (size_t)1 << sh.fold_log2;
    const size_t check_size = (size_t)4 << sh.blowup_log2;
    const size_t N = (size_t)1 << seg->po2, D = N << sh.blowup_log2;
    const size_t layers = ceil_log2(D);
    const size_t w_all = (size_t)t.group_size[0] + t.group_size[1] + t.group_size[2] + check_size;
    // no tree's cap is wider than that of a tree too tall to limit it, and no path longer than the whole height
    const size_t top = (size_t)1 << merkle_top_layer((size_t)1 << (8 * sizeof(size_t) - 1), queries);
    size_t words = (size_t)seg->n_globals + 1;
    words += 4 * top * 8;                     // top layers of the four trace trees
    words += (total_taps(t) + check_size) * 4;     // coeff_u
    words += queries * (w_all + 4 * layers * 8);   // trace openings
    const size_t final_degree = fri_walk(N, sh, [&](size_t, size_t domain) {
        words += top * 8 + queries * (fold * 4 + ceil_log2(domain / fold) * 8);
    });
    words += final_degree * 4;
    return words + 64;                        // + the proof-of-work nonce and slack
}
inline size_t seal_bound_words(const rk_segment* seg, size_t queries) {
    Shape sh;
    sh.queries = (uint32_t)queries;
    return queries > RK_MAX_QUERIES ? 0 : seal_bound_words(seg, sh);
}

}  // namespace rk
