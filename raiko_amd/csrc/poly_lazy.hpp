// Lazy accumulation of sum_i v_i * m_i for canonical Montgomery words v_i and extension elements m_i, the inner
// loop of the DEEP stage's streaming kernels (eval_dot_kernel, mix_kernel in kernels_poly.hip).
//
// bb::add(acc, bb::scale(m, v)) pays a Montgomery reduction and a modular add per component and term: 32 VALU
// instructions per term.  Here the 32 x 32-bit products are summed exactly in four unsigned 64-bit accumulators (one
// v_mad_u64_u32 per component and term), brought back under 2^60 every FOLD_TERMS terms by one more v_mad_u64_u32,
// and Montgomery-reduced once at the end: 5 instructions per term.
//
// Worst-case bounds (p = 2013265921, p^2 < 2^61.82; every input word is canonical, <= p - 1):
//   term        v * m.c[j] <= (p - 1)^2                                  = 4053239664633446400 < 2^61.82
//   fold(t)     = hi32(t) * (2^32 mod p) + lo32(t), 2^32 mod p = 2^28 - 2, the same residue as t;
//               <= (2^32 - 1) * (2^28 - 2) + (2^32 - 1) = (2^32 - 1) * (2^28 - 1)
//                                                                        = 1152921500043444225 < 2^60, for ANY 64-bit t
//   accumulator fold(..) + FOLD_TERMS terms <= 1152921500043444225 + 4 * 4053239664633446400
//                                                                        = 17365880158577229825 < 2^64 = 18446744073709551616
//               (a fifth term would reach 21419119823210676225 > 2^64: FOLD_TERMS = 4 is the most that fits)
//   finish      fold(t) < 2^60 < 2^63 as bb::uredc64 requires; uredc64 returns < 2^60 / 2^32 + p = 2^28 + p < 2p,
//               one conditional subtraction from canonical.
// So: starting from zero or from a folded value, at most FOLD_TERMS calls of mac() between two fold()s, and finish()
// at any point of that cycle.  The result is (sum_i v_i * m_i) * 2^-32 mod p per component, canonical: word for word
// what the chain of bb::add(acc, bb::scale(m_i, v_i)) gives.
#pragma once
#include "bb.hpp"

namespace pl {

constexpr int FOLD_TERMS = 4;
constexpr uint32_t TWO32_MOD_P = 268435454u;  // 2^32 - 2p = 2^28 - 2
static_assert((uint64_t)TWO32_MOD_P == ((uint64_t)1 << 32) % bb::P, "2^32 mod p");

struct Acc {
    uint64_t a[4];
};
RK_HD Acc zero() { return Acc{{0, 0, 0, 0}}; }
// acc += v * m, exact
RK_HD void mac(Acc& s, uint32_t v, const bb::Ext& m) {
#pragma unroll
    for (int j = 0; j < 4; j++) s.a[j] += (uint64_t)v * m.c[j];
}
// the same residue below 2^60, for any 64-bit t
RK_HD uint64_t fold(uint64_t t) { return (uint64_t)(uint32_t)(t >> 32) * TWO32_MOD_P + (uint32_t)t; }
RK_HD void fold(Acc& s) {
#pragma unroll
    for (int j = 0; j < 4; j++) s.a[j] = fold(s.a[j]);
}
// acc * 2^-32 mod p, canonical
RK_HD bb::Ext finish(const Acc& s) {
    bb::Ext r;
#pragma unroll
    for (int j = 0; j < 4; j++) r.c[j] = bb::ucanon(bb::uredc64(fold(s.a[j])));
    return r;
}

}  // namespace pl
