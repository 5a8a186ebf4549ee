// Host build of the external layer and of the permutation variants of poseidon2_core.hpp, for tests/test_p2_ext_layer.py:
// the test builds this file twice, as shipped and with -DRK_P2_EXT_M4_FIRST (the earlier layer forms), and compares
// output words.  Every entry takes (width, m4) in {24, 16} x {0, 1}; a negative return means an unknown combination.
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <utility>

#include "bb.hpp"
#include "poseidon2_any.hpp"

namespace {

template <class F>
int with_core(int width, int m4, F&& f) {
    if (width == 24 && m4 == 0) return f(p2::K0{});
    if (width == 24 && m4 == 1) return f(p2::K1{});
    if (width == 16 && m4 == 0) return f(p2::K2{});
    if (width == 16 && m4 == 1) return f(p2::K3{});
    return -1;
}

template <class C>
const typename C::Consts& consts_of(const p2::Any& k) {
    if constexpr (C::CELLS == 24 && C::M4_KIND == 0) return k.k0;
    else if constexpr (C::CELLS == 24) return k.k1;
    else if constexpr (C::M4_KIND == 0) return k.k2;
    else return k.k3;
}

}  // namespace

extern "C" {

// 1 when this build has the earlier layer forms
int p2f_m4_first() {
#if defined(RK_P2_EXT_M4_FIRST)
    return 1;
#else
    return 0;
#endif
}

// the signed layer of the full rounds: n states of `width` signed-lazy cells in, as many REDC outputs out
int p2f_layer_signed(int width, int m4, int n, const int32_t* y, int32_t* r) {
    return with_core(width, m4, [&](auto core) {
        using C = decltype(core);
        for (int t = 0; t < n; t++) C::m_ext_redc_s(y + (size_t)t * C::CELLS, r + (size_t)t * C::CELLS);
        return 0;
    });
}

// the blocks b0 .. b0 + bn - 1 only; the other cells of r are left as the caller set them
int p2f_layer_signed_blocks(int width, int m4, int b0, int bn, int n, const int32_t* y, int32_t* r) {
    return with_core(width, m4, [&](auto core) {
        using C = decltype(core);
        constexpr int NB = C::CELLS / 4;
        for (int t = 0; t < n; t++) {
            const int32_t* yi = y + (size_t)t * C::CELLS;
            int32_t* ri = r + (size_t)t * C::CELLS;
            if (b0 == 0 && bn == 2) C::template m_ext_redc_s<0, 2>(yi, ri);
            else if (b0 == NB - 2 && bn == 2) C::template m_ext_redc_s<NB - 2, 2>(yi, ri);
            else if (b0 == 0 && bn == 1) C::template m_ext_redc_s<0, 1>(yi, ri);
            else if (b0 == (C::RATE - 1) / 4 && bn == 1) C::template m_ext_redc_s<(C::RATE - 1) / 4, 1>(yi, ri);
            else return -2;
        }
        return 0;
    });
}

// the unsigned first layer, in place, on n states of canonical cells; nz in {width, 16, 1}: the cells from nz on are
// known to be zero (and are zero in the input)
int p2f_layer_unsigned(int width, int m4, int nz, int n, uint32_t* s) {
    return with_core(width, m4, [&](auto core) {
        using C = decltype(core);
        for (int t = 0; t < n; t++) {
            uint32_t* si = s + (size_t)t * C::CELLS;
            if (nz == C::CELLS) C::m_ext_redc(si);
            else if (nz == 16) C::template m_ext_redc<16>(si);
            else if (nz == 1) C::template m_ext_redc<1>(si);
            else return -2;
        }
        return 0;
    });
}

// the permutation under the caller's tables (Montgomery form).  form: 0 full; 1 digest (cells 0..7); 2 capacity
// (the last 8 cells); 3 digest with the cells from 16 on zero (fold, compression); 4 digest with the cells from 1 on
// zero (the first permutation of the grind); 5 cells 0..3 (its second); 6 the block of the last rate cell.
// The cells outside the kept range are unspecified afterwards.
int p2f_permute(int width, int m4, int form, const uint32_t* rc_ext, const uint32_t* rc_int, const uint32_t* diag, uint32_t* cells) {
    static p2::Any k;
    k.set(width, m4, false, rc_ext, rc_int, diag);
    return with_core(width, m4, [&](auto core) {
        using C = decltype(core);
        const typename C::Consts& kc = consts_of<C>(k);
        switch (form) {
            case 0: C::permute(cells, kc); return 0;
            case 1: C::template permute<0, p2::OUT>(cells, kc); return 0;
            case 2: C::template permute<C::RATE, p2::OUT>(cells, kc); return 0;
            case 3: C::template permute<0, p2::OUT, 16>(cells, kc); return 0;
            case 4: C::template permute<0, p2::OUT, 1>(cells, kc); return 0;
            case 5: C::template permute<0, 4>(cells, kc); return 0;
            case 6: C::template permute<(C::RATE - 1) / 4 * 4, 4>(cells, kc); return 0;
            default: return -2;
        }
    });
}

}  // extern "C"
