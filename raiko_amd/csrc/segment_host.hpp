// What the segment prover (prover.hip) and its host verifier (verify.hip) share at field level: the header binding, the
// points the tap set is opened at, and the fold of the tap openings into one small polynomial per combo.  The integer
// facts of a seal's shape (taps per register, Merkle cap, FRI round walk) are in taps.hpp.
#pragma once
#include "internal.hpp"

namespace rk {

using bb::Ext;

// What both sides absorb before the first commitment: the two info arrays, then the globals and po2 in one digest.
// `sponge` has mix(digest); the prover also writes globals and po2 to the seal, the verifier has read them from it and
// compared them with `pub` before it calls this.
template <class Sponge>
void bind_header(const p2::Any& k, Sponge& sponge, const rk_segment* pub) {
    uint32_t digest[8], e[16];
    for (int i = 0; i < 16; i++) e[i] = bb::encode(pub->proof_system_info[i]);
    k.hash_elems(e, 16, digest);
    sponge.mix(digest);
    for (int i = 0; i < 16; i++) e[i] = bb::encode(pub->circuit_info[i]);
    k.hash_elems(e, 16, digest);
    sponge.mix(digest);
    std::vector<uint32_t> io(pub->globals, pub->globals + pub->n_globals);
    io.push_back(bb::encode(pub->po2));
    k.hash_elems(io.data(), io.size(), digest);
    sponge.mix(digest);
}

// The points of the DEEP stage for a segment of 2^po2 rows: slot b <= max_back holds z * back_one^b (a register read
// `b` rows back is opened there), the last slot z^(D/N) (where the D/N parts of the check polynomial are opened).
inline std::vector<Ext> tap_points(const Sys& sys, uint32_t po2, const rk_taps& taps, const Ext& z) {
    const uint32_t back_one = bb::inv(bb::pow(sys.root27m, (uint64_t)1 << (27 - po2)));
    const uint32_t far = max_back(taps);
    std::vector<Ext> pts(far + 2);
    for (uint32_t b = 0; b <= far; b++) pts[b] = bb::scale(z, bb::pow(back_one, b));
    pts[far + 1] = bb::pow(z, (uint64_t)1 << sys.blowup_log2, sys.wm);
    return pts;
}

// coeff_u (one interpolating polynomial per register, then the check_size check openings) folded under the powers of
// `mix` in register order: the polynomial every combo's mixed column must agree with at its tap points, coefficient i
// of combo c at combo_off[c] + i, and the mixed check openings (a constant) last.
inline std::vector<Ext> combo_u(const rk_taps& taps, const std::vector<Ext>& coeff_u, const Ext& mix, size_t check_size, uint32_t wm) {
    const size_t tot_backs = taps.combo_off[taps.n_combos];
    std::vector<Ext> out(tot_backs + 1, bb::ext_zero());
    Ext cur = bb::ext_one();
    size_t pos = 0;
    for (uint32_t r = 0; r < taps.n_regs; r++) {
        const size_t at = taps.combo_off[taps.reg_combo[r]], sz = reg_taps(taps, r);
        for (size_t j = 0; j < sz; j++) out[at + j] = bb::add(out[at + j], bb::mul(cur, coeff_u[pos + j], wm));
        cur = bb::mul(cur, mix, wm);
        pos += sz;
    }
    for (size_t i = 0; i < check_size; i++) {
        out[tot_backs] = bb::add(out[tot_backs], bb::mul(cur, coeff_u[pos++], wm));
        cur = bb::mul(cur, mix, wm);
    }
    return out;
}

}  // namespace rk
