// TEST INFRASTRUCTURE: what rk_fri_transcript_rows_device adds to the open statement's stages, run on the CPU in the order
// of the launches of fri_tables.hip (lane bodies: raiko_amd/csrc/p3_kernels.hpp): the fold lanes with the columns X and
// FIRST, the challenger's chain as one lane walks it (p3k::fri_transcript_chain_lane; the GPU kernel spreads the same
// steps over one lane per cell), the fill lanes of the transcript and bits rows, and chip_row over the state chip's inputs.
// state_in / state_mult arrive with the sponge's inputs (rows below state_base) filled in; fold, transcript and bits must
// arrive zeroed, as the library clears them.
#include <vector>

#include "p3_kernels.hpp"

extern "C" {

// tab = rc_ext 128 | rc_int 13 | diag 16 (Montgomery words); steps: FRI_TRANSCRIPT_STEP_WORDS plain words per permutation
int emul_fri_transcript_rows(uint32_t log_max, uint32_t blowup_log2, uint32_t queries, uint32_t gen_l, uint32_t wm, uint32_t shiftm,
                             const uint32_t* fold_pub, const uint32_t* fold_rec, uint32_t n_steps, uint32_t pow_bits, size_t state_base,
                             const uint32_t* steps, const uint32_t* observed, const uint32_t* tab, int m4, uint32_t* fold, uint32_t* transcript,
                             uint32_t* bits, uint32_t* state_in, uint32_t* state_mult, uint32_t* state, size_t state_n) {
    p3k::FriArgs f{};
    f.L = log_max, f.R = log_max - blowup_log2, f.Q = queries, f.gen_l = gen_l, f.wm = wm, f.pub = fold_pub, f.rec = fold_rec;
    f.xcol = 1, f.shiftm = shiftm, f.firstcol = 1;
    f.fold = fold;
    for (uint32_t q = 0; q < queries; q++) p3k::fri_fold_lane(f, q);
    std::vector<uint32_t> samples((size_t)queries + 1, 0);
    p3k::FriTranscriptArgs a{};
    a.N = n_steps, a.Q = queries, a.L = log_max, a.pow_bits = pow_bits, a.state_base = state_base;
    a.steps = steps, a.observed = observed, a.transcript = transcript, a.bits = bits;
    a.state_in = state_in, a.state_mult = state_mult, a.samples = samples.data();
    p3k::P2ChipLayout L;
    L.W = 16, L.RP = 13, L.width = 314;
    if (m4) p3k::fri_transcript_chain_lane<1>(a, tab, L);
    else p3k::fri_transcript_chain_lane<0>(a, tab, L);
    for (uint32_t t = 0; t < n_steps + queries + 1; t++) {
        if (t < a.N) p3k::fri_transcript_fill_lane(a, t);
        else p3k::fri_bits_fill_lane(a, t - a.N);
    }
    for (size_t row = 0; row < state_n; row++) {
        if (m4) p3k::chip_row<16, 13, 1>(state + row * L.width, state_in + row * 16, state_mult[row], tab, L);
        else p3k::chip_row<16, 13, 0>(state + row * L.width, state_in + row * 16, state_mult[row], tab, L);
    }
    return 0;
}

}  // extern "C"
