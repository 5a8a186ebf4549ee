// CPU walk through the lane body of the Keccak-256 sponge table's rows kernel (kc::keccak_sponge_lane,
// raiko_amd/csrc/keccak_sponge.hpp): where the GPU runs one wavefront per block slot (keccak_sponge.hip), this runs lanes
// 0..63 of every slot in turn.  Built by tests/test_keccak_sponge.py, which compares the table with
// tests/keccak_sponge_ref.py word for word.
#include <cstddef>
#include <cstdint>

#include "keccak_sponge.hpp"

extern "C" uint32_t emul_keccak_sponge_width() { return kc::KeccakSpongeLayout::WIDTH; }

// blocks n_blocks x 17 lanes; first n_msgs + 1; msg_ids n_msgs Montgomery words or null; states / outs n_blocks x 25 lanes
// (what the chain kernel leaves); trace rows x width Montgomery words
extern "C" void emul_keccak_sponge_rows(const uint64_t* blocks, const uint32_t* first, const uint32_t* msg_ids, const uint64_t* states,
                                        const uint64_t* outs, size_t n_msgs, size_t n_blocks, size_t rows, uint32_t* trace) {
    const kc::KeccakSpongeArgs a{blocks, first, msg_ids, states, outs, n_msgs, n_blocks, rows, trace};
    const size_t slots = (rows + kc::KeccakSpongeLayout::ROWS - 1) / kc::KeccakSpongeLayout::ROWS;
    for (size_t slot = 0; slot < slots; slot++)
        for (uint32_t lane = 0; lane < 64; lane++) kc::keccak_sponge_lane(a, slot, lane);
}
