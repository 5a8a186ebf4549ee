// CPU walk through the lane body of the Keccak-f[1600] chip's rows kernel (kc::keccak_chip_lane, raiko_amd/csrc/keccak_chip.hpp):
// where the GPU runs one wavefront per permutation slot (keccak_chip.hip), this runs lanes 0..63 of every slot in turn.
// Built by tests/test_keccak_chip.py, which compares the table with tests/keccak_chip_ref.py word for word.
#include <cstddef>
#include <cstdint>

#include "keccak_chip.hpp"

extern "C" uint32_t emul_keccak_chip_width() { return kc::KeccakChipLayout::WIDTH; }

// states n x 25 lanes; ids / mult n Montgomery words or null; trace rows x width Montgomery words; out null or n x 25 lanes
extern "C" void emul_keccak_chip_rows(const uint64_t* states, const uint32_t* ids, const uint32_t* mult, size_t n, size_t rows, uint32_t* trace,
                                      uint64_t* out) {
    const kc::KeccakChipArgs a{states, ids, mult, n, rows, trace, out};
    const size_t slots = (rows + 24) / 25;
    for (size_t slot = 0; slot < slots; slot++)
        for (uint32_t lane = 0; lane < 64; lane++) kc::keccak_chip_lane(a, slot, lane);
}
