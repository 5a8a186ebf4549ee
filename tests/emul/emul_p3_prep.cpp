// CPU emulation of perm_entries_kernel (raiko_amd/csrc/p3.hip) with a preprocessed matrix beside the main trace: the
// lane bodies of p3_kernels.hpp, phase 1 (staging) for every lane of a workgroup, then phase 2 (one row per lane).
// Built by tests/test_p3_prep.py; tests/emul/emul.cpp has the same loop for tables without preprocessed columns.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "p3_kernels.hpp"

extern "C" void emul_perm_entries_prep(uint32_t* out, const uint32_t* trace, const uint32_t* prep, const uint32_t* desc, size_t n, size_t w, size_t pw,
                                       uint32_t n_chal, uint32_t n_lookups, uint32_t wm, uint32_t n_used, uint32_t desc_words) {
    p3k::PermArgs a{out, trace, desc, n, w, n_chal, n_lookups, wm, n_used, desc_words, prep, pw};
    std::vector<uint32_t> tile((size_t)(n_used ? n_used : 1) * p3k::PERM_LD, 0xdeadbeefu);
    for (size_t blk = 0; blk < (n + p3k::PERM_ROWS - 1) / p3k::PERM_ROWS; blk++) {
        std::fill(tile.begin(), tile.end(), 0xdeadbeefu);      // a read of a slot nobody staged shows
        for (unsigned tid = 0; tid < (unsigned)p3k::PERM_ROWS; tid++) p3k::perm_stage(a, blk, tid, tile.data());
        for (unsigned tid = 0; tid < (unsigned)p3k::PERM_ROWS; tid++) p3k::perm_row(a, blk, tid, tile.data());
    }
}
