// What the three rv32 translation units share (rv32_shards.hip, rv32_prep.hip, rv32_link.hip): the block size, the
// wave-aggregated histogram add, the LDS staging of a row-major tile, and two host helpers -- a table's rows for a count
// and the caller's segment table as the kernels take it.
#pragma once
#include "internal.hpp"
#include "rv32_rows.hpp"

namespace rv32 {

constexpr unsigned TB = 128;   // rows per block (the cpu rows kernel stages TB x 69 words in LDS, 121 / 133 / 141 for rv32i-cf / rv32im / rv32im-mem)

// a histogram bin += 1 for every lane with `on`; the lanes of a wave that agree with its first active lane add once
__device__ inline void hist_add(uint32_t* h, uint32_t v, bool on) {
    const uint64_t act = __ballot(on);
    if (!act) return;
    const int first = __ffsll((unsigned long long)act) - 1;
    const uint32_t lv = __shfl(v, first);
    const uint64_t same = __ballot(on && v == lv);
    if ((int)(threadIdx.x & 63) == first) atomicAdd(&h[lv], (uint32_t)__popcll(same));
    else if (on && v != lv) atomicAdd(&h[v], 1u);
}

// One tile of a row-major table, a row of W words per lane: the lane's row is zeroed in LDS (s_rows: blockDim.x x (W | 1)
// words; the odd stride avoids bank conflicts), fill(row) writes its canonical cells, every cell goes to Montgomery form
// and the tile's rows r0 .. of n_rows leave for HBM as whole lines.  Every lane of the block calls it.
template <unsigned W, class F>
__device__ __forceinline__ void row_tile(uint32_t* s_rows, uint32_t* out, size_t r0, size_t n_rows, F&& fill) {
    constexpr unsigned SW = W | 1;
    uint32_t* row = s_rows + threadIdx.x * SW;
    for (unsigned c = 0; c < W; c++) row[c] = 0;
    fill(row);
    for (unsigned c = 0; c < W; c++) row[c] = enc(row[c]);
    __syncthreads();
    const size_t rows = n_rows - r0 < blockDim.x ? n_rows - r0 : blockDim.x;
    for (size_t k = threadIdx.x; k < rows * W; k += blockDim.x) out[r0 * W + k] = s_rows[(k / W) * SW + k % W];
}

// One tile of a preprocessed matrix (rv32im-elf): the lane's FULL row of FW words is built in LDS as in row_tile, select
// picks its OW tuple cells, and only those leave for HBM, in Montgomery form, as whole lines.  Every lane of the block
// calls it.
template <unsigned FW, unsigned OW, class F, class S>
__device__ __forceinline__ void prep_tile(uint32_t* s_rows, uint32_t* out, size_t r0, size_t n_rows, F&& fill, S&& select) {
    constexpr unsigned SW = FW | 1;
    static_assert(OW <= FW, "the selected cells are staged in the full row's place");
    uint32_t* row = s_rows + threadIdx.x * SW;
    for (unsigned c = 0; c < FW; c++) row[c] = 0;
    fill(row);
    uint32_t o[OW];
    select(o, row);
#pragma unroll
    for (unsigned c = 0; c < OW; c++) row[c] = enc(o[c]);
    __syncthreads();
    const size_t rows = n_rows - r0 < blockDim.x ? n_rows - r0 : blockDim.x;
    for (size_t k = threadIdx.x; k < rows * OW; k += blockDim.x) out[r0 * OW + k] = s_rows[(k / OW) * SW + k % OW];
}

// the rows of a table that holds `count` of them: the power of two from 2^min_log up
inline size_t rows_for(size_t count, unsigned min_log) {
    size_t rows = (size_t)1 << min_log;
    while (rows < count) rows <<= 1;
    return rows;
}

// the caller's segment table as the kernels take it -> the image's words; RK_ERR_INVALID for more than
// RK_RV32ELF_MAX_SEGMENTS segments
inline int image_of(const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs, Image* img, size_t* n_words) {
    if (n_segs > RK_RV32ELF_MAX_SEGMENTS || (n_segs && (!seg_vaddr || !seg_words))) return RK_ERR_INVALID;
    *img = Image{};
    img->n_segs = n_segs;
    *n_words = 0;
    for (uint32_t k = 0; k < n_segs; k++) {
        img->vaddr[k] = seg_vaddr[k];
        img->words[k] = seg_words[k];
        *n_words += seg_words[k];
    }
    return RK_OK;
}

}  // namespace rv32
