// The preprocessed matrices of the keyed rv32 chip sets (include/raiko_hip.h: rk_rv32elf_prep_device,
// rk_rv32mem_prep_device, rk_rv32io_prep_device): the tuple columns of the program, byte, range and shift tables over a
// program image, written once per key.  The full rows are rv32_rows.hpp's lane bodies; prep_tile picks the tuple cells.
#include <algorithm>
#include <string>

#include "rv32_tiles.hpp"

namespace rv32 {

template <int MEM>   // 0: rv32im-elf's 42 columns; 1: rv32im-mem's 48; 2: the io form's 48 (the ecall word reads a0, a1)
__global__ void program_prep_kernel(const uint32_t* __restrict__ words, uint32_t n_words, const Image img, size_t n_rows,
                                    uint32_t* __restrict__ out) {
    extern __shared__ uint32_t s_rows[];
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    prep_tile<IM_PROG_W, MEM ? MEM_PROG_W : ELF_PROG_W>(
        s_rows, out, (size_t)blockIdx.x * blockDim.x, n_rows,
        [&](uint32_t* row) {
            if (s >= n_rows) return;
            const bool in = s < n_words;
            const uint32_t pc = in ? image_pc(img, (uint32_t)s) : 0u, ins = in ? words[s] : 0u;
            const Dec d = decode(ins);
            program_row_i(row, pc, ins, d, 0u);
            program_row_cf(row, d);
            program_row_im(row, ins, d);
        },
        [](uint32_t* o, const uint32_t* row) {
            if constexpr (MEM == 2) program_prep_row_io(o, row, decode(row[2] | row[3] << 16));
            else if constexpr (MEM == 1) program_prep_row_mem(o, row, decode(row[2] | row[3] << 16));
            else program_prep_row(o, row);
        });
}

__global__ void byte_prep_kernel(uint32_t* __restrict__ out) {
    extern __shared__ uint32_t s_rows[];
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    prep_tile<BYTE_W, ELF_TUPLE_W>(
        s_rows, out, (size_t)blockIdx.x * blockDim.x, (size_t)1 << RK_RV32_BYTE_LOG_ROWS,
        [&](uint32_t* row) {
            if (r < (3u << 16)) byte_row(row, r, 0u);
        },
        [](uint32_t* o, const uint32_t* row) { byte_prep_row(o, row); });
}

__global__ void shift_prep_kernel(uint32_t* __restrict__ out) {
    extern __shared__ uint32_t s_rows[];
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    prep_tile<SHIFT_W, ELF_TUPLE_W>(
        s_rows, out, (size_t)blockIdx.x * blockDim.x, (size_t)1 << RK_RV32CF_SHIFT_LOG_ROWS,
        [&](uint32_t* row) { shift_row(row, r, 0u); }, [](uint32_t* o, const uint32_t* row) { shift_prep_row(o, row); });
}

__global__ void range_prep_kernel(uint32_t* __restrict__ out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < (1u << 16)) out[v] = enc(v);
}

// the four preprocessed matrices of an image (rk_rv32elf_prep_device): everything is checked before the first launch
template <int MEM>
static int prep_device(rk_ctx* ctx, const Image& img, const uint32_t* words, size_t n_words, uint32_t* d_program, size_t program_rows,
                       uint32_t* d_byte, uint32_t* d_range, uint32_t* d_shift) {
    if (!ctx || !d_program || !d_byte || !d_range || !d_shift || (n_words && !words)) return RK_ERR_INVALID;
    if (n_words > (1u << 22) || rows_for(n_words, 1) != program_rows) return RK_ERR_CAPACITY;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    void* d_words = nullptr;
    RK_TRY(rk::dev_alloc(ctx, std::max<size_t>(n_words, 1) * 4, &d_words));
    auto enqueue = [&]() -> int {
        if (n_words) RK_HIP_TRY(ctx, hipMemcpyAsync(d_words, words, n_words * 4, hipMemcpyHostToDevice, ctx->stream));
        const unsigned pb = (unsigned)std::min<size_t>(program_rows, TB);
        RK_TRY(rk::launch(ctx, "rv32 program_prep_kernel", program_prep_kernel<MEM>, (unsigned)(program_rows / pb), pb,
                          pb * (IM_PROG_W | 1) * 4, (const uint32_t*)d_words, (uint32_t)n_words, img, program_rows, d_program));
        RK_TRY(rk::launch(ctx, "rv32 byte_prep_kernel", byte_prep_kernel, (1u << RK_RV32_BYTE_LOG_ROWS) / TB, TB, TB * (BYTE_W | 1) * 4,
                          d_byte));
        RK_TRY(rk::launch(ctx, "rv32 range_prep_kernel", range_prep_kernel, (1u << 16) / 256, 256, 0, d_range));
        return rk::launch(ctx, "rv32 shift_prep_kernel", shift_prep_kernel, (1u << RK_RV32CF_SHIFT_LOG_ROWS) / TB, TB,
                          TB * (SHIFT_W | 1) * 4, d_shift);
    };
    int st = enqueue();
    const hipError_t e = hipStreamSynchronize(ctx->stream);   // the caller's `words` and the scratch are free to go
    if (e != hipSuccess && st == RK_OK) {
        ctx->last_error = std::string("rk_rv32elf_prep_device sync: ") + hipGetErrorString(e);
        st = RK_ERR_HIP;
    }
    rk::dev_free(ctx, d_words);
    return st;
}

// the caller's segment table and words -> prep_device<MEM>
template <int MEM>
static int prep_entry(rk_ctx* ctx, const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs, const uint32_t* words,
                      size_t n_words, uint32_t* d_program, size_t program_rows, uint32_t* d_byte, uint32_t* d_range, uint32_t* d_shift) {
    Image img;
    size_t total = 0;
    RK_TRY(image_of(seg_vaddr, seg_words, n_segs, &img, &total));
    if (total != n_words) return RK_ERR_INVALID;
    return prep_device<MEM>(ctx, img, words, n_words, d_program, program_rows, d_byte, d_range, d_shift);
}

}  // namespace rv32

extern "C" {

int rk_rv32elf_prep_device(rk_ctx* ctx, const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs,
                           const uint32_t* words, size_t n_words, uint32_t* d_program, size_t program_rows, uint32_t* d_byte,
                           uint32_t* d_range, uint32_t* d_shift) {
    RK_GUARD_BEGIN
    return rv32::prep_entry<0>(ctx, seg_vaddr, seg_words, n_segs, words, n_words, d_program, program_rows, d_byte, d_range, d_shift);
    RK_GUARD_END
}
int rk_rv32mem_prep_device(rk_ctx* ctx, const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs,
                           const uint32_t* words, size_t n_words, uint32_t* d_program, size_t program_rows, uint32_t* d_byte,
                           uint32_t* d_range, uint32_t* d_shift) {
    RK_GUARD_BEGIN
    return rv32::prep_entry<1>(ctx, seg_vaddr, seg_words, n_segs, words, n_words, d_program, program_rows, d_byte, d_range, d_shift);
    RK_GUARD_END
}
int rk_rv32io_prep_device(rk_ctx* ctx, const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs,
                          const uint32_t* words, size_t n_words, uint32_t* d_program, size_t program_rows, uint32_t* d_byte,
                          uint32_t* d_range, uint32_t* d_shift) {
    RK_GUARD_BEGIN
    return rv32::prep_entry<2>(ctx, seg_vaddr, seg_words, n_segs, words, n_words, d_program, program_rows, d_byte, d_range, d_shift);
    RK_GUARD_END
}

}  // extern "C"
