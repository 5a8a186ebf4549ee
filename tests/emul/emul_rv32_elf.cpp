// CPU walk through the rv32im-elf lane bodies of raiko_amd/csrc/rv32_rows.hpp: the four preprocessed matrices of a
// program image (each full row built by the rv32im bodies, its tuple cells selected) and the program table's count
// column of a recorded trace (image_row of every pc, the executed word compared with the image's), in Montgomery form.
// Built by tests/test_rv32_elf_chips.py, which compares them with raiko_amd/rv32elf.py word for word.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rv32_rows.hpp"

using namespace rv32;

static Image image_of(const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs) {
    Image im{};
    im.n_segs = n_segs;
    for (uint32_t k = 0; k < n_segs; k++) im.vaddr[k] = seg_vaddr[k], im.words[k] = seg_words[k];
    return im;
}

// program: program_rows x 42, byte: 2^18 x 4, range: 2^16, shift: 2^12 x 4.  -> 0, or 1 for more segments than the table holds
extern "C" int emul_rv32elf_prep(const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs, const uint32_t* words,
                                 size_t n_words, uint32_t* program, size_t program_rows, uint32_t* byte, uint32_t* range,
                                 uint32_t* shift) {
    if (n_segs > RK_RV32ELF_MAX_SEGMENTS) return 1;
    const Image im = image_of(seg_vaddr, seg_words, n_segs);
    for (size_t s = 0; s < program_rows; s++) {
        uint32_t full[IM_PROG_W] = {0}, o[ELF_PROG_W];
        const bool in = s < n_words;
        const uint32_t pc = in ? image_pc(im, (uint32_t)s) : 0u, ins = in ? words[s] : 0u;
        const Dec d = decode(ins);
        program_row_i(full, pc, ins, d, 0u);
        program_row_cf(full, d);
        program_row_im(full, ins, d);
        program_prep_row(o, full);
        for (unsigned c = 0; c < ELF_PROG_W; c++) program[s * ELF_PROG_W + c] = enc(o[c]);
    }
    for (size_t r = 0; r < ((size_t)1 << RK_RV32_BYTE_LOG_ROWS); r++) {
        uint32_t full[BYTE_W] = {0}, o[ELF_TUPLE_W];
        if (r < (3u << 16)) byte_row(full, r, 0u);
        byte_prep_row(o, full);
        for (unsigned c = 0; c < ELF_TUPLE_W; c++) byte[r * ELF_TUPLE_W + c] = enc(o[c]);
    }
    for (uint32_t v = 0; v < (1u << 16); v++) range[v] = enc(v);
    for (size_t r = 0; r < ((size_t)1 << RK_RV32CF_SHIFT_LOG_ROWS); r++) {
        uint32_t full[SHIFT_W] = {0}, o[ELF_TUPLE_W];
        shift_row(full, r, 0u);
        shift_prep_row(o, full);
        for (unsigned c = 0; c < ELF_TUPLE_W; c++) shift[r * ELF_TUPLE_W + c] = enc(o[c]);
    }
    return 0;
}

// trace: cycles x (pc, ins, a, b, res, next, wr); mult: program_rows words.  -> 0, 1 an executed word is not the image's,
// 2 a pc outside the image
extern "C" int emul_rv32elf_program_mult(const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs,
                                         const uint32_t* words, size_t n_words, const uint32_t* trace, size_t cycles,
                                         uint32_t* mult, size_t program_rows) {
    const Image im = image_of(seg_vaddr, seg_words, n_segs);
    std::vector<uint32_t> count(program_rows, 0);
    for (size_t i = 0; i < cycles; i++) {
        const uint32_t pc = trace[7 * i], ins = trace[7 * i + 1];
        const uint32_t slot = image_row(im, pc);
        if (slot >= n_words) return 2;
        if (words[slot] != ins) return 1;
        count[slot]++;
    }
    for (size_t s = 0; s < program_rows; s++) mult[s] = enc(count[s]);
    return 0;
}
