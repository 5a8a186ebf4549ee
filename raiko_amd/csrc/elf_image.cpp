// rk_exec_program_image and rk_exec_memory_image (include/raiko_hip.h): the executable image of an ELF and its whole
// memory image, listed with the loader's own walk of the program headers (elf_image.hpp).  Host only, plain C++.
#include <algorithm>
#include <map>
#include <new>
#include <vector>

#include "elf_image.hpp"

namespace {

// the executable image: the PF_X segments with file bytes, as (vaddr, words) in header order
struct ImageSeg {
    uint32_t vaddr;
    std::vector<uint32_t> words;
};
int program_image(const uint8_t* elf, size_t n, std::vector<ImageSeg>& out, std::string& err) {
    uint32_t entry = 0;
    const int walked = rk_elf::walk_load_segments(elf, n, &entry, err, [&](uint32_t off, uint32_t vaddr, uint32_t filesz, uint32_t flags) {
        if (!(flags & 1u) || filesz == 0) return (int)RK_OK;   // PF_X
        if (out.size() == RK_RV32ELF_MAX_SEGMENTS) {   // the 17th: refused before its bytes are copied
            err = "too many executable segments";
            return (int)RK_ERR_CAPACITY;
        }
        if (vaddr & 3) { err = "misaligned executable segment"; return (int)RK_ERR_INVALID; }
        ImageSeg s{vaddr, std::vector<uint32_t>(((size_t)filesz + 3) / 4, 0u)};
        for (uint32_t b = 0; b < filesz; b++) s.words[b >> 2] |= (uint32_t)elf[off + b] << (8 * (b & 3));
        out.push_back(std::move(s));
        return (int)RK_OK;
    });
    if (walked != RK_OK) return walked;
    for (size_t a = 0; a < out.size(); a++)
        for (size_t b = a + 1; b < out.size(); b++) {
            const uint64_t a0 = out[a].vaddr, a1 = a0 + 4 * (uint64_t)out[a].words.size(), b0 = out[b].vaddr,
                           b1 = b0 + 4 * (uint64_t)out[b].words.size();
            if (a0 < b1 && b0 < a1) { err = "overlapping executable segments"; return RK_ERR_INVALID; }
        }
    return RK_OK;
}

}  // namespace

extern "C" {

int rk_exec_program_image(const uint8_t* elf, size_t elf_bytes, uint32_t* seg_vaddr, uint32_t* seg_words, size_t seg_capacity,
                          size_t* n_segs, uint32_t* words, size_t word_capacity, size_t* n_words) {
    try {
        if (!elf || !n_segs || !n_words) return RK_ERR_INVALID;
        *n_segs = *n_words = 0;
        std::vector<ImageSeg> image;
        std::string err;
        const int st = program_image(elf, elf_bytes, image, err);
        if (st != RK_OK) return st;
        size_t total = 0;
        for (const ImageSeg& s : image) total += s.words.size();
        *n_segs = image.size();
        *n_words = total;
        if (image.size() > seg_capacity || total > word_capacity) return RK_ERR_CAPACITY;
        if ((!image.empty() && (!seg_vaddr || !seg_words)) || (total && !words)) return RK_ERR_INVALID;
        for (size_t k = 0, at = 0; k < image.size(); at += image[k].words.size(), k++) {
            seg_vaddr[k] = image[k].vaddr;
            seg_words[k] = (uint32_t)image[k].words.size();
            std::copy(image[k].words.begin(), image[k].words.end(), words + at);
        }
        return RK_OK;
    } catch (const std::bad_alloc&) {
        return RK_ERR_NOMEM;
    } catch (...) {
        return RK_ERR_INTERNAL;
    }
}

// the memory image: every word that holds a file byte of a PT_LOAD segment, the bytes stored in program-header order as
// the executor's loader stores them (a later segment overwrites an earlier one), the word's other bytes 0
int rk_exec_memory_image(const uint8_t* elf, size_t elf_bytes, uint32_t* out_addr, uint32_t* out_words, size_t capacity, size_t* n) {
    try {
        if (!elf || !n) return RK_ERR_INVALID;
        *n = 0;
        std::map<uint32_t, uint32_t> image;   // word address -> word, ascending
        std::string err;
        uint32_t entry = 0;
        const int st = rk_elf::walk_load_segments(elf, elf_bytes, &entry, err, [&](uint32_t off, uint32_t vaddr, uint32_t filesz, uint32_t) {
            for (uint32_t b = 0; b < filesz; b++) {
                const uint32_t a = vaddr + b, sh = 8 * (a & 3);
                uint32_t& w = image[a >> 2];
                w = (w & ~(0xffu << sh)) | (uint32_t)elf[off + b] << sh;
            }
            return (int)RK_OK;
        });
        if (st != RK_OK) return st;
        *n = image.size();
        if (image.size() > capacity) return RK_ERR_CAPACITY;
        if (!image.empty() && (!out_addr || !out_words)) return RK_ERR_INVALID;
        size_t k = 0;
        for (const auto& kv : image) out_addr[k] = kv.first, out_words[k++] = kv.second;
        return RK_OK;
    } catch (const std::bad_alloc&) {
        return RK_ERR_NOMEM;
    } catch (...) {
        return RK_ERR_INTERNAL;
    }
}

}  // extern "C"
