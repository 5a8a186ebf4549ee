// rk_exec_program_image (raiko_amd/csrc/elf_image.cpp) on truncated and hostile ELF headers, as a program of its own:
// built by tests/test_rv32_elf_chips.py with -fsanitize=address,undefined together with elf_image.cpp (plain C++, no GPU
// toolchain), so every read past a header, a segment or an output buffer stops the run.  Every input lives in a heap
// block of exactly its size.  Prints "elf_image_main ok" and returns 0 when every call answered as expected.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/raiko_hip.h"

namespace {

struct Seg {
    uint32_t vaddr, filesz, memsz, flags;
    int64_t off;   // < 0: where the bytes are
};

void put16(std::vector<uint8_t>& b, size_t at, uint32_t v) { b[at] = v & 255, b[at + 1] = (v >> 8) & 255; }
void put32(std::vector<uint8_t>& b, size_t at, uint32_t v) { put16(b, at, v & 0xffff), put16(b, at + 2, v >> 16); }

std::vector<uint8_t> make_elf(const std::vector<Seg>& segs, int phnum = -1) {
    const size_t eh = 52, ph = 32;
    size_t body = eh + ph * segs.size(), total = body;
    for (const Seg& s : segs) total += s.filesz;
    std::vector<uint8_t> b(total, 0);
    std::memcpy(b.data(), "\x7f" "ELF", 4);
    b[4] = 1, b[5] = 1, b[6] = 1;
    put16(b, 16, 2), put16(b, 18, 243), put32(b, 20, 1), put32(b, 24, segs.empty() ? 0x200800u : segs[0].vaddr), put32(b, 28, eh);
    put16(b, 40, eh), put16(b, 42, ph), put16(b, 44, phnum < 0 ? (uint32_t)segs.size() : (uint32_t)phnum);
    for (size_t k = 0; k < segs.size(); k++) {
        const size_t at = eh + ph * k;
        put32(b, at, 1), put32(b, at + 4, segs[k].off < 0 ? (uint32_t)body : (uint32_t)segs[k].off), put32(b, at + 8, segs[k].vaddr);
        put32(b, at + 12, segs[k].vaddr), put32(b, at + 16, segs[k].filesz), put32(b, at + 20, segs[k].memsz), put32(b, at + 24, segs[k].flags);
        for (uint32_t i = 0; i < segs[k].filesz; i++) b[body + i] = (uint8_t)(0x13 + i + 7 * k);
        body += segs[k].filesz;
    }
    return b;
}

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        failures++;
    }
}

// the call on an exact-size heap copy of `elf` with output buffers of exactly the given capacities
int image(const std::vector<uint8_t>& elf, size_t seg_cap, size_t word_cap, size_t* n_segs, size_t* n_words,
          std::vector<uint32_t>* words_out = nullptr, std::vector<uint32_t>* vaddr_out = nullptr) {
    std::unique_ptr<uint8_t[]> copy(new uint8_t[elf.size() ? elf.size() : 1]);
    if (!elf.empty()) std::memcpy(copy.get(), elf.data(), elf.size());
    std::unique_ptr<uint32_t[]> va(new uint32_t[seg_cap ? seg_cap : 1]), sw(new uint32_t[seg_cap ? seg_cap : 1]),
        w(new uint32_t[word_cap ? word_cap : 1]);
    const int st = rk_exec_program_image(copy.get(), elf.size(), seg_cap ? va.get() : nullptr, seg_cap ? sw.get() : nullptr, seg_cap,
                                         n_segs, word_cap ? w.get() : nullptr, word_cap, n_words);
    if (st == RK_OK && words_out) words_out->assign(w.get(), w.get() + *n_words);
    if (st == RK_OK && vaddr_out) vaddr_out->assign(va.get(), va.get() + *n_segs);
    return st;
}

}  // namespace

int main() {
    size_t ns = 0, nw = 0;
    std::vector<uint32_t> words, vaddr;
    const std::vector<Seg> two = {{0x200800, 22, 22, 5, -1}, {0x300000, 8, 64, 7, -1}, {0x400000, 16, 16, 6, -1}};
    const std::vector<uint8_t> good = make_elf(two);
    // a well-formed file: two executable segments (the third is not PF_X), 22 bytes pad to 6 words
    expect(image(good, 16, 64, &ns, &nw, &words, &vaddr) == RK_OK && ns == 2 && nw == 8, "well-formed image");
    expect(vaddr.size() == 2 && vaddr[0] == 0x200800 && vaddr[1] == 0x300000, "segment order");
    expect(words.size() == 8 && words[5] == (0x13u + 20) + ((0x13u + 21) << 8), "zero padding of the last word");
    // output buffers too small, or absent: the sizes are reported, nothing is written
    expect(image(good, 1, 64, &ns, &nw) == RK_ERR_CAPACITY && ns == 2 && nw == 8, "segment capacity");
    expect(image(good, 16, 7, &ns, &nw) == RK_ERR_CAPACITY && ns == 2 && nw == 8, "word capacity");
    expect(image(good, 0, 0, &ns, &nw) == RK_ERR_CAPACITY && ns == 2 && nw == 8, "no buffers");
    expect(rk_exec_program_image(nullptr, 100, nullptr, nullptr, 0, &ns, nullptr, 0, &nw) == RK_ERR_INVALID, "null file");
    expect(rk_exec_program_image(good.data(), good.size(), nullptr, nullptr, 0, nullptr, nullptr, 0, &nw) == RK_ERR_INVALID, "null count");
    // truncated at every length: never a read past the end; only the whole file lists two segments
    for (size_t n = 0; n < good.size(); n++) {
        const std::vector<uint8_t> cut(good.begin(), good.begin() + n);
        const int st = image(cut, 16, 64, &ns, &nw);
        expect(st == RK_ERR_INVALID || (st == RK_OK && n >= 52 + 32 * 3), "truncated file");
    }
    // hostile program headers
    expect(image(make_elf({{0x200800, 8, 4, 5, -1}}), 16, 64, &ns, &nw) == RK_ERR_INVALID, "filesz > memsz");
    expect(image(make_elf({{0x200800, 8, 8, 5, 1 << 20}}), 16, 64, &ns, &nw) == RK_ERR_INVALID, "offset past the end");
    expect(image(make_elf({{0x200800, 8, 8, 5, 0x7ffffff0}}), 16, 64, &ns, &nw) == RK_ERR_INVALID, "offset near 2^31");
    expect(image(make_elf({{0x200800, 8, 8, 5, (int64_t)0xfffffffc}}), 16, 64, &ns, &nw) == RK_ERR_INVALID, "offset + filesz wraps 32 bits");
    expect(image(make_elf({{0xfffffffc, 8, 8, 5, -1}}), 16, 64, &ns, &nw) == RK_ERR_INVALID, "vaddr + memsz past 2^32");
    expect(image(make_elf({{0x200802, 8, 8, 5, -1}}), 16, 64, &ns, &nw) == RK_ERR_INVALID, "misaligned executable segment");
    expect(image(make_elf({{0x200800, 16, 16, 5, -1}, {0x200808, 16, 16, 5, -1}}), 16, 64, &ns, &nw) == RK_ERR_INVALID, "overlap");
    expect(image(make_elf({{0x200800, 5, 5, 5, -1}, {0x200804, 4, 4, 5, -1}}), 16, 64, &ns, &nw) == RK_ERR_INVALID, "overlap by padding");
    expect(image(make_elf(two, 0), 16, 64, &ns, &nw) == RK_OK && ns == 0 && nw == 0, "phnum 0");
    expect(image(make_elf(two, 40), 16, 64, &ns, &nw) == RK_ERR_INVALID, "phnum past the file");
    std::vector<Seg> many;
    for (uint32_t k = 0; k < 17; k++) many.push_back({0x200800 + 64 * k, 4, 4, 5, -1});
    expect(image(make_elf(many), 32, 64, &ns, &nw) == RK_ERR_CAPACITY, "17 executable segments");
    many.pop_back();
    expect(image(make_elf(many), 16, 16, &ns, &nw) == RK_OK && ns == 16 && nw == 16, "16 executable segments");
    {
        std::vector<uint8_t> b = good;
        put16(b, 42, 16);   // phentsize below a program header
        expect(image(b, 16, 64, &ns, &nw) == RK_ERR_INVALID, "phentsize 16");
        b = good;
        put32(b, 28, 0xfffffff0u);   // phoff
        expect(image(b, 16, 64, &ns, &nw) == RK_ERR_INVALID, "phoff past the end");
        b = good;
        put16(b, 42, 0xffff), put16(b, 44, 0xffff);
        expect(image(b, 16, 64, &ns, &nw) == RK_ERR_INVALID, "phentsize * phnum large");
    }
    // byte mutations of the ELF and program headers: any status, no bad access
    uint32_t lcg = 12345;
    for (int it = 0; it < 4000; it++) {
        std::vector<uint8_t> b = good;
        for (int k = 0; k < 1 + it % 3; k++) {
            lcg = lcg * 1664525u + 1013904223u;
            const size_t at = (lcg >> 8) % (52 + 32 * 3);
            lcg = lcg * 1664525u + 1013904223u;
            b[at] = (uint8_t)(lcg >> 16);
        }
        const int st = image(b, 16, 64, &ns, &nw);
        expect(st == RK_OK || st == RK_ERR_INVALID || st == RK_ERR_CAPACITY, "mutated header status");
        expect(st != RK_OK || (ns <= 16 && nw <= 64), "mutated header sizes");
    }
    if (failures) return 1;
    std::printf("elf_image_main ok\n");
    return 0;
}
