// The ELF32 program-header walk shared by the executor's loader (executor.cpp load_elf) and the program image of the
// rv32im-elf chip set (elf_image.cpp, rk_exec_program_image): one walk, the same file checks for both.  Plain C++: the
// image lister also builds without the GPU toolchain (tests/asan/elf_image_main.cpp runs it under sanitizers).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/raiko_hip.h"

namespace rk_elf {

// the one walk of an ELF's program headers: the file checks, then seg(file offset, vaddr, filesz, flags) for every PT_LOAD
// in program-header order (non-zero from seg ends the walk with that status); *entry = e_entry
template <class F>
int walk_load_segments(const uint8_t* elf, size_t n, uint32_t* entry, std::string& err, F&& seg) {
    auto rd16 = [&](size_t o) { return (uint32_t)elf[o] | (uint32_t)elf[o + 1] << 8; };
    auto rd32 = [&](size_t o) { return rd16(o) | rd16(o + 2) << 16; };
    if (!elf || n < 52 || std::memcmp(elf, "\x7f" "ELF", 4) != 0) { err = "not an ELF file"; return RK_ERR_INVALID; }
    if (elf[4] != 1 || elf[5] != 1) { err = "not a 32-bit little-endian ELF"; return RK_ERR_INVALID; }
    if (rd16(18) != 243) { err = "not a RISC-V ELF (e_machine != 243)"; return RK_ERR_INVALID; }
    *entry = rd32(24);
    uint32_t phoff = rd32(28), phentsize = rd16(42), phnum = rd16(44);
    if (phentsize < 32 || (uint64_t)phoff + (uint64_t)phentsize * phnum > n) { err = "program headers out of range"; return RK_ERR_INVALID; }
    for (uint32_t i = 0; i < phnum; i++) {
        size_t ph = phoff + (size_t)i * phentsize;
        if (rd32(ph) != 1) continue;  // PT_LOAD
        uint32_t off = rd32(ph + 4), vaddr = rd32(ph + 8), filesz = rd32(ph + 16), memsz = rd32(ph + 20), flags = rd32(ph + 24);
        if ((uint64_t)off + filesz > n || filesz > memsz || (uint64_t)vaddr + memsz > 0x100000000ull) {
            err = "PT_LOAD segment out of range";
            return RK_ERR_INVALID;
        }
        const int st = seg(off, vaddr, filesz, flags);
        if (st != RK_OK) return st;
    }
    return RK_OK;
}

}  // namespace rk_elf
