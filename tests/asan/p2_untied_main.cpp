// The host branches of p2::madk / mulk / smadk / smulk (raiko_amd/csrc/poseidon2_core.hpp) through Core::permute, as a
// program of its own: built by tests/test_p2_untied_host.py with -fsanitize=address,undefined from the header alone
// (plain C++, no GPU toolchain).  The helpers share their signature with the device forms, whose addend is an input
// operand of its own; here the same calls must still return acc + x * K.
//
// argv[1]: a text file of unsigned integers (Montgomery form):
//   W M4 NCASES, then rc_ext (8 W), rc_int (R_P), diag (W), then per case W input cells and W expected output cells.
// Every table and every state lives in a heap block of exactly its size.  Prints "p2_untied_main ok" and returns 0 when
// every output word is the expected one.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "poseidon2_core.hpp"

namespace {

bool read_words(std::FILE* f, uint32_t* out, size_t n) {
    for (size_t i = 0; i < n; i++) {
        unsigned long long v;
        if (std::fscanf(f, "%llu", &v) != 1 || v >= bb::P) return false;
        out[i] = (uint32_t)v;
    }
    return true;
}

template <class C>
int run(std::FILE* f, unsigned ncases) {
    std::unique_ptr<typename C::Consts> k(new typename C::Consts);
    std::memset(k.get(), 0, sizeof(typename C::Consts));
    if (!read_words(f, k->rc_ext, 2 * p2::ROUNDS_HALF_FULL * C::CELLS) || !read_words(f, k->rc_int, C::ROUNDS_PARTIAL) ||
        !read_words(f, k->diag, C::CELLS)) {
        std::printf("FAILED: tables\n");
        return 1;
    }
    C::derive(*k);
    int bad = 0;
    for (unsigned c = 0; c < ncases; c++) {
        std::unique_ptr<uint32_t[]> s(new uint32_t[C::CELLS]), want(new uint32_t[C::CELLS]);
        if (!read_words(f, s.get(), C::CELLS) || !read_words(f, want.get(), C::CELLS)) {
            std::printf("FAILED: case %u is short\n", c);
            return 1;
        }
        C::permute(s.get(), *k);
        for (int i = 0; i < C::CELLS; i++)
            if (s[i] != want[i]) {
                std::printf("FAILED: width %d m4 %d case %u cell %d: got %u, want %u\n", C::CELLS, C::M4_KIND, c, i, s[i], want[i]);
                bad++;
            }
    }
    std::printf("width %d m4 %d: %u cases, %d wrong words\n", C::CELLS, C::M4_KIND, ncases, bad);
    return bad != 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    unsigned w = 0, m4 = 0, ncases = 0;
    int st = 2, instances = 0;
    while (std::fscanf(f, "%u %u %u", &w, &m4, &ncases) == 3) {
        // risc0's and SP1's instances (the other two differ in the 4x4 block only and cost as much again to compile)
        if (w == 24 && m4 == 0) st = run<p2::Core<24, 21, 0>>(f, ncases);
        else if (w == 16 && m4 == 1) st = run<p2::Core<16, 13, 1>>(f, ncases);
        else st = 2;
        if (st != 0) break;
        instances++;
    }
    std::fclose(f);
    if (st == 0 && instances > 0) std::printf("p2_untied_main ok: %d instances\n", instances);
    return st;
}
