// The lane body of the Keccak-f[1600] chip's rows kernel (kc::keccak_chip_lane, raiko_amd/csrc/keccak_chip.hpp) as a program
// of its own: built by tests/test_keccak_chip.py with -fsanitize=address,undefined from the header alone (plain C++, no GPU
// toolchain).  Five permutations into a 128-row table -- the sixth slot is cut off by the table's end after three rows --,
// every buffer a heap block of exactly its size, lanes 0..63 of every slot in turn.  Checks that every word of the table
// was written (a field element, never the fill value) and that the outputs reported beside the table are the states the
// output rows hold; prints "keccak_chip_main ok" and returns 0.
#include <cstdint>
#include <cstdio>
#include <memory>

#include "keccak_chip.hpp"

int main() {
    using L = kc::KeccakChipLayout;
    const size_t n = 5, rows = 128, slots = (rows + 24) / 25;
    std::unique_ptr<uint64_t[]> states(new uint64_t[n * 25]), out(new uint64_t[n * 25]);
    std::unique_ptr<uint32_t[]> ids(new uint32_t[n]), mult(new uint32_t[n]), trace(new uint32_t[rows * L::WIDTH]);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (size_t i = 0; i < n * 25; i++) {   // splitmix64
        uint64_t z = (x += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        states[i] = z ^ (z >> 31);
    }
    for (size_t i = 0; i < n; i++) ids[i] = bb::encode((uint32_t)(100 + i)), mult[i] = bb::encode((uint32_t)(i % 3));
    for (size_t i = 0; i < rows * L::WIDTH; i++) trace[i] = 0xffffffffu;
    for (size_t i = 0; i < n * 25; i++) out[i] = 0;
    const kc::KeccakChipArgs a{states.get(), ids.get(), mult.get(), n, rows, trace.get(), out.get()};
    for (size_t slot = 0; slot < slots; slot++)
        for (uint32_t lane = 0; lane < 64; lane++) kc::keccak_chip_lane(a, slot, lane);
    size_t bad = 0;
    for (size_t i = 0; i < rows * L::WIDTH; i++) bad += trace[i] >= bb::P;
    for (size_t p = 0; p < n; p++)
        for (uint32_t i = 0; i < 25; i++) {
            uint64_t lane = 0;
            for (uint32_t l = 0; l < 4; l++) lane |= (uint64_t)bb::decode(trace[(25 * p + 24) * L::WIDTH + L::a(4 * i + l)]) << (16 * l);
            bad += lane != out[25 * p + i];
        }
    if (bad) {
        std::printf("FAILED: %zu words unwritten or outputs that differ from the output rows\n", bad);
        return 1;
    }
    std::printf("keccak_chip_main ok\n");
    return 0;
}
