// What the rv32 shard driver returns for a device error word: shard_verdict of raiko_amd/csrc/rv32_rows.hpp, the one
// place that orders the ShardErr bits, under plain g++.  A program of its own (tests/test_rv32_verdict.py builds it with
// AddressSanitizer and UBSan): every line of standard input is `chip_set bits m_total m_count heads mem_words`, decimal;
// for each it prints `status<TAB>message` (message empty when the status is RK_OK).  The first line it prints names the
// ShardErr values, so the test also pins the bits.
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "rv32_rows.hpp"

using namespace rv32;

template <int CS>
static ShardVerdict verdict_of(int cs, uint32_t bits, uint32_t m_total, size_t m_count, uint32_t heads, size_t mem_words) {
    if (cs == CS) return shard_verdict<CS>(bits, m_total, m_count, heads, mem_words);
    if constexpr (CS < CS_COMMIT) return verdict_of<CS + 1>(cs, bits, m_total, m_count, heads, mem_words);
    return {1, "no such chip set"};
}

int main() {
    std::printf("%u %u %u %u %u %u %u %u %u %u\n", (unsigned)ERR_WORD, (unsigned)ERR_SIDE_LIST, (unsigned)ERR_PC, (unsigned)ERR_M_RESULT,
                (unsigned)ERR_M_COUNT, (unsigned)ERR_ACCESS, (unsigned)ERR_HEADS, (unsigned)ERR_JOURNAL, (unsigned)ERR_IO_LIST,
                (unsigned)ERR_COMMIT_READ);
    int cs;
    unsigned bits, m_total, heads;
    unsigned long m_count, mem_words;
    while (std::scanf("%d %u %u %lu %u %lu", &cs, &bits, &m_total, &m_count, &heads, &mem_words) == 6) {
        const ShardVerdict v = verdict_of<CS_I>(cs, bits, m_total, m_count, heads, mem_words);
        std::printf("%d\t%s\n", v.status, v.message ? v.message : "");
    }
    return 0;
}
