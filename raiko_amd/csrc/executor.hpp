// What the executor (executor.cpp) records of a segment, as the witness generators read it (rv32_shards.hip, and
// rk_exec_witness / rk_exec_lookup_tables in executor.cpp itself).  The executor's own state stays private to it.
#pragma once
#include <array>
#include <cstdint>
#include <vector>

#include "../../include/raiko_hip.h"

// one executed cycle as the witness generator needs it
struct TraceRow {
    uint32_t pc, ins, a, b, res, next, wr;
};

// read-only view of one segment recorded with rk_exec_opts.record_trace; valid while the rk_exec lives
struct ExecSegmentView {
    const rk_exec_segment* seg;
    const std::vector<TraceRow>* trace;                   // seg->cycles rows
    const uint32_t* regs;                                 // x0..x31 at the segment's start, then at its end
    const std::vector<std::array<uint32_t, 2>>* ecalls;   // (cycle, a0 after the call) of every ecall row, in cycle order
    uint32_t pc_lo, pc_hi;                                // the lowest / highest pc executed
    // (cycle, word address addr >> 2, old word, new word) of every store, every load whose rd is not x0 (new = old) and
    // every word an ecall READ writes, in cycle order (the words of one ecall in ascending address order)
    const std::vector<std::array<uint32_t, 4>>* mem;
    // (cycle, t0, a0 before the call, a1, input position before it) of every ecall row, in cycle order
    const std::vector<std::array<uint32_t, 5>>* ecall_args;
    uint32_t in_start;                                    // the input position at the segment's start
    size_t n_input;                                       // the run's input words
    // (cycle, word address, word, word) of every word an ecall COMMIT reads, in cycle order and per call in ascending
    // address order from a0 & ~3: a list of its own -- `mem` holds none of them (the commit form merges the two)
    const std::vector<std::array<uint32_t, 4>>* commit_reads;
    uint32_t jpos_start;                                  // the journal's length at the segment's start
};

// RK_ERR_INVALID: no executor, or no recorded segment `index`; RK_ERR_INTERNAL: the trace is not seg->cycles rows long.
// Not part of the library's ABI.
__attribute__((visibility("hidden"))) int exec_segment_view(const rk_exec* ex, uint32_t index, ExecSegmentView* out);
// the distinct word addresses in the access list of recorded segment `index` (the rows of the rv32im-mem memory table):
// counted by a sort on the first call, remembered for the next
__attribute__((visibility("hidden"))) size_t exec_mem_words(const rk_exec* ex, uint32_t index);
