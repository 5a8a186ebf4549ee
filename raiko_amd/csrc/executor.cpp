// RV32IM executor + segmenter: the step BEFORE the proving path --
// `ExecutorImpl::from_elf(env, elf).run()` at reference provers/risc0/driver/src/bonsai.rs:267-269,
// which interprets the guest and cuts the run into segments of at most 2^segment_limit_po2 cycles
// (bonsai.rs:249) that `session.prove()` (bonsai.rs:271) then proves one by one.
//
// Host code only (the reference's executor is CPU code too, single-threaded): the machine, the ELF loader, the
// segmenter and the host-side witness of the stand-in trace circuit.  The witness written on the GPU -- the same columns
// and the tables of the rv32 chip sets -- is rv32_shards.hip, which reads a recorded segment through executor.hpp.  What is
// restated is the public part: the RV32IM instruction set (RISC-V unprivileged spec 2.2: RV32I +
// M), a little-endian paged memory, an ELF32 loader, and the cut into power-of-two segments.
// What is NOT risc0's (its executor lives in risc0-zkvm / risc0-circuit-rv32im 1.0.1, outside the
// reference tree): the cycle model (one cycle per instruction here; risc0 charges paging and
// multi-cycle ecalls), the ecall table (a three-call stand-in: halt / read input words / commit to
// the journal) and the state digest.  The witness layout of the rv32im circuit is not available
// either, so a segment here carries its bounds and state digests, not trace columns.
#include <algorithm>
#include <array>
#include <cstring>
#include <map>
#include <thread>
#include <memory>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/raiko_hip.h"
#include "elf_image.hpp"
#include "executor.hpp"
#include "internal.hpp"
#include "rv32_rows.hpp"

namespace {

constexpr uint32_t PAGE_WORDS = 1024;  // 4 KiB pages
constexpr uint32_t MIN_PO2 = 13;       // risc0's MIN_CYCLES_PO2 (RECALLED): the smallest segment it proves

struct Machine {
    uint32_t pc = 0;
    uint32_t x[32] = {0};
    std::map<uint32_t, std::vector<uint32_t>> pages;  // page index -> 1024 words (ordered: digests walk it)
    // the last page touched by an instruction fetch and by a data access: the map is searched only when an
    // access leaves them (map nodes and the vectors inside them never move once created)
    uint32_t fetch_idx = 0xffffffffu, data_idx = 0xffffffffu;
    uint32_t* fetch_page = nullptr;
    uint32_t* data_page = nullptr;

    uint32_t* page_for_write(uint32_t idx) {
        if (idx == data_idx && data_page) return data_page;
        auto& pg = pages[idx];
        if (pg.empty()) {
            pg.assign(PAGE_WORDS, 0);
            if (idx == fetch_idx) fetch_page = pg.data();  // a page first seen absent by the fetch path now exists
        }
        data_idx = idx;
        data_page = pg.data();
        return data_page;
    }
    uint32_t* word_ptr(uint32_t addr) { return page_for_write(addr >> 12) + ((addr >> 2) & (PAGE_WORDS - 1)); }
    uint32_t load_word(uint32_t addr) {
        const uint32_t idx = addr >> 12;
        if (idx == data_idx && data_page) return data_page[(addr >> 2) & (PAGE_WORDS - 1)];
        auto it = pages.find(idx);
        if (it == pages.end()) return 0u;
        data_idx = idx;
        data_page = it->second.data();
        return data_page[(addr >> 2) & (PAGE_WORDS - 1)];
    }
    uint32_t fetch(uint32_t addr) {
        const uint32_t idx = addr >> 12;
        if (idx != fetch_idx) {
            auto it = pages.find(idx);
            fetch_idx = idx;
            fetch_page = it == pages.end() ? nullptr : it->second.data();
        }
        return fetch_page ? fetch_page[(addr >> 2) & (PAGE_WORDS - 1)] : 0u;
    }
    uint8_t load_byte(uint32_t addr) { return (uint8_t)(load_word(addr & ~3u) >> (8 * (addr & 3))); }
    void store_byte(uint32_t addr, uint8_t v) {
        uint32_t* w = word_ptr(addr & ~3u);
        unsigned sh = 8 * (addr & 3);
        *w = (*w & ~(0xffu << sh)) | ((uint32_t)v << sh);
    }
};

// digest of the machine state: Poseidon2 sponge (the default instance) over pc, the registers and
// every touched page (index, then its words), each 32-bit word as two 16-bit field elements so the
// encoding is injective.  Stands where risc0's SystemState { pc, merkle_root } stands.
void state_digest(const p2::Any& k, const Machine& m, uint32_t* out8) {
    std::vector<uint32_t> e;
    auto put = [&](uint32_t w) {
        e.push_back(bb::encode(w & 0xffffu));
        e.push_back(bb::encode(w >> 16));
    };
    put(m.pc);
    for (int i = 0; i < 32; i++) put(m.x[i]);
    for (const auto& kv : m.pages) {
        bool any = false;
        for (uint32_t w : kv.second) any |= w != 0;
        if (!any) continue;  // an all-zero page is the same as an absent one
        put(kv.first);
        for (uint32_t w : kv.second) put(w);
    }
    k.hash_elems(e.data(), e.size(), out8);
}

}  // namespace

struct rk_exec {
    std::vector<rk_exec_segment> segments;
    std::vector<std::vector<TraceRow>> traces;   // per segment, when rk_exec_opts.record_trace is set
    std::vector<std::array<uint32_t, 64>> regs;  // per segment: x0..x31 at its start, then at its end
    // per segment, with record_trace: (cycle, a0 after the call) of every ecall row -- an ecall READ writes a0 outside
    // TraceRow -- and the lowest / highest pc executed (the rv32i chip set's program table, rk_exec_rv32_*)
    std::vector<std::vector<std::array<uint32_t, 2>>> ecalls;
    std::vector<std::array<uint32_t, 2>> pc_range;
    // per segment, with record_trace: (cycle, t0, a0 before the call, a1, input position before it) of every ecall row --
    // what the call read, beside what it left (rk_exec_ecall_args; the io form of the rv32im-mem chip set)
    std::vector<std::vector<std::array<uint32_t, 5>>> ecall_args;
    std::vector<uint32_t> in_start;              // per segment, with record_trace: the input position at its start
    // per segment, with record_trace: (cycle, word address, old word, new word) of every data access the rv32im-mem chip
    // set proves (ExecSegmentView.mem); `mem_now` collects the running segment's, `cycle_now` is its cycle counter
    std::vector<std::vector<std::array<uint32_t, 4>>> mem;
    std::vector<std::array<uint32_t, 4>> mem_now;
    uint32_t cycle_now = 0;
    // per segment, with record_trace: (cycle, word address, word, word) of every word an ecall COMMIT reads, in cycle
    // order and per call in ascending address order (rk_exec_commit_reads; the commit form of the rv32im-mem chip set):
    // a list beside `mem`, which stays what it is; `jpos_start` the journal's length at the segment's start
    std::vector<std::vector<std::array<uint32_t, 4>>> commit_reads;
    std::vector<std::array<uint32_t, 4>> commit_now;
    std::vector<uint32_t> jpos_start;
    mutable std::vector<size_t> mem_words;       // per segment: exec_mem_words's answer, SIZE_MAX until asked
    // the machine between segments (rk_exec_open / rk_exec_next_segment run it one segment at a time)
    Machine m;
    std::unique_ptr<p2::Any> k;                  // the default Poseidon2 instance: state digests at the boundaries
    rk_exec_opts o{};
    std::vector<uint32_t> input;                 // copy of the caller's input words
    size_t in_pos = 0;
    uint64_t total = 0;
    bool halted = false;
    int st = RK_OK;
    std::vector<uint8_t> journal;
    std::unordered_map<uint32_t, uint64_t> pc_cycles;   // rk_exec_opts.profile
    rk_exec_summary summary{};
    std::string error;
};

namespace {

int load_elf(Machine& m, const uint8_t* elf, size_t n, std::string& err) {
    RK_TRY(rk_elf::walk_load_segments(elf, n, &m.pc, err, [&](uint32_t off, uint32_t vaddr, uint32_t filesz, uint32_t) {
        for (uint32_t b = 0; b < filesz; b++) m.store_byte(vaddr + b, elf[off + b]);
        return (int)RK_OK;
    }));
    if (m.pc & 3) { err = "misaligned entry point"; return RK_ERR_INVALID; }
    return RK_OK;
}

inline int32_t sext(uint32_t v, unsigned bits) { return (int32_t)(v << (32 - bits)) >> (32 - bits); }

// one instruction; returns 0 to go on, 1 halted, negative rk_status on a trap
int step(Machine& m, rk_exec& ex, const rk_exec_opts& o, size_t& in_pos, std::string& err, TraceRow* row) {
    const uint32_t pc = m.pc, ins = m.fetch(pc);
    const uint32_t opc = ins & 0x7f, rd = (ins >> 7) & 31, f3 = (ins >> 12) & 7, rs1 = (ins >> 15) & 31, rs2 = (ins >> 20) & 31,
                   f7 = ins >> 25;
    const uint32_t a = m.x[rs1], b = m.x[rs2];
    uint32_t next = pc + 4, res = 0;
    bool wr = false;
    auto trap = [&](const char* what) {
        char buf[96];
        std::snprintf(buf, sizeof buf, "%s at pc 0x%08x (instruction 0x%08x)", what, pc, ins);
        err = buf;
        return RK_ERR_INVALID;
    };
    switch (opc) {
        case 0x37: res = ins & 0xfffff000u; wr = true; break;                       // LUI
        case 0x17: res = pc + (ins & 0xfffff000u); wr = true; break;                // AUIPC
        case 0x6f: {                                                                 // JAL
            uint32_t imm = ((ins >> 31) << 20) | (((ins >> 12) & 0xff) << 12) | (((ins >> 20) & 1) << 11) | (((ins >> 21) & 0x3ff) << 1);
            res = pc + 4; wr = true; next = pc + (uint32_t)sext(imm, 21);
            break;
        }
        case 0x67:                                                                   // JALR
            if (f3 != 0) return trap("illegal instruction");
            res = pc + 4; wr = true; next = (a + (uint32_t)sext(ins >> 20, 12)) & ~1u;
            break;
        case 0x63: {                                                                 // branches
            uint32_t imm = ((ins >> 31) << 12) | (((ins >> 7) & 1) << 11) | (((ins >> 25) & 0x3f) << 5) | (((ins >> 8) & 0xf) << 1);
            bool t;
            switch (f3) {
                case 0: t = a == b; break;
                case 1: t = a != b; break;
                case 4: t = (int32_t)a < (int32_t)b; break;
                case 5: t = (int32_t)a >= (int32_t)b; break;
                case 6: t = a < b; break;
                case 7: t = a >= b; break;
                default: return trap("illegal instruction");
            }
            if (t) next = pc + (uint32_t)sext(imm, 13);
            break;
        }
        case 0x03: {                                                                 // loads
            uint32_t addr = a + (uint32_t)sext(ins >> 20, 12);
            const uint32_t seen = row && rd != 0 ? m.load_word(addr & ~3u) : 0u;   // the word as the access finds it
            switch (f3) {
                case 0: res = (uint32_t)(int32_t)(int8_t)m.load_byte(addr); break;
                case 4: res = m.load_byte(addr); break;
                case 1: case 5: {
                    if (addr & 1) return trap("misaligned halfword load");
                    uint32_t h = m.load_byte(addr) | (uint32_t)m.load_byte(addr + 1) << 8;
                    res = f3 == 1 ? (uint32_t)sext(h, 16) : h;
                    break;
                }
                case 2:
                    if (addr & 3) return trap("misaligned word load");
                    res = m.load_word(addr);
                    break;
                default: return trap("illegal instruction");
            }
            if (row && rd != 0) ex.mem_now.push_back({ex.cycle_now, addr >> 2, seen, seen});
            wr = true;
            break;
        }
        case 0x23: {                                                                 // stores
            uint32_t addr = a + (uint32_t)sext(((ins >> 25) << 5) | ((ins >> 7) & 31), 12);
            const uint32_t seen = row ? m.load_word(addr & ~3u) : 0u;
            switch (f3) {
                case 0: m.store_byte(addr, (uint8_t)b); break;
                case 1:
                    if (addr & 1) return trap("misaligned halfword store");
                    m.store_byte(addr, (uint8_t)b); m.store_byte(addr + 1, (uint8_t)(b >> 8));
                    break;
                case 2:
                    if (addr & 3) return trap("misaligned word store");
                    *m.word_ptr(addr) = b;
                    break;
                default: return trap("illegal instruction");
            }
            if (row) ex.mem_now.push_back({ex.cycle_now, addr >> 2, seen, m.load_word(addr & ~3u)});
            break;
        }
        case 0x13: {                                                                 // OP-IMM
            uint32_t imm = (uint32_t)sext(ins >> 20, 12), sh = rs2;
            switch (f3) {
                case 0: res = a + imm; break;
                case 2: res = (int32_t)a < (int32_t)imm; break;
                case 3: res = a < imm; break;
                case 4: res = a ^ imm; break;
                case 6: res = a | imm; break;
                case 7: res = a & imm; break;
                case 1: if (f7 != 0) return trap("illegal instruction"); res = a << sh; break;
                case 5:
                    if (f7 == 0) res = a >> sh;
                    else if (f7 == 0x20) res = (uint32_t)((int32_t)a >> sh);
                    else return trap("illegal instruction");
                    break;
            }
            wr = true;
            break;
        }
        case 0x33: {                                                                 // OP (RV32I + M)
            if (f7 == 1) {
                const int64_t sa = (int32_t)a, sb = (int32_t)b;
                switch (f3) {
                    case 0: res = a * b; break;                                                   // MUL
                    case 1: res = (uint32_t)((uint64_t)(sa * sb) >> 32); break;                   // MULH
                    case 2: res = (uint32_t)((uint64_t)(sa * (int64_t)(uint64_t)b) >> 32); break; // MULHSU
                    case 3: res = (uint32_t)(((uint64_t)a * b) >> 32); break;                     // MULHU
                    case 4: res = b == 0 ? 0xffffffffu : (a == 0x80000000u && b == 0xffffffffu) ? a : (uint32_t)((int32_t)a / (int32_t)b); break;
                    case 5: res = b == 0 ? 0xffffffffu : a / b; break;
                    case 6: res = b == 0 ? a : (a == 0x80000000u && b == 0xffffffffu) ? 0 : (uint32_t)((int32_t)a % (int32_t)b); break;
                    case 7: res = b == 0 ? a : a % b; break;
                }
            } else if (f7 == 0 || f7 == 0x20) {
                const bool alt = f7 == 0x20;
                switch (f3) {
                    case 0: res = alt ? a - b : a + b; break;
                    case 5: res = alt ? (uint32_t)((int32_t)a >> (b & 31)) : a >> (b & 31); break;
                    default:
                        if (alt) return trap("illegal instruction");
                        switch (f3) {
                            case 1: res = a << (b & 31); break;
                            case 2: res = (int32_t)a < (int32_t)b; break;
                            case 3: res = a < b; break;
                            case 4: res = a ^ b; break;
                            case 6: res = a | b; break;
                            case 7: res = a & b; break;
                        }
                }
            } else {
                return trap("illegal instruction");
            }
            wr = true;
            break;
        }
        case 0x0f: break;                                                            // FENCE: no-op
        case 0x73: {                                                                 // SYSTEM
            if (ins != 0x00000073u) return trap(ins == 0x00100073u ? "ebreak" : "illegal instruction");
            // the stand-in ecall table: t0 selects the call
            switch (m.x[5]) {
                case RK_ECALL_HALT:
                    ex.summary.exit_code = m.x[10];
                    if (row) *row = TraceRow{pc, ins, a, b, 0u, next, 0u};
                    m.pc = next;
                    return 1;
                case RK_ECALL_READ: {  // a0 = destination (word aligned), a1 = capacity in words -> a0 = words read
                    uint32_t dst = m.x[10], cap = m.x[11], got = 0;
                    if (dst & 3) return trap("misaligned read destination");
                    while (got < cap && in_pos < o.n_input_words) {
                        uint32_t* w = m.word_ptr(dst + 4 * got);
                        if (row) ex.mem_now.push_back({ex.cycle_now, (dst + 4 * got) >> 2, *w, o.input_words[in_pos]});
                        *w = o.input_words[in_pos++];
                        got++;
                    }
                    m.x[10] = got;
                    break;
                }
                case RK_ECALL_COMMIT: {  // a0 = source, a1 = bytes: appended to the journal
                    uint32_t src = m.x[10], len = m.x[11];
                    if (ex.journal.size() + (size_t)len > ((size_t)1 << 24)) return trap("journal larger than 16 MiB");
                    for (uint32_t i = 0; i < len; i++) ex.journal.push_back(m.load_byte(src + i));
                    if (row && len) {
                        const uint32_t n_words = ((src & 3u) + len + 3u) >> 2;
                        for (uint32_t k = 0; k < n_words; k++) {
                            const uint32_t ad = (src & ~3u) + 4 * k, w = m.load_word(ad);
                            ex.commit_now.push_back({ex.cycle_now, ad >> 2, w, w});
                        }
                    }
                    break;
                }
                default: return trap("unknown ecall");
            }
            break;
        }
        default: return trap("illegal instruction");
    }
    if (wr && rd != 0) m.x[rd] = res;
    if (next & 3) return trap("misaligned jump target");
    if (row) *row = TraceRow{pc, ins, a, b, (wr && rd != 0) ? res : 0u, next, (wr && rd != 0) ? 1u : 0u};
    m.pc = next;
    return 0;
}

void refresh_summary(rk_exec* ex) {
    ex->summary.total_cycles = ex->total;
    ex->summary.n_segments = (uint32_t)ex->segments.size();
    ex->summary.journal_bytes = ex->journal.size();
    ex->summary.input_words_read = ex->in_pos;
    ex->summary.status = ex->st;
}

int exec_open(const uint8_t* elf, size_t elf_bytes, const rk_exec_opts* o, rk_exec** out) {
    if (!out) return RK_ERR_INVALID;
    *out = nullptr;
    if (!elf || !o || o->struct_size != sizeof(rk_exec_opts)) return RK_ERR_INVALID;
    if (o->segment_limit_po2 < MIN_PO2 || o->segment_limit_po2 > 24) return RK_ERR_INVALID;
    if (o->n_input_words && !o->input_words) return RK_ERR_INVALID;
    auto ex = std::make_unique<rk_exec>();
    ex->o = *o;
    if (o->n_input_words) ex->input.assign(o->input_words, o->input_words + o->n_input_words);
    ex->o.input_words = ex->input.data();
    ex->st = load_elf(ex->m, elf, elf_bytes, ex->error);
    rk::Sys sys;
    ex->k = std::make_unique<p2::Any>();
    rk_params def;
    rk::params_preset(&def, RK_PRESET_RISC0);
    if (ex->st == RK_OK) ex->st = rk::resolve_params(&def, &sys, ex->k.get());
    refresh_summary(ex.get());
    const int st = ex->st;
    *out = ex.release();  // also on failure: the caller reads the error text, then frees
    return st;
}

// one more segment; *more = 0 once the guest has halted (or the run has failed)
int exec_next(rk_exec* ex, int* more) {
    if (more) *more = 0;
    if (ex->st != RK_OK || ex->halted) return ex->st;
    Machine& m = ex->m;
    const rk_exec_opts& o = ex->o;
    const uint64_t limit = (uint64_t)1 << o.segment_limit_po2;
    rk_exec_segment seg{};
    seg.index = (uint32_t)ex->segments.size();
    seg.start_pc = m.pc;
    state_digest(*ex->k, m, seg.pre_state);
    uint64_t cycles = 0;
    std::vector<TraceRow> trace;
    std::array<uint32_t, 64> regs{};
    std::copy(m.x, m.x + 32, regs.begin());
    std::vector<std::array<uint32_t, 2>> ecalls;
    std::vector<std::array<uint32_t, 5>> ecall_args;
    const uint32_t in_start = (uint32_t)ex->in_pos, jpos_start = (uint32_t)ex->journal.size();
    uint32_t pc_lo = 0xffffffffu, pc_hi = 0;
    ex->mem_now.clear();
    ex->commit_now.clear();
    if (o.record_trace) trace.reserve((size_t)std::min<uint64_t>(limit, (uint64_t)1 << 22));  // 28 bytes per cycle, no regrowth copies
    while (cycles < limit) {
        if (o.session_limit && ex->total >= o.session_limit) {
            ex->error = "session limit reached";
            ex->st = RK_ERR_CAPACITY;
            break;
        }
        TraceRow row{};
        ex->cycle_now = (uint32_t)cycles;
        if (o.profile) ex->pc_cycles[m.pc]++;
        const std::array<uint32_t, 5> before{(uint32_t)cycles, m.x[5], m.x[10], m.x[11], (uint32_t)ex->in_pos};
        int r = step(m, *ex, o, ex->in_pos, ex->error, o.record_trace ? &row : nullptr);
        if (r < 0) { ex->st = r; break; }
        if (o.record_trace) {
            trace.push_back(row);
            if (row.ins == 0x00000073u) {
                ecalls.push_back({(uint32_t)cycles, m.x[10]});
                ecall_args.push_back(before);
            }
            pc_lo = std::min(pc_lo, row.pc);
            pc_hi = std::max(pc_hi, row.pc);
        }
        cycles++;
        ex->total++;
        if (r == 1) { ex->halted = true; break; }
    }
    if (ex->st == RK_OK) {
        seg.cycles = cycles;
        uint32_t po2 = MIN_PO2;
        while (((uint64_t)1 << po2) < cycles) po2++;
        seg.po2 = po2;
        seg.end_pc = m.pc;
        seg.exit = ex->halted ? RK_EXIT_HALTED : RK_EXIT_SYSTEM_SPLIT;
        state_digest(*ex->k, m, seg.post_state);
        ex->segments.push_back(seg);
        std::copy(m.x, m.x + 32, regs.begin() + 32);
        ex->regs.push_back(regs);
        if (o.record_trace) {
            ex->traces.push_back(std::move(trace));
            ex->ecalls.push_back(std::move(ecalls));
            ex->ecall_args.push_back(std::move(ecall_args));
            ex->in_start.push_back(in_start);
            ex->pc_range.push_back({pc_lo, pc_hi});
            ex->mem.push_back(std::move(ex->mem_now));
            ex->mem_now.clear();
            ex->commit_reads.push_back(std::move(ex->commit_now));
            ex->commit_now.clear();
            ex->jpos_start.push_back(jpos_start);
        }
        if (ex->segments.size() > (1u << 20)) { ex->error = "more than 2^20 segments"; ex->st = RK_ERR_CAPACITY; }
    }
    refresh_summary(ex);
    if (more) *more = (ex->st == RK_OK && !ex->halted) ? 1 : 0;
    return ex->st;
}

int exec_elf(const uint8_t* elf, size_t elf_bytes, const rk_exec_opts* o, rk_exec** out) {
    int st = exec_open(elf, elf_bytes, o, out);
    if (st != RK_OK) return st;
    int more = 1;
    while (more) st = exec_next(*out, &more);
    return st;
}

}  // namespace

// Not safe for two threads on one executor: the answer is kept in a mutable vector.  Its callers (rk_exec_rv32mem_sizes,
// rk_exec_rv32mem_shard_device) run on the thread that steps the executor, as every rk_exec_* call on one handle must.
size_t exec_mem_words(const rk_exec* ex, uint32_t index) {
    if (!ex || index >= ex->mem.size()) return 0;
    if (ex->mem_words.size() < ex->mem.size()) ex->mem_words.resize(ex->mem.size(), SIZE_MAX);
    if (ex->mem_words[index] == SIZE_MAX) {
        std::vector<uint32_t> a;
        a.reserve(ex->mem[index].size());
        for (const auto& m : ex->mem[index]) a.push_back(m[1]);
        std::sort(a.begin(), a.end());
        ex->mem_words[index] = (size_t)(std::unique(a.begin(), a.end()) - a.begin());
    }
    return ex->mem_words[index];
}

int exec_segment_view(const rk_exec* ex, uint32_t index, ExecSegmentView* out) {
    if (!ex || index >= ex->segments.size() || index >= ex->traces.size()) return RK_ERR_INVALID;
    if (ex->traces[index].size() != ex->segments[index].cycles) return RK_ERR_INTERNAL;
    *out = ExecSegmentView{&ex->segments[index], &ex->traces[index], ex->regs[index].data(), &ex->ecalls[index],
                           ex->pc_range[index][0], ex->pc_range[index][1], &ex->mem[index], &ex->ecall_args[index], ex->in_start[index],
                           (size_t)ex->o.n_input_words, &ex->commit_reads[index], ex->jpos_start[index]};
    return RK_OK;
}

extern "C" {

int rk_exec_elf(const uint8_t* elf, size_t elf_bytes, const rk_exec_opts* opts, rk_exec** out) {
    RK_GUARD_BEGIN
    return exec_elf(elf, elf_bytes, opts, out);
    RK_GUARD_END
}
int rk_exec_open(const uint8_t* elf, size_t elf_bytes, const rk_exec_opts* opts, rk_exec** out) {
    RK_GUARD_BEGIN
    return exec_open(elf, elf_bytes, opts, out);
    RK_GUARD_END
}
int rk_exec_next_segment(rk_exec* ex, int* more) {
    RK_GUARD_BEGIN
    if (!ex) return RK_ERR_INVALID;
    return exec_next(ex, more);
    RK_GUARD_END
}
int rk_exec_summary_get(const rk_exec* ex, rk_exec_summary* out) {
    if (!ex || !out) return RK_ERR_INVALID;
    *out = ex->summary;
    return RK_OK;
}
int rk_exec_segment_get(const rk_exec* ex, uint32_t index, rk_exec_segment* out) {
    if (!ex || !out || index >= ex->segments.size()) return RK_ERR_INVALID;
    *out = ex->segments[index];
    return RK_OK;
}
int rk_exec_profile(const rk_exec* ex, uint32_t* pcs, uint64_t* cycles, size_t capacity, size_t* n) {
    RK_GUARD_BEGIN
    if (!ex || !n) return RK_ERR_INVALID;
    *n = ex->pc_cycles.size();
    if (*n > capacity || (*n && (!pcs || !cycles))) return RK_ERR_CAPACITY;
    std::vector<std::pair<uint64_t, uint32_t>> v;
    v.reserve(*n);
    for (const auto& kv : ex->pc_cycles) v.push_back({kv.second, kv.first});
    std::sort(v.begin(), v.end(), [](const auto& a, const auto& b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
    for (size_t i = 0; i < v.size(); i++) {
        pcs[i] = v[i].second;
        cycles[i] = v[i].first;
    }
    return RK_OK;
    RK_GUARD_END
}
int rk_exec_journal(const rk_exec* ex, uint8_t* out, size_t capacity, size_t* len) {
    if (!ex || !len) return RK_ERR_INVALID;
    *len = ex->journal.size();
    if (ex->journal.size() > capacity || (!out && !ex->journal.empty())) return RK_ERR_CAPACITY;
    if (!ex->journal.empty()) std::memcpy(out, ex->journal.data(), ex->journal.size());
    return RK_OK;
}
// Witness of one executed segment for the stand-in trace circuit (include/raiko_hip.h): every 32-bit word as two
// 16-bit field elements; rows beyond the executed cycles repeat the final pc with active = seq = 0.
int rk_exec_witness(const rk_exec* ex, uint32_t index, uint32_t* code, uint32_t* data) {
    RK_GUARD_BEGIN
    if (!code || !data) return RK_ERR_INVALID;
    ExecSegmentView v;
    RK_TRY(exec_segment_view(ex, index, &v));
    const std::vector<TraceRow>& tr = *v.trace;
    const size_t n = (size_t)1 << v.seg->po2;
    if (tr.size() > n) return RK_ERR_INTERNAL;
    // every cell is below 2^16 (or a bit): one Montgomery product each; rows are independent, four threads split them
    auto put = [&](uint32_t* base, unsigned col, size_t i, uint32_t canon) { base[(size_t)col * n + i] = rv32::enc(canon); };
    auto fill = [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            put(code, 0, i, i == 0 ? 1u : 0u);         // first row
            put(code, 1, i, i + 1 == n ? 1u : 0u);     // last row
            const bool active = i < tr.size();
            uint32_t c[RK_TRACE_DATA_COLS];
            rv32::trace_cells(active ? tr[i] : rv32::padding_row(v.seg->end_pc), active, c);
            for (unsigned col = 0; col < RK_TRACE_DATA_COLS; col++) put(data, col, i, c[col]);
        }
    };
    const size_t n_threads = n >= (1u << 16) ? 4 : 1;
    std::vector<std::thread> pool;
    for (size_t t = 1; t < n_threads; t++) pool.emplace_back(fill, n * t / n_threads, n * (t + 1) / n_threads);
    fill(0, n / n_threads);
    for (auto& th : pool) th.join();
    return RK_OK;
    RK_GUARD_END
}
int rk_exec_lookup_tables(const rk_exec* ex, uint32_t index, uint32_t* range_table, uint32_t* program_table, size_t* program_rows) {
    RK_GUARD_BEGIN
    if (!range_table || !program_rows) return RK_ERR_INVALID;
    ExecSegmentView v;
    RK_TRY(exec_segment_view(ex, index, &v));
    const std::vector<TraceRow>& tr = *v.trace;
    // one pass over the executed cycles: how often each (pc, instruction) pair ran, how often each 16-bit value occurs
    // among the ten limbs a row sends to the range table
    std::vector<uint32_t> hist((size_t)1 << 16, 0);
    std::unordered_map<uint64_t, uint32_t> seen;
    // programs run from a few KiB of text: count per word of the executed pc range; the map only for what does not fit that
    // picture (a range above 16 MiB, an address executed with two different instruction words)
    const uint32_t pc_lo = v.pc_lo, pc_hi = v.pc_hi;
    struct Slot {
        uint32_t ins, count;
    };
    std::vector<Slot> direct;
    const bool use_direct = !tr.empty() && (pc_hi - pc_lo) / 4 < (1u << 22);
    if (use_direct) direct.assign((size_t)(pc_hi - pc_lo) / 4 + 1, Slot{0, 0});
    uint64_t last_key = ~(uint64_t)0;
    uint32_t* last = nullptr;
    for (const TraceRow& r : tr) {
        Slot* sl = use_direct && (r.pc & 3u) == 0 ? &direct[(r.pc - pc_lo) / 4] : nullptr;
        if (sl && (sl->count == 0 || sl->ins == r.ins)) {
            sl->ins = r.ins;
            sl->count++;
        } else {
            const uint64_t key = (uint64_t)r.pc << 32 | r.ins;
            if (key != last_key) {
                last = &seen[key];     // references into an unordered_map stay valid across rehashing
                last_key = key;
            }
            ++*last;
        }
        for (uint32_t v : {r.pc, r.next, r.a, r.b, r.res}) {
            hist[v & 0xffffu]++;
            hist[v >> 16]++;
        }
    }
    for (size_t i = 0; i < direct.size(); i++)
        if (direct[i].count) seen[(uint64_t)(pc_lo + 4 * (uint32_t)i) << 32 | direct[i].ins] += direct[i].count;
    size_t rows = 2;
    while (rows < seen.size()) rows <<= 1;
    const size_t capacity = *program_rows;
    *program_rows = rows;
    if (!program_table || capacity < rows) return RK_ERR_CAPACITY;
    auto mont = [](uint32_t canon) { return bb::mul(canon, bb::R2); };
    for (uint32_t v = 0; v < (1u << 16); v++) {
        range_table[2 * (size_t)v] = mont(v);
        range_table[2 * (size_t)v + 1] = mont(hist[v]);
    }
    std::vector<std::pair<uint64_t, uint32_t>> sorted(seen.begin(), seen.end());
    std::sort(sorted.begin(), sorted.end());
    std::memset(program_table, 0, rows * 5 * sizeof(uint32_t));
    for (size_t i = 0; i < sorted.size(); i++) {
        const uint32_t pc = (uint32_t)(sorted[i].first >> 32), ins = (uint32_t)sorted[i].first;
        uint32_t* row = program_table + 5 * i;
        row[0] = mont(pc & 0xffffu);
        row[1] = mont(pc >> 16);
        row[2] = mont(ins & 0xffffu);
        row[3] = mont(ins >> 16);
        row[4] = mont(sorted[i].second);
    }
    return RK_OK;
    RK_GUARD_END
}
const char* rk_exec_error(const rk_exec* ex) { return ex ? ex->error.c_str() : ""; }
int rk_exec_free(rk_exec* ex) {
    delete ex;
    return RK_OK;
}
int rk_exec_registers(const rk_exec* ex, uint32_t index, uint32_t* start, uint32_t* end) {
    if (!ex || !start || !end || index >= ex->regs.size()) return RK_ERR_INVALID;
    std::copy(ex->regs[index].begin(), ex->regs[index].begin() + 32, start);
    std::copy(ex->regs[index].begin() + 32, ex->regs[index].end(), end);
    return RK_OK;
}
int rk_exec_ecalls(const rk_exec* ex, uint32_t index, uint32_t* out, size_t capacity, size_t* n) {
    if (!ex || !n || index >= ex->ecalls.size()) return RK_ERR_INVALID;
    const auto& ec = ex->ecalls[index];
    *n = ec.size();
    if (ec.size() > capacity || (!out && !ec.empty())) return RK_ERR_CAPACITY;
    for (size_t k = 0; k < ec.size(); k++) out[2 * k] = ec[k][0], out[2 * k + 1] = ec[k][1];
    return RK_OK;
}
int rk_exec_ecall_args(const rk_exec* ex, uint32_t index, uint32_t* out, size_t capacity, size_t* n, uint32_t* pos_start) {
    if (!ex || !n || index >= ex->ecall_args.size()) return RK_ERR_INVALID;
    const auto& ea = ex->ecall_args[index];
    *n = ea.size();
    if (pos_start) *pos_start = ex->in_start[index];
    if (ea.size() > capacity || (!out && !ea.empty())) return RK_ERR_CAPACITY;
    for (size_t k = 0; k < ea.size(); k++) std::copy(ea[k].begin(), ea[k].end(), out + 5 * k);
    return RK_OK;
}
int rk_exec_mem_accesses(const rk_exec* ex, uint32_t index, uint32_t* out, size_t capacity, size_t* n) {
    if (!ex || !n || index >= ex->mem.size()) return RK_ERR_INVALID;
    const auto& mem = ex->mem[index];
    *n = mem.size();
    if (mem.size() > capacity || (!out && !mem.empty())) return RK_ERR_CAPACITY;
    for (size_t k = 0; k < mem.size(); k++) std::copy(mem[k].begin(), mem[k].end(), out + 4 * k);
    return RK_OK;
}
int rk_exec_commit_reads(const rk_exec* ex, uint32_t index, uint32_t* out, size_t capacity, size_t* n, uint32_t* jpos_start) {
    if (!ex || !n || index >= ex->commit_reads.size()) return RK_ERR_INVALID;
    const auto& cr = ex->commit_reads[index];
    *n = cr.size();
    if (jpos_start) *jpos_start = ex->jpos_start[index];
    if (cr.size() > capacity || (!out && !cr.empty())) return RK_ERR_CAPACITY;
    for (size_t k = 0; k < cr.size(); k++) std::copy(cr[k].begin(), cr[k].begin() + 3, out + 3 * k);
    return RK_OK;
}

}  // extern "C"
