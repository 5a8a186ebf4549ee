// RV32IM executor + segmenter: the step BEFORE the proving path --
// `ExecutorImpl::from_elf(env, elf).run()` at reference provers/risc0/driver/src/bonsai.rs:267-269,
// which interprets the guest and cuts the run into segments of at most 2^segment_limit_po2 cycles
// (bonsai.rs:249) that `session.prove()` (bonsai.rs:271) then proves one by one.
//
// Host code (no GPU work: the reference's executor is CPU code too, single-threaded).  What is
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
#include "internal.hpp"

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

// one executed cycle as the witness generator needs it
struct TraceRow {
    uint32_t pc, ins, a, b, res, next, wr;
};

struct rk_exec {
    std::vector<rk_exec_segment> segments;
    std::vector<std::vector<TraceRow>> traces;   // per segment, when rk_exec_opts.record_trace is set
    std::vector<std::array<uint32_t, 64>> regs;  // per segment: x0..x31 at its start, then at its end
    // per segment, with record_trace: (cycle, a0 after the call) of every ecall row -- an ecall READ writes a0 outside
    // TraceRow -- and the lowest / highest pc executed (the rv32i chip set's program table, rk_exec_rv32_*)
    std::vector<std::vector<std::array<uint32_t, 2>>> ecalls;
    std::vector<std::array<uint32_t, 2>> pc_range;
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
    auto rd16 = [&](size_t o) { return (uint32_t)elf[o] | (uint32_t)elf[o + 1] << 8; };
    auto rd32 = [&](size_t o) { return rd16(o) | rd16(o + 2) << 16; };
    if (n < 52 || std::memcmp(elf, "\x7f" "ELF", 4) != 0) { err = "not an ELF file"; return RK_ERR_INVALID; }
    if (elf[4] != 1 || elf[5] != 1) { err = "not a 32-bit little-endian ELF"; return RK_ERR_INVALID; }
    if (rd16(18) != 243) { err = "not a RISC-V ELF (e_machine != 243)"; return RK_ERR_INVALID; }
    m.pc = rd32(24);
    uint32_t phoff = rd32(28), phentsize = rd16(42), phnum = rd16(44);
    if (phentsize < 32 || (uint64_t)phoff + (uint64_t)phentsize * phnum > n) { err = "program headers out of range"; return RK_ERR_INVALID; }
    for (uint32_t i = 0; i < phnum; i++) {
        size_t ph = phoff + (size_t)i * phentsize;
        if (rd32(ph) != 1) continue;  // PT_LOAD
        uint32_t off = rd32(ph + 4), vaddr = rd32(ph + 8), filesz = rd32(ph + 16), memsz = rd32(ph + 20);
        if ((uint64_t)off + filesz > n || filesz > memsz || (uint64_t)vaddr + memsz > 0x100000000ull) {
            err = "PT_LOAD segment out of range";
            return RK_ERR_INVALID;
        }
        for (uint32_t b = 0; b < filesz; b++) m.store_byte(vaddr + b, elf[off + b]);
    }
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
            wr = true;
            break;
        }
        case 0x23: {                                                                 // stores
            uint32_t addr = a + (uint32_t)sext(((ins >> 25) << 5) | ((ins >> 7) & 31), 12);
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
                        *m.word_ptr(dst + 4 * got) = o.input_words[in_pos++];
                        got++;
                    }
                    m.x[10] = got;
                    break;
                }
                case RK_ECALL_COMMIT: {  // a0 = source, a1 = bytes: appended to the journal
                    uint32_t src = m.x[10], len = m.x[11];
                    if (ex.journal.size() + (size_t)len > ((size_t)1 << 24)) return trap("journal larger than 16 MiB");
                    for (uint32_t i = 0; i < len; i++) ex.journal.push_back(m.load_byte(src + i));
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
    uint32_t pc_lo = 0xffffffffu, pc_hi = 0;
    if (o.record_trace) trace.reserve((size_t)std::min<uint64_t>(limit, (uint64_t)1 << 22));  // 28 bytes per cycle, no regrowth copies
    while (cycles < limit) {
        if (o.session_limit && ex->total >= o.session_limit) {
            ex->error = "session limit reached";
            ex->st = RK_ERR_CAPACITY;
            break;
        }
        TraceRow row{};
        if (o.profile) ex->pc_cycles[m.pc]++;
        int r = step(m, *ex, o, ex->in_pos, ex->error, o.record_trace ? &row : nullptr);
        if (r < 0) { ex->st = r; break; }
        if (o.record_trace) {
            trace.push_back(row);
            if (row.ins == 0x00000073u) ecalls.push_back({(uint32_t)cycles, m.x[10]});
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
            ex->pc_range.push_back({pc_lo, pc_hi});
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

// The same columns written by the GPU: one lane per row, the trace rows (28 bytes per cycle) are the only upload --
// 2.5x less over PCIe than the 18 finished columns and none of the host's time (rk_exec_witness_device).
__global__ void exec_witness_kernel(uint32_t* __restrict__ code, uint32_t* __restrict__ data, const TraceRow* __restrict__ tr,
                                    size_t cycles, size_t n, uint32_t end_pc, uint32_t rows_only) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool active = i < cycles;
    TraceRow r{};
    if (active) r = tr[i];
    else r.pc = r.next = end_pc;
    const uint32_t lo = r.pc & 0xffffu, carry = (active && lo + 4 > 0xffffu) ? 1u : 0u;
    const uint32_t seq = (active && r.next == r.pc + 4 && r.pc <= 0xfffffffbu) ? 1u : 0u;
    // rows_only: the 16 data columns as one row-major row per lane (64 contiguous bytes: an rk_p3_table), no code columns
    auto put = [&](uint32_t* base, unsigned col, uint32_t canon) {
        base[rows_only ? i * RK_TRACE_DATA_COLS + col : (size_t)col * n + i] = bb::mul(canon, bb::R2);
    };
    if (!rows_only) {
        put(code, 0, i == 0 ? 1u : 0u);
        put(code, 1, i + 1 == n ? 1u : 0u);
    }
    put(data, 0, lo);
    put(data, 1, r.pc >> 16);
    put(data, 2, r.next & 0xffffu);
    put(data, 3, r.next >> 16);
    put(data, 4, r.ins & 0xffffu);
    put(data, 5, r.ins >> 16);
    put(data, 6, seq);
    put(data, 7, seq ? carry : 0u);
    put(data, 8, r.a & 0xffffu);
    put(data, 9, r.a >> 16);
    put(data, 10, r.b & 0xffffu);
    put(data, 11, r.b >> 16);
    put(data, 12, r.res & 0xffffu);
    put(data, 13, r.res >> 16);
    put(data, 14, r.wr);
    put(data, 15, active ? 1u : 0u);
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
    if (!ex || !code || !data || index >= ex->segments.size() || index >= ex->traces.size()) return RK_ERR_INVALID;
    const rk_exec_segment& seg = ex->segments[index];
    const std::vector<TraceRow>& tr = ex->traces[index];
    const size_t n = (size_t)1 << seg.po2;
    if (tr.size() != seg.cycles || tr.size() > n) return RK_ERR_INTERNAL;
    // every cell is below 2^16 (or a bit): one Montgomery product each; rows are independent, four threads split them
    auto put = [&](uint32_t* base, unsigned col, size_t i, uint32_t canon) { base[(size_t)col * n + i] = bb::mul(canon, bb::R2); };
    auto fill = [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            put(code, 0, i, i == 0 ? 1u : 0u);         // first row
            put(code, 1, i, i + 1 == n ? 1u : 0u);     // last row
            const bool active = i < tr.size();
            TraceRow r{};
            if (active) r = tr[i];
            else r.pc = r.next = seg.end_pc;           // padding: stay where the segment ended
            const uint32_t lo = r.pc & 0xffffu, carry = (active && lo + 4 > 0xffffu) ? 1u : 0u;
            const uint32_t seq = (active && r.next == r.pc + 4 && r.pc <= 0xfffffffbu) ? 1u : 0u;  // no wrap of the 32-bit pc
            put(data, 0, i, lo);
            put(data, 1, i, r.pc >> 16);
            put(data, 2, i, r.next & 0xffffu);
            put(data, 3, i, r.next >> 16);
            put(data, 4, i, r.ins & 0xffffu);
            put(data, 5, i, r.ins >> 16);
            put(data, 6, i, seq);
            put(data, 7, i, seq ? carry : 0u);
            put(data, 8, i, r.a & 0xffffu);
            put(data, 9, i, r.a >> 16);
            put(data, 10, i, r.b & 0xffffu);
            put(data, 11, i, r.b >> 16);
            put(data, 12, i, r.res & 0xffffu);
            put(data, 13, i, r.res >> 16);
            put(data, 14, i, r.wr);
            put(data, 15, i, active ? 1u : 0u);
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
    if (!ex || !range_table || !program_rows || index >= ex->segments.size() || index >= ex->traces.size()) return RK_ERR_INVALID;
    const std::vector<TraceRow>& tr = ex->traces[index];
    if (tr.size() != ex->segments[index].cycles) return RK_ERR_INTERNAL;
    // one pass over the executed cycles: how often each (pc, instruction) pair ran, how often each 16-bit value occurs
    // among the ten limbs a row sends to the range table
    std::vector<uint32_t> hist((size_t)1 << 16, 0);
    std::unordered_map<uint64_t, uint32_t> seen;
    // programs run from a few KiB of text: count per word of the executed pc range; the map only for what does not fit that
    // picture (a range above 16 MiB, an address executed with two different instruction words)
    uint32_t pc_lo = 0xffffffffu, pc_hi = 0;
    for (const TraceRow& r : tr) pc_lo = std::min(pc_lo, r.pc), pc_hi = std::max(pc_hi, r.pc);
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
static int witness_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_code, uint32_t* d_data, bool rows_only);
int rk_exec_witness_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_code, uint32_t* d_data) {
    RK_GUARD_BEGIN
    if (!d_code) return RK_ERR_INVALID;
    return witness_device(ctx, ex, index, d_code, d_data, false);
    RK_GUARD_END
}
int rk_exec_witness_device_rows(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_rows) {
    RK_GUARD_BEGIN
    return witness_device(ctx, ex, index, nullptr, d_rows, true);
    RK_GUARD_END
}
static int witness_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_code, uint32_t* d_data, bool rows_only) {
    {
    if (!ctx || !ex || !d_data || index >= ex->segments.size() || index >= ex->traces.size()) return RK_ERR_INVALID;
    const rk_exec_segment& seg = ex->segments[index];
    const std::vector<TraceRow>& tr = ex->traces[index];
    const size_t n = (size_t)1 << seg.po2;
    if (tr.size() != seg.cycles || tr.size() > n) return RK_ERR_INTERNAL;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    void* d_tr = nullptr;
    RK_TRY(rk::dev_alloc(ctx, std::max<size_t>(tr.size(), 1) * sizeof(TraceRow), &d_tr));
    int st = RK_OK;
    if (!tr.empty()) {
        // the trace stays valid while `ex` lives, but the caller may free `ex` right after this call: wait for the copy
        hipError_t e = hipMemcpyAsync(d_tr, tr.data(), tr.size() * sizeof(TraceRow), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            ctx->last_error = std::string("rk_exec_witness_device h2d: ") + hipGetErrorString(e);
            st = RK_ERR_HIP;
        }
    }
    if (st == RK_OK) {
        hipLaunchKernelGGL(exec_witness_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_code, d_data,
                           (const TraceRow*)d_tr, tr.size(), n, seg.end_pc, rows_only ? 1u : 0u);
        st = rk::post_launch(ctx, "exec_witness_kernel");
    }
    rk::dev_free(ctx, d_tr);
    return st;
    }
}
const char* rk_exec_error(const rk_exec* ex) { return ex ? ex->error.c_str() : ""; }
int rk_exec_free(rk_exec* ex) {
    delete ex;
    return RK_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The rv32i chip set (include/raiko_hip.h rk_exec_rv32_shard_device; raiko_amd/rv32.py is the same in numpy and names
// every column).  Per segment on the GPU: prep (decode, recompute the written value, pack the three accesses, count
// program hits) -> block_last (last access per register per 128 rows) -> scan (exclusive max-scan of those 32-vectors)
// -> rows (in-block resolve of each access's predecessor, the cpu row staged through LDS, RANGE16 / BYTE counts) ->
// the program, register, byte and range tables.
namespace rv32 {

constexpr unsigned TB = 128;   // rows per block (the cpu rows kernel stages TB x 69 words in LDS, 121 / 133 for rv32i-cf / rv32im)
constexpr unsigned CPU_W = RK_RV32_CPU_COLS, PROG_W = RK_RV32_PROGRAM_COLS, REG_W = RK_RV32_REGISTER_COLS,
                   BYTE_W = RK_RV32_BYTE_COLS, CF_CPU_W = RK_RV32CF_CPU_COLS, CF_PROG_W = RK_RV32CF_PROGRAM_COLS,
                   SHIFT_W = RK_RV32CF_SHIFT_COLS, SHIFT_USED = 9 * 256, IM_CPU_W = RK_RV32IM_CPU_COLS,
                   IM_PROG_W = RK_RV32IM_PROGRAM_COLS, MD_W = RK_RV32IM_MULDIV_COLS;
// the chip set a kernel writes: each one's tables are the previous one's with columns (and tables) appended
enum ChipSet : int { CS_I, CS_CF, CS_IM };
enum : unsigned {
    PC_LO, PC_HI, NX_LO, NX_HI, INS_LO, INS_HI, SEQ, CARRY, A_LO, A_HI, B_LO, B_HI, RES_LO, RES_HI, WR, ACTIVE,
    RS1, RS2, WREG, IMM_LO, IMM_HI, IS_ADD, IS_SUB, IS_SLT, IS_SLTU, IS_BIT, BOP, IS_IMM, IS_LUI, IS_AUIPC, IS_LINK,
    TSA, TSB, TSW, PA_TS, PB_TS, PW_TS, PW_LO, PW_HI, DA_LO, DA_HI, DB_LO, DB_HI, DW_LO, DW_HI,
    OB_LO, OB_HI, C0, C1, D_LO, D_HI, SA, SB, SNE, SA_CHK, SB_CHK, BA, BB = BA + 4, BR = BB + 4,
    // rv32i-cf (raiko_amd/rv32cf.py): the twelve looked-up fields, then the branch, next-pc and shift columns
    IS_JAL = BR + 4, IS_BEQ, IS_BNE, IS_BLT, IS_BGE, IS_BLTU, IS_BGEU, JIMM_LO, JIMM_HI, IS_SLL, IS_SRL, IS_SRA,
    IS_BR, TAKEN, BD_LO, BD_HI, BC0, BC1, EQ, INV, M_SA, M_SB, NC0, NC1, DROP, NXH,
    IS_SHIFT, KB, Q = KB + 3, SK = Q + 4, T, FILL, U_LO, U_HI, V_LO, V_HI, SX, SLO = SX + 4, SHI = SLO + 4,
    // rv32im (raiko_amd/rv32im.py): the eight M selectors and their sum (looked up), the op, the multiplicity
    IS_MUL = SHI + 4, IS_M = IS_MUL + 8, MOP, M_W
};
static_assert(SHI + 4 == CF_CPU_W, "rv32i-cf cpu columns");
static_assert(M_W + 1 == IM_CPU_W, "rv32im cpu columns");
constexpr uint32_t OPCODES[11] = {0x37, 0x17, 0x6f, 0x67, 0x63, 0x03, 0x23, 0x13, 0x33, 0x0f, 0x73};
enum { O_LUI, O_AUIPC, O_JAL, O_JALR, O_BRANCH, O_LOAD, O_STORE, O_OPIMM, O_OP, O_FENCE, O_SYSTEM };

struct Dec {
    int opc;   // index into OPCODES, -1 for none
    uint32_t f3, rd, rs1, rs2, wreg, imm, opr, is_add, is_sub, is_slt, is_sltu, is_bit, bop, is_imm, is_lui, is_auipc,
        is_link, wr;
    // rv32i-cf: bsel = the branch (0..5: BEQ BNE BLT BGE BLTU BGEU) or -1; jimm = imm_B of a branch, imm_J of JAL
    int bsel;
    uint32_t is_jal, jimm, is_sll, is_srl, is_sra;
    uint32_t is_m;   // rv32im: an M word (OP, funct7 = 1); its op is f3
};

__host__ __device__ inline Dec decode(uint32_t ins) {
    Dec d{};
    d.opc = -1;
    for (int k = 0; k < 11; k++)
        if ((ins & 0x7fu) == OPCODES[k]) d.opc = k;
    d.f3 = (ins >> 12) & 7;
    d.rd = (ins >> 7) & 31;
    d.rs1 = (ins >> 15) & 31;
    d.rs2 = (ins >> 20) & 31;
    const uint32_t b25 = (ins >> 25) & 1, b30 = (ins >> 30) & 1;
    d.opr = d.opc == O_OP && !b25;
    const uint32_t opimm = d.opc == O_OPIMM, alu = d.opr | opimm;
    d.is_add = (d.f3 == 0) && ((d.opr && !b30) || opimm);
    d.is_sub = d.opr && d.f3 == 0 && b30;
    d.is_slt = alu && d.f3 == 2;
    d.is_sltu = alu && d.f3 == 3;
    d.is_bit = alu && (d.f3 == 4 || d.f3 == 6 || d.f3 == 7);
    d.bop = !alu ? 0 : d.f3 == 4 ? 3 : d.f3 == 6 ? 2 : d.f3 == 7 ? 1 : 0;
    d.is_imm = opimm;
    d.is_lui = d.opc == O_LUI;
    d.is_auipc = d.opc == O_AUIPC;
    d.is_link = d.opc == O_JAL || d.opc == O_JALR;
    if (opimm || d.opc == O_LOAD || d.opc == O_JALR) d.imm = (uint32_t)((int32_t)ins >> 20);
    else if (d.is_lui || d.is_auipc) d.imm = ins & 0xfffff000u;
    const bool writes = d.is_lui || d.is_auipc || d.is_link || d.opc == O_LOAD || opimm || d.opc == O_OP;
    d.wr = (writes && d.rd != 0) || d.opc == O_SYSTEM;
    d.wreg = d.rd + (d.opc == O_SYSTEM ? 10u : 0u);
    d.is_jal = d.opc == O_JAL;
    d.bsel = -1;
    if (d.opc == O_BRANCH) {
        d.bsel = d.f3 < 2 ? (int)d.f3 : d.f3 >= 4 ? (int)d.f3 - 2 : -1;
        const uint32_t b = (ins >> 31) << 12 | ((ins >> 7) & 1) << 11 | ((ins >> 25) & 0x3f) << 5 | ((ins >> 8) & 0xf) << 1;
        d.jimm = (uint32_t)((int32_t)(b << 19) >> 19);
    } else if (d.is_jal) {
        const uint32_t j = (ins >> 31) << 20 | ((ins >> 12) & 0xff) << 12 | ((ins >> 20) & 1) << 11 | ((ins >> 21) & 0x3ff) << 1;
        d.jimm = (uint32_t)((int32_t)(j << 11) >> 11);
    }
    d.is_sll = alu && d.f3 == 1;
    d.is_srl = alu && d.f3 == 5 && !b30;
    d.is_sra = alu && d.f3 == 5 && b30;
    d.is_m = d.opc == O_OP && (ins >> 25) == 1;
    return d;
}

// the value a row writes: recomputed for the constrained ops, the side list's for an ecall, TraceRow.res otherwise
__device__ inline uint32_t written(const Dec& d, const TraceRow& r, uint32_t ecall_a0) {
    const uint32_t a = r.a, ob = d.is_imm ? d.imm : r.b;
    if (d.is_add) return a + ob;
    if (d.is_sub) return a - ob;
    if (d.is_sltu) return a < ob;
    if (d.is_slt) return (int32_t)a < (int32_t)ob;
    if (d.is_bit) return d.f3 == 4 ? a ^ ob : d.f3 == 6 ? a | ob : a & ob;
    if (d.is_lui) return d.imm;
    if (d.is_auipc) return r.pc + d.imm;
    if (d.is_link) return r.pc + 4;
    if (d.opc == O_SYSTEM) return ecall_a0;
    return r.res;
}

__device__ inline uint32_t enc(uint32_t canon) { return bb::mul(canon, bb::R2); }

// a histogram bin += 1 for every lane with `on`; the lanes of a wave that agree with its first active lane add once
__device__ inline void hist_add(uint32_t* h, uint32_t v, bool on) {
    const uint64_t act = __ballot(on);
    if (!act) return;
    const int first = __ffsll((unsigned long long)act) - 1;
    const uint32_t lv = __shfl(v, first);
    const uint64_t same = __ballot(on && v == lv);
    if ((int)(threadIdx.x & 63) == first) atomicAdd(&h[lv], (uint32_t)__popcll(same));
    else if (on && v != lv) atomicAdd(&h[v], 1u);
}

// the row a cpu lane writes row-major: staged in LDS (odd stride: no bank conflicts), then whole lines to HBM
template <unsigned W>
__device__ inline void flush_rows(uint32_t* out, const uint32_t* s, size_t r0, size_t n_rows) {
    constexpr unsigned SW = W | 1;
    const size_t rows = n_rows - r0 < blockDim.x ? n_rows - r0 : blockDim.x;
    for (size_t k = threadIdx.x; k < rows * W; k += blockDim.x) out[r0 * W + k] = s[(k / W) * SW + k % W];
}

__global__ void prep_kernel(const TraceRow* __restrict__ tr, size_t cycles, size_t n, const uint32_t* __restrict__ ecalls,
                            uint32_t n_ecalls, uint32_t pc_base, uint32_t n_slots, uint32_t* __restrict__ wval,
                            uint32_t* __restrict__ acc, uint32_t* __restrict__ prog_mult, uint32_t* __restrict__ prog_ins,
                            uint32_t* __restrict__ err, uint32_t* __restrict__ mflag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i >= cycles) {
        wval[i] = 0;
        acc[i] = 0;
        if (mflag) mflag[i] = 0;
        return;
    }
    const TraceRow r = tr[i];
    const Dec d = decode(r.ins);
    if (mflag) mflag[i] = d.is_m && d.wr;   // rv32im: the rows with M_W = 1, one muldiv row each
    uint32_t a0 = 0;
    if (d.opc == O_SYSTEM) {   // the side list is in cycle order: binary search
        uint32_t lo = 0, hi = n_ecalls;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) / 2;
            if (ecalls[2 * mid] < i) lo = mid + 1;
            else hi = mid;
        }
        if (lo < n_ecalls && ecalls[2 * lo] == i) a0 = ecalls[2 * lo + 1];
        else atomicOr(err, 2u);
    }
    wval[i] = written(d, r, a0);
    acc[i] = d.rs1 | d.rs2 << 5 | d.wreg << 10 | d.wr << 15 | 1u << 16;
    const uint32_t slot = (r.pc - pc_base) >> 2;
    if (slot >= n_slots) {
        atomicOr(err, 4u);
        return;
    }
    atomicAdd(&prog_mult[slot], 1u);
    const uint32_t old = atomicCAS(&prog_ins[slot], 0u, r.ins);
    if (old != 0 && old != r.ins) atomicOr(err, 1u);    // one pc, two instruction words in one shard
}

__device__ inline void unpack(uint32_t v, uint32_t& rs1, uint32_t& rs2, uint32_t& wreg, bool& wr, bool& active) {
    rs1 = v & 31;
    rs2 = (v >> 5) & 31;
    wreg = (v >> 10) & 31;
    wr = (v >> 15) & 1;
    active = (v >> 16) & 1;
}

__global__ void block_last_kernel(const uint32_t* __restrict__ acc, uint32_t* __restrict__ blk) {
    __shared__ uint32_t s[32];
    if (threadIdx.x < 32) s[threadIdx.x] = 0;
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    uint32_t rs1, rs2, wreg;
    bool wr, active;
    unpack(acc[i], rs1, rs2, wreg, wr, active);
    if (active) {
        const uint32_t tsa = (uint32_t)(3 * i + 1);
        atomicMax(&s[rs1], tsa);
        atomicMax(&s[rs2], tsa + 1);
        if (wr) atomicMax(&s[wreg], tsa + 2);
    }
    __syncthreads();
    if (threadIdx.x < 32) blk[(size_t)blockIdx.x * 32 + threadIdx.x] = s[threadIdx.x];
}

// one workgroup of 1024: lane = register (t & 31) x chunk of blocks (t >> 5); blk becomes its exclusive prefix max
__global__ void scan_kernel(uint32_t* __restrict__ blk, size_t nb, uint32_t* __restrict__ final_ts) {
    __shared__ uint32_t cm[32][32];
    const unsigned r = threadIdx.x & 31, c = threadIdx.x >> 5;
    const size_t j0 = nb * c / 32, j1 = nb * (c + 1) / 32;
    uint32_t m = 0;
    for (size_t j = j0; j < j1; j++) m = max(m, blk[j * 32 + r]);
    cm[c][r] = m;
    __syncthreads();
    uint32_t run = 0;
    for (unsigned k = 0; k < c; k++) run = max(run, cm[k][r]);
    for (size_t j = j0; j < j1; j++) {
        const uint32_t v = blk[j * 32 + r];
        blk[j * 32 + r] = run;
        run = max(run, v);
    }
    if (c == 31) final_ts[r] = run;
}

__device__ inline uint32_t value_at(uint32_t ts, uint32_t reg, const TraceRow* tr, const uint32_t* wval, const uint32_t* init) {
    if (ts == 0) return init[reg];
    const uint32_t j = (ts - 1) / 3, k = (ts - 1) % 3;
    return k == 0 ? tr[j].a : k == 1 ? tr[j].b : wval[j];
}

// CS_CF: the rv32i-cf row (columns 0..67 are the rv32i row, the rest rv32cf.py's) and its SHIFT counts; CS_IM: the
// rv32i-cf row with rv32im.py's M columns appended
template <int CS>
__global__ void __launch_bounds__(TB) rows_kernel(const TraceRow* __restrict__ tr, size_t cycles, uint32_t end_pc,
                                                   const uint32_t* __restrict__ acc, const uint32_t* __restrict__ wval,
                                                   const uint32_t* __restrict__ pre, const uint32_t* __restrict__ init,
                                                   uint32_t* __restrict__ out, uint32_t* __restrict__ hist,
                                                   uint32_t* __restrict__ byte_mult, uint32_t* __restrict__ shift_mult,
                                                   size_t n) {
    constexpr bool CF = CS != CS_I;
    constexpr unsigned W = CS == CS_IM ? IM_CPU_W : CF ? CF_CPU_W : CPU_W;
    extern __shared__ uint32_t s_rows[];            // TB x (W | 1)
    __shared__ uint32_t s_wave[32][TB / 64];
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t rs1, rs2, wreg;
    bool wr, active;
    unpack(acc[i], rs1, rs2, wreg, wr, active);
    const uint32_t tsa = (uint32_t)(3 * i + 1);
    // per register: the latest access among this wave's rows up to this one (inclusive max-scan over the lanes)
    uint32_t incl[32];
#pragma unroll
    for (unsigned r = 0; r < 32; r++) {
        uint32_t v = 0;
        if (active) {
            if (rs1 == r) v = tsa;
            if (rs2 == r) v = tsa + 1;
            if (wr && wreg == r) v = tsa + 2;
        }
#pragma unroll
        for (unsigned off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(v, off);
            if (lane >= off) v = max(v, t);
        }
        incl[r] = v;
        if (lane == 63) s_wave[r][wave] = v;
    }
    __syncthreads();
    uint32_t e1 = 0, e2 = 0, e3 = 0;
#pragma unroll
    for (unsigned r = 0; r < 32; r++) {
        uint32_t ex = __shfl_up(incl[r], 1);
        if (lane == 0) ex = 0;
        for (unsigned w = 0; w < wave; w++) ex = max(ex, s_wave[r][w]);
        ex = max(ex, pre[(size_t)blockIdx.x * 32 + r]);
        if (rs1 == r) e1 = ex;
        if (rs2 == r) e2 = ex;
        if (wreg == r) e3 = ex;
    }
    uint32_t* row = s_rows + threadIdx.x * (W | 1);
    for (unsigned c = 0; c < W; c++) row[c] = 0;
    uint32_t res = 0, bop = 0, ba = 0, bb_ = 0, pa = 0, pb = 0, pw = 0, sa = 0, sb = 0, is_slt = 0, d_lo = 0, d_hi = 0;
    bool is_br = false, is_link = false, is_shift = false, m_sa = false, m_sb = false;   // rv32i-cf multiplicities
    if (active) {
        const TraceRow r = tr[i];
        const Dec d = decode(r.ins);
        res = wval[i];
        pa = e1;
        pb = rs2 == rs1 ? tsa : e2;
        pw = wr ? (wreg == rs2 ? tsa + 1 : wreg == rs1 ? tsa : e3) : 0;
        const uint32_t pwv = wr ? value_at(pw, wreg, tr, wval, init) : 0;
        const uint32_t ob = d.is_imm ? d.imm : r.b;
        const uint32_t seq = (r.next == r.pc + 4 && r.pc <= 0xfffffffbu) ? 1u : 0u;
        const uint32_t carry = ((r.pc & 0xffffu) + 4 > 0xffffu) ? 1u : 0u;
        const bool sublt = d.is_sub || d.is_slt || d.is_sltu;
        const uint32_t dd = sublt ? r.a - ob : 0;
        uint32_t x = 0, y = 0;
        if (d.is_add) x = r.a, y = ob;
        else if (d.is_auipc) x = r.pc, y = d.imm;
        else if (d.is_link) x = r.pc, y = 4;
        else if (sublt) x = dd, y = ob;
        const uint32_t c0 = ((x & 0xffffu) + (y & 0xffffu)) >> 16, c1 = ((x >> 16) + (y >> 16) + c0) >> 16;
        sa = r.a >> 31;
        sb = ob >> 31;
        is_slt = d.is_slt;
        d_lo = dd & 0xffffu;
        d_hi = dd >> 16;
        const uint32_t da = tsa - pa - 1, db = tsa + 1 - pb - 1, dw = wr ? tsa + 2 - pw - 1 : 0;
        const uint32_t vals[][2] = {
            {PC_LO, r.pc & 0xffffu}, {PC_HI, r.pc >> 16}, {NX_LO, r.next & 0xffffu}, {NX_HI, r.next >> 16},
            {INS_LO, r.ins & 0xffffu}, {INS_HI, r.ins >> 16}, {SEQ, seq}, {CARRY, seq & carry},
            {A_LO, r.a & 0xffffu}, {A_HI, r.a >> 16}, {B_LO, r.b & 0xffffu}, {B_HI, r.b >> 16},
            {RES_LO, res & 0xffffu}, {RES_HI, res >> 16}, {WR, d.wr}, {ACTIVE, 1},
            {RS1, d.rs1}, {RS2, d.rs2}, {WREG, d.wreg}, {IMM_LO, d.imm & 0xffffu}, {IMM_HI, d.imm >> 16},
            {IS_ADD, d.is_add}, {IS_SUB, d.is_sub}, {IS_SLT, d.is_slt}, {IS_SLTU, d.is_sltu}, {IS_BIT, d.is_bit},
            {BOP, d.bop}, {IS_IMM, d.is_imm}, {IS_LUI, d.is_lui}, {IS_AUIPC, d.is_auipc}, {IS_LINK, d.is_link},
            {PA_TS, pa}, {PB_TS, pb}, {PW_TS, pw}, {PW_LO, pwv & 0xffffu}, {PW_HI, pwv >> 16},
            {DA_LO, da & 0x3fffu}, {DA_HI, da >> 14}, {DB_LO, db & 0x3fffu}, {DB_HI, db >> 14},
            {DW_LO, dw & 0x3fffu}, {DW_HI, dw >> 14}, {OB_LO, ob & 0xffffu}, {OB_HI, ob >> 16}, {C0, c0}, {C1, c1},
            {D_LO, d_lo}, {D_HI, d_hi}, {SA, sa}, {SB, sb}, {SNE, sa ^ sb},
            {SA_CHK, 2 * (r.a >> 16) - 65536 * sa}, {SB_CHK, 2 * (ob >> 16) - 65536 * sb}};
        for (const auto& kv : vals) row[kv[0]] = kv[1];
        if (d.is_bit) {
            bop = d.bop;
            ba = r.a;
            bb_ = ob;
            for (unsigned k = 0; k < 4; k++) {
                row[BA + k] = (r.a >> (8 * k)) & 255;
                row[BB + k] = (ob >> (8 * k)) & 255;
                row[BR + k] = (res >> (8 * k)) & 255;
            }
        }
        if constexpr (CF) {
            const uint32_t a = r.a, b = r.b;
            // branch decision
            is_br = d.bsel >= 0;
            const bool eqv = a == b, ltu = a < b, lts = (int32_t)a < (int32_t)b;
            const bool cond[6] = {eqv, !eqv, lts, !lts, ltu, !ltu};
            const bool taken = is_br && cond[d.bsel];
            if (is_br) {
                const uint32_t dd = a - b, z = (dd & 0xffffu) + (dd >> 16);
                row[IS_BEQ + d.bsel] = 1;
                row[BD_LO] = dd & 0xffffu;
                row[BD_HI] = dd >> 16;
                row[BC0] = (a & 0xffffu) < (b & 0xffffu);
                row[BC1] = ltu;
                row[EQ] = eqv;
                row[INV] = z ? bb::decode(bb::inv(enc(z))) : 0u;
            }
            m_sb = d.bsel == 2 || d.bsel == 3;
            m_sa = m_sb || d.is_sra;
            row[IS_BR] = is_br;
            row[TAKEN] = taken;
            row[M_SA] = m_sa;
            row[M_SB] = m_sb;
            // next pc = base + offset (mod 2^32), JALR's low bit dropped
            const bool jalr = d.opc == O_JALR;
            is_link = d.is_link;
            const uint32_t base = jalr ? a : r.pc, off = jalr ? d.imm : (taken || d.is_jal) ? d.jimm : 4u;
            const uint32_t nc0 = ((base & 0xffffu) + (off & 0xffffu)) >> 16, nc1 = ((base >> 16) + (off >> 16) + nc0) >> 16;
            row[IS_JAL] = d.is_jal;
            row[JIMM_LO] = d.jimm & 0xffffu;
            row[JIMM_HI] = d.jimm >> 16;
            row[NC0] = nc0;
            row[NC1] = nc1;
            row[DROP] = jalr ? (base + off) & 1u : 0u;
            row[NXH] = is_link ? (r.next & 0xffffu) >> 1 : 0u;
            // shifts: s = k + 8 q; the bytes of a' (a, complemented for SRA of a negative a) through the shift table
            row[IS_SLL] = d.is_sll;
            row[IS_SRL] = d.is_srl;
            row[IS_SRA] = d.is_sra;
            is_shift = d.is_sll || d.is_srl || d.is_sra;
            if (is_shift) {
                const uint32_t amt = d.is_imm ? d.rs2 : b & 31u, k = amt & 7u, q = amt >> 3;
                const bool fill = d.is_sra && (a >> 31);
                const uint32_t ap = fill ? ~a : a, sk = d.is_sll ? k : 8u - k;
                const uint32_t u = d.is_sll ? ap << amt : ap >> amt, v = fill ? ~u : u;
                row[IS_SHIFT] = 1;
                for (unsigned bit = 0; bit < 3; bit++) row[KB + bit] = (k >> bit) & 1u;
                row[Q + q] = 1;
                row[SK] = sk;
                row[T] = d.is_imm ? 0u : (b & 0xffffu) >> 5;
                row[FILL] = fill;
                row[U_LO] = u & 0xffffu;
                row[U_HI] = u >> 16;
                row[V_LO] = v & 0xffffu;
                row[V_HI] = v >> 16;
                for (unsigned j = 0; j < 4; j++) {
                    const uint32_t x = (ap >> (8 * j)) & 255u;
                    row[SX + j] = x;
                    row[SLO + j] = (x << sk) & 255u;
                    row[SHI + j] = (x << sk) >> 8;
                }
            }
        }
        if constexpr (CS == CS_IM) {
            if (d.is_m) {
                row[IS_MUL + d.f3] = 1;
                row[IS_M] = 1;
                row[MOP] = d.f3;
                row[M_W] = d.wr;
            }
        }
    } else {
        row[PC_LO] = row[NX_LO] = end_pc & 0xffffu;
        row[PC_HI] = row[NX_HI] = end_pc >> 16;
    }
    row[TSA] = tsa;
    row[TSB] = tsa + 1;
    row[TSW] = tsa + 2;
    // RANGE16: the limbs the row sends (rv32.py RANGE_SENDS), BYTE: four triples of a bitwise row
    const unsigned rc[] = {PC_LO, PC_HI, NX_LO, NX_HI, RES_LO, RES_HI, D_LO, D_HI, DA_LO, DA_HI, DB_LO, DB_HI};
    for (unsigned c : rc) hist_add(hist, row[c], active);
    hist_add(hist, row[DW_LO], wr);
    hist_add(hist, row[DW_HI], wr);
    hist_add(hist, row[SA_CHK], is_slt);
    hist_add(hist, row[SB_CHK], is_slt);
    if (bop)
        for (unsigned k = 0; k < 4; k++)
            atomicAdd(&byte_mult[(bop - 1) << 16 | ((ba >> (8 * k)) & 255) << 8 | ((bb_ >> (8 * k)) & 255)], 1u);
    if constexpr (CF) {   // rv32cf.py RANGE_SENDS past rv32i's, then the four SHIFT lookups (k, x) -> row k 256 + x
        hist_add(hist, row[BD_LO], is_br);
        hist_add(hist, row[BD_HI], is_br);
        hist_add(hist, row[NXH], is_link);
        hist_add(hist, row[T], is_shift);
        hist_add(hist, row[SA_CHK], m_sa);
        hist_add(hist, row[SB_CHK], m_sb);
        for (unsigned j = 0; j < 4; j++) hist_add(shift_mult, row[SK] << 8 | row[SX + j], is_shift);
    }
    for (unsigned c = 0; c < W; c++) row[c] = enc(row[c]);
    __syncthreads();
    flush_rows<W>(out, s_rows, (size_t)blockIdx.x * TB, n);
}

// CS_CF: the rv32i-cf program row, rv32i's 77 columns and the twelve fields the cf cpu row looks up; CS_IM: then the
// nine M fields and the funct7 test's three partial products
template <int CS>
__global__ void program_kernel(const uint32_t* __restrict__ prog_ins, const uint32_t* __restrict__ prog_mult,
                               uint32_t n_slots, uint32_t pc_base, size_t n_rows, uint32_t* __restrict__ out) {
    constexpr bool CF = CS != CS_I;
    constexpr unsigned W = CS == CS_IM ? IM_PROG_W : CF ? CF_PROG_W : PROG_W;
    extern __shared__ uint32_t s_rows[];
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t* row = s_rows + threadIdx.x * (W | 1);
    for (unsigned c = 0; c < W; c++) row[c] = 0;
    if (s < n_rows) {   // past the executed range: the row of word 0 at pc 0, multiplicity 0
        const bool in = s < n_slots;
        const uint32_t pc = in ? pc_base + 4 * (uint32_t)s : 0u, ins = in ? prog_ins[s] : 0u;
        const Dec d = decode(ins);
        const uint32_t v[20] = {pc & 0xffffu, pc >> 16, ins & 0xffffu, ins >> 16, d.rs1, d.rs2, d.wreg, d.imm & 0xffffu,
                                d.imm >> 16, d.is_add, d.is_sub, d.is_slt, d.is_sltu, d.is_bit, d.bop, d.is_imm,
                                d.is_lui, d.is_auipc, d.is_link, d.wr};
        for (unsigned c = 0; c < 20; c++) row[c] = v[c];
        row[20] = in ? prog_mult[s] : 0u;
        for (unsigned k = 0; k < 32; k++) row[21 + k] = (ins >> k) & 1;
        if (d.opc >= 0) {
            row[53 + d.opc] = 1;
            row[64 + d.f3] = 1;
        }
        const uint32_t b = ins >> 7;
        const uint32_t z1 = (~b & 1) & (~b >> 1 & 1), z2 = z1 & (~b >> 2 & 1), rdz = z2 & (~b >> 3 & 1) & (~b >> 4 & 1);
        row[72] = d.opr;
        row[73] = z1;
        row[74] = z2;
        row[75] = rdz;
        row[76] = d.rd;
        if constexpr (CF) {
            uint32_t* e = row + PROG_W - IS_JAL;     // e[c]: the field of cpu column c
            e[IS_JAL] = d.is_jal;
            if (d.bsel >= 0) e[IS_BEQ + d.bsel] = 1;
            e[JIMM_LO] = d.jimm & 0xffffu;
            e[JIMM_HI] = d.jimm >> 16;
            e[IS_SLL] = d.is_sll;
            e[IS_SRL] = d.is_srl;
            e[IS_SRA] = d.is_sra;
        }
        if constexpr (CS == CS_IM) {
            uint32_t* m = row + CF_PROG_W;          // IS_MUL .. IS_REMU, IS_M, then op b25 !b26, !b27 !b28, !b29 !b30
            const auto nb = [&](unsigned k) { return ((ins >> k) & 1u) ^ 1u; };
            const uint32_t f7a = (d.opc == O_OP) & (ins >> 25) & 1u & nb(26), f7b = f7a & nb(27) & nb(28), f7c = f7b & nb(29) & nb(30);
            if (d.is_m) m[d.f3] = 1;
            m[8] = d.is_m;
            m[9] = f7a;
            m[10] = f7b;
            m[11] = f7c;
        }
    }
    for (unsigned c = 0; c < W; c++) row[c] = enc(row[c]);
    __syncthreads();
    flush_rows<W>(out, s_rows, (size_t)blockIdx.x * blockDim.x, n_rows);
}

// the rv32i-cf shift table (rv32cf.py shift_rows): row k 256 + x = (k, x, x 2^k mod 256, x 2^k / 256, count, bits of x,
// k one-hot, bits of x 2^k); rows past 9 x 256 the true tuple (0, 0, 0, 0) with count 0
__global__ void shift_kernel(const uint32_t* __restrict__ shift_mult, uint32_t* __restrict__ out) {
    extern __shared__ uint32_t s_rows[];
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t* row = s_rows + threadIdx.x * (SHIFT_W | 1);
    for (unsigned c = 0; c < SHIFT_W; c++) row[c] = 0;
    const uint32_t k = r < SHIFT_USED ? (uint32_t)(r >> 8) : 0u, x = r < SHIFT_USED ? (uint32_t)(r & 255) : 0u, v = x << k;
    row[0] = k;
    row[1] = x;
    row[2] = v & 255u;
    row[3] = v >> 8;
    row[4] = r < SHIFT_USED ? shift_mult[r] : 0u;
    for (unsigned bit = 0; bit < 8; bit++) row[5 + bit] = (x >> bit) & 1u;
    row[13 + k] = 1;
    for (unsigned bit = 0; bit < 16; bit++) row[22 + bit] = (v >> bit) & 1u;
    for (unsigned c = 0; c < SHIFT_W; c++) row[c] = enc(row[c]);
    __syncthreads();
    flush_rows<SHIFT_W>(out, s_rows, (size_t)blockIdx.x * blockDim.x, (size_t)1 << RK_RV32CF_SHIFT_LOG_ROWS);
}

__global__ void byte_kernel(const uint32_t* __restrict__ byte_mult, uint32_t* __restrict__ out) {
    extern __shared__ uint32_t s_rows[];
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t* row = s_rows + threadIdx.x * (BYTE_W | 1);
    for (unsigned c = 0; c < BYTE_W; c++) row[c] = 0;
    if (r < (3u << 16)) {
        const uint32_t op = (uint32_t)(r >> 16) + 1, x = (r >> 8) & 255, y = r & 255;
        row[0] = op;
        row[1] = x;
        row[2] = y;
        row[3] = op == 1 ? (x & y) : op == 2 ? (x | y) : (x ^ y);
        for (unsigned k = 0; k < 8; k++) {
            row[4 + k] = (x >> k) & 1;
            row[12 + k] = (y >> k) & 1;
        }
        row[19 + op] = 1;
        row[23] = byte_mult[r];
    }
    for (unsigned c = 0; c < BYTE_W; c++) row[c] = enc(row[c]);
    __syncthreads();
    flush_rows<BYTE_W>(out, s_rows, (size_t)blockIdx.x * blockDim.x, (size_t)1 << RK_RV32_BYTE_LOG_ROWS);
}

__global__ void range_kernel(const uint32_t* __restrict__ hist, uint32_t* __restrict__ out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= (1u << 16)) return;
    out[2 * v] = enc(v);
    out[2 * v + 1] = enc(hist[v]);
}

// 32 lanes: the register table (rv32.py register_rows); fin gets the final values
__global__ void register_kernel(const uint32_t* __restrict__ final_ts, const uint32_t* __restrict__ init,
                                const TraceRow* __restrict__ tr, const uint32_t* __restrict__ wval,
                                uint32_t* __restrict__ fin, uint32_t* __restrict__ out) {
    __shared__ uint32_t s_fin[32];
    extern __shared__ uint32_t s_rows[];
    const unsigned r = threadIdx.x;
    s_fin[r] = value_at(final_ts[r], r, tr, wval, init);
    fin[r] = s_fin[r];
    __syncthreads();
    uint32_t* row = s_rows + r * (REG_W | 1);
    row[0] = r;
    row[1] = 0;
    row[2] = final_ts[r];
    for (unsigned j = 0; j < 32; j++) {
        const bool in = r + j < 32;
        row[3 + j] = in ? init[r + j] & 0xffffu : 0;
        row[35 + j] = in ? init[r + j] >> 16 : 0;
        row[67 + j] = in ? s_fin[r + j] & 0xffffu : 0;
        row[99 + j] = in ? s_fin[r + j] >> 16 : 0;
    }
    for (unsigned c = 0; c < REG_W; c++) row[c] = enc(row[c]);
    __syncthreads();
    flush_rows<REG_W>(out, s_rows, 0, 32);
}

// ---- rv32im: the muldiv table (raiko_amd/rv32im.py muldiv_witness names every column)
enum : unsigned {
    D_SEL, D_MULT = 8, D_OP, D_A_LO, D_A_HI, D_B_LO, D_B_HI, D_R_LO, D_R_HI, D_ONE, D_X, D_Y = D_X + 4, D_Z = D_Y + 4,
    D_C = D_Z + 4, D_CY = D_C + 8, D_S = D_CY + 8, D_L = D_S + 4, D_E = D_L + 4, D_AND = D_E + 4, D_BZ = D_AND + 8, D_BINV,
    D_OVF, D_OINV, D_BM_LO, D_BM_HI, D_KB, D_RM_LO, D_RM_HI, D_KR, D_DL_LO, D_DL_HI, D_K0
};
static_assert(D_K0 + 1 == MD_W, "rv32im muldiv columns");
// the byte pairs looked up as ANDs (rv32im.py BYTE_PAIRS), the top bytes looked up in the shift table (SIGN_BYTES)
constexpr unsigned MD_PAIRS[8][2] = {{D_X, D_X + 1}, {D_X + 2, D_Y}, {D_Y + 1, D_Y + 2}, {D_Z, D_Z + 1}, {D_Z + 2, D_C},
                                     {D_C + 1, D_C + 2}, {D_C + 4, D_C + 5}, {D_C + 6, D_C + 7}};
constexpr unsigned MD_RANGE[14] = {D_CY, D_CY + 1, D_CY + 2, D_CY + 3, D_CY + 4, D_CY + 5, D_CY + 6, D_CY + 7,
                                   D_BM_LO, D_BM_HI, D_RM_LO, D_RM_HI, D_DL_LO, D_DL_HI};

// per block of TB cpu rows: how many have M_W = 1
__global__ void mcount_kernel(const uint32_t* __restrict__ mflag, uint32_t* __restrict__ mblk) {
    const int c = __syncthreads_count(mflag[(size_t)blockIdx.x * TB + threadIdx.x] != 0);
    if (threadIdx.x == 0) mblk[blockIdx.x] = (uint32_t)c;
}

// one workgroup of 1024: mblk becomes its exclusive prefix sum, total the sum
__global__ void mscan_kernel(uint32_t* __restrict__ mblk, size_t nb, uint32_t* __restrict__ total) {
    __shared__ uint32_t part[1024];
    const unsigned t = threadIdx.x;
    const size_t j0 = nb * t / 1024, j1 = nb * (t + 1) / 1024;
    uint32_t sum = 0;
    for (size_t j = j0; j < j1; j++) sum += mblk[j];
    part[t] = sum;
    __syncthreads();
    for (unsigned off = 1; off < 1024; off <<= 1) {   // inclusive Hillis-Steele scan of the chunk sums
        const uint32_t v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (size_t j = j0; j < j1; j++) {
        const uint32_t v = mblk[j];
        mblk[j] = run;
        run += v;
    }
    if (t == 1023) *total = run;
}

// the muldiv index of every row with M_W = 1: its block's offset + the flagged rows before it in the block; idx[k] = the
// cpu row of muldiv row k (k < count)
__global__ void mcompact_kernel(const uint32_t* __restrict__ mflag, const uint32_t* __restrict__ mblk, size_t count,
                                uint32_t* __restrict__ idx) {
    __shared__ uint32_t s_wave[TB / 64];
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool on = mflag[i] != 0;
    const uint64_t bal = __ballot(on);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t k = mblk[blockIdx.x] + (uint32_t)__popcll(bal & ((1ull << lane) - 1));
    for (unsigned w = 0; w < wave; w++) k += s_wave[w];
    if (on && k < count) idx[k] = (uint32_t)i;
}

// one lane per muldiv row: row k < count is the witness of cpu row idx[k]'s op on its 32-bit operands (64-bit products
// and the division's quotient / remainder, the executor's conventions), rows past count padding (ONE = 1, the rest 0);
// the RANGE16 / BYTE / SHIFT counts of the active rows go to the shard's histograms
__global__ void muldiv_kernel(const TraceRow* __restrict__ tr, size_t cycles, const uint32_t* __restrict__ wval,
                              const uint32_t* __restrict__ idx, size_t count, size_t n_rows, uint32_t* __restrict__ out,
                              uint32_t* __restrict__ hist, uint32_t* __restrict__ byte_mult, uint32_t* __restrict__ shift_mult,
                              uint32_t* __restrict__ err) {
    extern __shared__ uint32_t s_rows[];
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t* row = s_rows + threadIdx.x * (MD_W | 1);
    for (unsigned c = 0; c < MD_W; c++) row[c] = 0;
    row[D_ONE] = 1;
    bool on = k < count;
    const uint32_t i = on ? idx[k] : 0u;
    if (on && i >= cycles) {   // the device's count is not the host's (reported after the run)
        atomicOr(err, 16u);
        on = false;
    }
    if (on) {
        const TraceRow r = tr[i];
        const uint32_t op = (r.ins >> 12) & 7, a = r.a, b = r.b, res = wval[i];
        const bool is_mul = op < 4, divs = op == 4 || op == 6, bz = b == 0, ovf = divs && a == 0x80000000u && b == 0xffffffffu;
        const bool sgn_x = op == 1 || op == 2 || divs, sgn_y = op == 1 || divs;
        uint32_t q, rm;
        if (bz) q = 0xffffffffu, rm = a;
        else if (ovf) q = 0x80000000u, rm = 0;
        else if (divs) q = (uint32_t)((int32_t)a / (int32_t)b), rm = (uint32_t)((int32_t)a % (int32_t)b);
        else q = a / b, rm = a % b;
        const uint32_t x = is_mul ? a : q, z = is_mul ? 0u : rm;
        uint32_t xe[8], ye[8], ze[8], cb[8];
        const uint32_t ex = sgn_x && (x >> 31), ey = sgn_y && (b >> 31), ez = divs && (z >> 31);
        for (unsigned j = 0; j < 4; j++) {
            xe[j] = (x >> (8 * j)) & 255u, ye[j] = (b >> (8 * j)) & 255u, ze[j] = (z >> (8 * j)) & 255u;
            xe[j + 4] = 255u * ex, ye[j + 4] = 255u * ey, ze[j + 4] = 255u * ez;
            row[D_X + j] = xe[j];
            row[D_Y + j] = ye[j];
            row[D_Z + j] = ze[j];
        }
        uint32_t carry = 0;   // < 8 * 255^2 + 255 + carry < 2^20: no overflow
        for (unsigned c = 0; c < 8; c++) {
            uint32_t acc = ze[c] + carry;
            for (unsigned j = 0; j <= c; j++) acc += xe[j] * ye[c - j];
            cb[c] = acc & 255u;
            carry = acc >> 8;
            row[D_C + c] = cb[c];
            row[D_CY + c] = carry;
        }
        const uint32_t sc = cb[3] >> 7, ec = divs && sc;
        const uint32_t lo_w = cb[0] | cb[1] << 8 | cb[2] << 16 | cb[3] << 24, hi_w = cb[4] | cb[5] << 8 | cb[6] << 16 | cb[7] << 24;
        const uint32_t want = op == 0 ? lo_w : is_mul ? hi_w : (op == 4 || op == 5) ? q : rm;
        if (want != res) atomicOr(err, 8u);   // the executor's result is not the op's
        row[D_SEL + op] = 1;
        row[D_MULT] = 1;
        row[D_OP] = op;
        row[D_A_LO] = a & 0xffffu;
        row[D_A_HI] = a >> 16;
        row[D_B_LO] = b & 0xffffu;
        row[D_B_HI] = b >> 16;
        row[D_R_LO] = res & 0xffffu;
        row[D_R_HI] = res >> 16;
        const uint32_t sgn[4] = {x >> 31, b >> 31, z >> 31, sc}, ext[4] = {ex, ey, ez, ec},
                       top[4] = {xe[3], ye[3], ze[3], cb[3]};
        for (unsigned j = 0; j < 4; j++) {
            row[D_S + j] = sgn[j];
            row[D_L + j] = (2 * top[j]) & 255u;
            row[D_E + j] = ext[j];
        }
        for (unsigned j = 0; j < 8; j++) row[D_AND + j] = row[MD_PAIRS[j][0]] & row[MD_PAIRS[j][1]];
        if (!is_mul) {
            const uint32_t bsum = (b & 0xffffu) + (b >> 16);
            row[D_BZ] = bz;
            row[D_BINV] = bsum ? bb::decode(bb::inv(enc(bsum))) : 0u;
        }
        if (divs) {
            uint32_t dev = 2 * (cb[0] + cb[1] + cb[2]) + 2 * (1 - sc) + row[D_L + 3];
            for (unsigned j = 0; j < 4; j++) dev += 2 * (255u - ye[j]);
            row[D_OVF] = ovf;
            row[D_OINV] = dev ? bb::decode(bb::inv(enc(dev))) : 0u;
        }
        const uint32_t bm = ey ? 0u - b : b, zm = ez ? 0u - z : z;   // |b|, |r| (two's complement; |-2^31| = 2^31)
        row[D_BM_LO] = bm & 0xffffu;
        row[D_BM_HI] = bm >> 16;
        row[D_KB] = ey && (b & 0xffffu);
        row[D_RM_LO] = zm & 0xffffu;
        row[D_RM_HI] = zm >> 16;
        row[D_KR] = ez && (z & 0xffffu);
        if (!is_mul && !bz) {   // |r| + 1 + DL = |b|
            const uint32_t dl = bm - zm - 1;
            row[D_DL_LO] = dl & 0xffffu;
            row[D_DL_HI] = dl >> 16;
            row[D_K0] = ((zm & 0xffffu) + 1 + (dl & 0xffffu)) >> 16;
        }
    }
    for (unsigned c : MD_RANGE) hist_add(hist, row[c], on);
    for (unsigned j = 0; j < 4; j++) hist_add(shift_mult, 256u + row[D_X + 3 + 4 * j], on);   // (1, top byte) -> row 256 + x
    // AND (op 1) of each byte pair; the wave-aggregated add, as M loops repeat their operands
    for (unsigned j = 0; j < 8; j++) hist_add(byte_mult, row[MD_PAIRS[j][0]] << 8 | row[MD_PAIRS[j][1]], on);
    for (unsigned c = 0; c < MD_W; c++) row[c] = enc(row[c]);
    __syncthreads();
    flush_rows<MD_W>(out, s_rows, (size_t)blockIdx.x * blockDim.x, n_rows);
}

}  // namespace rv32

static size_t rv32_program_rows(const rk_exec* ex, uint32_t index, uint32_t* n_slots) {
    const auto& pr = ex->pc_range[index];
    const uint32_t slots = ex->traces[index].empty() ? 0 : (pr[1] - pr[0]) / 4 + 1;
    size_t rows = 2;
    while (rows < slots) rows <<= 1;
    if (n_slots) *n_slots = slots;
    return rows;
}

// the rows of a segment's trace with M_W = 1 (an M word writing a register other than x0): its muldiv rows
static size_t rv32im_count(const rk_exec* ex, uint32_t index) {
    size_t c = 0;   // decode(ins).is_m && decode(ins).wr: opcode OP, funct7 = 1, rd != 0
    for (const TraceRow& r : ex->traces[index]) c += (r.ins & 0xfe00007fu) == 0x02000033u && (r.ins & 0xf80u);
    return c;
}

static size_t rv32im_muldiv_rows(size_t count) {
    size_t rows = (size_t)1 << RK_RV32IM_MULDIV_MIN_LOG_ROWS;
    while (rows < count) rows <<= 1;
    return rows;
}

// CS_CF: the rv32i-cf tables (d_shift the sixth); CS_IM: the rv32im tables (d_muldiv the seventh, muldiv_rows rows);
// CS_I: rv32i's five
template <int CS>
static int rv32_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_cpu, uint32_t* d_program,
                             size_t program_rows, uint32_t* d_register, uint32_t* d_byte, uint32_t* d_range,
                             uint32_t* d_shift, uint32_t* d_muldiv, size_t muldiv_rows) {
    using namespace rv32;
    constexpr bool CF = CS != CS_I, IM = CS == CS_IM;
    if (!ctx || !ex || !d_cpu || !d_program || !d_register || !d_byte || !d_range || (CF && !d_shift) || (IM && !d_muldiv) ||
        index >= ex->segments.size() || index >= ex->traces.size())
        return RK_ERR_INVALID;
    const rk_exec_segment& seg = ex->segments[index];
    const std::vector<TraceRow>& tr = ex->traces[index];
    const auto& ec = ex->ecalls[index];
    const size_t n = (size_t)1 << seg.po2, nb = n / TB;
    if (tr.size() != seg.cycles || tr.size() > n || n % TB) return RK_ERR_INTERNAL;
    uint32_t n_slots = 0;
    if (rv32_program_rows(ex, index, &n_slots) != program_rows) return RK_ERR_CAPACITY;
    if (n_slots > (1u << 22)) {
        ctx->last_error = "rk_exec_rv32_shard_device: executed pc range wider than 2^22 words";
        return RK_ERR_CAPACITY;
    }
    const size_t m_count = IM ? rv32im_count(ex, index) : 0;
    if (IM) {   // a power of two that holds every muldiv row, no taller than the cpu table; nothing is written otherwise
        if (muldiv_rows < rv32im_muldiv_rows(m_count)) {
            ctx->last_error = "rk_exec_rv32im_shard_device: the muldiv table has fewer rows than the segment needs";
            return RK_ERR_CAPACITY;
        }
        if (muldiv_rows & (muldiv_rows - 1) || muldiv_rows > std::max<size_t>(n, rv32im_muldiv_rows(0))) return RK_ERR_INVALID;
    }
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // scratch, in one allocation: trace | ecalls | wval | acc | blk | final_ts | fin | init | err | hist | byte | prog mult / ins
    // | shift counts | rv32im: M flags | block counts | total | muldiv row -> cpu row
    const size_t w_tr = (std::max<size_t>(tr.size(), 1) * sizeof(TraceRow) + 3) / 4, w_ec = 2 * std::max<size_t>(ec.size(), 1);
    size_t off[18], at = 0;
    const size_t words[18] = {w_tr, w_ec, n, n, nb * 32, 32, 32, 32, 1, (size_t)1 << 16, (size_t)3 << 16,
                              std::max<uint32_t>(n_slots, 1), std::max<uint32_t>(n_slots, 1), CF ? SHIFT_USED : 1u,
                              IM ? n : 1, IM ? nb : 1, 1, std::max<size_t>(m_count, 1)};
    for (int k = 0; k < 18; k++) off[k] = at, at += (words[k] + 63) & ~(size_t)63;
    void* base = nullptr;
    RK_TRY(rk::dev_alloc(ctx, at * 4, &base));
    uint32_t* w = (uint32_t*)base;
    const TraceRow* d_tr = (const TraceRow*)(w + off[0]);
    uint32_t *d_ec = w + off[1], *wval = w + off[2], *acc = w + off[3], *blk = w + off[4], *final_ts = w + off[5],
             *fin = w + off[6], *init = w + off[7], *err = w + off[8], *hist = w + off[9], *bmult = w + off[10],
             *pmult = w + off[11], *pins = w + off[12], *smult = w + off[13], *mflag = w + off[14], *mblk = w + off[15],
             *mtotal = w + off[16], *midx = w + off[17];
    std::vector<uint32_t> ec_flat(2 * ec.size());
    for (size_t k = 0; k < ec.size(); k++) ec_flat[2 * k] = ec[k][0], ec_flat[2 * k + 1] = ec[k][1];
    uint32_t host_fin[34] = {0};
    int st = RK_OK;
    auto hip = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && st == RK_OK) {
            ctx->last_error = std::string("rk_exec_rv32_shard_device ") + what + ": " + hipGetErrorString(e);
            st = RK_ERR_HIP;
        }
    };
    auto launched = [&](const char* what) {
        if (st == RK_OK) st = rk::post_launch(ctx, what);
    };
    if (!tr.empty()) hip(hipMemcpyAsync((void*)d_tr, tr.data(), tr.size() * sizeof(TraceRow), hipMemcpyHostToDevice, ctx->stream), "h2d");
    if (!ec.empty()) hip(hipMemcpyAsync(d_ec, ec_flat.data(), ec_flat.size() * 4, hipMemcpyHostToDevice, ctx->stream), "h2d");
    hip(hipMemcpyAsync(init, ex->regs[index].data(), 32 * 4, hipMemcpyHostToDevice, ctx->stream), "h2d");
    hip(hipMemsetAsync(err, 0, (off[13] + words[13] - off[8]) * 4, ctx->stream), "memset");   // err .. shift counts
    if (st == RK_OK) {
        hipLaunchKernelGGL(prep_kernel, dim3((unsigned)nb), dim3(TB), 0, ctx->stream, d_tr, tr.size(), n, d_ec,
                           (uint32_t)ec.size(), ex->pc_range[index][0], n_slots, wval, acc, pmult, pins, err,
                           IM ? mflag : nullptr);
        launched("rv32 prep_kernel");
    }
    if (st == RK_OK) {
        hipLaunchKernelGGL(block_last_kernel, dim3((unsigned)nb), dim3(TB), 0, ctx->stream, acc, blk);
        launched("rv32 block_last_kernel");
    }
    if (st == RK_OK) {
        hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, blk, nb, final_ts);
        launched("rv32 scan_kernel");
    }
    if (st == RK_OK) {
        const size_t lds = TB * ((IM ? IM_CPU_W : CF ? CF_CPU_W : CPU_W) | 1) * 4;
        if (lds > 64 * 1024)   // rv32im's 133-word rows: past the default dynamic LDS limit (160 KiB per CU)
            hip(hipFuncSetAttribute((const void*)rows_kernel<CS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "lds");
        if (st == RK_OK)
            hipLaunchKernelGGL(rows_kernel<CS>, dim3((unsigned)nb), dim3(TB), lds, ctx->stream, d_tr, tr.size(), seg.end_pc, acc,
                               wval, blk, init, d_cpu, hist, bmult, smult, n);
        launched("rv32 rows_kernel");
    }
    if (IM && st == RK_OK) {   // the muldiv rows: count per block, scan, compact, then one lane per row (before the
                               // byte / range / shift tables: its counts go into theirs)
        hipLaunchKernelGGL(mcount_kernel, dim3((unsigned)nb), dim3(TB), 0, ctx->stream, mflag, mblk);
        launched("rv32 mcount_kernel");
        if (st == RK_OK) {
            hipLaunchKernelGGL(mscan_kernel, dim3(1), dim3(1024), 0, ctx->stream, mblk, nb, mtotal);
            launched("rv32 mscan_kernel");
        }
        if (st == RK_OK) {
            hipLaunchKernelGGL(mcompact_kernel, dim3((unsigned)nb), dim3(TB), 0, ctx->stream, mflag, mblk, m_count, midx);
            launched("rv32 mcompact_kernel");
        }
        if (st == RK_OK) {
            const unsigned b = (unsigned)std::min<size_t>(muldiv_rows, TB);
            hipLaunchKernelGGL(muldiv_kernel, dim3((unsigned)(muldiv_rows / b)), dim3(b), b * (MD_W | 1) * 4, ctx->stream, d_tr,
                               tr.size(), wval, midx, m_count, muldiv_rows, d_muldiv, hist, bmult, smult, err);
            launched("rv32 muldiv_kernel");
        }
    }
    if (st == RK_OK) {
        const unsigned b = (unsigned)std::min<size_t>(program_rows, TB);
        hipLaunchKernelGGL(program_kernel<CS>, dim3((unsigned)((program_rows + b - 1) / b)), dim3(b),
                           b * ((IM ? IM_PROG_W : CF ? CF_PROG_W : PROG_W) | 1) * 4, ctx->stream, pins, pmult, n_slots, ex->pc_range[index][0],
                           program_rows, d_program);
        launched("rv32 program_kernel");
    }
    if (st == RK_OK) {
        hipLaunchKernelGGL(byte_kernel, dim3((1u << RK_RV32_BYTE_LOG_ROWS) / TB), dim3(TB), TB * (BYTE_W | 1) * 4,
                           ctx->stream, bmult, d_byte);
        launched("rv32 byte_kernel");
    }
    if (st == RK_OK) {
        hipLaunchKernelGGL(range_kernel, dim3((1u << 16) / TB), dim3(TB), 0, ctx->stream, hist, d_range);
        launched("rv32 range_kernel");
    }
    if (st == RK_OK) {
        hipLaunchKernelGGL(register_kernel, dim3(1), dim3(32), 32 * (REG_W | 1) * 4, ctx->stream, final_ts, init, d_tr,
                           wval, fin, d_register);
        launched("rv32 register_kernel");
    }
    if (CF && st == RK_OK) {   // after rows_kernel (and muldiv_kernel) on the stream: the counts are complete
        hipLaunchKernelGGL(shift_kernel, dim3((1u << RK_RV32CF_SHIFT_LOG_ROWS) / TB), dim3(TB), TB * (SHIFT_W | 1) * 4,
                           ctx->stream, smult, d_shift);
        launched("rv32 shift_kernel");
    }
    // the tables are complete and the scratch can go: read back the final registers and the error flags
    hip(hipMemcpyAsync(host_fin, fin, 32 * 4, hipMemcpyDeviceToHost, ctx->stream), "d2h");
    hip(hipMemcpyAsync(host_fin + 32, err, 4, hipMemcpyDeviceToHost, ctx->stream), "d2h");
    if (IM) hip(hipMemcpyAsync(host_fin + 33, mtotal, 4, hipMemcpyDeviceToHost, ctx->stream), "d2h");
    hip(hipStreamSynchronize(ctx->stream), "sync");
    rk::dev_free(ctx, base);
    if (st != RK_OK) return st;
    if (host_fin[32] & 7) {
        ctx->last_error = host_fin[32] & 1 ? "rk_exec_rv32_shard_device: a pc executed with two instruction words in one shard"
                                           : "rk_exec_rv32_shard_device: trace and side list disagree";
        return RK_ERR_INVALID;
    }
    if (IM && (host_fin[32] || host_fin[33] != m_count)) {
        ctx->last_error = "rk_exec_rv32im_shard_device: an M result or the muldiv row count is not the executor's";
        return RK_ERR_INTERNAL;
    }
    if (!std::equal(host_fin, host_fin + 32, ex->regs[index].begin() + 32)) {
        ctx->last_error = "rk_exec_rv32_shard_device: the register accesses do not end in the executor's registers";
        return RK_ERR_INTERNAL;
    }
    return RK_OK;
}

extern "C" {

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
int rk_exec_rv32_sizes(const rk_exec* ex, uint32_t index, size_t* program_rows) {
    RK_GUARD_BEGIN
    if (!ex || !program_rows || index >= ex->segments.size() || index >= ex->traces.size()) return RK_ERR_INVALID;
    *program_rows = rv32_program_rows(ex, index, nullptr);
    return RK_OK;
    RK_GUARD_END
}
int rk_exec_rv32_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_cpu, uint32_t* d_program,
                              size_t program_rows, uint32_t* d_register, uint32_t* d_byte, uint32_t* d_range) {
    RK_GUARD_BEGIN
    return rv32_shard_device<rv32::CS_I>(ctx, ex, index, d_cpu, d_program, program_rows, d_register, d_byte, d_range, nullptr,
                                         nullptr, 0);
    RK_GUARD_END
}
int rk_exec_rv32cf_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_cpu, uint32_t* d_program,
                                size_t program_rows, uint32_t* d_register, uint32_t* d_byte, uint32_t* d_range,
                                uint32_t* d_shift) {
    RK_GUARD_BEGIN
    return rv32_shard_device<rv32::CS_CF>(ctx, ex, index, d_cpu, d_program, program_rows, d_register, d_byte, d_range, d_shift,
                                          nullptr, 0);
    RK_GUARD_END
}
int rk_exec_rv32im_sizes(const rk_exec* ex, uint32_t index, size_t* muldiv_rows) {
    RK_GUARD_BEGIN
    if (!ex || !muldiv_rows || index >= ex->segments.size() || index >= ex->traces.size()) return RK_ERR_INVALID;
    *muldiv_rows = rv32im_muldiv_rows(rv32im_count(ex, index));
    return RK_OK;
    RK_GUARD_END
}
int rk_exec_rv32im_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_cpu, uint32_t* d_program,
                                size_t program_rows, uint32_t* d_register, uint32_t* d_byte, uint32_t* d_range,
                                uint32_t* d_shift, uint32_t* d_muldiv, size_t muldiv_rows) {
    RK_GUARD_BEGIN
    return rv32_shard_device<rv32::CS_IM>(ctx, ex, index, d_cpu, d_program, program_rows, d_register, d_byte, d_range, d_shift,
                                          d_muldiv, muldiv_rows);
    RK_GUARD_END
}

}  // extern "C"
