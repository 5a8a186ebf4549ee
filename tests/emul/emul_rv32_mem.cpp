// CPU walk through the rv32im-mem lane bodies of raiko_amd/csrc/rv32_rows.hpp: the 48-column preprocessed program matrix
// of an image, and the cpu, memop and memory tables of a recorded trace with its access list, in Montgomery form.  Where
// the GPU sorts the accesses by address and links neighbours (rv32_shards.hip), this walks the list in order and keeps
// the last access per word in a map.  Built by tests/test_rv32_mem_chips.py, which compares the tables with
// raiko_amd/rv32mem.py word for word.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

#include "rv32_rows.hpp"

using namespace rv32;

static void finish(uint32_t* row, unsigned w) {
    for (unsigned c = 0; c < w; c++) row[c] = enc(row[c]);
}

// program: program_rows x 48.  -> 0, or 1 for more segments than the table holds
extern "C" int emul_rv32mem_prep(const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs, const uint32_t* words,
                                 size_t n_words, uint32_t* program, size_t program_rows) {
    if (n_segs > RK_RV32ELF_MAX_SEGMENTS) return 1;
    Image im{};
    im.n_segs = n_segs;
    for (uint32_t k = 0; k < n_segs; k++) im.vaddr[k] = seg_vaddr[k], im.words[k] = seg_words[k];
    for (size_t s = 0; s < program_rows; s++) {
        uint32_t full[IM_PROG_W] = {0}, o[MEM_PROG_W];
        const bool in = s < n_words;
        const uint32_t pc = in ? image_pc(im, (uint32_t)s) : 0u, ins = in ? words[s] : 0u;
        const Dec d = decode(ins);
        program_row_i(full, pc, ins, d, 0u);
        program_row_cf(full, d);
        program_row_im(full, ins, d);
        program_prep_row_mem(o, full, d);
        for (unsigned c = 0; c < MEM_PROG_W; c++) program[s * MEM_PROG_W + c] = enc(o[c]);
    }
    return 0;
}

// trace: cycles x (pc, ins, a, b, res, next, wr); ecalls: n_ecalls x (cycle, a0 after); acc: count x (cycle, word address,
// before, after); cpu: n x 141, memop: memop_rows x 64, memory: memory_rows x 13.  -> 0, or 1 ecall list / 2 the access
// list does not fit the trace / 3 an access is not what its instruction names / 4 a table is too small
extern "C" int emul_rv32mem_shard(const uint32_t* trace, size_t cycles, size_t n, uint32_t end_pc, const uint32_t* init,
                                  const uint32_t* ecalls, size_t n_ecalls, const uint32_t* acc, size_t count, uint32_t* cpu,
                                  uint32_t* memop, size_t memop_rows, uint32_t* memory, size_t memory_rows) {
    std::fill(cpu, cpu + n * MEM_CPU_W, 0u);
    std::fill(memop, memop + memop_rows * MO_W, 0u);
    std::fill(memory, memory + memory_rows * BD_W, 0u);
    if (count > memop_rows) return 4;
    uint32_t last_ts[32] = {0}, last_val[32];
    std::copy(init, init + 32, last_val);
    struct Word {
        uint32_t init, fin, fts;
    };
    std::map<uint32_t, Word> words;   // ascending addresses: the memory table's order
    size_t ec = 0, k = 0;
    for (size_t i = 0; i < n; i++) {
        uint32_t* row = cpu + i * MEM_CPU_W;
        const uint32_t tsa = (uint32_t)(3 * i + 1);
        if (i < cycles) {
            const uint32_t* t = trace + 7 * i;
            const TraceRow r{t[0], t[1], t[2], t[3], t[4], t[5], t[6]};
            const Dec d = decode(r.ins);
            uint32_t a0 = 0;
            if (d.opc == O_SYSTEM) {
                if (ec >= n_ecalls || ecalls[2 * ec] != i) return 1;
                a0 = ecalls[2 * ec++ + 1];
            }
            const uint32_t res = written(d, r, a0);
            const uint32_t pa = last_ts[d.rs1];
            last_ts[d.rs1] = tsa, last_val[d.rs1] = r.a;
            const uint32_t pb = last_ts[d.rs2];
            last_ts[d.rs2] = tsa + 1, last_val[d.rs2] = r.b;
            const uint32_t pw = d.wr ? last_ts[d.wreg] : 0, pwv = d.wr ? last_val[d.wreg] : 0;
            if (d.wr) last_ts[d.wreg] = tsa + 2, last_val[d.wreg] = res;
            Mults m;
            cpu_row_i(row, r, d, res, tsa, pa, pb, pw, pwv, m);
            cpu_row_cf(row, r, d, m);
            cpu_row_im(row, d);
            uint32_t here = 0;
            for (; k < count && acc[4 * k] == i; k++, here++) {
                const MemAccess a{acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]};
                auto it = words.find(a.waddr);
                const uint32_t pts = it == words.end() ? 0u : it->second.fts;
                if (it == words.end()) it = words.insert({a.waddr, Word{a.before, 0, 0}}).first;
                it->second.fin = a.after;
                it->second.fts = tsa;
                uint32_t* mrow = memop + k * MO_W;
                mrow[G_ONE] = 1;
                if (!memop_row(mrow, a, r, d, res, pts)) return 3;
            }
            cpu_row_mem(row, d, here);
            if (here != (d.is_sys ? here : row[M_MEM])) return 2;
        } else {
            trace_cells(padding_row(end_pc), false, row);
        }
        row[TSA] = tsa, row[TSB] = tsa + 1, row[TSW] = tsa + 2;
        finish(row, MEM_CPU_W);
    }
    if (k != count) return 2;
    for (size_t j = 0; j < memop_rows; j++) {
        memop[j * MO_W + G_ONE] = 1;
        finish(memop + j * MO_W, MO_W);
    }
    if (words.size() > memory_rows) return 4;
    size_t j = 0;
    for (auto it = words.begin(); it != words.end(); ++it, j++) {
        auto nx = std::next(it);
        memory_row(memory + j * BD_W, it->first, it->second.init, it->second.fin, it->second.fts, nx != words.end(),
                   nx == words.end() ? 0u : nx->first);
        finish(memory + j * BD_W, BD_W);
    }
    return 0;
}

// the shard driver's check of an access list against its trace (mem_list_ok) -> 1 accepted, 0 refused
extern "C" int emul_rv32mem_list_ok(const uint32_t* trace, size_t cycles, const uint32_t* acc, size_t count) {
    std::vector<TraceRow> tr(cycles);
    for (size_t i = 0; i < cycles; i++) {
        const uint32_t* t = trace + 7 * i;
        tr[i] = TraceRow{t[0], t[1], t[2], t[3], t[4], t[5], t[6]};
    }
    std::vector<MemAccess> list(count);
    for (size_t k = 0; k < count; k++) list[k] = MemAccess{acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]};
    return mem_list_ok(tr.data(), cycles, list.data(), count) ? 1 : 0;
}
