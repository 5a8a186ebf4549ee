// CPU walk through the io-form lane bodies of raiko_amd/csrc/rv32_rows.hpp (raiko_amd/rv32io.py): the 48-column
// preprocessed program matrix of the io key, and the cpu, memop and io tables of a recorded trace with its access list and
// its ecall side list, in Montgomery form.  Where the GPU resolves predecessors by scans and finds an io row's call by
// binary search (rv32_shards.hip), this walks the rows in order.  Built by tests/test_rv32_io.py, which compares the tables
// with raiko_amd/rv32io.py word for word.
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
extern "C" int emul_rv32io_prep(const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs, const uint32_t* words,
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
        program_prep_row_io(o, full, d);
        for (unsigned c = 0; c < MEM_PROG_W; c++) program[s * MEM_PROG_W + c] = enc(o[c]);
    }
    return 0;
}

// trace: cycles x (pc, ins, a, b, res, next, wr); ecalls: n_ecalls x (cycle, a0 after); args: n_ecalls x (cycle, t0, a0, a1,
// pos); acc: count x (cycle, word address, before, after); cpu: n x 148, memop: memop_rows x 64, io: io_rows x 47.
// -> 0, or 1 a side list / 2 the access list does not fit the trace / 3 an access is not what its instruction names /
// 4 a table is too small / 5 an io row is not the call's
extern "C" int emul_rv32io_shard(const uint32_t* trace, size_t cycles, size_t n, uint32_t end_pc, const uint32_t* init,
                                 const uint32_t* ecalls, const uint32_t* args, size_t n_ecalls, const uint32_t* acc, size_t count,
                                 uint32_t n_input, uint32_t pos_start, uint32_t* cpu, uint32_t* memop, size_t memop_rows,
                                 uint32_t* io, size_t io_rows) {
    std::fill(cpu, cpu + n * IO_CPU_W, 0u);
    std::fill(memop, memop + memop_rows * MO_W, 0u);
    std::fill(io, io + io_rows * IO_W, 0u);
    if (count > memop_rows) return 4;
    uint32_t last_ts[32] = {0}, last_val[32];
    std::copy(init, init + 32, last_val);
    std::map<uint32_t, uint32_t> word_ts;
    size_t ec = 0, k = 0, q = 0;
    uint32_t pos = pos_start, prev_head_ts = 0;
    bool halted = false;
    for (size_t i = 0; i < n; i++) {
        uint32_t* row = cpu + i * IO_CPU_W;
        const uint32_t tsa = (uint32_t)(3 * i + 1);
        if (i < cycles) {
            const uint32_t* t = trace + 7 * i;
            TraceRow r{t[0], t[1], t[2], t[3], t[4], t[5], t[6]};
            const Dec d = decode_io(r.ins);
            uint32_t a0 = 0, t0 = 0, pt = 0;
            EcallArg e{};
            if (d.opc == O_SYSTEM) {
                if (ec >= n_ecalls || ecalls[2 * ec] != i || args[5 * ec] != i) return 1;
                e = EcallArg{args[5 * ec], args[5 * ec + 1], args[5 * ec + 2], args[5 * ec + 3], args[5 * ec + 4]};
                a0 = ecalls[2 * ec + 1];
                r.a = e.a0, r.b = e.a1, t0 = e.t0;   // the io form of the trace
                if (last_val[5] != t0) return 1;
                pt = last_ts[5];
                last_ts[5] = tsa;
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
            const size_t k0 = k;
            for (; k < count && acc[4 * k] == i; k++) {
                const MemAccess a{acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]};
                auto it = word_ts.find(a.waddr);
                const uint32_t pts = it == word_ts.end() ? 0u : it->second;
                word_ts[a.waddr] = tsa;
                uint32_t* mrow = memop + k * MO_W;
                mrow[G_ONE] = 1;
                if (!memop_row(mrow, a, r, d, res, pts, true)) return 3;
            }
            const uint32_t here = (uint32_t)(k - k0);
            cpu_row_mem(row, d, here);
            if (here != (d.is_sys ? here : row[M_MEM])) return 2;
            cpu_row_io(row, d, t0, tsa, pt);
            if (d.opc == O_SYSTEM) {   // the head row, then the word rows
                if (q + 1 + here > io_rows) return 4;
                if (e.pos != pos) return 5;
                uint32_t* h = io + q * IO_W;
                if (!io_head_row(h, e, a0, here, n_input, ec > 0, prev_head_ts)) return 5;
                halted = e.t0 == 0;
                io_row_tail(h, pos, true, halted);
                q++;
                for (uint32_t j = 0; j < here; j++, q++, pos++) {
                    const MemAccess a{acc[4 * (k0 + j)], acc[4 * (k0 + j) + 1], acc[4 * (k0 + j) + 2], acc[4 * (k0 + j) + 3]};
                    if (!io_word_row(io + q * IO_W, e, here, j, a)) return 5;
                    io_row_tail(io + q * IO_W, pos, true, 0u);
                }
                prev_head_ts = tsa;
                ec++;
            }
        } else {
            trace_cells(padding_row(end_pc), false, row);
        }
        row[TSA] = tsa, row[TSB] = tsa + 1, row[TSW] = tsa + 2;
        finish(row, IO_CPU_W);
    }
    if (k != count || ec != n_ecalls) return 2;
    for (size_t j = 0; j < memop_rows; j++) {
        memop[j * MO_W + G_ONE] = 1;
        finish(memop + j * MO_W, MO_W);
    }
    for (size_t j = 0; j < io_rows; j++) {
        if (j >= q) io_row_tail(io + j * IO_W, pos, false, halted);
        finish(io + j * IO_W, IO_W);
    }
    return 0;
}

// the shard driver's check of an ecall side list against its trace (io_list_ok) -> 1 accepted, 0 refused
extern "C" int emul_rv32io_list_ok(const uint32_t* trace, size_t cycles, const uint32_t* args, size_t count) {
    std::vector<TraceRow> tr(cycles);
    for (size_t i = 0; i < cycles; i++) {
        const uint32_t* t = trace + 7 * i;
        tr[i] = TraceRow{t[0], t[1], t[2], t[3], t[4], t[5], t[6]};
    }
    std::vector<EcallArg> list(count);
    for (size_t k = 0; k < count; k++) list[k] = EcallArg{args[5 * k], args[5 * k + 1], args[5 * k + 2], args[5 * k + 3], args[5 * k + 4]};
    return io_list_ok(tr.data(), cycles, list.data(), count) ? 1 : 0;
}
