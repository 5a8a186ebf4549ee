// CPU walk of a recorded trace through the lane bodies of raiko_amd/csrc/rv32_rows.hpp: the cpu and program tables of one
// shard, and rv32im's muldiv table, in Montgomery form.  Where the GPU resolves each register access's predecessor with
// scans (rv32_shards.hip), this walks the rows in order and keeps the last access per register.  Built by
// tests/test_rv32_chips.py, which compares the tables with rv32.py / rv32cf.py / rv32im.py word for word.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rv32_rows.hpp"

using namespace rv32;

static void finish(uint32_t* row, unsigned w) {
    for (unsigned c = 0; c < w; c++) row[c] = enc(row[c]);
}

// cs: 0 rv32i, 1 rv32i-cf, 2 rv32im.  trace: cycles x (pc, ins, a, b, res, next, wr); ecalls: n_ecalls x (cycle, a0 after);
// cpu: n rows, program: program_rows rows, muldiv: muldiv_rows rows (rv32im).  -> 0, or 1 ecall list / 2 pc range /
// 3 M result / 4 muldiv rows do not fit the trace
extern "C" int emul_rv32_shard(int cs, const uint32_t* trace, size_t cycles, size_t n, uint32_t end_pc, const uint32_t* init,
                               const uint32_t* ecalls, size_t n_ecalls, uint32_t pc_lo, size_t n_slots, size_t program_rows,
                               uint32_t* cpu, uint32_t* program, uint32_t* muldiv, size_t muldiv_rows) {
    const bool cf = cs >= CS_CF, im = cs == CS_IM;
    const unsigned cpu_w = im ? Chips<CS_IM>::cpu_w : cf ? Chips<CS_CF>::cpu_w : Chips<CS_I>::cpu_w;
    const unsigned prog_w = im ? Chips<CS_IM>::prog_w : cf ? Chips<CS_CF>::prog_w : Chips<CS_I>::prog_w;
    std::fill(cpu, cpu + n * cpu_w, 0u);
    std::fill(program, program + program_rows * prog_w, 0u);
    if (im) std::fill(muldiv, muldiv + muldiv_rows * MD_W, 0u);
    uint32_t last_ts[32] = {0}, last_val[32];
    std::copy(init, init + 32, last_val);
    std::vector<uint32_t> mult(n_slots, 0), word(n_slots, 0);
    size_t ec = 0, md = 0;
    for (size_t i = 0; i < n; i++) {
        uint32_t* row = cpu + i * cpu_w;
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
            if (cf) cpu_row_cf(row, r, d, m);
            if (im) cpu_row_im(row, d);
            if (im && d.is_m && d.wr) {
                if (md >= muldiv_rows) return 4;
                uint32_t* mrow = muldiv + md++ * MD_W;
                mrow[D_ONE] = 1;
                if (!muldiv_row(mrow, r, res)) return 3;
            }
            const size_t slot = (r.pc - pc_lo) >> 2;
            if (slot >= n_slots || (mult[slot] && word[slot] != r.ins)) return 2;
            mult[slot]++, word[slot] = r.ins;
        } else {
            trace_cells(padding_row(end_pc), false, row);
        }
        row[TSA] = tsa, row[TSB] = tsa + 1, row[TSW] = tsa + 2;
        finish(row, cpu_w);
    }
    for (size_t s = 0; s < program_rows; s++) {
        uint32_t* row = program + s * prog_w;
        const bool in = s < n_slots;
        const uint32_t pc = in ? pc_lo + 4 * (uint32_t)s : 0u, ins = in ? word[s] : 0u;
        const Dec d = decode(ins);
        program_row_i(row, pc, ins, d, in ? mult[s] : 0u);
        if (cf) program_row_cf(row, d);
        if (im) program_row_im(row, ins, d);
        finish(row, prog_w);
    }
    for (size_t k = 0; im && k < muldiv_rows; k++) {
        muldiv[k * MD_W + D_ONE] = 1;
        finish(muldiv + k * MD_W, MD_W);
    }
    return 0;
}
