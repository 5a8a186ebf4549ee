// The rows of the rv32 chip sets' tables (rv32i, rv32i-cf, rv32im, rv32im-elf, rv32im-mem) as lane bodies: one call fills one row with canonical
// values, on the GPU (rv32_kernels.hpp, rv32_kernels_mem.hpp, rv32_prep.hip: one lane per row, staged in LDS) and under plain g++ (tests/emul/emul_rv32_rows.cpp
// walks a trace through them against numpy).  raiko_amd/rv32.py, rv32cf.py and rv32im.py are the same in numpy and name
// every column; each chip set's rows are the previous one's with columns appended, so each row comes in pieces.  rv32im-elf
// (raiko_amd/rv32elf.py) is rv32im with the lookup tables' tuples preprocessed: its bodies (at the end) select those
// tuples from the full rows and find a pc's row in the program image.  rv32im-mem (raiko_amd/rv32mem.py) is rv32im-elf with
// nine cpu columns, six program fields and the memop and memory tables more (the last section).
#pragma once
#include <type_traits>

#include "bb.hpp"
#include "executor.hpp"

namespace rv32 {

constexpr unsigned CPU_W = RK_RV32_CPU_COLS, PROG_W = RK_RV32_PROGRAM_COLS, REG_W = RK_RV32_REGISTER_COLS,
                   BYTE_W = RK_RV32_BYTE_COLS, CF_CPU_W = RK_RV32CF_CPU_COLS, CF_PROG_W = RK_RV32CF_PROGRAM_COLS,
                   SHIFT_W = RK_RV32CF_SHIFT_COLS, SHIFT_USED = 9 * 256, IM_CPU_W = RK_RV32IM_CPU_COLS,
                   IM_PROG_W = RK_RV32IM_PROGRAM_COLS, MD_W = RK_RV32IM_MULDIV_COLS, MEM_CPU_W = RK_RV32MEM_CPU_COLS,
                   MO_W = RK_RV32MEM_MEMOP_COLS, BD_W = RK_RV32MEM_MEMORY_COLS, IO_CPU_W = RK_RV32IO_CPU_COLS,
                   IO_W = RK_RV32IO_IO_COLS, CM_MO_W = RK_RV32COMMIT_MEMOP_COLS, CM_IO_W = RK_RV32COMMIT_IO_COLS;
// the chip set a kernel writes, and what its rows are made of
enum ChipSet : int { CS_I, CS_CF, CS_IM, CS_ELF, CS_MEM, CS_IO, CS_COMMIT };
template <int CS>
struct Chips {
    // elf: rv32im's cpu, register and muldiv rows; the program, byte, range and shift traces are count columns
    // mem: rv32im-elf with nine cpu columns appended and the memop and memory tables
    // io: rv32im-mem with its ecalls bound to the input (raiko_amd/rv32io.py): seven cpu columns more and the io table
    // commit: the io form with the COMMIT journal bound (raiko_amd/rv32commit.py): a 65th memop column, 17 io columns more
    static constexpr bool cf = CS != CS_I, im = CS >= CS_IM, elf = CS >= CS_ELF, mem = CS >= CS_MEM, io = CS >= CS_IO,
                          commit = CS == CS_COMMIT;
    static constexpr unsigned cpu_w = io ? IO_CPU_W : mem ? MEM_CPU_W : im ? IM_CPU_W : cf ? CF_CPU_W : CPU_W,
                              prog_w = im ? IM_PROG_W : cf ? CF_PROG_W : PROG_W, mo_w = commit ? CM_MO_W : MO_W,
                              io_w = commit ? CM_IO_W : IO_W;
};

// ---- cpu columns
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
    IS_MUL = SHI + 4, IS_M = IS_MUL + 8, MOP, M_W,
    // rv32im-mem (raiko_amd/rv32mem.py): the six looked-up fields, the two multiplicities, the op of the ecall send
    IS_LOAD, IS_STORE, MEM_OP, MIMM_LO, MIMM_HI, IS_SYS, M_MEM, N_ECW, EC_OP,
    // the io form (raiko_amd/rv32io.py): the call number an ecall row reads from x5, the access before it, 5 IS_SYS, T0 = 0
    T0_LO, T0_HI, PT_TS, DT_LO, DT_HI, R5, T0Z
};
static_assert(ACTIVE + 1 == RK_TRACE_DATA_COLS, "the stand-in trace's columns come first");
static_assert(IS_JAL == CPU_W, "rv32i cpu columns");
static_assert(SHI + 4 == CF_CPU_W, "rv32i-cf cpu columns");
static_assert(M_W + 1 == IM_CPU_W, "rv32im cpu columns");
static_assert(EC_OP + 1 == MEM_CPU_W, "rv32im-mem cpu columns");
static_assert(T0Z + 1 == IO_CPU_W, "io cpu columns");
// ---- program columns: 0 .. P_MULT - 1 what a cpu row looks up (rv32.py PROGRAM_TUPLE), then the decoder's own; rv32i-cf
// appends its twelve fields at P_EXT, rv32im its nine at P_M and the funct7 test's three partial products at P_F7
enum : unsigned {
    P_MULT = 20, P_BITS, P_OPC = P_BITS + 32, P_F3 = P_OPC + 11, P_OPR = P_F3 + 8, P_Z1, P_Z2, P_RDZ, P_RD,
    P_EXT, P_M = P_EXT + 12, P_F7 = P_M + 9
};
static_assert(P_EXT == PROG_W && P_M == CF_PROG_W && P_F7 + 3 == IM_PROG_W, "program columns");
// ---- register, byte (ops AND = 1, OR = 2, XOR = 3) and shift columns
enum : unsigned { R_REG, R_ZERO, R_FTS, R_IL, R_IH = R_IL + 32, R_FL = R_IH + 32, R_FH = R_FL + 32 };
static_assert(R_FH + 32 == REG_W, "register columns");
enum : unsigned { Y_OP, Y_X, Y_Y, Y_Z, Y_XB, Y_YB = Y_XB + 8, Y_AND = Y_YB + 8, Y_OR, Y_XOR, Y_MULT };
static_assert(Y_MULT + 1 == BYTE_W, "byte columns");
enum : unsigned { H_K, H_X, H_LO, H_HI, H_MULT, H_XB, H_KS = H_XB + 8, H_VB = H_KS + 9 };
static_assert(H_VB + 16 == SHIFT_W, "shift columns");
// ---- rv32im: the muldiv table (rv32im.py muldiv_witness)
enum : unsigned {
    D_SEL, D_MULT = 8, D_OP, D_A_LO, D_A_HI, D_B_LO, D_B_HI, D_R_LO, D_R_HI, D_ONE, D_X, D_Y = D_X + 4, D_Z = D_Y + 4,
    D_C = D_Z + 4, D_CY = D_C + 8, D_S = D_CY + 8, D_L = D_S + 4, D_E = D_L + 4, D_AND = D_E + 4, D_BZ = D_AND + 8, D_BINV,
    D_OVF, D_OINV, D_BM_LO, D_BM_HI, D_KB, D_RM_LO, D_RM_HI, D_KR, D_DL_LO, D_DL_HI, D_K0
};
static_assert(D_K0 + 1 == MD_W, "rv32im muldiv columns");
// the byte pairs looked up as ANDs (rv32im.py BYTE_PAIRS), the limbs sent to RANGE16 (RANGE_COLS); the top bytes looked
// up in the shift table (SIGN_BYTES) are D_X + 3 + 4 j
constexpr unsigned MD_PAIRS[8][2] = {{D_X, D_X + 1}, {D_X + 2, D_Y}, {D_Y + 1, D_Y + 2}, {D_Z, D_Z + 1}, {D_Z + 2, D_C},
                                     {D_C + 1, D_C + 2}, {D_C + 4, D_C + 5}, {D_C + 6, D_C + 7}};
constexpr unsigned MD_RANGE[14] = {D_CY, D_CY + 1, D_CY + 2, D_CY + 3, D_CY + 4, D_CY + 5, D_CY + 6, D_CY + 7,
                                   D_BM_LO, D_BM_HI, D_RM_LO, D_RM_HI, D_DL_LO, D_DL_HI};

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
    // rv32im-mem: mimm = imm_I of a load, imm_S of a store; mem_ok = 0 for a LOAD / STORE word the executor traps
    uint32_t is_load, is_store, mem_op, mimm, is_sys, mem_ok;
};

RK_HD Dec decode(uint32_t ins) {
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
    d.is_load = d.opc == O_LOAD;
    d.is_store = d.opc == O_STORE;
    d.is_sys = d.opc == O_SYSTEM;
    d.mem_op = d.is_load ? d.f3 : d.is_store ? d.f3 + 8 : 0;
    d.mimm = d.is_load ? (uint32_t)((int32_t)ins >> 20) : d.is_store ? ((uint32_t)((int32_t)ins >> 25) << 5 | d.rd) : 0;
    d.mem_ok = !(d.is_load && (d.f3 == 3 || d.f3 > 5)) && !(d.is_store && d.f3 > 2);
    return d;
}

// the io key's reading of a word (rv32io.py): the ecall word reads a0 and a1
constexpr uint32_t ECALL_WORD = 0x00000073u;
RK_HD Dec decode_io(uint32_t ins) {
    Dec d = decode(ins);
    if (ins == ECALL_WORD) d.rs1 = 10, d.rs2 = 11;
    return d;
}

// the value a row writes: recomputed for the constrained ops, the side list's for an ecall, TraceRow.res otherwise
RK_HD uint32_t written(const Dec& d, const TraceRow& r, uint32_t ecall_a0) {
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

RK_HD uint32_t enc(uint32_t canon) { return bb::mul(canon, bb::R2); }

// the row past the executed cycles: stay where the segment ended
RK_HD TraceRow padding_row(uint32_t end_pc) {
    TraceRow r{};
    r.pc = r.next = end_pc;
    return r;
}

// the 16 cells of the stand-in trace circuit (include/raiko_hip.h), the first 16 of a cpu row: every 32-bit word as two
// 16-bit limbs; a row past the executed cycles (padding_row) has active = seq = 0
RK_HD void trace_cells(const TraceRow& r, bool active, uint32_t* c) {
    const uint32_t lo = r.pc & 0xffffu, carry = (active && lo + 4 > 0xffffu) ? 1u : 0u;
    const uint32_t seq = (active && r.next == r.pc + 4 && r.pc <= 0xfffffffbu) ? 1u : 0u;   // no wrap of the 32-bit pc
    c[PC_LO] = lo;
    c[PC_HI] = r.pc >> 16;
    c[NX_LO] = r.next & 0xffffu;
    c[NX_HI] = r.next >> 16;
    c[INS_LO] = r.ins & 0xffffu;
    c[INS_HI] = r.ins >> 16;
    c[SEQ] = seq;
    c[CARRY] = seq ? carry : 0u;
    c[A_LO] = r.a & 0xffffu;
    c[A_HI] = r.a >> 16;
    c[B_LO] = r.b & 0xffffu;
    c[B_HI] = r.b >> 16;
    c[RES_LO] = r.res & 0xffffu;
    c[RES_HI] = r.res >> 16;
    c[WR] = r.wr;
    c[ACTIVE] = active ? 1u : 0u;
}

// what an executed cpu row adds to the lookup tables' multiplicities beyond its unconditional sends
struct Mults {
    uint32_t is_slt = 0, bop = 0, ba = 0, bb = 0;   // SA_CHK / SB_CHK to RANGE16; the BYTE op (0: none) and its operands
    bool is_br = false, is_link = false, is_shift = false, m_sa = false, m_sb = false;   // rv32i-cf
};

// ---- the cpu row of an executed cycle; `row` is zero on entry.  res: the value the row writes (written); tsa: its first
// timestamp, 3 i + 1; pa / pb / pw: the timestamps of the accesses before its three (pw 0 without a write), pwv: the
// value the written register held
RK_HD void cpu_row_i(uint32_t* row, const TraceRow& r, const Dec& d, uint32_t res, uint32_t tsa, uint32_t pa, uint32_t pb,
                     uint32_t pw, uint32_t pwv, Mults& m) {
    const uint32_t ob = d.is_imm ? d.imm : r.b;
    const bool sublt = d.is_sub || d.is_slt || d.is_sltu;
    const uint32_t dd = sublt ? r.a - ob : 0;
    uint32_t x = 0, y = 0;
    if (d.is_add) x = r.a, y = ob;
    else if (d.is_auipc) x = r.pc, y = d.imm;
    else if (d.is_link) x = r.pc, y = 4;
    else if (sublt) x = dd, y = ob;
    const uint32_t c0 = ((x & 0xffffu) + (y & 0xffffu)) >> 16, c1 = ((x >> 16) + (y >> 16) + c0) >> 16;
    const uint32_t sa = r.a >> 31, sb = ob >> 31;
    const uint32_t da = tsa - pa - 1, db = tsa + 1 - pb - 1, dw = d.wr ? tsa + 2 - pw - 1 : 0;
    trace_cells(r, true, row);
    const uint32_t vals[][2] = {
        {RES_LO, res & 0xffffu}, {RES_HI, res >> 16}, {WR, d.wr},
        {RS1, d.rs1}, {RS2, d.rs2}, {WREG, d.wreg}, {IMM_LO, d.imm & 0xffffu}, {IMM_HI, d.imm >> 16},
        {IS_ADD, d.is_add}, {IS_SUB, d.is_sub}, {IS_SLT, d.is_slt}, {IS_SLTU, d.is_sltu}, {IS_BIT, d.is_bit},
        {BOP, d.bop}, {IS_IMM, d.is_imm}, {IS_LUI, d.is_lui}, {IS_AUIPC, d.is_auipc}, {IS_LINK, d.is_link},
        {PA_TS, pa}, {PB_TS, pb}, {PW_TS, pw}, {PW_LO, pwv & 0xffffu}, {PW_HI, pwv >> 16},
        {DA_LO, da & 0x3fffu}, {DA_HI, da >> 14}, {DB_LO, db & 0x3fffu}, {DB_HI, db >> 14},
        {DW_LO, dw & 0x3fffu}, {DW_HI, dw >> 14}, {OB_LO, ob & 0xffffu}, {OB_HI, ob >> 16}, {C0, c0}, {C1, c1},
        {D_LO, dd & 0xffffu}, {D_HI, dd >> 16}, {SA, sa}, {SB, sb}, {SNE, sa ^ sb},
        {SA_CHK, 2 * (r.a >> 16) - 65536 * sa}, {SB_CHK, 2 * (ob >> 16) - 65536 * sb}};
    for (const auto& kv : vals) row[kv[0]] = kv[1];
    m.is_slt = d.is_slt;
    if (d.is_bit) {
        m.bop = d.bop;
        m.ba = r.a;
        m.bb = ob;
        for (unsigned k = 0; k < 4; k++) {
            row[BA + k] = (r.a >> (8 * k)) & 255;
            row[BB + k] = (ob >> (8 * k)) & 255;
            row[BR + k] = (res >> (8 * k)) & 255;
        }
    }
}

// rv32i-cf (rv32cf.py cpu_rows): the branch decision, the next pc and the shift columns
RK_HD void cpu_row_cf(uint32_t* row, const TraceRow& r, const Dec& d, Mults& m) {
    const uint32_t a = r.a, b = r.b;
    // branch decision
    m.is_br = d.bsel >= 0;
    const bool eqv = a == b, ltu = a < b, lts = (int32_t)a < (int32_t)b;
    const bool cond[6] = {eqv, !eqv, lts, !lts, ltu, !ltu};
    const bool taken = m.is_br && cond[d.bsel];
    if (m.is_br) {
        const uint32_t dd = a - b, z = (dd & 0xffffu) + (dd >> 16);
        row[IS_BEQ + d.bsel] = 1;
        row[BD_LO] = dd & 0xffffu;
        row[BD_HI] = dd >> 16;
        row[BC0] = (a & 0xffffu) < (b & 0xffffu);
        row[BC1] = ltu;
        row[EQ] = eqv;
        row[INV] = z ? bb::decode(bb::inv(enc(z))) : 0u;
    }
    m.m_sb = d.bsel == 2 || d.bsel == 3;
    m.m_sa = m.m_sb || d.is_sra;
    row[IS_BR] = m.is_br;
    row[TAKEN] = taken;
    row[M_SA] = m.m_sa;
    row[M_SB] = m.m_sb;
    // next pc = base + offset (mod 2^32), JALR's low bit dropped
    const bool jalr = d.opc == O_JALR;
    m.is_link = d.is_link;
    const uint32_t base = jalr ? a : r.pc, off = jalr ? d.imm : (taken || d.is_jal) ? d.jimm : 4u;
    const uint32_t nc0 = ((base & 0xffffu) + (off & 0xffffu)) >> 16, nc1 = ((base >> 16) + (off >> 16) + nc0) >> 16;
    row[IS_JAL] = d.is_jal;
    row[JIMM_LO] = d.jimm & 0xffffu;
    row[JIMM_HI] = d.jimm >> 16;
    row[NC0] = nc0;
    row[NC1] = nc1;
    row[DROP] = jalr ? (base + off) & 1u : 0u;
    row[NXH] = m.is_link ? (r.next & 0xffffu) >> 1 : 0u;
    // shifts: s = k + 8 q; the bytes of a' (a, complemented for SRA of a negative a) through the shift table
    row[IS_SLL] = d.is_sll;
    row[IS_SRL] = d.is_srl;
    row[IS_SRA] = d.is_sra;
    m.is_shift = d.is_sll || d.is_srl || d.is_sra;
    if (m.is_shift) {
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

// rv32im (rv32im.py cpu_rows): the M selectors; M_W = 1 sends the row to the muldiv table
RK_HD void cpu_row_im(uint32_t* row, const Dec& d) {
    if (d.is_m) {
        row[IS_MUL + d.f3] = 1;
        row[IS_M] = 1;
        row[MOP] = d.f3;
        row[M_W] = d.wr;
    }
}

// ---- the program row of instruction word `ins` at `pc`, executed `mult` times; `row` is zero on entry
RK_HD void program_row_i(uint32_t* row, uint32_t pc, uint32_t ins, const Dec& d, uint32_t mult) {
    const uint32_t v[P_MULT] = {pc & 0xffffu, pc >> 16, ins & 0xffffu, ins >> 16, d.rs1, d.rs2, d.wreg, d.imm & 0xffffu,
                                d.imm >> 16, d.is_add, d.is_sub, d.is_slt, d.is_sltu, d.is_bit, d.bop, d.is_imm,
                                d.is_lui, d.is_auipc, d.is_link, d.wr};
    for (unsigned c = 0; c < P_MULT; c++) row[c] = v[c];
    row[P_MULT] = mult;
    for (unsigned k = 0; k < 32; k++) row[P_BITS + k] = (ins >> k) & 1;
    if (d.opc >= 0) {
        row[P_OPC + d.opc] = 1;
        row[P_F3 + d.f3] = 1;
    }
    const uint32_t b = ins >> 7;
    const uint32_t z1 = (~b & 1) & (~b >> 1 & 1), z2 = z1 & (~b >> 2 & 1), rdz = z2 & (~b >> 3 & 1) & (~b >> 4 & 1);
    row[P_OPR] = d.opr;
    row[P_Z1] = z1;
    row[P_Z2] = z2;
    row[P_RDZ] = rdz;
    row[P_RD] = d.rd;
}

// rv32i-cf: the twelve fields the cf cpu row looks up
RK_HD void program_row_cf(uint32_t* row, const Dec& d) {
    uint32_t* e = row + P_EXT - IS_JAL;     // e[c]: the field of cpu column c
    e[IS_JAL] = d.is_jal;
    if (d.bsel >= 0) e[IS_BEQ + d.bsel] = 1;
    e[JIMM_LO] = d.jimm & 0xffffu;
    e[JIMM_HI] = d.jimm >> 16;
    e[IS_SLL] = d.is_sll;
    e[IS_SRL] = d.is_srl;
    e[IS_SRA] = d.is_sra;
}

// rv32im: IS_MUL .. IS_REMU and IS_M, then the funct7 test's partial products op b25 !b26, !b27 !b28, !b29 !b30
RK_HD void program_row_im(uint32_t* row, uint32_t ins, const Dec& d) {
    const auto nb = [&](unsigned k) { return ((ins >> k) & 1u) ^ 1u; };
    const uint32_t f7a = (d.opc == O_OP) & (ins >> 25) & 1u & nb(26), f7b = f7a & nb(27) & nb(28), f7c = f7b & nb(29) & nb(30);
    if (d.is_m) row[P_M + d.f3] = 1;
    row[P_M + IS_M - IS_MUL] = d.is_m;
    row[P_F7] = f7a;
    row[P_F7 + 1] = f7b;
    row[P_F7 + 2] = f7c;
}

// ---- row r of the rv32i-cf shift table (rv32cf.py shift_rows): row k 256 + x = (k, x, x 2^k mod 256, x 2^k / 256, count,
// bits of x, k one-hot, bits of x 2^k); rows past 9 x 256 the true tuple (0, 0, 0, 0) with count 0
RK_HD void shift_row(uint32_t* row, size_t r, uint32_t mult) {
    const uint32_t k = r < SHIFT_USED ? (uint32_t)(r >> 8) : 0u, x = r < SHIFT_USED ? (uint32_t)(r & 255) : 0u, v = x << k;
    row[H_K] = k;
    row[H_X] = x;
    row[H_LO] = v & 255u;
    row[H_HI] = v >> 8;
    row[H_MULT] = mult;
    for (unsigned bit = 0; bit < 8; bit++) row[H_XB + bit] = (x >> bit) & 1u;
    row[H_KS + k] = 1;
    for (unsigned bit = 0; bit < 16; bit++) row[H_VB + bit] = (v >> bit) & 1u;
}

// ---- row r < 3 x 2^16 of the byte table (rv32.py byte_rows): (op, x, y) = (r >> 16) + 1, byte 1 of r, byte 0 of r
RK_HD void byte_row(uint32_t* row, size_t r, uint32_t mult) {
    const uint32_t op = (uint32_t)(r >> 16) + 1, x = (r >> 8) & 255, y = r & 255;
    row[Y_OP] = op;
    row[Y_X] = x;
    row[Y_Y] = y;
    row[Y_Z] = op == 1 ? (x & y) : op == 2 ? (x | y) : (x ^ y);
    for (unsigned k = 0; k < 8; k++) {
        row[Y_XB + k] = (x >> k) & 1;
        row[Y_YB + k] = (y >> k) & 1;
    }
    row[Y_AND + op - 1] = 1;
    row[Y_MULT] = mult;
}

// ---- row r of the register table (rv32.py register_rows): init / fin are the 32 registers at the shard's start and end
RK_HD void register_row(uint32_t* row, unsigned r, uint32_t final_ts, const uint32_t* init, const uint32_t* fin) {
    row[R_REG] = r;
    row[R_ZERO] = 0;
    row[R_FTS] = final_ts;
    for (unsigned j = 0; j < 32; j++) {
        const bool in = r + j < 32;
        row[R_IL + j] = in ? init[r + j] & 0xffffu : 0;
        row[R_IH + j] = in ? init[r + j] >> 16 : 0;
        row[R_FL + j] = in ? fin[r + j] & 0xffffu : 0;
        row[R_FH + j] = in ? fin[r + j] >> 16 : 0;
    }
}

// ---- the muldiv row of M cycle r writing res: the witness of the op on its 32-bit operands (64-bit products and the
// division's quotient / remainder, the executor's conventions); `row` is zero on entry but for D_ONE.  -> whether res is
// the op's result
RK_HD bool muldiv_row(uint32_t* row, const TraceRow& r, uint32_t res) {
    const uint32_t op = (r.ins >> 12) & 7, a = r.a, b = r.b;
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
    return want == res;
}

// ---- rv32im-elf (rv32elf.py): the preprocessed rows are the tuple columns of the full rows above
constexpr unsigned ELF_PROG_W = RK_RV32ELF_PROGRAM_PREP_COLS, ELF_TUPLE_W = 4, ELF_VALID = ELF_PROG_W - 1;
static_assert(P_MULT + 12 + 9 + 1 == ELF_PROG_W, "rv32im-elf program columns: the 41 looked-up fields, then VALID");

// the program image: up to RK_RV32ELF_MAX_SEGMENTS runs of words; row = the words before the segment + the word's index
struct Image {
    uint32_t n_segs;
    uint32_t vaddr[RK_RV32ELF_MAX_SEGMENTS], words[RK_RV32ELF_MAX_SEGMENTS];
};
constexpr uint32_t NO_ROW = 0xffffffffu;
// the image row of pc, NO_ROW for a pc outside every segment or not word-aligned
RK_HD uint32_t image_row(const Image& im, uint32_t pc) {
    uint32_t row = NO_ROW, before = 0;
    for (uint32_t k = 0; k < RK_RV32ELF_MAX_SEGMENTS; k++) {
        if (k < im.n_segs) {
            const uint32_t off = pc - im.vaddr[k];
            if (pc >= im.vaddr[k] && (off & 3u) == 0 && (off >> 2) < im.words[k]) row = before + (off >> 2);
            before += im.words[k];
        }
    }
    return row;
}
// the pc of image row s < the image's words
RK_HD uint32_t image_pc(const Image& im, uint32_t s) {
    uint32_t pc = 0, before = 0;
    for (uint32_t k = 0; k < RK_RV32ELF_MAX_SEGMENTS; k++) {
        if (k < im.n_segs) {
            if (s >= before && s - before < im.words[k]) pc = im.vaddr[k] + 4 * (s - before);
            before += im.words[k];
        }
    }
    return pc;
}
// full: an rv32im program row (program_row_i / _cf / _im) -> its 41 looked-up fields and VALID: one opcode class, and
// not an OP word with bit 25 set that is no M word (rv32im.program_air's test on a looked-up row)
RK_HD void program_prep_row(uint32_t* out, const uint32_t* full) {
    for (unsigned c = 0; c < P_MULT; c++) out[c] = full[c];
    for (unsigned c = 0; c < 12; c++) out[P_MULT + c] = full[P_EXT + c];
    for (unsigned c = 0; c < 9; c++) out[P_MULT + 12 + c] = full[P_M + c];
    uint32_t s = 0;
    for (unsigned k = 0; k < 11; k++) s += full[P_OPC + k];
    out[ELF_VALID] = s * (1u - (full[P_OPC + O_OP] * full[P_BITS + 25] - full[P_M + 8]));
}
RK_HD void byte_prep_row(uint32_t* out, const uint32_t* full) {
    out[0] = full[Y_OP], out[1] = full[Y_X], out[2] = full[Y_Y], out[3] = full[Y_Z];
}
RK_HD void shift_prep_row(uint32_t* out, const uint32_t* full) {
    out[0] = full[H_K], out[1] = full[H_X], out[2] = full[H_LO], out[3] = full[H_HI];
}

// ---- rv32im-mem (rv32mem.py): the nine appended cpu columns, the 48-column program selection, the memop and memory rows
constexpr unsigned MEM_PROG_W = RK_RV32MEM_PROGRAM_PREP_COLS, MEM_VALID = MEM_PROG_W - 1, EC_CODE = 16;
static_assert(ELF_VALID + 6 == MEM_VALID, "rv32im-mem program columns: rv32im-elf's 41 fields, six more, then VALID");
enum : unsigned {
    G_SEL, G_MULT = 9, G_OP, G_TS, G_A_LO, G_A_HI, G_MI_LO, G_MI_HI, G_B_LO, G_B_HI, G_R_LO, G_R_HI, G_AD_LO, G_AD_HI, G_K0, G_K1,
    G_WL, G_WL4, G_O0, G_O1, G_S, G_W = G_S + 4, G_N = G_W + 4, G_BB = G_N + 4, G_X = G_BB + 4, G_H0, G_H1, G_TOP, G_SG, G_SL,
    G_ONE, G_AND, G_PTS = G_AND + 6, G_DL, G_DH, G_W_LO, G_W_HI, G_N_LO, G_N_HI
};
static_assert(G_N_HI + 1 == MO_W, "rv32im-mem memop columns");
// the commit form (rv32commit.py): a tenth row kind, ECR, whose selector is a 65th column
constexpr unsigned G_ECR = MO_W, ECR_CODE = RK_RV32COMMIT_ECR_CODE;
static_assert(G_ECR + 1 == CM_MO_W, "commit memop columns");
enum : unsigned { B_WL, B_WH, B_I_LO, B_I_HI, B_F_LO, B_F_HI, B_FTS, B_REAL, B_GL, B_GH, B_WL4, B_SAME, B_FINV };
static_assert(B_FINV + 1 == BD_W, "rv32im-mem memory columns");
// the limbs a real memory row sends to RANGE16 (rv32mem.py MEMORY_RANGE)
constexpr unsigned BD_RANGE[5] = {B_GL, B_GH, B_WL, B_WL4, B_WH};
// the byte pairs looked up as ANDs (rv32mem.py BYTE_PAIRS) are G_W + 2 j, G_W + 2 j + 1 for j < 6 (W, N, BB are adjacent);
// the limbs sent to RANGE16 (RANGE_COLS)
static_assert(G_N == G_W + 4 && G_BB == G_W + 8, "the twelve bytes are adjacent");
constexpr unsigned MO_RANGE[6] = {G_AD_LO, G_AD_HI, G_WL, G_WL4, G_DL, G_DH};

// one entry of the executor's access list (ExecSegmentView.mem)
struct MemAccess {
    uint32_t cycle, waddr, before, after;
};

// the cpu columns past rv32im's, after cpu_row_i has set WR; n_ecw: the list's entries at this cycle (an ecall row's)
RK_HD void cpu_row_mem(uint32_t* row, const Dec& d, uint32_t n_ecw) {
    row[IS_LOAD] = d.is_load;
    row[IS_STORE] = d.is_store;
    row[MEM_OP] = d.mem_op;
    row[MIMM_LO] = d.mimm & 0xffffu;
    row[MIMM_HI] = d.mimm >> 16;
    row[IS_SYS] = d.is_sys;
    row[M_MEM] = d.is_load * row[WR] + d.is_store;
    row[N_ECW] = d.is_sys ? n_ecw : 0u;
    row[EC_OP] = EC_CODE * d.is_sys;
}

// the io form's cpu columns, after cpu_row_mem: the send to memop is gone (N_ECW = EC_OP = 0); an ecall row reads t0 from
// x5 at tsa, after the access at pt
RK_HD void cpu_row_io(uint32_t* row, const Dec& d, uint32_t t0, uint32_t tsa, uint32_t pt) {
    row[N_ECW] = 0;
    row[EC_OP] = 0;
    if (!d.is_sys) return;
    const uint32_t gap = tsa - pt - 1;
    row[T0_LO] = t0 & 0xffffu;
    row[T0_HI] = t0 >> 16;
    row[PT_TS] = pt;
    row[DT_LO] = gap & 0x3fffu;
    row[DT_HI] = gap >> 14;
    row[R5] = 5;
    row[T0Z] = t0 == 0;
}

// full: an rv32im program row of word `ins` -> rv32im-elf's 41 fields, the six of rv32im-mem, VALID
RK_HD void program_prep_row_mem(uint32_t* out, const uint32_t* full, const Dec& d) {
    uint32_t elf[ELF_PROG_W];
    program_prep_row(elf, full);
    for (unsigned c = 0; c < ELF_VALID; c++) out[c] = elf[c];
    const uint32_t f[6] = {d.is_load, d.is_store, d.mem_op, d.mimm & 0xffffu, d.mimm >> 16, d.is_sys};
    for (unsigned c = 0; c < 6; c++) out[ELF_VALID + c] = f[c];
    out[MEM_VALID] = elf[ELF_VALID] * d.mem_ok;
}
// the io key: the ecall word's tuple reads a0 and a1 (RS1, RS2 are tuple cells 4 and 5)
RK_HD void program_prep_row_io(uint32_t* out, const uint32_t* full, const Dec& d) {
    program_prep_row_mem(out, full, d);
    if ((full[2] | full[3] << 16) == ECALL_WORD) out[4] = 10, out[5] = 11;
}

// ---- the memop row of access m, made by the cycle r (decoded d) that claims res; pts: the timestamp of the access before
// it at its word (0: none); `row` is zero on entry but for G_ONE.  -> whether the access is the one the instruction names:
// its address, the loaded value, the stored word
// io (rv32io.py): an ECW row is written as the store of the word it leaves -- A its address, B and BB the word
// commit (rv32commit.py; the io form's trace, whose ecall rows hold t0 in res): an access at a COMMIT row is an ECR row,
// LW's witness of the word it reads -- A its address, R the word; `row` has CM_MO_W cells then
RK_HD bool memop_row(uint32_t* row, const MemAccess& m, const TraceRow& r, const Dec& d, uint32_t res, uint32_t pts, bool io = false,
                     bool commit = false) {
    const bool ecw = d.is_sys, ecr = ecw && commit && r.res == 2;
    const uint32_t op = ecr ? ECR_CODE : ecw ? EC_CODE : d.mem_op, f3 = op & 3u;
    const unsigned sel = ecr ? G_ECR : ecw ? 8u : d.is_store ? 5u + f3 : op < 4 ? op : op - 1;
    const uint32_t a = ecw ? (io ? m.waddr << 2 : 0u) : r.a, mi = ecw ? 0u : d.mimm, b = ecr ? 0u : ecw ? (io ? m.after : 0u) : r.b,
                   rs = ecr ? m.before : ecw ? 0u : res;
    const uint32_t ad = ecw ? m.waddr << 2 : a + mi;
    const uint32_t k0 = ((a & 0xffffu) + (mi & 0xffffu)) >> 16, k1 = ((a >> 16) + (mi >> 16) + k0) >> 16;
    const uint32_t o0 = ad & 1u, o1 = (ad >> 1) & 1u, wl = (ad & 0xffffu) >> 2, off = ad & 3u, ts = 3 * m.cycle + 1;
    row[G_SEL + sel] = 1;
    const uint32_t vals[][2] = {
        {G_MULT, 1}, {G_OP, op}, {G_TS, ts}, {G_A_LO, a & 0xffffu}, {G_A_HI, a >> 16}, {G_MI_LO, mi & 0xffffu}, {G_MI_HI, mi >> 16},
        {G_B_LO, b & 0xffffu}, {G_B_HI, b >> 16}, {G_R_LO, rs & 0xffffu}, {G_R_HI, rs >> 16}, {G_AD_LO, ad & 0xffffu},
        {G_AD_HI, ad >> 16}, {G_K0, k0}, {G_K1, k1}, {G_WL, wl}, {G_WL4, 4 * wl}, {G_O0, o0}, {G_O1, o1},
        {G_W_LO, m.before & 0xffffu}, {G_W_HI, m.before >> 16}, {G_N_LO, m.after & 0xffffu}, {G_N_HI, m.after >> 16},
        {G_PTS, pts}, {G_DL, (ts - pts - 1) & 0x3fffu}, {G_DH, (ts - pts - 1) >> 14}};
    for (const auto& kv : vals) row[kv[0]] = kv[1];
    row[G_S + off] = 1;
    const bool store = ecw ? io && !ecr : d.is_store;
    for (unsigned k = 0; k < 4; k++) {
        row[G_W + k] = (m.before >> (8 * k)) & 255u;
        row[G_N + k] = (m.after >> (8 * k)) & 255u;
        row[G_BB + k] = store ? (b >> (8 * k)) & 255u : 0u;
    }
    const uint32_t x = row[G_W + off], h0 = row[G_W + 2 * o1], h1 = row[G_W + 2 * o1 + 1];
    const uint32_t top = sel == 0 ? x : sel == 1 ? h1 : 0u;
    row[G_X] = x;
    row[G_H0] = h0;
    row[G_H1] = h1;
    row[G_TOP] = top;
    row[G_SG] = top >> 7;
    row[G_SL] = (2 * top) & 255u;
    for (unsigned j = 0; j < 6; j++) row[G_AND + j] = row[G_W + 2 * j] & row[G_W + 2 * j + 1];
    // what the instruction names
    if (ecw) return !ecr || m.before == m.after;
    const uint32_t half = h0 | h1 << 8, sh = 8 * off;
    uint32_t want_res = 0, want_after = m.before;
    switch (sel) {
        case 0: want_res = (uint32_t)(int32_t)(int8_t)x; break;
        case 1: want_res = (uint32_t)(int32_t)(int16_t)half; break;
        case 2: want_res = m.before; break;
        case 3: want_res = x; break;
        case 4: want_res = half; break;
        case 5: want_after = (m.before & ~(0xffu << sh)) | (b & 0xffu) << sh; break;
        case 6: want_after = (m.before & ~(0xffffu << sh)) | (b & 0xffffu) << sh; break;
        default: want_after = b; break;
    }
    return (ad >> 2) == m.waddr && want_after == m.after && (store || want_res == rs);
}

// ---- a memory (boundary) row: the word at waddr went from init to fin, last touched at fts (not 0); next: the next
// row's word address (has_next: there is one), larger than waddr: the distance is written limb by limb -- SAME and GL
// when the high limbs agree, GH otherwise
RK_HD void memory_row(uint32_t* row, uint32_t waddr, uint32_t init, uint32_t fin, uint32_t fts, bool has_next, uint32_t next) {
    const uint32_t wl = waddr & 0x3fffu, wh = waddr >> 14, nl = next & 0x3fffu, nh = next >> 14;
    const bool same = has_next && nh == wh;
    row[B_WL] = wl;
    row[B_WH] = wh;
    row[B_I_LO] = init & 0xffffu;
    row[B_I_HI] = init >> 16;
    row[B_F_LO] = fin & 0xffffu;
    row[B_F_HI] = fin >> 16;
    row[B_FTS] = fts;
    row[B_REAL] = 1;
    row[B_GL] = same ? nl - wl - 1 : 0u;
    row[B_GH] = has_next && !same ? nh - wh - 1 : 0u;
    row[B_WL4] = 4 * wl;
    row[B_SAME] = same;
    row[B_FINV] = bb::decode(bb::inv(enc(fts)));
}

// ---- what the witness needs of an access list against the trace it belongs to: cycle order, every entry at a load that
// writes rd, at a store or at the ecall word, exactly one entry at each of the first two, word addresses below 2^30.
// Host code (the shard driver refuses a list that fails it before anything is launched)
inline bool mem_list_ok(const TraceRow* tr, size_t cycles, const MemAccess* acc, size_t count) {
    auto kind = [](uint32_t ins) {   // 1: a load into a register other than x0, or a store; 2: the ecall word
        const uint32_t opc = ins & 0x7fu;
        return (opc == 0x03 && (ins & 0xf80u)) || opc == 0x23 ? 1 : opc == 0x73 ? 2 : 0;
    };
    size_t want = 0, got = 0;
    for (size_t i = 0; i < cycles; i++) want += kind(tr[i].ins) == 1;
    for (size_t k = 0; k < count; k++) {
        const MemAccess& m = acc[k];
        if (m.cycle >= cycles || (k && m.cycle < acc[k - 1].cycle) || m.waddr >= (1u << 30)) return false;
        const int kd = kind(tr[m.cycle].ins);
        if (kd == 0 || (kd == 1 && k && m.cycle == acc[k - 1].cycle)) return false;
        got += kd == 1;
    }
    return want == got;
}

// ---- the io table (rv32io.py io_rows): one head row per ecall, one word row per word a READ stores, padding
enum : unsigned {
    Q_HEAD, Q_WORD, Q_ACT, Q_HALT, Q_READ, Q_COMMIT, Q_TS, Q_T0, Q_ZERO, Q_OP16, Q_AD_LO, Q_AD_HI, Q_AQ, Q_K, Q_K1, Q_B_LO, Q_B_HI,
    Q_RES_LO, Q_RES_HI, Q_RH4, Q_REM, Q_Z, Q_RINV, Q_POS, Q_PL, Q_PL4, Q_PH, Q_NL, Q_NL4, Q_NH, Q_GL, Q_GL4, Q_GH, Q_EL, Q_EL4, Q_EH,
    Q_C, Q_FLO, Q_FHI, Q_KF, Q_ZC, Q_ZR, Q_V_LO, Q_V_HI, Q_GAP_L, Q_GAP_H, Q_HSEEN
};
static_assert(Q_HSEEN + 1 == IO_W, "io columns");
// the limbs sent to RANGE16 (rv32io.py IO_RANGE): by every active row, by a READ head, by a head, by a word row
constexpr unsigned IO_RANGE_ACT[6] = {Q_AD_LO, Q_AD_HI, Q_AQ, Q_PL, Q_PL4, Q_PH};
constexpr unsigned IO_RANGE_READ[12] = {Q_RH4, Q_NL, Q_NL4, Q_NH, Q_GL, Q_GL4, Q_GH, Q_EL, Q_EL4, Q_EH, Q_FLO, Q_FHI};
constexpr unsigned IO_RANGE_HEAD[2] = {Q_GAP_L, Q_GAP_H}, IO_RANGE_WORD[2] = {Q_V_LO, Q_V_HI};

// one entry of the executor's ecall side list (ExecSegmentView.ecall_args)
struct EcallArg {
    uint32_t cycle, t0, a0, a1, pos;
};

// the position limbs and what every row derives from its own cells
RK_HD void io_row_tail(uint32_t* row, uint32_t pos, bool active, uint32_t hseen) {
    row[Q_POS] = pos;
    if (active) {
        row[Q_PL] = pos & 0x3fffu;
        row[Q_PH] = pos >> 14;
    }
    row[Q_PL4] = 4 * row[Q_PL];
    row[Q_NL4] = 4 * row[Q_NL];
    row[Q_GL4] = 4 * row[Q_GL];
    row[Q_EL4] = 4 * row[Q_EL];
    row[Q_RH4] = 4 * row[Q_RES_HI];
    row[Q_Z] = row[Q_REM] == 0;
    row[Q_RINV] = row[Q_REM] ? bb::decode(bb::inv(enc(row[Q_REM]))) : 0u;
    row[Q_HSEEN] = hseen;
}

// the head row of ecall e that left res in a0 and stored `got` words; prev_ts: the timestamp of the head before it
// (has_prev).  `row` is zero on entry.  -> whether the call is what the executor's table does with these arguments
RK_HD bool io_head_row(uint32_t* row, const EcallArg& e, uint32_t res, uint32_t got, uint32_t n_input, bool has_prev, uint32_t prev_ts) {
    const uint32_t ts = 3 * e.cycle + 1, gap = has_prev ? ts - prev_ts - 1 : 0u;
    const uint32_t t0 = e.t0 < 3 ? e.t0 : 0u;
    row[Q_HEAD] = row[Q_ACT] = 1;
    row[Q_HALT + t0] = 1;
    row[Q_TS] = ts;
    row[Q_T0] = t0;
    row[Q_AD_LO] = e.a0 & 0xffffu;
    row[Q_AD_HI] = e.a0 >> 16;
    row[Q_B_LO] = e.a1 & 0xffffu;
    row[Q_B_HI] = e.a1 >> 16;
    row[Q_RES_LO] = res & 0xffffu;
    row[Q_RES_HI] = res >> 16;
    row[Q_GAP_L] = gap & 0x3fffu;
    row[Q_GAP_H] = gap >> 14;
    if (e.t0 != 1) return e.t0 < 3 && res == e.a0 && got == 0;
    const uint32_t left = n_input - e.pos, f = e.a1 - got, x = left - got;
    row[Q_AQ] = (e.a0 & 0xffffu) >> 2;
    row[Q_REM] = got;
    row[Q_NL] = n_input & 0x3fffu;
    row[Q_NH] = n_input >> 14;
    row[Q_GL] = got & 0x3fffu;
    row[Q_GH] = got >> 14;
    row[Q_EL] = x & 0x3fffu;
    row[Q_EH] = x >> 14;
    row[Q_C] = ((e.pos & 0x3fffu) + (got & 0x3fffu) + (x & 0x3fffu)) >> 14;
    row[Q_FLO] = f & 0xffffu;
    row[Q_FHI] = f >> 16;
    row[Q_KF] = ((got & 0xffffu) + (f & 0xffffu)) >> 16;
    row[Q_ZC] = f == 0;
    row[Q_ZR] = x == 0;
    return e.pos <= n_input && got == (e.a1 < left ? e.a1 : left) && res == got && (e.a0 & 3u) == 0;
}

// word row k < got of READ e: the access m it stored.  -> whether m is word k of the call
RK_HD bool io_word_row(uint32_t* row, const EcallArg& e, uint32_t got, uint32_t k, const MemAccess& m) {
    const uint32_t ad = e.a0 + 4 * k, before = ad - 4;
    row[Q_WORD] = row[Q_ACT] = 1;
    row[Q_TS] = 3 * e.cycle + 1;
    row[Q_OP16] = EC_CODE;
    row[Q_AD_LO] = ad & 0xffffu;
    row[Q_AD_HI] = ad >> 16;
    row[Q_AQ] = (ad & 0xffffu) >> 2;
    if (k) {
        row[Q_K] = ((before & 0xffffu) + 4) >> 16;
        row[Q_K1] = ((before >> 16) + row[Q_K]) >> 16;
    }
    row[Q_REM] = got - 1 - k;
    row[Q_V_LO] = m.after & 0xffffu;
    row[Q_V_HI] = m.after >> 16;
    return m.cycle == e.cycle && m.waddr == ad >> 2;
}

// ---- what the io witness needs of the side list against the trace: one entry per ecall row, in cycle order.  Host code
// (the shard driver refuses a list that fails it before anything is launched)
inline bool io_list_ok(const TraceRow* tr, size_t cycles, const EcallArg* args, size_t count) {
    size_t want = 0;
    for (size_t i = 0; i < cycles; i++) want += tr[i].ins == ECALL_WORD;
    for (size_t k = 0; k < count; k++)
        if (args[k].cycle >= cycles || (k && args[k].cycle <= args[k - 1].cycle) || tr[args[k].cycle].ins != ECALL_WORD) return false;
    return want == count;
}

// ---- the commit form (rv32commit.py): the io table's 17 columns more, the commit-word rows after a COMMIT head
enum : unsigned { Q_CW = IO_W, Q_S, Q_S0, Q_S1, Q_CNT, Q_C0, Q_C1, Q_T0B, Q_T1B, Q_BH7, Q_RML, Q_RMH, Q_RMH7, Q_JPOS, Q_JL, Q_JL4, Q_JH };
static_assert(Q_JH + 1 == CM_IO_W, "commit io columns");
// the limbs sent to RANGE16 beside the io form's (rv32commit.py IO_RANGE): by a COMMIT head, by a commit-word row
constexpr unsigned IO_RANGE_COMMIT[1] = {Q_BH7}, IO_RANGE_CW[6] = {Q_RML, Q_RMH, Q_RMH7, Q_JL, Q_JL4, Q_JH};
constexpr uint32_t MAX_COMMIT = 1u << 25, MAX_JOURNAL = 1u << 30;

// the words a COMMIT of a1 bytes from a0 reads
RK_HD uint32_t commit_words(uint32_t a0, uint32_t a1) { return a1 ? ((a0 & 3u) + a1 + 3u) >> 2 : 0u; }

// after io_head_row(..., got = 0 for a COMMIT): the byte countdown starts at a1.  n_reads: the commit reads at the call's
// cycle.  -> whether they are as many as the call's words and a1 is below 2^25
RK_HD bool io_commit_head(uint32_t* row, const EcallArg& e, uint32_t n_reads) {
    if (e.t0 != 2) return true;
    row[Q_REM] = e.a1;
    return n_reads == commit_words(e.a0, e.a1) && e.a1 < MAX_COMMIT;
}

// ... with jpos, the journal offset the call's first byte lands at: also whether the journal ends below 2^30 bytes after
// the call (rv32commit.py io_rows: JH stays a 16-bit limb).  What the witness calls
RK_HD bool io_commit_head(uint32_t* row, const EcallArg& e, uint32_t n_reads, uint32_t jpos) {
    if (!io_commit_head(row, e, n_reads)) return false;
    return e.t0 != 2 || (jpos < MAX_JOURNAL && e.a1 < MAX_JOURNAL - jpos);
}

// commit-word row k of COMMIT e, whose first byte lands at journal offset jpos; m: the commit read it answers; `row` is
// zero on entry.  In closed form from (a0, a1, k): row 0 starts at byte a0 & 3 of its word, every later one at byte 0, each
// takes bytes to its word's end or as many as are left.  -> whether m is word k of the call
RK_HD bool io_commit_row(uint32_t* row, const EcallArg& e, uint32_t k, uint32_t jpos, const MemAccess& m) {
    const uint32_t off = e.a0 & 3u, s = k ? 0u : off, taken = k ? 4 * k - off : 0u, before_left = e.a1 - taken;
    const uint32_t cnt = before_left < 4 - s ? before_left : 4 - s, left = before_left - cnt, t = 4 - s - cnt;
    const uint32_t ad = (e.a0 & ~3u) + 4 * k, before = ad - 4, jp = jpos + taken;
    row[Q_CW] = row[Q_ACT] = 1;
    row[Q_TS] = 3 * e.cycle + 1;
    row[Q_OP16] = ECR_CODE;
    row[Q_AD_LO] = ad & 0xffffu;
    row[Q_AD_HI] = ad >> 16;
    row[Q_AQ] = (ad & 0xffffu) >> 2;
    if (k) {
        row[Q_K] = ((before & 0xffffu) + 4) >> 16;
        row[Q_K1] = ((before >> 16) + row[Q_K]) >> 16;
    }
    row[Q_REM] = left;
    row[Q_RML] = left & 0xffffu;
    row[Q_RMH] = left >> 16;
    row[Q_S] = s;
    row[Q_S0] = s & 1u;
    row[Q_S1] = s >> 1;
    row[Q_CNT] = cnt;
    row[Q_C0] = (cnt - 1) & 1u;
    row[Q_C1] = (cnt - 1) >> 1;
    row[Q_T0B] = t & 1u;
    row[Q_T1B] = t >> 1;
    row[Q_V_LO] = m.before & 0xffffu;
    row[Q_V_HI] = m.before >> 16;
    row[Q_JL] = jp & 0x3fffu;
    row[Q_JH] = jp >> 14;
    return m.cycle == e.cycle && m.waddr == ad >> 2 && m.before == m.after && taken < e.a1;
}

// the journal position of a row (a commit-word row: where its bytes land) and what every row derives from its own cells,
// beside io_row_tail
RK_HD void io_commit_tail(uint32_t* row, uint32_t jpos) {
    row[Q_JPOS] = jpos;
    row[Q_BH7] = 128 * row[Q_B_HI];
    row[Q_RMH7] = 128 * row[Q_RMH];
    row[Q_JL4] = 4 * row[Q_JL];
}

// ---- what the commit witness needs of the commit reads against the side list and the access list: per COMMIT of the side
// list, in cycle order, the words (a0 & ~3) / 4 + k for k < commit_words, each read unchanged, and nothing else; no COMMIT
// of 2^25 bytes and more; no entry of the access list at a COMMIT's cycle.  Host code (the shard driver refuses lists that
// fail it before anything is launched)
inline bool commit_list_ok(const EcallArg* args, size_t n_args, const MemAccess* reads, size_t n_reads, const MemAccess* acc,
                           size_t n_acc) {
    size_t at = 0, ma = 0;
    for (size_t e = 0; e < n_args; e++) {
        if (args[e].t0 != 2) continue;
        if (args[e].a1 >= MAX_COMMIT) return false;
        const uint32_t n = commit_words(args[e].a0, args[e].a1);
        for (uint32_t k = 0; k < n; k++, at++) {
            if (at >= n_reads) return false;
            const MemAccess& m = reads[at];
            if (m.cycle != args[e].cycle || m.waddr != ((args[e].a0 & ~3u) + 4 * k) >> 2 || m.before != m.after) return false;
        }
        while (ma < n_acc && acc[ma].cycle < args[e].cycle) ma++;
        if (ma < n_acc && acc[ma].cycle == args[e].cycle) return false;
    }
    return at == n_reads;
}

// the access list memop and the memory table see: the cycle-order merge of the two (out: n_acc + n_reads entries)
inline void merge_accesses(const MemAccess* acc, size_t n_acc, const MemAccess* reads, size_t n_reads, MemAccess* out) {
    size_t i = 0, j = 0, o = 0;
    while (i < n_acc || j < n_reads) out[o++] = j >= n_reads || (i < n_acc && acc[i].cycle <= reads[j].cycle) ? acc[i++] : reads[j++];
}

// ---- the shard driver's error word: what a kernel finds wrong it ORs into one device word, read back after the run
enum ShardErr : uint32_t {
    ERR_WORD = 1,            // prep: one pc with two instruction words (rv32im-elf: a word that is not the image's)
    ERR_SIDE_LIST = 2,       // prep: an ecall row that is not in the side list
    ERR_PC = 4,              // prep: a pc outside the program's slots (rv32im-elf: outside the image)
    ERR_M_RESULT = 8,        // muldiv: the executor's result is not the op's
    ERR_M_COUNT = 16,        // muldiv: the device's count of M rows is not the host's
    ERR_ACCESS = 32,         // memop: an access is not what its instruction names
    ERR_HEADS = 64,          // mem_link: the device's count of distinct words is not the host's
    ERR_JOURNAL = 128,       // mem_journal_kernel's own flag word: the memory table is not one a journal can be read off
    ERR_IO_LIST = 256,       // io_patch / io_rows: the ecall side list is not the trace's ecalls
    ERR_COMMIT_READ = 512,   // io_rows: a commit read is not word k of its call
};

// What the driver returns for an error word, the muldiv rows (m_total) and the distinct words (heads) counted on the
// device against the host's m_count and mem_words: the first check that fails, in this order.  RK_OK: the driver goes on
// to compare the final registers.
struct ShardVerdict {
    int status;
    const char* message;
};
template <int CS>
inline ShardVerdict shard_verdict(uint32_t bits, uint32_t m_total, size_t m_count, uint32_t heads, size_t mem_words) {
    using CH = Chips<CS>;
    if (CH::io && (bits & ERR_IO_LIST))
        return {RK_ERR_INVALID, "rk_exec_rv32io_shard_device: the ecall side list is not the trace's ecalls"};
    if (CH::commit && (bits & ERR_COMMIT_READ))
        return {RK_ERR_INVALID, "rk_exec_rv32commit_shard_device: a commit read is not the word of its call"};
    if (CH::mem && (bits & ERR_ACCESS))
        return {RK_ERR_INTERNAL, "rk_exec_rv32mem_shard_device: an access is not the one its instruction names"};
    if (CH::mem && ((bits & ERR_HEADS) || heads != mem_words))
        return {RK_ERR_INTERNAL, "rk_exec_rv32mem_shard_device: the distinct words on the device are not the host's"};
    if (bits & (ERR_WORD | ERR_SIDE_LIST | ERR_PC)) {
        if (CH::elf && (bits & (ERR_WORD | ERR_PC)))
            return {RK_ERR_INVALID, bits & ERR_WORD ? "rk_exec_rv32elf_shard_device: an executed word is not the program image's word at its pc"
                                                    : "rk_exec_rv32elf_shard_device: a pc executed outside the program image"};
        return {RK_ERR_INVALID, bits & ERR_WORD ? "rk_exec_rv32_shard_device: a pc executed with two instruction words in one shard"
                                                : "rk_exec_rv32_shard_device: trace and side list disagree"};
    }
    if (CH::im && (bits || m_total != m_count))
        return {RK_ERR_INTERNAL, "rk_exec_rv32im_shard_device: an M result or the muldiv row count is not the executor's"};
    return {RK_OK, nullptr};
}

}  // namespace rv32
