// The kernels of the rv32 shard pipeline that every chip set runs (rv32_shards.hip includes this once; the driver and the
// stream order are there): prep, the register scans, the cpu rows, the program / byte / range / shift / register tables
// or their count columns, and rv32im's muldiv family.  What a row holds is rv32_rows.hpp's lane bodies; here is the
// wave-level code around them.  rv32_kernels_mem.hpp has the kernels that read the access list and the ecall side list.
#pragma once
#include "rv32_tiles.hpp"

namespace rv32 {

// ELF (rv32im-elf): the slot of a cycle is the image row of its pc -- the segment table arrives by value, in scalar
// registers -- and its word is compared with the image's; nothing is recorded (prog_ins unused)
template <bool ELF>
struct ImageArgs {};   // the other chip sets: no argument bytes
template <>
struct ImageArgs<true> {
    Image img;
    const uint32_t* words;   // the image's words, device memory
};
// IO (the io form, raiko_amd/rv32io.py): the key reads an ecall word as `ecall a0, a1` and bit 17 of acc marks its row: the
// fourth access, of x5
template <bool ELF, bool IO>
__global__ void prep_kernel(const TraceRow* __restrict__ tr, size_t cycles, size_t n, const uint32_t* __restrict__ ecalls,
                            uint32_t n_ecalls, uint32_t pc_base, uint32_t n_slots, uint32_t* __restrict__ wval,
                            uint32_t* __restrict__ acc, uint32_t* __restrict__ prog_mult, uint32_t* __restrict__ prog_ins,
                            uint32_t* __restrict__ err, uint32_t* __restrict__ mflag, const ImageArgs<ELF> image) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i >= cycles) {
        wval[i] = 0;
        acc[i] = 0;
        if (mflag) mflag[i] = 0;
        return;
    }
    const TraceRow r = tr[i];
    const Dec d = IO ? decode_io(r.ins) : decode(r.ins);
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
        else atomicOr(err, ERR_SIDE_LIST);
    }
    wval[i] = written(d, r, a0);
    acc[i] = d.rs1 | d.rs2 << 5 | d.wreg << 10 | d.wr << 15 | 1u << 16 | (IO ? d.is_sys << 17 : 0u);
    if constexpr (ELF) {
        const uint32_t slot = image_row(image.img, r.pc);
        if (slot >= n_slots) {   // NO_ROW: a pc outside the image
            atomicOr(err, ERR_PC);
            return;
        }
        atomicAdd(&prog_mult[slot], 1u);
        if (image.words[slot] != r.ins) atomicOr(err, ERR_WORD);   // the word is not the image's: a store changed it
    } else {
        const uint32_t slot = (r.pc - pc_base) >> 2;
        if (slot >= n_slots) {
            atomicOr(err, ERR_PC);
            return;
        }
        atomicAdd(&prog_mult[slot], 1u);
        const uint32_t old = atomicCAS(&prog_ins[slot], 0u, r.ins);
        if (old != 0 && old != r.ins) atomicOr(err, ERR_WORD);    // one pc, two instruction words in one shard
    }
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
        if (acc[i] >> 17 & 1) atomicMax(&s[5], tsa);   // the io form: an ecall row reads x5 at tsa (its rs1 is x10)
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

// io: the trace is the io form's (io_patch_kernel): an ecall row's a / b / res hold a0 / a1 / t0, and its first timestamp
// is also that of its read of x5
__device__ inline uint32_t value_at(uint32_t ts, uint32_t reg, const TraceRow* tr, const uint32_t* wval, const uint32_t* init,
                                    bool io = false) {
    if (ts == 0) return init[reg];
    const uint32_t j = (ts - 1) / 3, k = (ts - 1) % 3;
    if (io && k == 0 && reg == 5 && tr[j].ins == ECALL_WORD) return tr[j].res;
    return k == 0 ? tr[j].a : k == 1 ? tr[j].b : wval[j];
}

// the cpu table: each access's predecessor from the scans, then the chip set's row pieces and its lookups' counts
template <int CS>
__global__ void __launch_bounds__(TB) rows_kernel(const TraceRow* __restrict__ tr, size_t cycles, uint32_t end_pc,
                                                   const uint32_t* __restrict__ acc, const uint32_t* __restrict__ wval,
                                                   const uint32_t* __restrict__ pre, const uint32_t* __restrict__ init,
                                                   uint32_t* __restrict__ out, uint32_t* __restrict__ hist,
                                                   uint32_t* __restrict__ byte_mult, uint32_t* __restrict__ shift_mult,
                                                   const uint32_t* __restrict__ necw, size_t n) {
    using CH = Chips<CS>;
    extern __shared__ uint32_t s_rows[];            // TB x (cpu_w | 1)
    __shared__ uint32_t s_wave[32][TB / 64];
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t rs1, rs2, wreg;
    bool wr, active;
    unpack(acc[i], rs1, rs2, wreg, wr, active);
    const bool sys = CH::io && (acc[i] >> 17 & 1);   // the io form: the row also reads x5, at tsa
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
            if (CH::io && r == 5 && sys) v = tsa;
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
    uint32_t e1 = 0, e2 = 0, e3 = 0, e5 = 0;
#pragma unroll
    for (unsigned r = 0; r < 32; r++) {
        uint32_t ex = __shfl_up(incl[r], 1);
        if (lane == 0) ex = 0;
        for (unsigned w = 0; w < wave; w++) ex = max(ex, s_wave[r][w]);
        ex = max(ex, pre[(size_t)blockIdx.x * 32 + r]);
        if (rs1 == r) e1 = ex;
        if (rs2 == r) e2 = ex;
        if (wreg == r) e3 = ex;
        if (CH::io && r == 5) e5 = ex;
    }
    row_tile<CH::cpu_w>(s_rows, out, (size_t)blockIdx.x * TB, n, [&](uint32_t* row) {
        Mults m;
        if (active) {
            TraceRow r = tr[i];
            const Dec d = CH::io ? decode_io(r.ins) : decode(r.ins);
            const uint32_t t0 = r.res;
            if (CH::io && sys) r.res = 0;   // as the executor records it
            const uint32_t pb = rs2 == rs1 ? tsa : e2, pw = wr ? (wreg == rs2 ? tsa + 1 : wreg == rs1 ? tsa : e3) : 0;
            cpu_row_i(row, r, d, wval[i], tsa, e1, pb, pw, wr ? value_at(pw, wreg, tr, wval, init, CH::io) : 0, m);
            if constexpr (CH::cf) cpu_row_cf(row, r, d, m);
            if constexpr (CH::im) cpu_row_im(row, d);
            if constexpr (CH::mem) cpu_row_mem(row, d, necw[i]);   // necw: the access list's entries per cycle at ecall rows
            if constexpr (CH::io) cpu_row_io(row, d, t0, tsa, e5);
        } else {
            trace_cells(padding_row(end_pc), false, row);
        }
        row[TSA] = tsa;
        row[TSB] = tsa + 1;
        row[TSW] = tsa + 2;
        // RANGE16: the limbs the row sends (rv32.py RANGE_SENDS), BYTE: four triples of a bitwise row
        const unsigned rc[] = {PC_LO, PC_HI, NX_LO, NX_HI, RES_LO, RES_HI, D_LO, D_HI, DA_LO, DA_HI, DB_LO, DB_HI};
        for (unsigned c : rc) hist_add(hist, row[c], active);
        hist_add(hist, row[DW_LO], wr);
        hist_add(hist, row[DW_HI], wr);
        hist_add(hist, row[SA_CHK], m.is_slt);
        hist_add(hist, row[SB_CHK], m.is_slt);
        if constexpr (CH::io) {
            hist_add(hist, row[DT_LO], sys);
            hist_add(hist, row[DT_HI], sys);
        }
        if (m.bop)
            for (unsigned k = 0; k < 4; k++)
                atomicAdd(&byte_mult[(m.bop - 1) << 16 | ((m.ba >> (8 * k)) & 255) << 8 | ((m.bb >> (8 * k)) & 255)], 1u);
        if constexpr (CH::cf) {   // rv32cf.py RANGE_SENDS past rv32i's, then the four SHIFT lookups (k, x) -> row k 256 + x
            hist_add(hist, row[BD_LO], m.is_br);
            hist_add(hist, row[BD_HI], m.is_br);
            hist_add(hist, row[NXH], m.is_link);
            hist_add(hist, row[T], m.is_shift);
            hist_add(hist, row[SA_CHK], m.m_sa);
            hist_add(hist, row[SB_CHK], m.m_sb);
            for (unsigned j = 0; j < 4; j++) hist_add(shift_mult, row[SK] << 8 | row[SX + j], m.is_shift);
        }
    });
}

// the program table: one row per word of the executed pc range, then the row of word 0 at pc 0 with multiplicity 0
template <int CS>
__global__ void program_kernel(const uint32_t* __restrict__ prog_ins, const uint32_t* __restrict__ prog_mult,
                               uint32_t n_slots, uint32_t pc_base, size_t n_rows, uint32_t* __restrict__ out) {
    using CH = Chips<CS>;
    extern __shared__ uint32_t s_rows[];
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    row_tile<CH::prog_w>(s_rows, out, (size_t)blockIdx.x * blockDim.x, n_rows, [&](uint32_t* row) {
        if (s >= n_rows) return;
        const bool in = s < n_slots;
        const uint32_t pc = in ? pc_base + 4 * (uint32_t)s : 0u, ins = in ? prog_ins[s] : 0u;
        const Dec d = decode(ins);
        program_row_i(row, pc, ins, d, in ? prog_mult[s] : 0u);
        if constexpr (CH::cf) program_row_cf(row, d);
        if constexpr (CH::im) program_row_im(row, ins, d);
    });
}

// ---- rv32im-elf: a count column of n_rows words (counts past n_counts are 0)
__global__ void count_kernel(const uint32_t* __restrict__ counts, size_t n_counts, size_t n_rows, uint32_t* __restrict__ out) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_rows) out[r] = enc(r < n_counts ? counts[r] : 0u);
}

__global__ void shift_kernel(const uint32_t* __restrict__ shift_mult, uint32_t* __restrict__ out) {
    extern __shared__ uint32_t s_rows[];
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    row_tile<SHIFT_W>(s_rows, out, (size_t)blockIdx.x * blockDim.x, (size_t)1 << RK_RV32CF_SHIFT_LOG_ROWS,
                      [&](uint32_t* row) { shift_row(row, r, r < SHIFT_USED ? shift_mult[r] : 0u); });
}

__global__ void byte_kernel(const uint32_t* __restrict__ byte_mult, uint32_t* __restrict__ out) {
    extern __shared__ uint32_t s_rows[];
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    row_tile<BYTE_W>(s_rows, out, (size_t)blockIdx.x * blockDim.x, (size_t)1 << RK_RV32_BYTE_LOG_ROWS, [&](uint32_t* row) {
        if (r < (3u << 16)) byte_row(row, r, byte_mult[r]);
    });
}

__global__ void range_kernel(const uint32_t* __restrict__ hist, uint32_t* __restrict__ out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= (1u << 16)) return;
    out[2 * v] = enc(v);
    out[2 * v + 1] = enc(hist[v]);
}

// 32 lanes: the register table; fin gets the final values
__global__ void register_kernel(const uint32_t* __restrict__ final_ts, const uint32_t* __restrict__ init,
                                const TraceRow* __restrict__ tr, const uint32_t* __restrict__ wval,
                                uint32_t* __restrict__ fin, uint32_t* __restrict__ out, uint32_t io) {
    __shared__ uint32_t s_fin[32];
    extern __shared__ uint32_t s_rows[];
    const unsigned r = threadIdx.x;
    s_fin[r] = value_at(final_ts[r], r, tr, wval, init, io != 0);
    fin[r] = s_fin[r];
    __syncthreads();
    row_tile<REG_W>(s_rows, out, 0, 32, [&](uint32_t* row) { register_row(row, r, final_ts[r], init, s_fin); });
}

// ---- rv32im: the muldiv table
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

// one lane per muldiv row: row k < count is the witness of cpu row idx[k], rows past count padding (ONE = 1, the rest 0);
// the RANGE16 / BYTE / SHIFT counts of the active rows go to the shard's histograms
__global__ void muldiv_kernel(const TraceRow* __restrict__ tr, size_t cycles, const uint32_t* __restrict__ wval,
                              const uint32_t* __restrict__ idx, size_t count, size_t n_rows, uint32_t* __restrict__ out,
                              uint32_t* __restrict__ hist, uint32_t* __restrict__ byte_mult, uint32_t* __restrict__ shift_mult,
                              uint32_t* __restrict__ err) {
    extern __shared__ uint32_t s_rows[];
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    row_tile<MD_W>(s_rows, out, (size_t)blockIdx.x * blockDim.x, n_rows, [&](uint32_t* row) {
        row[D_ONE] = 1;
        bool on = k < count;
        const uint32_t i = on ? idx[k] : 0u;
        if (on && i >= cycles) {   // the device's count is not the host's (reported after the run)
            atomicOr(err, ERR_M_COUNT);
            on = false;
        }
        if (on && !muldiv_row(row, tr[i], wval[i])) atomicOr(err, ERR_M_RESULT);   // the executor's result is not the op's
        for (unsigned c : MD_RANGE) hist_add(hist, row[c], on);
        for (unsigned j = 0; j < 4; j++) hist_add(shift_mult, 256u + row[D_X + 3 + 4 * j], on);   // (1, top byte) -> row 256 + x
        // AND (op 1) of each byte pair; the wave-aggregated add, as M loops repeat their operands
        for (unsigned j = 0; j < 8; j++) hist_add(byte_mult, row[MD_PAIRS[j][0]] << 8 | row[MD_PAIRS[j][1]], on);
    });
}

}  // namespace rv32
