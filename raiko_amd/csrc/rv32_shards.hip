// The witness of an executed segment written on the GPU (include/raiko_hip.h): the stand-in trace circuit's columns
// (rk_exec_witness_device*) and the tables of the rv32 chip sets (rk_exec_rv32_shard_device,
// rk_exec_rv32cf_shard_device, rk_exec_rv32im_shard_device, rk_exec_rv32elf_shard_device, rk_exec_rv32mem_shard_device and
// the preprocessed matrices of the last two, rk_rv32elf_prep_device / rk_rv32mem_prep_device), and the link between shard
// memories read off a finished memory table (rk_rv32mem_journal_device, its host twin rk_rv32mem_journal_root;
// raiko_amd/rv32link.py).  The segment is read through executor.hpp's view; what a
// row holds is rv32_rows.hpp's lane bodies (raiko_amd/rv32.py, rv32cf.py, rv32im.py, rv32elf.py are the same in numpy and
// name every column).  What is here: the kernels around those bodies -- the wave-level code, the atomics, the LDS staging -- and
// the host driver.
#include "internal.hpp"

#include <algorithm>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "rv32_rows.hpp"

// The stand-in trace's columns: one lane per row, the trace rows (28 bytes per cycle) are the only upload -- 2.5x less
// over PCIe than the 18 finished columns and none of the host's time (rk_exec_witness_device).
__global__ void exec_witness_kernel(uint32_t* __restrict__ code, uint32_t* __restrict__ data, const TraceRow* __restrict__ tr,
                                    size_t cycles, size_t n, uint32_t end_pc, uint32_t rows_only) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool active = i < cycles;
    // rows_only: the 16 data columns as one row-major row per lane (64 contiguous bytes: an rk_p3_table), no code columns
    auto put = [&](uint32_t* base, unsigned col, uint32_t canon) {
        base[rows_only ? i * RK_TRACE_DATA_COLS + col : (size_t)col * n + i] = rv32::enc(canon);
    };
    if (!rows_only) {
        put(code, 0, i == 0 ? 1u : 0u);
        put(code, 1, i + 1 == n ? 1u : 0u);
    }
    uint32_t c[RK_TRACE_DATA_COLS];
    rv32::trace_cells(active ? tr[i] : rv32::padding_row(end_pc), active, c);
    for (unsigned col = 0; col < RK_TRACE_DATA_COLS; col++) put(data, col, c[col]);
}

static int witness_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_code, uint32_t* d_data, bool rows_only) {
    if (!ctx || !d_data) return RK_ERR_INVALID;
    ExecSegmentView v;
    RK_TRY(exec_segment_view(ex, index, &v));
    const std::vector<TraceRow>& tr = *v.trace;
    const size_t n = (size_t)1 << v.seg->po2;
    if (tr.size() > n) return RK_ERR_INTERNAL;
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
                           (const TraceRow*)d_tr, tr.size(), n, v.seg->end_pc, rows_only ? 1u : 0u);
        st = rk::post_launch(ctx, "exec_witness_kernel");
    }
    rk::dev_free(ctx, d_tr);
    return st;
}

// ---------------------------------------------------------------------------------------------------------------------
// The rv32 chip sets.  Per segment on the GPU: prep (decode, recompute the written value, pack the three accesses, count
// program hits) -> block_last (last access per register per 128 rows) -> scan (exclusive max-scan of those 32-vectors)
// -> rows (in-block resolve of each access's predecessor, the cpu row staged through LDS, RANGE16 / BYTE / SHIFT counts)
// -> rv32im: the muldiv rows -> the program, byte, range, register and shift tables.  rv32im-elf: the same pipeline; a
// cycle is counted at the image row of its pc (its word compared with the image's) and the program, byte, range and
// shift tables leave as count columns.  rv32im-mem: rv32im-elf's pipeline and, from the access list: keys (word address,
// list index; the ecall rows' per-cycle counts) -> rocPRIM's stable radix sort by the 30 address bits -> heads per block,
// scan -> link (each access's predecessor, the boundary rows) -> the memop rows.  The io form of rv32im-mem
// (rk_exec_rv32io_shard_device, raiko_amd/rv32io.py): the same pipeline over the io form of the trace (patch: an ecall
// row's a / b / res become the call's a0 / a1 / t0), the read of x5 in the scans, and from the ecall side list: offsets
// per ecall (1 + the words it stored), scan -> the io rows and the stream matrix -> its commitment (rk_mmcs_commit).
namespace rv32 {

constexpr unsigned TB = 128;   // rows per block (the cpu rows kernel stages TB x 69 words in LDS, 121 / 133 / 141 for rv32i-cf / rv32im / rv32im-mem)

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

// One tile of a row-major table, a row of W words per lane: the lane's row is zeroed in LDS (s_rows: blockDim.x x (W | 1)
// words; the odd stride avoids bank conflicts), fill(row) writes its canonical cells, every cell goes to Montgomery form
// and the tile's rows r0 .. of n_rows leave for HBM as whole lines.  Every lane of the block calls it.
template <unsigned W, class F>
__device__ __forceinline__ void row_tile(uint32_t* s_rows, uint32_t* out, size_t r0, size_t n_rows, F&& fill) {
    constexpr unsigned SW = W | 1;
    uint32_t* row = s_rows + threadIdx.x * SW;
    for (unsigned c = 0; c < W; c++) row[c] = 0;
    fill(row);
    for (unsigned c = 0; c < W; c++) row[c] = enc(row[c]);
    __syncthreads();
    const size_t rows = n_rows - r0 < blockDim.x ? n_rows - r0 : blockDim.x;
    for (size_t k = threadIdx.x; k < rows * W; k += blockDim.x) out[r0 * W + k] = s_rows[(k / W) * SW + k % W];
}

// One tile of a preprocessed matrix (rv32im-elf): the lane's FULL row of FW words is built in LDS as in row_tile, select
// picks its OW tuple cells, and only those leave for HBM, in Montgomery form, as whole lines.  Every lane of the block
// calls it.
template <unsigned FW, unsigned OW, class F, class S>
__device__ __forceinline__ void prep_tile(uint32_t* s_rows, uint32_t* out, size_t r0, size_t n_rows, F&& fill, S&& select) {
    constexpr unsigned SW = FW | 1;
    static_assert(OW <= FW, "the selected cells are staged in the full row's place");
    uint32_t* row = s_rows + threadIdx.x * SW;
    for (unsigned c = 0; c < FW; c++) row[c] = 0;
    fill(row);
    uint32_t o[OW];
    select(o, row);
#pragma unroll
    for (unsigned c = 0; c < OW; c++) row[c] = enc(o[c]);
    __syncthreads();
    const size_t rows = n_rows - r0 < blockDim.x ? n_rows - r0 : blockDim.x;
    for (size_t k = threadIdx.x; k < rows * OW; k += blockDim.x) out[r0 * OW + k] = s_rows[(k / OW) * SW + k % OW];
}

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
        else atomicOr(err, 2u);
    }
    wval[i] = written(d, r, a0);
    acc[i] = d.rs1 | d.rs2 << 5 | d.wreg << 10 | d.wr << 15 | 1u << 16 | (IO ? d.is_sys << 17 : 0u);
    if constexpr (ELF) {
        const uint32_t slot = image_row(image.img, r.pc);
        if (slot >= n_slots) {   // NO_ROW: a pc outside the image
            atomicOr(err, 4u);
            return;
        }
        atomicAdd(&prog_mult[slot], 1u);
        if (image.words[slot] != r.ins) atomicOr(err, 1u);   // the word is not the image's: a store changed it
    } else {
        const uint32_t slot = (r.pc - pc_base) >> 2;
        if (slot >= n_slots) {
            atomicOr(err, 4u);
            return;
        }
        atomicAdd(&prog_mult[slot], 1u);
        const uint32_t old = atomicCAS(&prog_ins[slot], 0u, r.ins);
        if (old != 0 && old != r.ins) atomicOr(err, 1u);    // one pc, two instruction words in one shard
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

// the io form: one lane per entry of the ecall side list writes a0 / a1 / t0 into its trace row's a / b / res (0 as the
// executor records them: other chip sets read them); err |= 256 for an entry that is at no ecall row
__global__ void io_patch_kernel(TraceRow* __restrict__ tr, size_t cycles, const EcallArg* __restrict__ args, size_t count,
                                uint32_t* __restrict__ err) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const EcallArg e = args[k];
    if (e.cycle >= cycles || tr[e.cycle].ins != ECALL_WORD) {
        atomicOr(err, 256u);
        return;
    }
    tr[e.cycle].a = e.a0;
    tr[e.cycle].b = e.a1;
    tr[e.cycle].res = e.t0;
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

// ---- rv32im-elf: a count column of n_rows words (counts past n_counts are 0), and the four preprocessed matrices
__global__ void count_kernel(const uint32_t* __restrict__ counts, size_t n_counts, size_t n_rows, uint32_t* __restrict__ out) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_rows) out[r] = enc(r < n_counts ? counts[r] : 0u);
}

template <int MEM>   // 0: rv32im-elf's 42 columns; 1: rv32im-mem's 48; 2: the io form's 48 (the ecall word reads a0, a1)
__global__ void program_prep_kernel(const uint32_t* __restrict__ words, uint32_t n_words, const Image img, size_t n_rows,
                                    uint32_t* __restrict__ out) {
    extern __shared__ uint32_t s_rows[];
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    prep_tile<IM_PROG_W, MEM ? MEM_PROG_W : ELF_PROG_W>(
        s_rows, out, (size_t)blockIdx.x * blockDim.x, n_rows,
        [&](uint32_t* row) {
            if (s >= n_rows) return;
            const bool in = s < n_words;
            const uint32_t pc = in ? image_pc(img, (uint32_t)s) : 0u, ins = in ? words[s] : 0u;
            const Dec d = decode(ins);
            program_row_i(row, pc, ins, d, 0u);
            program_row_cf(row, d);
            program_row_im(row, ins, d);
        },
        [](uint32_t* o, const uint32_t* row) {
            if constexpr (MEM == 2) program_prep_row_io(o, row, decode(row[2] | row[3] << 16));
            else if constexpr (MEM == 1) program_prep_row_mem(o, row, decode(row[2] | row[3] << 16));
            else program_prep_row(o, row);
        });
}

__global__ void byte_prep_kernel(uint32_t* __restrict__ out) {
    extern __shared__ uint32_t s_rows[];
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    prep_tile<BYTE_W, ELF_TUPLE_W>(
        s_rows, out, (size_t)blockIdx.x * blockDim.x, (size_t)1 << RK_RV32_BYTE_LOG_ROWS,
        [&](uint32_t* row) {
            if (r < (3u << 16)) byte_row(row, r, 0u);
        },
        [](uint32_t* o, const uint32_t* row) { byte_prep_row(o, row); });
}

__global__ void shift_prep_kernel(uint32_t* __restrict__ out) {
    extern __shared__ uint32_t s_rows[];
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    prep_tile<SHIFT_W, ELF_TUPLE_W>(
        s_rows, out, (size_t)blockIdx.x * blockDim.x, (size_t)1 << RK_RV32CF_SHIFT_LOG_ROWS,
        [&](uint32_t* row) { shift_row(row, r, 0u); }, [](uint32_t* o, const uint32_t* row) { shift_prep_row(o, row); });
}

__global__ void range_prep_kernel(uint32_t* __restrict__ out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < (1u << 16)) out[v] = enc(v);
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
            atomicOr(err, 16u);
            on = false;
        }
        if (on && !muldiv_row(row, tr[i], wval[i])) atomicOr(err, 8u);   // the executor's result is not the op's
        for (unsigned c : MD_RANGE) hist_add(hist, row[c], on);
        for (unsigned j = 0; j < 4; j++) hist_add(shift_mult, 256u + row[D_X + 3 + 4 * j], on);   // (1, top byte) -> row 256 + x
        // AND (op 1) of each byte pair; the wave-aggregated add, as M loops repeat their operands
        for (unsigned j = 0; j < 8; j++) hist_add(byte_mult, row[MD_PAIRS[j][0]] << 8 | row[MD_PAIRS[j][1]], on);
    });
}

// ---- rv32im-mem: the memop and memory tables from the access list (acc: count entries in cycle order)
// one lane per access: its sort key (the word address, 30 bits) and payload (its list index); an access at an ecall row
// is counted at its cycle (necw: what rows_kernel writes as N_ECW)
__global__ void mem_keys_kernel(const MemAccess* __restrict__ acc, size_t count, const TraceRow* __restrict__ tr,
                                uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ necw) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const MemAccess m = acc[k];
    keys[k] = m.waddr;
    vals[k] = (uint32_t)k;
    if ((tr[m.cycle].ins & 0x7fu) == OPCODES[O_SYSTEM]) atomicAdd(&necw[m.cycle], 1u);   // m.cycle < cycles: checked on the host
}

__device__ inline bool mem_head(const uint32_t* keys, size_t i, size_t count) {
    return i < count && (i == 0 || keys[i] != keys[i - 1]);
}

// per block of TB sorted positions: how many start a run of one address
__global__ void mhead_count_kernel(const uint32_t* __restrict__ keys, size_t count, uint32_t* __restrict__ hblk) {
    const int c = __syncthreads_count(mem_head(keys, (size_t)blockIdx.x * TB + threadIdx.x, count));
    if (threadIdx.x == 0) hblk[blockIdx.x] = (uint32_t)c;
}

// one lane per sorted position i: the access before it at its word is its left neighbour unless it heads its run (pts, in
// list order).  A head writes the boundary row of its word: its index is the heads before it (hblk: the exclusive scan
// over blocks, then the ballot compaction of mcompact_kernel), INIT its own old word, FINAL / FTS its run's tail, found
// by binary search for the next address, and the limb-wise distance to that address.  The block's rows leave LDS as whole lines.
__global__ void __launch_bounds__(TB) mem_link_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                       const MemAccess* __restrict__ acc, size_t count,
                                                       const uint32_t* __restrict__ hblk, uint32_t* __restrict__ pts,
                                                       uint32_t* __restrict__ out, size_t n_rows, uint32_t* __restrict__ hist,
                                                       uint32_t* __restrict__ err) {
    __shared__ uint32_t s_rows[TB * BD_W];
    __shared__ uint32_t s_wave[TB / 64];
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool on = i < count, head = mem_head(keys, i, count);
    const uint32_t key = on ? keys[i] : 0u;
    if (on) pts[vals[i]] = head ? 0u : 3 * acc[vals[i - 1]].cycle + 1;
    const uint64_t bal = __ballot(head);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t li = (uint32_t)__popcll(bal & ((1ull << lane) - 1)), total = 0;
    for (unsigned w = 0; w < TB / 64; w++) {
        if (w < wave) li += s_wave[w];
        total += s_wave[w];
    }
    uint32_t row[BD_W] = {0};
    if (head) {
        size_t lo = i + 1, hi = count;   // the first position past the run
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            if (keys[mid] == key) lo = mid + 1;
            else hi = mid;
        }
        const MemAccess first = acc[vals[i]], last = acc[vals[lo - 1]];
        memory_row(row, key, first.before, last.after, 3 * last.cycle + 1, lo < count, lo < count ? keys[lo] : 0u);
        for (unsigned c = 0; c < BD_W; c++) s_rows[li * BD_W + c] = enc(row[c]);
    }
    for (unsigned c : BD_RANGE) hist_add(hist, row[c], head);
    __syncthreads();
    const size_t r0 = hblk[blockIdx.x];
    if (r0 + total > n_rows) {   // the device's count of distinct words is not the host's (reported after the run)
        if (threadIdx.x == 0) atomicOr(err, 64u);
        return;
    }
    for (size_t k = threadIdx.x; k < (size_t)total * BD_W; k += TB) out[r0 * BD_W + k] = s_rows[k];
}

// one lane per memop row: row k < count is the witness of access k, rows past count padding (ONE = 1, the rest 0); the
// RANGE16 / BYTE / SHIFT counts of the active rows go to the shard's histograms.  W: MO_W, or CM_MO_W in the commit form
// (io = 2), where an access at a COMMIT row is an ECR row
template <unsigned W>
__global__ void memop_kernel(const TraceRow* __restrict__ tr, const uint32_t* __restrict__ wval, const MemAccess* __restrict__ acc,
                             const uint32_t* __restrict__ pts, size_t count, size_t n_rows, uint32_t* __restrict__ out,
                             uint32_t* __restrict__ hist, uint32_t* __restrict__ byte_mult, uint32_t* __restrict__ shift_mult,
                             uint32_t* __restrict__ err, uint32_t io) {
    extern __shared__ uint32_t s_rows[];
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    row_tile<W>(s_rows, out, (size_t)blockIdx.x * blockDim.x, n_rows, [&](uint32_t* row) {
        row[G_ONE] = 1;
        const bool on = k < count;
        if (on) {
            const MemAccess m = acc[k];
            const TraceRow r = tr[m.cycle];
            if (!memop_row(row, m, r, decode(r.ins), wval[m.cycle], pts[k], io != 0, W == CM_MO_W)) atomicOr(err, 32u);   // not what the instruction names
        }
        for (unsigned c : MO_RANGE) hist_add(hist, row[c], on);
        hist_add(shift_mult, 256u + row[G_TOP], on);   // (1, top byte) -> row 256 + x
        for (unsigned j = 0; j < 6; j++) hist_add(byte_mult, row[G_W + 2 * j] << 8 | row[G_W + 2 * j + 1], on);   // AND (op 1)
    });
}

// ---- the io form (raiko_amd/rv32io.py): the io table from the ecall side list (args: count entries in cycle order)
// per block of TB ecalls: ecall e takes 1 + GOT rows (GOT: necw at its cycle, what mem_keys_kernel counted); eoff[e] = the
// rows of the block's ecalls before it (a wave scan, the waves' totals through LDS), eblk[block] = the block's rows, which
// mscan_kernel turns into the rows before the block
// COMMIT (the commit form, raiko_amd/rv32commit.py): a COMMIT takes 1 + NCW rows, NCW = commit_words(a0, a1) from its
// arguments alone; the same pass scans NCW -- coff / cblk: the dense index of the call's first commit-log row -- and the
// bytes a1 of the COMMITs -- joff / jblk: the call's journal position past jpos_start
struct CommitScan {
    uint32_t *coff, *cblk, *joff, *jblk;
};
template <bool COMMIT>
struct CommitScanOf {};   // the io form: no argument bytes
template <>
struct CommitScanOf<true> : CommitScan {};
template <bool COMMIT>
__global__ void __launch_bounds__(TB) io_offsets_kernel(const EcallArg* __restrict__ args, size_t count, const uint32_t* __restrict__ necw,
                                                         uint32_t* __restrict__ eoff, uint32_t* __restrict__ eblk, CommitScanOf<COMMIT> cs) {
    constexpr unsigned NV = COMMIT ? 3 : 1;
    __shared__ uint32_t s_wave[NV][TB / 64];
    const size_t e = (size_t)blockIdx.x * TB + threadIdx.x;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t wgt[NV] = {};
    if (e < count) {
        const EcallArg a = args[e];
        wgt[0] = 1u + necw[a.cycle];   // cycle < cycles: checked on the host
        if constexpr (COMMIT) {
            if (a.t0 == 2) {
                wgt[1] = commit_words(a.a0, a.a1);
                wgt[2] = a.a1;
                wgt[0] = 1u + wgt[1];
            }
        }
    }
    uint32_t v[NV];
#pragma unroll
    for (unsigned j = 0; j < NV; j++) {
        v[j] = wgt[j];
#pragma unroll
        for (unsigned off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(v[j], off);
            if (lane >= off) v[j] += t;
        }
        if (lane == 63) s_wave[j][wave] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (unsigned j = 0; j < NV; j++) {
        uint32_t before = 0, total = 0;
        for (unsigned w = 0; w < TB / 64; w++) {
            if (w < wave) before += s_wave[j][w];
            total += s_wave[j][w];
        }
        uint32_t *off = eoff, *blk = eblk;
        if constexpr (COMMIT) {
            off = j == 0 ? eoff : j == 1 ? cs.coff : cs.joff;
            blk = j == 0 ? eblk : j == 1 ? cs.cblk : cs.jblk;
        }
        if (e < count) off[e] = before + v[j] - wgt[j];
        if (threadIdx.x == 0) blk[blockIdx.x] = total;
    }
}

// one lane per io row: row i < total belongs to the last ecall e with first(e) = eblk[e / TB] + eoff[e] <= i (binary
// search; first is strictly increasing) and is its head (i = first) or its word i - first - 1, whose access is that far
// past the first access at the ecall's cycle (binary search in the access list, which is in cycle order).  Rows from
// total on are padding at the final position.  A word row also writes its stream tuple, Montgomery, at row POS -
// pos_start of the matrix the digest commits to (stream: n_rows x 6, zeroed before).  The block's rows leave LDS as whole
// lines (row_tile: stride 47, odd).  err |= 256: the side list is not the trace's ecalls -- a call number that is none of
// the three, a result, a count of stored words or a position that is not the call's, a word that is not where READ stores
// COMMIT (the commit form): rows of CM_IO_W words (stride 65, odd; 128 rows are 33 KiB of LDS).  `acc` is the merged list,
// so necw at a COMMIT's cycle is the count of its commit reads.  Commit-word row k of COMMIT e is computed in closed form
// from (a0, a1, k) (io_commit_row); its word is reads[dense], dense = cblk[e / TB] + coff[e] + k -- no search --, and its
// log tuple goes to row `dense` of the matrix the commit log's digest commits to (clog: n_rows x 6, Montgomery, zeroed
// before) and, canonical, of dlog (n_rows x 3).  err |= 512: a commit read that is not word k of its call
struct CommitRows {
    const MemAccess* reads;
    uint32_t n_reads;
    const uint32_t *coff, *cblk, *joff, *jblk;
    uint32_t jpos_start, jpos_end, pos_end;
    uint32_t *clog, *dlog;
};
template <bool COMMIT>
struct CommitRowsOf {};   // the io form: no argument bytes
template <>
struct CommitRowsOf<true> : CommitRows {};
template <bool COMMIT>
__global__ void io_rows_kernel(const EcallArg* __restrict__ args, size_t count, const uint32_t* __restrict__ ecalls,
                               const uint32_t* __restrict__ necw, const uint32_t* __restrict__ eoff, const uint32_t* __restrict__ eblk,
                               const MemAccess* __restrict__ acc, size_t mem_count, uint32_t n_input, uint32_t pos_start,
                               uint32_t total, size_t n_rows, uint32_t* __restrict__ out, uint32_t* __restrict__ stream,
                               uint32_t* __restrict__ hist, uint32_t* __restrict__ err, CommitRowsOf<COMMIT> cm) {
    extern __shared__ uint32_t s_rows[];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    row_tile<COMMIT ? CM_IO_W : IO_W>(s_rows, out, (size_t)blockIdx.x * blockDim.x, n_rows, [&](uint32_t* row) {
        const bool on = i < total;
        bool head = false, read = false, word = false, chead = false, cw = false;
        const bool halted = count && args[count - 1].t0 == 0;
        if (on) {
            size_t lo = 0, hi = count;   // the last e with first(e) <= i
            while (hi - lo > 1) {
                const size_t mid = (lo + hi) / 2;
                if (eblk[mid / TB] + eoff[mid] <= i) lo = mid;
                else hi = mid;
            }
            const EcallArg e = args[lo];
            const uint32_t first = eblk[lo / TB] + eoff[lo], k = (uint32_t)i - first;
            const bool is_commit = COMMIT && e.t0 == 2;
            const uint32_t got = is_commit ? 0u : necw[e.cycle];
            uint32_t jpos = 0;
            if constexpr (COMMIT) jpos = cm.jpos_start + cm.jblk[lo / TB] + cm.joff[lo];
            bool ok = true;
            if (k == 0) {
                head = true;
                read = e.t0 == 1;
                chead = is_commit;
                ok = ecalls[2 * lo] == e.cycle && io_head_row(row, e, ecalls[2 * lo + 1], got, n_input, lo > 0, lo ? 3 * args[lo - 1].cycle + 1 : 0u);
                // the positions chain: this call starts where the one before stopped
                uint32_t prev_got = 0;
                if (lo && !(COMMIT && args[lo - 1].t0 == 2)) prev_got = necw[args[lo - 1].cycle];
                ok = ok && e.pos == (lo ? args[lo - 1].pos + prev_got : pos_start);
                if constexpr (COMMIT) ok = ok && io_commit_head(row, e, necw[e.cycle], jpos);
                io_row_tail(row, e.pos, true, halted && lo + 1 == count);
                if constexpr (COMMIT) io_commit_tail(row, jpos);
            } else if (is_commit) {
                if constexpr (COMMIT) {
                    const uint32_t dense = cm.cblk[lo / TB] + cm.coff[lo] + (k - 1);
                    ok = k - 1 < commit_words(e.a0, e.a1) && e.a1 < MAX_COMMIT && dense < cm.n_reads && dense < n_rows;
                    if (ok) ok = io_commit_row(row, e, k - 1, jpos, cm.reads[dense]);
                    const uint32_t jp = row[Q_JL] | row[Q_JH] << 14;
                    ok = ok && jp < (1u << 30);
                    cw = ok;   // the limbs of a row that is not the call's go to no histogram
                    io_row_tail(row, e.pos, true, 0u);
                    io_commit_tail(row, jp);
                    if (ok) {
                        const uint32_t t[RK_RV32LINK_TUPLE] = {row[Q_JL], row[Q_JH], row[Q_V_LO], row[Q_V_HI], row[Q_S], row[Q_CNT]};
                        for (unsigned j = 0; j < RK_RV32LINK_TUPLE; j++) cm.clog[(size_t)dense * RK_RV32LINK_TUPLE + j] = enc(t[j]);
                        cm.dlog[(size_t)dense * 3 + 0] = jp;
                        cm.dlog[(size_t)dense * 3 + 1] = row[Q_V_LO] | row[Q_V_HI] << 16;
                        cm.dlog[(size_t)dense * 3 + 2] = row[Q_S] | row[Q_CNT] << 16;
                    } else {
                        atomicOr(err, 512u);
                        ok = true;
                    }
                }
            } else {
                word = true;
                size_t a = 0, b = mem_count;   // the first access at the ecall's cycle
                while (a < b) {
                    const size_t mid = (a + b) / 2;
                    if (acc[mid].cycle < e.cycle) a = mid + 1;
                    else b = mid;
                }
                const size_t at = a + (k - 1);
                ok = at < mem_count && k - 1 < got && e.t0 == 1;
                const uint32_t pos = e.pos + (k - 1);
                if (ok) ok = io_word_row(row, e, got, k - 1, acc[at]);
                io_row_tail(row, pos, true, 0u);
                if constexpr (COMMIT) io_commit_tail(row, jpos);
                if (ok && pos - pos_start < n_rows) {
                    const uint32_t t[RK_RV32LINK_TUPLE] = {row[Q_PL], row[Q_PH], row[Q_V_LO], row[Q_V_HI], 0u, 0u};
                    for (unsigned j = 0; j < RK_RV32LINK_TUPLE; j++) stream[(size_t)(pos - pos_start) * RK_RV32LINK_TUPLE + j] = enc(t[j]);
                }
            }
            if (!ok) atomicOr(err, 256u);
        } else {
            if constexpr (COMMIT) {
                io_row_tail(row, cm.pos_end, false, halted);
                io_commit_tail(row, cm.jpos_end);
            } else {
                io_row_tail(row, pos_start + (total - (uint32_t)count), false, halted);
            }
        }
        for (unsigned c : IO_RANGE_ACT) hist_add(hist, row[c], on);
        for (unsigned c : IO_RANGE_READ) hist_add(hist, row[c], read);
        for (unsigned c : IO_RANGE_HEAD) hist_add(hist, row[c], head);
        for (unsigned c : IO_RANGE_WORD) hist_add(hist, row[c], word);
        if constexpr (COMMIT) {
            for (unsigned c : IO_RANGE_COMMIT) hist_add(hist, row[c], chead && row[c] < (1u << 16));
            for (unsigned c : IO_RANGE_CW) hist_add(hist, row[c], cw);
        }
    });
}

// ---- the link between shard memories (raiko_amd/rv32link.py): from a finished memory table, one lane per row.  The
// block's rows come in as whole lines through LDS (stride 13: odd); a lane decodes its row's six limbs and REAL, writes
// the link row (the six limbs as they are, Montgomery; zeros on a padding row) and the journal row (word address, INIT,
// FINAL, canonical; zeros likewise) into LDS, and both tiles leave as whole lines.  A block's count of real rows is one
// __syncthreads_count.  err |= 128: REAL is not boolean, a real row follows a padding row (lane 0 of a later block reads
// the row before its tile from HBM), or a limb of a real row is no 16-bit (WL: 14-bit) value.
static_assert(B_WL == 0 && B_F_HI + 1 == RK_RV32LINK_TUPLE, "the link tuple is the memory row's first six cells");
__global__ void __launch_bounds__(TB) mem_journal_kernel(const uint32_t* __restrict__ mem, uint32_t* __restrict__ journal,
                                                          uint32_t* __restrict__ link, uint32_t* __restrict__ count,
                                                          uint32_t* __restrict__ err) {
    constexpr unsigned LW = RK_RV32LINK_TUPLE, LS = LW | 1, JW = 3;
    __shared__ uint32_t s_in[TB * BD_W], s_link[TB * LS], s_j[TB * JW];
    const unsigned nb = blockDim.x;
    const size_t r0 = (size_t)blockIdx.x * nb;
    for (unsigned k = threadIdx.x; k < nb * BD_W; k += nb) s_in[k] = mem[r0 * BD_W + k];
    __syncthreads();
    const uint32_t* row = s_in + threadIdx.x * BD_W;
    const uint32_t real = bb::decode(row[B_REAL]);
    const uint32_t prev = threadIdx.x ? bb::decode(s_in[(threadIdx.x - 1) * BD_W + B_REAL])
                                      : (r0 ? bb::decode(mem[(r0 - 1) * BD_W + B_REAL]) : 1u);
    uint32_t c[LW];
    uint32_t over = 0;
#pragma unroll
    for (unsigned j = 0; j < LW; j++) {
        c[j] = bb::decode(row[B_WL + j]);
        over |= c[j] >> 16;
    }
    over |= c[B_WL] >> 14;
    const bool on = real == 1;
    if (real > 1 || (on && (prev != 1 || over))) atomicOr(err, 128u);
#pragma unroll
    for (unsigned j = 0; j < LW; j++) s_link[threadIdx.x * LS + j] = on ? row[B_WL + j] : 0u;
    s_j[threadIdx.x * JW + 0] = on ? (c[B_WL] | c[B_WH] << 14) : 0u;
    s_j[threadIdx.x * JW + 1] = on ? (c[B_I_LO] | c[B_I_HI] << 16) : 0u;
    s_j[threadIdx.x * JW + 2] = on ? (c[B_F_LO] | c[B_F_HI] << 16) : 0u;
    const int n_real = __syncthreads_count(on);
    if (threadIdx.x == 0 && n_real) atomicAdd(count, (uint32_t)n_real);
    for (unsigned k = threadIdx.x; k < nb * LW; k += nb) link[r0 * LW + k] = s_link[(k / LW) * LS + k % LW];
    for (unsigned k = threadIdx.x; k < nb * JW; k += nb) journal[r0 * JW + k] = s_j[k];
}

static size_t program_rows_of(const ExecSegmentView& v, uint32_t* n_slots) {
    const uint32_t slots = v.trace->empty() ? 0 : (v.pc_hi - v.pc_lo) / 4 + 1;
    size_t rows = 2;
    while (rows < slots) rows <<= 1;
    if (n_slots) *n_slots = slots;
    return rows;
}

// the rows of a segment's trace with M_W = 1 (an M word writing a register other than x0): its muldiv rows
static size_t m_count_of(const ExecSegmentView& v) {
    size_t c = 0;   // decode(ins).is_m && decode(ins).wr: opcode OP, funct7 = 1, rd != 0
    for (const TraceRow& r : *v.trace) c += (r.ins & 0xfe00007fu) == 0x02000033u && (r.ins & 0xf80u);
    return c;
}

// the program table's rows over an image of n_words words
static size_t image_rows_for(size_t n_words) {
    size_t rows = 2;
    while (rows < n_words) rows <<= 1;
    return rows;
}

// the caller's segment table as the kernels take it -> the image's words; RK_ERR_INVALID for more than
// RK_RV32ELF_MAX_SEGMENTS segments
static int image_of(const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs, Image* img, size_t* n_words) {
    if (n_segs > RK_RV32ELF_MAX_SEGMENTS || (n_segs && (!seg_vaddr || !seg_words))) return RK_ERR_INVALID;
    *img = Image{};
    img->n_segs = n_segs;
    *n_words = 0;
    for (uint32_t k = 0; k < n_segs; k++) {
        img->vaddr[k] = seg_vaddr[k];
        img->words[k] = seg_words[k];
        *n_words += seg_words[k];
    }
    return RK_OK;
}

static size_t muldiv_rows_for(size_t count) {
    size_t rows = (size_t)1 << RK_RV32IM_MULDIV_MIN_LOG_ROWS;
    while (rows < count) rows <<= 1;
    return rows;
}

// the io form: the words the segment's READ ecalls stored (the access list's entries at ecall rows), the io table's rows
static size_t io_words_of(const ExecSegmentView& v) {
    size_t c = 0;
    for (const auto& m : *v.mem) c += m[0] < v.trace->size() && (*v.trace)[m[0]].ins == ECALL_WORD;
    return c;
}
static size_t io_rows_for(size_t count) {
    size_t rows = 2;
    while (rows < count) rows <<= 1;
    return rows;
}

// the commit form: the access list memop and the memory table see (merge_accesses), and its distinct word addresses
static std::vector<std::array<uint32_t, 4>> merged_list(const ExecSegmentView& v) {
    static_assert(sizeof(MemAccess) == sizeof(std::array<uint32_t, 4>), "an access is four words, as the executor records it");
    std::vector<std::array<uint32_t, 4>> out(v.mem->size() + v.commit_reads->size());
    merge_accesses((const MemAccess*)v.mem->data(), v.mem->size(), (const MemAccess*)v.commit_reads->data(), v.commit_reads->size(),
                   (MemAccess*)out.data());
    return out;
}
static size_t distinct_words(const std::vector<std::array<uint32_t, 4>>& list) {
    std::vector<uint32_t> a;
    a.reserve(list.size());
    for (const auto& m : list) a.push_back(m[1]);
    std::sort(a.begin(), a.end());
    return (size_t)(std::unique(a.begin(), a.end()) - a.begin());
}

// rv32im-mem: the memop / memory table's rows for `count` accesses / distinct words
static size_t mem_rows_for(size_t count) {
    size_t rows = (size_t)1 << RK_RV32MEM_MIN_LOG_ROWS;
    while (rows < count) rows <<= 1;
    return rows;
}

namespace {

// the tables a shard's driver writes: rv32i's five, d_shift the sixth of rv32i-cf, d_muldiv (muldiv_rows rows) the
// seventh of rv32im.  rv32im-elf: program / byte / range / shift are the count columns, img / image_words (device, n_words
// of them) the program image the cycles are counted against
struct ShardOut {
    uint32_t *cpu, *program;
    size_t program_rows;
    uint32_t *reg, *byte, *range, *shift, *muldiv;
    size_t muldiv_rows;
    Image img;
    const uint32_t* image_words;
    size_t n_words;
    uint32_t* memop = nullptr;   // rv32im-mem
    size_t memop_rows = 0;
    uint32_t* memory = nullptr;
    size_t memory_rows = 0;
    uint32_t* io = nullptr;      // the io form
    size_t io_rows = 0;
    uint32_t* h_publics = nullptr;
    uint32_t* log = nullptr;     // the commit form: the commit log (io_rows x 3, canonical) and its rows
    size_t* n_log = nullptr;
};

// the driver's scratch: one allocation, each part's offset in words from one take(), rounded to 64 words
struct Scratch {
    size_t words = 0;
    size_t take(size_t w) {
        const size_t at = words;
        words += (w + 63) & ~(size_t)63;
        return at;
    }
    size_t tr, ec, wval, acc, blk, final_ts, fin, init;
    size_t err, hist, bmult, pmult, pins, smult, clear_end;   // [err, clear_end): zero before the first kernel
    size_t mflag, mblk, mtotal, midx;                          // rv32im
    size_t macc, mkeys, mvals, mkeys2, mvals2, mpts, necw, hblk, htotal;   // rv32im-mem
    size_t eargs, eoff, eblk, etotal, stream, nodes;                       // the io form
    size_t creads, coff, cblk, ctotal, joff, jblk, jtotal, clog, cnodes;   // the commit form
    Scratch(bool cf, bool im, bool elf, bool mem, size_t cycles, size_t n_ecalls, size_t n, uint32_t n_slots, size_t m_count,
            size_t mem_count, size_t io_rows = 0, bool commit = false, size_t n_reads = 0) {
        const size_t nb = n / TB, slots = std::max<uint32_t>(n_slots, 1), sw = cf ? SHIFT_USED : 1u;
        tr = take((std::max<size_t>(cycles, 1) * sizeof(TraceRow) + 3) / 4);
        ec = take(2 * std::max<size_t>(n_ecalls, 1));
        wval = take(n);
        acc = take(n);
        blk = take(nb * 32);
        final_ts = take(32);
        fin = take(32);
        init = take(32);
        err = take(1);
        hist = take((size_t)1 << 16);
        bmult = take((size_t)3 << 16);
        pmult = take(slots);
        pins = take(elf ? 1 : slots);   // rv32im-elf compares with the image: no word is recorded
        smult = take(sw);
        clear_end = smult + sw;
        mflag = take(im ? n : 1);
        mblk = take(im ? nb : 1);
        mtotal = take(1);
        midx = take(std::max<size_t>(m_count, 1));
        macc = mkeys = mvals = mkeys2 = mvals2 = mpts = necw = hblk = htotal = 0;
        if (mem) {
            const size_t mc = std::max<size_t>(mem_count, 1);
            macc = take(4 * mc);
            mkeys = take(mc);
            mvals = take(mc);
            mkeys2 = take(mc);
            mvals2 = take(mc);
            mpts = take(mc);
            necw = take(n);
            hblk = take((mc + TB - 1) / TB);
            htotal = take(1);
        }
        eargs = eoff = eblk = etotal = stream = nodes = 0;
        if (io_rows) {
            const size_t ne = std::max<size_t>(n_ecalls, 1);
            eargs = take(5 * ne);
            eoff = take(ne);
            eblk = take((ne + TB - 1) / TB);
            etotal = take(1);
            stream = take(io_rows * RK_RV32LINK_TUPLE);
            nodes = take(2 * io_rows * 8);
        }
        creads = coff = cblk = ctotal = joff = jblk = jtotal = clog = cnodes = 0;
        if (io_rows && commit) {
            const size_t ne = std::max<size_t>(n_ecalls, 1);
            creads = take(4 * std::max<size_t>(n_reads, 1));
            coff = take(ne);
            cblk = take((ne + TB - 1) / TB);
            ctotal = take(1);
            joff = take(ne);
            jblk = take((ne + TB - 1) / TB);
            jtotal = take(1);
            clog = take(io_rows * RK_RV32LINK_TUPLE);
            cnodes = take(2 * io_rows * 8);
        }
    }
};

}  // namespace

// the copies and the launches of one shard, in stream order; returns at the first error
template <int CS>
static int shard_enqueue(rk_ctx* ctx, const ExecSegmentView& v, const ShardOut& o, const Scratch& L, uint32_t* w,
                         const std::vector<uint32_t>& ec_flat, uint32_t n_slots, size_t m_count, void* sort_tmp, size_t sort_bytes) {
    using CH = Chips<CS>;
    constexpr int RCS = CH::commit ? (int)CS_IO : CS;   // the commit form's cpu rows are the io form's: one instantiation
    const std::vector<TraceRow>& tr = *v.trace;
    const size_t n = (size_t)1 << v.seg->po2, nb = n / TB;
    const TraceRow* d_tr = (const TraceRow*)(w + L.tr);
    uint32_t *wval = w + L.wval, *acc = w + L.acc, *blk = w + L.blk, *final_ts = w + L.final_ts, *init = w + L.init,
             *err = w + L.err, *hist = w + L.hist, *bmult = w + L.bmult, *pmult = w + L.pmult, *pins = w + L.pins,
             *smult = w + L.smult, *mflag = w + L.mflag, *mblk = w + L.mblk, *midx = w + L.midx;
    if (!tr.empty()) RK_HIP_TRY(ctx, hipMemcpyAsync(w + L.tr, tr.data(), tr.size() * sizeof(TraceRow), hipMemcpyHostToDevice, ctx->stream));
    if (!ec_flat.empty()) RK_HIP_TRY(ctx, hipMemcpyAsync(w + L.ec, ec_flat.data(), ec_flat.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    RK_HIP_TRY(ctx, hipMemcpyAsync(init, v.regs, 32 * 4, hipMemcpyHostToDevice, ctx->stream));
    RK_HIP_TRY(ctx, hipMemsetAsync(err, 0, (L.clear_end - L.err) * 4, ctx->stream));
    ImageArgs<CH::elf> image;
    if constexpr (CH::elf) image = {o.img, o.image_words};
    const size_t n_ec = CH::io ? v.ecall_args->size() : 0;
    const EcallArg* eargs = (const EcallArg*)(w + L.eargs);
    if constexpr (CH::io) {   // the io form of the trace: an ecall row's a / b / res are the call's a0 / a1 / t0
        static_assert(sizeof(EcallArg) == sizeof((*v.ecall_args)[0]), "an entry is five words, as the executor records it");
        if (n_ec) {
            RK_HIP_TRY(ctx, hipMemcpyAsync(w + L.eargs, v.ecall_args->data(), n_ec * sizeof(EcallArg), hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(io_patch_kernel, dim3((unsigned)((n_ec + TB - 1) / TB)), dim3(TB), 0, ctx->stream, (TraceRow*)(w + L.tr),
                               tr.size(), eargs, n_ec, err);
            RK_TRY(rk::post_launch(ctx, "rv32 io_patch_kernel"));
        }
    }
    hipLaunchKernelGGL((prep_kernel<CH::elf, CH::io>), dim3((unsigned)nb), dim3(TB), 0, ctx->stream, d_tr, tr.size(), n, w + L.ec,
                       (uint32_t)ec_flat.size() / 2, v.pc_lo, n_slots, wval, acc, pmult, pins, err, CH::im ? mflag : nullptr, image);
    RK_TRY(rk::post_launch(ctx, "rv32 prep_kernel"));
    const size_t mem_count = CH::mem ? v.mem->size() : 0;
    const MemAccess* macc = (const MemAccess*)(w + L.macc);
    if constexpr (CH::mem) {   // the sorted access list, each access's predecessor and the boundary rows (before rows_kernel: necw)
        static_assert(sizeof(MemAccess) == 16, "an access is four words, as the executor records it");
        RK_HIP_TRY(ctx, hipMemsetAsync(w + L.necw, 0, ((size_t)1 << v.seg->po2) * 4, ctx->stream));
        RK_HIP_TRY(ctx, hipMemsetAsync(w + L.htotal, 0, 4, ctx->stream));
        RK_HIP_TRY(ctx, hipMemsetAsync(o.memory, 0, o.memory_rows * BD_W * 4, ctx->stream));   // the rows past the touched words
        if (mem_count) {
            RK_HIP_TRY(ctx, hipMemcpyAsync(w + L.macc, v.mem->data(), mem_count * sizeof(MemAccess), hipMemcpyHostToDevice, ctx->stream));
            const unsigned kb = (unsigned)((mem_count + TB - 1) / TB);
            hipLaunchKernelGGL(mem_keys_kernel, dim3(kb), dim3(TB), 0, ctx->stream, macc, mem_count, d_tr, w + L.mkeys, w + L.mvals, w + L.necw);
            RK_TRY(rk::post_launch(ctx, "rv32 mem_keys_kernel"));
            size_t bytes = sort_bytes;
            RK_HIP_TRY(ctx, rocprim::radix_sort_pairs(sort_tmp, bytes, w + L.mkeys, w + L.mkeys2, w + L.mvals, w + L.mvals2, mem_count, 0, 30,
                                                      ctx->stream));
            hipLaunchKernelGGL(mhead_count_kernel, dim3(kb), dim3(TB), 0, ctx->stream, w + L.mkeys2, mem_count, w + L.hblk);
            RK_TRY(rk::post_launch(ctx, "rv32 mhead_count_kernel"));
            hipLaunchKernelGGL(mscan_kernel, dim3(1), dim3(1024), 0, ctx->stream, w + L.hblk, (size_t)kb, w + L.htotal);
            RK_TRY(rk::post_launch(ctx, "rv32 mscan_kernel"));
            hipLaunchKernelGGL(mem_link_kernel, dim3(kb), dim3(TB), 0, ctx->stream, w + L.mkeys2, w + L.mvals2, macc, mem_count, w + L.hblk,
                               w + L.mpts, o.memory, o.memory_rows, hist, err);
            RK_TRY(rk::post_launch(ctx, "rv32 mem_link_kernel"));
        }
    }
    hipLaunchKernelGGL(block_last_kernel, dim3((unsigned)nb), dim3(TB), 0, ctx->stream, acc, blk);
    RK_TRY(rk::post_launch(ctx, "rv32 block_last_kernel"));
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, blk, nb, final_ts);
    RK_TRY(rk::post_launch(ctx, "rv32 scan_kernel"));
    const size_t lds = TB * (CH::cpu_w | 1) * 4;
    if (lds > 64 * 1024)   // rv32im's 133-word rows: past the default dynamic LDS limit (160 KiB per CU)
        RK_HIP_TRY(ctx, hipFuncSetAttribute((const void*)rows_kernel<RCS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(rows_kernel<RCS>, dim3((unsigned)nb), dim3(TB), lds, ctx->stream, d_tr, tr.size(), v.seg->end_pc, acc, wval,
                       blk, init, o.cpu, hist, bmult, smult, w + L.necw, n);
    RK_TRY(rk::post_launch(ctx, "rv32 rows_kernel"));
    if (CH::im) {   // the muldiv rows: count per block, scan, compact, then one lane per row (before the byte / range /
                    // shift tables: its counts go into theirs)
        hipLaunchKernelGGL(mcount_kernel, dim3((unsigned)nb), dim3(TB), 0, ctx->stream, mflag, mblk);
        RK_TRY(rk::post_launch(ctx, "rv32 mcount_kernel"));
        hipLaunchKernelGGL(mscan_kernel, dim3(1), dim3(1024), 0, ctx->stream, mblk, nb, w + L.mtotal);
        RK_TRY(rk::post_launch(ctx, "rv32 mscan_kernel"));
        hipLaunchKernelGGL(mcompact_kernel, dim3((unsigned)nb), dim3(TB), 0, ctx->stream, mflag, mblk, m_count, midx);
        RK_TRY(rk::post_launch(ctx, "rv32 mcompact_kernel"));
        const unsigned b = (unsigned)std::min<size_t>(o.muldiv_rows, TB);
        hipLaunchKernelGGL(muldiv_kernel, dim3((unsigned)(o.muldiv_rows / b)), dim3(b), b * (MD_W | 1) * 4, ctx->stream, d_tr,
                           tr.size(), wval, midx, m_count, o.muldiv_rows, o.muldiv, hist, bmult, smult, err);
        RK_TRY(rk::post_launch(ctx, "rv32 muldiv_kernel"));
    }
    if constexpr (CH::mem) {   // one lane per memop row (before the count columns: its counts go into theirs)
        const unsigned b = (unsigned)std::min<size_t>(o.memop_rows, TB);
        hipLaunchKernelGGL(memop_kernel<CH::mo_w>, dim3((unsigned)(o.memop_rows / b)), dim3(b), b * (CH::mo_w | 1) * 4, ctx->stream, d_tr, wval, macc,
                           w + L.mpts, mem_count, o.memop_rows, o.memop, hist, bmult, smult, err, CH::io ? 1u : 0u);
        RK_TRY(rk::post_launch(ctx, "rv32 memop_kernel"));
    }
    if constexpr (CH::io) {   // the io rows (before the count columns: its counts go into the range table's), then the digest
        const uint32_t total = (uint32_t)(n_ec + io_words_of(v));   // the commit form: v.mem is the merged list
        RK_HIP_TRY(ctx, hipMemsetAsync(w + L.stream, 0, o.io_rows * RK_RV32LINK_TUPLE * 4, ctx->stream));
        CommitScanOf<CH::commit> scan;
        CommitRowsOf<CH::commit> cm;
        if constexpr (CH::commit) {
            static_assert(sizeof(MemAccess) == sizeof((*v.commit_reads)[0]), "a commit read is four words, as the executor records it");
            const size_t n_reads = v.commit_reads->size();
            uint32_t bytes = 0;
            for (const auto& e : *v.ecall_args) bytes += e[1] == 2 ? e[3] : 0u;
            RK_HIP_TRY(ctx, hipMemsetAsync(w + L.clog, 0, o.io_rows * RK_RV32LINK_TUPLE * 4, ctx->stream));
            RK_HIP_TRY(ctx, hipMemsetAsync(o.log, 0, o.io_rows * 3 * 4, ctx->stream));
            if (n_reads)
                RK_HIP_TRY(ctx, hipMemcpyAsync(w + L.creads, v.commit_reads->data(), n_reads * sizeof(MemAccess), hipMemcpyHostToDevice, ctx->stream));
            scan.coff = w + L.coff, scan.cblk = w + L.cblk, scan.joff = w + L.joff, scan.jblk = w + L.jblk;
            cm.reads = (const MemAccess*)(w + L.creads), cm.n_reads = (uint32_t)n_reads;
            cm.coff = scan.coff, cm.cblk = scan.cblk, cm.joff = scan.joff, cm.jblk = scan.jblk;
            cm.jpos_start = v.jpos_start, cm.jpos_end = v.jpos_start + bytes;
            cm.pos_end = v.in_start + (uint32_t)(total - n_ec - n_reads);
            cm.clog = w + L.clog, cm.dlog = o.log;
        }
        if (n_ec) {
            const unsigned eb = (unsigned)((n_ec + TB - 1) / TB);
            hipLaunchKernelGGL(io_offsets_kernel<CH::commit>, dim3(eb), dim3(TB), 0, ctx->stream, eargs, n_ec, w + L.necw, w + L.eoff,
                               w + L.eblk, scan);
            RK_TRY(rk::post_launch(ctx, "rv32 io_offsets_kernel"));
            hipLaunchKernelGGL(mscan_kernel, dim3(1), dim3(1024), 0, ctx->stream, w + L.eblk, (size_t)eb, w + L.etotal);
            RK_TRY(rk::post_launch(ctx, "rv32 mscan_kernel"));
            if constexpr (CH::commit) {
                hipLaunchKernelGGL(mscan_kernel, dim3(1), dim3(1024), 0, ctx->stream, w + L.cblk, (size_t)eb, w + L.ctotal);
                RK_TRY(rk::post_launch(ctx, "rv32 mscan_kernel"));
                hipLaunchKernelGGL(mscan_kernel, dim3(1), dim3(1024), 0, ctx->stream, w + L.jblk, (size_t)eb, w + L.jtotal);
                RK_TRY(rk::post_launch(ctx, "rv32 mscan_kernel"));
            }
        }
        const unsigned b = (unsigned)std::min<size_t>(o.io_rows, TB);
        hipLaunchKernelGGL(io_rows_kernel<CH::commit>, dim3((unsigned)(o.io_rows / b)), dim3(b), b * (CH::io_w | 1) * 4, ctx->stream, eargs,
                           n_ec, w + L.ec, w + L.necw, w + L.eoff, w + L.eblk, macc, mem_count, (uint32_t)v.n_input, v.in_start, total,
                           o.io_rows, o.io, w + L.stream, hist, err, cm);
        RK_TRY(rk::post_launch(ctx, "rv32 io_rows_kernel"));
        const rk_matrix m{w + L.stream, (uint32_t)o.io_rows, RK_RV32LINK_TUPLE, 1};
        RK_TRY(rk_mmcs_commit(ctx, &m, 1, w + L.nodes, o.h_publics + 6));
        if constexpr (CH::commit) {
            const rk_matrix cl{w + L.clog, (uint32_t)o.io_rows, RK_RV32LINK_TUPLE, 1};
            RK_TRY(rk_mmcs_commit(ctx, &cl, 1, w + L.cnodes, o.h_publics + RK_RV32IO_PUBLICS + 2));
        }
    }
    if constexpr (CH::elf) {   // the tuples are in the key: each lookup table's trace is its count column
        const struct { const uint32_t* counts; size_t n_counts, n_rows; uint32_t* out; } cols[4] = {
            {pmult, n_slots, o.program_rows, o.program}, {bmult, (size_t)3 << 16, (size_t)1 << RK_RV32_BYTE_LOG_ROWS, o.byte},
            {hist, (size_t)1 << 16, (size_t)1 << 16, o.range}, {smult, SHIFT_USED, (size_t)1 << RK_RV32CF_SHIFT_LOG_ROWS, o.shift}};
        for (const auto& c : cols) {
            hipLaunchKernelGGL(count_kernel, dim3((unsigned)((c.n_rows + 255) / 256)), dim3(256), 0, ctx->stream, c.counts, c.n_counts,
                               c.n_rows, c.out);
            RK_TRY(rk::post_launch(ctx, "rv32 count_kernel"));
        }
    } else {
        const unsigned pb = (unsigned)std::min<size_t>(o.program_rows, TB);
        hipLaunchKernelGGL(program_kernel<CS>, dim3((unsigned)((o.program_rows + pb - 1) / pb)), dim3(pb), pb * (CH::prog_w | 1) * 4,
                           ctx->stream, pins, pmult, n_slots, v.pc_lo, o.program_rows, o.program);
        RK_TRY(rk::post_launch(ctx, "rv32 program_kernel"));
        hipLaunchKernelGGL(byte_kernel, dim3((1u << RK_RV32_BYTE_LOG_ROWS) / TB), dim3(TB), TB * (BYTE_W | 1) * 4, ctx->stream,
                           bmult, o.byte);
        RK_TRY(rk::post_launch(ctx, "rv32 byte_kernel"));
        hipLaunchKernelGGL(range_kernel, dim3((1u << 16) / TB), dim3(TB), 0, ctx->stream, hist, o.range);
        RK_TRY(rk::post_launch(ctx, "rv32 range_kernel"));
    }
    hipLaunchKernelGGL(register_kernel, dim3(1), dim3(32), 32 * (REG_W | 1) * 4, ctx->stream, final_ts, init, d_tr, wval,
                       w + L.fin, o.reg, CH::io ? 1u : 0u);
    RK_TRY(rk::post_launch(ctx, "rv32 register_kernel"));
    if (CH::cf && !CH::elf) {   // after rows_kernel (and muldiv_kernel) on the stream: the counts are complete
        hipLaunchKernelGGL(shift_kernel, dim3((1u << RK_RV32CF_SHIFT_LOG_ROWS) / TB), dim3(TB), TB * (SHIFT_W | 1) * 4,
                           ctx->stream, smult, o.shift);
        RK_TRY(rk::post_launch(ctx, "rv32 shift_kernel"));
    }
    return RK_OK;
}

// One shard's tables.  Owns the scratch block and the host staging of the ecall list: whatever shard_enqueue returns, the
// read-backs are queued and the stream is drained before either goes, so no queued copy outlives its host buffer and the
// scratch is never returned with work in flight.
template <int CS>
static int shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, const ShardOut& o) {
    using CH = Chips<CS>;
    if (!ctx || !o.cpu || !o.program || !o.reg || !o.byte || !o.range || (CH::cf && !o.shift) || (CH::im && !o.muldiv) ||
        (CH::mem && (!o.memop || !o.memory)) || (CH::io && (!o.io || !o.h_publics)) || (CH::commit && (!o.log || !o.n_log)))
        return RK_ERR_INVALID;
    ExecSegmentView v;
    RK_TRY(exec_segment_view(ex, index, &v));
    const ExecSegmentView vu = v;   // as the executor recorded it; the commit form's v.mem is the merged list
    std::vector<std::array<uint32_t, 4>> merged;
    if (CH::commit) {
        merged = merged_list(v);
        v.mem = &merged;
    }
    const size_t cycles = v.trace->size(), n = (size_t)1 << v.seg->po2;
    if (cycles > n || n % TB) return RK_ERR_INTERNAL;
    uint32_t n_slots = 0;
    if (CH::elf) {   // one slot per word of the image
        if (!o.image_words && o.n_words) return RK_ERR_INVALID;
        if (o.n_words > (1u << 22) || image_rows_for(o.n_words) != o.program_rows) return RK_ERR_CAPACITY;
        n_slots = (uint32_t)o.n_words;
    } else if (program_rows_of(v, &n_slots) != o.program_rows) {
        return RK_ERR_CAPACITY;
    }
    if (n_slots > (1u << 22)) {
        ctx->last_error = "rk_exec_rv32_shard_device: executed pc range wider than 2^22 words";
        return RK_ERR_CAPACITY;
    }
    const size_t m_count = CH::im ? m_count_of(v) : 0;
    if (CH::im) {   // a power of two that holds every muldiv row, no taller than the cpu table; nothing is written otherwise
        if (o.muldiv_rows < muldiv_rows_for(m_count)) {
            ctx->last_error = "rk_exec_rv32im_shard_device: the muldiv table has fewer rows than the segment needs";
            return RK_ERR_CAPACITY;
        }
        if (o.muldiv_rows & (o.muldiv_rows - 1) || o.muldiv_rows > std::max<size_t>(n, muldiv_rows_for(0))) return RK_ERR_INVALID;
    }
    const size_t mem_count = CH::mem ? v.mem->size() : 0,
                 mem_words = CH::commit ? distinct_words(merged) : CH::mem ? exec_mem_words(ex, index) : 0;
    if (CH::mem) {   // powers of two that hold every row, at most twice the cpu table; nothing is written otherwise
        const struct { size_t rows, need; const char* what; } t[2] = {{o.memop_rows, mem_rows_for(mem_count), "memop"},
                                                                      {o.memory_rows, mem_rows_for(mem_words), "memory"}};
        for (const auto& c : t)
            if (c.rows < c.need || c.rows & (c.rows - 1) || c.rows > 2 * n) {
                ctx->last_error = std::string("rk_exec_rv32mem_shard_device: the ") + c.what + " table's rows are not a power of two from what the segment needs up to twice the cpu table's";
                return RK_ERR_INVALID;
            }
        static_assert(sizeof(MemAccess) == sizeof((*v.mem)[0]), "an access is four words, as the executor records it");
        if (!mem_list_ok(v.trace->data(), cycles, (const MemAccess*)v.mem->data(), mem_count)) {
            ctx->last_error = "rk_exec_rv32mem_shard_device: the access list is not in cycle order or is not the trace's loads, stores and ecalls";
            return RK_ERR_INVALID;
        }
    }
    if (CH::io) {   // a power of two >= 2 that holds every row, at most twice the cpu table; the side list the trace's ecalls
        const size_t need = io_rows_for(v.ecall_args->size() + io_words_of(v));
        if (o.io_rows < 2 || o.io_rows & (o.io_rows - 1) || o.io_rows > 2 * n) {
            ctx->last_error = "rk_exec_rv32io_shard_device: the io table's rows are not a power of two from 2 up to twice the cpu table's";
            return RK_ERR_INVALID;
        }
        if (o.io_rows < need) {
            ctx->last_error = "rk_exec_rv32io_shard_device: the io table has fewer rows than the segment needs";
            return RK_ERR_CAPACITY;
        }
        if (v.n_input >= ((size_t)1 << 30)) {
            ctx->last_error = "rk_exec_rv32io_shard_device: an input of 2^30 words or more";
            return RK_ERR_CAPACITY;
        }
        static_assert(sizeof(EcallArg) == sizeof((*v.ecall_args)[0]), "an entry is five words, as the executor records it");
        if (v.ecall_args->size() != v.ecalls->size() ||
            !io_list_ok(v.trace->data(), cycles, (const EcallArg*)v.ecall_args->data(), v.ecall_args->size())) {
            ctx->last_error = "rk_exec_rv32io_shard_device: the ecall side list is not the trace's ecall rows in cycle order";
            return RK_ERR_INVALID;
        }
    }
    if (CH::commit) {   // the commit reads are the words of the trace's COMMITs; the journal stays below 2^30 bytes
        uint64_t bytes = vu.jpos_start;
        for (const auto& e : *vu.ecall_args) bytes += e[1] == 2 ? e[3] : 0u;
        if (bytes >= ((uint64_t)1 << 30) ||
            !commit_list_ok((const EcallArg*)vu.ecall_args->data(), vu.ecall_args->size(), (const MemAccess*)vu.commit_reads->data(),
                            vu.commit_reads->size(), (const MemAccess*)vu.mem->data(), vu.mem->size())) {
            ctx->last_error = "rk_exec_rv32commit_shard_device: the commit reads are not the words of the trace's COMMITs in cycle order";
            return RK_ERR_INVALID;
        }
    }
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const Scratch L(CH::cf, CH::im, CH::elf, CH::mem, cycles, v.ecalls->size(), n, n_slots, m_count, mem_count, CH::io ? o.io_rows : 0,
                    CH::commit, CH::commit ? v.commit_reads->size() : 0);
    rk::DevBuf sort_tmp;   // rocPRIM's temporary storage for the sort of mem_count pairs
    size_t sort_bytes = 0;
    if (mem_count) {
        RK_HIP_TRY(ctx, rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                                  (uint32_t*)nullptr, mem_count, 0, 30, ctx->stream));
        RK_TRY(sort_tmp.alloc(ctx, std::max<size_t>(sort_bytes, 4)));
    }
    void* base = nullptr;
    RK_TRY(rk::dev_alloc(ctx, L.words * 4, &base));
    uint32_t* w = (uint32_t*)base;
    std::vector<uint32_t> ec_flat(2 * v.ecalls->size());
    for (size_t k = 0; k < v.ecalls->size(); k++) ec_flat[2 * k] = (*v.ecalls)[k][0], ec_flat[2 * k + 1] = (*v.ecalls)[k][1];
    int st = shard_enqueue<CS>(ctx, v, o, L, w, ec_flat, n_slots, m_count, sort_tmp.p, sort_bytes);
    // the tables are complete and the scratch can go: read back the final registers and the error flags
    uint32_t host_fin[35] = {0};
    auto hip = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && st == RK_OK) {
            ctx->last_error = std::string("rk_exec_rv32_shard_device ") + what + ": " + hipGetErrorString(e);
            st = RK_ERR_HIP;
        }
    };
    hip(hipMemcpyAsync(host_fin, w + L.fin, 32 * 4, hipMemcpyDeviceToHost, ctx->stream), "d2h");
    hip(hipMemcpyAsync(host_fin + 32, w + L.err, 4, hipMemcpyDeviceToHost, ctx->stream), "d2h");
    if (CH::im) hip(hipMemcpyAsync(host_fin + 33, w + L.mtotal, 4, hipMemcpyDeviceToHost, ctx->stream), "d2h");
    if (CH::mem && mem_count) hip(hipMemcpyAsync(host_fin + 34, w + L.htotal, 4, hipMemcpyDeviceToHost, ctx->stream), "d2h");
    hip(hipStreamSynchronize(ctx->stream), "sync");
    rk::dev_free(ctx, base);
    if (st != RK_OK) return st;
    if (CH::io) {
        if (host_fin[32] & 256) {
            ctx->last_error = "rk_exec_rv32io_shard_device: the ecall side list is not the trace's ecalls";
            return RK_ERR_INVALID;
        }
        const auto& ea = *v.ecall_args;
        const bool halted = !ea.empty() && ea.back()[1] == 0;
        const uint32_t exit_code = halted ? ea.back()[2] : 0u;
        const uint32_t pub[6] = {v.in_start, v.in_start + (uint32_t)io_words_of(vu), (uint32_t)v.n_input, halted ? 1u : 0u,
                                 exit_code & 0xffffu, exit_code >> 16};
        for (unsigned j = 0; j < 6; j++) o.h_publics[j] = enc(pub[j]);
        if (CH::commit) {
            if (host_fin[32] & 512) {
                ctx->last_error = "rk_exec_rv32commit_shard_device: a commit read is not the word of its call";
                return RK_ERR_INVALID;
            }
            uint32_t bytes = 0;
            for (const auto& e : ea) bytes += e[1] == 2 ? e[3] : 0u;
            o.h_publics[RK_RV32IO_PUBLICS] = enc(v.jpos_start);
            o.h_publics[RK_RV32IO_PUBLICS + 1] = enc(v.jpos_start + bytes);
            *o.n_log = v.commit_reads->size();
        }
    }
    if (CH::mem && (host_fin[32] & 32)) {
        ctx->last_error = "rk_exec_rv32mem_shard_device: an access is not the one its instruction names";
        return RK_ERR_INTERNAL;
    }
    if (CH::mem && ((host_fin[32] & 64) || host_fin[34] != mem_words)) {
        ctx->last_error = "rk_exec_rv32mem_shard_device: the distinct words on the device are not the host's";
        return RK_ERR_INTERNAL;
    }
    if (host_fin[32] & 7) {
        if (CH::elf && (host_fin[32] & 5))
            ctx->last_error = host_fin[32] & 1 ? "rk_exec_rv32elf_shard_device: an executed word is not the program image's word at its pc"
                                               : "rk_exec_rv32elf_shard_device: a pc executed outside the program image";
        else
            ctx->last_error = host_fin[32] & 1 ? "rk_exec_rv32_shard_device: a pc executed with two instruction words in one shard"
                                               : "rk_exec_rv32_shard_device: trace and side list disagree";
        return RK_ERR_INVALID;
    }
    if (CH::im && (host_fin[32] || host_fin[33] != m_count)) {
        ctx->last_error = "rk_exec_rv32im_shard_device: an M result or the muldiv row count is not the executor's";
        return RK_ERR_INTERNAL;
    }
    if (!std::equal(host_fin, host_fin + 32, v.regs + 32)) {
        ctx->last_error = "rk_exec_rv32_shard_device: the register accesses do not end in the executor's registers";
        return RK_ERR_INTERNAL;
    }
    return RK_OK;
}

// the four preprocessed matrices of an image (rk_rv32elf_prep_device): everything is checked before the first launch
template <int MEM>
static int prep_device(rk_ctx* ctx, const Image& img, const uint32_t* words, size_t n_words, uint32_t* d_program, size_t program_rows,
                       uint32_t* d_byte, uint32_t* d_range, uint32_t* d_shift) {
    if (!ctx || !d_program || !d_byte || !d_range || !d_shift || (n_words && !words)) return RK_ERR_INVALID;
    if (n_words > (1u << 22) || image_rows_for(n_words) != program_rows) return RK_ERR_CAPACITY;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    void* d_words = nullptr;
    RK_TRY(rk::dev_alloc(ctx, std::max<size_t>(n_words, 1) * 4, &d_words));
    auto enqueue = [&]() -> int {
        if (n_words) RK_HIP_TRY(ctx, hipMemcpyAsync(d_words, words, n_words * 4, hipMemcpyHostToDevice, ctx->stream));
        const unsigned pb = (unsigned)std::min<size_t>(program_rows, TB);
        hipLaunchKernelGGL(program_prep_kernel<MEM>, dim3((unsigned)(program_rows / pb)), dim3(pb), pb * (IM_PROG_W | 1) * 4, ctx->stream,
                           (const uint32_t*)d_words, (uint32_t)n_words, img, program_rows, d_program);
        RK_TRY(rk::post_launch(ctx, "rv32 program_prep_kernel"));
        hipLaunchKernelGGL(byte_prep_kernel, dim3((1u << RK_RV32_BYTE_LOG_ROWS) / TB), dim3(TB), TB * (BYTE_W | 1) * 4, ctx->stream, d_byte);
        RK_TRY(rk::post_launch(ctx, "rv32 byte_prep_kernel"));
        hipLaunchKernelGGL(range_prep_kernel, dim3((1u << 16) / 256), dim3(256), 0, ctx->stream, d_range);
        RK_TRY(rk::post_launch(ctx, "rv32 range_prep_kernel"));
        hipLaunchKernelGGL(shift_prep_kernel, dim3((1u << RK_RV32CF_SHIFT_LOG_ROWS) / TB), dim3(TB), TB * (SHIFT_W | 1) * 4, ctx->stream,
                           d_shift);
        return rk::post_launch(ctx, "rv32 shift_prep_kernel");
    };
    int st = enqueue();
    const hipError_t e = hipStreamSynchronize(ctx->stream);   // the caller's `words` and the scratch are free to go
    if (e != hipSuccess && st == RK_OK) {
        ctx->last_error = std::string("rk_rv32elf_prep_device sync: ") + hipGetErrorString(e);
        st = RK_ERR_HIP;
    }
    rk::dev_free(ctx, d_words);
    return st;
}

// rk_rv32mem_journal_device: the kernel, then the library's own commitment of the link matrix.  The two scratch words
// (count, error) are read back after the tree is built; the stream is drained before they go
static int journal_device(rk_ctx* ctx, const uint32_t* d_memory, size_t memory_rows, uint32_t* d_journal, uint32_t* d_link,
                          uint32_t* d_nodes, size_t* n_real, uint32_t h_root[8]) {
    if (!ctx || !d_memory || !d_journal || !d_link || !d_nodes || !n_real || !h_root) return RK_ERR_INVALID;
    if (memory_rows < 2 || (memory_rows & (memory_rows - 1)) || memory_rows > ((size_t)1 << ntt::LAMBDA)) return RK_ERR_INVALID;
    *n_real = 0;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    void* d_flags = nullptr;
    RK_TRY(rk::dev_alloc(ctx, 8, &d_flags));
    uint32_t flags[2] = {0, 0};
    auto enqueue = [&]() -> int {
        RK_HIP_TRY(ctx, hipMemsetAsync(d_flags, 0, 8, ctx->stream));
        const unsigned b = (unsigned)std::min<size_t>(memory_rows, TB);
        hipLaunchKernelGGL(mem_journal_kernel, dim3((unsigned)(memory_rows / b)), dim3(b), 0, ctx->stream, d_memory, d_journal, d_link,
                           (uint32_t*)d_flags, (uint32_t*)d_flags + 1);
        RK_TRY(rk::post_launch(ctx, "rv32 mem_journal_kernel"));
        const rk_matrix m{d_link, (uint32_t)memory_rows, RK_RV32LINK_TUPLE, 1};
        RK_TRY(rk_mmcs_commit(ctx, &m, 1, d_nodes, h_root));
        return rk::d2h_sync(ctx, flags, d_flags, 8);
    };
    int st = enqueue();
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess && st == RK_OK) {
        ctx->last_error = std::string("rk_rv32mem_journal_device sync: ") + hipGetErrorString(e);
        st = RK_ERR_HIP;
    }
    rk::dev_free(ctx, d_flags);
    if (st != RK_OK) return st;
    if (flags[1]) {
        ctx->last_error = "rk_rv32mem_journal_device: the memory table's real rows are not a prefix or a limb is out of range";
        return RK_ERR_INVALID;
    }
    *n_real = flags[0];
    return RK_OK;
}

// the digest of a journal on the host: the leaves of the real rows, then level by level the nodes above a real row; a
// subtree of zero rows has one digest per level.  Linear in the journal's rows (n log_rows compressions at most)
static int journal_root(const rk_params* params, const uint32_t* journal, size_t n, uint32_t log_rows, uint32_t root[8]) {
    if (!root || (n && !journal) || log_rows < 1 || log_rows > ntt::LAMBDA || n > ((size_t)1 << log_rows)) return RK_ERR_INVALID;
    for (size_t i = 0; i < n; i++)
        if (journal[3 * i] >= (1u << 30) || (i && journal[3 * i] <= journal[3 * (i - 1)])) return RK_ERR_INVALID;
    rk_params def;
    rk::params_preset(&def, RK_PRESET_SP1);
    rk::Sys sys;
    auto k = std::make_unique<p2::Any>();
    RK_TRY(rk::resolve_params(params ? params : &def, &sys, k.get()));
    uint32_t zero[8], row[RK_RV32LINK_TUPLE] = {0};
    k->hash_elems(row, RK_RV32LINK_TUPLE, zero);
    std::vector<uint32_t> cur(8 * std::max<size_t>(n, 1));
    for (size_t i = 0; i < n; i++) {
        const uint32_t a = journal[3 * i], init = journal[3 * i + 1], fin = journal[3 * i + 2];
        const uint32_t limbs[RK_RV32LINK_TUPLE] = {a & 0x3fffu, a >> 14, init & 0xffffu, init >> 16, fin & 0xffffu, fin >> 16};
        for (unsigned j = 0; j < RK_RV32LINK_TUPLE; j++) row[j] = enc(limbs[j]);
        k->hash_elems(row, RK_RV32LINK_TUPLE, &cur[8 * i]);
    }
    size_t cnt = n;
    for (uint32_t lvl = 0; lvl < log_rows; lvl++) {
        const size_t up = (cnt + 1) / 2;
        for (size_t i = 0; i < up; i++) {
            uint32_t out[8];
            k->hash_pair(&cur[16 * i], 2 * i + 1 < cnt ? &cur[16 * i + 8] : zero, out);
            std::memcpy(&cur[8 * i], out, 32);
        }
        uint32_t z2[8];
        k->hash_pair(zero, zero, z2);
        std::memcpy(zero, z2, 32);
        cnt = up;
    }
    std::memcpy(root, cnt ? cur.data() : zero, 32);
    return RK_OK;
}

}  // namespace rv32

extern "C" {

int rk_rv32mem_journal_device(rk_ctx* ctx, const uint32_t* d_memory, size_t memory_rows, uint32_t* d_journal, uint32_t* d_link,
                              uint32_t* d_nodes, size_t* n_real, uint32_t h_root[8]) {
    RK_GUARD_BEGIN
    return rv32::journal_device(ctx, d_memory, memory_rows, d_journal, d_link, d_nodes, n_real, h_root);
    RK_GUARD_END
}
int rk_rv32mem_journal_root(const rk_params* params, const uint32_t* journal, size_t n, uint32_t log_rows, uint32_t root[8]) {
    RK_GUARD_BEGIN
    return rv32::journal_root(params, journal, n, log_rows, root);
    RK_GUARD_END
}

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
int rk_exec_rv32_sizes(const rk_exec* ex, uint32_t index, size_t* program_rows) {
    RK_GUARD_BEGIN
    if (!program_rows) return RK_ERR_INVALID;
    ExecSegmentView v;
    RK_TRY(exec_segment_view(ex, index, &v));
    *program_rows = rv32::program_rows_of(v, nullptr);
    return RK_OK;
    RK_GUARD_END
}
int rk_exec_rv32_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_cpu, uint32_t* d_program,
                              size_t program_rows, uint32_t* d_register, uint32_t* d_byte, uint32_t* d_range) {
    RK_GUARD_BEGIN
    return rv32::shard_device<rv32::CS_I>(ctx, ex, index, {d_cpu, d_program, program_rows, d_register, d_byte, d_range, nullptr,
                                                           nullptr, 0});
    RK_GUARD_END
}
int rk_exec_rv32cf_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_cpu, uint32_t* d_program,
                                size_t program_rows, uint32_t* d_register, uint32_t* d_byte, uint32_t* d_range,
                                uint32_t* d_shift) {
    RK_GUARD_BEGIN
    return rv32::shard_device<rv32::CS_CF>(ctx, ex, index, {d_cpu, d_program, program_rows, d_register, d_byte, d_range, d_shift,
                                                            nullptr, 0});
    RK_GUARD_END
}
int rk_exec_rv32im_sizes(const rk_exec* ex, uint32_t index, size_t* muldiv_rows) {
    RK_GUARD_BEGIN
    if (!muldiv_rows) return RK_ERR_INVALID;
    ExecSegmentView v;
    RK_TRY(exec_segment_view(ex, index, &v));
    *muldiv_rows = rv32::muldiv_rows_for(rv32::m_count_of(v));
    return RK_OK;
    RK_GUARD_END
}
int rk_exec_rv32im_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_cpu, uint32_t* d_program,
                                size_t program_rows, uint32_t* d_register, uint32_t* d_byte, uint32_t* d_range,
                                uint32_t* d_shift, uint32_t* d_muldiv, size_t muldiv_rows) {
    RK_GUARD_BEGIN
    return rv32::shard_device<rv32::CS_IM>(ctx, ex, index, {d_cpu, d_program, program_rows, d_register, d_byte, d_range, d_shift,
                                                            d_muldiv, muldiv_rows});
    RK_GUARD_END
}
int rk_rv32elf_prep_device(rk_ctx* ctx, const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs,
                           const uint32_t* words, size_t n_words, uint32_t* d_program, size_t program_rows, uint32_t* d_byte,
                           uint32_t* d_range, uint32_t* d_shift) {
    RK_GUARD_BEGIN
    rv32::Image img;
    size_t total = 0;
    RK_TRY(rv32::image_of(seg_vaddr, seg_words, n_segs, &img, &total));
    if (total != n_words) return RK_ERR_INVALID;
    return rv32::prep_device<0>(ctx, img, words, n_words, d_program, program_rows, d_byte, d_range, d_shift);
    RK_GUARD_END
}
int rk_rv32mem_prep_device(rk_ctx* ctx, const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs,
                           const uint32_t* words, size_t n_words, uint32_t* d_program, size_t program_rows, uint32_t* d_byte,
                           uint32_t* d_range, uint32_t* d_shift) {
    RK_GUARD_BEGIN
    rv32::Image img;
    size_t total = 0;
    RK_TRY(rv32::image_of(seg_vaddr, seg_words, n_segs, &img, &total));
    if (total != n_words) return RK_ERR_INVALID;
    return rv32::prep_device<1>(ctx, img, words, n_words, d_program, program_rows, d_byte, d_range, d_shift);
    RK_GUARD_END
}
int rk_exec_rv32mem_sizes(const rk_exec* ex, uint32_t index, size_t* memop_rows, size_t* memory_rows) {
    RK_GUARD_BEGIN
    if (!memop_rows || !memory_rows) return RK_ERR_INVALID;
    ExecSegmentView v;
    RK_TRY(exec_segment_view(ex, index, &v));
    if (v.mem->size() > ((size_t)2 << v.seg->po2)) return RK_ERR_CAPACITY;
    *memop_rows = rv32::mem_rows_for(v.mem->size());
    *memory_rows = rv32::mem_rows_for(exec_mem_words(ex, index));
    return RK_OK;
    RK_GUARD_END
}
int rk_rv32io_prep_device(rk_ctx* ctx, const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs,
                          const uint32_t* words, size_t n_words, uint32_t* d_program, size_t program_rows, uint32_t* d_byte,
                          uint32_t* d_range, uint32_t* d_shift) {
    RK_GUARD_BEGIN
    rv32::Image img;
    size_t total = 0;
    RK_TRY(rv32::image_of(seg_vaddr, seg_words, n_segs, &img, &total));
    if (total != n_words) return RK_ERR_INVALID;
    return rv32::prep_device<2>(ctx, img, words, n_words, d_program, program_rows, d_byte, d_range, d_shift);
    RK_GUARD_END
}
int rk_exec_rv32io_sizes(const rk_exec* ex, uint32_t index, size_t* memop_rows, size_t* memory_rows, size_t* io_rows) {
    RK_GUARD_BEGIN
    if (!io_rows) return RK_ERR_INVALID;
    RK_TRY(rk_exec_rv32mem_sizes(ex, index, memop_rows, memory_rows));
    ExecSegmentView v;
    RK_TRY(exec_segment_view(ex, index, &v));
    *io_rows = rv32::io_rows_for(v.ecall_args->size() + rv32::io_words_of(v));
    if (*io_rows > ((size_t)2 << v.seg->po2)) return RK_ERR_CAPACITY;
    return RK_OK;
    RK_GUARD_END
}
int rk_exec_rv32io_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, const uint32_t* seg_vaddr,
                                const uint32_t* seg_words, uint32_t n_segs, const uint32_t* d_image_words, uint32_t* d_cpu,
                                uint32_t* d_program_mult, size_t program_rows, uint32_t* d_register, uint32_t* d_byte_mult,
                                uint32_t* d_range_mult, uint32_t* d_shift_mult, uint32_t* d_muldiv, size_t muldiv_rows,
                                uint32_t* d_memop, size_t memop_rows, uint32_t* d_memory, size_t memory_rows, uint32_t* d_io,
                                size_t io_rows, uint32_t h_publics[RK_RV32IO_PUBLICS]) {
    RK_GUARD_BEGIN
    rv32::ShardOut o{d_cpu, d_program_mult, program_rows, d_register, d_byte_mult, d_range_mult, d_shift_mult, d_muldiv, muldiv_rows,
                     {}, d_image_words, 0, d_memop, memop_rows, d_memory, memory_rows, d_io, io_rows, h_publics};
    RK_TRY(rv32::image_of(seg_vaddr, seg_words, n_segs, &o.img, &o.n_words));
    return rv32::shard_device<rv32::CS_IO>(ctx, ex, index, o);
    RK_GUARD_END
}
int rk_exec_rv32commit_sizes(const rk_exec* ex, uint32_t index, size_t* memop_rows, size_t* memory_rows, size_t* io_rows) {
    RK_GUARD_BEGIN
    if (!memop_rows || !memory_rows || !io_rows) return RK_ERR_INVALID;
    ExecSegmentView v;
    RK_TRY(exec_segment_view(ex, index, &v));
    const auto merged = rv32::merged_list(v);
    if (merged.size() > ((size_t)2 << v.seg->po2)) return RK_ERR_CAPACITY;
    *memop_rows = rv32::mem_rows_for(merged.size());
    *memory_rows = rv32::mem_rows_for(rv32::distinct_words(merged));
    *io_rows = rv32::io_rows_for(v.ecall_args->size() + rv32::io_words_of(v) + v.commit_reads->size());
    if (*io_rows > ((size_t)2 << v.seg->po2)) return RK_ERR_CAPACITY;
    return RK_OK;
    RK_GUARD_END
}
int rk_exec_rv32commit_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, const uint32_t* seg_vaddr,
                                    const uint32_t* seg_words, uint32_t n_segs, const uint32_t* d_image_words, uint32_t* d_cpu,
                                    uint32_t* d_program_mult, size_t program_rows, uint32_t* d_register, uint32_t* d_byte_mult,
                                    uint32_t* d_range_mult, uint32_t* d_shift_mult, uint32_t* d_muldiv, size_t muldiv_rows,
                                    uint32_t* d_memop, size_t memop_rows, uint32_t* d_memory, size_t memory_rows, uint32_t* d_io,
                                    size_t io_rows, uint32_t h_publics[RK_RV32COMMIT_PUBLICS], uint32_t* d_log, size_t* n_log) {
    RK_GUARD_BEGIN
    rv32::ShardOut o{d_cpu, d_program_mult, program_rows, d_register, d_byte_mult, d_range_mult, d_shift_mult, d_muldiv, muldiv_rows,
                     {}, d_image_words, 0, d_memop, memop_rows, d_memory, memory_rows, d_io, io_rows, h_publics, d_log, n_log};
    RK_TRY(rv32::image_of(seg_vaddr, seg_words, n_segs, &o.img, &o.n_words));
    return rv32::shard_device<rv32::CS_COMMIT>(ctx, ex, index, o);
    RK_GUARD_END
}
int rk_exec_rv32elf_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, const uint32_t* seg_vaddr,
                                 const uint32_t* seg_words, uint32_t n_segs, const uint32_t* d_image_words, uint32_t* d_cpu,
                                 uint32_t* d_program_mult, size_t program_rows, uint32_t* d_register, uint32_t* d_byte_mult,
                                 uint32_t* d_range_mult, uint32_t* d_shift_mult, uint32_t* d_muldiv, size_t muldiv_rows) {
    RK_GUARD_BEGIN
    rv32::ShardOut o{d_cpu, d_program_mult, program_rows, d_register, d_byte_mult, d_range_mult, d_shift_mult, d_muldiv, muldiv_rows,
                     {}, d_image_words, 0};
    RK_TRY(rv32::image_of(seg_vaddr, seg_words, n_segs, &o.img, &o.n_words));
    return rv32::shard_device<rv32::CS_ELF>(ctx, ex, index, o);
    RK_GUARD_END
}
int rk_exec_rv32mem_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, const uint32_t* seg_vaddr,
                                 const uint32_t* seg_words, uint32_t n_segs, const uint32_t* d_image_words, uint32_t* d_cpu,
                                 uint32_t* d_program_mult, size_t program_rows, uint32_t* d_register, uint32_t* d_byte_mult,
                                 uint32_t* d_range_mult, uint32_t* d_shift_mult, uint32_t* d_muldiv, size_t muldiv_rows,
                                 uint32_t* d_memop, size_t memop_rows, uint32_t* d_memory, size_t memory_rows) {
    RK_GUARD_BEGIN
    rv32::ShardOut o{d_cpu, d_program_mult, program_rows, d_register, d_byte_mult, d_range_mult, d_shift_mult, d_muldiv, muldiv_rows,
                     {}, d_image_words, 0, d_memop, memop_rows, d_memory, memory_rows};
    RK_TRY(rv32::image_of(seg_vaddr, seg_words, n_segs, &o.img, &o.n_words));
    return rv32::shard_device<rv32::CS_MEM>(ctx, ex, index, o);
    RK_GUARD_END
}

}  // extern "C"
