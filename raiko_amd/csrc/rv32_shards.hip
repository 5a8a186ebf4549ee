// The witness of an executed segment written on the GPU (include/raiko_hip.h): the stand-in trace circuit's columns
// (rk_exec_witness_device*) and the tables of the rv32 chip sets (rk_exec_rv32_shard_device, rk_exec_rv32cf_shard_device,
// rk_exec_rv32im_shard_device, rk_exec_rv32elf_shard_device, rk_exec_rv32mem_shard_device, rk_exec_rv32io_shard_device,
// rk_exec_rv32commit_shard_device) with their *_sizes.  The segment is read through executor.hpp's view; what a row holds
// is rv32_rows.hpp's lane bodies (raiko_amd/rv32.py, rv32cf.py, rv32im.py, rv32elf.py are the same in numpy and name every
// column); the kernels around those bodies are rv32_kernels.hpp and rv32_kernels_mem.hpp, included here: one translation
// unit.  What is here: the host driver -- check, allocate, enqueue stage by stage, read back, verdict.  The preprocessed
// matrices of the keyed chip sets are rv32_prep.hip, the link between shard memories rv32_link.hip.
#include "internal.hpp"

#include <algorithm>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "rv32_kernels.hpp"
#include "rv32_kernels_mem.hpp"

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
    if (st == RK_OK)
        st = rk::launch(ctx, "exec_witness_kernel", exec_witness_kernel, (unsigned)((n + 255) / 256), 256, 0, d_code, d_data,
                        (const TraceRow*)d_tr, tr.size(), n, v.seg->end_pc, rows_only ? 1u : 0u);
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

static size_t program_rows_of(const ExecSegmentView& v, uint32_t* n_slots) {
    const uint32_t slots = v.trace->empty() ? 0 : (v.pc_hi - v.pc_lo) / 4 + 1;
    if (n_slots) *n_slots = slots;
    return rows_for(slots, 1);
}

// the rows of a segment's trace with M_W = 1 (an M word writing a register other than x0): its muldiv rows
static size_t m_count_of(const ExecSegmentView& v) {
    size_t c = 0;   // decode(ins).is_m && decode(ins).wr: opcode OP, funct7 = 1, rd != 0
    for (const TraceRow& r : *v.trace) c += (r.ins & 0xfe00007fu) == 0x02000033u && (r.ins & 0xf80u);
    return c;
}

// the io form: the words the segment's READ ecalls stored (the access list's entries at ecall rows), the io table's rows
static size_t io_words_of(const ExecSegmentView& v) {
    size_t c = 0;
    for (const auto& m : *v.mem) c += m[0] < v.trace->size() && (*v.trace)[m[0]].ins == ECALL_WORD;
    return c;
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

namespace {

// the tables a shard's driver writes: rv32i's five, d_shift the sixth of rv32i-cf, d_muldiv (muldiv_rows rows) the
// seventh of rv32im.  rv32im-elf: program / byte / range / shift are the count columns, img / image_words (device, n_words
// of them) the program image the cycles are counted against
struct ShardOut {
    uint32_t *cpu = nullptr, *program = nullptr;
    size_t program_rows = 0;
    uint32_t *reg = nullptr, *byte = nullptr, *range = nullptr, *shift = nullptr, *muldiv = nullptr;
    size_t muldiv_rows = 0;
    Image img{};
    const uint32_t* image_words = nullptr;
    size_t n_words = 0;
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

// the tables every chip set has (a chip set without shift or muldiv passes nullptr, 0)
ShardOut tables_out(uint32_t* d_cpu, uint32_t* d_program, size_t program_rows, uint32_t* d_register, uint32_t* d_byte, uint32_t* d_range,
                    uint32_t* d_shift, uint32_t* d_muldiv, size_t muldiv_rows) {
    ShardOut o;
    o.cpu = d_cpu, o.program = d_program, o.program_rows = program_rows, o.reg = d_register, o.byte = d_byte, o.range = d_range;
    o.shift = d_shift, o.muldiv = d_muldiv, o.muldiv_rows = muldiv_rows;
    return o;
}

// the keyed chip sets: those tables and the program image; each entry point names what it has beyond them
int elf_out(const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs, const uint32_t* d_image_words, uint32_t* d_cpu,
            uint32_t* d_program_mult, size_t program_rows, uint32_t* d_register, uint32_t* d_byte_mult, uint32_t* d_range_mult,
            uint32_t* d_shift_mult, uint32_t* d_muldiv, size_t muldiv_rows, ShardOut* o) {
    *o = tables_out(d_cpu, d_program_mult, program_rows, d_register, d_byte_mult, d_range_mult, d_shift_mult, d_muldiv, muldiv_rows);
    o->image_words = d_image_words;
    return image_of(seg_vaddr, seg_words, n_segs, &o->img, &o->n_words);
}

// What a shard's run needs of its segment, worked out once by shard_check.  v is the segment as the kernels read it: in
// the commit form its access list is `merged`, which the plan owns (so a plan stays where it is)
struct ShardPlan {
    ExecSegmentView v;
    std::vector<std::array<uint32_t, 4>> merged;
    size_t n = 0, cycles = 0;            // the cpu table's rows, the trace's
    uint32_t n_slots = 0;                // the program's slots: the executed pc range's words, rv32im-elf: the image's
    size_t m_count = 0;                  // rv32im: the rows with M_W = 1
    size_t mem_count = 0, mem_words = 0;   // rv32im-mem: the accesses and their distinct words
    size_t n_ec = 0, io_words = 0;       // the io form: the ecalls, and the accesses at ecall rows (the commit reads among them)
    size_t n_reads = 0;                  // the commit form: the commit reads, and the bytes its COMMITs append to the journal
    uint32_t commit_bytes = 0;
    ShardPlan() = default;
    ShardPlan(const ShardPlan&) = delete;
    ShardPlan& operator=(const ShardPlan&) = delete;
};

// the side lists against the trace and the tables' rows against what they need (shard_check's second half)
template <int CS>
int lists_check(rk_ctx* ctx, const ExecSegmentView& vu, const ShardOut& o, const ShardPlan& p) {
    using CH = Chips<CS>;
    const ExecSegmentView& v = p.v;
    if constexpr (CH::mem) {   // powers of two that hold every row, at most twice the cpu table; nothing is written otherwise
        const struct { size_t rows, need; const char* what; } t[2] = {
            {o.memop_rows, rows_for(p.mem_count, RK_RV32MEM_MIN_LOG_ROWS), "memop"},
            {o.memory_rows, rows_for(p.mem_words, RK_RV32MEM_MIN_LOG_ROWS), "memory"}};
        for (const auto& c : t)
            if (c.rows < c.need || c.rows & (c.rows - 1) || c.rows > 2 * p.n) {
                ctx->last_error = std::string("rk_exec_rv32mem_shard_device: the ") + c.what + " table's rows are not a power of two from what the segment needs up to twice the cpu table's";
                return RK_ERR_INVALID;
            }
        static_assert(sizeof(MemAccess) == sizeof((*v.mem)[0]), "an access is four words, as the executor records it");
        if (!mem_list_ok(v.trace->data(), p.cycles, (const MemAccess*)v.mem->data(), p.mem_count)) {
            ctx->last_error = "rk_exec_rv32mem_shard_device: the access list is not in cycle order or is not the trace's loads, stores and ecalls";
            return RK_ERR_INVALID;
        }
    }
    if constexpr (CH::io) {   // a power of two >= 2 that holds every row, at most twice the cpu table; the side list the trace's ecalls
        if (o.io_rows < 2 || o.io_rows & (o.io_rows - 1) || o.io_rows > 2 * p.n) {
            ctx->last_error = "rk_exec_rv32io_shard_device: the io table's rows are not a power of two from 2 up to twice the cpu table's";
            return RK_ERR_INVALID;
        }
        if (o.io_rows < rows_for(p.n_ec + p.io_words, 1)) {
            ctx->last_error = "rk_exec_rv32io_shard_device: the io table has fewer rows than the segment needs";
            return RK_ERR_CAPACITY;
        }
        if (v.n_input >= ((size_t)1 << 30)) {
            ctx->last_error = "rk_exec_rv32io_shard_device: an input of 2^30 words or more";
            return RK_ERR_CAPACITY;
        }
        static_assert(sizeof(EcallArg) == sizeof((*v.ecall_args)[0]), "an entry is five words, as the executor records it");
        if (p.n_ec != v.ecalls->size() || !io_list_ok(v.trace->data(), p.cycles, (const EcallArg*)v.ecall_args->data(), p.n_ec)) {
            ctx->last_error = "rk_exec_rv32io_shard_device: the ecall side list is not the trace's ecall rows in cycle order";
            return RK_ERR_INVALID;
        }
    }
    if constexpr (CH::commit) {   // the commit reads are the words of the trace's COMMITs; the journal stays below 2^30 bytes
        static_assert(sizeof(MemAccess) == sizeof((*v.commit_reads)[0]), "a commit read is four words, as the executor records it");
        uint64_t bytes = vu.jpos_start;
        for (const auto& e : *vu.ecall_args) bytes += e[1] == 2 ? e[3] : 0u;
        if (bytes >= ((uint64_t)1 << 30) ||
            !commit_list_ok((const EcallArg*)vu.ecall_args->data(), vu.ecall_args->size(), (const MemAccess*)vu.commit_reads->data(),
                            vu.commit_reads->size(), (const MemAccess*)vu.mem->data(), vu.mem->size())) {
            ctx->last_error = "rk_exec_rv32commit_shard_device: the commit reads are not the words of the trace's COMMITs in cycle order";
            return RK_ERR_INVALID;
        }
    }
    return RK_OK;
}

// Everything that can refuse a shard, on the host: the arguments, the segment, every table's rows and the side lists.
// Fills the plan; nothing touches the GPU before this has returned RK_OK
template <int CS>
int shard_check(rk_ctx* ctx, const rk_exec* ex, uint32_t index, const ShardOut& o, ShardPlan* p) {
    using CH = Chips<CS>;
    if (!ctx || !o.cpu || !o.program || !o.reg || !o.byte || !o.range || (CH::cf && !o.shift) || (CH::im && !o.muldiv) ||
        (CH::mem && (!o.memop || !o.memory)) || (CH::io && (!o.io || !o.h_publics)) || (CH::commit && (!o.log || !o.n_log)))
        return RK_ERR_INVALID;
    ExecSegmentView& v = p->v;
    RK_TRY(exec_segment_view(ex, index, &v));
    const ExecSegmentView vu = v;   // as the executor recorded it; the commit form's v.mem is the merged list
    if constexpr (CH::commit) {
        p->merged = merged_list(v);
        v.mem = &p->merged;
    }
    p->cycles = v.trace->size(), p->n = (size_t)1 << v.seg->po2;
    if (p->cycles > p->n || p->n % TB) return RK_ERR_INTERNAL;
    if constexpr (CH::elf) {   // one slot per word of the image
        if (!o.image_words && o.n_words) return RK_ERR_INVALID;
        if (o.n_words > (1u << 22) || rows_for(o.n_words, 1) != o.program_rows) return RK_ERR_CAPACITY;
        p->n_slots = (uint32_t)o.n_words;
    } else if (program_rows_of(v, &p->n_slots) != o.program_rows) {
        return RK_ERR_CAPACITY;
    }
    if (p->n_slots > (1u << 22)) {
        ctx->last_error = "rk_exec_rv32_shard_device: executed pc range wider than 2^22 words";
        return RK_ERR_CAPACITY;
    }
    if constexpr (CH::im) {   // a power of two that holds every muldiv row, no taller than the cpu table; nothing is written otherwise
        p->m_count = m_count_of(v);
        if (o.muldiv_rows < rows_for(p->m_count, RK_RV32IM_MULDIV_MIN_LOG_ROWS)) {
            ctx->last_error = "rk_exec_rv32im_shard_device: the muldiv table has fewer rows than the segment needs";
            return RK_ERR_CAPACITY;
        }
        if (o.muldiv_rows & (o.muldiv_rows - 1) || o.muldiv_rows > std::max<size_t>(p->n, rows_for(0, RK_RV32IM_MULDIV_MIN_LOG_ROWS)))
            return RK_ERR_INVALID;
    }
    if constexpr (CH::mem) {
        p->mem_count = v.mem->size();
        p->mem_words = CH::commit ? distinct_words(p->merged) : exec_mem_words(ex, index);
    }
    if constexpr (CH::io) p->n_ec = v.ecall_args->size(), p->io_words = io_words_of(v);
    if constexpr (CH::commit) {
        p->n_reads = v.commit_reads->size();
        for (const auto& e : *v.ecall_args) p->commit_bytes += e[1] == 2 ? e[3] : 0u;
    }
    return lists_check<CS>(ctx, vu, o, *p);
}

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
    size_t macc = 0, mkeys = 0, mvals = 0, mkeys2 = 0, mvals2 = 0, mpts = 0, necw = 0, hblk = 0, htotal = 0;   // rv32im-mem
    size_t eargs = 0, eoff = 0, eblk = 0, etotal = 0, stream = 0, nodes = 0;                                   // the io form
    size_t creads = 0, coff = 0, cblk = 0, ctotal = 0, joff = 0, jblk = 0, jtotal = 0, clog = 0, cnodes = 0;   // the commit form
    template <int CS>
    static Scratch of(const ShardPlan& p, const ShardOut& o) {
        using CH = Chips<CS>;
        Scratch L;
        const size_t n = p.n, nb = n / TB, slots = std::max<uint32_t>(p.n_slots, 1), sw = CH::cf ? SHIFT_USED : 1u;
        const size_t ne = std::max<size_t>(p.v.ecalls->size(), 1), eb = (ne + TB - 1) / TB;
        L.tr = L.take((std::max<size_t>(p.cycles, 1) * sizeof(TraceRow) + 3) / 4);
        L.ec = L.take(2 * ne);
        L.wval = L.take(n);
        L.acc = L.take(n);
        L.blk = L.take(nb * 32);
        L.final_ts = L.take(32);
        L.fin = L.take(32);
        L.init = L.take(32);
        L.err = L.take(1);
        L.hist = L.take((size_t)1 << 16);
        L.bmult = L.take((size_t)3 << 16);
        L.pmult = L.take(slots);
        L.pins = L.take(CH::elf ? 1 : slots);   // rv32im-elf compares with the image: no word is recorded
        L.smult = L.take(sw);
        L.clear_end = L.smult + sw;
        L.mflag = L.take(CH::im ? n : 1);
        L.mblk = L.take(CH::im ? nb : 1);
        L.mtotal = L.take(1);
        L.midx = L.take(std::max<size_t>(p.m_count, 1));
        if constexpr (CH::mem) {
            const size_t mc = std::max<size_t>(p.mem_count, 1);
            L.macc = L.take(4 * mc);
            L.mkeys = L.take(mc);
            L.mvals = L.take(mc);
            L.mkeys2 = L.take(mc);
            L.mvals2 = L.take(mc);
            L.mpts = L.take(mc);
            L.necw = L.take(n);
            L.hblk = L.take((mc + TB - 1) / TB);
            L.htotal = L.take(1);
        }
        if constexpr (CH::io) {
            L.eargs = L.take(5 * ne);
            L.eoff = L.take(ne);
            L.eblk = L.take(eb);
            L.etotal = L.take(1);
            L.stream = L.take(o.io_rows * RK_RV32LINK_TUPLE);
            L.nodes = L.take(2 * o.io_rows * 8);
        }
        if constexpr (CH::commit) {
            L.creads = L.take(4 * std::max<size_t>(p.n_reads, 1));
            L.coff = L.take(ne);
            L.cblk = L.take(eb);
            L.ctotal = L.take(1);
            L.joff = L.take(ne);
            L.jblk = L.take(eb);
            L.jtotal = L.take(1);
            L.clog = L.take(o.io_rows * RK_RV32LINK_TUPLE);
            L.cnodes = L.take(2 * o.io_rows * 8);
        }
        return L;
    }
};

// One shard's run: the plan, the tables, the scratch block `w` with its layout and rocPRIM's temporary, and the stages of
// the pipeline over them.  A stage is the copies and launches of one part, in stream order, and returns at the first error
template <int CS>
struct ShardRun {
    using CH = Chips<CS>;
    rk_ctx* ctx;
    const ShardPlan& p;
    const ShardOut& o;
    const Scratch& L;
    uint32_t* w;
    void* sort_tmp;
    size_t sort_bytes;
    const TraceRow* tr() const { return (const TraceRow*)(w + L.tr); }
    const MemAccess* macc() const { return (const MemAccess*)(w + L.macc); }
    const EcallArg* eargs() const { return (const EcallArg*)(w + L.eargs); }
    unsigned nb() const { return (unsigned)(p.n / TB); }

    int upload(const std::vector<uint32_t>& ec_flat) const {
        const std::vector<TraceRow>& t = *p.v.trace;
        if (!t.empty()) RK_HIP_TRY(ctx, hipMemcpyAsync(w + L.tr, t.data(), t.size() * sizeof(TraceRow), hipMemcpyHostToDevice, ctx->stream));
        if (!ec_flat.empty()) RK_HIP_TRY(ctx, hipMemcpyAsync(w + L.ec, ec_flat.data(), ec_flat.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        RK_HIP_TRY(ctx, hipMemcpyAsync(w + L.init, p.v.regs, 32 * 4, hipMemcpyHostToDevice, ctx->stream));
        RK_HIP_TRY(ctx, hipMemsetAsync(w + L.err, 0, (L.clear_end - L.err) * 4, ctx->stream));
        return RK_OK;
    }

    // the io form of the trace: an ecall row's a / b / res are the call's a0 / a1 / t0
    int io_patch() const {
        if (!p.n_ec) return RK_OK;
        RK_HIP_TRY(ctx, hipMemcpyAsync(w + L.eargs, p.v.ecall_args->data(), p.n_ec * sizeof(EcallArg), hipMemcpyHostToDevice, ctx->stream));
        return rk::launch(ctx, "rv32 io_patch_kernel", io_patch_kernel, (unsigned)((p.n_ec + TB - 1) / TB), TB, 0, (TraceRow*)(w + L.tr),
                          p.cycles, eargs(), p.n_ec, w + L.err);
    }

    int prep() const {
        ImageArgs<CH::elf> image;
        if constexpr (CH::elf) image = {o.img, o.image_words};
        return rk::launch(ctx, "rv32 prep_kernel", prep_kernel<CH::elf, CH::io>, nb(), TB, 0, tr(), p.cycles, p.n, w + L.ec,
                          (uint32_t)p.v.ecalls->size(), p.v.pc_lo, p.n_slots, w + L.wval, w + L.acc, w + L.pmult, w + L.pins, w + L.err,
                          CH::im ? w + L.mflag : nullptr, image);
    }

    // rv32im-mem: the sorted access list, each access's predecessor and the boundary rows (before rows_kernel: necw)
    int mem() const {
        static_assert(sizeof(MemAccess) == 16, "an access is four words, as the executor records it");
        const size_t count = p.mem_count;
        RK_HIP_TRY(ctx, hipMemsetAsync(w + L.necw, 0, p.n * 4, ctx->stream));
        RK_HIP_TRY(ctx, hipMemsetAsync(w + L.htotal, 0, 4, ctx->stream));
        RK_HIP_TRY(ctx, hipMemsetAsync(o.memory, 0, o.memory_rows * BD_W * 4, ctx->stream));   // the rows past the touched words
        if (!count) return RK_OK;
        RK_HIP_TRY(ctx, hipMemcpyAsync(w + L.macc, p.v.mem->data(), count * sizeof(MemAccess), hipMemcpyHostToDevice, ctx->stream));
        const unsigned kb = (unsigned)((count + TB - 1) / TB);
        RK_TRY(rk::launch(ctx, "rv32 mem_keys_kernel", mem_keys_kernel, kb, TB, 0, macc(), count, tr(), w + L.mkeys, w + L.mvals, w + L.necw));
        size_t bytes = sort_bytes;
        RK_HIP_TRY(ctx, rocprim::radix_sort_pairs(sort_tmp, bytes, w + L.mkeys, w + L.mkeys2, w + L.mvals, w + L.mvals2, count, 0, 30,
                                                  ctx->stream));
        RK_TRY(rk::launch(ctx, "rv32 mhead_count_kernel", mhead_count_kernel, kb, TB, 0, w + L.mkeys2, count, w + L.hblk));
        RK_TRY(rk::launch(ctx, "rv32 mscan_kernel", mscan_kernel, 1, 1024, 0, w + L.hblk, (size_t)kb, w + L.htotal));
        return rk::launch(ctx, "rv32 mem_link_kernel", mem_link_kernel, kb, TB, 0, w + L.mkeys2, w + L.mvals2, macc(), count, w + L.hblk,
                          w + L.mpts, o.memory, o.memory_rows, w + L.hist, w + L.err);
    }

    // the last access per register per block, then their exclusive max-scan over the blocks
    int scans() const {
        RK_TRY(rk::launch(ctx, "rv32 block_last_kernel", block_last_kernel, nb(), TB, 0, w + L.acc, w + L.blk));
        return rk::launch(ctx, "rv32 scan_kernel", scan_kernel, 1, 1024, 0, w + L.blk, (size_t)nb(), w + L.final_ts);
    }

    int rows() const {
        constexpr int RCS = CH::commit ? (int)CS_IO : CS;   // the commit form's cpu rows are the io form's: one instantiation
        const size_t lds = TB * (CH::cpu_w | 1) * 4;
        if (lds > 64 * 1024)   // rv32im's 133-word rows: past the default dynamic LDS limit (160 KiB per CU)
            RK_HIP_TRY(ctx, hipFuncSetAttribute((const void*)rows_kernel<RCS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        return rk::launch(ctx, "rv32 rows_kernel", rows_kernel<RCS>, nb(), TB, lds, tr(), p.cycles, p.v.seg->end_pc, w + L.acc, w + L.wval,
                          w + L.blk, w + L.init, o.cpu, w + L.hist, w + L.bmult, w + L.smult, w + L.necw, p.n);
    }

    // rv32im: the muldiv rows: count per block, scan, compact, then one lane per row (before the byte / range / shift
    // tables: its counts go into theirs)
    int muldiv() const {
        uint32_t *mflag = w + L.mflag, *mblk = w + L.mblk, *midx = w + L.midx;
        RK_TRY(rk::launch(ctx, "rv32 mcount_kernel", mcount_kernel, nb(), TB, 0, mflag, mblk));
        RK_TRY(rk::launch(ctx, "rv32 mscan_kernel", mscan_kernel, 1, 1024, 0, mblk, (size_t)nb(), w + L.mtotal));
        RK_TRY(rk::launch(ctx, "rv32 mcompact_kernel", mcompact_kernel, nb(), TB, 0, mflag, mblk, p.m_count, midx));
        const unsigned b = (unsigned)std::min<size_t>(o.muldiv_rows, TB);
        return rk::launch(ctx, "rv32 muldiv_kernel", muldiv_kernel, (unsigned)(o.muldiv_rows / b), b, b * (MD_W | 1) * 4, tr(), p.cycles,
                          w + L.wval, midx, p.m_count, o.muldiv_rows, o.muldiv, w + L.hist, w + L.bmult, w + L.smult, w + L.err);
    }

    // rv32im-mem: one lane per memop row (before the count columns: its counts go into theirs)
    int memop() const {
        const unsigned b = (unsigned)std::min<size_t>(o.memop_rows, TB);
        return rk::launch(ctx, "rv32 memop_kernel", memop_kernel<CH::mo_w>, (unsigned)(o.memop_rows / b), b, b * (CH::mo_w | 1) * 4, tr(),
                          w + L.wval, macc(), w + L.mpts, p.mem_count, o.memop_rows, o.memop, w + L.hist, w + L.bmult, w + L.smult,
                          w + L.err, CH::io ? 1u : 0u);
    }

    // the commit form's part of the io stage: the commit log's two matrices cleared, the commit reads uploaded, and what
    // io_offsets_kernel and io_rows_kernel take beyond the io form's arguments
    int commit_part(uint32_t total, CommitScan* scan, CommitRows* cm) const {
        RK_HIP_TRY(ctx, hipMemsetAsync(w + L.clog, 0, o.io_rows * RK_RV32LINK_TUPLE * 4, ctx->stream));
        RK_HIP_TRY(ctx, hipMemsetAsync(o.log, 0, o.io_rows * 3 * 4, ctx->stream));
        if (p.n_reads)
            RK_HIP_TRY(ctx, hipMemcpyAsync(w + L.creads, p.v.commit_reads->data(), p.n_reads * sizeof(MemAccess), hipMemcpyHostToDevice, ctx->stream));
        scan->coff = w + L.coff, scan->cblk = w + L.cblk, scan->joff = w + L.joff, scan->jblk = w + L.jblk;
        cm->reads = (const MemAccess*)(w + L.creads), cm->n_reads = (uint32_t)p.n_reads;
        cm->coff = scan->coff, cm->cblk = scan->cblk, cm->joff = scan->joff, cm->jblk = scan->jblk;
        cm->jpos_start = p.v.jpos_start, cm->jpos_end = p.v.jpos_start + p.commit_bytes;
        cm->pos_end = p.v.in_start + (uint32_t)(total - p.n_ec - p.n_reads);
        cm->clog = w + L.clog, cm->dlog = o.log;
        return RK_OK;
    }

    // the io form: the io rows (before the count columns: its counts go into the range table's), then the digest of the
    // stream matrix and, in the commit form, of the commit log
    int io() const {
        const size_t n_ec = p.n_ec;
        const uint32_t total = (uint32_t)(n_ec + p.io_words);   // the commit form: counted over the merged list
        RK_HIP_TRY(ctx, hipMemsetAsync(w + L.stream, 0, o.io_rows * RK_RV32LINK_TUPLE * 4, ctx->stream));
        CommitScanOf<CH::commit> scan;
        CommitRowsOf<CH::commit> cm;
        if constexpr (CH::commit) RK_TRY(commit_part(total, &scan, &cm));
        if (n_ec) {
            const unsigned eb = (unsigned)((n_ec + TB - 1) / TB);
            RK_TRY(rk::launch(ctx, "rv32 io_offsets_kernel", io_offsets_kernel<CH::commit>, eb, TB, 0, eargs(), n_ec, w + L.necw, w + L.eoff,
                              w + L.eblk, scan));
            RK_TRY(rk::launch(ctx, "rv32 mscan_kernel", mscan_kernel, 1, 1024, 0, w + L.eblk, (size_t)eb, w + L.etotal));
            if constexpr (CH::commit) {
                RK_TRY(rk::launch(ctx, "rv32 mscan_kernel", mscan_kernel, 1, 1024, 0, w + L.cblk, (size_t)eb, w + L.ctotal));
                RK_TRY(rk::launch(ctx, "rv32 mscan_kernel", mscan_kernel, 1, 1024, 0, w + L.jblk, (size_t)eb, w + L.jtotal));
            }
        }
        const unsigned b = (unsigned)std::min<size_t>(o.io_rows, TB);
        RK_TRY(rk::launch(ctx, "rv32 io_rows_kernel", io_rows_kernel<CH::commit>, (unsigned)(o.io_rows / b), b, b * (CH::io_w | 1) * 4, eargs(),
                          n_ec, w + L.ec, w + L.necw, w + L.eoff, w + L.eblk, macc(), p.mem_count, (uint32_t)p.v.n_input, p.v.in_start, total,
                          o.io_rows, o.io, w + L.stream, w + L.hist, w + L.err, cm));
        const rk_matrix m{w + L.stream, (uint32_t)o.io_rows, RK_RV32LINK_TUPLE, 1};
        RK_TRY(rk_mmcs_commit(ctx, &m, 1, w + L.nodes, o.h_publics + 6));
        if constexpr (CH::commit) {
            const rk_matrix cl{w + L.clog, (uint32_t)o.io_rows, RK_RV32LINK_TUPLE, 1};
            RK_TRY(rk_mmcs_commit(ctx, &cl, 1, w + L.cnodes, o.h_publics + RK_RV32IO_PUBLICS + 2));
        }
        return RK_OK;
    }

    // the lookup tables, after every kernel that counts into them: rv32im-elf's count columns (the tuples are in the key:
    // each lookup table's trace is its count column) or the program, byte and range tables; the register and shift tables
    int tables() const {
        uint32_t *hist = w + L.hist, *bmult = w + L.bmult, *pmult = w + L.pmult, *smult = w + L.smult;
        if constexpr (CH::elf) {
            const struct { const uint32_t* counts; size_t n_counts, n_rows; uint32_t* out; } cols[4] = {
                {pmult, p.n_slots, o.program_rows, o.program}, {bmult, (size_t)3 << 16, (size_t)1 << RK_RV32_BYTE_LOG_ROWS, o.byte},
                {hist, (size_t)1 << 16, (size_t)1 << 16, o.range}, {smult, SHIFT_USED, (size_t)1 << RK_RV32CF_SHIFT_LOG_ROWS, o.shift}};
            for (const auto& c : cols)
                RK_TRY(rk::launch(ctx, "rv32 count_kernel", count_kernel, (unsigned)((c.n_rows + 255) / 256), 256, 0, c.counts, c.n_counts,
                                  c.n_rows, c.out));
        } else {
            const unsigned pb = (unsigned)std::min<size_t>(o.program_rows, TB);
            RK_TRY(rk::launch(ctx, "rv32 program_kernel", program_kernel<CS>, (unsigned)((o.program_rows + pb - 1) / pb), pb,
                              pb * (CH::prog_w | 1) * 4, w + L.pins, pmult, p.n_slots, p.v.pc_lo, o.program_rows, o.program));
            RK_TRY(rk::launch(ctx, "rv32 byte_kernel", byte_kernel, (1u << RK_RV32_BYTE_LOG_ROWS) / TB, TB, TB * (BYTE_W | 1) * 4, bmult,
                              o.byte));
            RK_TRY(rk::launch(ctx, "rv32 range_kernel", range_kernel, (1u << 16) / TB, TB, 0, hist, o.range));
        }
        RK_TRY(rk::launch(ctx, "rv32 register_kernel", register_kernel, 1, 32, 32 * (REG_W | 1) * 4, w + L.final_ts, w + L.init, tr(),
                          w + L.wval, w + L.fin, o.reg, CH::io ? 1u : 0u));
        if constexpr (CH::cf && !CH::elf)   // after rows_kernel (and muldiv_kernel) on the stream: the counts are complete
            RK_TRY(rk::launch(ctx, "rv32 shift_kernel", shift_kernel, (1u << RK_RV32CF_SHIFT_LOG_ROWS) / TB, TB, TB * (SHIFT_W | 1) * 4, smult,
                              o.shift));
        return RK_OK;
    }

    // the copies and the launches of one shard, in stream order; returns at the first error
    int enqueue(const std::vector<uint32_t>& ec_flat) const {
        RK_TRY(upload(ec_flat));
        if constexpr (CH::io) RK_TRY(io_patch());
        RK_TRY(prep());
        if constexpr (CH::mem) RK_TRY(mem());
        RK_TRY(scans());
        RK_TRY(rows());
        if constexpr (CH::im) RK_TRY(muldiv());
        if constexpr (CH::mem) RK_TRY(memop());
        if constexpr (CH::io) RK_TRY(io());
        return tables();
    }
};

}  // namespace

// what comes back from the device after a shard: the final registers, the error word (ShardErr) and the two counts
struct ShardBack {
    uint32_t fin[32] = {0};
    uint32_t err = 0, m_total = 0, heads = 0;
};

// queues the read-backs and drains the stream, whatever `st` the enqueue returned; -> st, or the first error here
template <int CS>
static int shard_read_back(const ShardRun<CS>& r, int st, ShardBack* b) {
    using CH = Chips<CS>;
    rk_ctx* ctx = r.ctx;
    auto hip = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && st == RK_OK) {
            ctx->last_error = std::string("rk_exec_rv32_shard_device ") + what + ": " + hipGetErrorString(e);
            st = RK_ERR_HIP;
        }
    };
    hip(hipMemcpyAsync(b->fin, r.w + r.L.fin, 32 * 4, hipMemcpyDeviceToHost, ctx->stream), "d2h");
    hip(hipMemcpyAsync(&b->err, r.w + r.L.err, 4, hipMemcpyDeviceToHost, ctx->stream), "d2h");
    if constexpr (CH::im) hip(hipMemcpyAsync(&b->m_total, r.w + r.L.mtotal, 4, hipMemcpyDeviceToHost, ctx->stream), "d2h");
    if constexpr (CH::mem)
        if (r.p.mem_count) hip(hipMemcpyAsync(&b->heads, r.w + r.L.htotal, 4, hipMemcpyDeviceToHost, ctx->stream), "d2h");
    hip(hipStreamSynchronize(ctx->stream), "sync");
    return st;
}

// the io form's public values, and the commit form's with its log's rows.  They are written between the verdict's first
// checks and its later ones: a shard whose side list or commit reads are refused leaves them alone, one refused for
// anything later has them
template <int CS>
static void write_publics(const ShardPlan& p, const ShardOut& o, uint32_t bits) {
    if (bits & ERR_IO_LIST) return;
    const ExecSegmentView& v = p.v;
    const auto& ea = *v.ecall_args;
    const bool halted = !ea.empty() && ea.back()[1] == 0;
    const uint32_t exit_code = halted ? ea.back()[2] : 0u;
    // the words the READs stored: the accesses at ecall rows that are no commit reads
    const uint32_t pub[6] = {v.in_start, v.in_start + (uint32_t)(p.io_words - p.n_reads), (uint32_t)v.n_input, halted ? 1u : 0u,
                             exit_code & 0xffffu, exit_code >> 16};
    for (unsigned j = 0; j < 6; j++) o.h_publics[j] = enc(pub[j]);
    if constexpr (Chips<CS>::commit) {
        if (bits & ERR_COMMIT_READ) return;
        o.h_publics[RK_RV32IO_PUBLICS] = enc(v.jpos_start);
        o.h_publics[RK_RV32IO_PUBLICS + 1] = enc(v.jpos_start + p.commit_bytes);
        *o.n_log = p.n_reads;
    }
}

// One shard's tables: check, allocate, enqueue, read back and drain, free, verdict.  Owns the scratch block and the host
// staging of the ecall list: whatever the enqueue returns, the read-backs are queued and the stream is drained before
// either goes, so no queued copy outlives its host buffer and the scratch is never returned with work in flight.
template <int CS>
static int shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, const ShardOut& o) {
    using CH = Chips<CS>;
    ShardPlan p;
    RK_TRY(shard_check<CS>(ctx, ex, index, o, &p));
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const Scratch L = Scratch::of<CS>(p, o);
    rk::DevBuf sort_tmp;   // rocPRIM's temporary storage for the sort of mem_count pairs
    size_t sort_bytes = 0;
    if (p.mem_count) {
        RK_HIP_TRY(ctx, rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                                  (uint32_t*)nullptr, p.mem_count, 0, 30, ctx->stream));
        RK_TRY(sort_tmp.alloc(ctx, std::max<size_t>(sort_bytes, 4)));
    }
    void* base = nullptr;
    RK_TRY(rk::dev_alloc(ctx, L.words * 4, &base));
    const auto& ecalls = *p.v.ecalls;
    std::vector<uint32_t> ec_flat(2 * ecalls.size());
    for (size_t k = 0; k < ecalls.size(); k++) ec_flat[2 * k] = ecalls[k][0], ec_flat[2 * k + 1] = ecalls[k][1];
    const ShardRun<CS> r{ctx, p, o, L, (uint32_t*)base, sort_tmp.p, sort_bytes};
    // the tables are complete and the scratch can go: read back the final registers and the error flags
    ShardBack back;
    const int st = shard_read_back(r, r.enqueue(ec_flat), &back);
    rk::dev_free(ctx, base);
    if (st != RK_OK) return st;
    const ShardVerdict vd = shard_verdict<CS>(back.err, back.m_total, p.m_count, back.heads, p.mem_words);
    if constexpr (CH::io) write_publics<CS>(p, o, back.err);
    if (vd.status != RK_OK) {
        ctx->last_error = vd.message;
        return vd.status;
    }
    if (!std::equal(back.fin, back.fin + 32, p.v.regs + 32)) {
        ctx->last_error = "rk_exec_rv32_shard_device: the register accesses do not end in the executor's registers";
        return RK_ERR_INTERNAL;
    }
    return RK_OK;
}

}  // namespace rv32

extern "C" {

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
    return rv32::shard_device<rv32::CS_I>(ctx, ex, index,
                                          rv32::tables_out(d_cpu, d_program, program_rows, d_register, d_byte, d_range, nullptr, nullptr, 0));
    RK_GUARD_END
}
int rk_exec_rv32cf_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_cpu, uint32_t* d_program,
                                size_t program_rows, uint32_t* d_register, uint32_t* d_byte, uint32_t* d_range,
                                uint32_t* d_shift) {
    RK_GUARD_BEGIN
    return rv32::shard_device<rv32::CS_CF>(ctx, ex, index,
                                           rv32::tables_out(d_cpu, d_program, program_rows, d_register, d_byte, d_range, d_shift, nullptr, 0));
    RK_GUARD_END
}
int rk_exec_rv32im_sizes(const rk_exec* ex, uint32_t index, size_t* muldiv_rows) {
    RK_GUARD_BEGIN
    if (!muldiv_rows) return RK_ERR_INVALID;
    ExecSegmentView v;
    RK_TRY(exec_segment_view(ex, index, &v));
    *muldiv_rows = rv32::rows_for(rv32::m_count_of(v), RK_RV32IM_MULDIV_MIN_LOG_ROWS);
    return RK_OK;
    RK_GUARD_END
}
int rk_exec_rv32im_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_cpu, uint32_t* d_program,
                                size_t program_rows, uint32_t* d_register, uint32_t* d_byte, uint32_t* d_range,
                                uint32_t* d_shift, uint32_t* d_muldiv, size_t muldiv_rows) {
    RK_GUARD_BEGIN
    return rv32::shard_device<rv32::CS_IM>(
        ctx, ex, index, rv32::tables_out(d_cpu, d_program, program_rows, d_register, d_byte, d_range, d_shift, d_muldiv, muldiv_rows));
    RK_GUARD_END
}
int rk_exec_rv32mem_sizes(const rk_exec* ex, uint32_t index, size_t* memop_rows, size_t* memory_rows) {
    RK_GUARD_BEGIN
    if (!memop_rows || !memory_rows) return RK_ERR_INVALID;
    ExecSegmentView v;
    RK_TRY(exec_segment_view(ex, index, &v));
    if (v.mem->size() > ((size_t)2 << v.seg->po2)) return RK_ERR_CAPACITY;
    *memop_rows = rv32::rows_for(v.mem->size(), RK_RV32MEM_MIN_LOG_ROWS);
    *memory_rows = rv32::rows_for(exec_mem_words(ex, index), RK_RV32MEM_MIN_LOG_ROWS);
    return RK_OK;
    RK_GUARD_END
}
int rk_exec_rv32io_sizes(const rk_exec* ex, uint32_t index, size_t* memop_rows, size_t* memory_rows, size_t* io_rows) {
    RK_GUARD_BEGIN
    if (!io_rows) return RK_ERR_INVALID;
    RK_TRY(rk_exec_rv32mem_sizes(ex, index, memop_rows, memory_rows));
    ExecSegmentView v;
    RK_TRY(exec_segment_view(ex, index, &v));
    *io_rows = rv32::rows_for(v.ecall_args->size() + rv32::io_words_of(v), 1);
    if (*io_rows > ((size_t)2 << v.seg->po2)) return RK_ERR_CAPACITY;
    return RK_OK;
    RK_GUARD_END
}
int rk_exec_rv32commit_sizes(const rk_exec* ex, uint32_t index, size_t* memop_rows, size_t* memory_rows, size_t* io_rows) {
    RK_GUARD_BEGIN
    if (!memop_rows || !memory_rows || !io_rows) return RK_ERR_INVALID;
    ExecSegmentView v;
    RK_TRY(exec_segment_view(ex, index, &v));
    const auto merged = rv32::merged_list(v);
    if (merged.size() > ((size_t)2 << v.seg->po2)) return RK_ERR_CAPACITY;
    *memop_rows = rv32::rows_for(merged.size(), RK_RV32MEM_MIN_LOG_ROWS);
    *memory_rows = rv32::rows_for(rv32::distinct_words(merged), RK_RV32MEM_MIN_LOG_ROWS);
    *io_rows = rv32::rows_for(v.ecall_args->size() + rv32::io_words_of(v) + v.commit_reads->size(), 1);
    if (*io_rows > ((size_t)2 << v.seg->po2)) return RK_ERR_CAPACITY;
    return RK_OK;
    RK_GUARD_END
}
int rk_exec_rv32elf_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, const uint32_t* seg_vaddr,
                                 const uint32_t* seg_words, uint32_t n_segs, const uint32_t* d_image_words, uint32_t* d_cpu,
                                 uint32_t* d_program_mult, size_t program_rows, uint32_t* d_register, uint32_t* d_byte_mult,
                                 uint32_t* d_range_mult, uint32_t* d_shift_mult, uint32_t* d_muldiv, size_t muldiv_rows) {
    RK_GUARD_BEGIN
    rv32::ShardOut o;
    RK_TRY(rv32::elf_out(seg_vaddr, seg_words, n_segs, d_image_words, d_cpu, d_program_mult, program_rows, d_register, d_byte_mult,
                         d_range_mult, d_shift_mult, d_muldiv, muldiv_rows, &o));
    return rv32::shard_device<rv32::CS_ELF>(ctx, ex, index, o);
    RK_GUARD_END
}
int rk_exec_rv32mem_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, const uint32_t* seg_vaddr,
                                 const uint32_t* seg_words, uint32_t n_segs, const uint32_t* d_image_words, uint32_t* d_cpu,
                                 uint32_t* d_program_mult, size_t program_rows, uint32_t* d_register, uint32_t* d_byte_mult,
                                 uint32_t* d_range_mult, uint32_t* d_shift_mult, uint32_t* d_muldiv, size_t muldiv_rows,
                                 uint32_t* d_memop, size_t memop_rows, uint32_t* d_memory, size_t memory_rows) {
    RK_GUARD_BEGIN
    rv32::ShardOut o;
    RK_TRY(rv32::elf_out(seg_vaddr, seg_words, n_segs, d_image_words, d_cpu, d_program_mult, program_rows, d_register, d_byte_mult,
                         d_range_mult, d_shift_mult, d_muldiv, muldiv_rows, &o));
    o.memop = d_memop, o.memop_rows = memop_rows, o.memory = d_memory, o.memory_rows = memory_rows;
    return rv32::shard_device<rv32::CS_MEM>(ctx, ex, index, o);
    RK_GUARD_END
}
int rk_exec_rv32io_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, const uint32_t* seg_vaddr,
                                const uint32_t* seg_words, uint32_t n_segs, const uint32_t* d_image_words, uint32_t* d_cpu,
                                uint32_t* d_program_mult, size_t program_rows, uint32_t* d_register, uint32_t* d_byte_mult,
                                uint32_t* d_range_mult, uint32_t* d_shift_mult, uint32_t* d_muldiv, size_t muldiv_rows,
                                uint32_t* d_memop, size_t memop_rows, uint32_t* d_memory, size_t memory_rows, uint32_t* d_io,
                                size_t io_rows, uint32_t h_publics[RK_RV32IO_PUBLICS]) {
    RK_GUARD_BEGIN
    rv32::ShardOut o;
    RK_TRY(rv32::elf_out(seg_vaddr, seg_words, n_segs, d_image_words, d_cpu, d_program_mult, program_rows, d_register, d_byte_mult,
                         d_range_mult, d_shift_mult, d_muldiv, muldiv_rows, &o));
    o.memop = d_memop, o.memop_rows = memop_rows, o.memory = d_memory, o.memory_rows = memory_rows;
    o.io = d_io, o.io_rows = io_rows, o.h_publics = h_publics;
    return rv32::shard_device<rv32::CS_IO>(ctx, ex, index, o);
    RK_GUARD_END
}
int rk_exec_rv32commit_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, const uint32_t* seg_vaddr,
                                    const uint32_t* seg_words, uint32_t n_segs, const uint32_t* d_image_words, uint32_t* d_cpu,
                                    uint32_t* d_program_mult, size_t program_rows, uint32_t* d_register, uint32_t* d_byte_mult,
                                    uint32_t* d_range_mult, uint32_t* d_shift_mult, uint32_t* d_muldiv, size_t muldiv_rows,
                                    uint32_t* d_memop, size_t memop_rows, uint32_t* d_memory, size_t memory_rows, uint32_t* d_io,
                                    size_t io_rows, uint32_t h_publics[RK_RV32COMMIT_PUBLICS], uint32_t* d_log, size_t* n_log) {
    RK_GUARD_BEGIN
    rv32::ShardOut o;
    RK_TRY(rv32::elf_out(seg_vaddr, seg_words, n_segs, d_image_words, d_cpu, d_program_mult, program_rows, d_register, d_byte_mult,
                         d_range_mult, d_shift_mult, d_muldiv, muldiv_rows, &o));
    o.memop = d_memop, o.memop_rows = memop_rows, o.memory = d_memory, o.memory_rows = memory_rows;
    o.io = d_io, o.io_rows = io_rows, o.h_publics = h_publics, o.log = d_log, o.n_log = n_log;
    return rv32::shard_device<rv32::CS_COMMIT>(ctx, ex, index, o);
    RK_GUARD_END
}

}  // extern "C"
