// The kernels of the rv32 shard pipeline that read the two side lists (rv32_shards.hip includes this once, after
// rv32_kernels.hpp): from the access list rv32im-mem's sort keys, heads, links and memop rows; from the ecall side list the
// io form's patch of the trace, its offsets and its io rows, with the commit form's scans and rows as template arguments.
#pragma once
#include "rv32_kernels.hpp"

namespace rv32 {

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
        if (threadIdx.x == 0) atomicOr(err, ERR_HEADS);
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
            if (!memop_row(row, m, r, decode(r.ins), wval[m.cycle], pts[k], io != 0, W == CM_MO_W)) atomicOr(err, ERR_ACCESS);   // not what the instruction names
        }
        for (unsigned c : MO_RANGE) hist_add(hist, row[c], on);
        hist_add(shift_mult, 256u + row[G_TOP], on);   // (1, top byte) -> row 256 + x
        for (unsigned j = 0; j < 6; j++) hist_add(byte_mult, row[G_W + 2 * j] << 8 | row[G_W + 2 * j + 1], on);   // AND (op 1)
    });
}

// the io form: one lane per entry of the ecall side list writes a0 / a1 / t0 into its trace row's a / b / res (0 as the
// executor records them: other chip sets read them); err |= ERR_IO_LIST for an entry that is at no ecall row
__global__ void io_patch_kernel(TraceRow* __restrict__ tr, size_t cycles, const EcallArg* __restrict__ args, size_t count,
                                uint32_t* __restrict__ err) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const EcallArg e = args[k];
    if (e.cycle >= cycles || tr[e.cycle].ins != ECALL_WORD) {
        atomicOr(err, ERR_IO_LIST);
        return;
    }
    tr[e.cycle].a = e.a0;
    tr[e.cycle].b = e.a1;
    tr[e.cycle].res = e.t0;
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
// lines (row_tile: stride 47, odd).  err |= ERR_IO_LIST: the side list is not the trace's ecalls -- a call number that is none of
// the three, a result, a count of stored words or a position that is not the call's, a word that is not where READ stores
// COMMIT (the commit form): rows of CM_IO_W words (stride 65, odd; 128 rows are 33 KiB of LDS).  `acc` is the merged list,
// so necw at a COMMIT's cycle is the count of its commit reads.  Commit-word row k of COMMIT e is computed in closed form
// from (a0, a1, k) (io_commit_row); its word is reads[dense], dense = cblk[e / TB] + coff[e] + k -- no search --, and its
// log tuple goes to row `dense` of the matrix the commit log's digest commits to (clog: n_rows x 6, Montgomery, zeroed
// before) and, canonical, of dlog (n_rows x 3).  err |= ERR_COMMIT_READ: a commit read that is not word k of its call
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
                        atomicOr(err, ERR_COMMIT_READ);
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
            if (!ok) atomicOr(err, ERR_IO_LIST);
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

}  // namespace rv32
