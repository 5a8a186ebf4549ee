// CPU walk through the commit-form lane bodies of raiko_amd/csrc/rv32_rows.hpp (raiko_amd/rv32commit.py): the memop table
// (65 columns, ECR rows) over the merged access list and the io table (64 columns, commit-word rows) of a recorded trace
// with its access list, its ecall side list and its commit reads, in Montgomery form, and the commit log.  The cpu table is
// the io form's (tests/emul/emul_rv32_io.cpp).  Where the GPU finds a row's call by binary search and its commit read by a
// scanned dense index (rv32_shards.hip), this walks the calls in order.  Built by tests/test_rv32_commit.py, which compares
// the tables with raiko_amd/rv32commit.py word for word.
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

static std::vector<MemAccess> accesses(const uint32_t* a, size_t count, unsigned stride) {
    std::vector<MemAccess> out(count);
    for (size_t k = 0; k < count; k++) out[k] = MemAccess{a[stride * k], a[stride * k + 1], a[stride * k + 2], a[stride * k + (stride == 4 ? 3 : 2)]};
    return out;
}

static std::vector<EcallArg> arg_list(const uint32_t* args, size_t count) {
    std::vector<EcallArg> out(count);
    for (size_t k = 0; k < count; k++) out[k] = EcallArg{args[5 * k], args[5 * k + 1], args[5 * k + 2], args[5 * k + 3], args[5 * k + 4]};
    return out;
}

// the shard driver's check of the commit reads (n_reads x (cycle, word address, word)) against the side list and the
// access list (commit_list_ok) -> 1 accepted, 0 refused
extern "C" int emul_rv32commit_list_ok(const uint32_t* args, size_t n_args, const uint32_t* reads, size_t n_reads, const uint32_t* acc,
                                       size_t n_acc) {
    const auto ea = arg_list(args, n_args);
    const auto rd = accesses(reads, n_reads, 3), ac = accesses(acc, n_acc, 4);
    return commit_list_ok(ea.data(), n_args, rd.data(), n_reads, ac.data(), n_acc) ? 1 : 0;
}

// trace: cycles x (pc, ins, a, b, res, next, wr); ecalls: n_ecalls x (cycle, a0 after); args: n_ecalls x (cycle, t0, a0, a1,
// pos); acc: count x (cycle, word address, before, after); reads: n_reads x (cycle, word address, word); memop: memop_rows
// x 65, io: io_rows x 64, log: io_rows x 3 (canonical), *n_log its rows.
// -> 0, or 1 a side list / 2 the lists do not fit the trace / 3 an access is not what its instruction names / 4 a table is
// too small / 5 an io row is not the call's
extern "C" int emul_rv32commit_shard(const uint32_t* trace, size_t cycles, const uint32_t* ecalls, const uint32_t* args, size_t n_ecalls,
                                     const uint32_t* acc, size_t count, const uint32_t* reads, size_t n_reads, uint32_t n_input,
                                     uint32_t pos_start, uint32_t jpos_start, uint32_t* memop, size_t memop_rows, uint32_t* io,
                                     size_t io_rows, uint32_t* log, size_t* n_log) {
    std::fill(memop, memop + memop_rows * CM_MO_W, 0u);
    std::fill(io, io + io_rows * CM_IO_W, 0u);
    std::fill(log, log + io_rows * 3, 0u);
    const auto ea = arg_list(args, n_ecalls);
    const auto rd = accesses(reads, n_reads, 3), ac = accesses(acc, count, 4);
    if (!commit_list_ok(ea.data(), n_ecalls, rd.data(), n_reads, ac.data(), count)) return 2;
    std::vector<MemAccess> merged(count + n_reads);
    merge_accesses(ac.data(), count, rd.data(), n_reads, merged.data());
    if (merged.size() > memop_rows) return 4;
    // the memop rows, over the io form of the trace: an ecall row's a / b / res are the call's a0 / a1 / t0
    std::map<uint32_t, uint32_t> word_ts;
    size_t ec = 0;
    for (size_t k = 0; k < merged.size(); k++) {
        const MemAccess& a = merged[k];
        if (a.cycle >= cycles || (k && a.cycle < merged[k - 1].cycle)) return 2;
        const uint32_t* t = trace + 7 * a.cycle;
        TraceRow r{t[0], t[1], t[2], t[3], t[4], t[5], t[6]};
        const Dec d = decode_io(r.ins);
        uint32_t res = r.res;
        if (d.opc == O_SYSTEM) {
            while (ec < n_ecalls && ea[ec].cycle < a.cycle) ec++;
            if (ec >= n_ecalls || ea[ec].cycle != a.cycle) return 1;
            r.a = ea[ec].a0, r.b = ea[ec].a1, r.res = ea[ec].t0;
            res = 0;
        }
        const uint32_t tsa = 3 * a.cycle + 1;
        auto it = word_ts.find(a.waddr);
        const uint32_t pts = it == word_ts.end() ? 0u : it->second;
        word_ts[a.waddr] = tsa;
        uint32_t* mrow = memop + k * CM_MO_W;
        mrow[G_ONE] = 1;
        if (!memop_row(mrow, a, r, d, res, pts, true, true)) return 3;
    }
    for (size_t j = 0; j < memop_rows; j++) {
        memop[j * CM_MO_W + G_ONE] = 1;
        finish(memop + j * CM_MO_W, CM_MO_W);
    }
    // the io rows: per call its head, READ's word rows or COMMIT's commit-word rows
    size_t q = 0, at = 0, dense = 0;
    uint32_t pos = pos_start, jpos = jpos_start, prev_head_ts = 0;
    bool halted = false;
    for (size_t e = 0; e < n_ecalls; e++) {
        const EcallArg& c = ea[e];
        if (ecalls[2 * e] != c.cycle || c.pos != pos) return 1;
        while (at < count && ac[at].cycle < c.cycle) at++;
        size_t here = 0;
        while (at + here < count && ac[at + here].cycle == c.cycle) here++;
        const uint32_t ncw = c.t0 == 2 ? commit_words(c.a0, c.a1) : 0u;
        if (q + 1 + here + ncw > io_rows) return 4;
        uint32_t* h = io + q * CM_IO_W;
        if (!io_head_row(h, c, ecalls[2 * e + 1], (uint32_t)here, n_input, e > 0, prev_head_ts)) return 5;
        size_t mine = 0;
        while (dense + mine < n_reads && rd[dense + mine].cycle == c.cycle) mine++;
        if (!io_commit_head(h, c, (uint32_t)mine, jpos)) return 5;
        halted = c.t0 == 0;
        io_row_tail(h, pos, true, halted);
        io_commit_tail(h, jpos);
        q++;
        for (uint32_t j = 0; j < here; j++, q++, pos++) {
            if (!io_word_row(io + q * CM_IO_W, c, (uint32_t)here, j, ac[at + j])) return 5;
            io_row_tail(io + q * CM_IO_W, pos, true, 0u);
            io_commit_tail(io + q * CM_IO_W, jpos);
        }
        for (uint32_t j = 0; j < ncw; j++, q++, dense++) {
            uint32_t* row = io + q * CM_IO_W;
            if (!io_commit_row(row, c, j, jpos, rd[dense])) return 5;
            const uint32_t jp = row[Q_JL] | row[Q_JH] << 14;
            io_row_tail(row, pos, true, 0u);
            io_commit_tail(row, jp);
            log[3 * dense] = jp, log[3 * dense + 1] = row[Q_V_LO] | row[Q_V_HI] << 16, log[3 * dense + 2] = row[Q_S] | row[Q_CNT] << 16;
        }
        jpos += c.t0 == 2 ? c.a1 : 0u;
        prev_head_ts = 3 * c.cycle + 1;
    }
    if (dense != n_reads) return 2;
    *n_log = dense;
    for (size_t j = 0; j < io_rows; j++) {
        if (j >= q) {
            io_row_tail(io + j * CM_IO_W, pos, false, halted);
            io_commit_tail(io + j * CM_IO_W, jpos);
        }
        finish(io + j * CM_IO_W, CM_IO_W);
    }
    return 0;
}
