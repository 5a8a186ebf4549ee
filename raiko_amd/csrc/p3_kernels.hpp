// Lane-level bodies of the uni-stark path's own kernels (p3.hip, p3_air.hip, fri_tables.hip) as host/device functions: the GPU kernels are
// these phases with __syncthreads() between them; tests/emul runs the same code on the CPU one emulated lane at a time.
#pragma once
#include "bb.hpp"

namespace p3k {

// ---- lookups: the permutation trace (sp1-core generate_permutation_trace, RECALLED).  desc = the challenge vector
// [alpha | beta^0 | beta^1 ..] (4 words each, n_chal words), the flat interactions (kind, bus, mult_is_const, mult, n_values,
// slots...; constants as Montgomery words; columns renumbered to slots of the `used` list), then the n_used distinct
// columns the interactions read (c < w: column c of the main trace; otherwise column c - w of the row-major preprocessed
// matrix `prep`, pw words a row).  A workgroup takes PERM_ROWS rows of the row-major trace: first every wave
// stages the used columns of its rows in LDS -- one row per load instruction, the lanes along the used columns, so a row's
// cache lines are fetched once instead of once per interaction --, then one lane per row walks the interactions out of LDS
// (slot-major: conflict-free).  out = 4 (nb + 1) columns of n words: the nb batch entries, then the row totals (the
// prefix sums turn those into the running sum in place).
constexpr int PERM_ROWS = 256, PERM_LD = PERM_ROWS + 1;   // odd slot stride: the staging writes (lanes along slots) and the reads (lanes along rows) both spread over the banks
struct PermArgs {
    uint32_t* out;
    const uint32_t* trace;
    const uint32_t* desc;
    size_t n, w;
    uint32_t n_chal, n_lookups, wm, n_used, desc_words;
    const uint32_t* prep = nullptr;   // preprocessed rows (an rk_p3_key's), null when no interaction reads one
    size_t pw = 0;
};
// phase 1: lane `tid` of workgroup `blk` stages its share of the tile (n_used x PERM_LD words).  A wave takes 64 rows, eight
// at a time: the loads of eight rows are issued before the first LDS store waits for any of them (one row per iteration
// would serialise 64 memory latencies per wave)
RK_HD void perm_stage(const PermArgs& a, size_t blk, unsigned tid, uint32_t* tile) {
    const size_t r0 = blk * PERM_ROWS;
    const uint32_t* used = a.desc + a.desc_words;
    const unsigned wave = tid >> 6, lane = tid & 63;
    constexpr int GROUP = 8, PER_LANE = 2;   // 2 x 64 lanes cover the 120 columns an AIR's interactions may read
    uint32_t col[PER_LANE];
    for (int q = 0; q < PER_LANE; q++) col[q] = lane + 64 * q < a.n_used ? used[lane + 64 * q] : 0;
    for (unsigned i = 0; i < 64; i += GROUP) {
        uint32_t v[GROUP][PER_LANE];
#pragma unroll
        for (int j = 0; j < GROUP; j++) {
            const size_t r = r0 + wave * 64 + i + j;
            const size_t rr = r < a.n ? r : a.n - 1;                          // past the end: a valid row, never stored
            const uint32_t* row = a.trace + rr * a.w;
            const uint32_t* prow = a.prep + rr * a.pw;                        // only read for columns >= w, which need a.prep
#pragma unroll
            for (int q = 0; q < PER_LANE; q++)
                v[j][q] = lane + 64 * q < a.n_used ? (col[q] < a.w ? row[col[q]] : prow[col[q] - a.w]) : 0;
        }
#pragma unroll
        for (int j = 0; j < GROUP; j++) {
            const unsigned lr = wave * 64 + i + j;
            if (r0 + lr >= a.n) continue;
#pragma unroll
            for (int q = 0; q < PER_LANE; q++)
                if (lane + 64 * q < a.n_used) tile[(lane + 64 * q) * PERM_LD + lr] = v[j][q];
        }
    }
}
// phase 2: lane `tid` walks the interactions of its row.  (Inverting the denominators of eight interactions together --
// Montgomery's trick -- was measured and dropped: 0.50 ms against 0.45 at 2^20 rows x 16 interactions; the three arrays
// it keeps per lane cost more than the fourteen base-field powers it saves.)
RK_HD void perm_row(const PermArgs& a, size_t blk, unsigned tid, const uint32_t* tile) {
    const size_t r = blk * PERM_ROWS + tid;
    if (r >= a.n) return;
    const uint32_t* row = tile + tid;
    const uint32_t* ch = a.desc;
    const uint32_t* d = a.desc + a.n_chal;
    const bb::Ext alpha{{ch[0], ch[1], ch[2], ch[3]}};
    bb::Ext total = bb::ext_zero(), entry = bb::ext_zero();
    const uint32_t nb = (a.n_lookups + 1) / 2;
    for (uint32_t i = 0; i < a.n_lookups; i++) {
        const uint32_t kind = d[0], bus = d[1], is_const = d[2], mult = d[3], nv = d[4];
        bb::Ext rlc = bb::add(alpha, bb::scale(bb::Ext{{ch[4], ch[5], ch[6], ch[7]}}, bus));
        for (uint32_t j = 0; j < nv; j++) {
            const uint32_t* b = ch + 8 + 4 * j;
            rlc = bb::add(rlc, bb::scale(bb::Ext{{b[0], b[1], b[2], b[3]}}, row[d[5 + j] * PERM_LD]));
        }
        const uint32_t m = is_const ? mult : row[mult * PERM_LD];
        const bb::Ext term = bb::scale(bb::inv(rlc, a.wm), kind == 0 ? m : bb::neg(m));
        entry = bb::add(entry, term);
        d += 5 + nv;
        if ((i & 1u) || i + 1 == a.n_lookups) {
            const uint32_t b = i >> 1;
            for (int k = 0; k < 4; k++) a.out[(size_t)(4 * b + k) * a.n + r] = entry.c[k];
            total = bb::add(total, entry);
            entry = bb::ext_zero();
        }
    }
    for (int k = 0; k < 4; k++) a.out[(size_t)(4 * nb + k) * a.n + r] = total.c[k];
}

// ---- the Poseidon2 chip's rows (rk_p2_chip_trace): one lane per permutation; tab = rc_ext | rc_int | diag (Montgomery words)
struct P2ChipLayout {
    uint32_t W, RP, width;
    RK_HD uint32_t in() const { return 0; }
    RK_HD uint32_t x3(uint32_t r) const { return r < 4 ? W + 2 * W * r : W + 8 * W + 2 * RP - 1 + W + 2 * W * (r - 4); }
    RK_HD uint32_t post(uint32_t r) const { return x3(r) + W; }
    RK_HD uint32_t x3i(uint32_t k) const { return W + 8 * W + k; }
    RK_HD uint32_t s0(uint32_t k) const { return W + 8 * W + RP + (k - 1); }   // k >= 1
    RK_HD uint32_t int_out() const { return W + 8 * W + 2 * RP - 1; }
    RK_HD uint32_t mult() const { return width - 1; }
    RK_HD uint32_t out() const { return post(7); }
};
template <int W, int M4>
RK_HD void chip_m_ext(uint32_t (&c)[W]) {
    uint32_t sums[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < W; i += 4) {
        const uint32_t a = c[i], b = c[i + 1], d = c[i + 2], e = c[i + 3];
        if (M4 == 0) {
            const uint32_t t0 = bb::add(a, b), t1 = bb::add(d, e), t2 = bb::add(bb::dbl(b), t1), t3 = bb::add(bb::dbl(e), t0);
            const uint32_t t4 = bb::add(bb::dbl(bb::dbl(t1)), t3), t5 = bb::add(bb::dbl(bb::dbl(t0)), t2);
            c[i] = bb::add(t3, t5), c[i + 1] = t5, c[i + 2] = bb::add(t2, t4), c[i + 3] = t4;
        } else {
            const uint32_t s = bb::add(bb::add(a, b), bb::add(d, e));
            c[i] = bb::add(bb::add(s, a), bb::dbl(b));
            c[i + 1] = bb::add(bb::add(s, b), bb::dbl(d));
            c[i + 2] = bb::add(bb::add(s, d), bb::dbl(e));
            c[i + 3] = bb::add(bb::add(s, e), bb::dbl(a));
        }
#pragma unroll
        for (int j = 0; j < 4; j++) sums[j] = bb::add(sums[j], c[i + j]);
    }
#pragma unroll
    for (int i = 0; i < W; i++) c[i] = bb::add(c[i], sums[i & 3]);
}
// the permutation: c = the input state on entry, the output on return; ROWS: the intermediate values go to their columns
template <int W, int RP, int M4, bool ROWS>
RK_HD void chip_permute(uint32_t (&c)[W], uint32_t* row, const uint32_t* tab, const P2ChipLayout& L) {
    const uint32_t *rc_ext = tab, *rc_int = tab + 8 * W, *diag = rc_int + RP;
    chip_m_ext<W, M4>(c);
    for (int rd = 0; rd < 8; rd++) {
        if (rd == 4) {
            for (int k = 0; k < RP; k++) {
                if (ROWS && k > 0) row[L.s0(k)] = c[0];
                const uint32_t t = bb::add(c[0], rc_int[k]), x3 = bb::mul(bb::sqr(t), t);
                if (ROWS) row[L.x3i(k)] = x3;
                c[0] = bb::mul(bb::sqr(x3), t);
                uint32_t sum = 0;
#pragma unroll
                for (int i = 0; i < W; i++) sum = bb::add(sum, c[i]);
#pragma unroll
                for (int i = 0; i < W; i++) c[i] = bb::add(sum, bb::mul(c[i], diag[i]));
            }
            if (ROWS) {
#pragma unroll
                for (int i = 0; i < W; i++) row[L.int_out() + i] = c[i];
            }
        }
#pragma unroll
        for (int i = 0; i < W; i++) {
            const uint32_t s = bb::add(c[i], rc_ext[rd * W + i]), x3 = bb::mul(bb::sqr(s), s);
            if (ROWS) row[L.x3(rd) + i] = x3;
            c[i] = bb::mul(bb::sqr(x3), s);
        }
        chip_m_ext<W, M4>(c);
        if (ROWS) {
#pragma unroll
            for (int i = 0; i < W; i++) row[L.post(rd) + i] = c[i];
        }
    }
}
template <int W, int RP, int M4>
RK_HD void chip_row(uint32_t* row, const uint32_t* in, uint32_t mult, const uint32_t* tab, const P2ChipLayout& L) {
    uint32_t c[W];
#pragma unroll
    for (int i = 0; i < W; i++) row[i] = c[i] = in[i];
    chip_permute<W, RP, M4, true>(c, row, tab, L);
    row[L.mult()] = mult;
}

// ---- the FRI commit-phase tables (rk_fri_chip_rows_device; column plans: raiko_amd/fri_chip.py).  pub = beta 4 R | roots
// 8 R | final 4; rec = per query: index | per round: joining reduced opening 4, sibling 4, path 8 lfh (rk_p3_fri_openings).
// Every cell is a Montgomery word; rows the lanes do not write stay zero (the caller clears the buffers).
struct FriArgs {
    uint32_t L, R, Q;           // log_max, rounds, queries
    uint32_t gen_l, wm;         // the generator of the 2^L subgroup, the extension's W
    const uint32_t *pub, *rec;
    uint32_t *fold, *path, *claims, *chip_in, *chip_mult;
    uint32_t xcol, shiftm;      // xcol = 1: the fold rows end in X = shift (1 - 2 bit) x0 (rk_fri_reduce_rows_device); claims may then be null
    uint32_t firstcol;          // 1: behind X the column FIRST = the row is a query's first (rk_fri_transcript_rows_device)
    RK_HD uint32_t lfh(uint32_t rd) const { return L - 1 - rd; }
    RK_HD size_t per_record() const { return 1 + 8 * (size_t)R + 8 * steps_before(R); }
    RK_HD size_t steps_before(uint32_t rd) const { return (size_t)rd * (L - 1) - (size_t)rd * (rd - 1) / 2; }   // sum of lfh(r), r < rd
    RK_HD size_t rec_round(uint32_t rd) const { return 1 + 8 * (size_t)rd + 8 * steps_before(rd); }
    RK_HD uint32_t fold_width() const { return 41 + R + 2 * (L - 1) + xcol + firstcol; }
    RK_HD uint32_t path_width() const { return 48 + R; }
};
constexpr uint32_t FRI_CLAIMS_WIDTH = 8;
// fold columns: query | round | real | idx | bit | pidx | ro 4 | sib 4 | cur 4 | e0 4 | e1 4 | folded 4 | x0 | x0^2 |
// leaf digest 8 | zero | round one-hot R | bits of pidx L-1 | partial products of x0 L-1 (round 0 only)
// One lane per query walks its rounds (the chain is sequential): fold rows q R + rd (all but the digest) and claim rows.
RK_HD void fri_fold_lane(const FriArgs& a, uint32_t q) {
    const uint32_t* rec = a.rec + a.per_record() * q;
    uint32_t idx = bb::decode(rec[0]);
    const uint32_t fw = a.fold_width();
    bb::Ext folded = bb::ext_zero();
    uint32_t x0 = 0;
    for (uint32_t rd = 0; rd < a.R; rd++) {
        const uint32_t lfh = a.lfh(rd), bit = idx & 1u, pidx = idx >> 1;
        const uint32_t* rr = rec + a.rec_round(rd);
        uint32_t* row = a.fold + ((size_t)q * a.R + rd) * fw;
        const bb::Ext ro{{rr[0], rr[1], rr[2], rr[3]}}, sib{{rr[4], rr[5], rr[6], rr[7]}};
        const bb::Ext cur = rd ? bb::add(folded, ro) : ro;
        const bb::Ext e0 = bit ? sib : cur, e1 = bit ? cur : sib;
        uint32_t* pp = row + 41 + a.R + (a.L - 1);
        if (rd == 0) {   // x0 = gen(L)^bitrev(pidx, L-1) as the product over the bits, c_j = gen(L)^(2^(L-2-j))
            uint32_t c[32];
            c[a.L - 2] = a.gen_l;
            for (uint32_t j = a.L - 2; j > 0; j--) c[j - 1] = bb::sqr(c[j]);
            x0 = bb::ONE;
            for (uint32_t j = 0; j + 1 < a.L; j++) {
                if ((pidx >> j) & 1u) x0 = bb::mul(x0, c[j]);
                pp[j] = x0;
            }
        } else {
            x0 = bit ? bb::neg(bb::sqr(x0)) : bb::sqr(x0);
        }
        const bb::Ext beta{{a.pub[4 * rd], a.pub[4 * rd + 1], a.pub[4 * rd + 2], a.pub[4 * rd + 3]}};
        const bb::Ext slope = bb::scale(bb::sub(e1, e0), bb::inv(bb::sub(bb::neg(x0), x0)));
        folded = bb::add(e0, bb::mul(bb::sub(beta, bb::ext_from(x0)), slope, a.wm));
        const uint32_t qm = bb::encode(q), rdm = bb::encode(rd), idxm = bb::encode(idx);
        row[0] = qm, row[1] = rdm, row[2] = bb::ONE, row[3] = idxm, row[4] = bit ? bb::ONE : 0u, row[5] = bb::encode(pidx);
        for (int k = 0; k < 4; k++) {
            row[6 + k] = ro.c[k], row[10 + k] = sib.c[k], row[14 + k] = cur.c[k];
            row[18 + k] = e0.c[k], row[22 + k] = e1.c[k], row[26 + k] = folded.c[k];
        }
        row[30] = x0, row[31] = bb::sqr(x0);
        row[41 + rd] = bb::ONE;
        for (uint32_t j = 0; j < lfh; j++) row[41 + a.R + j] = (pidx >> j) & 1u ? bb::ONE : 0u;
        if (a.xcol) row[fw - 1 - a.firstcol] = bb::mul(a.shiftm, bit ? bb::neg(x0) : x0);   // the point of the height-(L - rd) coset at idx
        if (a.firstcol) row[fw - 1] = rd == 0 ? bb::ONE : 0u;
        if (a.claims) {
            uint32_t* cl = a.claims + ((size_t)q * a.R + rd) * FRI_CLAIMS_WIDTH;
            cl[0] = qm, cl[1] = rdm, cl[2] = idxm, cl[7] = bb::ONE;
            for (int k = 0; k < 4; k++) cl[3 + k] = ro.c[k];
        }
        idx = pidx;
    }
}
// path columns: merkle_path_air's 43 (cur 8 | sib 8 | bit | left 8 | right 8 | parent 8 | real | last) | first | pos |
// steps left | query | round | round one-hot R.  Lane t = rd Q + q (round-major: the lanes of a wave share the path
// length) hashes the leaf (e0 | e1 of its fold row, whose digest cells it fills), walks the lfh compressions and writes
// the path rows steps_before(rd) Q + q lfh + s and the chip's inputs (row offset + t: the leaf state, then left | right of every step).
struct FriPathState {
    uint32_t cur[8];
    uint32_t pos, rd, q, lfh, t;
    size_t off;   // first path row; off + t = first chip input
};
template <int M4>
RK_HD void fri_path_begin(const FriArgs& a, uint32_t t, const uint32_t* tab, const P2ChipLayout& L, FriPathState& st) {
    st.t = t, st.rd = t / a.Q, st.q = t % a.Q, st.lfh = a.lfh(st.rd);
    st.off = a.steps_before(st.rd) * a.Q + (size_t)st.q * st.lfh;
    uint32_t* frow = a.fold + ((size_t)st.q * a.R + st.rd) * a.fold_width();
    uint32_t* cin = a.chip_in + (st.off + t) * 16;
    uint32_t c[16];
    for (int i = 0; i < 8; i++) cin[i] = c[i] = frow[18 + i];
    for (int i = 8; i < 16; i++) cin[i] = c[i] = 0;
    a.chip_mult[st.off + t] = bb::ONE;
    chip_permute<16, 13, M4, false>(c, nullptr, tab, L);
    for (int i = 0; i < 8; i++) frow[32 + i] = st.cur[i] = c[i];
    st.pos = (bb::decode(a.rec[a.per_record() * st.q]) >> st.rd) >> 1;
}
// step s of the lane's path: every cell of the row (path_width words at `row`), the chip input of the compression
template <int M4>
RK_HD void fri_path_step(const FriArgs& a, FriPathState& st, uint32_t s, const uint32_t* tab, const P2ChipLayout& L, uint32_t* row) {
    const uint32_t* sib = a.rec + a.per_record() * st.q + a.rec_round(st.rd) + 8 + 8 * s;
    uint32_t* cin = a.chip_in + (st.off + st.t + 1 + s) * 16;
    const uint32_t bit = st.pos & 1u;
    uint32_t c[16];
    for (int i = 0; i < 8; i++) {
        c[i] = bit ? sib[i] : st.cur[i];
        c[8 + i] = bit ? st.cur[i] : sib[i];
        row[i] = st.cur[i], row[8 + i] = sib[i], row[17 + i] = c[i], row[25 + i] = c[8 + i];
    }
    for (int i = 0; i < 16; i++) cin[i] = c[i];
    a.chip_mult[st.off + st.t + 1 + s] = bb::ONE;
    chip_permute<16, 13, M4, false>(c, nullptr, tab, L);
    for (int i = 0; i < 8; i++) row[33 + i] = st.cur[i] = c[i];
    row[16] = bit ? bb::ONE : 0u;
    row[41] = bb::ONE;
    row[42] = s + 1 == st.lfh ? bb::ONE : 0u;
    row[43] = s == 0 ? bb::ONE : 0u;
    row[44] = bb::encode(st.pos);
    row[45] = bb::encode(st.lfh - s);
    row[46] = bb::encode(st.q), row[47] = bb::encode(st.rd);
    for (uint32_t r = 0; r < a.R; r++) row[48 + r] = r == st.rd ? bb::ONE : 0u;
    st.pos >>= 1;
}
template <int M4>
RK_HD void fri_path_lane(const FriArgs& a, uint32_t t, const uint32_t* tab, const P2ChipLayout& L) {
    FriPathState st;
    fri_path_begin<M4>(a, t, tab, L, st);
    for (uint32_t s = 0; s < st.lfh; s++) fri_path_step<M4>(a, st, s, tab, L, a.path + (st.off + s) * a.path_width());
}

// ---- the reduced-openings table (rk_fri_reduce_rows_device; column plan and schedule: raiko_amd/fri_reduce.py).  One row
// per (query, slot, column); a slot is an opened matrix or the single row of a round without one.  slots = 8 plain words
// each: round | width | points | offset of the matrix's row in a record | gen(log_n) (Montgomery) | last slot of its round |
// first row within a query | 0.  pub = alpha 4 | zeta 4 | per slot and point: first power A 4, S 4 (zero where the slot has
// no such point); rec = per query: index | the opened rows (rk_p3_fri_inputs); apow = alpha^(2^i), i < 32.
// columns: query | round | idx | X | real | last column | receives | ends the query | column | P | per point: power 4,
// running sum 4, quotient 4 | the round's running reduced opening 4 | slot one-hot M
constexpr uint32_t FRI_REDUCE_FIXED = 38, FRI_REDUCE_TPB = 256, FRI_REDUCE_SLOT_WORDS = 8;
struct FriReduceArgs {
    uint32_t L, R, Q, M;        // log_max, rounds, queries, slots
    uint32_t rows_per_query, wm, shiftm, gen_l;
    size_t per_record;
    const uint32_t *slots, *pub, *rec, *apow;
    uint32_t* out;
    uint32_t stride;            // words from one row to the next; 0 = the table's own width (rk_fri_open_rows_device: the wider row of reduce'')
    RK_HD uint32_t width() const { return FRI_REDUCE_FIXED + M; }
    RK_HD uint32_t row_words() const { return stride ? stride : width(); }
};
RK_HD bb::Ext fri_load_ext(const uint32_t* p) { return bb::Ext{{p[0], p[1], p[2], p[3]}}; }
struct FriReduceCtx {
    uint32_t idx, x;            // the query's index entering the round, the point of the round's coset there
};
RK_HD FriReduceCtx fri_reduce_begin(const FriReduceArgs& a, uint32_t q, uint32_t rd) {
    const uint32_t idx = bb::decode(a.rec[a.per_record * q]) >> rd;
    uint32_t g = a.gen_l;
    for (uint32_t i = 0; i < rd; i++) g = bb::sqr(g);
    return FriReduceCtx{idx, bb::mul(a.shiftm, bb::pow(g, bb::bitrev(idx, a.L - rd)))};
}
// what a lane carries for its column: the opened value, per point the power A alpha^col and -- `sum` -- first its own
// term power * P, after the scan the running sum up to and including its column
struct FriReduceLane {
    uint32_t p;
    bb::Ext pw[2], sum[2];
};
RK_HD void fri_reduce_term(const FriReduceArgs& a, uint32_t q, uint32_t m, uint32_t col, FriReduceLane& ln) {
    const uint32_t* slot = a.slots + FRI_REDUCE_SLOT_WORDS * m;
    ln.p = slot[2] ? a.rec[a.per_record * q + 1 + slot[3] + col] : 0u;
    bb::Ext ac = bb::ext_one();
    for (uint32_t i = 0; col >> i; i++)
        if ((col >> i) & 1u) ac = bb::mul(ac, fri_load_ext(a.apow + 4 * i), a.wm);
#pragma unroll
    for (uint32_t j = 0; j < 2; j++) {
        ln.pw[j] = j < slot[2] ? bb::mul(fri_load_ext(a.pub + 8 + 16 * m + 8 * j), ac, a.wm) : bb::ext_zero();
        ln.sum[j] = bb::scale(ln.pw[j], ln.p);
    }
}
// one step of a scan: the running sums of a lane further down join this lane's
RK_HD void fri_reduce_join(FriReduceLane& ln, const bb::Ext& s0, const bb::Ext& s1) {
    ln.sum[0] = bb::add(ln.sum[0], s0), ln.sum[1] = bb::add(ln.sum[1], s1);
}
// the row of (query, slot m, column) once the lane's sums are final; rop = the round's reduced opening before this
// matrix.  Returns it after this row: on a matrix's last column the quotients (sum - S) / (X - z) join.
RK_HD bb::Ext fri_reduce_row(const FriReduceArgs& a, uint32_t q, uint32_t m, uint32_t col, const FriReduceCtx& cx, const FriReduceLane& ln,
                             bb::Ext rop) {
    const uint32_t* slot = a.slots + FRI_REDUCE_SLOT_WORDS * m;
    uint32_t* row = a.out + ((size_t)q * a.rows_per_query + slot[6] + col) * a.row_words();
    const bool last = col + 1 == slot[1];
    bb::Ext quot[2] = {bb::ext_zero(), bb::ext_zero()};
    if (last) {
        const bb::Ext zeta = fri_load_ext(a.pub + 4);
#pragma unroll
        for (uint32_t j = 0; j < 2; j++) {   // fixed trip count: quot and the lane's sums stay in registers
            if (j >= slot[2]) break;
            const bb::Ext z = j ? bb::scale(zeta, slot[4]) : zeta;
            const bb::Ext num = bb::sub(ln.sum[j], fri_load_ext(a.pub + 8 + 16 * m + 8 * j + 4));
            quot[j] = bb::mul(num, bb::inv(bb::sub(bb::ext_from(cx.x), z), a.wm), a.wm);
            rop = bb::add(rop, quot[j]);
        }
    }
    row[0] = bb::encode(q), row[1] = bb::encode(slot[0]), row[2] = bb::encode(cx.idx), row[3] = cx.x, row[4] = bb::ONE;
    row[5] = last ? bb::ONE : 0u, row[6] = last && slot[5] ? bb::ONE : 0u, row[7] = last && m + 1 == a.M ? bb::ONE : 0u;
    row[8] = bb::encode(col), row[9] = ln.p;
#pragma unroll
    for (int j = 0; j < 2; j++)
        for (int k = 0; k < 4; k++) row[10 + 12 * j + k] = ln.pw[j].c[k], row[14 + 12 * j + k] = ln.sum[j].c[k], row[18 + 12 * j + k] = quot[j].c[k];
    for (int k = 0; k < 4; k++) row[34 + k] = rop.c[k];
    for (uint32_t s = 0; s < a.M; s++) row[FRI_REDUCE_FIXED + s] = s == m ? bb::ONE : 0u;
    return rop;
}

// ---- the input-batch openings (rk_fri_open_rows_device; column plans: raiko_amd/fri_open.py).  reduce'' = the reduce row
// with the sponge columns behind the slot one-hot: PTR 8 | BUF 8 | CAP 8 | OUT 16 | FLUSH | GEND | BATCH.  A group = the
// matrices of one (round, batch): consecutive slots, hence consecutive reduce rows, one absorbed cell per row.
// groups = 8 plain words each: first slot | slots | cells | first row within a query | permutations of the groups before
// it (per query) | batch | round | 0.  rowinfo = 2 words per row of a query: the cell's number within its group | flags
// (1 absorbs, 2 ends its group, batch << 2; batch 0 trace, 1 permutation, 2 quotient, 3 preprocessed).  levels = 40 words per
// batch present, in batch-number order (the preprocessed tree last): batch | B (tree height) | rows of the
// batches before it | chip inputs of the batches before it | injections | offset of the batch's path in a path record |
// the group its leaf is | L - B | then per step the group injected there (FRI_OPEN_NONE: none).
// digests = 8 words per (query, group), written by the sponge lanes and read by the ipath lanes.
constexpr uint32_t FRI_OPEN_SPONGE_COLS = 43, FRI_OPEN_GROUP_WORDS = 8, FRI_OPEN_LEVEL_WORDS = 40, FRI_OPEN_NONE = 0xffffffffu;
constexpr uint32_t FRI_OPEN_IPATH_FIXED = 68;
struct FriOpenArgs {
    uint32_t L, Q, M, G, NB;    // log_max, queries, slots, groups, batches present
    uint32_t rows_per_query, stride, sponge_at;   // reduce'': words per row, the first sponge column
    size_t per_record, per_path, chip_base;       // chip_base: the chip's first input row behind the commit-phase paths
    const uint32_t *slots, *groups, *rowinfo, *levels, *rec, *paths;
    uint32_t *reduce, *ipath, *state_in, *state_mult, *chip_in, *chip_mult, *digests;
    RK_HD uint32_t ipath_width() const { return FRI_OPEN_IPATH_FIXED + NB; }
};
// One lane per (query, group), t = g Q + q (group-major: the lanes of a wave share the chain's length): the sponge of
// hash_elems with pad_free over the group's cells.  OUT goes into the flush rows, the 16 cells entering every permutation
// into the state chip's inputs, the digest into `digests`.
template <int M4>
RK_HD void fri_open_sponge_lane(const FriOpenArgs& a, uint32_t t, const uint32_t* tab, const P2ChipLayout& L) {
    const uint32_t g = t / a.Q, q = t % a.Q;
    const uint32_t* gr = a.groups + FRI_OPEN_GROUP_WORDS * g;
    const uint32_t n_perm = (gr[2] + 7) / 8;
    const size_t srow0 = (size_t)gr[4] * a.Q + (size_t)q * n_perm;
    uint32_t* row = a.reduce + ((size_t)q * a.rows_per_query + gr[3]) * a.stride + a.sponge_at + 24;
    const uint32_t* rec = a.rec + a.per_record * q + 1;
    uint32_t s[16];
    for (int i = 0; i < 16; i++) s[i] = 0;
    uint32_t pos = 0, blk = 0, cell = 0;
    for (uint32_t m = gr[0]; m < gr[0] + gr[1]; m++) {
        const uint32_t* slot = a.slots + FRI_REDUCE_SLOT_WORDS * m;
        for (uint32_t col = 0; col < slot[1]; col++, cell++, row += a.stride) {
            s[pos++] = rec[slot[3] + col];
            if (pos == 8 || cell + 1 == gr[2]) {
                uint32_t* sin = a.state_in + (srow0 + blk) * 16;
                for (int i = 0; i < 16; i++) sin[i] = s[i];
                a.state_mult[srow0 + blk] = bb::ONE;
                chip_permute<16, 13, M4, false>(s, nullptr, tab, L);
                for (int i = 0; i < 16; i++) row[i] = s[i];
                pos = 0, blk++;
            }
        }
    }
    uint32_t* dig = a.digests + ((size_t)q * a.G + g) * 8;
    for (int i = 0; i < 8; i++) dig[i] = s[i];
}
// One lane per reduce row: PTR, BUF, CAP, FLUSH, GEND and BATCH from the P cells of the row's block (the reduce kernel wrote
// them) and the OUT of the flush row before the block (the sponge lanes wrote it).  No row reads what another lane writes here.
RK_HD void fri_open_fill_lane(const FriOpenArgs& a, size_t r) {
    const uint32_t i = (uint32_t)(r % a.rows_per_query);
    const uint32_t cell = a.rowinfo[2 * i], flags = a.rowinfo[2 * i + 1];
    if (!(flags & 1u)) return;
    uint32_t* row = a.reduce + r * a.stride;
    uint32_t* sp = row + a.sponge_at;
    const uint32_t pos = cell & 7u;
    const bool gend = (flags & 2u) != 0;
    for (uint32_t j = 0; j < 8; j++) sp[j] = j == pos ? bb::ONE : 0u;
    for (uint32_t j = 0; j <= pos; j++) sp[8 + j] = (row - (size_t)(pos - j) * a.stride)[9];
    if (cell >= 8) {
        const uint32_t* prev = row - (size_t)(pos + 1) * a.stride + a.sponge_at + 24;
        for (uint32_t j = pos + 1; j < 8; j++) sp[8 + j] = prev[j];
        for (uint32_t j = 0; j < 8; j++) sp[16 + j] = prev[8 + j];
    }
    sp[40] = pos == 7 || gend ? bb::ONE : 0u;
    sp[41] = gend ? bb::ONE : 0u;
    sp[42] = bb::encode(flags >> 2);
}
// ipath columns: cur 8 | sib 8 | bit | left 8 | right 8 | parent 8 | real | last | first | pos | steps left | query | batch |
// pos >> 1 | injects | ex 8 | node 8 | round of the leaf (first row) | round of the injection | batch one-hot NB.
// One lane per (query, batch), t = k Q + q (batch-major: the lanes of a wave share the tree's height), walks the levels of
// rk_mmcs_verify: parent = compress(left, right), and where a group of shorter matrices joins node = compress(parent, ex);
// rows (rows before + q B + s), and the chip inputs of its compressions in the order it performs them.
template <int M4>
RK_HD void fri_open_ipath_lane(const FriOpenArgs& a, uint32_t t, const uint32_t* tab, const P2ChipLayout& L) {
    const uint32_t k = t / a.Q, q = t % a.Q;
    const uint32_t* lv = a.levels + FRI_OPEN_LEVEL_WORDS * k;
    const uint32_t B = lv[1], w = a.ipath_width();
    uint32_t pos = bb::decode(a.rec[a.per_record * q]) >> lv[7];
    uint32_t cur[8];
    const uint32_t* leaf = a.digests + ((size_t)q * a.G + lv[6]) * 8;
    for (int i = 0; i < 8; i++) cur[i] = leaf[i];
    uint32_t* row = a.ipath + ((size_t)lv[2] + (size_t)q * B) * w;
    size_t chip = a.chip_base + lv[3] + (size_t)q * (B + lv[4]);
    const uint32_t* sib = a.paths + a.per_path * q + lv[5];
    for (uint32_t s = 0; s < B; s++, row += w, sib += 8) {
        const uint32_t bit = pos & 1u, cnt = B - s;
        uint32_t c[16];
        for (int i = 0; i < 8; i++) {
            c[i] = bit ? sib[i] : cur[i];
            c[8 + i] = bit ? cur[i] : sib[i];
            row[i] = cur[i], row[8 + i] = sib[i], row[17 + i] = c[i], row[25 + i] = c[8 + i];
        }
        uint32_t* cin = a.chip_in + chip * 16;
        for (int i = 0; i < 16; i++) cin[i] = c[i];
        a.chip_mult[chip++] = bb::ONE;
        chip_permute<16, 13, M4, false>(c, nullptr, tab, L);
        for (int i = 0; i < 8; i++) row[33 + i] = cur[i] = c[i];
        row[16] = bit ? bb::ONE : 0u;
        row[41] = bb::ONE;
        row[42] = s + 1 == B ? bb::ONE : 0u;
        row[43] = s == 0 ? bb::ONE : 0u;
        row[44] = bb::encode(pos);
        row[45] = bb::encode(cnt);
        row[46] = bb::encode(q), row[47] = bb::encode(lv[0]), row[48] = bb::encode(pos >> 1);
        const uint32_t gi = lv[8 + s];
        if (gi != FRI_OPEN_NONE) {
            const uint32_t* ex = a.digests + ((size_t)q * a.G + gi) * 8;
            for (int i = 0; i < 8; i++) c[i] = cur[i], c[8 + i] = row[50 + i] = ex[i];
            cin = a.chip_in + chip * 16;
            for (int i = 0; i < 16; i++) cin[i] = c[i];
            a.chip_mult[chip++] = bb::ONE;
            chip_permute<16, 13, M4, false>(c, nullptr, tab, L);
            for (int i = 0; i < 8; i++) cur[i] = c[i];
            row[49] = bb::ONE;
            row[67] = bb::encode(a.L + 1 - cnt);
        }
        for (int i = 0; i < 8; i++) row[58 + i] = cur[i];
        if (s == 0) row[66] = bb::encode(a.L - cnt);
        for (uint32_t j = 0; j < a.NB; j++) row[FRI_OPEN_IPATH_FIXED + j] = j == k ? bb::ONE : 0u;
        pos >>= 1;
    }
}

// ---- the transcript (rk_fri_transcript_rows_device; column plans: raiko_amd/fri_transcript.py).  steps = 10 plain words per
// duplex permutation of the challenger: words absorbed | their offset in `observed` | per output cell 0..7 the sample_bits
// slot that consumes it + 1 (0: none; slot 0 = the proof of work, slot q + 1 = query q).
// transcript columns: IN 16 | OUT 16 | step one-hot N | real | per output cell: consumed by a sample_bits 8 | its slot 8.
// bits columns: slot | value | 31 bits | b30 b29 b28 | real | slot - 1 | idx | is the proof of work | is a query.
// `samples` = one word per slot, the output cell the chain kernel saw consumed there.
constexpr uint32_t FRI_TRANSCRIPT_STEP_WORDS = 10, FRI_TRANSCRIPT_FIXED = 49, FRI_BITS_WIDTH = 39, FRI_TRANSCRIPT_MAX_STEPS = 1024;
struct FriTranscriptArgs {
    uint32_t N, Q, L, pow_bits;     // duplex permutations, queries, log_max
    size_t state_base;              // the state chip's first input row behind the sponge's
    const uint32_t *steps, *observed;
    uint32_t *transcript, *bits, *state_in, *state_mult, *samples;
    RK_HD uint32_t width() const { return FRI_TRANSCRIPT_FIXED + N; }
};
// The chain as one lane walks it, all 16 cells in its registers: what fri_transcript_chain_kernel (fri_tables.hip) does
// with one lane per cell, and what the CPU emulation runs.  Step s overwrites the first n_in cells with observed words,
// permutes, and leaves IN | OUT in row s, IN in the state chip's inputs, the consumed cells in `samples`.
template <int M4>
RK_HD void fri_transcript_chain_lane(const FriTranscriptArgs& a, const uint32_t* tab, const P2ChipLayout& L) {
    uint32_t c[16];
    for (int i = 0; i < 16; i++) c[i] = 0;
    for (uint32_t s = 0; s < a.N; s++) {
        const uint32_t* st = a.steps + FRI_TRANSCRIPT_STEP_WORDS * s;
        uint32_t* row = a.transcript + (size_t)s * a.width();
        uint32_t* sin = a.state_in + (a.state_base + s) * 16;
        for (uint32_t i = 0; i < st[0]; i++) c[i] = a.observed[st[1] + i];
        for (int i = 0; i < 16; i++) row[i] = sin[i] = c[i];
        a.state_mult[a.state_base + s] = bb::ONE;
        chip_permute<16, 13, M4, false>(c, nullptr, tab, L);
        for (int i = 0; i < 16; i++) row[16 + i] = c[i];
        for (int i = 0; i < 8; i++)
            if (st[2 + i]) a.samples[st[2 + i] - 1] = c[i];
    }
}
// One lane per transcript row: everything but IN and OUT (the chain writes those)
RK_HD void fri_transcript_fill_lane(const FriTranscriptArgs& a, uint32_t s) {
    uint32_t* row = a.transcript + (size_t)s * a.width();
    const uint32_t* st = a.steps + FRI_TRANSCRIPT_STEP_WORDS * s;
    for (uint32_t j = 0; j < a.N; j++) row[32 + j] = j == s ? bb::ONE : 0u;
    row[32 + a.N] = bb::ONE;
    for (uint32_t j = 0; j < 8; j++) {
        row[33 + a.N + j] = st[2 + j] ? bb::ONE : 0u;
        row[41 + a.N + j] = st[2 + j] ? bb::encode(st[2 + j] - 1) : 0u;
    }
}
// One lane per bits row (slot): the canonical form of the sampled cell and what the checks read of it
RK_HD void fri_bits_fill_lane(const FriTranscriptArgs& a, uint32_t slot) {
    uint32_t* row = a.bits + (size_t)slot * FRI_BITS_WIDTH;
    const uint32_t vm = a.samples[slot], v = bb::decode(vm);
    const uint32_t nb = slot ? a.L : a.pow_bits;
    row[0] = bb::encode(slot), row[1] = vm;
    for (uint32_t i = 0; i < 31; i++) row[2 + i] = (v >> i) & 1u ? bb::ONE : 0u;
    row[33] = ((v >> 28) & 7u) == 7u ? bb::ONE : 0u;
    row[34] = bb::ONE;
    row[35] = slot ? bb::encode(slot - 1) : 0u;
    row[36] = bb::encode(v & (uint32_t)(((uint64_t)1 << nb) - 1));
    row[37] = slot ? 0u : bb::ONE, row[38] = slot ? bb::ONE : 0u;
}

}  // namespace p3k
