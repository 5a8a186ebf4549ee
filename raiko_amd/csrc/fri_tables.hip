// The rows of the FRI lookup tables on the GPU (include/raiko_hip.h: rk_fri_chip_*, rk_fri_reduce_*, rk_fri_open_*,
// rk_fri_transcript_*): four statements about the FRI queries of a shard proof, each containing the one before -- the
// commit phase (fold, path, claims, chip), the reduced openings (fold', path, reduce, chip), the input-batch openings
// (fold', path, reduce'', ipath, chip, state), the transcript (fold'', path, reduce'', ipath, transcript, bits, chip,
// state).  Here: the kernels (lane bodies: p3_kernels.hpp), the size plans, and the row writing as stages the four entry
// points share -- commit, reduce, open, transcript, and the Poseidon2 chip (p3_air.hip) fed by their lanes.  AIRs and
// numpy witnesses: raiko_amd/fri_chip.py, fri_reduce.py, fri_open.py, fri_transcript.py.
#include "cell_perm.hpp"
#include "p3_air.hpp"

#include <algorithm>
#include <vector>

namespace {

using rk::DevBuf;
using p3k::P2ChipLayout;

uint32_t log_height(uint64_t rows) { return std::max(1u, log2u((size_t)rows)); }

// ---------------------------------------------------------------- kernels and size plans
// the FRI commit-phase tables (rk_fri_chip_rows_device): lane bodies in p3_kernels.hpp.  Every lane stores its own rows
// cell by cell; staging a step's 64 rows in LDS and storing them in whole lines was measured and dropped (path kernel,
// 2 000 lanes / 21 000 rows: 0.59 ms against 0.40 -- the lane is bound by its chain of permutations, and the staged
// form adds two barriers and a 64-row copy loop per step)
__global__ void __launch_bounds__(64) fri_fold_kernel(p3k::FriArgs a) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < a.Q) p3k::fri_fold_lane(a, q);
}
template <int M4>
__global__ void __launch_bounds__(64) fri_path_kernel(p3k::FriArgs a, const uint32_t* __restrict__ tab, P2ChipLayout L) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < a.Q * a.R) p3k::fri_path_lane<M4>(a, t, tab, L);
}
int fri_sizes(uint32_t log_max, uint32_t blow, uint32_t queries, rk_fri_chip_size_info* o) {
    if (!o || blow < 1 || blow > 4 || log_max <= blow || log_max > ntt::LAMBDA || queries == 0 || queries > RK_MAX_QUERIES) return RK_ERR_INVALID;
    p3k::FriArgs a{};
    a.L = log_max, a.R = log_max - blow, a.Q = queries;
    *o = rk_fri_chip_size_info{};
    o->n_rounds = a.R;
    o->fold_width = a.fold_width(), o->path_width = a.path_width(), o->claims_width = p3k::FRI_CLAIMS_WIDTH, o->chip_width = 314;
    o->fold_rows = (uint64_t)a.Q * a.R;
    o->path_rows = (uint64_t)a.Q * a.steps_before(a.R);
    o->chip_rows = o->fold_rows + o->path_rows;
    o->fold_log_height = o->claims_log_height = log_height(o->fold_rows);
    o->path_log_height = log_height(o->path_rows);
    o->chip_log_height = log_height(o->chip_rows);
    o->publics_words = 12 * (uint64_t)a.R + 4;
    o->records_words = (uint64_t)a.Q * a.per_record();
    return RK_OK;
}

// the reduced-openings table (rk_fri_reduce_rows_device): lane bodies in p3_kernels.hpp.  A workgroup takes one (query,
// round) and walks the round's matrices; within a matrix its 256 lanes take 256 consecutive columns at a time.  A lane's
// power A alpha^col comes from the alpha^(2^i) of fri_reduce_pows_kernel, its running sum from a shuffle scan across the
// wave, the carry across waves and across 256-column pieces through LDS.  Every lane stores its own row cell by cell, as
// the other two kernels.
__global__ void fri_reduce_pows_kernel(uint32_t* __restrict__ apow, const uint32_t* __restrict__ pub, uint32_t wm) {
    if (blockIdx.x || threadIdx.x) return;
    bb::Ext p = p3k::fri_load_ext(pub);
    for (int i = 0; i < 32; i++) {
        for (int k = 0; k < 4; k++) apow[4 * i + k] = p.c[k];
        p = bb::mul(p, p, wm);
    }
}
__global__ void __launch_bounds__(p3k::FRI_REDUCE_TPB) fri_reduce_kernel(p3k::FriReduceArgs a) {
    constexpr uint32_t WAVES = p3k::FRI_REDUCE_TPB / 64;
    __shared__ bb::Ext wtot[2][WAVES];
    __shared__ bb::Ext s_rop;
    const uint32_t q = blockIdx.x / a.R, rd = blockIdx.x % a.R, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const p3k::FriReduceCtx cx = p3k::fri_reduce_begin(a, q, rd);
    bb::Ext rop = bb::ext_zero();
    for (uint32_t m = 0; m < a.M; m++) {
        const uint32_t* slot = a.slots + p3k::FRI_REDUCE_SLOT_WORDS * m;
        if (slot[0] != rd) continue;                      // the same for every lane of the workgroup
        const uint32_t width = slot[1];
        bb::Ext carry[2] = {bb::ext_zero(), bb::ext_zero()};
        for (uint32_t base = 0; base < width; base += p3k::FRI_REDUCE_TPB) {
            const uint32_t col = base + tid;
            p3k::FriReduceLane ln;
            if (col < width) {
                p3k::fri_reduce_term(a, q, m, col, ln);
            } else {
                ln.p = 0;
                ln.pw[0] = ln.pw[1] = ln.sum[0] = ln.sum[1] = bb::ext_zero();
            }
            for (uint32_t d = 1; d < 64; d <<= 1) {
                bb::Ext s0, s1;
                for (int k = 0; k < 4; k++) s0.c[k] = __shfl_up(ln.sum[0].c[k], d), s1.c[k] = __shfl_up(ln.sum[1].c[k], d);
                if (lane >= d) p3k::fri_reduce_join(ln, s0, s1);
            }
            if (lane == 63) wtot[0][wave] = ln.sum[0], wtot[1][wave] = ln.sum[1];
            __syncthreads();
            bb::Ext before[2] = {carry[0], carry[1]};
            for (uint32_t w = 0; w < WAVES; w++)
                for (int j = 0; j < 2; j++) {
                    if (w < wave) before[j] = bb::add(before[j], wtot[j][w]);
                    carry[j] = bb::add(carry[j], wtot[j][w]);
                }
            p3k::fri_reduce_join(ln, before[0], before[1]);
            if (col < width) {
                const bb::Ext after = p3k::fri_reduce_row(a, q, m, col, cx, ln, rop);
                if (col + 1 == width) s_rop = after;
            }
            __syncthreads();
        }
        rop = s_rop;
    }
}

struct FriReducePlan {
    rk_fri_reduce_size_info sz;
    std::vector<uint32_t> slots;      // FRI_REDUCE_SLOT_WORDS per slot, gen(log_n) left 0 (the context's root fills it)
    std::vector<uint32_t> log_n;
    std::vector<uint32_t> batch;      // per slot; FRI_OPEN_NONE = the single row of a round without a matrix
};
// the schedule of the reduce table from the layout of rk_p3_fri_inputs (Montgomery words; 5 per matrix): the matrices by
// round, in the layout's order within a round, and one single-row slot for every round without a matrix.  Batches: 0
// trace, 1 permutation, 2 quotient, 3 preprocessed (keyed proofs), in the verifier's order 0, 3, 1, 2
int fri_reduce_plan(uint32_t log_max, uint32_t blow, uint32_t queries, const uint32_t* layout, uint32_t n_matrices, FriReducePlan* plan) {
    rk_fri_chip_size_info chip;
    RK_TRY(fri_sizes(log_max, blow, queries, &chip));
    if (!layout || n_matrices == 0 || n_matrices > 4096) return RK_ERR_INVALID;
    const uint32_t R = chip.n_rounds;
    struct M { uint32_t batch, rd, width, points, log_n, off; };
    std::vector<M> ms(n_matrices);
    uint64_t off = 0;
    for (uint32_t i = 0; i < n_matrices; i++) {
        for (int k = 0; k < 5; k++)
            if (layout[5 * i + k] >= bb::P) return RK_ERR_INVALID;
        M& m = ms[i];
        m.batch = bb::decode(layout[5 * i]), m.rd = bb::decode(layout[5 * i + 1]), m.width = bb::decode(layout[5 * i + 2]);
        m.points = bb::decode(layout[5 * i + 3]), m.log_n = bb::decode(layout[5 * i + 4]);
        static const uint32_t place[4] = {0, 2, 3, 1};   // of a batch in the verifier's order
        if (m.batch > 3 || (i ? place[m.batch] < place[ms[i - 1].batch] : m.batch != 0)) return RK_ERR_INVALID;
        if (m.rd >= R || m.width == 0 || m.width > (1u << 16)) return RK_ERR_INVALID;   // rd < R: no matrix is taller than log_max
        if (m.points != (m.batch == 2 ? 1u : 2u) || m.log_n + blow + m.rd != log_max) return RK_ERR_INVALID;
        m.off = (uint32_t)off;
        off += m.width;
    }
    plan->slots.clear(), plan->log_n.clear(), plan->batch.clear();
    uint64_t rows = 0;
    for (uint32_t rd = 0; rd < R; rd++) {
        const size_t first = plan->slots.size();
        for (const M& m : ms)
            if (m.rd == rd) {
                plan->slots.insert(plan->slots.end(), {rd, m.width, m.points, m.off, 0u, 0u, (uint32_t)rows, 0u});
                plan->log_n.push_back(m.log_n);
                plan->batch.push_back(m.batch);
                rows += m.width;
            }
        if (plan->slots.size() == first) {
            plan->slots.insert(plan->slots.end(), {rd, 1u, 0u, 0u, 0u, 0u, (uint32_t)rows, 0u});
            plan->log_n.push_back(0);
            plan->batch.push_back(p3k::FRI_OPEN_NONE);
            rows += 1;
        }
        plan->slots[plan->slots.size() - p3k::FRI_REDUCE_SLOT_WORDS + 5] = 1;
    }
    rk_fri_reduce_size_info& o = plan->sz;
    o = rk_fri_reduce_size_info{};
    o.n_rounds = R, o.n_slots = (uint32_t)(plan->slots.size() / p3k::FRI_REDUCE_SLOT_WORDS);
    o.fold_width = chip.fold_width + 1, o.path_width = chip.path_width, o.reduce_width = p3k::FRI_REDUCE_FIXED + o.n_slots, o.chip_width = chip.chip_width;
    o.fold_rows = chip.fold_rows, o.path_rows = chip.path_rows, o.chip_rows = chip.chip_rows, o.reduce_rows = rows * queries;
    if (o.reduce_rows > ((uint64_t)1 << 26)) return RK_ERR_INVALID;
    o.fold_log_height = chip.fold_log_height, o.path_log_height = chip.path_log_height, o.chip_log_height = chip.chip_log_height;
    o.reduce_log_height = log_height(o.reduce_rows);
    o.fold_publics_words = chip.publics_words, o.fold_records_words = chip.records_words;
    o.reduce_publics_words = 8 + 16 * (uint64_t)o.n_slots, o.inputs_words = (uint64_t)queries * (1 + off);
    o.rows_per_query = rows;
    return RK_OK;
}

// the input-batch openings (rk_fri_open_rows_device): lane bodies in p3_kernels.hpp.  The sponge and ipath lanes are bound
// by their chains of permutations, as the path kernel's; the fill kernel is one store-only lane per reduce row.
template <int M4>
__global__ void __launch_bounds__(64) fri_open_sponge_kernel(p3k::FriOpenArgs a, const uint32_t* __restrict__ tab, P2ChipLayout L) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < a.Q * a.G) p3k::fri_open_sponge_lane<M4>(a, t, tab, L);
}
__global__ void __launch_bounds__(256) fri_open_fill_kernel(p3k::FriOpenArgs a) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < (size_t)a.Q * a.rows_per_query) p3k::fri_open_fill_lane(a, r);
}
template <int M4>
__global__ void __launch_bounds__(64) fri_open_ipath_kernel(p3k::FriOpenArgs a, const uint32_t* __restrict__ tab, P2ChipLayout L) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < a.Q * a.NB) p3k::fri_open_ipath_lane<M4>(a, t, tab, L);
}

struct FriOpenPlan {
    FriReducePlan red;
    rk_fri_open_size_info sz;
    std::vector<uint32_t> groups, rowinfo, levels;
    uint64_t chip_base = 0;
};
// groups, row classes and tree levels from the reduce schedule: a group is a maximal run of slots of one (round, batch)
int fri_open_plan(uint32_t log_max, uint32_t blow, uint32_t queries, const uint32_t* layout, uint32_t n_matrices, FriOpenPlan* plan) {
    RK_TRY(fri_reduce_plan(log_max, blow, queries, layout, n_matrices, &plan->red));
    const rk_fri_reduce_size_info& r = plan->red.sz;
    const std::vector<uint32_t>& slots = plan->red.slots;
    const uint32_t M = r.n_slots, W = p3k::FRI_REDUCE_SLOT_WORDS;
    plan->groups.clear(), plan->levels.clear();
    plan->rowinfo.assign(2 * (size_t)r.rows_per_query, 0);
    uint64_t perms = 0;
    uint32_t height[4] = {0, 0, 0, 0};               // log LDE height of a batch's tallest matrix; 0 = batch absent
    for (uint32_t m = 0; m < M;) {
        const uint32_t b = plan->red.batch[m], rd = slots[W * m];
        if (b == p3k::FRI_OPEN_NONE) {
            m++;
            continue;
        }
        uint32_t end = m, cells = 0;
        while (end < M && plan->red.batch[end] == b && slots[W * end] == rd) cells += slots[W * end + 1], end++;
        plan->groups.insert(plan->groups.end(), {m, end - m, cells, slots[W * m + 6], (uint32_t)perms, b, rd, 0u});
        for (uint32_t i = 0; i < cells; i++) {
            plan->rowinfo[2 * ((size_t)slots[W * m + 6] + i)] = i;
            plan->rowinfo[2 * ((size_t)slots[W * m + 6] + i) + 1] = 1u | (i + 1 == cells ? 2u : 0u) | (b << 2);
        }
        perms += (cells + 7) / 8;
        height[b] = std::max(height[b], log_max - rd);
        m = end;
    }
    if (height[0] != log_max || height[2] != log_max) return RK_ERR_INVALID;   // every table is in the trace and the quotient batch
    const uint32_t G = (uint32_t)(plan->groups.size() / p3k::FRI_OPEN_GROUP_WORDS);
    uint64_t rows = 0, chips = 0, path_off = 0;
    uint32_t nb = 0;
    for (uint32_t b = 0; b < 4; b++) {   // in batch-number order: the preprocessed tree comes last, nothing of a three-batch plan moves
        const uint32_t B = height[b];
        if (B) {
            std::vector<uint32_t> lv(p3k::FRI_OPEN_LEVEL_WORDS, p3k::FRI_OPEN_NONE);
            uint32_t inj = 0, top = p3k::FRI_OPEN_NONE;
            for (uint32_t g = 0; g < G; g++) {
                const uint32_t* gr = &plan->groups[p3k::FRI_OPEN_GROUP_WORDS * g];
                if (gr[5] != b) continue;
                const uint32_t lh = log_max - gr[6];
                if (lh == B) top = g;
                else lv[8 + (B - 1 - lh)] = g, inj++;   // joins behind the step whose parent is a node of the height-2^lh level
            }
            lv[0] = b, lv[1] = B, lv[2] = (uint32_t)rows, lv[3] = (uint32_t)chips, lv[4] = inj, lv[5] = (uint32_t)path_off, lv[6] = top, lv[7] = log_max - B;
            plan->levels.insert(plan->levels.end(), lv.begin(), lv.end());
            rows += (uint64_t)queries * B, chips += (uint64_t)queries * (B + inj);
            nb++;
        }
        path_off += 8 * (uint64_t)B;
    }
    rk_fri_open_size_info& o = plan->sz;
    o = rk_fri_open_size_info{};
    o.n_rounds = r.n_rounds, o.n_slots = M, o.n_groups = G, o.n_batches = nb;
    o.fold_width = r.fold_width, o.path_width = r.path_width, o.reduce_width = r.reduce_width + p3k::FRI_OPEN_SPONGE_COLS;
    o.ipath_width = p3k::FRI_OPEN_IPATH_FIXED + nb, o.chip_width = r.chip_width, o.state_width = r.chip_width;
    o.fold_rows = r.fold_rows, o.path_rows = r.path_rows, o.reduce_rows = r.reduce_rows, o.ipath_rows = rows;
    o.chip_rows = r.chip_rows + chips, o.state_rows = perms * queries, o.rows_per_query = r.rows_per_query;
    if (o.chip_rows > ((uint64_t)1 << 24) || o.state_rows > ((uint64_t)1 << 24)) return RK_ERR_INVALID;
    o.fold_log_height = r.fold_log_height, o.path_log_height = r.path_log_height, o.reduce_log_height = r.reduce_log_height;
    o.ipath_log_height = log_height(rows), o.chip_log_height = log_height(o.chip_rows), o.state_log_height = log_height(o.state_rows);
    o.fold_publics_words = r.fold_publics_words, o.fold_records_words = r.fold_records_words;
    o.reduce_publics_words = r.reduce_publics_words, o.inputs_words = r.inputs_words;
    o.roots_words = height[3] ? 34 : 25, o.paths_words = (uint64_t)queries * path_off;
    o.log_pmax = height[1], o.log_kmax = height[3];
    plan->chip_base = r.chip_rows;
    return RK_OK;
}

// the transcript (rk_fri_transcript_rows_device).  The challenger is ONE chain of dependent permutations, so a lane per
// chain would leave 63 lanes idle for the latency of every permutation; the chain kernel is one wave with one lane per
// state cell instead (CellPerm, cell_perm.hpp): the first half-wave's 16 cells hold the state, the second half-wave
// follows with its results dropped (hash_fold_cells_kernel's idle half-waves), every lane executes every permutation.
// Lane-per-chain form of the same steps: p3k::fri_transcript_chain_lane.
template <class C>
__global__ void __launch_bounds__(64) fri_transcript_chain_kernel(p3k::FriTranscriptArgs a, const typename C::Consts* __restrict__ kc) {
    const typename C::Consts& k = *kc;
    const unsigned lane = threadIdx.x, cell = lane & 31u;
    const bool writes = lane < 16;
    CellPerm<C> cp;
    cp.init(k, cell);
    uint32_t x = 0;
    for (uint32_t s = 0; s < a.N; s++) {
        const uint32_t* st = a.steps + p3k::FRI_TRANSCRIPT_STEP_WORDS * s;
        uint32_t* row = a.transcript + (size_t)s * a.width();
        if (cell < st[0]) x = a.observed[st[1] + cell];
        if (writes) row[cell] = a.state_in[(a.state_base + s) * 16 + cell] = x;
        if (lane == 0) a.state_mult[a.state_base + s] = bb::ONE;
        x = cp.permute(x, k);
        if (writes) row[16 + cell] = x;
        if (lane < 8 && st[2 + lane]) a.samples[st[2 + lane] - 1] = x;
    }
}
__global__ void __launch_bounds__(64) fri_transcript_fill_kernel(p3k::FriTranscriptArgs a) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < a.N) p3k::fri_transcript_fill_lane(a, t);
    else if (t - a.N <= a.Q) p3k::fri_bits_fill_lane(a, t - a.N);
}

struct FriTranscriptPlan {
    FriOpenPlan open;
    rk_fri_transcript_size_info sz;
    std::vector<uint32_t> steps;      // FRI_TRANSCRIPT_STEP_WORDS per duplex permutation
};
// the duplex permutations from the challenger's calls (Montgomery pairs, rk_p3_fri_transcript): p3_host.hpp's Challenger replayed
// without hashing -- which step absorbs which observed words, which output cell every sample pops
int fri_transcript_plan(uint32_t log_max, uint32_t blow, uint32_t queries, const uint32_t* layout, uint32_t n_matrices, const uint32_t* ops,
                        uint32_t n_ops, FriTranscriptPlan* plan) {
    RK_TRY(fri_open_plan(log_max, blow, queries, layout, n_matrices, &plan->open));
    if (!ops || n_ops == 0 || n_ops > (1u << 16)) return RK_ERR_INVALID;
    std::vector<uint32_t>& steps = plan->steps;
    steps.clear();
    uint32_t n_in = 0, n_out = 0, n_bits = 0, pow_bits = 0;
    uint64_t n_obs = 0, n_pub = 0;
    auto duplex = [&] {
        steps.insert(steps.end(), {n_in, (uint32_t)(n_obs - n_in), 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u});
        n_in = 0, n_out = 8;
    };
    for (uint32_t i = 0; i < n_ops; i++) {
        if (ops[2 * i] >= bb::P || ops[2 * i + 1] >= bb::P) return RK_ERR_INVALID;
        const uint32_t kind = bb::decode(ops[2 * i]), count = bb::decode(ops[2 * i + 1]);
        if (kind > 2 || (kind < 2 && (count == 0 || count > (1u << 20) || n_bits))) return RK_ERR_INVALID;   // the sample_bits come last
        if (kind == 0) {
            for (uint32_t j = 0; j < count; j++) {
                n_out = 0, n_in++, n_obs++;
                if (n_in == 8) duplex();
            }
            continue;
        }
        for (uint32_t j = 0; j < (kind == 1 ? count : 1u); j++) {
            if (n_in != 0 || n_out == 0) duplex();
            --n_out;
            if (kind == 1) {
                n_pub++;
            } else {
                if (n_bits ? count != log_max : count > 27) return RK_ERR_INVALID;
                if (!n_bits) pow_bits = count;
                steps[steps.size() - p3k::FRI_TRANSCRIPT_STEP_WORDS + 2 + n_out] = ++n_bits;   // slot + 1
            }
        }
        if (steps.size() > (size_t)p3k::FRI_TRANSCRIPT_STEP_WORDS * p3k::FRI_TRANSCRIPT_MAX_STEPS) return RK_ERR_INVALID;
    }
    if (n_bits != queries + 1 || steps.size() > (size_t)p3k::FRI_TRANSCRIPT_STEP_WORDS * p3k::FRI_TRANSCRIPT_MAX_STEPS) return RK_ERR_INVALID;
    const rk_fri_open_size_info& p = plan->open.sz;
    const uint32_t N = (uint32_t)(steps.size() / p3k::FRI_TRANSCRIPT_STEP_WORDS);
    rk_fri_transcript_size_info& o = plan->sz;
    o = rk_fri_transcript_size_info{};
    o.n_rounds = p.n_rounds, o.n_slots = p.n_slots, o.n_groups = p.n_groups, o.n_batches = p.n_batches, o.log_pmax = p.log_pmax, o.log_kmax = p.log_kmax;
    o.n_steps = N, o.pow_bits = pow_bits;
    o.fold_width = p.fold_width + 1, o.path_width = p.path_width, o.reduce_width = p.reduce_width, o.ipath_width = p.ipath_width;
    o.transcript_width = p3k::FRI_TRANSCRIPT_FIXED + N, o.bits_width = p3k::FRI_BITS_WIDTH, o.chip_width = p.chip_width, o.state_width = p.state_width;
    o.fold_rows = p.fold_rows, o.path_rows = p.path_rows, o.reduce_rows = p.reduce_rows, o.ipath_rows = p.ipath_rows;
    o.transcript_rows = N, o.bits_rows = (uint64_t)queries + 1, o.chip_rows = p.chip_rows, o.state_rows = p.state_rows + N;
    o.rows_per_query = p.rows_per_query;
    if (o.state_rows > ((uint64_t)1 << 24)) return RK_ERR_INVALID;
    o.fold_log_height = p.fold_log_height, o.path_log_height = p.path_log_height, o.reduce_log_height = p.reduce_log_height;
    o.ipath_log_height = p.ipath_log_height, o.chip_log_height = p.chip_log_height;
    o.transcript_log_height = log_height(N), o.bits_log_height = log_height(o.bits_rows), o.state_log_height = log_height(o.state_rows);
    o.fold_publics_words = p.fold_publics_words, o.fold_records_words = p.fold_records_words, o.reduce_publics_words = p.reduce_publics_words;
    o.inputs_words = p.inputs_words, o.roots_words = p.roots_words, o.paths_words = p.paths_words;
    o.observed_words = n_obs, o.transcript_publics_words = n_obs + n_pub;
    return RK_OK;
}

// ---------------------------------------------------------------- the row writing, as stages
template <class... P, class... A>
int launch(rk_ctx* ctx, const char* name, void (*kernel)(P...), dim3 grid, dim3 block, A... args) {
    hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, args...);
    return rk::post_launch(ctx, name);
}
// a kernel that has one instantiation per external matrix of the Poseidon2 instance (p2::Any::m4)
template <class... P, class... A>
int launch_m4(rk_ctx* ctx, const char* name, void (*k0)(P...), void (*k1)(P...), dim3 grid, dim3 block, A... args) {
    return launch(ctx, name, ctx->h_p2.m4() ? k1 : k0, grid, block, args...);
}

// what all three statements need of the context: the width-16 Poseidon2, the context's own blow-up, a fold by two; the
// sponge of the input batches (pad_free) where the statement opens them
int fri_scope(const rk_ctx* ctx, uint32_t blowup_log2, bool sponge) {
    const p2::Any& k = ctx->h_p2;
    if (k.cells() != 16 || (sponge && !k.pad_free) || ctx->sys.blowup_log2 != blowup_log2 || ctx->sys.fri_fold_log2 != 1) return RK_ERR_INVALID;
    return RK_OK;
}

struct OutTable {   // an output table as the caller passed it, and the size the plan gives it
    uint32_t* p;
    size_t capacity;
    uint32_t width, log_height;
    size_t words() const { return (size_t)width << log_height; }
};
int check_outputs(const OutTable* t, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (t[i].capacity < t[i].words()) return RK_ERR_CAPACITY;
    return RK_OK;
}
// rows and inputs the lanes do not write are padding: all zero (multiplicity 0, no selector set)
int clear_outputs(rk_ctx* ctx, const OutTable* t, size_t n) {
    for (size_t i = 0; i < n; i++) RK_HIP_TRY(ctx, hipMemsetAsync(t[i].p, 0, t[i].words() * 4, ctx->stream));
    return RK_OK;
}

struct ChipFeed {   // the inputs of a Poseidon2 chip table, written by the lanes that send to it: 16 words and a multiplicity per row
    uint32_t *in = nullptr, *mult = nullptr;
    size_t n = 0;
};

// One call of an entry point, past its checks.  The scratch blocks are released with it: after the last launch that
// reads them has been enqueued on ctx->stream, which also orders whoever gets a block next behind that launch.
struct FriCall {
    rk_ctx* ctx;
    uint32_t log_max, n_rounds, queries;
    std::vector<DevBuf> scratch;
    P2ChipLayout L{};
    uint32_t gen_l = 0;
    uint32_t *d_tab = nullptr, *d_slots = nullptr;   // the chip's constants (begin); the reduce schedule (reduce)

    // a scratch block of `words` words, filled from `h` where given
    int dev(size_t words, uint32_t** out, const uint32_t* h = nullptr) {
        scratch.emplace_back();
        RK_TRY(scratch.back().alloc(ctx, words * 4));
        *out = scratch.back().u32();
        return h ? rk::upload(ctx, *out, h, words * 4) : RK_OK;
    }
    int begin() {
        RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
        L = rk::p2_chip_layout(ctx->h_p2);
        gen_l = bb::pow(ctx->sys.root27m, (uint64_t)1 << (27 - log_max));
        const std::vector<uint32_t> tab = rk::p2_chip_tab(ctx->h_p2);
        return dev(tab.size(), &d_tab, tab.data());
    }
    // the feed of a chip table of 2^log_height rows, all padding so far
    int chip_feed(uint32_t log_height, ChipFeed* f) {
        f->n = (size_t)1 << log_height;
        RK_TRY(dev(f->n * 16, &f->in));
        RK_TRY(dev(f->n, &f->mult));
        RK_HIP_TRY(ctx, hipMemsetAsync(f->in, 0, f->n * 16 * 4, ctx->stream));
        RK_HIP_TRY(ctx, hipMemsetAsync(f->mult, 0, f->n * 4, ctx->stream));
        return RK_OK;
    }
    int chip_trace(const ChipFeed& f, uint32_t* d_out) { return rk::p2_chip_trace(ctx, d_tab, L, f.in, f.mult, f.n, d_out); }

    // the commit phase: the fold chain of every query, then the Merkle path of every (query, round).  xcol: the fold
    // rows end in the point X (fold'), firstcol: and behind it in FIRST (fold''); d_claims: the claims table, or null where
    // a reduce table takes its place
    int commit(const uint32_t* d_publics, const uint32_t* d_records, uint32_t* d_fold, uint32_t* d_path, uint32_t* d_claims, bool xcol, const ChipFeed& chip,
               bool firstcol = false) {
        p3k::FriArgs a{};
        a.L = log_max, a.R = n_rounds, a.Q = queries, a.gen_l = gen_l, a.wm = ctx->sys.wm;
        a.pub = d_publics, a.rec = d_records;
        a.fold = d_fold, a.path = d_path, a.claims = d_claims, a.chip_in = chip.in, a.chip_mult = chip.mult;
        if (xcol) a.xcol = 1, a.shiftm = ctx->sys.shiftm;
        if (firstcol) a.firstcol = 1;
        RK_TRY(launch(ctx, "fri_fold_kernel", fri_fold_kernel, dim3((queries + 63) / 64), dim3(64), a));
        const dim3 grid((unsigned)(((uint64_t)queries * n_rounds + 63) / 64));
        return launch_m4(ctx, "fri_path_kernel", fri_path_kernel<0>, fri_path_kernel<1>, grid, dim3(64), a, d_tab, L);
    }
    // the reduced openings: the schedule with every matrix's generator under the context's root, the powers of alpha,
    // then one workgroup per (query, round).  stride: words per row of d_reduce, 0 = the reduce table's own width
    int reduce(FriReducePlan& plan, const uint32_t* d_reduce_publics, const uint32_t* d_inputs, uint32_t* d_reduce, uint32_t stride) {
        const rk_fri_reduce_size_info& sz = plan.sz;
        for (uint32_t m = 0; m < sz.n_slots; m++)
            plan.slots[p3k::FRI_REDUCE_SLOT_WORDS * m + 4] = bb::pow(ctx->sys.root27m, (uint64_t)1 << (27 - plan.log_n[m]));
        uint32_t* apow;
        RK_TRY(dev(plan.slots.size(), &d_slots, plan.slots.data()));
        RK_TRY(dev(32 * 4, &apow));
        p3k::FriReduceArgs r{};
        r.L = log_max, r.R = n_rounds, r.Q = queries, r.M = sz.n_slots;
        r.rows_per_query = (uint32_t)sz.rows_per_query, r.wm = ctx->sys.wm, r.shiftm = ctx->sys.shiftm, r.gen_l = gen_l;
        r.per_record = (size_t)(sz.inputs_words / queries);
        r.slots = d_slots, r.pub = d_reduce_publics, r.rec = d_inputs, r.apow = apow, r.out = d_reduce, r.stride = stride;
        RK_TRY(launch(ctx, "fri_reduce_pows_kernel", fri_reduce_pows_kernel, dim3(1), dim3(64), apow, d_reduce_publics, r.wm));
        return launch(ctx, "fri_reduce_kernel", fri_reduce_kernel, dim3(queries * n_rounds), dim3(p3k::FRI_REDUCE_TPB), r);
    }
    // the input-batch openings over the rows `reduce` left in d_reduce: the sponge of every (query, group), the sponge
    // columns of every reduce'' row, the path of every (query, batch)
    int open(const FriOpenPlan& plan, const uint32_t* d_inputs, const uint32_t* d_paths, uint32_t* d_reduce, uint32_t* d_ipath, const ChipFeed& chip, const ChipFeed& state) {
        const rk_fri_open_size_info& sz = plan.sz;
        uint32_t *groups, *rowinfo, *levels, *dig;
        RK_TRY(dev(plan.groups.size(), &groups, plan.groups.data()));
        RK_TRY(dev(plan.rowinfo.size(), &rowinfo, plan.rowinfo.data()));
        RK_TRY(dev(plan.levels.size(), &levels, plan.levels.data()));
        RK_TRY(dev((size_t)queries * sz.n_groups * 8, &dig));
        p3k::FriOpenArgs o{};
        o.L = log_max, o.Q = queries, o.M = sz.n_slots, o.G = sz.n_groups, o.NB = sz.n_batches;
        o.rows_per_query = (uint32_t)sz.rows_per_query, o.stride = sz.reduce_width, o.sponge_at = sz.reduce_width - p3k::FRI_OPEN_SPONGE_COLS;
        o.per_record = (size_t)(sz.inputs_words / queries), o.per_path = (size_t)(sz.paths_words / queries), o.chip_base = (size_t)plan.chip_base;
        o.slots = d_slots, o.groups = groups, o.rowinfo = rowinfo, o.levels = levels, o.rec = d_inputs, o.paths = d_paths;
        o.reduce = d_reduce, o.ipath = d_ipath, o.state_in = state.in, o.state_mult = state.mult, o.chip_in = chip.in, o.chip_mult = chip.mult, o.digests = dig;
        const dim3 block(64), sgrid((unsigned)(((size_t)queries * sz.n_groups + 63) / 64)), igrid((unsigned)(((size_t)queries * sz.n_batches + 63) / 64));
        RK_TRY(launch_m4(ctx, "fri_open_sponge_kernel", fri_open_sponge_kernel<0>, fri_open_sponge_kernel<1>, sgrid, block, o, d_tab, L));
        RK_TRY(launch(ctx, "fri_open_fill_kernel", fri_open_fill_kernel, dim3((unsigned)((sz.reduce_rows + 255) / 256)), dim3(256), o));
        return launch_m4(ctx, "fri_open_ipath_kernel", fri_open_ipath_kernel<0>, fri_open_ipath_kernel<1>, igrid, block, o, d_tab, L);
    }
    // the transcript: the chain of the challenger's permutations (one wave), whose inputs join the state chip's behind the
    // sponge's, then the cells of the transcript and bits rows that follow from the plan and the sampled cells
    int transcript(const FriTranscriptPlan& plan, const uint32_t* d_observed, uint32_t* d_transcript, uint32_t* d_bits, const ChipFeed& state) {
        const rk_fri_transcript_size_info& sz = plan.sz;
        uint32_t *steps, *samples;
        RK_TRY(dev(plan.steps.size(), &steps, plan.steps.data()));
        RK_TRY(dev((size_t)queries + 1, &samples));
        p3k::FriTranscriptArgs t{};
        t.N = sz.n_steps, t.Q = queries, t.L = log_max, t.pow_bits = sz.pow_bits, t.state_base = (size_t)plan.open.sz.state_rows;
        t.steps = steps, t.observed = d_observed, t.transcript = d_transcript, t.bits = d_bits;
        t.state_in = state.in, t.state_mult = state.mult, t.samples = samples;
        if (ctx->h_p2.m4()) {
            RK_TRY(launch(ctx, "fri_transcript_chain_kernel", fri_transcript_chain_kernel<p2::K3>, dim3(1), dim3(64), t, (const p2::K3::Consts*)ctx->d_p2));
        } else {
            RK_TRY(launch(ctx, "fri_transcript_chain_kernel", fri_transcript_chain_kernel<p2::K2>, dim3(1), dim3(64), t, (const p2::K2::Consts*)ctx->d_p2));
        }
        return launch(ctx, "fri_transcript_fill_kernel", fri_transcript_fill_kernel, dim3((sz.n_steps + queries + 1 + 63) / 64), dim3(64), t);
    }
};

}  // namespace

// Every entry point: null checks, plan, scope, outputs -- nothing is written or enqueued before all of them pass --, then
// the stages in order.  The tables the lanes write come first in `outs` and are cleared; a chip table is written whole.
extern "C" {

int rk_fri_chip_sizes(uint32_t log_max, uint32_t blowup_log2, uint32_t queries, rk_fri_chip_size_info* out) {
    return fri_sizes(log_max, blowup_log2, queries, out);
}
int rk_fri_chip_rows_device(rk_ctx* ctx, uint32_t log_max, uint32_t blowup_log2, uint32_t queries, const uint32_t* d_publics,
                            const uint32_t* d_records, uint32_t* d_fold, size_t fold_capacity, uint32_t* d_path, size_t path_capacity,
                            uint32_t* d_claims, size_t claims_capacity, uint32_t* d_chip, size_t chip_capacity) {
    RK_GUARD_BEGIN
    if (!ctx || !d_publics || !d_records || !d_fold || !d_path || !d_claims || !d_chip) return RK_ERR_INVALID;
    rk_fri_chip_size_info sz;
    RK_TRY(fri_sizes(log_max, blowup_log2, queries, &sz));
    RK_TRY(fri_scope(ctx, blowup_log2, /*sponge=*/false));
    const OutTable outs[] = {{d_fold, fold_capacity, sz.fold_width, sz.fold_log_height},
                             {d_path, path_capacity, sz.path_width, sz.path_log_height},
                             {d_claims, claims_capacity, sz.claims_width, sz.claims_log_height},
                             {d_chip, chip_capacity, sz.chip_width, sz.chip_log_height}};
    RK_TRY(check_outputs(outs, 4));
    FriCall c{ctx, log_max, sz.n_rounds, queries};
    ChipFeed chip;
    RK_TRY(c.begin());
    RK_TRY(clear_outputs(ctx, outs, 3));
    RK_TRY(c.chip_feed(sz.chip_log_height, &chip));
    RK_TRY(c.commit(d_publics, d_records, d_fold, d_path, d_claims, /*xcol=*/false, chip));
    return c.chip_trace(chip, d_chip);
    RK_GUARD_END
}

int rk_fri_reduce_sizes(uint32_t log_max, uint32_t blowup_log2, uint32_t queries, const uint32_t* layout, uint32_t n_matrices,
                        rk_fri_reduce_size_info* out) {
    RK_GUARD_BEGIN
    if (!out) return RK_ERR_INVALID;
    FriReducePlan plan;
    RK_TRY(fri_reduce_plan(log_max, blowup_log2, queries, layout, n_matrices, &plan));
    *out = plan.sz;
    return RK_OK;
    RK_GUARD_END
}
int rk_fri_reduce_rows_device(rk_ctx* ctx, uint32_t log_max, uint32_t blowup_log2, uint32_t queries, const uint32_t* layout, uint32_t n_matrices,
                              const uint32_t* d_fold_publics, const uint32_t* d_fold_records, const uint32_t* d_reduce_publics,
                              const uint32_t* d_inputs, uint32_t* d_fold, size_t fold_capacity, uint32_t* d_path, size_t path_capacity,
                              uint32_t* d_reduce, size_t reduce_capacity, uint32_t* d_chip, size_t chip_capacity) {
    RK_GUARD_BEGIN
    if (!ctx || !d_fold_publics || !d_fold_records || !d_reduce_publics || !d_inputs || !d_fold || !d_path || !d_reduce || !d_chip) return RK_ERR_INVALID;
    FriReducePlan plan;
    RK_TRY(fri_reduce_plan(log_max, blowup_log2, queries, layout, n_matrices, &plan));
    const rk_fri_reduce_size_info& sz = plan.sz;
    RK_TRY(fri_scope(ctx, blowup_log2, /*sponge=*/false));
    const OutTable outs[] = {{d_fold, fold_capacity, sz.fold_width, sz.fold_log_height},
                             {d_path, path_capacity, sz.path_width, sz.path_log_height},
                             {d_reduce, reduce_capacity, sz.reduce_width, sz.reduce_log_height},
                             {d_chip, chip_capacity, sz.chip_width, sz.chip_log_height}};
    RK_TRY(check_outputs(outs, 4));
    FriCall c{ctx, log_max, sz.n_rounds, queries};
    ChipFeed chip;
    RK_TRY(c.begin());
    RK_TRY(clear_outputs(ctx, outs, 3));
    RK_TRY(c.chip_feed(sz.chip_log_height, &chip));
    RK_TRY(c.commit(d_fold_publics, d_fold_records, d_fold, d_path, nullptr, /*xcol=*/true, chip));
    RK_TRY(c.reduce(plan, d_reduce_publics, d_inputs, d_reduce, /*stride=*/0));
    return c.chip_trace(chip, d_chip);
    RK_GUARD_END
}

int rk_fri_open_sizes(uint32_t log_max, uint32_t blowup_log2, uint32_t queries, const uint32_t* layout, uint32_t n_matrices,
                      rk_fri_open_size_info* out) {
    RK_GUARD_BEGIN
    if (!out) return RK_ERR_INVALID;
    FriOpenPlan plan;
    RK_TRY(fri_open_plan(log_max, blowup_log2, queries, layout, n_matrices, &plan));
    *out = plan.sz;
    return RK_OK;
    RK_GUARD_END
}
int rk_fri_open_rows_device(rk_ctx* ctx, uint32_t log_max, uint32_t blowup_log2, uint32_t queries, const uint32_t* layout, uint32_t n_matrices,
                            const uint32_t* d_fold_publics, const uint32_t* d_fold_records, const uint32_t* d_reduce_publics,
                            const uint32_t* d_inputs, const uint32_t* d_roots, const uint32_t* d_paths, uint32_t* d_fold, size_t fold_capacity,
                            uint32_t* d_path, size_t path_capacity, uint32_t* d_reduce, size_t reduce_capacity, uint32_t* d_ipath,
                            size_t ipath_capacity, uint32_t* d_chip, size_t chip_capacity, uint32_t* d_state, size_t state_capacity) {
    RK_GUARD_BEGIN
    if (!ctx || !d_fold_publics || !d_fold_records || !d_reduce_publics || !d_inputs || !d_roots || !d_paths || !d_fold || !d_path || !d_reduce ||
        !d_ipath || !d_chip || !d_state)
        return RK_ERR_INVALID;
    FriOpenPlan plan;
    RK_TRY(fri_open_plan(log_max, blowup_log2, queries, layout, n_matrices, &plan));
    const rk_fri_open_size_info& sz = plan.sz;
    RK_TRY(fri_scope(ctx, blowup_log2, /*sponge=*/true));
    const OutTable outs[] = {{d_fold, fold_capacity, sz.fold_width, sz.fold_log_height},
                             {d_path, path_capacity, sz.path_width, sz.path_log_height},
                             {d_reduce, reduce_capacity, sz.reduce_width, sz.reduce_log_height},
                             {d_ipath, ipath_capacity, sz.ipath_width, sz.ipath_log_height},
                             {d_chip, chip_capacity, sz.chip_width, sz.chip_log_height},
                             {d_state, state_capacity, sz.state_width, sz.state_log_height}};
    RK_TRY(check_outputs(outs, 6));
    FriCall c{ctx, log_max, sz.n_rounds, queries};
    ChipFeed chip, state;
    RK_TRY(c.begin());
    RK_TRY(clear_outputs(ctx, outs, 4));
    RK_TRY(c.chip_feed(sz.chip_log_height, &chip));
    RK_TRY(c.chip_feed(sz.state_log_height, &state));
    RK_TRY(c.commit(d_fold_publics, d_fold_records, d_fold, d_path, nullptr, /*xcol=*/true, chip));
    RK_TRY(c.reduce(plan.red, d_reduce_publics, d_inputs, d_reduce, /*stride=*/sz.reduce_width));
    RK_TRY(c.open(plan, d_inputs, d_paths, d_reduce, d_ipath, chip, state));
    RK_TRY(c.chip_trace(chip, d_chip));
    return c.chip_trace(state, d_state);
    RK_GUARD_END
}

int rk_fri_transcript_sizes(uint32_t log_max, uint32_t blowup_log2, uint32_t queries, const uint32_t* layout, uint32_t n_matrices,
                            const uint32_t* ops, uint32_t n_ops, rk_fri_transcript_size_info* out) {
    RK_GUARD_BEGIN
    if (!out) return RK_ERR_INVALID;
    FriTranscriptPlan plan;
    RK_TRY(fri_transcript_plan(log_max, blowup_log2, queries, layout, n_matrices, ops, n_ops, &plan));
    *out = plan.sz;
    return RK_OK;
    RK_GUARD_END
}
int rk_fri_transcript_rows_device(rk_ctx* ctx, uint32_t log_max, uint32_t blowup_log2, uint32_t queries, const uint32_t* layout,
                                  uint32_t n_matrices, const uint32_t* ops, uint32_t n_ops, const uint32_t* d_fold_publics,
                                  const uint32_t* d_fold_records, const uint32_t* d_reduce_publics, const uint32_t* d_inputs,
                                  const uint32_t* d_roots, const uint32_t* d_paths, const uint32_t* d_observed, uint32_t* d_fold,
                                  size_t fold_capacity, uint32_t* d_path, size_t path_capacity, uint32_t* d_reduce, size_t reduce_capacity,
                                  uint32_t* d_ipath, size_t ipath_capacity, uint32_t* d_transcript, size_t transcript_capacity,
                                  uint32_t* d_bits, size_t bits_capacity, uint32_t* d_chip, size_t chip_capacity, uint32_t* d_state,
                                  size_t state_capacity) {
    RK_GUARD_BEGIN
    if (!ctx || !d_fold_publics || !d_fold_records || !d_reduce_publics || !d_inputs || !d_roots || !d_paths || !d_observed || !d_fold ||
        !d_path || !d_reduce || !d_ipath || !d_transcript || !d_bits || !d_chip || !d_state)
        return RK_ERR_INVALID;
    FriTranscriptPlan plan;
    RK_TRY(fri_transcript_plan(log_max, blowup_log2, queries, layout, n_matrices, ops, n_ops, &plan));
    const rk_fri_transcript_size_info& sz = plan.sz;
    RK_TRY(fri_scope(ctx, blowup_log2, /*sponge=*/true));
    const OutTable outs[] = {{d_fold, fold_capacity, sz.fold_width, sz.fold_log_height},
                             {d_path, path_capacity, sz.path_width, sz.path_log_height},
                             {d_reduce, reduce_capacity, sz.reduce_width, sz.reduce_log_height},
                             {d_ipath, ipath_capacity, sz.ipath_width, sz.ipath_log_height},
                             {d_transcript, transcript_capacity, sz.transcript_width, sz.transcript_log_height},
                             {d_bits, bits_capacity, sz.bits_width, sz.bits_log_height},
                             {d_chip, chip_capacity, sz.chip_width, sz.chip_log_height},
                             {d_state, state_capacity, sz.state_width, sz.state_log_height}};
    RK_TRY(check_outputs(outs, 8));
    FriCall c{ctx, log_max, sz.n_rounds, queries};
    ChipFeed chip, state;
    RK_TRY(c.begin());
    RK_TRY(clear_outputs(ctx, outs, 6));
    RK_TRY(c.chip_feed(sz.chip_log_height, &chip));
    RK_TRY(c.chip_feed(sz.state_log_height, &state));
    RK_TRY(c.commit(d_fold_publics, d_fold_records, d_fold, d_path, nullptr, /*xcol=*/true, chip, /*firstcol=*/true));
    RK_TRY(c.reduce(plan.open.red, d_reduce_publics, d_inputs, d_reduce, /*stride=*/sz.reduce_width));
    RK_TRY(c.open(plan.open, d_inputs, d_paths, d_reduce, d_ipath, chip, state));
    RK_TRY(c.transcript(plan, d_observed, d_transcript, d_bits, state));
    RK_TRY(c.chip_trace(chip, d_chip));
    return c.chip_trace(state, d_state);
    RK_GUARD_END
}

}  // extern "C"
