// The AIR front end of rk_p3_* (include/raiko_hip.h): rk_air_create / rk_air_create_lookup -- validation, symbolic degree,
// translation of the step list into an rk_program for the GPU evaluator, sp1-core's eval_permutation_constraints written
// as steps (PermStepGen) -- and the Poseidon2 chip: its AIR written from the configured instance's constants and its rows
// written on the GPU (rk_p2_chip_*), and the rows of the FRI commit-phase tables (rk_fri_chip_*; AIRs: raiko_amd/fri_chip.py).
// Prover and verifier are in p3.hip.  Reference call site of the path:
// provers/sp1/driver/src/lib.rs:44-57; p3-uni-stark symbolic_builder.rs / symbolic_expression.rs, sp1-core
// stark/permutation.rs, sp1-recursion-core's Poseidon2 wide chip: outside the reference tree, RECALLED.
#include "p3_air.hpp"
#include "p3_kernels.hpp"

#include <array>
#include <cstring>
#include <map>
#include <memory>
#include <tuple>

namespace {

using rk::DevBuf;
using rk::NEXT_BACK;

// ---------------------------------------------------------------- AIR: checks, symbolic degree, host evaluation
int air_scan(const rk_air_step* steps, size_t n, uint32_t width, uint32_t n_public, uint32_t perm_width, uint32_t n_chal, rk_air_info* info) {
    std::vector<uint32_t> deg;
    deg.reserve(n);
    uint32_t max_deg = 0, n_con = 0;
    for (size_t s = 0; s < n; s++) {
        const rk_air_step& st = steps[s];
        const size_t nv = deg.size();
        switch (st.op) {
            case RK_AIR_CONST: if (st.a >= bb::P) return RK_ERR_INVALID; deg.push_back(0); break;
            case RK_AIR_LOCAL: case RK_AIR_NEXT: if (st.a >= width) return RK_ERR_INVALID; deg.push_back(1); break;
            case RK_AIR_PUBLIC: if (st.a >= n_public) return RK_ERR_INVALID; deg.push_back(0); break;
            case RK_AIR_IS_FIRST_ROW: case RK_AIR_IS_LAST_ROW: deg.push_back(1); break;
            case RK_AIR_IS_TRANSITION: deg.push_back(0); break;
            case RK_AIR_PERM_LOCAL: case RK_AIR_PERM_NEXT: if (st.a >= perm_width) return RK_ERR_INVALID; deg.push_back(1); break;
            case RK_AIR_CHALLENGE: if (st.a >= n_chal) return RK_ERR_INVALID; deg.push_back(0); break;
            case RK_AIR_CUMSUM: if (st.a >= 4 || perm_width == 0) return RK_ERR_INVALID; deg.push_back(0); break;
            case RK_AIR_ADD: case RK_AIR_SUB:
                if (st.a >= nv || st.b >= nv) return RK_ERR_INVALID;
                deg.push_back(std::max(deg[st.a], deg[st.b]));
                break;
            case RK_AIR_MUL:
                if (st.a >= nv || st.b >= nv) return RK_ERR_INVALID;
                deg.push_back(std::min<uint32_t>(deg[st.a] + deg[st.b], 1u << 20));
                break;
            case RK_AIR_NEG: if (st.a >= nv) return RK_ERR_INVALID; deg.push_back(deg[st.a]); break;
            case RK_AIR_ASSERT_ZERO:
                if (st.a >= nv) return RK_ERR_INVALID;
                max_deg = std::max(max_deg, deg[st.a]);
                n_con++;
                break;
            default: return RK_ERR_INVALID;
        }
    }
    // p3-uni-stark get_log_quotient_degree: log2_ceil(max(constraint degree, 2) - 1)
    info->n_steps = n;
    info->n_constraints = n_con;
    info->max_degree = max_deg;
    info->log_quotient_degree = log2u(std::max(max_deg, 2u) - 1);
    return RK_OK;
}

// sp1-core eval_permutation_constraints (RECALLED) written into a step list over base values: every extension identity
// is four base asserts (the evaluator works on base columns; W is baked in).  `raw` = the caller's interactions as given
// (canonical constants, column numbers).  Appended to `steps`, whose values so far number `nv`.  Equal values are shared.
struct PermStepGen {
    std::vector<rk_air_step>& steps;
    uint32_t nv, w;
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, uint32_t> memo;
    using E = std::array<uint32_t, 4>;
    uint32_t push(uint32_t op, uint32_t a = 0, uint32_t b = 0) {
        const auto key = std::make_tuple(op, a, b);
        auto it = memo.find(key);
        if (it != memo.end()) return it->second;
        steps.push_back(rk_air_step{op, a, b});
        memo.emplace(key, nv);
        return nv++;
    }
    void assert_zero(uint32_t v) { steps.push_back(rk_air_step{RK_AIR_ASSERT_ZERO, v, 0}); }
    uint32_t add(uint32_t a, uint32_t b) { return push(RK_AIR_ADD, a, b); }
    uint32_t sub(uint32_t a, uint32_t b) { return push(RK_AIR_SUB, a, b); }
    uint32_t mul(uint32_t a, uint32_t b) { return push(RK_AIR_MUL, a, b); }
    uint32_t cst(uint32_t canon) { return push(RK_AIR_CONST, canon); }
    uint32_t col(uint32_t c) { return push(RK_AIR_LOCAL, c); }
    E leaf(uint32_t op, uint32_t at) { return E{push(op, 4 * at), push(op, 4 * at + 1), push(op, 4 * at + 2), push(op, 4 * at + 3)}; }
    E add(const E& x, const E& y) { return E{push(RK_AIR_ADD, x[0], y[0]), push(RK_AIR_ADD, x[1], y[1]), push(RK_AIR_ADD, x[2], y[2]), push(RK_AIR_ADD, x[3], y[3])}; }
    E sub(const E& x, const E& y) { return E{push(RK_AIR_SUB, x[0], y[0]), push(RK_AIR_SUB, x[1], y[1]), push(RK_AIR_SUB, x[2], y[2]), push(RK_AIR_SUB, x[3], y[3])}; }
    E scale(const E& x, uint32_t e) { return E{push(RK_AIR_MUL, x[0], e), push(RK_AIR_MUL, x[1], e), push(RK_AIR_MUL, x[2], e), push(RK_AIR_MUL, x[3], e)}; }
    E mul(const E& x, const E& y) {   // modulo t^4 - W
        E out;
        for (int k = 0; k < 4; k++) {
            uint32_t t = push(RK_AIR_MUL, x[0], y[k]);
            for (int i = 1; i <= k; i++) t = push(RK_AIR_ADD, t, push(RK_AIR_MUL, x[i], y[k - i]));
            if (k < 3) {
                uint32_t h = push(RK_AIR_MUL, x[k + 1], y[3]);
                for (int i = k + 2; i < 4; i++) h = push(RK_AIR_ADD, h, push(RK_AIR_MUL, x[i], y[k + 4 - i]));
                t = push(RK_AIR_ADD, t, push(RK_AIR_MUL, h, push(RK_AIR_CONST, w)));
            }
            out[k] = t;
        }
        return out;
    }
    void assert_ext_zero(int32_t cond, const E& x) {
        for (int k = 0; k < 4; k++) assert_zero(cond < 0 ? x[k] : push(RK_AIR_MUL, (uint32_t)cond, x[k]));
    }
    void run(const uint32_t* raw, uint32_t n_lookups) {
        struct Ix {
            uint32_t kind, bus, is_const, mult, nv;
            const uint32_t* cols;
        };
        std::vector<Ix> its;
        for (uint32_t i = 0; i < n_lookups; i++) {
            its.push_back(Ix{raw[0], raw[1], raw[2], raw[3], raw[4], raw + 5});
            raw += 5 + raw[4];
        }
        const uint32_t nb = (n_lookups + 1) / 2;
        const E alpha = leaf(RK_AIR_CHALLENGE, 0);
        auto rlc = [&](const Ix& it) {
            E acc = add(alpha, scale(leaf(RK_AIR_CHALLENGE, 1), push(RK_AIR_CONST, it.bus)));
            for (uint32_t j = 0; j < it.nv; j++) acc = add(acc, scale(leaf(RK_AIR_CHALLENGE, 2 + j), push(RK_AIR_LOCAL, it.cols[j])));
            return acc;
        };
        auto signed_mult = [&](const Ix& it) {
            const uint32_t m = it.is_const ? push(RK_AIR_CONST, it.mult) : push(RK_AIR_LOCAL, it.mult);
            return it.kind == 0 ? m : push(RK_AIR_NEG, m);
        };
        std::vector<E> el, en;
        for (uint32_t b = 0; b < nb; b++) el.push_back(leaf(RK_AIR_PERM_LOCAL, b));
        for (uint32_t b = 0; b < nb; b++) en.push_back(leaf(RK_AIR_PERM_NEXT, b));
        for (uint32_t b = 0; b < nb; b++) {
            if (2 * b + 1 < n_lookups) {   // entry * rlc0 * rlc1 = m0 * rlc1 + m1 * rlc0
                const E r0 = rlc(its[2 * b]), r1 = rlc(its[2 * b + 1]);
                const E lhs = mul(mul(el[b], r0), r1);
                const E rhs = add(scale(r1, signed_mult(its[2 * b])), scale(r0, signed_mult(its[2 * b + 1])));
                assert_ext_zero(-1, sub(lhs, rhs));
            } else {                       // entry * rlc = m
                const E lhs = mul(el[b], rlc(its[2 * b]));
                assert_zero(push(RK_AIR_SUB, lhs[0], signed_mult(its[2 * b])));
                for (int k = 1; k < 4; k++) assert_zero(lhs[k]);
            }
        }
        const E phi_l = leaf(RK_AIR_PERM_LOCAL, nb), phi_n = leaf(RK_AIR_PERM_NEXT, nb);
        E sum_l = el[0], sum_n = en[0];
        for (uint32_t b = 1; b < nb; b++) sum_l = add(sum_l, el[b]), sum_n = add(sum_n, en[b]);
        assert_ext_zero((int32_t)push(RK_AIR_IS_FIRST_ROW), sub(phi_l, sum_l));
        assert_ext_zero((int32_t)push(RK_AIR_IS_TRANSITION), sub(sub(phi_n, phi_l), sum_n));
        assert_ext_zero((int32_t)push(RK_AIR_IS_LAST_ROW), sub(phi_l, leaf(RK_AIR_CUMSUM, 0)));
    }
};

// ---------------------------------------------------------------- the Poseidon2 chip (rk_p2_chip_*)
// One row = one permutation of the configured instance with the values a degree-3 AIR needs in columns -- the shape of
// sp1-recursion-core's Poseidon2 wide chip (RECALLED), the table a recursion / compress layer spends most of its rows
// on (every Merkle path step and sponge block of the proofs it verifies is one lookup into it):
//   in W | per external round r = 0..3: x3_r W (the cube of state + rc), post_r W (the state after the round) |
//   x3i_k R_P (cube of cell 0 + rc in internal round k) | s0_k R_P - 1 (cell 0 entering internal round k >= 1) |
//   int_out W (the state after the internal rounds) | external rounds 4..7 likewise | multiplicity
// x^7 = x3 * x3 * x keeps every constraint at degree 3; between commitments the state is carried as expressions.
using p3k::P2ChipLayout;
P2ChipLayout p2_chip_layout(const p2::Any& k) {
    P2ChipLayout L;
    L.W = (uint32_t)k.cells();
    L.RP = (uint32_t)k.rounds_partial();
    L.width = L.W + 16 * L.W + 2 * L.RP - 1 + L.W + 1;
    return L;
}
void p2_chip_steps(const p2::Any& k, std::vector<rk_air_step>& steps) {
    const P2ChipLayout L = p2_chip_layout(k);
    const uint32_t W = L.W;
    PermStepGen g{steps, 0, 0, {}};
    auto m_ext = [&](std::vector<uint32_t>& c) {   // the external layer on expressions: the 4x4 block on every four cells, then the sums of the cells four apart
        uint32_t sums[4] = {0, 0, 0, 0};
        for (uint32_t i = 0; i < W; i += 4) {
            const uint32_t a = c[i], b = c[i + 1], d = c[i + 2], e = c[i + 3];
            if (!k.m4()) {
                const uint32_t t0 = g.add(a, b), t1 = g.add(d, e), t2 = g.add(g.add(b, b), t1), t3 = g.add(g.add(e, e), t0);
                const uint32_t t1_4 = g.add(g.add(t1, t1), g.add(t1, t1)), t0_4 = g.add(g.add(t0, t0), g.add(t0, t0));
                const uint32_t t4 = g.add(t1_4, t3), t5 = g.add(t0_4, t2);
                c[i] = g.add(t3, t5), c[i + 1] = t5, c[i + 2] = g.add(t2, t4), c[i + 3] = t4;
            } else {
                const uint32_t s = g.add(g.add(a, b), g.add(d, e));
                c[i] = g.add(g.add(s, a), g.add(b, b));
                c[i + 1] = g.add(g.add(s, b), g.add(d, d));
                c[i + 2] = g.add(g.add(s, d), g.add(e, e));
                c[i + 3] = g.add(g.add(s, e), g.add(a, a));
            }
            for (int j = 0; j < 4; j++) sums[j] = i == 0 ? c[j] : g.add(sums[j], c[i + j]);
        }
        for (uint32_t i = 0; i < W; i++) c[i] = g.add(c[i], sums[i & 3]);
    };
    auto ext_round = [&](std::vector<uint32_t>& st, uint32_t r) {
        std::vector<uint32_t> x7(W);
        for (uint32_t i = 0; i < W; i++) {
            const uint32_t s = g.add(st[i], g.cst(bb::decode(k.rc_ext()[r * W + i]))), x3 = g.col(L.x3(r) + i);
            g.assert_zero(g.sub(x3, g.mul(g.mul(s, s), s)));
            x7[i] = g.mul(g.mul(x3, x3), s);
        }
        m_ext(x7);
        for (uint32_t i = 0; i < W; i++) {
            st[i] = g.col(L.post(r) + i);
            g.assert_zero(g.sub(st[i], x7[i]));
        }
    };
    std::vector<uint32_t> st(W);
    for (uint32_t i = 0; i < W; i++) st[i] = g.col(L.in() + i);
    m_ext(st);
    for (uint32_t r = 0; r < 4; r++) ext_round(st, r);
    for (uint32_t kk = 0; kk < L.RP; kk++) {
        uint32_t s0 = st[0];
        if (kk > 0) {
            s0 = g.col(L.s0(kk));
            g.assert_zero(g.sub(s0, st[0]));
        }
        const uint32_t t = g.add(s0, g.cst(bb::decode(k.rc_int()[kk]))), x3 = g.col(L.x3i(kk));
        g.assert_zero(g.sub(x3, g.mul(g.mul(t, t), t)));
        st[0] = g.mul(g.mul(x3, x3), t);
        uint32_t sum = st[0];
        for (uint32_t i = 1; i < W; i++) sum = g.add(sum, st[i]);
        for (uint32_t i = 0; i < W; i++) st[i] = g.add(sum, g.mul(st[i], g.cst(bb::decode(k.diag()[i]))));
    }
    for (uint32_t i = 0; i < W; i++) {
        const uint32_t c = g.col(L.int_out() + i);
        g.assert_zero(g.sub(c, st[i]));
        st[i] = c;
    }
    for (uint32_t r = 4; r < 8; r++) ext_round(st, r);
}

// the chip's rows on the GPU: one lane per permutation (p3k::chip_row, p3_kernels.hpp)
template <int W, int RP, int M4>
__global__ void __launch_bounds__(128) p2_chip_trace_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, const uint32_t* __restrict__ mult,
                                                            const uint32_t* __restrict__ tab, size_t n, P2ChipLayout L) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    p3k::chip_row<W, RP, M4>(out + r * L.width, in + r * W, mult ? mult[r] : bb::ONE, tab, L);
}

std::vector<uint32_t> p2_chip_tab(const p2::Any& k) {   // rc_ext | rc_int | diag: what p3k::chip_permute reads
    const P2ChipLayout L = p2_chip_layout(k);
    std::vector<uint32_t> tab(k.rc_ext(), k.rc_ext() + 8 * L.W);
    tab.insert(tab.end(), k.rc_int(), k.rc_int() + L.RP);
    tab.insert(tab.end(), k.diag(), k.diag() + L.W);
    return tab;
}

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
    auto lh = [](uint64_t rows) { return std::max(1u, log2u((size_t)rows)); };
    *o = rk_fri_chip_size_info{};
    o->n_rounds = a.R;
    o->fold_width = a.fold_width(), o->path_width = a.path_width(), o->claims_width = p3k::FRI_CLAIMS_WIDTH, o->chip_width = 314;
    o->fold_rows = (uint64_t)a.Q * a.R;
    o->path_rows = (uint64_t)a.Q * a.steps_before(a.R);
    o->chip_rows = o->fold_rows + o->path_rows;
    o->fold_log_height = o->claims_log_height = lh(o->fold_rows);
    o->path_log_height = lh(o->path_rows);
    o->chip_log_height = lh(o->chip_rows);
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
    std::vector<uint32_t> batch;      // per slot; 3 = the single row of a round without a matrix
};
// the schedule of the reduce table from the layout of rk_p3_fri_inputs (Montgomery words; 5 per matrix): the matrices by
// round, in the layout's order within a round, and one single-row slot for every round without a matrix
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
        if (m.batch > 2 || (i && m.batch < ms[i - 1].batch) || m.rd >= R || m.width == 0 || m.width > (1u << 16)) return RK_ERR_INVALID;
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
            plan->batch.push_back(3);
            rows += 1;
        }
        plan->slots[plan->slots.size() - p3k::FRI_REDUCE_SLOT_WORDS + 5] = 1;
    }
    auto lh = [](uint64_t r) { return std::max(1u, log2u((size_t)r)); };
    rk_fri_reduce_size_info& o = plan->sz;
    o = rk_fri_reduce_size_info{};
    o.n_rounds = R, o.n_slots = (uint32_t)(plan->slots.size() / p3k::FRI_REDUCE_SLOT_WORDS);
    o.fold_width = chip.fold_width + 1, o.path_width = chip.path_width, o.reduce_width = p3k::FRI_REDUCE_FIXED + o.n_slots, o.chip_width = chip.chip_width;
    o.fold_rows = chip.fold_rows, o.path_rows = chip.path_rows, o.chip_rows = chip.chip_rows, o.reduce_rows = rows * queries;
    if (o.reduce_rows > ((uint64_t)1 << 26)) return RK_ERR_INVALID;
    o.fold_log_height = chip.fold_log_height, o.path_log_height = chip.path_log_height, o.chip_log_height = chip.chip_log_height;
    o.reduce_log_height = lh(o.reduce_rows);
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
    uint32_t height[3] = {0, 0, 0};                  // log LDE height of a batch's tallest matrix; 0 = batch absent
    for (uint32_t m = 0; m < M;) {
        const uint32_t b = plan->red.batch[m], rd = slots[W * m];
        if (b == 3) {
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
    for (uint32_t b = 0; b < 3; b++) {
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
    auto lh = [](uint64_t n) { return std::max(1u, log2u((size_t)n)); };
    rk_fri_open_size_info& o = plan->sz;
    o = rk_fri_open_size_info{};
    o.n_rounds = r.n_rounds, o.n_slots = M, o.n_groups = G, o.n_batches = nb;
    o.fold_width = r.fold_width, o.path_width = r.path_width, o.reduce_width = r.reduce_width + p3k::FRI_OPEN_SPONGE_COLS;
    o.ipath_width = p3k::FRI_OPEN_IPATH_FIXED + nb, o.chip_width = r.chip_width, o.state_width = r.chip_width;
    o.fold_rows = r.fold_rows, o.path_rows = r.path_rows, o.reduce_rows = r.reduce_rows, o.ipath_rows = rows;
    o.chip_rows = r.chip_rows + chips, o.state_rows = perms * queries, o.rows_per_query = r.rows_per_query;
    if (o.chip_rows > ((uint64_t)1 << 24) || o.state_rows > ((uint64_t)1 << 24)) return RK_ERR_INVALID;
    o.fold_log_height = r.fold_log_height, o.path_log_height = r.path_log_height, o.reduce_log_height = r.reduce_log_height;
    o.ipath_log_height = lh(rows), o.chip_log_height = lh(o.chip_rows), o.state_log_height = lh(o.state_rows);
    o.fold_publics_words = r.fold_publics_words, o.fold_records_words = r.fold_records_words;
    o.reduce_publics_words = r.reduce_publics_words, o.inputs_words = r.inputs_words;
    o.roots_words = 25, o.paths_words = (uint64_t)queries * path_off;
    o.log_pmax = height[1];
    plan->chip_base = r.chip_rows;
    return RK_OK;
}

}  // namespace

extern "C" {

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
    const p2::Any& k = ctx->h_p2;
    if (k.cells() != 16 || ctx->sys.blowup_log2 != blowup_log2 || ctx->sys.fri_fold_log2 != 1) return RK_ERR_INVALID;
    const size_t fold_words = ((size_t)sz.fold_width) << sz.fold_log_height, path_words = ((size_t)sz.path_width) << sz.path_log_height;
    const size_t reduce_words = ((size_t)sz.reduce_width) << sz.reduce_log_height, chip_words = ((size_t)sz.chip_width) << sz.chip_log_height;
    if (fold_capacity < fold_words || path_capacity < path_words || reduce_capacity < reduce_words || chip_capacity < chip_words) return RK_ERR_CAPACITY;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (uint32_t m = 0; m < sz.n_slots; m++)
        plan.slots[p3k::FRI_REDUCE_SLOT_WORDS * m + 4] = bb::pow(ctx->sys.root27m, (uint64_t)1 << (27 - plan.log_n[m]));
    const P2ChipLayout L = p2_chip_layout(k);
    const std::vector<uint32_t> tab = p2_chip_tab(k);
    const size_t chip_n = (size_t)1 << sz.chip_log_height;
    DevBuf d_tab, d_in, d_mult, d_slots, d_apow;
    RK_TRY(d_tab.alloc(ctx, tab.size() * 4));
    RK_TRY(d_in.alloc(ctx, chip_n * 16 * 4));
    RK_TRY(d_mult.alloc(ctx, chip_n * 4));
    RK_TRY(d_slots.alloc(ctx, plan.slots.size() * 4));
    RK_TRY(d_apow.alloc(ctx, 32 * 4 * 4));
    RK_TRY(rk::upload(ctx, d_tab.p, tab.data(), tab.size() * 4));
    RK_TRY(rk::upload(ctx, d_slots.p, plan.slots.data(), plan.slots.size() * 4));
    RK_HIP_TRY(ctx, hipMemsetAsync(d_fold, 0, fold_words * 4, ctx->stream));
    RK_HIP_TRY(ctx, hipMemsetAsync(d_path, 0, path_words * 4, ctx->stream));
    RK_HIP_TRY(ctx, hipMemsetAsync(d_reduce, 0, reduce_words * 4, ctx->stream));
    RK_HIP_TRY(ctx, hipMemsetAsync(d_in.p, 0, chip_n * 16 * 4, ctx->stream));
    RK_HIP_TRY(ctx, hipMemsetAsync(d_mult.p, 0, chip_n * 4, ctx->stream));
    p3k::FriArgs a{};
    a.L = log_max, a.R = sz.n_rounds, a.Q = queries;
    a.gen_l = bb::pow(ctx->sys.root27m, (uint64_t)1 << (27 - log_max));
    a.wm = ctx->sys.wm;
    a.pub = d_fold_publics, a.rec = d_fold_records;
    a.fold = d_fold, a.path = d_path, a.claims = nullptr, a.chip_in = d_in.u32(), a.chip_mult = d_mult.u32();
    a.xcol = 1, a.shiftm = ctx->sys.shiftm;
    hipLaunchKernelGGL(fri_fold_kernel, dim3((queries + 63) / 64), dim3(64), 0, ctx->stream, a);
    RK_TRY(rk::post_launch(ctx, "fri_fold_kernel"));
    const dim3 grid((unsigned)((sz.fold_rows + 63) / 64)), block(64);
    if (k.m4()) hipLaunchKernelGGL((fri_path_kernel<1>), grid, block, 0, ctx->stream, a, (const uint32_t*)d_tab.u32(), L);
    else hipLaunchKernelGGL((fri_path_kernel<0>), grid, block, 0, ctx->stream, a, (const uint32_t*)d_tab.u32(), L);
    RK_TRY(rk::post_launch(ctx, "fri_path_kernel"));
    p3k::FriReduceArgs r{};
    r.L = log_max, r.R = sz.n_rounds, r.Q = queries, r.M = sz.n_slots;
    r.rows_per_query = (uint32_t)sz.rows_per_query, r.wm = ctx->sys.wm, r.shiftm = ctx->sys.shiftm, r.gen_l = a.gen_l;
    r.per_record = (size_t)(sz.inputs_words / queries);
    r.slots = d_slots.u32(), r.pub = d_reduce_publics, r.rec = d_inputs, r.apow = d_apow.u32(), r.out = d_reduce;
    hipLaunchKernelGGL(fri_reduce_pows_kernel, dim3(1), dim3(64), 0, ctx->stream, d_apow.u32(), d_reduce_publics, r.wm);
    RK_TRY(rk::post_launch(ctx, "fri_reduce_pows_kernel"));
    hipLaunchKernelGGL(fri_reduce_kernel, dim3(queries * sz.n_rounds), dim3(p3k::FRI_REDUCE_TPB), 0, ctx->stream, r);
    RK_TRY(rk::post_launch(ctx, "fri_reduce_kernel"));
    return rk_p2_chip_trace(ctx, d_in.u32(), d_mult.u32(), chip_n, d_chip);
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
    const p2::Any& k = ctx->h_p2;
    if (k.cells() != 16 || !k.pad_free || ctx->sys.blowup_log2 != blowup_log2 || ctx->sys.fri_fold_log2 != 1) return RK_ERR_INVALID;
    const size_t fold_words = ((size_t)sz.fold_width) << sz.fold_log_height, path_words = ((size_t)sz.path_width) << sz.path_log_height;
    const size_t reduce_words = ((size_t)sz.reduce_width) << sz.reduce_log_height, ipath_words = ((size_t)sz.ipath_width) << sz.ipath_log_height;
    const size_t chip_words = ((size_t)sz.chip_width) << sz.chip_log_height, state_words = ((size_t)sz.state_width) << sz.state_log_height;
    if (fold_capacity < fold_words || path_capacity < path_words || reduce_capacity < reduce_words || ipath_capacity < ipath_words ||
        chip_capacity < chip_words || state_capacity < state_words)
        return RK_ERR_CAPACITY;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (uint32_t m = 0; m < sz.n_slots; m++)
        plan.red.slots[p3k::FRI_REDUCE_SLOT_WORDS * m + 4] = bb::pow(ctx->sys.root27m, (uint64_t)1 << (27 - plan.red.log_n[m]));
    const P2ChipLayout L = p2_chip_layout(k);
    const std::vector<uint32_t> tab = p2_chip_tab(k);
    const size_t chip_n = (size_t)1 << sz.chip_log_height, state_n = (size_t)1 << sz.state_log_height;
    const size_t dig_words = (size_t)queries * sz.n_groups * 8;
    DevBuf d_tab, d_in, d_mult, d_sin, d_smult, d_slots, d_apow, d_groups, d_rowinfo, d_levels, d_dig;
    RK_TRY(d_tab.alloc(ctx, tab.size() * 4));
    RK_TRY(d_in.alloc(ctx, chip_n * 16 * 4));
    RK_TRY(d_mult.alloc(ctx, chip_n * 4));
    RK_TRY(d_sin.alloc(ctx, state_n * 16 * 4));
    RK_TRY(d_smult.alloc(ctx, state_n * 4));
    RK_TRY(d_slots.alloc(ctx, plan.red.slots.size() * 4));
    RK_TRY(d_apow.alloc(ctx, 32 * 4 * 4));
    RK_TRY(d_groups.alloc(ctx, plan.groups.size() * 4));
    RK_TRY(d_rowinfo.alloc(ctx, plan.rowinfo.size() * 4));
    RK_TRY(d_levels.alloc(ctx, plan.levels.size() * 4));
    RK_TRY(d_dig.alloc(ctx, dig_words * 4));
    RK_TRY(rk::upload(ctx, d_tab.p, tab.data(), tab.size() * 4));
    RK_TRY(rk::upload(ctx, d_slots.p, plan.red.slots.data(), plan.red.slots.size() * 4));
    RK_TRY(rk::upload(ctx, d_groups.p, plan.groups.data(), plan.groups.size() * 4));
    RK_TRY(rk::upload(ctx, d_rowinfo.p, plan.rowinfo.data(), plan.rowinfo.size() * 4));
    RK_TRY(rk::upload(ctx, d_levels.p, plan.levels.data(), plan.levels.size() * 4));
    // rows and inputs the lanes do not write are padding: all zero (multiplicity 0, no selector set)
    RK_HIP_TRY(ctx, hipMemsetAsync(d_fold, 0, fold_words * 4, ctx->stream));
    RK_HIP_TRY(ctx, hipMemsetAsync(d_path, 0, path_words * 4, ctx->stream));
    RK_HIP_TRY(ctx, hipMemsetAsync(d_reduce, 0, reduce_words * 4, ctx->stream));
    RK_HIP_TRY(ctx, hipMemsetAsync(d_ipath, 0, ipath_words * 4, ctx->stream));
    RK_HIP_TRY(ctx, hipMemsetAsync(d_in.p, 0, chip_n * 16 * 4, ctx->stream));
    RK_HIP_TRY(ctx, hipMemsetAsync(d_mult.p, 0, chip_n * 4, ctx->stream));
    RK_HIP_TRY(ctx, hipMemsetAsync(d_sin.p, 0, state_n * 16 * 4, ctx->stream));
    RK_HIP_TRY(ctx, hipMemsetAsync(d_smult.p, 0, state_n * 4, ctx->stream));
    p3k::FriArgs a{};
    a.L = log_max, a.R = sz.n_rounds, a.Q = queries;
    a.gen_l = bb::pow(ctx->sys.root27m, (uint64_t)1 << (27 - log_max));
    a.wm = ctx->sys.wm;
    a.pub = d_fold_publics, a.rec = d_fold_records;
    a.fold = d_fold, a.path = d_path, a.claims = nullptr, a.chip_in = d_in.u32(), a.chip_mult = d_mult.u32();
    a.xcol = 1, a.shiftm = ctx->sys.shiftm;
    hipLaunchKernelGGL(fri_fold_kernel, dim3((queries + 63) / 64), dim3(64), 0, ctx->stream, a);
    RK_TRY(rk::post_launch(ctx, "fri_fold_kernel"));
    const dim3 grid((unsigned)((sz.fold_rows + 63) / 64)), block(64);
    const uint32_t* d_tabw = d_tab.u32();
    if (k.m4()) hipLaunchKernelGGL((fri_path_kernel<1>), grid, block, 0, ctx->stream, a, d_tabw, L);
    else hipLaunchKernelGGL((fri_path_kernel<0>), grid, block, 0, ctx->stream, a, d_tabw, L);
    RK_TRY(rk::post_launch(ctx, "fri_path_kernel"));
    p3k::FriReduceArgs r{};
    r.L = log_max, r.R = sz.n_rounds, r.Q = queries, r.M = sz.n_slots;
    r.rows_per_query = (uint32_t)sz.rows_per_query, r.wm = ctx->sys.wm, r.shiftm = ctx->sys.shiftm, r.gen_l = a.gen_l;
    r.per_record = (size_t)(sz.inputs_words / queries);
    r.slots = d_slots.u32(), r.pub = d_reduce_publics, r.rec = d_inputs, r.apow = d_apow.u32(), r.out = d_reduce;
    r.stride = sz.reduce_width;
    hipLaunchKernelGGL(fri_reduce_pows_kernel, dim3(1), dim3(64), 0, ctx->stream, d_apow.u32(), d_reduce_publics, r.wm);
    RK_TRY(rk::post_launch(ctx, "fri_reduce_pows_kernel"));
    hipLaunchKernelGGL(fri_reduce_kernel, dim3(queries * sz.n_rounds), dim3(p3k::FRI_REDUCE_TPB), 0, ctx->stream, r);
    RK_TRY(rk::post_launch(ctx, "fri_reduce_kernel"));
    p3k::FriOpenArgs o{};
    o.L = log_max, o.Q = queries, o.M = sz.n_slots, o.G = sz.n_groups, o.NB = sz.n_batches;
    o.rows_per_query = (uint32_t)sz.rows_per_query, o.stride = sz.reduce_width, o.sponge_at = sz.reduce_width - p3k::FRI_OPEN_SPONGE_COLS;
    o.per_record = r.per_record, o.per_path = (size_t)(sz.paths_words / queries), o.chip_base = (size_t)plan.chip_base;
    o.slots = d_slots.u32(), o.groups = d_groups.u32(), o.rowinfo = d_rowinfo.u32(), o.levels = d_levels.u32(), o.rec = d_inputs, o.paths = d_paths;
    o.reduce = d_reduce, o.ipath = d_ipath, o.state_in = d_sin.u32(), o.state_mult = d_smult.u32(), o.chip_in = d_in.u32(), o.chip_mult = d_mult.u32();
    o.digests = d_dig.u32();
    const dim3 sgrid((unsigned)(((size_t)queries * sz.n_groups + 63) / 64));
    if (k.m4()) hipLaunchKernelGGL((fri_open_sponge_kernel<1>), sgrid, block, 0, ctx->stream, o, d_tabw, L);
    else hipLaunchKernelGGL((fri_open_sponge_kernel<0>), sgrid, block, 0, ctx->stream, o, d_tabw, L);
    RK_TRY(rk::post_launch(ctx, "fri_open_sponge_kernel"));
    hipLaunchKernelGGL(fri_open_fill_kernel, dim3((unsigned)((sz.reduce_rows + 255) / 256)), dim3(256), 0, ctx->stream, o);
    RK_TRY(rk::post_launch(ctx, "fri_open_fill_kernel"));
    const dim3 igrid((unsigned)(((size_t)queries * sz.n_batches + 63) / 64));
    if (k.m4()) hipLaunchKernelGGL((fri_open_ipath_kernel<1>), igrid, block, 0, ctx->stream, o, d_tabw, L);
    else hipLaunchKernelGGL((fri_open_ipath_kernel<0>), igrid, block, 0, ctx->stream, o, d_tabw, L);
    RK_TRY(rk::post_launch(ctx, "fri_open_ipath_kernel"));
    RK_TRY(rk_p2_chip_trace(ctx, d_in.u32(), d_mult.u32(), chip_n, d_chip));
    return rk_p2_chip_trace(ctx, d_sin.u32(), d_smult.u32(), state_n, d_state);
    RK_GUARD_END
}

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
    const p2::Any& k = ctx->h_p2;
    if (k.cells() != 16 || ctx->sys.blowup_log2 != blowup_log2 || ctx->sys.fri_fold_log2 != 1) return RK_ERR_INVALID;
    const size_t fold_words = ((size_t)sz.fold_width) << sz.fold_log_height, path_words = ((size_t)sz.path_width) << sz.path_log_height;
    const size_t claims_words = ((size_t)sz.claims_width) << sz.claims_log_height, chip_words = ((size_t)sz.chip_width) << sz.chip_log_height;
    if (fold_capacity < fold_words || path_capacity < path_words || claims_capacity < claims_words || chip_capacity < chip_words) return RK_ERR_CAPACITY;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const P2ChipLayout L = p2_chip_layout(k);
    const std::vector<uint32_t> tab = p2_chip_tab(k);
    const size_t chip_n = (size_t)1 << sz.chip_log_height;
    DevBuf d_tab, d_in, d_mult;
    RK_TRY(d_tab.alloc(ctx, tab.size() * 4));
    RK_TRY(d_in.alloc(ctx, chip_n * 16 * 4));
    RK_TRY(d_mult.alloc(ctx, chip_n * 4));
    RK_TRY(rk::upload(ctx, d_tab.p, tab.data(), tab.size() * 4));
    // rows and inputs the lanes do not write are padding: all zero (multiplicity 0, no selector set)
    RK_HIP_TRY(ctx, hipMemsetAsync(d_fold, 0, fold_words * 4, ctx->stream));
    RK_HIP_TRY(ctx, hipMemsetAsync(d_path, 0, path_words * 4, ctx->stream));
    RK_HIP_TRY(ctx, hipMemsetAsync(d_claims, 0, claims_words * 4, ctx->stream));
    RK_HIP_TRY(ctx, hipMemsetAsync(d_in.p, 0, chip_n * 16 * 4, ctx->stream));
    RK_HIP_TRY(ctx, hipMemsetAsync(d_mult.p, 0, chip_n * 4, ctx->stream));
    p3k::FriArgs a{};
    a.L = log_max, a.R = sz.n_rounds, a.Q = queries;
    a.gen_l = bb::pow(ctx->sys.root27m, (uint64_t)1 << (27 - log_max));
    a.wm = ctx->sys.wm;
    a.pub = d_publics, a.rec = d_records;
    a.fold = d_fold, a.path = d_path, a.claims = d_claims, a.chip_in = d_in.u32(), a.chip_mult = d_mult.u32();
    hipLaunchKernelGGL(fri_fold_kernel, dim3((queries + 63) / 64), dim3(64), 0, ctx->stream, a);
    RK_TRY(rk::post_launch(ctx, "fri_fold_kernel"));
    const dim3 grid((unsigned)((sz.fold_rows + 63) / 64)), block(64);
    if (k.m4()) hipLaunchKernelGGL((fri_path_kernel<1>), grid, block, 0, ctx->stream, a, (const uint32_t*)d_tab.u32(), L);
    else hipLaunchKernelGGL((fri_path_kernel<0>), grid, block, 0, ctx->stream, a, (const uint32_t*)d_tab.u32(), L);
    RK_TRY(rk::post_launch(ctx, "fri_path_kernel"));
    return rk_p2_chip_trace(ctx, d_in.u32(), d_mult.u32(), chip_n, d_chip);
    RK_GUARD_END
}

int rk_air_create(const rk_air_step* steps, size_t n_steps, uint32_t width, uint32_t n_public, rk_air** out) {
    return rk_air_create_lookup(steps, n_steps, width, n_public, nullptr, 0, 0, 0, out);
}
int rk_air_create_lookup(const rk_air_step* steps_in, size_t n_steps_in, uint32_t width, uint32_t n_public, const uint32_t* iw,
                         uint32_t n_interactions, size_t n_words, uint32_t ext_w, rk_air** out) {
    RK_GUARD_BEGIN
    if (!out) return RK_ERR_INVALID;
    *out = nullptr;
    const rk_air_step* steps = steps_in;
    size_t n_steps = n_steps_in;
    // a table that only takes part in lookups has no constraints of its own: an empty list is fine when the library writes the rest
    if (((!steps || n_steps == 0) && !(ext_w && n_steps == 0)) || n_steps > ((size_t)1 << 27) || width == 0 || width > (1u << 16) || n_public > (1u << 20)) return RK_ERR_INVALID;
    if (n_interactions > 4096 || (n_interactions && !iw) || (!n_interactions && n_words)) return RK_ERR_INVALID;
    if (ext_w >= bb::P || (ext_w && !n_interactions)) return RK_ERR_INVALID;
    std::unique_ptr<rk_air> air(new rk_air);
    {   // the interactions: kind, bus, mult_is_const, mult, n_values, columns...
        size_t at = 0;
        uint32_t max_values = 0;
        for (uint32_t i = 0; i < n_interactions; i++) {
            if (at + 5 > n_words) return RK_ERR_INVALID;
            const uint32_t kind = iw[at], bus = iw[at + 1], is_const = iw[at + 2], mult = iw[at + 3], nv = iw[at + 4];
            if (kind > 1 || bus >= bb::P || is_const > 1 || nv > 64 || at + 5 + nv > n_words) return RK_ERR_INVALID;
            if (is_const ? mult >= bb::P : mult >= width) return RK_ERR_INVALID;
            auto slot = [&](uint32_t col) {
                auto it = std::find(air->used.begin(), air->used.end(), col);
                if (it == air->used.end()) {
                    air->used.push_back(col);
                    return (uint32_t)air->used.size() - 1;
                }
                return (uint32_t)(it - air->used.begin());
            };
            air->lookups.insert(air->lookups.end(), {kind, bb::encode(bus), is_const, is_const ? bb::encode(mult) : slot(mult), nv});
            for (uint32_t j = 0; j < nv; j++) {
                if (iw[at + 5 + j] >= width) return RK_ERR_INVALID;
                air->lookups.push_back(slot(iw[at + 5 + j]));
            }
            max_values = std::max(max_values, nv);
            at += 5 + nv;
        }
        if (at != n_words) return RK_ERR_INVALID;
        if (air->used.size() > 120) return RK_ERR_INVALID;   // the staged tile (120 x 257 words of LDS)
        air->n_lookups = n_interactions;
        if (n_interactions) {
            air->perm_width = 4 * ((n_interactions + 1) / 2 + 1);
            air->n_chal = 4 * (max_values + 2);
        }
    }
    const uint32_t pw = air->perm_width, n_chal = air->n_chal;
    std::vector<rk_air_step> extended;
    if (ext_w) {   // the caller's list holds the main constraints only: append eval_permutation_constraints for x^4 - ext_w
        if (n_steps) RK_TRY(air_scan(steps, n_steps, width, n_public, 0, 0, &air->info));   // ... and may not name the permutation trace itself
        if (n_steps) extended.assign(steps, steps + n_steps);
        uint32_t nv = 0;
        for (const rk_air_step& st : extended) nv += st.op != RK_AIR_ASSERT_ZERO;
        PermStepGen gen{extended, nv, ext_w, {}};
        gen.run(iw, n_interactions);
        steps = extended.data();
        n_steps = extended.size();
    }
    RK_TRY(air_scan(steps, n_steps, width, n_public, pw, n_chal, &air->info));
    air->steps.assign(steps, steps + n_steps);
    air->width = width;
    air->n_public = n_public;
    // the list as an rk_program: taps 0..2 = the selector columns (group 0), 3 + c = LOCAL c, 3 + width + c = NEXT c
    // (group 2), then PERM_LOCAL / PERM_NEXT c (group 1); PUBLIC / CHALLENGE / CUMSUM = GET_GLOBAL of the proof's globals
    // (public values | challenges | cumulative sum); NEG a = 0 - a; the asserts one AND_EQZ chain
    std::vector<rk::Tap> taps;
    for (uint32_t c = 0; c < 3; c++) taps.push_back(rk::Tap{0, c, 0});
    for (uint32_t c = 0; c < width; c++) taps.push_back(rk::Tap{2, c, 0});
    for (uint32_t c = 0; c < width; c++) taps.push_back(rk::Tap{2, c, NEXT_BACK});
    for (uint32_t c = 0; c < pw; c++) taps.push_back(rk::Tap{1, c, 0});
    for (uint32_t c = 0; c < pw; c++) taps.push_back(rk::Tap{1, c, NEXT_BACK});
    std::vector<rk_poly_step> ps;
    ps.reserve(n_steps + 2);
    std::vector<uint32_t> fp_of;   // AIR value -> position in the program's field-value list
    fp_of.reserve(n_steps);
    uint32_t n_fp = 0, n_mx = 0, zero = rk::PROGRAM_NONE;
    ps.push_back(rk_poly_step{RK_STEP_TRUE, 0, 0, 0});
    uint32_t chain = n_mx++;
    for (size_t s = 0; s < n_steps; s++) {
        const rk_air_step& st = steps[s];
        switch (st.op) {
            case RK_AIR_CONST: ps.push_back(rk_poly_step{RK_STEP_CONST, st.a, 0, 0}); fp_of.push_back(n_fp++); break;
            case RK_AIR_LOCAL: ps.push_back(rk_poly_step{RK_STEP_GET, 3 + st.a, 0, 0}); fp_of.push_back(n_fp++); break;
            case RK_AIR_NEXT: ps.push_back(rk_poly_step{RK_STEP_GET, 3 + width + st.a, 0, 0}); fp_of.push_back(n_fp++); break;
            case RK_AIR_PUBLIC: ps.push_back(rk_poly_step{RK_STEP_GET_GLOBAL, 0, st.a, 0}); fp_of.push_back(n_fp++); break;
            case RK_AIR_PERM_LOCAL: ps.push_back(rk_poly_step{RK_STEP_GET, 3 + 2 * width + st.a, 0, 0}); fp_of.push_back(n_fp++); break;
            case RK_AIR_PERM_NEXT: ps.push_back(rk_poly_step{RK_STEP_GET, 3 + 2 * width + pw + st.a, 0, 0}); fp_of.push_back(n_fp++); break;
            case RK_AIR_CHALLENGE: ps.push_back(rk_poly_step{RK_STEP_GET_GLOBAL, 0, n_public + st.a, 0}); fp_of.push_back(n_fp++); break;
            case RK_AIR_CUMSUM: ps.push_back(rk_poly_step{RK_STEP_GET_GLOBAL, 0, n_public + n_chal + st.a, 0}); fp_of.push_back(n_fp++); break;
            case RK_AIR_IS_FIRST_ROW: case RK_AIR_IS_LAST_ROW: case RK_AIR_IS_TRANSITION:
                air->sel_mask |= 1u << (st.op - RK_AIR_IS_FIRST_ROW);
                ps.push_back(rk_poly_step{RK_STEP_GET, st.op - RK_AIR_IS_FIRST_ROW, 0, 0});
                fp_of.push_back(n_fp++);
                break;
            case RK_AIR_ADD: ps.push_back(rk_poly_step{RK_STEP_ADD, fp_of[st.a], fp_of[st.b], 0}); fp_of.push_back(n_fp++); break;
            case RK_AIR_SUB: ps.push_back(rk_poly_step{RK_STEP_SUB, fp_of[st.a], fp_of[st.b], 0}); fp_of.push_back(n_fp++); break;
            case RK_AIR_MUL: ps.push_back(rk_poly_step{RK_STEP_MUL, fp_of[st.a], fp_of[st.b], 0}); fp_of.push_back(n_fp++); break;
            case RK_AIR_NEG:
                if (zero == rk::PROGRAM_NONE) {
                    ps.push_back(rk_poly_step{RK_STEP_CONST, 0, 0, 0});
                    zero = n_fp++;
                }
                ps.push_back(rk_poly_step{RK_STEP_SUB, zero, fp_of[st.a], 0});
                fp_of.push_back(n_fp++);
                break;
            default:  // ASSERT_ZERO
                ps.push_back(rk_poly_step{RK_STEP_AND_EQZ, chain, fp_of[st.a], 0});
                chain = n_mx++;
                break;
        }
    }
    RK_TRY(rk::program_create_raw(ps.data(), ps.size(), chain, std::move(taps), /*horner=*/true, &air->prog));
    rk_program_info pi;
    (void)rk_program_get_info(air->prog, &pi);
    air->info.n_ops = pi.n_ops;
    air->info.n_fp_slots = pi.n_fp_slots;
    *out = air.release();
    return RK_OK;
    RK_GUARD_END
}
uint32_t rk_p2_chip_width(const rk_params* params) {
    rk_params def;
    rk::params_preset(&def, RK_PRESET_SP1);
    rk::Sys sys;
    auto k = std::make_unique<p2::Any>();
    if (rk::resolve_params(params ? params : &def, &sys, k.get()) != RK_OK) return 0;
    return p2_chip_layout(*k).width;
}
int rk_p2_chip_air_ex(const rk_params* params, uint32_t bus, uint32_t n_out, rk_air** out) {
    RK_GUARD_BEGIN
    if (!out) return RK_ERR_INVALID;
    *out = nullptr;
    rk_params def;
    rk::params_preset(&def, RK_PRESET_SP1);
    const rk_params& par = params ? *params : def;
    rk::Sys sys;
    auto k = std::make_unique<p2::Any>();
    RK_TRY(rk::resolve_params(&par, &sys, k.get()));
    if (bus >= bb::P || (n_out != (uint32_t)p2::OUT && n_out != 16)) return RK_ERR_INVALID;
    const P2ChipLayout L = p2_chip_layout(*k);
    std::vector<rk_air_step> steps;
    p2_chip_steps(*k, steps);
    // receives (bus: in[0..W), out[0..n_out)) `multiplicity` times per row
    std::vector<uint32_t> ix = {1, bus, 0, L.mult(), L.W + n_out};
    for (uint32_t i = 0; i < L.W; i++) ix.push_back(L.in() + i);
    for (uint32_t i = 0; i < n_out; i++) ix.push_back(L.out() + i);
    return rk_air_create_lookup(steps.data(), steps.size(), L.width, 0, ix.data(), 1, ix.size(), par.ext_w, out);
    RK_GUARD_END
}
int rk_p2_chip_air(const rk_params* params, uint32_t bus, rk_air** out) { return rk_p2_chip_air_ex(params, bus, (uint32_t)p2::OUT, out); }
int rk_p2_chip_trace(rk_ctx* ctx, const uint32_t* d_inputs, const uint32_t* d_mult, size_t n, uint32_t* d_trace) {
    RK_GUARD_BEGIN
    if (!ctx || !d_inputs || !d_trace || n == 0 || n > ((size_t)1 << 24)) return RK_ERR_INVALID;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const p2::Any& k = ctx->h_p2;
    const P2ChipLayout L = p2_chip_layout(k);
    const std::vector<uint32_t> tab = p2_chip_tab(k);
    DevBuf d_tab;
    RK_TRY(d_tab.alloc(ctx, tab.size() * 4));
    RK_TRY(rk::upload(ctx, d_tab.p, tab.data(), tab.size() * 4));
    const dim3 grid((unsigned)((n + 127) / 128)), block(128);
    switch (k.kind) {
        case 0: hipLaunchKernelGGL((p2_chip_trace_kernel<24, 21, 0>), grid, block, 0, ctx->stream, d_trace, d_inputs, d_mult, (const uint32_t*)d_tab.u32(), n, L); break;
        case 1: hipLaunchKernelGGL((p2_chip_trace_kernel<24, 21, 1>), grid, block, 0, ctx->stream, d_trace, d_inputs, d_mult, (const uint32_t*)d_tab.u32(), n, L); break;
        case 2: hipLaunchKernelGGL((p2_chip_trace_kernel<16, 13, 0>), grid, block, 0, ctx->stream, d_trace, d_inputs, d_mult, (const uint32_t*)d_tab.u32(), n, L); break;
        default: hipLaunchKernelGGL((p2_chip_trace_kernel<16, 13, 1>), grid, block, 0, ctx->stream, d_trace, d_inputs, d_mult, (const uint32_t*)d_tab.u32(), n, L); break;
    }
    return rk::post_launch(ctx, "p2_chip_trace_kernel");
    RK_GUARD_END
}
int rk_air_get_steps(const rk_air* air, rk_air_step* out, size_t capacity, size_t* n_steps) {
    if (!air || !n_steps) return RK_ERR_INVALID;
    *n_steps = air->steps.size();
    if (!out || capacity < air->steps.size()) return RK_ERR_CAPACITY;
    std::memcpy(out, air->steps.data(), air->steps.size() * sizeof(rk_air_step));
    return RK_OK;
}
int rk_air_destroy(rk_air* air) {
    RK_GUARD_BEGIN
    if (!air) return RK_OK;
    (void)rk_program_destroy(air->prog);
    delete air;
    return RK_OK;
    RK_GUARD_END
}
int rk_air_get_info(const rk_air* air, rk_air_info* out) {
    if (!air || !out) return RK_ERR_INVALID;
    *out = air->info;
    return RK_OK;
}
int rk_air_compile(rk_air* air, rk_ctx* ctx) {
    RK_GUARD_BEGIN
    if (!air || !ctx) return RK_ERR_INVALID;
    return rk_program_compile(air->prog, ctx);
    RK_GUARD_END
}

}  // extern "C"
