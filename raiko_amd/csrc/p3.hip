// rk_p3_prove, rk_p3_setup / rk_p3_prove_key (include/raiko_hip.h; the AIR front end rk_air_* is in p3_air.hip, the host verifier rk_p3_verify in p3_verify.hip, the
// shards in flight rk_p3_prove_shards in p3_shards.hip, what prover and verifier share in p3_host.hpp): a univariate STARK over the two-adic FRI PCS for AIRs
// handed over as data -- the proof system behind SP1's `client.setup(ELF)` / `client.prove(&pk, stdin)` (reference
// provers/sp1/driver/src/lib.rs:44-57, shard knobs docs/README_Sp1.md:19-32) as far as it exists without SP1's chips:
// Plonky3's p3-uni-stark prover.rs / verifier.rs on p3-fri's TwoAdicFriPcs with a DuplexChallenger, several tables
// under shared challenges the way sp1-core proves the chips of a shard (Plonky3@88ea2b8, reference
// Cargo.lock:4889-5127; the crates are outside the reference tree: RECALLED), with sp1-core's permutation (LogUp)
// argument between the tables (rk_air_create_lookup).  SP1's chips and its recursion VM are NOT here.
//
// Device side of one proof:
//   trace LDE      rows -> columns, iNTT (coset shift fused), expanding NTT (kernels_pcs.hip): the LDE stays the way the
//                  NTT leaves it -- column-major, natural order -- and is committed as rk_matrix layout 2 (committed row r =
//                  natural index bitrev(r)): the hashing, the opened values, the reduced openings and the quotient all walk
//                  the natural index with coalesced column loads and only WRITE at bit-reversed positions, so no pass over
//                  the data exists just to reorder it (the round-2 operator form, rk_pcs_coset_lde_rows, spends 30 % of
//                  its time transposing back to rows)
//   commitments    rk_mmcs_commit (mmcs.hip)
//   lookups        perm_entries_kernel (one lane per row: the batches' sum of +-mult / (alpha + sum beta^j x_j), extension
//                  inverses in registers) writes the permutation trace column-major; the running-sum column is four base
//                  prefix sums (psum_* kernels: workgroup totals, one carry pass, apply); the same LDE / commit as a trace
//   quotient       the AIR is translated once into an rk_program (circuit_program.hip): LOCAL / NEXT are taps of the
//                  column-major LDE (NEXT = one trace row ahead, cyclic), the three selectors are taps of three
//                  columns written by selector_kernel, the asserts one AND_EQZ chain with Horner-ordered powers of
//                  alpha; rk::program_eval_domain runs the interpreter or the hiprtc-generated kernel over the
//                  quotient domain (a sub-coset of the LDE: stride 2^(blow-up - log quotient degree)) and leaves the
//                  result split into chunks, column-major, ready for the chunks' own LDE
//   chunk LDE      iNTT, coefficient i of chunk j times w_(N qd)^(-j i) (chunk_shift_kernel), expanding NTT, to rows
//   openings       rk_pcs_eval_at_many / rk_pcs_reduce_openings, FRI commit phase rk_fri_fold_evals + rk_mmcs_commit
//   queries        every opened row and sibling digest of the proof in ONE gather launch and one download
//   preprocessed   columns fixed before any witness (rk_air_create_prep) are committed ONCE by rk_p3_setup into an rk_p3_key
//                  (p3_host.hpp): their LDE, their tree, their rows.  rk_p3_prove_key observes the key's root after the init
//                  words and reads all three in place: the LDE as the evaluator's fourth column group and in the opening
//                  round (between the traces and the permutation traces), the rows in perm_entries_kernel, the tree in
//                  the queries' gather.  rk_p3_prove is rk_p3_prove_key without a key
// The transcript (DuplexChallenger) runs on the host between those steps; the proof of work on the GPU.
#include "p3_host.hpp"
#include "p3_kernels.hpp"

#include <chrono>
#include <cstring>

namespace {

using bb::Ext;
using p3h::Challenger;
using p3h::MAX_TABLES;
using p3h::check_tables;
using rk::DevBuf;
using rk::NEXT_BACK;

// ---------------------------------------------------------------- kernels
// LagrangeSelectors on the quotient coset (p3-commit domain.rs selectors_on_coset): point i is x = shift * w_d^i;
// Z_H(x) = x^n - 1 takes d / n values.  Columns: 0 is_first_row = Z_H / (x - 1), 1 is_last_row = Z_H / (x - g^-1),
// 2 is_transition = x - g^-1.  One lane per point; the two inversions are Fermat powers (a few hundred products per
// point against the hundreds of thousands a wide AIR costs).
struct SelArgs {
    uint32_t* out;       // 3 columns of d words
    size_t d;
    unsigned log_d;
    uint32_t shiftm, g_inv;
    uint32_t zh[16];     // shift^n * w_(d/n)^r - 1
    uint32_t ratio_mask, want;   // want: bit c set = column c is read by the AIR
};
__global__ void selector_kernel(SelArgs a, ntt::Tables tb) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.d) return;
    const uint32_t x = bb::mul(a.shiftm, ntt::root_pow(tb, 0, (uint32_t)(i << (ntt::LAMBDA - a.log_d))));
    const uint32_t zh = a.zh[i & a.ratio_mask];
    if (a.want & 1u) a.out[i] = bb::mul(zh, bb::inv(bb::sub(x, bb::ONE)));
    if (a.want & 2u) a.out[a.d + i] = bb::mul(zh, bb::inv(bb::sub(x, a.g_inv)));
    if (a.want & 4u) a.out[2 * a.d + i] = bb::sub(x, a.g_inv);
}

// bit-reversed coefficients of the chunk columns (4 per chunk, n words each): coefficient i of chunk j times
// w_(n qd)^(-j i) -- Pcs::commit's `shift = generator / domain.shift` for the chunk domain shift * w^j * H_n
__global__ void chunk_shift_kernel(uint32_t* __restrict__ q, size_t n, unsigned log_n, unsigned log_nq, unsigned n_cols, ntt::Tables tb) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * n_cols) return;
    const uint32_t col = (uint32_t)(t >> log_n), p = (uint32_t)(t & (n - 1)), j = col >> 2;
    if (j == 0) return;
    const uint32_t i = bb::bitrev(p, log_n);
    const uint32_t e = (uint32_t)(((uint64_t)j * i) & (((uint64_t)1 << log_nq) - 1));
    q[t] = bb::mul(q[t], ntt::root_pow(tb, 1, e << (ntt::LAMBDA - log_nq)));
}

// out[i] += in[i] (extension elements as 4 words): the shorter reduced opening joining the folded vector
__global__ void add_words_kernel(uint32_t* __restrict__ io, const uint32_t* __restrict__ in, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) io[i] = bb::add(io[i], in[i]);
}

// ---- lookups: the permutation trace.  The lane bodies are p3_kernels.hpp's (tests/emul runs them on the CPU too)
using p3k::PERM_LD;
using p3k::PERM_ROWS;
using p3k::PermArgs;
__global__ void __launch_bounds__(PERM_ROWS) perm_entries_kernel(PermArgs a) {
    extern __shared__ uint32_t tile[];   // n_used x PERM_LD
    p3k::perm_stage(a, blockIdx.x, threadIdx.x, tile);
    __syncthreads();
    p3k::perm_row(a, blockIdx.x, threadIdx.x, tile);
}

// inclusive prefix sums of `cols` columns of n words (blockIdx.y = column), in place: workgroup totals, one carry pass
// per column, apply
constexpr int PS_TPB = 256, PS_CH = 8, PS_BLOCK = PS_TPB * PS_CH;
__device__ uint32_t psum_block_scan(uint32_t v, uint32_t* sh) {   // inclusive, across the workgroup
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < PS_TPB; d <<= 1) {
        const uint32_t o = t >= d ? sh[t - d] : 0u;
        __syncthreads();
        if (t >= d) {
            v = bb::add(o, v);
            sh[t] = v;
        }
        __syncthreads();
    }
    return v;
}
__global__ void psum_totals_kernel(uint32_t* __restrict__ totals, const uint32_t* __restrict__ io, size_t n, size_t n_blocks) {
    __shared__ uint32_t sh[PS_TPB];
    const uint32_t* col = io + (size_t)blockIdx.y * n;
    const size_t base = (size_t)blockIdx.x * PS_BLOCK;
    uint32_t acc = 0;
    for (int j = 0; j < PS_CH; j++) {   // lane t takes elements t, t + 256, ...: coalesced; only the sum matters here
        const size_t i = base + (size_t)j * PS_TPB + threadIdx.x;
        if (i < n) acc = bb::add(acc, col[i]);
    }
    acc = psum_block_scan(acc, sh);
    if (threadIdx.x == PS_TPB - 1) totals[(size_t)blockIdx.y * n_blocks + blockIdx.x] = acc;
}
__global__ void psum_carry_kernel(uint32_t* totals, size_t n_blocks) {   // totals[b] <- sum of the blocks before b
    __shared__ uint32_t sh[PS_TPB];
    uint32_t* t = totals + (size_t)blockIdx.x * n_blocks;
    const size_t per = (n_blocks + PS_TPB - 1) / PS_TPB;
    const size_t lo0 = (size_t)threadIdx.x * per, lo = lo0 < n_blocks ? lo0 : n_blocks, hi = lo + per < n_blocks ? lo + per : n_blocks;
    uint32_t acc = 0;
    for (size_t i = lo; i < hi; i++) acc = bb::add(acc, t[i]);
    const uint32_t incl = psum_block_scan(acc, sh);
    uint32_t run = bb::sub(incl, acc);
    for (size_t i = lo; i < hi; i++) {
        const uint32_t v = t[i];
        t[i] = run;
        run = bb::add(run, v);
    }
}
__global__ void psum_apply_kernel(uint32_t* __restrict__ io, const uint32_t* __restrict__ totals, size_t n, size_t n_blocks) {
    __shared__ uint32_t sh[PS_TPB];
    uint32_t* col = io + (size_t)blockIdx.y * n;
    const size_t base = (size_t)blockIdx.x * PS_BLOCK + (size_t)threadIdx.x * PS_CH;   // lane t: 8 consecutive words (two 16 B loads)
    uint32_t v[PS_CH];
    uint32_t acc = 0;
#pragma unroll
    for (int j = 0; j < PS_CH; j++) {
        v[j] = base + j < n ? col[base + j] : 0u;
        acc = bb::add(acc, v[j]);
        v[j] = acc;
    }
    const uint32_t incl = psum_block_scan(acc, sh);
    const uint32_t carry = bb::add(bb::sub(incl, acc), totals[(size_t)blockIdx.y * n_blocks + blockIdx.x]);
#pragma unroll
    for (int j = 0; j < PS_CH; j++)
        if (base + j < n) col[base + j] = bb::add(v[j], carry);
}

// every opened row / digest of a proof's query phase: job = (source address, words, destination offset); one
// 64-lane group per job
struct GatherJob {
    uint64_t src;
    uint64_t stride;     // in words: 1 for a digest or a row of a row-major matrix, the column length for a row of a column-major one
    uint32_t words, dst;
};
__global__ void gather_jobs_kernel(uint32_t* __restrict__ dst, const GatherJob* __restrict__ jobs, size_t n_jobs) {
    const size_t j = (size_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    if (j >= n_jobs) return;
    const GatherJob jb = jobs[j];
    const uint32_t* s = reinterpret_cast<const uint32_t*>(jb.src);
    for (uint32_t w = threadIdx.x & 63; w < jb.words; w += 64) dst[jb.dst + w] = s[(size_t)w * jb.stride];
}

// ---------------------------------------------------------------- prover state

struct TableState {
    unsigned k = 0, lqd = 0;      // log2 rows, log2 quotient degree
    size_t n = 0, H = 0, w = 0;
    DevBuf lde;                   // w columns of H natural-order evaluations (rk_matrix layout 2: committed row r at index bitrev(r))
    DevBuf chunks;                // 4 qd columns of H: the qd chunk LDEs side by side (as one matrix they hash, open and
                                  // reduce exactly like qd matrices of width 4 that follow each other in the batch)
    std::vector<uint32_t> y;      // opened values: local 4w | next 4w | [prep local 4cw | prep next 4cw] | [perm local 4pw | perm next 4pw] | chunks 16 each
    size_t pw = 0;                // base columns of the permutation trace (0: the table has no lookups)
    size_t cw = 0;                // preprocessed columns (0: none); their LDE and rows are the key's, read in place
    const uint32_t* prep_lde = nullptr;    // cw columns of H, laid out like lde
    const uint32_t* prep_rows = nullptr;   // row-major n x cw, there when the interactions read it
    DevBuf staged;                // a host trace's copy in HBM, kept for the permutation trace
    const uint32_t* d_trace = nullptr;
    DevBuf perm;                  // pw columns of H, laid out like lde
    uint32_t cumsum[4] = {0, 0, 0, 0};
};

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// the exact size of the proof rk_p3_prove writes for these tables
size_t proof_bound(const rk_params& p, const rk_p3_table* t, uint32_t n, const uint32_t* lqd) {
    unsigned log_n[MAX_TABLES];
    for (uint32_t i = 0; i < n; i++) log_n[i] = t[i].log_height;
    return p3h::Layout(p.blowup_log2, t, n, lqd, log_n).words(p.queries);
}

// One rk_p3_prove: the state the stages share and the stages in the order the transcript imposes
struct ProofRun {
    rk_ctx* ctx;
    const rk_p3_table* tables;
    uint32_t n_tables;
    const rk_p3_key* key = nullptr;      // the preprocessed batch (rk_p3_prove_key), committed at setup
    rk_params par;
    unsigned blow = 0;
    uint32_t lqd[MAX_TABLES];
    rk_p3_timing& tm;
    double t_mark = 0;
    std::vector<uint32_t> pf;            // the proof words before the query openings
    Challenger ch;
    std::vector<TableState> ts;
    std::vector<rk_matrix> tmats, pmats, qmats;   // the three input batches: traces, permutation traces, quotient chunks
    DevBuf tnodes, pnodes, qnodes;
    size_t Ht = 0, Hp = 0, Hq = 0;
    unsigned log_max = 0, n_rounds = 0;
    std::vector<uint32_t> pchal;         // lookups: [alpha | beta^0 | .. | beta^K], every table reads a prefix
    uint32_t root[8];
    Ext zeta;
    DevBuf ro[ntt::LAMBDA + 1];          // reduced openings per LDE height
    struct Layer {
        DevBuf values, nodes;            // 2^(log_max - round) extension elements; the tree over their pairs
    };
    std::vector<Layer> layers;

    ProofRun(rk_ctx* c, const rk_p3_table* t, uint32_t n) : ctx(c), tables(t), n_tables(n), tm(c->p3_timing), ch(&c->h_p2) {}
    void lap(float& slot) {
        (void)hipStreamSynchronize(ctx->stream);
        const double t = now_ms();
        slot += (float)(t - t_mark);
        t_mark = t;
    }
    void push(const uint32_t* w, size_t n) { pf.insert(pf.end(), w, w + n); }

    int commit_traces();
    int permutation_traces();
    int quotients(const Ext& alpha);
    int open();
    int fri();
    int queries(uint32_t* h_proof, size_t capacity, size_t* proof_words);
};

int ProofRun::commit_traces() {
    // ---- trace LDEs and their commitment
    ts = std::vector<TableState>(n_tables);
    tmats.resize(n_tables);
    pf.push_back(n_tables);
    for (uint32_t t = 0; t < n_tables; t++) {
        const rk_p3_table& tb = tables[t];
        TableState& s = ts[t];
        s.k = tb.log_height;
        s.lqd = lqd[t];
        s.n = (size_t)1 << s.k;
        s.H = s.n << blow;
        s.w = tb.width;
        pf.push_back(tb.log_height);
        s.pw = tb.air->perm_width;
        s.cw = tb.air->prep_width;
        if (s.cw) {
            s.prep_lde = key->tables[t].lde.u32();
            s.prep_rows = key->tables[t].rows.u32();
        }
        s.d_trace = tb.trace;
        if (!tb.on_device) {
            RK_TRY(s.staged.alloc(ctx, s.n * s.w * 4));
            RK_HIP_TRY(ctx, hipMemcpyAsync(s.staged.p, tb.trace, s.n * s.w * 4, hipMemcpyHostToDevice, ctx->stream));
            s.d_trace = s.staged.u32();
        }
        RK_TRY(s.lde.alloc(ctx, s.H * s.w * 4));
        RK_TRY(rk::pcs_coset_lde_cols(ctx, s.lde.u32(), s.d_trace, s.n, s.w));
        if (!tb.on_device) RK_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the caller's host buffer is free again
        if (!s.pw) s.staged.release();   // only the lookups read the rows again
        tmats[t] = rk_matrix{s.lde.u32(), (uint32_t)s.H, (uint32_t)s.w, 2};
        Ht = std::max(Ht, s.H);
        log_max = std::max(log_max, s.k + blow);
    }
    lap(tm.lde);
    RK_TRY(tnodes.alloc(ctx, 2 * Ht * p2::OUT * 4));
    RK_TRY(rk_mmcs_commit(ctx, tmats.data(), n_tables, tnodes.u32(), root));
    push(root, 8);
    ch.observe(root, 8);
    for (uint32_t t = 0; t < n_tables; t++) ch.observe(tables[t].public_values, tables[t].n_public);
    lap(tm.commit);

    return RK_OK;
}

int ProofRun::permutation_traces() {
    // ---- lookups: permutation traces, their LDE and commitment (nothing of this without interactions)
    {
        uint32_t n_chal = 0;
        for (uint32_t t = 0; t < n_tables; t++) n_chal = std::max(n_chal, tables[t].air->n_chal);
        if (n_chal) {
            const Ext pa = ch.sample_ext(), pb = ch.sample_ext();
            pchal.resize(n_chal);
            std::memcpy(pchal.data(), pa.c, 16);
            Ext cur = bb::ext_one();
            for (uint32_t j = 1; 4 * j < n_chal; j++) {
                std::memcpy(&pchal[4 * j], cur.c, 16);
                cur = bb::mul(cur, pb, ctx->sys.wm);
            }
        }
        for (uint32_t t = 0; t < n_tables && n_chal; t++) {
            TableState& s = ts[t];
            if (!s.pw) continue;
            const rk_air& air = *tables[t].air;
            std::vector<uint32_t> desc(pchal.begin(), pchal.begin() + air.n_chal);
            desc.insert(desc.end(), air.lookups.begin(), air.lookups.end());
            const uint32_t desc_words = (uint32_t)desc.size();
            desc.insert(desc.end(), air.used.begin(), air.used.end());
            DevBuf d_desc, cols, totals;
            RK_TRY(d_desc.alloc(ctx, desc.size() * 4));
            RK_TRY(rk::upload(ctx, d_desc.p, desc.data(), desc.size() * 4));
            RK_TRY(cols.alloc(ctx, s.n * s.pw * 4));
            PermArgs a{cols.u32(), s.d_trace, d_desc.u32(), s.n, s.w, air.n_chal, air.n_lookups, ctx->sys.wm, (uint32_t)air.used.size(), desc_words,
                       air.perm_reads_prep ? s.prep_rows : nullptr, s.cw};
            const size_t lds = std::max<size_t>(air.used.size(), 1) * PERM_LD * 4;
            if (lds > 64 * 1024)
                RK_HIP_TRY(ctx, hipFuncSetAttribute((const void*)perm_entries_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(perm_entries_kernel, dim3((unsigned)((s.n + PERM_ROWS - 1) / PERM_ROWS)), dim3(PERM_ROWS), lds, ctx->stream, a);
            RK_TRY(rk::post_launch(ctx, "perm_entries_kernel"));
            s.staged.release();
            // the running sum: four base prefix sums over the row totals, in place
            const size_t nblk = (s.n + PS_BLOCK - 1) / PS_BLOCK;
            uint32_t* phi = cols.u32() + (s.pw - 4) * s.n;
            RK_TRY(totals.alloc(ctx, 4 * nblk * 4));
            hipLaunchKernelGGL(psum_totals_kernel, dim3((unsigned)nblk, 4), dim3(PS_TPB), 0, ctx->stream, totals.u32(), (const uint32_t*)phi, s.n, nblk);
            RK_TRY(rk::post_launch(ctx, "psum_totals_kernel"));
            hipLaunchKernelGGL(psum_carry_kernel, dim3(4), dim3(PS_TPB), 0, ctx->stream, totals.u32(), nblk);
            RK_TRY(rk::post_launch(ctx, "psum_carry_kernel"));
            hipLaunchKernelGGL(psum_apply_kernel, dim3((unsigned)nblk, 4), dim3(PS_TPB), 0, ctx->stream, phi, (const uint32_t*)totals.u32(), s.n, nblk);
            RK_TRY(rk::post_launch(ctx, "psum_apply_kernel"));
            for (int k = 0; k < 4; k++)
                RK_HIP_TRY(ctx, hipMemcpyAsync(&s.cumsum[k], phi + (size_t)k * s.n + (s.n - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
            // the same LDE as a trace's, from columns
            RK_TRY(rk::ntt_reverse(ctx, cols.u32(), s.n, s.pw, /*fuse_zk_shift=*/true));
            RK_TRY(s.perm.alloc(ctx, s.H * s.pw * 4));
            RK_TRY(rk::ntt_forward(ctx, s.perm.u32(), cols.u32(), s.n, s.pw, blow));
            pmats.push_back(rk_matrix{s.perm.u32(), (uint32_t)s.H, (uint32_t)s.pw, 2});
            Hp = std::max(Hp, s.H);
        }
        if (!pmats.empty()) {
            lap(tm.perm);
            RK_TRY(pnodes.alloc(ctx, 2 * Hp * p2::OUT * 4));
            RK_TRY(rk_mmcs_commit(ctx, pmats.data(), (uint32_t)pmats.size(), pnodes.u32(), root));
            RK_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the cumulative sums have landed
            push(root, 8);
            ch.observe(root, 8);
            for (const TableState& s : ts)
                if (s.pw) {
                    push(s.cumsum, 4);
                    ch.observe(s.cumsum, 4);
                }
            lap(tm.commit);
        }
    }
    return RK_OK;
}

int ProofRun::quotients(const Ext& alpha) {
    // ---- quotients
    for (uint32_t t = 0; t < n_tables; t++) {
        const rk_p3_table& tb = tables[t];
        TableState& s = ts[t];
        const unsigned kq = s.k + s.lqd;
        const size_t qd = (size_t)1 << s.lqd, d = s.n << s.lqd, n_qcols = 4 * qd;
        rk_program* pg = tb.air->prog;
        DevBuf sel, q;
        if (pg->group_min[0]) {
            RK_TRY(sel.alloc(ctx, 3 * d * 4));
            SelArgs a{};
            a.out = sel.u32();
            a.d = d;
            a.log_d = kq;
            a.shiftm = ctx->sys.shiftm;
            a.g_inv = bb::inv(bb::pow(ctx->sys.root27m, (uint64_t)1 << (27 - s.k)));
            const uint32_t sn = bb::pow(ctx->sys.shiftm, s.n), wr = bb::pow(ctx->sys.root27m, (uint64_t)1 << (27 - s.lqd));
            for (unsigned r = 0; r < qd; r++) a.zh[r] = bb::sub(bb::mul(sn, bb::pow(wr, r)), bb::ONE);
            a.ratio_mask = (uint32_t)qd - 1;
            a.want = tb.air->sel_mask;
            hipLaunchKernelGGL(selector_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, ctx->stream, a, ctx->tb);
            RK_TRY(rk::post_launch(ctx, "selector_kernel"));
        }
        RK_TRY(q.alloc(ctx, n_qcols * s.n * 4));
        rk::EvalDomain dom;
        dom.ctx = ctx;
        dom.po2 = s.k;
        dom.ratio_log2 = dom.split_log2 = s.lqd;
        dom.d_cols[0] = sel.u32();
        dom.group_size[0] = 3;
        dom.col_len[0] = d;
        dom.d_cols[2] = s.lde.u32();
        dom.group_size[2] = (uint32_t)s.w;
        dom.col_len[2] = s.H;
        dom.stride_log2[2] = blow - s.lqd;
        if (s.cw) {   // the key's LDE where it lies: a column group of its own
            dom.d_cols[3] = s.prep_lde;
            dom.group_size[3] = (uint32_t)s.cw;
            dom.col_len[3] = s.H;
            dom.stride_log2[3] = blow - s.lqd;
        }
        dom.globals = tb.public_values;
        dom.n_globals = tb.n_public;
        std::vector<uint32_t> globals;   // lookups: public values | challenges | cumulative sum
        if (s.pw) {
            dom.d_cols[1] = s.perm.u32();
            dom.group_size[1] = (uint32_t)s.pw;
            dom.col_len[1] = s.H;
            dom.stride_log2[1] = blow - s.lqd;
            globals.assign(tb.public_values, tb.public_values + tb.n_public);
            globals.insert(globals.end(), pchal.begin(), pchal.begin() + tb.air->n_chal);
            globals.insert(globals.end(), s.cumsum, s.cumsum + 4);
            dom.globals = globals.data();
            dom.n_globals = (uint32_t)globals.size();
        }
        RK_TRY(rk::program_eval_domain(pg, dom, alpha.c, q.u32()));
        sel.release();
        // the chunks' own LDE: interpolate over H_n, move to the chunk's coset, evaluate on the LDE coset
        RK_TRY(rk::ntt_reverse(ctx, q.u32(), s.n, n_qcols, /*fuse_zk_shift=*/false));
        if (qd > 1) {
            const size_t tot = s.n * n_qcols;
            hipLaunchKernelGGL(chunk_shift_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, q.u32(), s.n, s.k, kq,
                               (unsigned)n_qcols, ctx->tb);
            RK_TRY(rk::post_launch(ctx, "chunk_shift_kernel"));
        }
        RK_TRY(s.chunks.alloc(ctx, n_qcols * s.H * 4));
        RK_TRY(rk::ntt_forward(ctx, s.chunks.u32(), q.u32(), s.n, n_qcols, blow));
        qmats.push_back(rk_matrix{s.chunks.u32(), (uint32_t)s.H, (uint32_t)n_qcols, 2});
        Hq = std::max(Hq, s.H);
    }
    lap(tm.quotient);
    RK_TRY(qnodes.alloc(ctx, 2 * Hq * p2::OUT * 4));
    RK_TRY(rk_mmcs_commit(ctx, qmats.data(), (uint32_t)qmats.size(), qnodes.u32(), root));
    push(root, 8);
    ch.observe(root, 8);
    zeta = ch.sample_ext();
    lap(tm.commit);

    return RK_OK;
}

int ProofRun::open() {
    // ---- PCS open: opened values and reduced openings
    const Ext alpha2 = ch.sample_ext();
    uint64_t num_reduced[ntt::LAMBDA + 1] = {0};
    // every opened value first (no host round trip between the launches), ONE download, then the reduced openings, which
    // need the opened values on the host: a shard of a dozen tables waits once instead of three dozen times
    struct Opening {
        TableState* s;
        const uint32_t* mat;
        size_t w, n_points, y_at, d_at;   // y_at: words into s->y; d_at: words into the device buffer
    };
    std::vector<Opening> openings;
    size_t y_words = 0;
    for (TableState& s : ts) s.y.resize(8 * s.w + 8 * s.cw + 8 * s.pw + ((size_t)16 << s.lqd));
    auto add_opening = [&](TableState& s, const uint32_t* mat, size_t w, size_t n_points, size_t y_at) {
        openings.push_back(Opening{&s, mat, w, n_points, y_at, y_words});
        y_words += 4 * w * n_points;
    };
    for (TableState& s : ts) add_opening(s, s.lde.u32(), s.w, 2, 0);                       // round 0: every trace at zeta and zeta * g
    for (TableState& s : ts)
        if (s.cw) add_opening(s, s.prep_lde, s.cw, 2, 8 * s.w);                            // the preprocessed batch (the key's), likewise
    for (TableState& s : ts)
        if (s.pw) add_opening(s, s.perm.u32(), s.pw, 2, 8 * s.w + 8 * s.cw);               // (lookups): the permutation traces, likewise
    for (TableState& s : ts) add_opening(s, s.chunks.u32(), (size_t)4 << s.lqd, 1, 8 * s.w + 8 * s.cw + 8 * s.pw);   // last round: every quotient chunk at zeta
    DevBuf d_ys;
    RK_TRY(d_ys.alloc(ctx, y_words * 4));
    auto points_of = [&](const TableState& s, uint32_t pts[8]) {
        std::memcpy(pts, zeta.c, 16);
        const Ext zn = bb::scale(zeta, bb::pow(ctx->sys.root27m, (uint64_t)1 << (27 - s.k)));
        std::memcpy(pts + 4, zn.c, 16);
    };
    for (const Opening& o : openings) {
        uint32_t pts[8];
        points_of(*o.s, pts);
        RK_TRY(rk::pcs_eval_at(ctx, d_ys.u32() + o.d_at, o.mat, o.s->H, o.w, pts, o.n_points, /*cols=*/true));
    }
    {
        std::vector<uint32_t> h_ys(y_words);
        RK_TRY(rk::d2h_sync(ctx, h_ys.data(), d_ys.p, y_words * 4));
        for (const Opening& o : openings) std::memcpy(o.s->y.data() + o.y_at, &h_ys[o.d_at], 4 * o.w * o.n_points * 4);
    }
    for (const Opening& o : openings) {
        TableState& s = *o.s;
        const unsigned lh = s.k + blow;
        if (!ro[lh].p) {
            RK_TRY(ro[lh].alloc(ctx, s.H * 16));
            RK_HIP_TRY(ctx, hipMemsetAsync(ro[lh].p, 0, s.H * 16, ctx->stream));
        }
        uint32_t pts[8];
        points_of(s, pts);
        RK_TRY(rk::pcs_reduce_openings(ctx, ro[lh].u32(), o.mat, s.H, o.w, o.n_points, pts, s.y.data() + o.y_at, alpha2, num_reduced[lh], /*cols=*/true));
        num_reduced[lh] += o.n_points * o.w;
    }
    for (const TableState& s : ts) push(s.y.data(), s.y.size());
    lap(tm.open);

    return RK_OK;
}

int ProofRun::fri() {
    // ---- FRI commit phase
    n_rounds = log_max - blow;
    layers = std::vector<Layer>(n_rounds);
    DevBuf folded = std::move(ro[log_max]);
    size_t len = (size_t)1 << log_max;
    pf.push_back(n_rounds);
    for (unsigned rd = 0; rd < n_rounds; rd++) {
        Layer& L = layers[rd];
        RK_TRY(L.nodes.alloc(ctx, len * p2::OUT * 4));   // 2 * (len / 2) digests
        const rk_matrix lm{folded.u32(), (uint32_t)(len / 2), 8, 1};
        RK_TRY(rk_mmcs_commit(ctx, &lm, 1, L.nodes.u32(), root));
        push(root, 8);
        ch.observe(root, 8);
        const Ext beta = ch.sample_ext();
        DevBuf nxt;
        RK_TRY(nxt.alloc(ctx, len / 2 * 16));
        RK_TRY(rk::fri_fold_evals(ctx, nxt.u32(), folded.u32(), len / 2, beta));
        L.values = std::move(folded);
        folded = std::move(nxt);
        len /= 2;
        const unsigned lg = log2u(len);
        if (lg != log_max && ro[lg].p) {
            hipLaunchKernelGGL(add_words_kernel, dim3((unsigned)((len * 4 + 255) / 256)), dim3(256), 0, ctx->stream, folded.u32(),
                               (const uint32_t*)ro[lg].u32(), len * 4);
            RK_TRY(rk::post_launch(ctx, "add_words_kernel"));
        }
    }
    std::vector<uint32_t> fin(len * 4);
    RK_TRY(rk::d2h_sync(ctx, fin.data(), folded.p, len * 16));
    for (size_t i = 1; i < len; i++)
        if (std::memcmp(&fin[4 * i], &fin[0], 16) != 0) return RK_ERR_INTERNAL;   // `blowup` values of a constant
    push(fin.data(), 4);
    ch.observe(fin.data(), 4);
    uint32_t witness = 0;
    if (par.pow_bits) RK_TRY(rk::duplex_grind(ctx, ch.state, ch.in, ch.n_in, par.pow_bits, &witness));
    if (!ch.check_witness(par.pow_bits, witness)) return RK_ERR_INTERNAL;
    pf.push_back(witness);
    lap(tm.fri);

    return RK_OK;
}

int ProofRun::queries(uint32_t* h_proof, size_t capacity, size_t* proof_words) {
    // ---- queries: all indices first (they depend on the transcript only), then one gather
    std::vector<GatherJob> jobs;
    uint32_t at = 0;
    auto job = [&](const uint32_t* src, uint32_t words, uint64_t stride = 1) {
        jobs.push_back(GatherJob{(uint64_t)(uintptr_t)src, stride, words, at});
        at += words;
    };
    auto open_batch = [&](const std::vector<rk_matrix>& mats, const uint32_t* nodes, size_t H, uint32_t index) {
        for (const rk_matrix& m : mats) {   // layout 2: committed row r of a column-major matrix sits at index bitrev(r) of every column
            const uint32_t r = (uint32_t)(index / (H / m.height));
            job(m.d_values + bb::bitrev(r, log2u(m.height)), m.width, m.height);
        }
        for (size_t idx = H + index; idx > 1; idx >>= 1) job(nodes + (idx ^ 1) * p2::OUT, p2::OUT);
    };
    for (uint32_t qi = 0; qi < par.queries; qi++) {
        const uint32_t index = ch.sample_bits(log_max);
        open_batch(tmats, tnodes.u32(), Ht, index >> (log_max - log2u(Ht)));
        if (key && key->has_root()) open_batch(key->mats, key->nodes.u32(), key->H, index >> (log_max - log2u(key->H)));
        if (!pmats.empty()) open_batch(pmats, pnodes.u32(), Hp, index >> (log_max - log2u(Hp)));
        open_batch(qmats, qnodes.u32(), Hq, index >> (log_max - log2u(Hq)));
        for (unsigned rd = 0; rd < n_rounds; rd++) {
            const uint32_t idx = index >> rd, pair = idx >> 1;
            const size_t height = ((size_t)1 << (log_max - rd)) / 2;
            job(layers[rd].values.u32() + (2 * (size_t)pair + ((idx ^ 1) & 1)) * 4, 4);
            for (size_t a = height + pair; a > 1; a >>= 1) job(layers[rd].nodes.u32() + (a ^ 1) * p2::OUT, p2::OUT);
        }
    }
    if (pf.size() + at > capacity) return RK_ERR_INTERNAL;  // the bound is exact: cannot happen
    {
        DevBuf d_jobs, d_out;
        RK_TRY(d_jobs.alloc(ctx, jobs.size() * sizeof(GatherJob)));
        RK_TRY(d_out.alloc(ctx, (size_t)at * 4 + 16));
        RK_HIP_TRY(ctx, hipMemcpyAsync(d_jobs.p, jobs.data(), jobs.size() * sizeof(GatherJob), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(gather_jobs_kernel, dim3((unsigned)((jobs.size() + 3) / 4)), dim3(256), 0, ctx->stream, d_out.u32(),
                           (const GatherJob*)d_jobs.p, jobs.size());
        RK_TRY(rk::post_launch(ctx, "gather_jobs_kernel"));
        std::memcpy(h_proof, pf.data(), pf.size() * 4);
        RK_TRY(rk::d2h_sync(ctx, h_proof + pf.size(), d_out.p, (size_t)at * 4));
    }
    *proof_words = pf.size() + at;
    return RK_OK;
}

// the key against the context and the tables: all of it before anything is launched
int check_key(rk_ctx* ctx, const rk_params& par, const rk_p3_key& key, const rk_p3_table* tables, uint32_t n_tables) {
    if (key.device != ctx->device || !key.same_commitment_params(par, rk::p2_chip_tab(ctx->h_p2)) || key.tables.size() != n_tables) return RK_ERR_INVALID;
    for (uint32_t t = 0; t < n_tables; t++) {
        const rk_p3_key::Table& kt = key.tables[t];
        if (kt.prep_width != tables[t].air->prep_width) return RK_ERR_INVALID;
        if (kt.prep_width && kt.log_height != tables[t].log_height) return RK_ERR_INVALID;
        if (tables[t].air->perm_reads_prep && !kt.rows.p) return RK_ERR_INVALID;
    }
    return RK_OK;
}

int p3_prove(rk_ctx* ctx, const rk_p3_key* key, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init, size_t n_init,
             uint32_t* h_proof, size_t capacity, size_t* proof_words) {
    ProofRun run(ctx, tables, n_tables);
    run.key = key;
    RK_TRY(rk_get_params(ctx, &run.par));
    RK_TRY(check_tables(run.par, tables, n_tables, true, run.lqd, /*keyed=*/key != nullptr));
    if (key) RK_TRY(check_key(ctx, run.par, *key, tables, n_tables));
    for (size_t i = 0; i < n_init; i++)
        if (init[i] >= bb::P) return RK_ERR_INVALID;
    const size_t bound = proof_bound(run.par, tables, n_tables, run.lqd);
    if (capacity < bound) {
        *proof_words = bound;
        return RK_ERR_CAPACITY;
    }
    run.blow = run.par.blowup_log2;
    run.tm = rk_p3_timing{};
    const double t_start = now_ms();
    run.t_mark = t_start;
    run.pf.reserve(bound);
    run.ch.observe(init, n_init);
    if (key && key->has_root()) run.ch.observe(key->root, 8);   // the verifying key binds the statement before any witness
    RK_TRY(run.commit_traces());
    RK_TRY(run.permutation_traces());     // nothing of it without interactions
    const Ext alpha = run.ch.sample_ext();
    RK_TRY(run.quotients(alpha));
    RK_TRY(run.open());
    RK_TRY(run.fri());
    RK_TRY(run.queries(h_proof, capacity, proof_words));
    run.lap(run.tm.query);
    run.tm.total = (float)(now_ms() - t_start);
    return RK_OK;
}

size_t bound_words(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, bool keyed) {
    const rk_params par = p3h::params_or_sp1(params);
    rk::Sys sys;
    auto k = std::make_unique<p2::Any>();
    if (rk::resolve_params(&par, &sys, k.get()) != RK_OK) return 0;
    uint32_t lqd[MAX_TABLES];
    if (check_tables(par, tables, n_tables, false, lqd, keyed) != RK_OK) return 0;
    for (uint32_t t = 0; t < n_tables; t++)
        if (tables[t].log_height < 1 || tables[t].log_height + par.blowup_log2 > ntt::LAMBDA) return 0;
    return proof_bound(par, tables, n_tables, lqd);
}

// rk_p3_setup: the preprocessed matrices' LDEs and their commitment, once.  The same two calls a proof spends on its
// trace (pcs_coset_lde_cols, rk_mmcs_commit), off the per-proof path.
int key_alloc(rk_ctx* ctx, rk_p3_key& key, rk_p3_key::Buf& b, size_t bytes) {
    RK_HIP_TRY(ctx, hipMalloc(&b.p, bytes));
    key.bytes += bytes;
    return RK_OK;
}
int p3_setup(rk_ctx* ctx, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* const* prep_traces, rk_p3_key** out) {
    std::unique_ptr<rk_p3_key> key(new rk_p3_key);
    RK_TRY(rk_get_params(ctx, &key->par));
    key->par.p2_rc_ext = key->par.p2_rc_int = key->par.p2_diag = nullptr;   // the context's own storage
    key->p2_tab = rk::p2_chip_tab(ctx->h_p2);
    uint32_t lqd[MAX_TABLES];
    RK_TRY(check_tables(key->par, tables, n_tables, false, lqd, /*keyed=*/true));
    const unsigned blow = key->par.blowup_log2;
    for (uint32_t t = 0; t < n_tables; t++) {
        if (!tables[t].air->prep_width) continue;
        if (!prep_traces || !prep_traces[t] || tables[t].log_height < 1 || tables[t].log_height + blow > ntt::LAMBDA || tables[t].on_device > 1)
            return RK_ERR_INVALID;
    }
    key->device = ctx->device;
    key->tables = std::vector<rk_p3_key::Table>(n_tables);
    for (uint32_t t = 0; t < n_tables; t++) {
        const rk_air& air = *tables[t].air;
        if (!air.prep_width) continue;
        rk_p3_key::Table& kt = key->tables[t];
        kt.prep_width = air.prep_width;
        kt.log_height = tables[t].log_height;
        const size_t n = (size_t)1 << kt.log_height, H = n << blow, cw = kt.prep_width;
        const uint32_t* d_rows = prep_traces[t];
        DevBuf staged;
        if (!tables[t].on_device || air.perm_reads_prep) {   // rows the key keeps, or a host matrix on its way through HBM
            void* dst = nullptr;
            if (air.perm_reads_prep) {
                RK_TRY(key_alloc(ctx, *key, kt.rows, n * cw * 4));
                dst = kt.rows.p;
            } else {
                RK_TRY(staged.alloc(ctx, n * cw * 4));
                dst = staged.p;
            }
            RK_HIP_TRY(ctx, hipMemcpyAsync(dst, prep_traces[t], n * cw * 4, tables[t].on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
            d_rows = (const uint32_t*)dst;
        }
        RK_TRY(key_alloc(ctx, *key, kt.lde, H * cw * 4));
        RK_TRY(rk::pcs_coset_lde_cols(ctx, kt.lde.u32(), d_rows, n, cw));
        RK_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the caller's matrix and the staging block are free again
        key->mats.push_back(rk_matrix{kt.lde.u32(), (uint32_t)H, (uint32_t)cw, 2});
        key->H = std::max(key->H, H);
    }
    if (key->has_root()) {
        RK_TRY(key_alloc(ctx, *key, key->nodes, 2 * key->H * p2::OUT * 4));
        RK_TRY(rk_mmcs_commit(ctx, key->mats.data(), (uint32_t)key->mats.size(), key->nodes.u32(), key->root));
        RK_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    *out = key.release();
    return RK_OK;
}

}  // namespace

extern "C" {

size_t rk_p3_proof_bound_words(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables) {
    return bound_words(params, tables, n_tables, /*keyed=*/false);
}
size_t rk_p3_proof_bound_words_key(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables) {
    return bound_words(params, tables, n_tables, /*keyed=*/true);
}

int rk_p3_prove(rk_ctx* ctx, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init_words, size_t n_init, uint32_t* h_proof,
                size_t capacity_words, size_t* proof_words) {
    return rk_p3_prove_key(ctx, nullptr, tables, n_tables, init_words, n_init, h_proof, capacity_words, proof_words);
}
int rk_p3_prove_key(rk_ctx* ctx, const rk_p3_key* key, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init_words, size_t n_init,
                    uint32_t* h_proof, size_t capacity_words, size_t* proof_words) {
    RK_GUARD_BEGIN
    if (!ctx || !h_proof || !proof_words || (n_init && !init_words)) return RK_ERR_INVALID;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = p3_prove(ctx, key, tables, n_tables, init_words, n_init, h_proof, capacity_words, proof_words);
    if (rc != RK_OK) (void)hipStreamSynchronize(ctx->stream);   // scoped buffers are back in the pool: nothing may still read them
    return rc;
    RK_GUARD_END
}

int rk_p3_setup(rk_ctx* ctx, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* const* prep_traces, rk_p3_key** out) {
    RK_GUARD_BEGIN
    if (!out) return RK_ERR_INVALID;
    *out = nullptr;
    if (!ctx) return RK_ERR_INVALID;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = p3_setup(ctx, tables, n_tables, prep_traces, out);
    if (rc != RK_OK) (void)hipStreamSynchronize(ctx->stream);
    return rc;
    RK_GUARD_END
}
int rk_p3_key_root(const rk_p3_key* key, uint32_t out[8]) {
    if (!key || !out || !key->has_root()) return RK_ERR_INVALID;
    std::memcpy(out, key->root, 32);
    return RK_OK;
}
size_t rk_p3_key_bytes(const rk_p3_key* key) { return key ? key->bytes : 0; }
int rk_p3_key_destroy(rk_p3_key* key) {
    RK_GUARD_BEGIN
    if (!key) return RK_OK;
    (void)hipSetDevice(key->device);
    delete key;
    return RK_OK;
    RK_GUARD_END
}

int rk_p3_last_timing(rk_ctx* ctx, rk_p3_timing* out) {
    if (!ctx || !out) return RK_ERR_INVALID;
    *out = ctx->p3_timing;
    return RK_OK;
}

}  // extern "C"
