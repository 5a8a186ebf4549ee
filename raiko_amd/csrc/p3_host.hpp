// What the uni-stark prover (p3.hip) and its host verifier (p3_verify.hip) share: the limits of a statement, the
// DuplexChallenger both run the transcript on, the checks both make on the tables, "the caller's parameter set or the
// SP1 preset", and the layout of a proof -- the one place its size is worked out.
#pragma once
#include "p3_air.hpp"

#include <algorithm>

namespace p3h {

using bb::Ext;
constexpr uint32_t MAX_TABLES = 32, MAX_QD_LOG = 4;

inline rk_params params_or_sp1(const rk_params* params) {
    rk_params def;
    rk::params_preset(&def, RK_PRESET_SP1);
    return params ? *params : def;
}

// ---------------------------------------------------------------- p3-challenger DuplexChallenger (host)
// rk_p3_fri_transcript: the challenger's calls in order, every word it observed and every field element it sampled
struct Transcript {
    std::vector<uint32_t> ops;        // (kind, count) pairs: 0 observe n words, 1 sample n field elements, 2 sample_bits(b)
    std::vector<uint32_t> observed;   // Montgomery
    std::vector<uint32_t> sampled;    // Montgomery, those behind sample_bits included
    void op(uint32_t kind, uint32_t n) { ops.push_back(kind), ops.push_back(n); }
};
struct Challenger {
    const p2::Any* k;
    uint32_t state[p2::MAX_CELLS], in[p2::MAX_CELLS], out[p2::MAX_CELLS];
    unsigned n_in = 0, n_out = 0;
    Transcript* log = nullptr;
    explicit Challenger(const p2::Any* kk) : k(kk) { std::memset(state, 0, sizeof state); }
    unsigned rate() const { return (unsigned)k->rate(); }
    void duplex() {
        for (unsigned i = 0; i < n_in; i++) state[i] = in[i];
        n_in = 0;
        k->permute(state);
        for (unsigned i = 0; i < rate(); i++) out[i] = state[i];
        n_out = rate();
    }
    void observe(uint32_t v) {
        n_out = 0;
        in[n_in++] = v;
        if (n_in == rate()) duplex();
    }
    void observe(const uint32_t* v, size_t n) {
        if (log && n) log->op(0, (uint32_t)n), log->observed.insert(log->observed.end(), v, v + n);
        for (size_t i = 0; i < n; i++) observe(v[i]);
    }
    uint32_t sample() {
        if (n_in != 0 || n_out == 0) duplex();
        if (log) log->sampled.push_back(out[n_out - 1]);
        return out[--n_out];
    }
    Ext sample_ext() {
        if (log) log->op(1, 4);
        Ext r;
        for (int i = 0; i < 4; i++) r.c[i] = sample();
        return r;
    }
    uint32_t sample_bits(unsigned bits) {
        if (log) log->op(2, bits);
        return bb::decode(sample()) & (uint32_t)(((uint64_t)1 << bits) - 1);
    }
    bool check_witness(unsigned bits, uint32_t w) {
        const uint32_t wm = bb::encode(w);
        observe(&wm, 1);
        return sample_bits(bits) == 0;
    }
};

// keyed: the caller knows the fourth batch (rk_p3_setup / rk_p3_prove_key / rk_p3_verify_key and the _key captures); every other entry point
// refuses AIRs with preprocessed columns here, before anything else happens
inline int check_tables(const rk_params& par, const rk_p3_table* tables, uint32_t n_tables, bool prover, uint32_t* lqd, bool keyed = false) {
    if (!tables || n_tables == 0 || n_tables > MAX_TABLES) return RK_ERR_INVALID;
    for (uint32_t t = 0; t < n_tables; t++) {
        const rk_p3_table& tb = tables[t];
        if (tb.air && tb.air->prep_width && !keyed) return RK_ERR_INVALID;
        if (!tb.air || tb.width != tb.air->width || tb.n_public != tb.air->n_public || (tb.n_public && !tb.public_values)) return RK_ERR_INVALID;
        for (uint32_t i = 0; i < tb.n_public; i++)
            if (tb.public_values[i] >= bb::P) return RK_ERR_INVALID;
        lqd[t] = tb.air->info.log_quotient_degree;
        if (lqd[t] > par.blowup_log2 || lqd[t] > MAX_QD_LOG) return RK_ERR_INVALID;  // the LDE must cover the quotient domain
        if (prover && (!tb.trace || tb.log_height < 1 || tb.log_height + par.blowup_log2 > ntt::LAMBDA || tb.on_device > 1)) return RK_ERR_INVALID;
    }
    return RK_OK;
}

// The words of a proof, from the blow-up, the tables' widths, permutation widths and log quotient degrees (lqd) and their
// log heights (log_n: the prover's own, or the ones the verifier read from the header):
//   head   table count, heights | trace root | [permutation root, 4 words of cumulative sum per table with lookups] |
//          quotient root | per table: local 4w, next 4w, [prep local 4c, prep next 4c], [perm local 4pw, perm next 4pw],
//          chunks 16 each | round count, 8 words of root per round, final polynomial 4, witness
//   query  trace rows, path 8 log_max | [preprocessed rows, path 8 log_kmax] | [permutation rows, path 8 log_pmax] |
//          quotient rows, path 8 log_max | per round: sibling 4, path 8 (log_max - 1 - round)
// (c = the AIR's prep_width; the preprocessed root is the key's and not in the proof)
struct Layout {
    unsigned log_max = 0, log_pmax = 0, log_kmax = 0, n_rounds = 0;
    size_t trow = 0, prow = 0, qrow = 0, krow = 0;   // words of one opened row of the trace, permutation, quotient and preprocessed batch
    size_t head_words = 0, query_words = 0;
    Layout() = default;
    Layout(unsigned blow, const rk_p3_table* t, uint32_t n, const uint32_t* lqd, const unsigned* log_n) {
        head_words = 1 + n + 16;
        for (uint32_t i = 0; i < n; i++) {
            const size_t pw = t[i].air->perm_width, cw = t[i].air->prep_width;
            head_words += 8 * (size_t)t[i].width + 8 * cw + 8 * pw + (pw ? 4 : 0) + ((size_t)16 << lqd[i]);
            log_max = std::max(log_max, log_n[i] + blow);
            if (pw) log_pmax = std::max(log_pmax, log_n[i] + blow);
            if (cw) log_kmax = std::max(log_kmax, log_n[i] + blow);
            trow += t[i].width;
            prow += pw;
            krow += cw;
            qrow += (size_t)4 << lqd[i];
        }
        n_rounds = log_max - blow;
        head_words += 1 + 8 * (size_t)n_rounds + 4 + 1 + (prow ? 8 : 0);
        query_words = trow + qrow + 16 * (size_t)log_max + (prow ? prow + 8 * (size_t)log_pmax : 0) + (krow ? krow + 8 * (size_t)log_kmax : 0);
        for (unsigned r = 0; r < n_rounds; r++) query_words += 4 + 8 * (size_t)(log_max - 1 - r);
    }
    size_t words(uint32_t queries) const { return head_words + query_words * queries; }
};

}  // namespace p3h

// rk_p3_setup's result (include/raiko_hip.h): the preprocessed batch of a statement, committed once.  Its device memory is
// the key's own (hipMalloc, not a context's pool): it outlives the context that made it.
struct rk_p3_key {
    struct Buf {   // plain device allocation released with the key
        void* p = nullptr;
        Buf() = default;
        Buf(const Buf&) = delete;
        Buf& operator=(const Buf&) = delete;
        ~Buf() {
            if (p) (void)hipFree(p);
        }
        uint32_t* u32() const { return (uint32_t*)p; }
    };
    struct Table {
        uint32_t prep_width = 0, log_height = 0;   // log_height: 0 where prep_width is
        Buf lde;    // prep_width columns of 2^(log_height + blow-up) natural-order evaluations (rk_matrix layout 2, as TableState::lde)
        Buf rows;   // the row-major matrix, kept where the table's interactions read it (the analogue of TableState::staged)
    };
    int device = 0;
    rk_params par{};                 // the parameter set the LDEs and the tree were made under (its table pointers are not kept:
    std::vector<uint32_t> p2_tab;    // the Poseidon2 constants themselves, rk::p2_chip_tab)
    std::vector<Table> tables;
    std::vector<rk_matrix> mats;     // the preprocessed matrices in table order: the batch as rk_mmcs_commit took it
    Buf nodes;
    size_t H = 0;                    // leaves of the tree = the LDE height of the tallest preprocessed table
    uint32_t root[8] = {0};
    size_t bytes = 0;
    bool has_root() const { return !mats.empty(); }
    // whether a parameter set with Poseidon2 constants p2 (rk::p2_chip_tab) is the one the LDEs and the tree were made
    // under: everything they depend on (queries and pow_bits may differ between setup and proof)
    bool same_commitment_params(const rk_params& a, const std::vector<uint32_t>& p2) const {
        return a.ext_w == par.ext_w && a.root_2_27 == par.root_2_27 && a.coset_shift == par.coset_shift && a.p2_width == par.p2_width &&
               a.p2_m4 == par.p2_m4 && a.p2_pad_free == par.p2_pad_free && a.blowup_log2 == par.blowup_log2 && p2 == p2_tab;
    }
};
