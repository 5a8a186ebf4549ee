// rk_p3_verify and what rides on it (include/raiko_hip.h): the host verifier of the uni-stark proofs p3.hip writes --
// Plonky3's p3-uni-stark verifier.rs on p3-fri's TwoAdicFriPcs with a DuplexChallenger, several tables under shared
// challenges, sp1-core's permutation argument between them -- and the calls that hand out what one run of it read:
// rk_p3_verify_hashes (every Poseidon2 permutation) and the four rk_p3_fri_* captures the FRI lookup tables are written
// from (fri_tables.hip), each with a _key twin for proofs under a verifying key.  Host code only.
//
// The check runs in stages over one parsed view of the proof (Opened), each doing its own reads, in the order that fixes
// which defect a proof with several is refused for:
//   open_statement     parameters, tables, canonical words; header and heights, roots, the lookups' challenges and
//                      cumulative sums, alpha, zeta, the opened values
//   check_constraints  the quotient recombined from its chunks against the AIR folded at zeta, per table
//   open_fri           commit-phase roots and betas, final polynomial, proof of work, total length, query indices
//   check_query        one query: the input openings (three batches, four with preprocessed columns), the reduced
//                      openings, the fold rounds
// Verdicts: 0 accept; 1 malformed / short / trailing / non-canonical word, 2 shape mismatch, 3 constraint identity
// (OodEvaluationMismatch), 4 proof of work, 5 input opening, 6 commit-phase opening, 7 final polynomial, 8 the lookups'
// cumulative sums do not cancel (rk_p3_verify_claims: with the caller's claims added, see add_claims).  The total length is checked before any query: a proof with trailing words AND a
// defect inside a query is refused with 1.
#include "p3_host.hpp"

#include <initializer_list>
#include <thread>

namespace {

using bb::Ext;
using p3h::Challenger;
using p3h::Layout;
using p3h::MAX_TABLES;

struct Reader {
    const uint32_t* p;
    size_t n, pos = 0;
    bool bad = false;
    const uint32_t* take(size_t k) {
        if (pos + k > n) {
            bad = true;
            return nullptr;
        }
        const uint32_t* q = p + pos;
        pos += k;
        return q;
    }
};
struct Selectors {
    Ext is_first, is_last, is_trans, inv_zeroifier;
};
Selectors selectors_at(const Ext& x, unsigned log_n, uint32_t root27m, uint32_t wm) {
    const Ext z_h = bb::sub(bb::pow(x, (uint64_t)1 << log_n, wm), bb::ext_one());
    const uint32_t g_inv = bb::inv(bb::pow(root27m, (uint64_t)1 << (27 - log_n)));
    Selectors s;
    s.is_first = bb::mul(z_h, bb::inv(bb::sub(x, bb::ext_one()), wm), wm);
    s.is_last = bb::mul(z_h, bb::inv(bb::sub(x, bb::ext_from(g_inv)), wm), wm);
    s.is_trans = bb::sub(x, bb::ext_from(g_inv));
    s.inv_zeroifier = bb::inv(z_h, wm);
    return s;
}
Ext load_ext(const uint32_t* p);
// the claims' side of the lookup argument under the proof's challenges: total += sign / rlc(tuple) per tuple, rlc =
// chal[0] + chal[1] bus + sum_j chal[2 + j] x_j.  false for a tuple whose rlc is zero (reason 8)
bool add_claims(const rk_p3_claim* claims, uint32_t n_claims, const std::vector<uint32_t>& pchal, uint32_t wm, Ext& total) {
    for (uint32_t c = 0; c < n_claims; c++) {
        const rk_p3_claim& cl = claims[c];
        const Ext head = bb::add(load_ext(&pchal[0]), bb::scale(load_ext(&pchal[4]), bb::encode(cl.bus)));
        Ext sum = bb::ext_zero();
        for (size_t i = 0; i < cl.n; i++) {
            Ext rlc = head;
            for (uint32_t j = 0; j < cl.tuple_len; j++)
                rlc = bb::add(rlc, bb::scale(load_ext(&pchal[4 * (2 + (size_t)j)]), cl.tuples[i * cl.tuple_len + j]));
            if (bb::eq(rlc, bb::ext_zero())) return false;
            sum = bb::add(sum, bb::inv(rlc, wm));
        }
        total = cl.sign > 0 ? bb::add(total, sum) : bb::sub(total, sum);
    }
    return true;
}
// the arguments of the claims: what RK_ERR_INVALID names in the header
int check_claims(const rk_p3_claim* claims, uint32_t n_claims, uint32_t n_chal) {
    if (n_claims && !claims) return RK_ERR_INVALID;
    for (uint32_t c = 0; c < n_claims; c++) {
        const rk_p3_claim& cl = claims[c];
        if ((cl.sign != 1 && cl.sign != -1) || cl.bus >= bb::P || (cl.n && cl.tuple_len && !cl.tuples)) return RK_ERR_INVALID;
        if (4 * ((uint64_t)cl.tuple_len + 2) > n_chal) return RK_ERR_INVALID;   // also: tables without lookups (n_chal 0)
        for (size_t i = 0; i < cl.n * cl.tuple_len; i++)
            if (cl.tuples[i] >= bb::P) return RK_ERR_INVALID;
    }
    return 0;
}
Ext load_ext(const uint32_t* p) { return Ext{{p[0], p[1], p[2], p[3]}}; }
void put(std::vector<uint32_t>& v, const uint32_t* w, size_t n) { v.insert(v.end(), w, w + n); }

// folder.rs on extension elements (the verifier's side): accumulator = accumulator * alpha + x per assert, in order
struct PermView {   // the verifier's view of a table's lookup argument (all null without one)
    const Ext *local = nullptr, *next = nullptr;
    const uint32_t *chal = nullptr, *cumsum = nullptr;
    const Ext *prep_local = nullptr, *prep_next = nullptr;   // and of its preprocessed columns (null without any)
};
Ext air_fold(const rk_air& air, const Ext* local, const Ext* next, const uint32_t* pub, const Ext& is_first, const Ext& is_last,
             const Ext& is_trans, const Ext& alpha, uint32_t wm, const PermView& pv) {
    std::vector<Ext> v;
    v.reserve(air.steps.size());
    Ext acc = bb::ext_zero();
    for (const rk_air_step& st : air.steps) {
        switch (st.op) {
            case RK_AIR_CONST: v.push_back(bb::ext_from(bb::encode(st.a))); break;
            case RK_AIR_LOCAL: v.push_back(local[st.a]); break;
            case RK_AIR_NEXT: v.push_back(next[st.a]); break;
            case RK_AIR_PUBLIC: v.push_back(bb::ext_from(pub[st.a])); break;
            case RK_AIR_IS_FIRST_ROW: v.push_back(is_first); break;
            case RK_AIR_IS_LAST_ROW: v.push_back(is_last); break;
            case RK_AIR_IS_TRANSITION: v.push_back(is_trans); break;
            case RK_AIR_PERM_LOCAL: v.push_back(pv.local[st.a]); break;
            case RK_AIR_PERM_NEXT: v.push_back(pv.next[st.a]); break;
            case RK_AIR_CHALLENGE: v.push_back(bb::ext_from(pv.chal[st.a])); break;
            case RK_AIR_CUMSUM: v.push_back(bb::ext_from(pv.cumsum[st.a])); break;
            case RK_AIR_PREP_LOCAL: v.push_back(pv.prep_local[st.a]); break;
            case RK_AIR_PREP_NEXT: v.push_back(pv.prep_next[st.a]); break;
            case RK_AIR_ADD: v.push_back(bb::add(v[st.a], v[st.b])); break;
            case RK_AIR_SUB: v.push_back(bb::sub(v[st.a], v[st.b])); break;
            case RK_AIR_MUL: v.push_back(bb::mul(v[st.a], v[st.b], wm)); break;
            case RK_AIR_NEG: v.push_back(bb::sub(bb::ext_zero(), v[st.a])); break;
            default: acc = bb::add(bb::mul(acc, alpha, wm), v[st.a]); break;
        }
    }
    return acc;
}

// ---------------------------------------------------------------- what a run can record (the rk_p3_fri_* captures)
enum : unsigned { CAP_OPENINGS = 1, CAP_INPUTS = 2, CAP_PATHS = 4, CAP_TRANSCRIPT = 8 };
struct Record {
    std::vector<uint32_t> publics, records;
    size_t per_record = 0;   // words one query writes into `records`
};
struct Captures {
    unsigned want;
    uint32_t log_max = 0, n_rounds = 0, blowup_log2 = 0, queries = 0;
    // rk_p3_fri_openings: what the commit-phase check of every query read
    //   publics: beta 4 R | commit-phase roots 8 R | final polynomial 4
    //   records, per query: index | per round: joining reduced opening 4, sibling 4, path 8 lfh
    Record openings;
    // rk_p3_fri_inputs: what the reduced openings of every query are computed from, grouped by matrix and point: every
    // group is (sum_k alpha^k p_k(x) - S) / (x - z) with S = sum_k alpha^k y_k over the same powers
    //   layout, per opened matrix in the verifier's order (Opened::mats): batch, round L - lh, width, points, log_n
    //   publics: alpha 4 | zeta 4 | per matrix and point: first power A 4, S 4
    //   records, per query: index | trace rows | preprocessed rows (keyed) | permutation rows | quotient rows: the
    //   layout's order, a slot's offset in a record is a running sum over the layout
    Record inputs;
    std::vector<uint32_t> layout;
    // rk_p3_fri_input_paths: the commitments of the input batches and the Merkle paths of their openings
    //   publics: trace root 8 | permutation root 8 (zeros without one) | quotient root 8 | log_pmax, and with a
    //   preprocessed batch | the caller's preprocessed root 8 | log_kmax
    //   records, per query, in batch-number order: trace path 8 L | permutation path 8 log_pmax | quotient path 8 L |
    //   preprocessed path 8 log_kmax
    Record paths;
    p3h::Transcript transcript;   // rk_p3_fri_transcript
};

// ---------------------------------------------------------------- the parsed proof
struct Statement {   // the arguments of rk_p3_verify
    const rk_params* params;
    const rk_p3_table* tables;
    uint32_t n_tables;
    const uint32_t* init;
    size_t n_init;
    const uint32_t* proof;
    size_t words;
    bool keyed = false;                    // rk_p3_verify_key: the caller knows the preprocessed batch
    const uint32_t* prep_root = nullptr;   // the verifying key's root, null when no table has preprocessed columns
    const rk_p3_claim* claims = nullptr;   // rk_p3_verify_claims: interactions the verifier adds to the lookup argument
    uint32_t n_claims = 0;
};
// the input batches.  The numbers are what the captures index by; the ORDER of a proof and of the reduced openings is
// trace, preprocessed, permutation, quotient (BATCH_ORDER)
enum { TRACE = 0, PERM = 1, QUOTIENT = 2, PREP = 3, N_BATCHES = 4 };
constexpr int BATCH_ORDER[N_BATCHES] = {TRACE, PREP, PERM, QUOTIENT};
struct OpenedMatrix {
    uint32_t batch;
    unsigned log_n, lh;        // log2 of the trace's rows and of the LDE's
    uint32_t width, at;        // columns, and where they start in the batch's opened row
    uint32_t points;           // 2: zeta and zeta * g; 1: zeta
    const uint32_t* y[2];      // the opened values per point, 4 words per column
};
struct Opened {
    rk_params par;
    rk::Sys sys;
    std::unique_ptr<p2::Any> k = std::make_unique<p2::Any>();
    Challenger ch{k.get()};
    const rk_p3_table* tables = nullptr;
    uint32_t n_tables = 0, lqd[MAX_TABLES];
    unsigned log_n[MAX_TABLES];
    Reader r{nullptr, 0};
    Layout lay;
    // pointers into the proof, and the challenges in between
    const uint32_t* root[N_BATCHES] = {nullptr, nullptr, nullptr, nullptr};   // PREP: the caller's, not the proof's
    const uint32_t* cumsum[MAX_TABLES] = {nullptr};
    std::vector<uint32_t> pchal;   // lookups: [alpha | beta^0 | .. | beta^K], every table reads a prefix
    struct TableY {
        const uint32_t *local, *next, *klocal, *knext, *plocal, *pnext, *chunks;   // k..: the preprocessed columns
    } y[MAX_TABLES];
    Ext alpha, zeta, alpha2, final_poly;
    const uint32_t *commits = nullptr, *fp = nullptr;
    std::vector<Ext> betas;
    // every opened matrix in the verifier's order -- traces, preprocessed, permutation traces, quotient chunks, by table in each: the
    // order the batches are hashed in, the reduced openings take their powers of alpha in and rk_p3_fri_inputs lays out
    std::vector<OpenedMatrix> mats;
    std::vector<uint32_t> heights[N_BATCHES], widths[N_BATCHES];   // the same per batch, as rk_mmcs_verify reads them
    std::vector<uint32_t> indices;

    uint32_t gen(unsigned bits) const { return bb::pow(sys.root27m, (uint64_t)1 << (27 - bits)); }
    void add_matrix(uint32_t batch, uint32_t t, uint32_t width, uint32_t points, const uint32_t* y0, const uint32_t* y1) {
        uint32_t at = 0;
        for (uint32_t w : widths[batch]) at += w;
        mats.push_back(OpenedMatrix{batch, log_n[t], log_n[t] + sys.blowup_log2, width, at, points, {y0, y1}});
        heights[batch].push_back(1u << (log_n[t] + sys.blowup_log2));
        widths[batch].push_back(width);
    }
};

int open_statement(Opened& o, const Statement& st, p3h::Transcript* log) {
    o.par = p3h::params_or_sp1(st.params);
    RK_TRY(rk::resolve_params(&o.par, &o.sys, o.k.get()));
    const rk_p3_table* tables = o.tables = st.tables;
    const uint32_t n_tables = o.n_tables = st.n_tables;
    RK_TRY(p3h::check_tables(o.par, tables, n_tables, false, o.lqd, st.keyed));
    if (!st.proof || (st.n_init && !st.init)) return RK_ERR_INVALID;
    uint32_t n_chal = 0;   // a table without lookups has none
    for (uint32_t t = 0; t < n_tables; t++) n_chal = std::max(n_chal, tables[t].air->n_chal);
    RK_TRY(check_claims(st.claims, st.n_claims, n_chal));
    {   // the verifying key: the root and the pinned height of every table with preprocessed columns, both or neither
        bool any = false;
        for (uint32_t t = 0; t < n_tables; t++) {
            if (!tables[t].air->prep_width) continue;
            any = true;
            if (!tables[t].log_height) return RK_ERR_INVALID;
        }
        if (any != (st.prep_root != nullptr)) return RK_ERR_INVALID;
        for (int i = 0; any && i < 8; i++)
            if (st.prep_root[i] >= bb::P) return RK_ERR_INVALID;
        o.root[PREP] = st.prep_root;
    }
    for (size_t i = 0; i < st.n_init; i++)
        if (st.init[i] >= bb::P) return RK_ERR_INVALID;
    for (size_t i = 0; i < st.words; i++)
        if (st.proof[i] >= bb::P) return 1;
    const unsigned blow = o.sys.blowup_log2;
    Reader& r = o.r = Reader{st.proof, st.words};
    const uint32_t* hdr = r.take(1 + (size_t)n_tables);
    if (!hdr || hdr[0] != n_tables) return 2;
    for (uint32_t t = 0; t < n_tables; t++) {
        o.log_n[t] = hdr[1 + t];
        if (o.log_n[t] < 1 || o.log_n[t] + blow > ntt::LAMBDA) return 2;
        if (tables[t].log_height && tables[t].log_height != o.log_n[t]) return 2;   // a height the statement pins (a 2^16-row range table)
    }
    o.lay = Layout(blow, tables, n_tables, o.lqd, o.log_n);
    Challenger& ch = o.ch;
    ch.log = log;
    ch.observe(st.init, st.n_init);
    if (o.root[PREP]) ch.observe(o.root[PREP], 8);
    if (!(o.root[TRACE] = r.take(8))) return 1;
    ch.observe(o.root[TRACE], 8);
    for (uint32_t t = 0; t < n_tables; t++) ch.observe(tables[t].public_values, tables[t].n_public);
    // lookups: the permutation challenges, the second commitment, the cumulative sums (which must cancel)
    o.pchal.assign(n_chal, 0);
    if (o.lay.prow) {
        const Ext pa = ch.sample_ext(), pb = ch.sample_ext();
        std::memcpy(o.pchal.data(), pa.c, 16);
        Ext cur = bb::ext_one();
        for (uint32_t j = 1; 4 * j < n_chal; j++) {
            std::memcpy(&o.pchal[4 * j], cur.c, 16);
            cur = bb::mul(cur, pb, o.sys.wm);
        }
        if (!(o.root[PERM] = r.take(8))) return 1;
        ch.observe(o.root[PERM], 8);
        Ext total = bb::ext_zero();
        for (uint32_t t = 0; t < n_tables; t++) {
            if (!tables[t].air->perm_width) continue;
            if (!(o.cumsum[t] = r.take(4))) return 1;
            ch.observe(o.cumsum[t], 4);
            total = bb::add(total, load_ext(o.cumsum[t]));
        }
        if (!add_claims(st.claims, st.n_claims, o.pchal, o.sys.wm, total) || !bb::eq(total, bb::ext_zero())) return 8;
    }
    o.alpha = ch.sample_ext();
    if (!(o.root[QUOTIENT] = r.take(8))) return 1;
    ch.observe(o.root[QUOTIENT], 8);
    o.zeta = ch.sample_ext();
    for (uint32_t t = 0; t < n_tables; t++) {
        const size_t w = tables[t].width, pw = tables[t].air->perm_width, cw = tables[t].air->prep_width;
        Opened::TableY& y = o.y[t];
        y.local = r.take(4 * w);
        y.next = r.take(4 * w);
        y.klocal = cw ? r.take(4 * cw) : nullptr;
        y.knext = cw ? r.take(4 * cw) : nullptr;
        y.plocal = pw ? r.take(4 * pw) : nullptr;
        y.pnext = pw ? r.take(4 * pw) : nullptr;
        y.chunks = r.take((size_t)16 << o.lqd[t]);
        if (r.bad) return 1;
    }
    // every table is in the trace and the quotient batch: both trees have the global maximum height; the permutation
    // batch only holds the tables with lookups, the preprocessed batch those with preprocessed columns
    for (uint32_t t = 0; t < n_tables; t++) o.add_matrix(TRACE, t, tables[t].width, 2, o.y[t].local, o.y[t].next);
    for (uint32_t t = 0; t < n_tables; t++)
        if (tables[t].air->prep_width) o.add_matrix(PREP, t, tables[t].air->prep_width, 2, o.y[t].klocal, o.y[t].knext);
    for (uint32_t t = 0; t < n_tables; t++)
        if (tables[t].air->perm_width) o.add_matrix(PERM, t, tables[t].air->perm_width, 2, o.y[t].plocal, o.y[t].pnext);
    for (uint32_t t = 0; t < n_tables; t++)
        for (uint32_t j = 0; j < (1u << o.lqd[t]); j++) o.add_matrix(QUOTIENT, t, 4, 1, o.y[t].chunks + 16 * (size_t)j, nullptr);
    return 0;
}

int check_constraints(const Opened& o) {
    const uint32_t wm = o.sys.wm, shiftm = o.sys.shiftm;
    for (uint32_t t = 0; t < o.n_tables; t++) {
        const unsigned kq = o.log_n[t] + o.lqd[t];
        const size_t qd = (size_t)1 << o.lqd[t], n = (size_t)1 << o.log_n[t];
        // quotient(zeta) = sum_i zps_i * sum_e x^e * chunk_i[e], zps_i = prod_{j != i} Z_j(zeta) / Z_j(first point of domain i)
        Ext quotient = bb::ext_zero();
        for (size_t i = 0; i < qd; i++) {
            Ext zp = bb::ext_one();
            const uint32_t first_i = bb::mul(shiftm, bb::pow(o.gen(kq), i));
            for (size_t j = 0; j < qd; j++) {
                if (j == i) continue;
                const uint32_t sj_inv = bb::inv(bb::mul(shiftm, bb::pow(o.gen(kq), j)));
                const Ext a = bb::sub(bb::pow(bb::scale(o.zeta, sj_inv), n, wm), bb::ext_one());
                const uint32_t b = bb::sub(bb::pow(bb::mul(first_i, sj_inv), n), bb::ONE);
                zp = bb::mul(zp, bb::scale(a, bb::inv(b)), wm);
            }
            for (int e = 0; e < 4; e++) {
                Ext mono = bb::ext_zero();
                mono.c[e] = bb::ONE;
                quotient = bb::add(quotient, bb::mul(bb::mul(zp, mono, wm), load_ext(o.y[t].chunks + (i * 4 + e) * 4), wm));
            }
        }
        const Selectors s = selectors_at(o.zeta, o.log_n[t], o.sys.root27m, wm);
        const Opened::TableY& y = o.y[t];
        const PermView pv{(const Ext*)y.plocal, (const Ext*)y.pnext, o.pchal.data(), o.cumsum[t], (const Ext*)y.klocal, (const Ext*)y.knext};
        const Ext folded = air_fold(*o.tables[t].air, (const Ext*)y.local, (const Ext*)y.next, o.tables[t].public_values, s.is_first, s.is_last,
                                    s.is_trans, o.alpha, wm, pv);
        if (!bb::eq(bb::mul(folded, s.inv_zeroifier, wm), quotient)) return 3;
    }
    return 0;
}

int open_fri(Opened& o) {
    Reader& r = o.r;
    Challenger& ch = o.ch;
    o.alpha2 = ch.sample_ext();
    const uint32_t* nr = r.take(1);
    if (!nr) return 1;
    const uint32_t n_rounds = o.lay.n_rounds;
    if (*nr != n_rounds) return 2;
    o.commits = r.take(8 * (size_t)n_rounds);
    if (r.bad) return 1;
    o.betas.resize(n_rounds);
    for (uint32_t rd = 0; rd < n_rounds; rd++) {
        ch.observe(o.commits + 8 * rd, 8);
        o.betas[rd] = ch.sample_ext();
    }
    o.fp = r.take(4);
    const uint32_t* wit = r.take(1);
    if (r.bad) return 1;
    o.final_poly = load_ext(o.fp);
    ch.observe(o.fp, 4);
    if (!ch.check_witness(o.sys.pow_bits, *wit)) return 4;
    if (r.pos != o.lay.head_words) return RK_ERR_INTERNAL;   // the reads up to here and Layout describe one head
    if (o.lay.words(o.sys.queries) != r.n) return 1;        // short or trailing words
    o.indices.resize(o.sys.queries);
    for (uint32_t& index : o.indices) index = ch.sample_bits(o.lay.log_max);
    return 0;
}

// what check_query read and computed for one query: the rows and Merkle paths of the three input batches, and per fold
// round the sibling, its path and the reduced opening that joined (zero where no matrix has that height)
struct QueryView {
    uint32_t index;
    const uint32_t *rows[N_BATCHES], *paths[N_BATCHES];
    const uint32_t *sib[ntt::LAMBDA], *path[ntt::LAMBDA];
    Ext joined[ntt::LAMBDA];
};

int check_query(const Opened& o, uint32_t index, Reader r, QueryView& q) {
    const Layout& lay = o.lay;
    const unsigned log_max = lay.log_max;
    const uint32_t wm = o.sys.wm;
    const size_t row_words[N_BATCHES] = {lay.trow, lay.prow, lay.qrow, lay.krow};
    const unsigned tree[N_BATCHES] = {log_max, lay.log_pmax, log_max, lay.log_kmax};
    q.index = index;
    for (int b : BATCH_ORDER) {
        const bool there = (b != PERM || lay.prow) && (b != PREP || lay.krow);
        q.rows[b] = there ? r.take(row_words[b]) : nullptr;
        q.paths[b] = there ? r.take(8 * (size_t)tree[b]) : nullptr;
    }
    if (r.bad) return 1;
    for (int b : BATCH_ORDER)   // the preprocessed batch against the caller's root
        if (q.rows[b] && rk_mmcs_verify(&o.par, o.heights[b].data(), o.widths[b].data(), (uint32_t)o.heights[b].size(), index >> (log_max - tree[b]),
                                        q.rows[b], q.paths[b], o.root[b]) != 0)
            return 5;
    // the reduced opening per LDE height: sum over the matrices of that height, their points and columns, in the
    // verifier's order, of alpha^k (p(x) - p(z)) / (x - z) at x = shift * g^bitrev(index >> (log_max - lh))
    Ext rop[ntt::LAMBDA + 1], apow[ntt::LAMBDA + 1];
    uint32_t x[ntt::LAMBDA + 1];
    bool used[ntt::LAMBDA + 1] = {false};
    for (const OpenedMatrix& m : o.mats) {
        const unsigned lh = m.lh;
        if (!used[lh]) {
            used[lh] = true;
            rop[lh] = bb::ext_zero(), apow[lh] = bb::ext_one();
            x[lh] = bb::mul(o.sys.shiftm, bb::pow(o.gen(lh), bb::bitrev(index >> (log_max - lh), lh)));
        }
        const uint32_t* row = q.rows[m.batch] + m.at;
        for (uint32_t p = 0; p < m.points; p++) {
            const Ext z = p ? bb::scale(o.zeta, o.gen(m.log_n)) : o.zeta;
            const Ext inv_den = bb::inv(bb::sub(bb::ext_from(x[lh]), z), wm);
            for (uint32_t c = 0; c < m.width; c++) {
                const Ext quot = bb::mul(bb::sub(bb::ext_from(row[c]), load_ext(m.y[p] + 4 * c)), inv_den, wm);
                rop[lh] = bb::add(rop[lh], bb::mul(apow[lh], quot, wm));
                apow[lh] = bb::mul(apow[lh], o.alpha2, wm);
            }
        }
    }
    Ext folded = bb::ext_zero();
    uint32_t idx = index;
    for (uint32_t rd = 0; rd < lay.n_rounds; rd++) {
        const unsigned lfh = log_max - 1 - rd;
        q.joined[rd] = used[lfh + 1] ? rop[lfh + 1] : bb::ext_zero();
        if (used[lfh + 1]) folded = bb::add(folded, rop[lfh + 1]);
        q.sib[rd] = r.take(4);
        q.path[rd] = r.take(8 * (size_t)lfh);
        if (r.bad) return 1;
        uint32_t pair[8];
        std::memcpy(pair + 4 * (idx & 1), folded.c, 16);
        std::memcpy(pair + 4 * ((idx ^ 1) & 1), q.sib[rd], 16);
        const uint32_t dh = 1u << lfh, dw = 8;
        static const uint32_t no_path[8] = {0};
        if (rk_mmcs_verify(&o.par, &dh, &dw, 1, idx >> 1, pair, lfh ? q.path[rd] : no_path, o.commits + 8 * rd) != 0) return 6;
        idx >>= 1;
        // fold_row: the line through (x0, e0) and (-x0, e1) at beta; x0 = g^bitrev(idx) in the subgroup of order 2^(lfh+1)
        const uint32_t x0 = bb::pow(o.gen(lfh + 1), bb::bitrev(idx, lfh));
        const Ext e0 = load_ext(pair), e1 = load_ext(pair + 4);
        const Ext slope = bb::scale(bb::sub(e1, e0), bb::inv(bb::sub(bb::neg(x0), x0)));
        folded = bb::add(e0, bb::mul(bb::sub(o.betas[rd], bb::ext_from(x0)), slope, wm));
    }
    if (!bb::eq(folded, o.final_poly)) return 7;
    return 0;
}

// ---- the captures: the query-independent side once the proof is parsed, then one record per accepted query
void begin_captures(const Opened& o, Captures& c) {
    const Layout& lay = o.lay;
    const uint32_t wm = o.sys.wm;
    c.log_max = lay.log_max, c.n_rounds = lay.n_rounds, c.blowup_log2 = o.sys.blowup_log2, c.queries = o.sys.queries;
    if (c.want & CAP_OPENINGS) {
        for (const Ext& beta : o.betas) put(c.openings.publics, beta.c, 4);
        put(c.openings.publics, o.commits, 8 * (size_t)lay.n_rounds);
        put(c.openings.publics, o.fp, 4);
        c.openings.per_record = 1;
        for (uint32_t rd = 0; rd < lay.n_rounds; rd++) c.openings.per_record += 8 + 8 * (size_t)(lay.log_max - 1 - rd);
    }
    if (c.want & CAP_INPUTS) {   // A and S of every group, with the powers the loop in check_query gives its terms
        Ext ap[ntt::LAMBDA + 1];
        for (Ext& a : ap) a = bb::ext_one();
        put(c.inputs.publics, o.alpha2.c, 4);
        put(c.inputs.publics, o.zeta.c, 4);
        for (const OpenedMatrix& m : o.mats) {
            for (uint32_t v : {m.batch, lay.log_max - m.lh, m.width, m.points, m.log_n}) c.layout.push_back(bb::encode(v));
            for (uint32_t p = 0; p < m.points; p++) {
                Ext s = bb::ext_zero();
                put(c.inputs.publics, ap[m.lh].c, 4);
                for (uint32_t col = 0; col < m.width; col++) {
                    s = bb::add(s, bb::mul(ap[m.lh], load_ext(m.y[p] + 4 * col), wm));
                    ap[m.lh] = bb::mul(ap[m.lh], o.alpha2, wm);
                }
                put(c.inputs.publics, s.c, 4);
            }
        }
        c.inputs.per_record = 1 + lay.trow + lay.krow + lay.prow + lay.qrow;
    }
    if (c.want & CAP_PATHS) {
        c.paths.publics.assign(lay.krow ? 34 : 25, 0);
        for (int b = 0; b < 3; b++)
            if (o.root[b]) std::copy(o.root[b], o.root[b] + 8, c.paths.publics.begin() + 8 * b);
        c.paths.publics[24] = bb::encode(lay.log_pmax);
        c.paths.per_record = 8 * (size_t)(2 * lay.log_max + lay.log_pmax);
        if (lay.krow) {   // the fourth batch is appended: nothing of the three-batch form moves
            std::copy(o.root[PREP], o.root[PREP] + 8, c.paths.publics.begin() + 25);
            c.paths.publics[33] = bb::encode(lay.log_kmax);
            c.paths.per_record += 8 * (size_t)lay.log_kmax;
        }
    }
    for (Record* rec : {&c.openings, &c.inputs, &c.paths}) rec->records.assign(rec->per_record * o.sys.queries, 0);
}
void record_openings(const Opened& o, const QueryView& q, uint32_t* rec) {
    *rec++ = bb::encode(q.index);
    for (uint32_t rd = 0; rd < o.lay.n_rounds; rd++) {
        const size_t lfh = o.lay.log_max - 1 - rd;
        rec = std::copy(q.joined[rd].c, q.joined[rd].c + 4, rec);
        rec = std::copy(q.sib[rd], q.sib[rd] + 4, rec);
        rec = std::copy(q.path[rd], q.path[rd] + 8 * lfh, rec);
    }
}
void record_inputs(const Opened& o, const QueryView& q, uint32_t* rec) {
    const size_t row_words[N_BATCHES] = {o.lay.trow, o.lay.prow, o.lay.qrow, o.lay.krow};
    *rec++ = bb::encode(q.index);
    for (int b : BATCH_ORDER)
        if (q.rows[b]) rec = std::copy(q.rows[b], q.rows[b] + row_words[b], rec);
}
void record_paths(const Opened& o, const QueryView& q, uint32_t* rec) {
    const size_t tree[N_BATCHES] = {o.lay.log_max, o.lay.log_pmax, o.lay.log_max, o.lay.log_kmax};
    for (int b = 0; b < N_BATCHES; b++)
        if (q.paths[b]) rec = std::copy(q.paths[b], q.paths[b] + 8 * tree[b], rec);
}

int p3_verify(const Statement& st, bool one_thread = false, Captures* cap = nullptr) {
    Opened o;
    int rc = open_statement(o, st, cap && (cap->want & CAP_TRANSCRIPT) ? &cap->transcript : nullptr);
    if (rc == 0) rc = check_constraints(o);
    if (rc == 0) rc = open_fri(o);
    if (rc != 0) return rc;
    if (cap) begin_captures(o, *cap);
    // the query positions come from the transcript one after the other; the queries themselves are independent and of
    // one size, so they are checked on a few threads (100 queries cost ~40 ms of Poseidon2 on one core)
    const uint32_t queries = o.sys.queries;
    const unsigned hw = std::thread::hardware_concurrency();
    const unsigned n_thr = queries >= 16 && !one_thread ? std::max(1u, std::min(4u, hw / 2)) : 1u;
    std::vector<int> first_bad(n_thr, 0);
    std::vector<uint32_t> first_at(n_thr, 0xffffffffu);
    auto run = [&](unsigned t) {
        QueryView q;
        for (uint32_t qi = t; qi < queries; qi += n_thr) {
            Reader rq{st.proof, st.words};
            rq.pos = o.lay.head_words + o.lay.query_words * qi;
            const int v = check_query(o, o.indices[qi], rq, q);
            if (v != 0) {
                first_bad[t] = v;
                first_at[t] = qi;
                return;
            }
            if (!cap) continue;
            if (cap->want & CAP_OPENINGS) record_openings(o, q, cap->openings.records.data() + cap->openings.per_record * qi);
            if (cap->want & CAP_INPUTS) record_inputs(o, q, cap->inputs.records.data() + cap->inputs.per_record * qi);
            if (cap->want & CAP_PATHS) record_paths(o, q, cap->paths.records.data() + cap->paths.per_record * qi);
        }
    };
    if (n_thr == 1) {
        run(0);
    } else {
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < n_thr; t++) pool.emplace_back(run, t);
        for (auto& th : pool) th.join();
    }
    uint32_t best = 0xffffffffu;
    for (unsigned t = 0; t < n_thr; t++)   // the verdict of the first failing query, as a sequential check would give it
        if (first_at[t] < best) {
            best = first_at[t];
            rc = first_bad[t];
        }
    return rc;
}

// ---------------------------------------------------------------- the capture entry points, behind their signatures
struct Out {   // one array a capture hands back: where it was recorded, the caller's buffer, its capacity, its size
    const std::vector<uint32_t>* src;
    uint32_t* dst;
    size_t capacity;
    size_t* words;
    bool encode = false;   // plain integers that leave in Montgomery form
};
// the tables are written for the width-16 Poseidon2 and a fold by two; those with sponge columns for the padding-free
// sponge; the bits table tells a proof-of-work sample from its low bits by the canonical 31-bit form: pow_bits <= 27
bool scope_fold(const rk_params& p) { return p.p2_width == 16 && p.fri_fold_log2 == 1; }
bool scope_sponge(const rk_params& p) { return scope_fold(p) && p.p2_pad_free == 1; }
bool scope_transcript(const rk_params& p) { return scope_sponge(p) && p.pow_bits <= 27; }

// One run of the verifier recording `want`: the sizes are always reported; RK_ERR_CAPACITY and nothing written where a
// buffer is too small; otherwise the shape (Montgomery) and the arrays
int capture(unsigned want, bool (*scope)(const rk_params&), Statement st, uint32_t shape[4], Captures& cap, std::initializer_list<Out> outs) {
    bool ok = shape != nullptr;
    for (const Out& o : outs) ok = ok && o.words && (!o.capacity || o.dst);
    if (!ok) return RK_ERR_INVALID;
    for (const Out& o : outs) *o.words = 0;
    const rk_params par = p3h::params_or_sp1(st.params);
    if (!scope(par)) return RK_ERR_INVALID;
    st.params = &par;
    cap.want = want;
    const int verdict = p3_verify(st, false, &cap);
    if (verdict != 0) return verdict;
    bool fits = true;
    for (const Out& o : outs) fits = (*o.words = o.src->size()) <= o.capacity && fits;
    if (!fits) return RK_ERR_CAPACITY;
    const uint32_t s[4] = {cap.log_max, cap.n_rounds, cap.blowup_log2, cap.queries};
    for (int i = 0; i < 4; i++) shape[i] = bb::encode(s[i]);
    for (const Out& o : outs)
        for (size_t i = 0; i < o.src->size(); i++) o.dst[i] = o.encode ? bb::encode((*o.src)[i]) : (*o.src)[i];
    return 0;
}

// the statement of a _key entry point: the caller knows the preprocessed batch (open_statement's rule on prep_root)
Statement keyed_statement(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* prep_root, const uint32_t* init,
                          size_t n_init, const uint32_t* proof, size_t words) {
    Statement st{params, tables, n_tables, init, n_init, proof, words};
    st.keyed = true;
    st.prep_root = prep_root;
    return st;
}

int verify_hashes(const Statement& st, uint32_t* states, size_t capacity, size_t* n_permutations) {
    if (!n_permutations || (capacity && !states)) return RK_ERR_INVALID;
    const size_t w = p3h::params_or_sp1(st.params).p2_width;
    std::vector<uint32_t> log;
    struct Scope {   // the log is this thread's for the duration of the check, also when the verifier throws
        explicit Scope(std::vector<uint32_t>* l) { p2::g_permute_log = l; }
        ~Scope() { p2::g_permute_log = nullptr; }
    };
    int verdict;
    {
        Scope scope(&log);
        verdict = p3_verify(st, /*one_thread=*/true);
    }
    if (verdict < 0 || (w != 16 && w != 24)) return verdict < 0 ? verdict : RK_ERR_INVALID;
    *n_permutations = log.size() / w;
    if (*n_permutations > capacity) return RK_ERR_CAPACITY;
    std::memcpy(states, log.data(), log.size() * 4);
    return verdict;
}
int fri_openings(const Statement& st, uint32_t shape[4], uint32_t* publics, size_t publics_capacity, uint32_t* records, size_t records_capacity,
                 size_t* publics_words, size_t* records_words) {
    Captures c{};
    return capture(CAP_OPENINGS, scope_fold, st, shape, c,
                   {{&c.openings.publics, publics, publics_capacity, publics_words}, {&c.openings.records, records, records_capacity, records_words}});
}
int fri_inputs(const Statement& st, uint32_t shape[4], uint32_t* layout, size_t layout_capacity, uint32_t* publics, size_t publics_capacity,
               uint32_t* records, size_t records_capacity, size_t* layout_words, size_t* publics_words, size_t* records_words) {
    Captures c{};
    return capture(CAP_INPUTS, scope_fold, st, shape, c,
                   {{&c.layout, layout, layout_capacity, layout_words},
                    {&c.inputs.publics, publics, publics_capacity, publics_words},
                    {&c.inputs.records, records, records_capacity, records_words}});
}
int fri_input_paths(const Statement& st, uint32_t shape[4], uint32_t* publics, size_t publics_capacity, uint32_t* records, size_t records_capacity,
                    size_t* publics_words, size_t* records_words) {
    Captures c{};
    return capture(CAP_PATHS, scope_sponge, st, shape, c,
                   {{&c.paths.publics, publics, publics_capacity, publics_words}, {&c.paths.records, records, records_capacity, records_words}});
}
int fri_transcript(const Statement& st, uint32_t shape[4], uint32_t* ops, size_t ops_capacity, uint32_t* observed, size_t observed_capacity,
                   uint32_t* sampled, size_t sampled_capacity, size_t* ops_words, size_t* observed_words, size_t* sampled_words) {
    Captures c{};
    return capture(CAP_TRANSCRIPT, scope_transcript, st, shape, c,
                   {{&c.transcript.ops, ops, ops_capacity, ops_words, /*encode=*/true},
                    {&c.transcript.observed, observed, observed_capacity, observed_words},
                    {&c.transcript.sampled, sampled, sampled_capacity, sampled_words}});
}

}  // namespace

extern "C" {

int rk_p3_verify(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init_words, size_t n_init,
                 const uint32_t* proof, size_t proof_words) {
    RK_GUARD_BEGIN
    return p3_verify({params, tables, n_tables, init_words, n_init, proof, proof_words});
    RK_GUARD_END
}

int rk_p3_verify_key(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* prep_root, const uint32_t* init_words,
                     size_t n_init, const uint32_t* proof, size_t proof_words) {
    RK_GUARD_BEGIN
    return p3_verify(keyed_statement(params, tables, n_tables, prep_root, init_words, n_init, proof, proof_words));
    RK_GUARD_END
}

int rk_p3_verify_claims(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* prep_root, const uint32_t* init_words,
                        size_t n_init, const uint32_t* proof, size_t proof_words, const rk_p3_claim* claims, uint32_t n_claims) {
    RK_GUARD_BEGIN
    Statement st = prep_root ? keyed_statement(params, tables, n_tables, prep_root, init_words, n_init, proof, proof_words)
                             : Statement{params, tables, n_tables, init_words, n_init, proof, proof_words};
    st.claims = claims;
    st.n_claims = n_claims;
    return p3_verify(st);
    RK_GUARD_END
}

int rk_p3_verify_hashes(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init_words, size_t n_init,
                        const uint32_t* proof, size_t proof_words, uint32_t* states, size_t capacity, size_t* n_permutations) {
    RK_GUARD_BEGIN
    return verify_hashes({params, tables, n_tables, init_words, n_init, proof, proof_words}, states, capacity, n_permutations);
    RK_GUARD_END
}
int rk_p3_verify_hashes_key(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* prep_root,
                            const uint32_t* init_words, size_t n_init, const uint32_t* proof, size_t proof_words, uint32_t* states, size_t capacity,
                            size_t* n_permutations) {
    RK_GUARD_BEGIN
    return verify_hashes(keyed_statement(params, tables, n_tables, prep_root, init_words, n_init, proof, proof_words), states, capacity, n_permutations);
    RK_GUARD_END
}

int rk_p3_fri_openings(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init_words, size_t n_init,
                       const uint32_t* proof, size_t proof_words, uint32_t shape[4], uint32_t* publics, size_t publics_capacity,
                       uint32_t* records, size_t records_capacity, size_t* publics_words, size_t* records_words) {
    RK_GUARD_BEGIN
    return fri_openings({params, tables, n_tables, init_words, n_init, proof, proof_words}, shape, publics, publics_capacity, records,
                        records_capacity, publics_words, records_words);
    RK_GUARD_END
}
int rk_p3_fri_openings_key(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* prep_root,
                           const uint32_t* init_words, size_t n_init, const uint32_t* proof, size_t proof_words, uint32_t shape[4],
                           uint32_t* publics, size_t publics_capacity, uint32_t* records, size_t records_capacity, size_t* publics_words,
                           size_t* records_words) {
    RK_GUARD_BEGIN
    return fri_openings(keyed_statement(params, tables, n_tables, prep_root, init_words, n_init, proof, proof_words), shape, publics,
                        publics_capacity, records, records_capacity, publics_words, records_words);
    RK_GUARD_END
}

int rk_p3_fri_inputs(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init_words, size_t n_init,
                     const uint32_t* proof, size_t proof_words, uint32_t shape[4], uint32_t* layout, size_t layout_capacity, uint32_t* publics,
                     size_t publics_capacity, uint32_t* records, size_t records_capacity, size_t* layout_words, size_t* publics_words,
                     size_t* records_words) {
    RK_GUARD_BEGIN
    return fri_inputs({params, tables, n_tables, init_words, n_init, proof, proof_words}, shape, layout, layout_capacity, publics,
                      publics_capacity, records, records_capacity, layout_words, publics_words, records_words);
    RK_GUARD_END
}
int rk_p3_fri_inputs_key(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* prep_root,
                         const uint32_t* init_words, size_t n_init, const uint32_t* proof, size_t proof_words, uint32_t shape[4], uint32_t* layout,
                         size_t layout_capacity, uint32_t* publics, size_t publics_capacity, uint32_t* records, size_t records_capacity,
                         size_t* layout_words, size_t* publics_words, size_t* records_words) {
    RK_GUARD_BEGIN
    return fri_inputs(keyed_statement(params, tables, n_tables, prep_root, init_words, n_init, proof, proof_words), shape, layout, layout_capacity,
                      publics, publics_capacity, records, records_capacity, layout_words, publics_words, records_words);
    RK_GUARD_END
}

int rk_p3_fri_input_paths(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init_words, size_t n_init,
                          const uint32_t* proof, size_t proof_words, uint32_t shape[4], uint32_t* publics, size_t publics_capacity,
                          uint32_t* records, size_t records_capacity, size_t* publics_words, size_t* records_words) {
    RK_GUARD_BEGIN
    return fri_input_paths({params, tables, n_tables, init_words, n_init, proof, proof_words}, shape, publics, publics_capacity, records,
                           records_capacity, publics_words, records_words);
    RK_GUARD_END
}
int rk_p3_fri_input_paths_key(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* prep_root,
                              const uint32_t* init_words, size_t n_init, const uint32_t* proof, size_t proof_words, uint32_t shape[4],
                              uint32_t* publics, size_t publics_capacity, uint32_t* records, size_t records_capacity, size_t* publics_words,
                              size_t* records_words) {
    RK_GUARD_BEGIN
    return fri_input_paths(keyed_statement(params, tables, n_tables, prep_root, init_words, n_init, proof, proof_words), shape, publics,
                           publics_capacity, records, records_capacity, publics_words, records_words);
    RK_GUARD_END
}

int rk_p3_fri_transcript(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init_words, size_t n_init,
                         const uint32_t* proof, size_t proof_words, uint32_t shape[4], uint32_t* ops, size_t ops_capacity, uint32_t* observed,
                         size_t observed_capacity, uint32_t* sampled, size_t sampled_capacity, size_t* ops_words, size_t* observed_words,
                         size_t* sampled_words) {
    RK_GUARD_BEGIN
    return fri_transcript({params, tables, n_tables, init_words, n_init, proof, proof_words}, shape, ops, ops_capacity, observed,
                          observed_capacity, sampled, sampled_capacity, ops_words, observed_words, sampled_words);
    RK_GUARD_END
}
int rk_p3_fri_transcript_key(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* prep_root,
                             const uint32_t* init_words, size_t n_init, const uint32_t* proof, size_t proof_words, uint32_t shape[4], uint32_t* ops,
                             size_t ops_capacity, uint32_t* observed, size_t observed_capacity, uint32_t* sampled, size_t sampled_capacity,
                             size_t* ops_words, size_t* observed_words, size_t* sampled_words) {
    RK_GUARD_BEGIN
    return fri_transcript(keyed_statement(params, tables, n_tables, prep_root, init_words, n_init, proof, proof_words), shape, ops, ops_capacity,
                          observed, observed_capacity, sampled, sampled_capacity, ops_words, observed_words, sampled_words);
    RK_GUARD_END
}

}  // extern "C"
