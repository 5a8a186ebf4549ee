// Host-side seal verifier: the counterpart of `receipt.verify(image_id)` that the reference
// calls after proving (provers/risc0/driver/src/lib.rs:136, benchmark.rs:19, bonsai.rs:67),
// restating risc0-zkp 1.0.1 verify/{mod,fri,merkle,read_iop}.rs for the flow of
// rk_prove_segment.  Pure CPU code (no GPU needed): a host can check seals produced elsewhere.
//
// Checked: transcript binding, Merkle openings, the DEEP quotient at every query, FRI folds, the
// final low-degree polynomial and -- when the caller supplies the circuit's `poly_ext`
// (rk_verify_opts) -- the constraint identity on the tap openings.  The rv32im constraint system
// itself (risc0-circuit-rv32im) is not in this repo; examples/toy_circuit shows a complete one.
#include "segment_host.hpp"

#include <cstring>
#include <memory>

namespace {

using bb::Ext;

// the compiled-in risc0 parameter set (what rk_verify_segment assumes)
struct Defaults {
    rk::Sys sys;
    p2::Any p2any;
    Defaults() {
        rk_params def;
        rk::params_preset(&def, RK_PRESET_RISC0);
        (void)rk::resolve_params(&def, &sys, &p2any);
    }
};
const Defaults& defaults() {
    static Defaults d;
    return d;
}
using Sponge = p2::Rng;

struct Reader {
    const uint32_t* p;
    size_t len, pos = 0;
    bool short_read = false;
    void read(uint32_t* out, size_t n) {
        if (pos + n > len) {
            short_read = true;
            std::memset(out, 0, n * 4);
            return;
        }
        std::memcpy(out, p + pos, n * 4);
        pos += n;
    }
};

struct TreeVerifier {  // MerkleTreeVerifier
    size_t rows = 0, cols = 0, top_size = 1;
    std::vector<uint32_t> top;  // heap, index 1 = root
    void init(const p2::Any& k, Reader& r, Sponge& rng, size_t rows_, size_t cols_, size_t queries) {
        rows = rows_;
        cols = cols_;
        top_size = (size_t)1 << rk::merkle_top_layer(rows, queries);
        top.assign(2 * top_size * 8, 0);
        r.read(top.data() + top_size * 8, top_size * 8);
        for (size_t i = top_size; i-- > 1;) k.hash_pair(&top[2 * i * 8], &top[(2 * i + 1) * 8], &top[i * 8]);
        rng.mix(&top[8]);
    }
    bool open(const p2::Any& k, Reader& r, size_t idx, uint32_t* row) const {
        if (idx >= rows) return false;
        r.read(row, cols);
        uint32_t cur[8], other[8], nxt[8];
        k.hash_elems(row, cols, cur);
        idx += rows;
        while (idx >= 2 * top_size) {
            bool right = idx & 1;
            r.read(other, 8);
            idx >>= 1;
            if (right) k.hash_pair(other, cur, nxt);
            else k.hash_pair(cur, other, nxt);
            std::memcpy(cur, nxt, 32);
        }
        return std::memcmp(cur, &top[idx * 8], 32) == 0;
    }
};

Ext poly_eval(const Ext* c, size_t n, const Ext& x, uint32_t wm) {
    Ext acc = bb::ext_zero();
    for (size_t i = n; i-- > 0;) acc = bb::add(bb::mul(acc, x, wm), c[i]);
    return acc;
}

// the parameter set a seal is checked under: opts->params (the whole blob), else the three width-24 tables of ABI 1,
// else the defaults
struct ParamSet {
    rk::Sys sys = defaults().sys;
    std::unique_ptr<p2::Any> custom;
    const p2::Any* k = &defaults().p2any;
    int resolve(const rk_verify_opts* opts) {
        rk_params pp;
        const rk_params* from = nullptr;
        if (opts && opts->params) {
            from = opts->params;
        } else if (opts && (opts->p2_rc_ext || opts->p2_rc_int || opts->p2_diag)) {
            if (!opts->p2_rc_ext || !opts->p2_rc_int || !opts->p2_diag) return RK_ERR_INVALID;
            rk::params_preset(&pp, RK_PRESET_RISC0);
            pp.p2_rc_ext = opts->p2_rc_ext;
            pp.p2_rc_int = opts->p2_rc_int;
            pp.p2_diag = opts->p2_diag;
            from = &pp;
        }
        if (!from) return RK_OK;
        custom = std::make_unique<p2::Any>();
        k = custom.get();
        return rk::resolve_params(from, &sys, custom.get()) == RK_OK ? RK_OK : RK_ERR_INVALID;
    }
};

// One rk_verify_segment_ex: what was read from the seal and drawn from the sponge, and the checks in the order of the
// prover's stages.  Every stage returns 0 or the reason code of its first failed check.
struct SegmentCheck {
    const rk_segment* pub;
    const rk_verify_opts* opts;
    const rk_taps& taps;
    const rk::Sys& sys;
    const p2::Any& k;
    const rk::Shape shape;
    const uint32_t wm;
    const size_t QUERIES, FOLD, CHECK, N, D;
    Reader r;
    Sponge rng;

    TreeVerifier tg[3], tcheck;
    std::vector<uint32_t> accum_mix;
    Ext poly_mix, z, mix;
    std::vector<Ext> pts;       // rk::tap_points: slot b = z * back_one^b, last slot = z^(D/N)
    std::vector<Ext> coeff_u;   // as sent: one interpolating polynomial per register, then the check openings
    std::vector<Ext> combo_u;   // rk::combo_u of them under `mix`
    struct Round {
        size_t domain;
        TreeVerifier tree;
        Ext mix;
    };
    std::vector<Round> rounds;
    size_t degree = 0;          // of the final polynomial
    std::vector<uint32_t> final_coeffs;

    SegmentCheck(const rk_segment* p, const rk_verify_opts* o, const ParamSet& ps, const uint32_t* seal, size_t seal_words)
        : pub(p), opts(o), taps(p->taps), sys(ps.sys), k(*ps.k), shape(ps.sys.shape()), wm(ps.sys.wm), QUERIES(shape.queries),
          FOLD((size_t)1 << shape.fold_log2), CHECK((size_t)4 << shape.blowup_log2), N((size_t)1 << p->po2),
          D(N << shape.blowup_log2), r{seal, seal_words}, rng(ps.k) {}

    // the header, the four trace commitments and the tap openings (reasons 10, 60)
    int header_and_commitments() {
        std::vector<uint32_t> globals(pub->n_globals);
        r.read(globals.data(), pub->n_globals);
        uint32_t po2 = 0;
        r.read(&po2, 1);
        if (r.short_read || po2 != pub->po2) return 10;
        if (pub->n_globals && std::memcmp(globals.data(), pub->globals, pub->n_globals * 4) != 0) return 10;
        rk::bind_header(k, rng, pub);
        tg[1].init(k, r, rng, D, taps.group_size[1], QUERIES);
        tg[2].init(k, r, rng, D, taps.group_size[2], QUERIES);
        accum_mix.resize(pub->n_accum_mix);
        for (uint32_t i = 0; i < pub->n_accum_mix; i++) accum_mix[i] = rng.random_elem();
        tg[0].init(k, r, rng, D, taps.group_size[0], QUERIES);
        poly_mix = rng.random_ext();
        tcheck.init(k, r, rng, D, CHECK, QUERIES);
        z = rng.random_ext();
        pts = rk::tap_points(sys, pub->po2, taps, z);
        coeff_u.resize(rk::total_taps(taps) + CHECK);
        uint32_t digest[8];
        r.read((uint32_t*)coeff_u.data(), coeff_u.size() * 4);
        k.hash_elems((const uint32_t*)coeff_u.data(), coeff_u.size() * 4, digest);
        rng.mix(digest);
        return r.short_read ? 60 : 0;
    }

    // verify/mod.rs: U polynomials back to evaluation form, the circuit's mixed constraint polynomial on them, against
    // check(z) * ((3z)^N - 1) with check(z) = sum_i z^i * g_i(z^(D/N)), g_i = the extension element whose component e is
    // opened in check column (D/N) e + bitrev(i)   (reasons 70, 71)
    int constraint_identity() {
        const size_t tot_taps = rk::total_taps(taps);
        std::vector<Ext> eval_u(tot_taps);
        size_t pos = 0;
        for (uint32_t i = 0; i < taps.n_regs; i++) {
            const size_t sz = rk::reg_taps(taps, i), b0 = taps.combo_off[taps.reg_combo[i]];
            for (size_t j = 0; j < sz; j++) eval_u[pos + j] = poly_eval(&coeff_u[pos], sz, pts[taps.combo_backs[b0 + j]], wm);
            pos += sz;
        }
        Ext result;
        if (opts->poly_ext) {
            if (opts->poly_ext(opts->user, pub, poly_mix.c, (const uint32_t*)eval_u.data(), tot_taps, accum_mix.data(),
                               pub->n_accum_mix, result.c) != 0)
                return 71;
        } else if (rk::program_poly_ext(opts->program, wm, poly_mix.c, (const uint32_t*)eval_u.data(), tot_taps, pub->globals,
                                        pub->n_globals, accum_mix.data(), pub->n_accum_mix, result.c) != RK_OK) {
            return 71;
        }
        // part j of the check polynomial sits in column bitrev(j) of each component ([0,2,1,3] for blow-up 4)
        const size_t parts = (size_t)1 << shape.blowup_log2;
        Ext check = bb::ext_zero(), zi = bb::ext_one();
        for (size_t i = 0; i < parts; i++) {
            for (int e = 0; e < 4; e++) {
                Ext basis = bb::ext_zero();
                basis.c[e] = bb::ONE;
                check = bb::add(check, bb::mul(bb::mul(coeff_u[tot_taps + bb::bitrev((uint32_t)i, shape.blowup_log2) + parts * e], zi, wm), basis, wm));
            }
            zi = bb::mul(zi, z, wm);
        }
        Ext vanish = bb::sub(bb::pow(bb::scale(z, sys.shiftm), N, wm), bb::ext_one());
        return bb::eq(bb::mul(check, vanish, wm), result) ? 0 : 70;
    }

    // the DEEP mix, FRI's commitments, the final polynomial and the proof of work (reasons 60, 62)
    int fri_commitments() {
        mix = rng.random_ext();
        combo_u = rk::combo_u(taps, coeff_u, mix, CHECK, wm);
        degree = rk::fri_walk(N, shape, [&](size_t, size_t domain) {
            rounds.emplace_back();
            Round& rd = rounds.back();
            rd.domain = domain;
            rd.tree.init(k, r, rng, domain / FOLD, FOLD * 4, QUERIES);
            rd.mix = rng.random_ext();
        });
        uint32_t digest[8];
        final_coeffs.resize(4 * degree);
        r.read(final_coeffs.data(), final_coeffs.size());
        k.hash_elems(final_coeffs.data(), final_coeffs.size(), digest);
        rng.mix(digest);
        if (r.short_read) return 60;
        if (shape.pow_bits) {  // the nonce, absorbed, must zero the next pow_bits random bits
            uint32_t nonce = 0;
            r.read(&nonce, 1);
            if (r.short_read) return 60;
            if (nonce >= bb::P) return 62;
            k.hash_elems(&nonce, 1, digest);
            rng.mix(digest);
            if (rng.random_bits(shape.pow_bits) != 0) return 62;
        }
        return 0;
    }

    struct QueryConsts {
        uint32_t gen0, gen_final, fold_root_inv, fold_inv;   // generators of the first and last domain; 1 / the FOLD-th root, 1 / FOLD
    };
    // one query: the four trace openings, the DEEP quotient at its point, every fold, the final polynomial
    // (reasons 2x, 3x, 4x, 50, 60)
    int query(const QueryConsts& qc) {
        size_t pos = rng.random_bits(log2u(D)) % D;
        const Ext x = bb::ext_from(bb::pow(qc.gen0, pos));
        std::vector<uint32_t> row[3];
        uint32_t check_row[64];
        for (int g = 0; g < 3; g++) {
            row[g].resize(taps.group_size[g] + 1);
            if (!tg[g].open(k, r, pos, row[g].data())) return r.short_read ? 60 : 20 + g;
        }
        if (!tcheck.open(k, r, pos, check_row)) return r.short_read ? 60 : 23;
        std::vector<Ext> tot(taps.n_combos + 1, bb::ext_zero());
        Ext cur = bb::ext_one();
        for (uint32_t i = 0; i < taps.n_regs; i++) {
            uint32_t v = row[taps.reg_group[i]][taps.reg_offset[i]];
            tot[taps.reg_combo[i]] = bb::add(tot[taps.reg_combo[i]], bb::scale(cur, v));
            cur = bb::mul(cur, mix, wm);
        }
        for (size_t i = 0; i < CHECK; i++) {
            tot[taps.n_combos] = bb::add(tot[taps.n_combos], bb::scale(cur, check_row[i]));
            cur = bb::mul(cur, mix, wm);
        }
        Ext goal = bb::ext_zero();
        for (uint32_t c = 0; c < taps.n_combos; c++) {
            size_t b0 = taps.combo_off[c], b1 = taps.combo_off[c + 1];
            Ext num = bb::sub(tot[c], poly_eval(&combo_u[b0], b1 - b0, x, wm));
            Ext den = bb::ext_one();
            for (size_t b = b0; b < b1; b++) den = bb::mul(den, bb::sub(x, pts[taps.combo_backs[b]]), wm);
            goal = bb::add(goal, bb::mul(num, bb::inv(den, wm), wm));
        }
        goal = bb::add(goal, bb::mul(bb::sub(tot[taps.n_combos], combo_u.back()), bb::inv(bb::sub(x, pts.back()), wm), wm));

        for (size_t kr = 0; kr < rounds.size(); kr++) {
            const Round& rd = rounds[kr];
            size_t rows = rd.domain / FOLD;
            size_t quot = pos / rows, group = pos % rows;
            uint32_t data[64];
            if (!rd.tree.open(k, r, group, data)) return r.short_read ? 60 : 30 + (int)(kr < 9 ? kr : 9);
            Ext de[16];
            for (size_t i = 0; i < FOLD; i++)
                for (int c = 0; c < 4; c++) de[i].c[c] = data[c * FOLD + i];
            if (!bb::eq(de[quot], goal)) return 40 + (int)(kr < 9 ? kr : 9);
            // interpolate the FOLD coset values and evaluate at mix * w^-group
            Ext co[16];
            for (size_t i = 0; i < FOLD; i++) {
                Ext acc = bb::ext_zero();
                for (size_t j = 0; j < FOLD; j++)
                    acc = bb::add(acc, bb::scale(de[j], bb::pow(qc.fold_root_inv, (uint64_t)((i * j) & (FOLD - 1)))));
                co[i] = bb::scale(acc, qc.fold_inv);
            }
            uint32_t inv_wk = bb::pow(bb::inv(bb::pow(sys.root27m, (uint64_t)1 << (27 - log2u(rd.domain)))), group);
            goal = poly_eval(co, FOLD, bb::scale(rd.mix, inv_wk), wm);
            pos = group;
        }
        const Ext xf = bb::ext_from(bb::pow(qc.gen_final, pos));
        Ext fx = bb::ext_zero();
        for (size_t i = degree; i-- > 0;) {
            Ext c{{final_coeffs[i], final_coeffs[degree + i], final_coeffs[2 * degree + i], final_coeffs[3 * degree + i]}};
            fx = bb::add(bb::mul(fx, xf, wm), c);
        }
        return bb::eq(fx, goal) ? 0 : 50;
    }

    int run() {
        if (int why = header_and_commitments()) return why;
        if (opts && (opts->poly_ext || opts->program))
            if (int why = constraint_identity()) return why;
        if (int why = fri_commitments()) return why;
        const uint32_t w27 = sys.root27m;
        const size_t last_domain = degree << shape.blowup_log2;
        const QueryConsts qc{bb::pow(w27, (uint64_t)1 << (27 - log2u(D))), bb::pow(w27, (uint64_t)1 << (27 - log2u(last_domain))),
                             bb::inv(bb::pow(w27, (uint64_t)1 << (27 - shape.fold_log2))), bb::inv(bb::encode((uint32_t)FOLD))};
        for (size_t q = 0; q < QUERIES; q++)
            if (int why = query(qc)) return why;
        if (r.short_read) return 60;
        if (r.pos != r.len) return 61;
        return RK_OK;
    }
};

// 0: the seal is a valid proof for the public data of `pub` (po2, taps, globals, infos);
// RK_ERR_INVALID: malformed arguments; otherwise a positive reason code:
//   10 header mismatch, 2x group opening failed (x = group id, 3 = check), 3x FRI round opening,
//   4x fold inconsistency, 50 final polynomial mismatch, 60 seal too short, 61 trailing words,
//   62 proof of work, 63 a seal word that is not a canonical field element (>= p),
//   70 constraint identity (only with opts->poly_ext), 71 poly_ext callback failed
int verify_segment(const rk_segment* pub, const rk_verify_opts* opts, const uint32_t* seal, size_t seal_words) {
    if (!pub || !seal) return RK_ERR_INVALID;
    if (rk::check_taps(pub->taps) != RK_OK) return RK_ERR_INVALID;
    if (pub->n_globals && !pub->globals) return RK_ERR_INVALID;
    if (pub->n_accum_mix > (1u << 16)) return RK_ERR_INVALID;
    ParamSet ps;
    RK_TRY(ps.resolve(opts));
    const rk::Shape shape = ps.sys.shape();
    if (!rk::shape_ok(shape) || pub->po2 < 1 || pub->po2 + shape.blowup_log2 > ntt::LAMBDA) return RK_ERR_INVALID;
    // Every word of a seal is a field element in Montgomery form (values, digests, the nonce) or the small integer
    // po2: the arithmetic of the stages (bb::add / sub / mont_reduce) is arithmetic mod p only for operands < p, so a seal
    // from elsewhere carrying a + p in place of a is refused before anything is computed from it (risc0's read_iop
    // rejects invalid elements the same way; rk_mmcs_verify does it per opened row)
    for (size_t i = 0; i < seal_words; i++)
        if (seal[i] >= bb::P) return 63;
    return SegmentCheck(pub, opts, ps, seal, seal_words).run();
}

}  // namespace

extern "C" {

int rk_verify_segment_ex(const rk_segment* pub, const rk_verify_opts* opts, const uint32_t* seal, size_t seal_words) {
    RK_GUARD_BEGIN
    return verify_segment(pub, opts, seal, seal_words);
    RK_GUARD_END
}
// the compiled-in Poseidon2 instance, no constraint identity
int rk_verify_segment(const rk_segment* pub, const uint32_t* seal, size_t seal_words) {
    return rk_verify_segment_ex(pub, nullptr, seal, seal_words);
}

}  // extern "C"
