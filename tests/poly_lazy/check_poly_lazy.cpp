// Stand-alone check of raiko_amd/csrc/poly_lazy.hpp on the host: the accumulate / fold / finish functions at the
// worst cases of their 64-bit accumulators, against plain `% p` arithmetic in 128-bit integers.  The accumulators are
// unsigned, so an overflow shows as a wrong result (the build's -fsanitize=undefined covers the rest of the
// arithmetic: shifts, signed conversions).  Exit status 0 = every case agrees.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "poly_lazy.hpp"

typedef unsigned __int128 u128;
static const uint64_t P = bb::P;
static int failures = 0;

static uint64_t powmod(uint64_t a, uint64_t e) {
    u128 r = 1, b = a % P;
    for (; e; e >>= 1, b = b * b % P)
        if (e & 1) r = r * b % P;
    return (uint64_t)r;
}
static const uint64_t RINV = powmod(((uint64_t)1 << 32) % P, P - 2);   // 2^-32 mod p

struct Term {
    uint32_t v;
    bb::Ext m;
};
// the reference: (sum v * m) * 2^-32 mod p per component, the sum reduced term by term in 128 bits
static bb::Ext reference(const std::vector<Term>& terms) {
    bb::Ext r;
    for (int j = 0; j < 4; j++) {
        u128 s = 0;
        for (const Term& t : terms) s = (s + (u128)t.v * t.m.c[j]) % P;
        r.c[j] = (uint32_t)(s * RINV % P);
    }
    return r;
}
// the policy of the header as the kernels apply it: a fold after every FOLD_TERMS terms, finish wherever the sum ends
static bb::Ext lazy(const std::vector<Term>& terms) {
    pl::Acc acc = pl::zero();
    int n = 0;
    for (const Term& t : terms) {
        pl::mac(acc, t.v, t.m);
        if (++n == pl::FOLD_TERMS) {
            pl::fold(acc);
            n = 0;
        }
    }
    return pl::finish(acc);
}
// the chain the kernels used before: canonical arithmetic per term
static bb::Ext eager(const std::vector<Term>& terms) {
    bb::Ext acc = bb::ext_zero();
    for (const Term& t : terms) acc = bb::add(acc, bb::scale(t.m, t.v));
    return acc;
}
static void check(const char* what, size_t n, const bb::Ext& got, const bb::Ext& want) {
    for (int j = 0; j < 4; j++)
        if (got.c[j] != want.c[j] || got.c[j] >= P) {
            std::printf("FAIL %s, %zu terms, component %d: got %u, want %u\n", what, n, j, got.c[j], want.c[j]);
            failures++;
        }
}

int main() {
    const uint32_t top = bb::P - 1;
    const size_t lengths[] = {1, (size_t)pl::FOLD_TERMS - 1, (size_t)pl::FOLD_TERMS, (size_t)pl::FOLD_TERMS + 1, 1000};
    // every coefficient p - 1, every multiplier p - 1
    for (size_t n : lengths) {
        std::vector<Term> terms(n, Term{top, bb::Ext{{top, top, top, top}}});
        check("saturated lazy = reference", n, lazy(terms), reference(terms));
        check("saturated eager = reference", n, eager(terms), reference(terms));
    }
    // mixed: extremes and small values side by side, and pseudo-random words
    uint64_t lcg = 88172645463325252ull;
    auto next = [&]() {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)((lcg >> 33) % P);
    };
    for (size_t n : lengths) {
        std::vector<Term> terms(n);
        for (size_t i = 0; i < n; i++) terms[i] = Term{i % 3 ? top : next(), bb::Ext{{top, 0, 1, next()}}};
        check("mixed lazy = reference", n, lazy(terms), reference(terms));
        check("mixed lazy = eager", n, lazy(terms), eager(terms));
    }
    // the accumulator's own worst case, whatever came before: fold of the largest 64-bit value, FOLD_TERMS largest
    // terms on top; the exact sum must still be below 2^64 (the header's bound) and finish must reduce it
    {
        const uint64_t folded = pl::fold(~(uint64_t)0);
        if (folded != (u128)0xffffffffu * pl::TWO32_MOD_P + 0xffffffffu || folded % P != (uint64_t)(~(uint64_t)0 % P)) {
            std::printf("FAIL fold(2^64 - 1) = %llu\n", (unsigned long long)folded);
            failures++;
        }
        pl::Acc acc{{folded, folded, folded, folded}};
        u128 exact = folded;
        for (int i = 0; i < pl::FOLD_TERMS; i++) {
            pl::mac(acc, top, bb::Ext{{top, top, top, top}});
            exact += (u128)top * top;
        }
        if (exact >> 64 || acc.a[0] != (uint64_t)exact) {
            std::printf("FAIL folded value + %d largest terms leaves 64 bits\n", pl::FOLD_TERMS);
            failures++;
        }
        const uint32_t want = (uint32_t)(exact % P * RINV % P);
        check("largest accumulator", (size_t)pl::FOLD_TERMS, pl::finish(acc), bb::Ext{{want, want, want, want}});
        // one more term would not fit: the interval is the longest one possible
        if (!((exact + (u128)top * top) >> 64)) {
            std::printf("FAIL FOLD_TERMS + 1 terms would fit: the bound in the header is not tight\n");
            failures++;
        }
    }
    // fold keeps the residue and its bound on a sweep of values
    for (int i = 0; i < 100000; i++) {
        uint64_t t = ((uint64_t)next() << 33) ^ ((uint64_t)next() << 2) ^ next();
        if (i < 64) t = ~(uint64_t)0 >> i;
        const uint64_t f = pl::fold(t);
        if (f % P != t % P || f >= ((uint64_t)1 << 60)) {
            std::printf("FAIL fold(%llu) = %llu\n", (unsigned long long)t, (unsigned long long)f);
            failures++;
            break;
        }
    }
    if (failures) return 1;
    std::printf("poly_lazy ok\n");
    return 0;
}
