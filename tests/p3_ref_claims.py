"""TEST INFRASTRUCTURE: the claim sum of rk_p3_verify_claims in exact Python integers, over tests/p3_ref.py's field code
and transcript -- nothing of the product is called, the proof words are only read.

The permutation challenges (alpha, beta) are replayed from the proof (p3_ref.transcript); a claim's tuple contributes
sign / rlc, rlc = chal[0] + chal[1] bus + sum_j chal[2 + j] x_j over the extension elements chal = [alpha | 1 | beta |
beta^2 ..] (p3_ref.challenge_words), exactly as p3_ref.perm_entries reads an interaction.  The lookup argument holds when
the tables' cumulative sums plus the claims' terms are zero."""
import field_ref as F
import p3_ref as R


def claim_total(preset, tables, init_mont, words, claims):
    """claims: [(bus, sign, [canonical tuples])] -> the extension element sum(cumulative sums) + sum(sign / rlc), or
    None when some tuple's rlc is zero (no inverse: the verifier refuses)"""
    W = R.PRESETS[preset][0]
    pf = R.parse(tables, words)
    _alpha, _zeta, pch = R.transcript(preset, tables, [int(v) for v in F.from_mont(init_mont)], pf)
    assert pch is not None, "a proof without lookups has no permutation challenges"
    longest = max([len(t) for _b, _s, ts in claims for t in ts] + [1])
    cw = R.challenge_words(pch, W, longest)
    chal = [tuple(cw[4 * e:4 * e + 4]) for e in range(len(cw) // 4)]
    total = (0, 0, 0, 0)
    for c in pf["cumsums"]:
        total = F.ext_add(total, tuple(c))
    for bus, sign, tuples in claims:
        assert sign in (1, -1)
        for t in tuples:
            rlc = F.ext_add(chal[0], F.ext_scale(chal[1], bus % F.P))
            for j, x in enumerate(t):
                rlc = F.ext_add(rlc, F.ext_scale(chal[2 + j], int(x) % F.P))
            if not any(rlc):
                return None
            term = F.ext_inv(rlc, W)
            total = F.ext_add(total, term) if sign > 0 else F.ext_sub(total, term)
    return tuple(int(v) % F.P for v in total)


def accepts(preset, tables, init_mont, words, claims):
    """whether the lookup argument with the claims holds: what rk_p3_verify_claims's reason 8 must agree with"""
    return claim_total(preset, tables, init_mont, words, claims) == (0, 0, 0, 0)
