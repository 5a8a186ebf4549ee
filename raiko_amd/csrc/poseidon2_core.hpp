// Poseidon2 over BabyBear, x^7, R_F = 8 -- width 24 / rate 16 / R_P = 21 is the
// permutation of risc0's default "poseidon2" hash suite; width 16 / R_P = 13 is SP1's shape (risc0-zkp
// core/hash/poseidon2, un-vendored; reached from the reference through
// `session.prove()` at provers/risc0/driver/src/bonsai.rs:271).  Constants come
// from tools/gen_poseidon2_consts.py (Grain LFSR + published diagonal).
//
// Host and device share this code: the device keeps the 24-word state in VGPRs
// (all indices are compile-time after unrolling) and reads round constants
// through wave-uniform scalar loads.
//
// gfx950 cost model (profiles/r01_ubench_isa.txt): every VALU instruction -- 32-bit
// multiplies and 64-bit mads included -- issues at 16 lanes/clk/SIMD, only plain VGPR add/sub
// is twice as fast.  The permutation is therefore written to minimise instruction count:
//   * S-box: signed Montgomery products (3 instructions each, no reduction inside the chain);
//   * external layer: exact signed 64-bit accumulation of the signed-lazy S-box outputs
//     (v_mad_i64_i32 with small literal multipliers, 64-bit adds) followed by one signed REDC per
//     cell -- no modular addition and no canonicalisation anywhere in a full round.
//     REDC divides by 2^32, so inside a block of four full rounds the state carries a known
//     scale factor 2^(32 e) (e = 0, -7, -56, -399, then -2800): the round constants are
//     pre-scaled per round.  The first block's factor is absorbed by the constants of the
//     partial rounds (one product for cell 0), the second block's by one product per OUTPUT cell
//     after the last layer, so a caller that keeps only some cells (digest, sponge capacity)
//     pays only for those;
//   * internal layers: in blocks of PR_BLOCK rounds, the cells other than 0 are written once per block
//     (PR_BLOCK products and one signed REDC per cell) while cell 0 runs every round (see partial_rounds()).
#pragma once
#include "bb.hpp"

// Rounds per block of the partial rounds (2 or 3; 3 is the shipped choice).  RK_P2_DIRECT selects
// the one-round-at-a-time form instead, for A/B in tools/ubench_p2.hip and tools/census_p2.py.
#ifndef RK_P2_BLOCK
#define RK_P2_BLOCK 3
#endif

namespace p2 {

constexpr int OUT = 8;              // digest cells
constexpr int ROUNDS_HALF_FULL = 4;  // R_F = 8

// acc + x * c for a wave-uniform constant c (scalar register operand): one v_mad_u64_u32.
// Plain C on purpose: an inline-asm mad makes the hazard recogniser pad every product with
// s_nop 1 (its vcc write followed by an opaque SGPR read).
RK_HD uint64_t mad_sc(uint64_t acc, uint32_t x, uint32_t c) { return acc + (uint64_t)x * (uint64_t)c; }
RK_HD uint64_t mul_sc(uint32_t x, uint32_t c) { return (uint64_t)x * (uint64_t)c; }
// signed forms (v_mad_i64_i32), same reason
RK_HD int64_t smad_sc(int64_t acc, int32_t x, int32_t c) { return acc + (int64_t)x * (int64_t)c; }
RK_HD int64_t smul_sc(int32_t x, int32_t c) { return (int64_t)x * (int64_t)c; }

// acc + x * K with a literal multiplier: one v_mad_u64_u32.  The addend is an input of its own, not tied to
// the result: a tied accumulator that is still live afterwards costs a v_mov_b64 first.
template <int K>
RK_HD uint64_t madk(uint32_t x, uint64_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint64_t r;
    asm("v_mad_u64_u32 %0, vcc, %1, %2, %3" : "=v"(r) : "v"(x), "n"(K), "v"(acc) : "vcc");
    return r;
#else
    return acc + (uint64_t)x * (uint64_t)K;
#endif
}
template <int K>
RK_HD uint64_t mulk(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint64_t r;
    asm("v_mad_u64_u32 %0, vcc, %1, %2, 0" : "=v"(r) : "v"(x), "n"(K) : "vcc");
    return r;
#else
    return (uint64_t)x * (uint64_t)K;
#endif
}

// signed forms: acc + x * K on signed-lazy values (v_mad_i64_i32)
template <int K>
RK_HD int64_t smadk(int32_t x, int64_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    int64_t r;
    asm("v_mad_i64_i32 %0, vcc, %1, %2, %3" : "=v"(r) : "v"(x), "n"(K), "v"(acc) : "vcc");
    return r;
#else
    return acc + (int64_t)x * (int64_t)K;
#endif
}
template <int K>
RK_HD int64_t smulk(int32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    int64_t r;
    asm("v_mad_i64_i32 %0, vcc, %1, %2, 0" : "=v"(r) : "v"(x), "n"(K) : "vcc");
    return r;
#else
    return (int64_t)x * (int64_t)K;
#endif
}

#if defined(__HIP_DEVICE_COMPILE__)
typedef uint32_t sgpr16 __attribute__((ext_vector_type(16)));
typedef sgpr16 __attribute__((aligned(4))) sgpr16_u;   // a scalar load needs dword alignment only
// The chunks are plain loads from the constant address space through a wave-uniform pointer: the compiler selects
// s_load_dwordx16 and, because the load is its own, puts the s_waitcnt before the first read, copy or spill of the
// destination.  An earlier form issued the load from inline asm without a wait and handed the registers back as an
// ordinary "=s" value: the compiler may copy such a value at once (a live-range split), SGPRs with an SMEM load in
// flight have no interlock, and the copy then holds whatever was in the registers before.  That happened in
// hash_rows_multi_kernel at width 24 and showed as digests that changed from run to run once two proofs contended for
// memory.  Nothing in flight is ever a C++ value here.
struct KStream {
    const uint32_t* p;
    sgpr16 cur, nxt;
    static __device__ __forceinline__ sgpr16 chunk(const uint32_t* q) {
        return *(const __attribute__((address_space(4))) sgpr16_u*)(uintptr_t)q;
    }
    __device__ __forceinline__ explicit KStream(const uint32_t* base) : p(base) {
        asm volatile("" : "+s"(p));   // uniform, and opaque: the loads are not merged with the caller's own of *kc
        cur = chunk(p);
        nxt = chunk(p + 16);
    }
    // The pointer and `acc` (the running sum the constant is about to be multiplied into) go through one empty asm
    // statement: the load of the chunk after next cannot be issued before that sum exists, so the compiler neither
    // bunches the loads of several chunks together at the top (2400 constants do not fit the SGPRs) nor loses the
    // overlap of a chunk's latency with the products of the chunk before it.
    template <int POS, class A>
    __device__ __forceinline__ uint32_t get(A& acc) {
        uint32_t c = cur[POS & 15];
        if constexpr ((POS & 15) == 15) {
            cur = nxt;
            asm volatile("" : "+s"(p), "+v"(acc));
            nxt = chunk(p + (POS / 16 + 2) * 16);
        }
        return c;
    }
    __device__ __forceinline__ void drain() {}
};
#else
struct KStream {
    const uint32_t* p;
    explicit KStream(const uint32_t* base) : p(base) {}
    template <int POS, class A>
    uint32_t get(A&) { return p[POS]; }
    void drain() {}
};
#endif

// acc += x * (constant at stream position POS)
template <int POS>
RK_HD void pr_fma(KStream& ks, uint64_t& acc, uint32_t x) {
    uint32_t c = ks.template get<POS>(acc);
    acc = mad_sc(acc, x, c);
}
template <int POS>
RK_HD void pr_sfma(KStream& ks, int64_t& acc, int32_t x) {
    const int32_t c = (int32_t)ks.template get<POS>(acc);
    acc = smad_sc(acc, x, c);
}

// One Poseidon2 instance family: width W (rate W - 8), RP partial rounds, 4x4 block M4K of the
// external layer (0: the Poseidon2 paper's / risc0's, 1: circ(2,3,1,1), Plonky3's MDSMat4).
// risc0's suite is Core<24, 21, 0>; SP1 / Plonky3's BabyBear permutation is Core<16, 13, 1>.
template <int W, int RP, int M4K>
struct Core {
static constexpr int CELLS = W;
static constexpr int RATE = W - 8;
static constexpr int ROUNDS_PARTIAL = RP;
static constexpr int M4_KIND = M4K;

#if defined(RK_P2_DIRECT)
static constexpr int PR_STREAM_USED = ROUNDS_PARTIAL * CELLS;  // one multiplier per cell per round
#else
// blocks of PR_BLOCK rounds, the remainder (RP mod PR_BLOCK rounds) last: 21 = 7 x 3, 13 = 4 x 3 + 1
static constexpr int PR_BLOCK = RK_P2_BLOCK;
static_assert(PR_BLOCK >= 1 && PR_BLOCK <= 3, "the bounds of partial_rounds() are worked out for blocks of up to 3 rounds");
static constexpr int PR_NB = (RP + PR_BLOCK - 1) / PR_BLOCK;
static constexpr int blk_len(int b) { return b < RP / PR_BLOCK ? PR_BLOCK : RP % PR_BLOCK; }
static constexpr int blk_next(int b) { return b + 1 < PR_NB ? blk_len(b + 1) : 1; }
// stream: the entry cells' dot-product constants for block 0, then per block and per cell i >= 1 the
// blk_len multipliers of the cell update and the blk_next - 1 dot-product constants of the next block
static constexpr int blk_off(int b) {
    int n = (CELLS - 1) * (blk_len(0) - 1);
    for (int c = 0; c < b; c++) n += (CELLS - 1) * (blk_len(c) + blk_next(c) - 1);
    return n;
}
static constexpr int PR_STREAM_USED = blk_off(PR_NB);
#endif
static constexpr int PR_STREAM_WORDS = (PR_STREAM_USED + 15) / 16 * 16 + 16;

struct Consts {
    // the instance (Montgomery form), set by the caller
    uint32_t rc_ext[2 * ROUNDS_HALF_FULL * CELLS];
    uint32_t rc_int[ROUNDS_PARTIAL];
    uint32_t diag[CELLS];
    // derived by derive()
    uint32_t rc_ext_in[2 * ROUNDS_HALF_FULL * CELLS];  // rc * scale(round) as the S-box input offset: rc - p after an
                                                       // unsigned state (rounds 0, 4), centred in (-p/2, p/2] otherwise
    uint32_t rc_int_mp[ROUNDS_PARTIAL];                // rc - p
    uint32_t fix[2];                                   // block-end rescale constants 2^(32 (2 - e_end)), plain residues
    uint32_t fix0_nq;                                  // fix[0] * (-p^-1) mod 2^32 (bb::umul_const companion)
    uint32_t fix1_q;                                   // fix[1] * p^-1 mod 2^32 (bb::smul_const companion)
    uint32_t sig0_c, sig0_nq;                          // fix[0] * 2^32 and its companion: entry sum -> Montgomery form
    uint32_t r3_c, r3_nq;                              // 2^96 mod p and its companion: S -> S * 2^32 (direct form)
    // blocked partial rounds (see partial_rounds()), centred representatives |c| <= (p - 1) / 2
    int32_t pr_fix0;                                   // fix[0]: entry cell 0 and entry sum to Montgomery form
    uint32_t pr_fix0_q;                                // its bb::smul_const companion
    int32_t pr_d0;                                     // d_0 (Montgomery residue)
    int32_t pr_r2;                                     // 2^64 mod p: S (plain) -> S * 2^32 inside a REDC
    int32_t pr_r3;                                     // 2^96 mod p: S (plain) -> SM2 = S * 2^64 mod p
    uint32_t pr_r3_q;                                  // its bb::smul_const companion
    int32_t pr_csum[3];                                // c_n * 2^32 mod p, c_n = sum_{i >= 1} d_i^n (n < PR_BLOCK - 1)
    // per-cell multipliers of the partial rounds in the order partial_rounds() consumes them (+ one
    // chunk of padding for the read-ahead)
    uint32_t pr_stream[PR_STREAM_WORDS];
};

// exponent e of the scale 2^(32 e) carried by the state at the S-box input of each full round
// (first block follows the initial external layer + REDC; second block starts from Montgomery form)
static constexpr int scale_exp(int r) {
    constexpr int t[2 * ROUNDS_HALF_FULL] = {0, -7, -56, -399, 1, 0, -7, -56};
    return t[r];
}

static inline void derive(Consts& k) {
    const uint32_t Rm = bb::encode(bb::ONE);  // Montgomery form of the field element 2^32
    const uint32_t Rinv_m = bb::inv(Rm);
    auto rpow = [&](long e) {  // Montgomery form of 2^(32 e)
        return e >= 0 ? bb::pow(Rm, (uint64_t)e) : bb::pow(Rinv_m, (uint64_t)(-e));
    };
    for (int r = 0; r < 2 * ROUNDS_HALF_FULL; r++) {
        // stored residue v = rc * 2^32 (Montgomery form).  The S-box input of round r holds the
        // residue a * 2^(32 e) for the true state a, so the residue to add is rc * 2^(32 e):
        // bb::mul(v, f) = v * f / 2^32 with the residue f = 2^(32 e) = rpow(e - 1).
        uint32_t f = rpow((long)scale_exp(r) - 1);
        const bool after_unsigned = r % ROUNDS_HALF_FULL == 0;  // input in [0, p + 53): offset rc - p
        for (int i = 0; i < CELLS; i++) {
            uint32_t c = bb::mul(k.rc_ext[r * CELLS + i], f);
            // otherwise the input is a signed REDC output, |x| <= p/2 + 53: centred offset, |x + rc| < 2^31
            k.rc_ext_in[r * CELLS + i] = (after_unsigned || c > bb::P / 2) ? c - bb::P : c;
        }
    }
    for (int i = 0; i < ROUNDS_PARTIAL; i++) k.rc_int_mp[i] = k.rc_int[i] - bb::P;
    // a block ends with the state scaled by 2^(32 e_end), e_end = 7 e - 7 for the last round's e;
    // x -> x * K / 2^32 with K = 2^(32 (2 - e_end)) (plain residue) gives Montgomery form
    for (int b = 0; b < 2; b++) {
        long e = scale_exp(b * ROUNDS_HALF_FULL + ROUNDS_HALF_FULL - 1);
        k.fix[b] = bb::decode(rpow(2 - (7 * e - 7)));
    }
    k.fix0_nq = k.fix[0] * (0u - bb::MPRIME);
    k.fix1_q = k.fix[1] * bb::MPRIME;
    k.sig0_c = bb::encode(k.fix[0]);
    k.sig0_nq = k.sig0_c * (0u - bb::MPRIME);
    k.r3_c = bb::encode(bb::encode(bb::ONE));
    k.r3_nq = k.r3_c * (0u - bb::MPRIME);
#if defined(RK_P2_DIRECT)
    // direct partial rounds: round r, cell i multiplies by d_i (Montgomery residue); in round 0 the cells
    // other than 0 still carry the first block's scale, so their multiplier is d_i * fix[0] / 2^32
    int n = 0;
    for (int r = 0; r < ROUNDS_PARTIAL; r++)
        for (int i = 0; i < CELLS; i++) k.pr_stream[n++] = (r == 0 && i > 0) ? bb::mul(k.diag[i], k.fix[0]) : k.diag[i];
#else
    // blocked partial rounds.  Plain field arithmetic here: a value v "carries" 2^32 when v = x 2^32 mod p for
    // the element x (Montgomery form), and a REDC takes one 2^32 away.  The entry cells carry 2^32 / G with
    // G = fix[0] / 2^32 (the first block of full rounds), so whatever multiplies them in block 0 also carries G.
    auto mulp = [](uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)a * b % bb::P); };
    auto cen = [](uint32_t c) { return c > bb::P / 2 ? (int32_t)(c - bb::P) : (int32_t)c; };
    const uint32_t R1 = bb::ONE, R2 = mulp(R1, R1), R3 = mulp(R2, R1), G = bb::decode(k.fix[0]);
    uint32_t pw[CELLS][PR_BLOCK + 1];  // d_i^n, plain
    for (int i = 0; i < CELLS; i++) {
        pw[i][0] = 1;
        for (int m = 1; m <= PR_BLOCK; m++) pw[i][m] = mulp(pw[i][m - 1], bb::decode(k.diag[i]));
    }
    for (int m = 0; m < 3; m++) {
        uint32_t c = 0;
        for (int i = 1; i < CELLS && m < PR_BLOCK; i++) c = (c + pw[i][m]) % bb::P;
        k.pr_csum[m] = cen(mulp(c, R1));
    }
    k.pr_fix0 = cen(k.fix[0]);
    k.pr_fix0_q = (uint32_t)k.pr_fix0 * bb::MPRIME;
    k.pr_d0 = cen(k.diag[0]);
    k.pr_r2 = cen(R2);
    k.pr_r3 = cen(R3);
    k.pr_r3_q = (uint32_t)k.pr_r3 * bb::MPRIME;
    int n = 0;
    auto put = [&](uint32_t c) { k.pr_stream[n++] = (uint32_t)cen(c); };
    // D_j = sum_i d_i^j x_i over the entry cells: the dot products feed a sum that carries 2^32
    for (int i = 1; i < CELLS; i++)
        for (int j = 1; j < blk_len(0); j++) put(mulp(pw[i][j], G));
    for (int b = 0; b < PR_NB; b++) {
        const int K = blk_len(b);
        const uint32_t g = b == 0 ? G : 1;
        for (int i = 1; i < CELLS; i++) {
            put(mulp(mulp(pw[i][K], R1), g));                                // d_i^K x_i: REDC of it carries 2^32
            for (int m = 0; m + 1 < K; m++) put(mulp(pw[i][K - 1 - m], R2));  // d_i^(K-1-m) S_m, S_m plain
            for (int j = 1; j < blk_next(b); j++) put(pw[i][j]);              // the next block's D_j
        }
    }
#endif
    while (n < PR_STREAM_WORDS) k.pr_stream[n++] = 0;
}

// External layer circ(2*M4, M4, ..., M4), M4 = [[5,7,1,3],[4,6,1,1],[1,3,5,7],[1,1,4,6]] (M4K = 0) or
// circ(2,3,1,1) (M4K = 1).  M4 is linear, so M4(y_b) + sum_b' M4(y_b') = M4(y_b + c) with the column sums
// c_j = sum_b y[4b + j]: the layer is  c -> z_i = y_i + c_(i & 3) -> M4(z_b) -> REDC, block by block.  Per round at
// width 24: 24 mads for c, 24 for z, 8 64-bit adds per block, against 60 + 20 + 24 for M4 per block, the sum of
// the M4 outputs over the blocks and that sum added to every cell (RK_P2_EXT_M4_FIRST keeps that form for A/B).  Only
// a block's four z and its M4 temporaries are alive at a time, and a caller that needs some blocks only pays c plus
// those blocks.  w = M_E y is the same exact integer in both forms, so every REDC output is the same 32-bit word.
//
// M4 on exact 64-bit integers.  M4K = 0 follows the Poseidon2 paper's add / double schedule (eight v_lshl_add_u64;
// times 2 and times 4, not shifts: the signed values may be negative); M4K = 1 is the block sum plus z_i + 2 z_(i+1).
template <class T>
static RK_HD void m4_wide(T a, T b, T c, T d, T* w) {
    if constexpr (M4K == 0) {
        T t0 = a + b, t1 = c + d;
        T t2 = b * 2 + t1;  // 2b +  c +  d
        T t3 = d * 2 + t0;  //  a +  b + 2d
        T t4 = t1 * 4 + t3;  //  a +  b + 4c + 6d
        T t5 = t0 * 4 + t2;  // 4a + 6b +  c +  d
        w[0] = t3 + t5;      // 5a + 7b +  c + 3d
        w[1] = t5;
        w[2] = t2 + t4;      //  a + 3b + 5c + 7d
        w[3] = t4;
    } else {
        T sum = (a + b) + (c + d);
        w[0] = (b * 2 + a) + sum;  // 2a + 3b +  c +  d
        w[1] = (c * 2 + b) + sum;  //  a + 2b + 3c +  d
        w[2] = (d * 2 + c) + sum;  //  a +  b + 2c + 3d
        w[3] = (a * 2 + d) + sum;  // 3a +  b +  c + 2d
    }
}

#if defined(RK_P2_EXT_M4_FIRST)
// the earlier forms: M4 per block on the 32-bit cells, then the sum over the blocks added to every cell; the
// template parameters are accepted and ignored (every cell is read and written)
// External layer circ(2*M4, M4, ..., M4), M4 = [[5,7,1,3],[4,6,1,1],[1,3,5,7],[1,1,4,6]], on
// canonical cells, exact: w[i] < 112 p < 2^38.  Then s[i] = w[i] * 2^-32 (mod p) in [0, p + 53).
template <int NZ = CELLS>
static RK_HD void m_ext_redc(uint32_t* s) {
    uint64_t w[CELLS];
#pragma unroll
    for (int i = 0; i < CELLS; i += 4) {
        uint32_t a = s[i], b = s[i + 1], c = s[i + 2], d = s[i + 3];
        uint32_t t0 = a + b, t1 = c + d;                     // < 2p < 2^32
        if constexpr (M4K == 0) {
            uint64_t u1 = madk<1>(t1, madk<6>(b, mulk<4>(a)));  // 4a + 6b +  c +  d
            uint64_t u0 = madk<2>(d, madk<1>(t0, u1));          // 5a + 7b +  c + 3d
            uint64_t u3 = madk<1>(t0, madk<6>(d, mulk<4>(c)));  //  a +  b + 4c + 6d
            uint64_t u2 = madk<2>(b, madk<1>(t1, u3));          //  a + 3b + 5c + 7d
            w[i] = u0; w[i + 1] = u1; w[i + 2] = u2; w[i + 3] = u3;
        } else {  // circ(2, 3, 1, 1): every output is the block sum plus one cell plus twice the next
            uint64_t sum = madk<1>(t1, mulk<1>(t0));
            w[i] = madk<2>(b, madk<1>(a, sum));      // 2a + 3b +  c +  d
            w[i + 1] = madk<2>(c, madk<1>(b, sum));  //  a + 2b + 3c +  d
            w[i + 2] = madk<2>(d, madk<1>(c, sum));  //  a +  b + 2c + 3d
            w[i + 3] = madk<2>(a, madk<1>(d, sum));  // 3a +  b +  c + 2d
        }
    }
    uint64_t t[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        t[j] = w[j];
#pragma unroll
        for (int b = 4; b < CELLS; b += 4) t[j] += w[b + j];
    }
#pragma unroll
    for (int i = 0; i < CELLS; i++) s[i] = bb::uredc64(w[i] + t[i & 3]);
}

// The same layer on signed-lazy cells |y| < p (S-box outputs), exact in int64 (|w| < 112 p), then
// r[i] = w[i] * 2^-32 (mod p) as a signed value, |r| <= p/2 + 53.  M4 follows the Poseidon2 paper's
// add / double schedule: the first two sums and the two doublings take the 32-bit cells through
// v_mad_i64_i32 (sums like a + b do not fit 32 bits here), the rest are 64-bit shift-adds
// (v_lshl_add_u64) -- ten instructions per four cells, against two per CELL for a canonicalisation
// that would let the unsigned form above be used.
template <int B0 = 0, int BN = CELLS / 4>
static RK_HD void m_ext_redc_s(const int32_t* y, int32_t* r) {
    int64_t w[CELLS];
#pragma unroll
    for (int i = 0; i < CELLS; i += 4) {
        int32_t a = y[i], b = y[i + 1], c = y[i + 2], d = y[i + 3];
        int64_t t0 = smadk<1>(b, smulk<1>(a));  //  a +  b
        int64_t t1 = smadk<1>(d, smulk<1>(c));  //  c +  d
        if constexpr (M4K == 0) {
            int64_t t2 = smadk<2>(b, t1);           // 2b +  c +  d
            int64_t t3 = smadk<2>(d, t0);           //  a +  b + 2d
            int64_t t4 = t1 * 4 + t3;               //  a +  b + 4c + 6d (times 4, not << 2: t1 may be negative)
            int64_t t5 = t0 * 4 + t2;               // 4a + 6b +  c +  d
            w[i] = t3 + t5;                         // 5a + 7b +  c + 3d
            w[i + 1] = t5;
            w[i + 2] = t2 + t4;                     //  a + 3b + 5c + 7d
            w[i + 3] = t4;
        } else {  // circ(2, 3, 1, 1)
            int64_t sum = t0 + t1;
            w[i] = smadk<2>(b, smadk<1>(a, sum));
            w[i + 1] = smadk<2>(c, smadk<1>(b, sum));
            w[i + 2] = smadk<2>(d, smadk<1>(c, sum));
            w[i + 3] = smadk<2>(a, smadk<1>(d, sum));
        }
    }
    int64_t t[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        t[j] = w[j];
#pragma unroll
        for (int b = 4; b < CELLS; b += 4) t[j] += w[b + j];
    }
#pragma unroll
    for (int i = 0; i < CELLS; i++) r[i] = bb::redc64(w[i] + t[i & 3]);
}

#else
// The layer on canonical cells, exact: c_j < (W/4) p, z_i < (W/4 + 1) p <= 7p, w_i <= 16 z < 112 p < 2^38.  Then
// s[i] = w[i] * 2^-32 (mod p) in [0, p + 53).  Two canonical cells add in 32 bits (< 2p < 2^32) before they enter
// the 64-bit column sum.  Cells NZ .. W-1 are known to be zero (the capacity of a fresh sponge, the padding of a
// compression): they are neither summed nor added, z_i = c_(i & 3) there.
template <int NZ = CELLS>
static RK_HD void m_ext_redc(uint32_t* s) {
    static_assert(NZ >= 1 && NZ <= CELLS, "NZ leading cells may be non-zero");
    uint64_t c[4];
    static_for<0, 4>([&](auto jc) __attribute__((always_inline)) {
        constexpr int J = decltype(jc)::value;
        constexpr int N = NZ > J ? (NZ - J + 3) / 4 : 0;  // non-zero cells of column J
        uint64_t acc = 0;
        static_for<0, N / 2>([&](auto pc) __attribute__((always_inline)) {
            constexpr int I = 8 * decltype(pc)::value + J;
            const uint32_t pr = s[I] + s[I + 4];
            if constexpr (I == J) acc = pr;
            else acc = madk<1>(pr, acc);
        });
        if constexpr (N % 2 == 1) {
            if constexpr (N == 1) acc = s[J];
            else acc = madk<1>(s[4 * (N - 1) + J], acc);
        }
        c[J] = acc;
    });
#pragma unroll
    for (int i = 0; i < CELLS; i += 4) {
        uint64_t z[4], w[4];
#pragma unroll
        for (int j = 0; j < 4; j++) z[j] = i + j < NZ ? madk<1>(s[i + j], c[j]) : c[j];
        m4_wide<uint64_t>(z[0], z[1], z[2], z[3], w);
#pragma unroll
        for (int j = 0; j < 4; j++) s[i + j] = bb::uredc64(w[j]);
    }
}

// The same layer on signed-lazy cells |y| < p (S-box outputs), exact in int64: |c_j| < (W/4) p, |z_i| < 7p,
// |w_i| < 112 p (49 p for M4K = 1), then r[i] = w[i] * 2^-32 (mod p) as a signed value, |r| <= p/2 + 53.  Sums like
// a + b do not fit 32 bits here, so the cells enter 64 bits through v_mad_i64_i32 (times 1), two per cell; the rest
// is 64-bit shift-adds.  Only the blocks B0 .. B0 + BN - 1 are produced (cells 4 B0 .. 4 (B0 + BN) - 1 of r); the
// column sums still read every cell of y.
template <int B0 = 0, int BN = CELLS / 4>
static RK_HD void m_ext_redc_s(const int32_t* y, int32_t* r) {
    static_assert(B0 >= 0 && BN >= 1 && 4 * (B0 + BN) <= CELLS, "blocks of four cells");
    int64_t c[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        c[j] = smulk<1>(y[j]);
#pragma unroll
        for (int b = 4; b < CELLS; b += 4) c[j] = smadk<1>(y[b + j], c[j]);
    }
#pragma unroll
    for (int i = 4 * B0; i < 4 * (B0 + BN); i += 4) {
        int64_t z[4], w[4];
#pragma unroll
        for (int j = 0; j < 4; j++) z[j] = smadk<1>(y[i + j], c[j]);
        m4_wide<int64_t>(z[0], z[1], z[2], z[3], w);
#pragma unroll
        for (int j = 0; j < 4; j++) r[i + j] = bb::redc64(w[j]);
    }
}
#endif

// (x + c)^7 * 2^(-6*32) as a signed-lazy value, |result| < p.  x + c must fit an int32: x unsigned in
// [0, p + 2^22) with c = rc - p, or x a signed REDC output (|x| <= p/2 + 53) with c centred.
static RK_HD int32_t sbox7_lazy(uint32_t x, uint32_t c_mp) {
    int32_t s = (int32_t)(x + c_mp);
    int32_t s2 = bb::smul(s, s);
    int32_t s3 = bb::smul(s2, s);
    int32_t s6 = bb::smul(s3, s3);
    return bb::smul(s6, s);
}
// One full round on the 32-bit patterns of the cells (unsigned after the first layer / the partial
// rounds, signed otherwise: the offset form of the round constants follows, see derive()).
// Only the blocks B0 .. B0 + BN - 1 of the output are written; the other cells of s are left as they were.
template <int B0 = 0, int BN = CELLS / 4>
static RK_HD void full_round(uint32_t* s, const Consts& k, int r) {
    int32_t y[CELLS], o[CELLS];
#pragma unroll
    for (int i = 0; i < CELLS; i++) y[i] = sbox7_lazy(s[i], k.rc_ext_in[r * CELLS + i]);
    m_ext_redc_s<B0, BN>(y, o);
#pragma unroll
    for (int i = 4 * B0; i < 4 * (B0 + BN); i++) s[i] = (uint32_t)o[i];
}

// Reader of Consts::pr_stream.  On the device the constants live in scalar registers: chunks of
// 16 are fetched one chunk ahead of their use (left to itself the compiler's scheduling of ~2400
// scalar loads spills SGPRs: KStream says where each chunk's load may start, the compiler issues
// it and waits for it).  Positions are consumed strictly in order.
#if defined(RK_P2_DIRECT)
// The partial rounds, one at a time, at three instructions per cell per round.  With S the sum of
// the cells (after the S-box on cell 0) the layer is y_i = d_i x_i + S.  In Montgomery form
// (everything times 2^32) and with SM2 = S * 2^32 (mod p) as a plain 32-bit addend,
//     y_i = REDC(d_i * x_i + SM2) = (d_i x_i + S 2^32) / 2^32
// is one v_mad_u64_u32 whose 64-bit addend is SM2 zero-extended, plus the two instructions of the
// REDC: the addition of S rides inside the reduction, and no canonicalisation is needed because
// the product tolerates any 32-bit x (d_i * x + SM2 + q p < 2^64 for x, SM2 < 2^32 - p).  Per round:
// 17 for the S-box chain of cell 0, 6 to turn the 64-bit sum into SM2 (REDC, then a product by
// 2^96), 3 x CELLS for the cells and CELLS - 1 to accumulate the next sum: 118 at width 24 against
// ~144 for the closed form of round 1 (every round a dot product with constant vectors).
// Entry: signed cells |x| <= p/2 + 53 scaled by the first block (see permute()); exit: Montgomery
// form, canonical.
static RK_HD void partial_rounds(uint32_t* s, const Consts& k) {
    // + p gives non-negative representatives, which is all the unsigned products below need
#pragma unroll
    for (int i = 0; i < CELLS; i++) s[i] += bb::P;
    KStream ks(k.pr_stream);
    // cell 0 feeds an S-box: its true (Montgomery) value, one product by fix[0]
    uint32_t x0 = bb::ucanon(bb::umul_const(s[0], k.fix[0], k.fix0_nq));
    // sum of the other cells: their representatives add up in 64 bits; REDC and one product by
    // fix[0] * 2^32 give the sum in Montgomery form (< 2p)
    uint64_t sig = 0;
#pragma unroll
    for (int i = 1; i < CELLS; i++) sig = bb::acc_u32(sig, s[i]);
    sig = bb::umul_const(bb::uredc64(sig), k.sig0_c, k.sig0_nq);
    static_for<0, ROUNDS_PARTIAL>([&](auto rc) __attribute__((always_inline)) {
        constexpr int R = decltype(rc)::value;
        constexpr int BASE = R * CELLS;
        const uint32_t y0 = bb::canon(sbox7_lazy(x0, k.rc_int_mp[R]));
        const uint64_t S = bb::acc_u32(sig, y0);                                       // < 2^38
        const uint32_t sm2 = bb::umul_const(bb::uredc64(S), k.r3_c, k.r3_nq);          // S * 2^32 mod p, < 2p
        uint64_t t0 = sm2;
        pr_fma<BASE>(ks, t0, y0);
        x0 = bb::ucanon(bb::uredc64(t0));
        uint64_t nsig = 0;
        static_for<1, CELLS>([&](auto ic) __attribute__((always_inline)) {
            constexpr int I = decltype(ic)::value;
            uint64_t t = sm2;
            pr_fma<BASE + I>(ks, t, s[I]);
            s[I] = bb::uredc64(t);  // <= 2p
            nsig = bb::acc_u32(nsig, s[I]);
        });
        sig = nsig;
    });
    s[0] = x0;
#pragma unroll
    for (int i = 1; i < CELLS; i++) s[i] = bb::ucanon(s[i]);
    ks.drain();
}
#else
// The partial rounds in blocks of K = PR_BLOCK rounds.  Round r of the layer, with the internal
// diagonal d:  y = (x_0 + c_r)^7,  S_r = y + sigma_r  (sigma_r = sum_{i >= 1} x_i),  x_0 <- d_0 y + S_r,
// x_i <- d_i x_i + S_r.  Over a block starting at round a, the cells i >= 1 are a fixed linear map of
// their values x_i at the start of the block and of the block's sums:
//     x_i(a + K)   = d_i^K x_i + sum_{m < K} d_i^(K-1-m) S_(a+m)
//     sigma_(a+j)  = D_j + sum_{m < j} c_(j-1-m) S_(a+m),   D_j = sum_{i >= 1} d_i^j x_i,  c_n = sum_{i >= 1} d_i^n
// Cell 0 runs explicitly every round (it feeds the S-box); its sums need D_1 .. D_(K-1), dot products
// over the block's entry values that are accumulated while the previous block writes the cells.  The
// other cells are written once per block: K products by wave-uniform constants and one signed REDC, the
// block's last sum riding inside that REDC as the addend SM2 = S * 2^64 mod p.  At width 24, K = 3:
// 8 instructions per cell per block (3 products, 2 REDC, 1 into the next sum, 2 into the next D)
// against 12 for three direct rounds.
//
// Everything is signed and every constant centred, |c| <= h = (p - 1) / 2; bb::redc64 returns
// |r| <= |t| / 2^32 + p / 2.  Worst-case bounds for K = 3 (W = 24; W = 16 is below them):
//   entry cells |x| <= p/2 + 53 (m_ext_redc_s);  block cells |X| <= 0.979 p < 2^31
//   y = S-box output of x_0 in [0, p) with the offset rc - p: |y| <= 0.934 p
//   D accumulators: terms |c X| <= 2^60.9, bb::fold64 after every 4th, so |D| < 2^62.9 before a fold,
//     < 2^58.5 after the last one
//   sums T_j (64-bit, carry 2^32): |T| < 2^60.5; S_j = REDC(T_j) (plain): |S| <= 1.37 h; |SM2| <= 1.27 h
//   cell 0 before the canonicalisation: |x_0| <= 0.88 p < p (bb::canon needs (-p, p))
//   cell update t = c_K X + sum c S + SM2: |t| < 2^61.9
// (the closed recurrence for |X|: |X'| <= h (|X| + |S_0| + |S_1|) / 2^32 + |SM2| / 2^32 + p/2).
// Exit: Montgomery form, canonical.
static RK_HD void partial_rounds(uint32_t* s, const Consts& k) {
    constexpr int NV = CELLS - 1;
    KStream ks(k.pr_stream);
    // cell 0 feeds an S-box: its true (Montgomery) value, one product by fix[0] (|.| <= 1.24 h)
    uint32_t x0 = bb::canon(bb::smul_const((int32_t)s[0], k.pr_fix0, k.pr_fix0_q));
    // the entry sum: REDC of the raw sum (|.| < 24 p) and one product by fix[0] carry it like y
    int64_t sig = 0;
#pragma unroll
    for (int i = 1; i < CELLS; i++) sig = smadk<1>((int32_t)s[i], sig);
    sig = smul_sc(bb::redc64(sig), k.pr_fix0);
    // D_1 .. D_(K-1) of the first block, over the entry cells
    int64_t D[PR_BLOCK];
    static_for<1, PR_BLOCK>([&](auto jc) __attribute__((always_inline)) { D[decltype(jc)::value] = 0; });
    static_for<1, CELLS>([&](auto ic) __attribute__((always_inline)) {
        constexpr int I = decltype(ic)::value;
        static_for<1, blk_len(0)>([&](auto jc) __attribute__((always_inline)) {
            constexpr int J = decltype(jc)::value;
            pr_sfma<(I - 1) * (blk_len(0) - 1) + J - 1>(ks, D[J], (int32_t)s[I]);
            if constexpr (I % 4 == 0 && I < NV) D[J] = bb::fold64(D[J]);
        });
    });
    static_for<0, PR_NB>([&](auto bc) __attribute__((always_inline)) {
        constexpr int B = decltype(bc)::value;
        constexpr int K = blk_len(B), KN = blk_next(B), R0 = B * PR_BLOCK;
        int32_t sp[PR_BLOCK];
        int64_t sm2 = 0;
        static_for<0, K>([&](auto jc) __attribute__((always_inline)) {
            constexpr int J = decltype(jc)::value;
            const int32_t y = sbox7_lazy(x0, k.rc_int_mp[R0 + J]);
            // T = (y + sigma) 2^32 mod p, 64-bit
            int64_t T;
            if constexpr (J == 0) {
                T = smadk<1>(y, sig);
            } else {
                T = smadk<1>(y, bb::fold64(D[J]));
                static_for<0, J>([&](auto mc) __attribute__((always_inline)) {
                    constexpr int M = decltype(mc)::value;
                    T = smad_sc(T, sp[M], k.pr_csum[J - 1 - M]);
                });
            }
            sp[J] = bb::redc64(T);  // S, plain
            if constexpr (J + 1 < K) {
                x0 = bb::canon(bb::redc64(smad_sc(smul_sc(y, k.pr_d0), sp[J], k.pr_r2)));
            } else {
                sm2 = bb::smul_const(sp[J], k.pr_r3, k.pr_r3_q);
                x0 = bb::canon(bb::redc64(smad_sc(sm2, y, k.pr_d0)));
            }
        });
        // the other cells, the next block's entry sum and its D_j
        int64_t nsig = 0, nD[PR_BLOCK];
        static_for<1, KN>([&](auto jc) __attribute__((always_inline)) { nD[decltype(jc)::value] = 0; });
        static_for<1, CELLS>([&](auto ic) __attribute__((always_inline)) {
            constexpr int I = decltype(ic)::value;
            constexpr int POS = blk_off(B) + (I - 1) * (K + KN - 1);
            int64_t t = sm2;
            pr_sfma<POS>(ks, t, (int32_t)s[I]);
            static_for<0, K - 1>([&](auto mc) __attribute__((always_inline)) {
                constexpr int M = decltype(mc)::value;
                pr_sfma<POS + 1 + M>(ks, t, sp[M]);
            });
            const int32_t v = bb::redc64(t);
            s[I] = (uint32_t)v;
            nsig = smadk<1>(v, nsig);
            static_for<1, KN>([&](auto jc) __attribute__((always_inline)) {
                constexpr int J = decltype(jc)::value;
                pr_sfma<POS + K + J - 1>(ks, nD[J], v);
                if constexpr (I % 4 == 0 && I < NV) nD[J] = bb::fold64(nD[J]);
            });
        });
        sig = nsig;
        static_for<1, KN>([&](auto jc) __attribute__((always_inline)) { D[decltype(jc)::value] = nD[decltype(jc)::value]; });
    });
    s[0] = x0;
#pragma unroll
    for (int i = 1; i < CELLS; i++) s[i] = bb::canon((int32_t)s[i]);
    ks.drain();
}
#endif

// The permutation.  A caller that reads only the cells KEEP0 .. KEEP0 + KEEPN - 1 of the result (whole blocks of
// four: the digest 0..7, the capacity W-8..W-1 of a sponge whose next block overwrites the rate) says so, and one
// whose input cells NZ .. W-1 are zero says that: the last full round is then peeled out of its rolled loop and its
// layer produces the kept blocks only (column sums, then z, M4 and REDC for those blocks), and the first layer skips
// the zero cells.  The kept cells are word for word those of the full form; the other cells of s are unspecified.
// The defaults are the full form: every cell written, no input assumed zero.
template <int KEEP0 = 0, int KEEPN = CELLS, int NZ = CELLS>
static RK_HD void permute(uint32_t* s, const Consts& k) {
    static_assert(KEEP0 % 4 == 0 && KEEPN % 4 == 0 && KEEP0 >= 0 && KEEPN >= 4 && KEEP0 + KEEPN <= CELLS, "kept cells are whole blocks");
    m_ext_redc<NZ>(s);  // canonical Montgomery input -> plain residues (scale 2^0), cells in [0, p + 53)
#pragma unroll 1
    for (int r = 0; r < ROUNDS_HALF_FULL; r++) full_round(s, k, r);
    // signed cells (|x| <= p/2 + 53) scaled by 2^(32 * -2800): partial_rounds() owns the scale
    partial_rounds(s, k);  // Montgomery form again, canonical
    if constexpr (KEEPN == CELLS) {
#pragma unroll 1
        for (int r = ROUNDS_HALF_FULL; r < 2 * ROUNDS_HALF_FULL; r++) full_round(s, k, r);
    } else {
#pragma unroll 1
        for (int r = ROUNDS_HALF_FULL; r < 2 * ROUNDS_HALF_FULL - 1; r++) full_round(s, k, r);
        full_round<KEEP0 / 4, KEEPN / 4>(s, k, 2 * ROUNDS_HALF_FULL - 1);
    }
    // per-cell rescale to Montgomery form + canonical range, kept cells only
#pragma unroll
    for (int i = KEEP0; i < KEEP0 + KEEPN; i++) s[i] = bb::canon(bb::smul_const((int32_t)s[i], (int32_t)k.fix[1], k.fix1_q));
}

};  // struct Core

// risc0's instance under the names the rest of the library grew up with
using C24 = Core<24, 21, 0>;
constexpr int CELLS = C24::CELLS;
constexpr int RATE = C24::RATE;
constexpr int ROUNDS_PARTIAL = C24::ROUNDS_PARTIAL;
using Consts = C24::Consts;
inline void derive(Consts& k) { C24::derive(k); }
RK_HD void permute(uint32_t* s, const Consts& k) { C24::permute(s, k); }

}  // namespace p2
