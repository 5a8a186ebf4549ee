/* raiko_hip.h -- C ABI of libraiko_hip.so, the MI355X (gfx950) STARK proving
 * backend for raiko's risc0 block-proof path.
 *
 * Boundary being replaced (reference = Champii/raiko @ 2024-08-07):
 *   - plugin level:   `trait Prover { run, cancel }`        lib/src/prover.rs:52-62
 *                     `Risc0Prover::run`                    provers/risc0/driver/src/lib.rs:56-112
 *                     `prove_locally` -> `session.prove()`  provers/risc0/driver/src/bonsai.rs:230-272
 *   - operator level: `risc0_zkp::hal::Hal` of risc0-zkp 1.0.1 (Cargo.lock:7243), the trait
 *                     risc0's own CUDA/Metal backends implement; that crate is not vendored
 *                     in the reference, so each entry point cites the trait method by name.
 *
 * Rules of the ABI: plain pointers and sizes only; every function returns
 * RK_OK (0) or a negative rk_status and never aborts; `d_` pointers are device
 * memory of the ctx's GPU; work is asynchronous on the ctx stream unless the
 * function returns data to the host (those synchronise the stream).  A ctx is
 * used by one thread at a time; different ctxs, also of one GPU, run concurrently
 * (rk_prove_session does exactly that).
 * All field elements are BabyBear Montgomery residues (u32 < p = 15*2^27+1);
 * extension elements are 4 consecutive u32; digests are 8 consecutive u32.
 * Matrices are column-major: element (row r, column c) at c*rows + r.
 */
#ifndef RAIKO_HIP_H
#define RAIKO_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    RK_OK = 0,
    RK_ERR_INVALID = -1,   /* bad argument (size not a power of two, null pointer, ...) */
    RK_ERR_HIP = -2,       /* a HIP runtime call failed; see rk_last_error */
    RK_ERR_NOMEM = -3,
    RK_ERR_NODEVICE = -4,
    RK_ERR_CAPACITY = -5,  /* caller-provided output buffer too small */
    RK_ERR_INTERNAL = -6,  /* a prover invariant failed (non-zero remainder in the DEEP division) */
    RK_ERR_VERIFY = -7,    /* rk_prove_session: a produced seal did not pass rk_verify_segment */
    RK_ERR_CALLBACK = -8   /* a circuit hook (rk_circuit_hooks) returned non-zero */
} rk_status;

typedef struct rk_ctx rk_ctx;

/* ---- library / device management ---- */
int rk_abi_version(void);
const char* rk_strerror(int status);
const char* rk_last_error(rk_ctx* ctx);            /* detail text of the last RK_ERR_HIP */
int rk_device_count(int* count);
/* stream = a hipStream_t the caller owns (e.g. torch's current stream) or NULL for a private one */
int rk_ctx_create(int device, void* stream, rk_ctx** out);
int rk_ctx_destroy(rk_ctx* ctx);
int rk_sync(rk_ctx* ctx);
int rk_alloc(rk_ctx* ctx, size_t bytes, void** d_ptr);
int rk_free(rk_ctx* ctx, void* d_ptr);
int rk_h2d(rk_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int rk_d2h(rk_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);

/* Poseidon2 t=24 constants, Montgomery form: 192 external round constants (8 rounds x 24),
 * 21 internal round constants, 24 internal-diagonal entries.  Defaults are compiled in. */
int rk_set_poseidon2_params(rk_ctx* ctx, const uint32_t* rc_ext, const uint32_t* rc_int, const uint32_t* diag);

/* ---- the parameter blob: everything instance-specific about the proof system in one place ----
 * (the same kernels serve risc0's parameter set and SP1 / Plonky3's;
 * presets carry the RECALLED values of both, any field can be overridden.)  Field elements in the
 * blob are CANONICAL integers except the Poseidon2 tables, which are Montgomery residues like
 * every buffer of the ABI.  rk_set_params validates (ext_w a non-residue, root of exact order
 * 2^27, shapes in range), rebuilds the context's twiddle / shift tables and replaces its
 * Poseidon2 instance; RK_ERR_INVALID leaves the context unchanged. */
typedef enum { RK_PRESET_RISC0 = 0, RK_PRESET_SP1 = 1 } rk_preset;
typedef struct {
    uint32_t struct_size;        /* = sizeof(rk_params): guards against a caller built for another layout */
    /* field */
    uint32_t ext_w;              /* extension Fp[x]/(x^4 - ext_w): p - 11 (risc0: x^4 + 11), 11 (Plonky3: x^4 - 11) */
    uint32_t root_2_27;          /* generator of the 2^27 subgroup: 137 (risc0), 0x1a427a41 (Plonky3) */
    uint32_t coset_shift;        /* shift of the zk / LDE coset: 3 (risc0), 31 (Plonky3) */
    /* Poseidon2 */
    uint32_t p2_width;           /* 24 (rate 16, R_P 21) or 16 (rate 8, R_P 13); R_F = 8, x^7, digest = 8 cells */
    uint32_t p2_m4;              /* 4x4 block of the external layer: 0 = [[5,7,1,3],[4,6,1,1],[1,3,5,7],[1,1,4,6]]
                                  * (Poseidon2 paper, risc0), 1 = circ(2,3,1,1) (Plonky3 MDSMat4) */
    uint32_t p2_pad_free;        /* sponge: 0 = zero-pad the last partial block (risc0), 1 = padding-free overwrite
                                  * (Plonky3 PaddingFreeSponge: cells beyond the input keep their values) */
    const uint32_t* p2_rc_ext;   /* 8 * p2_width external round constants; NULL = derived defaults */
    const uint32_t* p2_rc_int;   /* 21 or 13 internal round constants; NULL = derived defaults */
    const uint32_t* p2_diag;     /* p2_width internal-diagonal entries (matrix 1 1^T + diag); NULL = defaults */
    /* protocol */
    uint32_t queries;            /* 50 (risc0), 100 (SP1 core) */
    uint32_t blowup_log2;        /* 2 (risc0), 1 (SP1 core); 1..4.  The LDE domain of a segment has 2^(po2 + blowup_log2)
                                  * points, the check polynomial 4 * 2^blowup_log2 columns, hooks see that domain */
    uint32_t fri_fold_log2;      /* 4 (risc0), 1 (Plonky3): FRI folds by 2^fri_fold_log2 per round (1..4) */
    uint32_t fri_min_degree;     /* 256 (risc0), 1 (Plonky3: down to a constant): folding stops at this many coefficients */
    uint32_t pow_bits;           /* 0 (risc0), 16 (SP1 core): proof-of-work bits ground before the queries are drawn
                                  * (rk_pow_grind), 0..24 */
} rk_params;
int rk_params_preset(rk_params* out, int preset);
int rk_set_params(rk_ctx* ctx, const rk_params* params);
int rk_get_params(rk_ctx* ctx, rk_params* out);    /* pointers in *out refer to the context's own copies */

/* ---- Hal trait operators (risc0-zkp 1.0.1 hal/mod.rs `trait Hal`) ---- */
/* Alignment: the five entry points below (interpolate, evaluate, zk_shift, expand-into-evaluate, bit reverse) accept
 * device pointers that are only word (4-byte) aligned, e.g. a slice t[1:] of a tensor: the NTTs then take the
 * general passes instead of the 2^18 .. 2^22 fused kernels, with the same result.  Entry points that take
 * extension-element buffers (`_ext` arguments) read them with 16-byte loads and need 16-byte aligned pointers. */
/* Hal::batch_interpolate_ntt: `count` columns of `size` natural-order evaluations ->
 * bit-reversed coefficients, in place. */
int rk_batch_interpolate_ntt(rk_ctx* ctx, uint32_t* d_io, size_t size, size_t count);
/* Hal::batch_evaluate_ntt: bit-reversed coefficients -> natural-order evaluations, in place. */
int rk_batch_evaluate_ntt(rk_ctx* ctx, uint32_t* d_io, size_t size, size_t count, uint32_t expand_bits);
/* Hal::zk_shift: io[col][i] *= 3^bitrev(i). */
int rk_zk_shift(rk_ctx* ctx, uint32_t* d_io, size_t size, size_t count);
/* Hal::batch_expand_into_evaluate_ntt: zero-extend `in_size` bit-reversed coefficients to
 * in_size << expand_bits and evaluate (natural order out). */
int rk_batch_expand_into_evaluate_ntt(rk_ctx* ctx, uint32_t* d_out, const uint32_t* d_in, size_t in_size,
                                      size_t count, uint32_t expand_bits);
/* Hal::batch_bit_reverse */
int rk_batch_bit_reverse(rk_ctx* ctx, uint32_t* d_io, size_t size, size_t count);
/* Hal::hash_rows: one Poseidon2 sponge digest per row of a column-major rows x cols matrix. */
int rk_hash_rows(rk_ctx* ctx, uint32_t* d_out_digests, const uint32_t* d_matrix, size_t rows, size_t cols);
/* Hal::hash_fold: nodes[out_size + i] = H(nodes[2*(out_size+i)], nodes[2*(out_size+i)+1]), i < out_size. */
int rk_hash_fold(rk_ctx* ctx, uint32_t* d_nodes, size_t input_size, size_t output_size);
/* Hal::batch_evaluate_any: out[e] = sum_k coeffs[which[e]*size + k] * xs[e]^k (host arrays for
 * which/xs/out: they are transcript-sized). */
int rk_batch_evaluate_any(rk_ctx* ctx, const uint32_t* d_coeffs, size_t poly_count, size_t size,
                          const uint32_t* h_which, const uint32_t* h_xs, size_t eval_count, uint32_t* h_out);
/* Hal::mix_poly_coeffs: out[combos[i]*count + idx] += mix_start * mix^i * in[i*count + idx]. */
int rk_mix_poly_coeffs(rk_ctx* ctx, uint32_t* d_out_ext, const uint32_t mix_start[4], const uint32_t mix[4],
                       const uint32_t* d_in, const uint32_t* h_combos, size_t input_size, size_t count);
/* Hal::eltwise_* */
int rk_eltwise_add_elem(rk_ctx* ctx, uint32_t* d_out, const uint32_t* d_a, const uint32_t* d_b, size_t n);
int rk_eltwise_sum_extelem(rk_ctx* ctx, uint32_t* d_out, const uint32_t* d_in_ext, size_t count, size_t to_add);
int rk_eltwise_copy_elem(rk_ctx* ctx, uint32_t* d_out, const uint32_t* d_in, size_t n);
int rk_eltwise_zeroize_elem(rk_ctx* ctx, uint32_t* d_io, size_t n);
/* Hal::fri_fold: fold of 4 coefficient planes by 2^fri_fold_log2 of the context's parameters
 * (16 by default; bit-reversed order in and out). */
int rk_fri_fold(rk_ctx* ctx, uint32_t* d_out, const uint32_t* d_in, size_t out_count, const uint32_t mix[4]);
/* Plonky3's FRI fold (p3-fri `fold_even_odd`, RECALLED; SP1's arity-2 fold works on evaluations, risc0's
 * rk_fri_fold on coefficients): d_in_ext = 2 * n_out extension elements (4 consecutive words each), the
 * evaluations of p over the subgroup of order 2 * n_out in bit-reversed order; d_out_ext = the n_out evaluations
 * of p_even + beta * p_odd over the squared subgroup, bit-reversed:
 *   out[i] = (p(x) + p(-x)) / 2 + beta * (p(x) - p(-x)) / (2 x),   x = g^bitrev(i). */
int rk_fri_fold_evals(rk_ctx* ctx, uint32_t* d_out_ext, const uint32_t* d_in_ext, size_t n_out, const uint32_t beta[4]);
/* Hal::gather_sample: dst[g] = src[g*stride + idx], g < size. */
int rk_gather_sample(rk_ctx* ctx, uint32_t* d_dst, const uint32_t* d_src, size_t idx, size_t size, size_t stride);

/* Hal::prefix_products: in-place inclusive running product of `count` extension elements
 * (io[i] = io[0] * ... * io[i]); the grand-product accumulator of the accum group. */
int rk_prefix_products(rk_ctx* ctx, uint32_t* d_io_ext, size_t count);
/* Hal::scatter: for cycle c < n_cycles and k in [h_index[c], h_index[c+1]):
 * d_into[h_offsets[k]] = h_values[k] (witness-generation helper; index has n_cycles + 1 entries,
 * the host arrays are copied before the call returns; a later entry wins over an earlier one
 * with the same offset).  Offsets >= into_words are rejected with RK_ERR_INVALID. */
int rk_scatter(rk_ctx* ctx, uint32_t* d_into, size_t into_words, const uint32_t* h_index, size_t n_cycles,
               const uint32_t* h_offsets, const uint32_t* h_values);

/* Proof of work on the transcript (Plonky3 challenger `grind` / `check_witness`, restated on this
 * library's Poseidon2 transcript; risc0 has none): the smallest nonce w (a field element written as the
 * u32 < p it is stored as) such that after absorbing hash([w]) the next random_bits(bits) are all
 * zero.  sponge_cells = the transcript generator's p2_width state words right after a commit.  One
 * lane per candidate, two permutations each. */
int rk_pow_grind(rk_ctx* ctx, const uint32_t* sponge_cells, uint32_t bits, uint32_t* nonce);

/* ---- fused building blocks (no single Hal counterpart) ---- */
/* MerkleTreeProver::new (risc0-zkp prove/merkle.rs): hash_rows + every hash_fold level into
 * d_nodes (2*rows digests, heap order, root at index 1). */
int rk_merkle_build(rk_ctx* ctx, uint32_t* d_nodes, const uint32_t* d_matrix, size_t rows, size_t cols);
/* ---- mixed-matrix commitment: Plonky3's MerkleTreeMmcs (p3-merkle-tree `MerkleTree::new`, RECALLED; what
 * SP1 commits a shard's per-chip traces with -- provers/sp1/driver/src/lib.rs:48-57 reaches it through
 * sp1-sdk) on this library's Poseidon2 sponge and 2-to-1 compression ----
 * Matrices of different power-of-two heights, row-major (element (r, c) at r * width + c, Plonky3's
 * RowMajorMatrix) or column-major, in one tree: the leaves are the hashes of the concatenated rows of
 * the tallest matrices (given order); going up, a level whose size equals the height of further
 * matrices takes them in -- node = compress(compress(left, right), hash(concatenated rows of those
 * matrices)).  d_nodes: 2 * H digests in heap order (H = largest height; leaves at H + i, root at 1). */
typedef struct {
    const uint32_t* d_values;      /* device */
    uint32_t height;               /* power of two */
    uint32_t width;
    uint32_t row_major;            /* 1: (r, c) at r * width + c; 0: at c * height + r; 2: at c * height + bitrev(r) -- a column-major
                                    * matrix whose columns are in NATURAL order while the committed rows are the bit-reversed
                                    * ones (Plonky3 commits `lde.bit_reverse_rows()`): the evaluations exactly as the NTT leaves
                                    * them, no reordering pass */
} rk_matrix;
int rk_mmcs_commit(rk_ctx* ctx, const rk_matrix* mats, uint32_t n_mats, uint32_t* d_nodes, uint32_t h_root[8]);
/* Mmcs::open_batch at leaf `index` of the tallest matrices: row (index >> log2(H / height)) of every
 * matrix, concatenated in the given order into h_rows (sum of widths words), and the log2(H) sibling
 * digests from the leaf level up into h_path. */
int rk_mmcs_open(rk_ctx* ctx, const rk_matrix* mats, uint32_t n_mats, const uint32_t* d_nodes, uint32_t index,
                 uint32_t* h_rows, uint32_t* h_path);
/* Mmcs::verify_batch on the host (no GPU): heights / widths of the matrices in commit order, the opened rows
 * and path, against `root`.  params NULL = risc0's Poseidon2 instance.  0 = accepted, 1 = rejected. */
int rk_mmcs_verify(const rk_params* params, const uint32_t* heights, const uint32_t* widths, uint32_t n_mats,
                   uint32_t index, const uint32_t* rows, const uint32_t* path, const uint32_t root[8]);

/* ---- Plonky3 two-adic FRI PCS, the data-parallel steps (SP1: provers/sp1/driver/src/lib.rs:48-57 -> sp1-core ->
 * p3-fri TwoAdicFriPcs::commit / open; RECALLED, the crates are outside the reference tree).  Matrices are
 * row-major height x width; coset shift, 2-adic generator, extension and blow-up come from rk_set_params. ----
 * commit: `coset_lde_batch(evals, log_blowup, shift).bit_reverse_rows()`: d_in = evaluations of `width` polynomials
 * over the subgroup of order `height` (natural order); d_out = (height << blowup_log2) x width, row r = their values
 * at shift * g^bitrev(r), g generating the larger subgroup.  Feed d_out to rk_mmcs_commit. */
int rk_pcs_coset_lde_rows(rk_ctx* ctx, uint32_t* d_out, const uint32_t* d_in, size_t height, size_t width);
/* open: the opened values of one committed matrix at the extension point z (`interpolate_coset` on the LDE's low
 * coset, i.e. its first lde_height >> blowup_log2 rows): d_out_ext = width extension elements p_c(z). */
int rk_pcs_eval_at(rk_ctx* ctx, uint32_t* d_out_ext, const uint32_t* d_lde, size_t lde_height, size_t width, const uint32_t z[4]);
/* the same for n_points (<= 4) points in one pass over the low coset (a trace is opened at zeta and zeta * g):
 * h_points = n_points x 4 words, d_out_ext = n_points x width extension elements, point-major. */
int rk_pcs_eval_at_many(rk_ctx* ctx, uint32_t* d_out_ext, const uint32_t* d_lde, size_t lde_height, size_t width, uint32_t n_points,
                        const uint32_t* h_points);
/* open, "reduce rows": for the n_points (<= 8) opening points of one matrix, h_points = n_points x 4 words and
 * h_opened = n_points x width x 4 words (the values rk_pcs_eval_at returned),
 *   d_ro_ext[r] += alpha^(alpha_offset + j * width) * (sum_c alpha^c M[r][c] - sum_c alpha^c opened_j[c]) / (x_r - z_j)
 * over all rows r and points j, x_r = shift * g^bitrev(r).  d_ro_ext (lde_height extension elements, one vector per
 * matrix height, zeroed by the caller) is what the FRI commit phase folds with rk_fri_fold_evals. */
int rk_pcs_reduce_openings(rk_ctx* ctx, uint32_t* d_ro_ext, const uint32_t* d_lde, size_t lde_height, size_t width, uint32_t n_points,
                           const uint32_t* h_points, const uint32_t* h_opened, const uint32_t alpha[4], uint64_t alpha_offset);
/* The same three steps for hosts that can keep the LDE the way the NTT leaves it -- `width` columns of
 * height << blowup_log2 evaluations in NATURAL order, i.e. rk_matrix layout 2 (row_major = 2: committed row r at index
 * bitrev(r) of every column).  rk_mmcs_commit / rk_mmcs_open take that layout as it is; the values returned here are those
 * of the row-major forms above (same d_out_ext, same d_ro_ext indexed by committed row).  No pass exists only to reorder:
 * a 2^20 x 256 LDE costs 3.4 ms instead of 5.0 (rk_p3_prove works this way). */
int rk_pcs_coset_lde_cols(rk_ctx* ctx, uint32_t* d_cols, const uint32_t* d_in_rows, size_t height, size_t width);
int rk_pcs_eval_at_many_cols(rk_ctx* ctx, uint32_t* d_out_ext, const uint32_t* d_lde_cols, size_t lde_height, size_t width, uint32_t n_points,
                             const uint32_t* h_points);
int rk_pcs_reduce_openings_cols(rk_ctx* ctx, uint32_t* d_ro_ext, const uint32_t* d_lde_cols, size_t lde_height, size_t width, uint32_t n_points,
                                const uint32_t* h_points, const uint32_t* h_opened, const uint32_t alpha[4], uint64_t alpha_offset);
/* `challenger.grind(bits)` of Plonky3's DuplexChallenger (p3-challenger, RECALLED): sponge_state = the challenger's
 * `width` state cells (Montgomery words), input_buffer = its n_input (< rate = width - 8) buffered observations.
 * *witness = the smallest field element w (canonical integer) for which observing w and then sample_bits(bits) gives
 * zero: w joins the inputs, they overwrite the first cells, one permutation, the last rate cell is the sample.
 * Plonky3 accepts any such w (`find_any`); the smallest is returned so that the result is reproducible. */
int rk_duplex_grind(rk_ctx* ctx, const uint32_t* sponge_state, const uint32_t* input_buffer, uint32_t n_input, uint32_t bits,
                    uint32_t* witness);

/* synthetic division of one extension polynomial (count coefficients, natural order) by (x - z),
 * in place (core/poly.rs poly_divide); the remainder f(z) goes to h_rem (4 words, may be NULL). */
int rk_poly_divide(rk_ctx* ctx, uint32_t* d_polys_ext, size_t count, const uint32_t z[4], uint32_t* h_rem);

/* ---- whole-segment prover (Prover::commit_group/finalize + fri_prove of risc0-zkp 1.0.1) ---- */
typedef struct {
    uint32_t group_size[3];        /* columns per register group: 0 accum, 1 code, 2 data */
    uint32_t n_regs;               /* registers sorted by (group, offset); must cover every column once */
    const uint32_t* reg_group;
    const uint32_t* reg_offset;
    const uint32_t* reg_combo;
    uint32_t n_combos;
    const uint32_t* combo_off;     /* n_combos + 1 prefix offsets into combo_backs */
    const uint32_t* combo_backs;
} rk_taps;

/* ---- circuit hooks: the two places where a segment proof depends on Fiat-Shamir randomness that
 * exists only after earlier groups are committed (risc0-circuit-rv32im 1.0.1 prove/mod.rs
 * prove_segment + risc0-zkp prove/prover.rs finalize; CircuitHal::accumulate / eval_check) ----
 *   1. after code and data are committed the prover draws n_accum_mix field elements and calls
 *      `accumulate`, which fills the accum group from them and the witness;
 *   2. after accum is committed it draws poly_mix and calls `eval_check`, which evaluates the
 *      circuit's mixed constraint polynomial over the 4N-point LDE domain.
 * Hooks run on the thread that called rk_prove_segment (a prover thread of rk_prove_session),
 * may call rk_* operators on view->ctx, must enqueue their device work on view->stream and must
 * not synchronise other streams; they return 0 or non-zero (-> RK_ERR_CALLBACK). */
typedef struct {
    rk_ctx* ctx;
    void* stream;                  /* hipStream_t of ctx */
    uint32_t po2;
    uint32_t group_size[3];        /* 0 accum, 1 code, 2 data */
    const uint32_t* d_trace[3];    /* device, column-major 2^po2 x group_size[g]: the witness as handed in
                                    * ([1], [2]; valid in `accumulate` only, NULL otherwise) */
    const uint32_t* d_lde[3];      /* device, column-major 4*2^po2 x group_size[g]: evaluations on the coset
                                    * 3*w^i, natural order (PolyGroup::evaluated); NULL until committed.
                                    * (4 = 2^blowup_log2, 3 = coset_shift of the context's rk_params).
                                    * READ-ONLY, as the type says: d_lde[1] may be the LDE of a code-cache entry
                                    * (rk_code_cache_configure) that other proofs in flight read too */
    const uint32_t* globals;       /* host */
    uint32_t n_globals;
    const uint32_t* mix;           /* host: the n_accum_mix elements drawn before the accum commit */
    uint32_t n_mix;
} rk_circuit_view;
typedef struct rk_program rk_program;   /* a circuit's constraint polynomial as data, see below */
typedef struct {
    void* user;
    /* CircuitHal::accumulate: write the accum group, column-major 2^po2 x group_size[0], to d_accum */
    int (*accumulate)(void* user, const rk_circuit_view* view, uint32_t* d_accum);
    /* CircuitHal::eval_check: write 4 x 4*2^po2 values (component e of point i at e*4*2^po2 + i):
     * sum_k poly_mix^k * constraint_k at x_i = 3*w^i, divided by (x_i^(2^po2) - 1) */
    int (*eval_check)(void* user, const rk_circuit_view* view, const uint32_t poly_mix[4], uint32_t* d_check);
    /* used when eval_check is NULL: the library evaluates the step program on the GPU
     * (rk_program_eval_check) -- no circuit-specific kernel needed */
    const rk_program* program;
} rk_circuit_hooks;

/* ---- the constraint polynomial as data: risc0-zkp 1.0.1 adapter.rs `PolyExtStepDef` ----
 * risc0 ships every circuit's mixed constraint polynomial as a list of steps over two growing
 * value lists (RECALLED from the crate; it is outside the reference tree): field values
 * (CONST / GET / GET_GLOBAL / ADD / SUB / MUL push one) and mix states {tot, mul} (TRUE /
 * AND_EQZ / AND_COND push one); operands are positions in the list of their kind:
 *   CONST a            value a (a canonical integer)
 *   GET a              tap a: eval_u[a] (rk_poly_ext_fn's order: registers by (group, offset), backs in combo order)
 *   GET_GLOBAL a b     args[a][b]: a = 0 the segment's globals, a = 1 the accum mix
 *   ADD|SUB|MUL a b    field values a, b
 *   TRUE               {tot 0, mul 1}
 *   AND_EQZ a b        x = mix state a, v = field value b:   {x.tot + x.mul * v,  x.mul * poly_mix}
 *   AND_COND a b c     x = mix state a, cond = field value b, inner = mix state c:
 *                      {x.tot + cond * inner.tot * x.mul,  x.mul * inner.mul}
 * and `ret` names the mix state whose tot is the result.  The verifier interprets the list on the
 * tap openings (CircuitDef::poly_ext); risc0's eval_check kernels are the same list turned into
 * straight-line code by its build.  Here the list is an operand: rk_program_create validates it,
 * drops dead steps, folds every `mul` into a compile-time power of poly_mix, assigns the live
 * intermediate values to reusable slots, and the result serves both sides --
 * rk_program_eval_check runs it for all 4 * 2^po2 points of the LDE domain on the GPU (one point per
 * lane, slots in LDS, the step list read through the scalar cache), rk_program_poly_ext runs it on
 * extension elements on the host.  tools/circuit_gen.py turns the same list into straight-line HIP
 * (what risc0's build does) when the interpreter's per-step overhead matters. */
typedef enum {
    RK_STEP_CONST = 0, RK_STEP_GET = 1, RK_STEP_GET_GLOBAL = 2, RK_STEP_ADD = 3, RK_STEP_SUB = 4, RK_STEP_MUL = 5,
    RK_STEP_TRUE = 6, RK_STEP_AND_EQZ = 7, RK_STEP_AND_COND = 8
} rk_step_op;
typedef struct { uint32_t op, a, b, c; } rk_poly_step;
typedef struct {
    uint64_t n_steps;          /* as given */
    uint64_t n_ops;            /* arithmetic steps left after dead-code elimination (what a point costs) */
    uint32_t n_fp_slots;       /* slots the live field values need at the same time */
    uint32_t n_mix_slots;      /* ... and the live mix states (4 words each) */
    uint32_t n_consts;         /* distinct constants */
    uint32_t n_mix_powers;     /* distinct powers of poly_mix */
    uint32_t max_power;        /* the highest of them = number of constraints on the longest path */
    uint32_t n_taps;           /* taps of the tap set it was created against */
} rk_program_info;
/* taps: the tap set the GET indices refer to (copied).  RK_ERR_INVALID for an operand that names a
 * value not yet pushed, a tap / argument list that does not exist, or an unknown op. */
int rk_program_create(const rk_poly_step* steps, size_t n_steps, uint32_t ret, const rk_taps* taps, rk_program** out);
int rk_program_destroy(rk_program* prog);
int rk_program_get_info(const rk_program* prog, rk_program_info* out);
/* CircuitHal::eval_check from the program, on view->ctx / view->stream (what the prover calls for
 * hooks with `program` set; a hook of the caller's may call it too) */
int rk_program_eval_check(const rk_program* prog, const rk_circuit_view* view, const uint32_t poly_mix[4],
                          uint32_t* d_check);
/* Optional: turn the list into a gfx950 code object for ctx's GPU now (straight-line HIP generated from the list
 * -- what tools/circuit_gen.py emits at build time -- compiled with hiprtc; seconds for 10^4 steps).  From then on
 * rk_program_eval_check on that GPU runs the generated kernel (about 3x the interpreter's speed) instead of the
 * interpreter; results are identical.  RK_ERR_HIP with the compiler's log in rk_last_error if it cannot be
 * built -- the interpreter stays in charge.
 * With RK_JIT_CACHE_DIR set, the code object is kept there under a name derived from the generated source, the
 * architecture and the hiprtc version, and loaded instead of compiled the next time (a host restart then costs
 * milliseconds, not the ~20 s of a 30 k-step list). */
int rk_program_compile(rk_program* prog, rk_ctx* ctx);
/* the HIP source rk_program_compile hands to the compiler (NUL-terminated; *length without the NUL;
 * RK_ERR_CAPACITY with *length set when `out` is too small) */
int rk_program_source(const rk_program* prog, char* out, size_t capacity, size_t* length);
/* CircuitDef::poly_ext from the program (host): the value rk_poly_ext_fn returns.  ext_w: canonical W
 * of the extension (rk_params.ext_w; 0 = risc0's) */
int rk_program_poly_ext(const rk_program* prog, uint32_t ext_w, const uint32_t poly_mix[4], const uint32_t* eval_u_ext,
                        size_t n_taps, const uint32_t* globals, uint32_t n_globals, const uint32_t* mix, uint32_t n_mix,
                        uint32_t out_ext[4]);

typedef struct {
    uint32_t po2;                  /* segment has 2^po2 rows */
    uint32_t on_device;            /* 0: group[] and check are host pointers; 1: device pointers, left untouched
                                    * (the prover works on a copy); 2: device pointers the prover may overwrite */
    rk_taps taps;
    const uint32_t* group[3];      /* trace evaluations, column-major 2^po2 x group_size[g] */
    const uint32_t* check;         /* eval_check output: 4 x 4*2^po2 evaluations (CircuitHal::eval_check) */
    const uint32_t* globals;       /* host, n_globals elements */
    uint32_t n_globals;
    uint32_t n_accum_mix;          /* Fiat-Shamir elements drawn before the accum group is committed */
    uint8_t proof_system_info[16];
    uint8_t circuit_info[16];
    const rk_circuit_hooks* hooks; /* NULL: group[0] and check are taken as given (pre-computed stand-ins).
                                    * A non-NULL `accumulate` replaces group[0], a non-NULL `eval_check`
                                    * replaces check (the replaced pointer is ignored and may be NULL) */
} rk_segment;

/* Produces the seal (the u32 Fiat-Shamir transcript) of one segment. */
int rk_prove_segment(rk_ctx* ctx, const rk_segment* seg, uint32_t* h_seal, size_t seal_capacity_words,
                     size_t* seal_words);
/* Host-side verifier (no GPU needed): the counterpart of `receipt.verify()` the reference calls
 * after proving (provers/risc0/driver/src/lib.rs:136, benchmark.rs:19); restates risc0-zkp
 * verify/{mod,fri,merkle}.rs for the flow of rk_prove_segment.  Reads only the public part of
 * `pub` (po2, taps, globals, n_accum_mix, infos).  Returns 0 for a valid seal, RK_ERR_INVALID for
 * malformed arguments, a positive reason code otherwise (see verify.hip).  The circuit's
 * constraint identity is NOT checked (no rv32im circuit in this repo). */
int rk_verify_segment(const rk_segment* pub, const uint32_t* seal, size_t seal_words);
/* The same with options.  p2_*: the Poseidon2 instance the seal was produced under (all three or
 * none; none = the compiled-in defaults, which is what rk_verify_segment assumes).  poly_ext:
 * CircuitDef::poly_ext -- the circuit's mixed constraint polynomial on the tap openings; when
 * given, the verifier also checks the constraint identity
 *     poly_ext(poly_mix, eval_u, globals, mix) == check(z) * ((3z)^(2^po2) - 1)
 * (reason code 70 on mismatch; the same with `program` in place of the callback).  eval_u holds one extension element per tap, registers in
 * (group, offset) order, each register's backs in combo order: the value of the register's
 * polynomial at 3*z*w^-back. */
typedef int (*rk_poly_ext_fn)(void* user, const rk_segment* pub, const uint32_t poly_mix[4], const uint32_t* eval_u_ext,
                              size_t n_taps, const uint32_t* mix, uint32_t n_mix, uint32_t out_ext[4]);
typedef struct {
    const uint32_t* p2_rc_ext;     /* 192 */
    const uint32_t* p2_rc_int;     /* 21 */
    const uint32_t* p2_diag;       /* 24 */
    rk_poly_ext_fn poly_ext;
    void* user;
    const rk_program* program;     /* used when poly_ext is NULL: the constraint identity from the step program */
    const rk_params* params;       /* optional: the parameter blob the seal was produced under (field, Poseidon2
                                    * instance incl. width 16, queries); overrides the three p2_* pointers */
} rk_verify_opts;
int rk_verify_segment_ex(const rk_segment* pub, const rk_verify_opts* opts, const uint32_t* seal, size_t seal_words);
/* Upper bound on the seal size for a given shape (0 for a shape rk_prove_segment rejects), for up to
 * RK_MAX_QUERIES queries' worth of openings when called without parameters. */
size_t rk_seal_bound_words(const rk_segment* seg);
size_t rk_seal_bound_words_for(const rk_segment* seg, uint32_t queries);
/* the same for a whole parameter set (queries, blow-up, fold arity, final degree, proof of work) */
size_t rk_seal_bound_words_params(const rk_segment* seg, const rk_params* params);
#define RK_MAX_QUERIES 256

/* ---- whole-session prover: what replaces `session.prove()` (provers/risc0/driver/src/bonsai.rs:271,
 * which proves the segments one after the other) ----
 * Proves segs[0..n) on one GPU with `inflight` segments in flight (one prover context, HIP stream
 * and host thread each, taken from a shared index) and, for host-resident segments
 * (on_device == 0), one more context that uploads `upload_ahead` segments ahead into a ring of
 * device buffers, so the PCIe transfer runs under the previous proofs.  With `verify` != 0 every
 * seal is checked with rk_verify_segment on one more host thread while the GPU goes on.  Seal i goes to
 * h_seals[i] (capacity seal_capacity_words[i], e.g. rk_seal_bound_words), its length to
 * seal_words[i].  Returns RK_OK or the first failure (RK_ERR_VERIFY for a seal that does not
 * verify) with the segment's index in *failed_index; rk_session_last_error gives the detail.
 * Contexts and staging buffers persist per device for the life of the process (the reference's
 * `Prover` has no `self`: lib/src/prover.rs:52-62); concurrent calls for one device are
 * serialised.  rk_session_release frees them. */
typedef struct {
    int device;        /* the GPU, when n_devices == 0 */
    int inflight;      /* per GPU, 1..16; 3 is where an MI355X saturates at 2^20-cycle segments */
    int upload_ahead;  /* per GPU, 0..16 staged segments waiting for a prover; 2 hides a 20 ms upload */
    int verify;        /* 0: no verification; 1: verify every seal (the library picks up to 4 host threads);
                        * 2..16: that many verifier threads */
    const int* devices; /* optional list of distinct GPUs of this node: every GPU's prover contexts take
                         * segments from ONE shared index (a work queue: a short last segment or a slower
                         * GPU does not stall the others), seals land in the caller's host buffers, so a
                         * single-process host needs no collective */
    int n_devices;      /* 0: use `device` */
    const rk_verify_opts* verify_opts; /* optional, for verify != 0 */
    const rk_params* params;    /* optional: the parameter set of this session's proofs (and of their verification,
                                 * unless verify_opts carries its own); NULL = risc0's.  The device's contexts are
                                 * re-parameterised only when the set differs from the previous session's */
} rk_session_opts;
int rk_prove_session(const rk_session_opts* opts, const rk_segment* segs, size_t n, uint32_t* const* h_seals,
                     const size_t* seal_capacity_words, size_t* seal_words, size_t* failed_index);
/* The same for a session whose segments arrive while it runs (risc0's executor can yield segments one by one:
 * `run_with_callback`): segment k is proven while the executor is still producing segment k + 1.  A worker thread
 * proves whatever has been submitted since its last look as one rk_prove_session batch.  The rk_segment is copied at
 * submit; what it points at, the seal buffer and *seal_words must stay valid until rk_stream_close returns -- which
 * waits for everything submitted, frees the stream, and returns RK_OK or the first failure with the index (in
 * submission order) in *failed_index.  opts as for rk_prove_session (devices / params / verify_opts are copied;
 * tables a params blob points at stay the caller's). */
typedef struct rk_stream rk_stream;
int rk_stream_open(const rk_session_opts* opts, rk_stream** out);
int rk_stream_submit(rk_stream* stream, const rk_segment* seg, uint32_t* h_seal, size_t seal_capacity_words, size_t* seal_words);
/* Back-pressure for hosts whose sessions are larger than memory (the reference keeps segments on disk for that reason:
 * segment_path, bonsai.rs:261-266): blocks until at most max_pending submitted segments are unfinished (or one has
 * failed: the status so far is returned), and reports in *finished_prefix how many segments from the start of the
 * submission order are done -- their inputs and everything their rk_segment pointed at may be freed, their seals and
 * seal_words are final.  A host submits segment k, waits with max_pending = inflight + upload_ahead, frees what the
 * prefix has released, and only then generates the witness of segment k + 1. */
int rk_stream_wait(rk_stream* stream, size_t max_pending, size_t* finished_prefix);
int rk_stream_close(rk_stream* stream, size_t* failed_index);
const char* rk_session_last_error(int device);
/* how many segments `device` proved in the last session it took part in (the balance of the work queue) */
int rk_session_last_proven(int device, size_t* count);
int rk_session_release(void);
/* ---- the code group's commitment, cached per device ----
 * The code (control) columns depend on the circuit and po2 alone, so every segment of one size commits the same code
 * group.  rk_prove_segment (and with it every session entry point) fingerprints the code input it is given where it
 * lies in device memory -- every word, on every call: a keyed 123-bit hash, never the address -- and when the device
 * already holds the group committed from the same words under the same po2, column count, blow-up, query count, field
 * and Poseidon2 instance, it reuses coefficients, LDE, Merkle tree and top layer: the seal is word for word the one a
 * recomputation gives.  An entry costs 36 * cols * 2^po2 + 256 * 2^po2 bytes at blow-up 4 (576 MiB for 16 columns at
 * po2 20) of device memory outside every context's pool, is shared by all contexts of the device and outlives them;
 * least recently used entries go when max_bytes would be exceeded.  With the cache on, an on_device = 2 code buffer is
 * left untouched.  Inputs with a word >= p or of more than 2^28 words are committed the ordinary way.
 * rk_code_cache_configure: max_bytes of `device` (default 2 GiB, or RK_CODE_CACHE_BYTES from the environment, read
 * once); 0 switches the cache off and frees its entries.  rk_code_cache_stats: lookups that hit / missed since the
 * process started and the bytes held now (any pointer may be NULL).  rk_session_release drops the entries too. */
int rk_code_cache_configure(int device, size_t max_bytes);
int rk_code_cache_stats(int device, uint64_t* hits, uint64_t* misses, uint64_t* bytes);
/* Test switch: with RK_TEST_LOGICAL_DEVICES=k in the environment the session entry points see k devices, logical
 * device d running on physical GPU d mod (number of GPUs) -- the multi-device path (a pool, a feeder and `inflight`
 * provers per device, session-wide claim flags, pinning of device-resident segments to the first device of the GPU
 * that holds them) on a box with one GPU.  Not for production: the devices share one GPU's memory and time. */

/* ---- the one collective of the path, for hosts that run one process per GPU (raiko's own single-process
 * host needs none: rk_prove_session writes every seal into the caller's buffers) ----
 * Rank r proves global segments r, r + world, ... and the ranks exchange the variable-length seals with two
 * ncclAllGather calls over RCCL (xGMI inside a node): a length table, then padded payloads.  RCCL is looked up at run
 * time (librccl.so.1); RK_ERR_NODEVICE when it is not there.  rk_comm_unique_id is called by one rank, the 128 bytes go to
 * the others out of band (a file, MPI, the launcher's store), every rank then calls rk_comm_create. */
typedef struct rk_comm rk_comm;
#define RK_COMM_ID_BYTES 128
int rk_comm_unique_id(uint8_t id[RK_COMM_ID_BYTES]);
int rk_comm_create(const uint8_t id[RK_COMM_ID_BYTES], int rank, int world, int device, rk_comm** out);
int rk_comm_destroy(rk_comm* comm);
const char* rk_comm_last_error(rk_comm* comm);
/* h_local_seals / local_words: this rank's n_local seals in the order it proved them (segments rank, rank + world, ...;
 * n_local must be that count for n_total).  On return EVERY rank has out_words[i] for all i < n_total and, where h_out and
 * h_out[i] are given, seal i copied into h_out[i] (RK_ERR_CAPACITY if out_capacity[i] is too small; the others are
 * still delivered). */
int rk_gather_seals(rk_comm* comm, const uint32_t* const* h_local_seals, const size_t* local_words, size_t n_local, size_t n_total,
                    uint32_t* const* h_out, const size_t* out_capacity, size_t* out_words);
/* the host half of the gather: the gathered length table (world x per_rank words) and padded payloads
 * (world x per_rank x max_len words) into segment order */
int rk_gather_unpack(const uint32_t* all_lens, const uint32_t* all_payload, int world, size_t per_rank, size_t max_len, size_t n_total,
                     uint32_t* const* h_out, const size_t* out_capacity, size_t* out_words);

/* ---- RV32IM executor + segmenter: the step before the path ----
 * `ExecutorImpl::from_elf(env, elf).run()` (provers/risc0/driver/src/bonsai.rs:267-269): interprets a
 * 32-bit RISC-V ELF (RV32I + M) and cuts the run into segments of at most 2^segment_limit_po2
 * cycles (bonsai.rs:249), each with the machine-state digests before and after it.  Host code.
 * NOT risc0's: the cycle model (one cycle per instruction), the ecall table (t0 selects:
 * RK_ECALL_HALT a0 = exit code; RK_ECALL_READ a0 = word-aligned destination, a1 = capacity in
 * words -> a0 = words taken from input_words; RK_ECALL_COMMIT a0 = source, a1 = bytes appended to
 * the journal) and the state digest (Poseidon2 over pc, registers and touched pages).  The
 * rv32im witness layout is outside this repo: a segment carries bounds and digests, not columns. */
typedef struct rk_exec rk_exec;
enum { RK_ECALL_HALT = 0, RK_ECALL_READ = 1, RK_ECALL_COMMIT = 2 };
enum { RK_EXIT_HALTED = 0, RK_EXIT_SYSTEM_SPLIT = 2 };
typedef struct {
    uint32_t struct_size;          /* = sizeof(rk_exec_opts) */
    uint32_t segment_limit_po2;    /* 13..24 */
    uint64_t session_limit;        /* total cycles allowed, 0 = no limit (session_limit(None), bonsai.rs:248) */
    const uint32_t* input_words;   /* env.write_slice(&encoded_input), bonsai.rs:250 */
    size_t n_input_words;
    uint32_t record_trace;         /* keep every executed cycle (28 bytes each) for rk_exec_witness */
    uint32_t profile;              /* count executed cycles per pc (rk_exec_profile): what the reference switches on with
                                    * `profile: true` -> env_builder.enable_profiler(..), bonsai.rs:252-255 */
} rk_exec_opts;
typedef struct {
    uint64_t total_cycles;
    uint32_t n_segments;
    uint32_t exit_code;            /* a0 of the halting ecall */
    size_t journal_bytes;
    size_t input_words_read;
    int status;                    /* RK_OK, or why the run stopped (the segments before it stay readable) */
} rk_exec_summary;
typedef struct {
    uint32_t index;
    uint32_t po2;                  /* smallest power of two >= cycles, at least 13 */
    uint64_t cycles;
    uint32_t start_pc, end_pc;
    uint32_t exit;                 /* RK_EXIT_SYSTEM_SPLIT for every segment but the last */
    uint32_t pre_state[8], post_state[8];   /* post_state of segment i == pre_state of segment i + 1 */
} rk_exec_segment;
/* *out is set also when the run traps (status < 0): read rk_exec_error, then rk_exec_free */
int rk_exec_elf(const uint8_t* elf, size_t elf_bytes, const rk_exec_opts* opts, rk_exec** out);
/* the same one segment at a time (risc0's `run_with_callback` shape): a host can hand segment k to the prover
 * while segment k + 1 executes.  rk_exec_open loads the ELF (input words are copied), every
 * rk_exec_next_segment runs up to the next boundary; *more = 0 once the guest has halted. */
int rk_exec_open(const uint8_t* elf, size_t elf_bytes, const rk_exec_opts* opts, rk_exec** out);
int rk_exec_next_segment(rk_exec* ex, int* more);
int rk_exec_summary_get(const rk_exec* ex, rk_exec_summary* out);
int rk_exec_segment_get(const rk_exec* ex, uint32_t index, rk_exec_segment* out);
int rk_exec_journal(const rk_exec* ex, uint8_t* out, size_t capacity, size_t* len);
/* the cycle profile of a run made with rk_exec_opts.profile: distinct program counters and the cycles spent at each,
 * most expensive first; *n = how many there are (RK_ERR_CAPACITY when more than `capacity`: call again) */
int rk_exec_profile(const rk_exec* ex, uint32_t* pcs, uint64_t* cycles, size_t capacity, size_t* n);
/* Witness generation for the STAND-IN trace circuit (not rv32im's: that layout is in a crate outside the
 * reference tree).  Columns of executed segment `index`, column-major 2^po2 rows, Montgomery form, every 32-bit
 * machine word as two 16-bit field elements; needs rk_exec_opts.record_trace:
 *   code (RK_TRACE_CODE_COLS = 2):   0 first-row selector, 1 last-row selector
 *   data (RK_TRACE_DATA_COLS = 16):  0/1 pc lo/hi, 2/3 next pc lo/hi, 4/5 instruction lo/hi, 6 seq (next = pc + 4),
 *                                    7 carry of pc_lo + 4, 8/9 rs1 value, 10/11 rs2 value, 12/13 value written to rd,
 *                                    14 rd written, 15 active (0 on the padding rows after the last cycle)
 * The constraints a proof over them checks (raiko_amd/circuit_program.py trace_program): flags are bits, a seq row
 * advances pc by 4 with the stated carry, every row starts where the previous one went, padding is final, the
 * segment's first and last pc are the public ones.  Limb ranges, instruction decoding, registers and memory are
 * NOT constrained: this is the witness path exercised end to end, not a zkVM. */
#define RK_TRACE_CODE_COLS 2
#define RK_TRACE_DATA_COLS 16
int rk_exec_witness(const rk_exec* ex, uint32_t index, uint32_t* code, uint32_t* data);
/* The two tables the data columns look values up in when the segment is proven as a uni-stark shard with lookups
 * (rk_air_create_lookup; raiko_amd/executor.py p3_trace_air(lookups=True)) -- what SP1's cpu chip has in its program and
 * range chips.  Row-major Montgomery words, ready to be an rk_p3_table's trace:
 *   range_table    65536 x 2: (v, how often v occurs among the ten 16-bit limbs -- pc, next pc, rs1, rs2, rd value -- of
 *                  the executed cycles)
 *   program_table  rows x 5: (pc lo, pc hi, instruction lo, instruction hi, cycles spent there), the distinct pairs in
 *                  ascending order, zero-padded to a power of two >= 2
 * *program_rows: in = the capacity of program_table in rows, out = the rows needed (RK_ERR_CAPACITY when it did not fit,
 * nothing written: call again).  Needs rk_exec_opts.record_trace. */
int rk_exec_lookup_tables(const rk_exec* ex, uint32_t index, uint32_t* range_table, uint32_t* program_table, size_t* program_rows);
/* the same columns written on the GPU into device buffers (2 and 16 columns of 2^po2 words), asynchronously on the
 * ctx stream: only the executed cycles (28 bytes each) cross PCIe; the trace has been copied when the call returns.
 * Hand the buffers to rk_prove_segment / a session as on_device inputs after rk_sync(ctx). */
int rk_exec_witness_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_code, uint32_t* d_data);
/* the 16 data columns as ONE row-major matrix (2^po2 rows x RK_TRACE_DATA_COLS words) in device memory: the form an
 * on_device rk_p3_table takes (the execution proven as uni-stark shards: raiko_amd/executor.py p3_trace_air) */
int rk_exec_witness_device_rows(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_rows);
/* The machine's registers x0..x31 at the start and at the end of executed segment `index` (32 words each). */
int rk_exec_registers(const rk_exec* ex, uint32_t index, uint32_t* start, uint32_t* end);
/* The ecall rows of segment `index` (needs record_trace): *n pairs (cycle within the segment, a0 after the call) in
 * cycle order.  An ecall READ writes a0 outside the trace row (whose rd written flag stays 0); the rv32i chip set treats
 * every ecall row as a write of x10 with this value.  The executor traps every other word of the SYSTEM opcode (ebreak,
 * rd != 0, ...), so the rows of word 0x00000073 are all the SYSTEM rows a trace holds.  RK_ERR_CAPACITY with *n set when
 * more than `capacity` pairs. */
int rk_exec_ecalls(const rk_exec* ex, uint32_t index, uint32_t* out, size_t capacity, size_t* n);
/* THE RV32I CHIP SET: segment `index` as the five tables of a uni-stark shard whose AIRs constrain the register file
 * and the integer ALU (raiko_amd/rv32.py builds the same tables in numpy, names every column and writes the AIRs):
 *   cpu       2^po2 x RK_RV32_CPU_COLS: the 16 data columns above at the same places, the decoded fields, three register
 *             accesses per row at timestamps 3 row + 1 / 2 / 3 (read rs1, read rs2, write the destination) with their
 *             previous timestamps, operand / carry / borrow / sign / byte columns of the ALU
 *   program   program_rows x RK_RV32_PROGRAM_COLS: one row per word of the executed pc range, the fields decoded from
 *             its 32 bits (which the program AIR proves from those bits) and how often the shard ran it
 *   register  RK_RV32_REGISTER_ROWS x RK_RV32_REGISTER_COLS: every register's initial value at timestamp 0 and final
 *             (value, timestamp), bound to the shard's public values by shift registers
 *   byte      2^RK_RV32_BYTE_LOG_ROWS x RK_RV32_BYTE_COLS: (op, x, y, x op y) for AND / OR / XOR of bytes, with counts
 *   range     65536 x 2: (v, count) over the 16-bit limbs the cpu rows send
 * Row-major Montgomery words in device memory, ready to be on_device rk_p3_tables.  Registers follow an offline memory
 * argument on a REGISTER bus.  CONSTRAINED: the value written by ADD, SUB, ADDI, AND, OR, XOR, ANDI, ORI, XORI, SLT,
 * SLTU, SLTI, SLTIU, LUI, AUIPC and the link value of JAL / JALR.  FREE: results of shifts, of the M extension and of
 * loads; branch and jump decisions and targets; memory (a store is two register reads); the a0 an ecall leaves.
 * Written on the GPU from the executed cycles (28 bytes each) and the ecall side list; the host does no per-cycle work.
 * Needs record_trace.  rk_exec_rv32_sizes: the program table's rows (a power of two >= 2).  rk_exec_rv32_shard_device
 * runs on the ctx stream and returns when the tables are complete; RK_ERR_CAPACITY when program_rows is not the size
 * rk_exec_rv32_sizes gives or the executed pc range is wider than 2^22 words, RK_ERR_INVALID when one pc ran two
 * different instruction words in the segment. */
#define RK_RV32_CPU_COLS 68
#define RK_RV32_PROGRAM_COLS 77
#define RK_RV32_REGISTER_COLS 131
#define RK_RV32_REGISTER_ROWS 32
#define RK_RV32_BYTE_COLS 24
#define RK_RV32_BYTE_LOG_ROWS 18
int rk_exec_rv32_sizes(const rk_exec* ex, uint32_t index, size_t* program_rows);
int rk_exec_rv32_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_cpu, uint32_t* d_program,
                              size_t program_rows, uint32_t* d_register, uint32_t* d_byte, uint32_t* d_range);
/* THE RV32I-CF CHIP SET: rv32i's five tables with the control flow and the shifts constrained as well, plus a sixth
 * (raiko_amd/rv32cf.py builds the same tables in numpy, names every column and writes the AIRs):
 *   cpu       2^po2 x RK_RV32CF_CPU_COLS: columns 0..67 the rv32i row above, word for word; then the decoded branch /
 *             jump / shift selectors and the branch or jump offset, the branch decision's difference, borrow and
 *             equality columns, the next pc's carries and dropped bit, the shift amount's decomposition, the shifted
 *             operand's bytes with their shift-table parts and the assembled result
 *   program   program_rows x RK_RV32CF_PROGRAM_COLS: columns 0..76 the rv32i row, then the twelve fields above
 *   register, byte, range   as for rv32i
 *   shift     2^RK_RV32CF_SHIFT_LOG_ROWS x RK_RV32CF_SHIFT_COLS: (k, x, lo, hi) with x 2^k = lo + 256 hi for k in 0..8
 *             and x in 0..255 (2304 rows, the rest the tuple (0, 0, 0, 0)), with counts and bit decompositions
 * CONSTRAINED: everything rv32i constrains; the next pc of every row (pc + imm_B on a taken branch, pc + imm_J on JAL,
 * (rs1 + imm_I) & ~1 on JALR, pc + 4 otherwise); the decision of BEQ, BNE, BLT, BGE, BLTU, BGEU; the value written by
 * SLL, SRL, SRA, SLLI, SRLI, SRAI.  FREE: results of the M extension and of loads; memory (LB, LH, LW, LBU, LHU, SB, SH,
 * SW); the a0 an ecall leaves.  Sizes, errors and stream behaviour as for rk_exec_rv32_shard_device. */
#define RK_RV32CF_CPU_COLS 121
#define RK_RV32CF_PROGRAM_COLS 89
#define RK_RV32CF_SHIFT_COLS 38
#define RK_RV32CF_SHIFT_LOG_ROWS 12
int rk_exec_rv32cf_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_cpu, uint32_t* d_program,
                                size_t program_rows, uint32_t* d_register, uint32_t* d_byte, uint32_t* d_range,
                                uint32_t* d_shift);
/* THE RV32IM CHIP SET: rv32i-cf's six tables with the M extension constrained as well, plus a seventh
 * (raiko_amd/rv32im.py builds the same tables in numpy, names every column and writes the AIRs):
 *   cpu       2^po2 x RK_RV32IM_CPU_COLS: columns 0..120 the rv32i-cf row above, word for word; then IS_MUL .. IS_REMU and
 *             their sum IS_M (looked up in the program table), the op (funct3) and M_W = IS_M * WR, the multiplicity of
 *             the row's (op, rs1 value, rs2 value, result) send to the muldiv table
 *   program   program_rows x RK_RV32IM_PROGRAM_COLS: columns 0..88 the rv32i-cf row, then the nine fields above and the
 *             three partial products of the funct7 = 0000001 test
 *   register, byte, range, shift   as for rv32i-cf (the counts include the muldiv table's lookups)
 *   muldiv    muldiv_rows x RK_RV32IM_MULDIV_COLS: one row per cpu row with M_W = 1, in execution order, then padding
 *             rows of multiplicity 0: the op, operands and result, their byte limbs, the 64-bit product (or q b + r) with
 *             its carries, sign bits, the b = 0 and overflow flags and the remainder bound's magnitudes
 * CONSTRAINED: everything rv32i-cf constrains; the result of MUL / MULH / MULHSU / MULHU / DIV / DIVU / REM / REMU with
 * the RISC-V conventions for b = 0 and -2^31 / -1.  FREE: loads, stores and memory; the a0 an ecall leaves.
 * rk_exec_rv32im_sizes: the muldiv table's rows for segment `index` (2^max(RK_RV32IM_MULDIV_MIN_LOG_ROWS, ceil(log2
 * count))).  rk_exec_rv32im_shard_device takes any power of two from that up to 2^po2 as muldiv_rows: RK_ERR_CAPACITY
 * (nothing written, nothing launched) when it is smaller, RK_ERR_INVALID when it is not a power of two or taller;
 * otherwise sizes, errors and stream behaviour as for rk_exec_rv32_shard_device. */
#define RK_RV32IM_CPU_COLS 132
#define RK_RV32IM_PROGRAM_COLS 101
#define RK_RV32IM_MULDIV_COLS 78
#define RK_RV32IM_MULDIV_MIN_LOG_ROWS 1
int rk_exec_rv32im_sizes(const rk_exec* ex, uint32_t index, size_t* muldiv_rows);
int rk_exec_rv32im_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, uint32_t* d_cpu, uint32_t* d_program,
                                size_t program_rows, uint32_t* d_register, uint32_t* d_byte, uint32_t* d_range,
                                uint32_t* d_shift, uint32_t* d_muldiv, size_t muldiv_rows);
/* THE RV32IM-ELF CHIP SET: rv32im's statement with the program bound to the ELF (raiko_amd/rv32elf.py builds the same
 * tables in numpy and writes the AIRs).  What a shard cannot change is PREPROCESSED -- committed once per ELF by
 * rk_p3_setup into a key, whose root names the program to the verifier -- and a shard's trace keeps what it decides:
 *   cpu, register, muldiv   rv32im's tables, word for word
 *   program   preprocessed RK_RV32ELF_PROGRAM_PREP_COLS columns per word of the program image: the 41 fields an rv32im
 *             cpu row looks up, in that order, and VALID (1 where a cpu row may look the word up); trace: 1 column, how
 *             often the shard ran the word.  The one constraint: count * (1 - VALID) = 0
 *   byte      preprocessed (op, x, y, x op y), 2^RK_RV32_BYTE_LOG_ROWS rows; trace: the count
 *   range     preprocessed v = 0 .. 65535; trace: the count
 *   shift     preprocessed (k, x, lo, hi), 2^RK_RV32CF_SHIFT_LOG_ROWS rows; trace: the count
 * THE PROGRAM IMAGE: the words of every PT_LOAD segment with PF_X set and file bytes, in program-header order, each
 * segment's file bytes zero-padded to whole words; its rows are padded to a power of two >= 2 with the row of word 0 at
 * pc 0.  rk_exec_program_image lists it with the loader's own walk of the program headers (host only): *n_segs /
 * *n_words are set whenever the file is well formed, RK_ERR_CAPACITY when either buffer is too small (call again) or
 * the file has more than RK_RV32ELF_MAX_SEGMENTS executable segments, RK_ERR_INVALID for a file rk_exec_open refuses, a
 * misaligned executable segment or executable segments that overlap.
 * WHAT SETUP IS TRUSTED FOR: rv32im proves every decoded field from the word's bits inside each proof; here the decode
 * is done once, by rk_rv32elf_prep_device, outside any proof.  A verifier trusts a root exactly as far as it trusts
 * whoever derived it from the ELF.  In exchange every executed (pc, word) is a row of that image -- a pc outside it or a
 * word a store changed cannot be proven -- and all shards of a run answer to one root.
 * CONSTRAINED / FREE: as rv32im (free: loads, stores and memory; the a0 an ecall leaves).
 * rk_rv32elf_prep_device: the four preprocessed matrices, row-major Montgomery words, written on the ctx stream into
 * device buffers of program_rows x 42, 2^18 x 4, 2^16 x 1 and 2^12 x 4 words (seg_vaddr / seg_words / words: host
 * memory, as rk_exec_program_image gives them); returns when they are complete: hand them to rk_p3_setup as on_device
 * matrices.  program_rows must be the power of two >= max(2, n_words): RK_ERR_CAPACITY otherwise; more than
 * RK_RV32ELF_MAX_SEGMENTS segments or seg_words that do not sum to n_words: RK_ERR_INVALID; both before any launch.
 * rk_exec_rv32elf_shard_device: segment `index` as the seven traces -- rv32im's cpu, register and muldiv tables and the
 * four count columns (program_rows, 2^18, 2^16, 2^12 words) -- by rv32im's pipeline: a cycle is counted at the image row
 * of its pc and its word compared with d_image_words (the image's words in device memory, n_words of them in segment
 * order).  RK_ERR_INVALID when a cycle ran a pc outside the image or a word that is not the image's; sizes, capacities
 * (program_rows as above, muldiv_rows as rk_exec_rv32im_shard_device) and stream behaviour as for
 * rk_exec_rv32im_shard_device: everything is refused before the first launch when a size is wrong. */
#define RK_RV32ELF_MAX_SEGMENTS 16
#define RK_RV32ELF_PROGRAM_PREP_COLS 42
int rk_exec_program_image(const uint8_t* elf, size_t elf_bytes, uint32_t* seg_vaddr, uint32_t* seg_words, size_t seg_capacity,
                          size_t* n_segs, uint32_t* words, size_t word_capacity, size_t* n_words);
int rk_rv32elf_prep_device(rk_ctx* ctx, const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs,
                           const uint32_t* words, size_t n_words, uint32_t* d_program, size_t program_rows, uint32_t* d_byte,
                           uint32_t* d_range, uint32_t* d_shift);
int rk_exec_rv32elf_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, const uint32_t* seg_vaddr,
                                 const uint32_t* seg_words, uint32_t n_segs, const uint32_t* d_image_words, uint32_t* d_cpu,
                                 uint32_t* d_program_mult, size_t program_rows, uint32_t* d_register, uint32_t* d_byte_mult,
                                 uint32_t* d_range_mult, uint32_t* d_shift_mult, uint32_t* d_muldiv, size_t muldiv_rows);
/* THE RV32IM-MEM CHIP SET: rv32im-elf's statement with loads, stores and memory constrained WITHIN A SHARD
 * (raiko_amd/rv32mem.py builds the same tables in numpy, names every column and writes the AIRs).  Keyed like rv32im-elf
 * and proven through rk_p3_prove_shards_key; nine tables, rv32im-elf's seven in their order, then memop and memory:
 *   cpu       2^po2 x RK_RV32MEM_CPU_COLS: columns 0..131 the rv32im row, word for word; then IS_LOAD, IS_STORE, MEM_OP
 *             (funct3 + 8 IS_STORE), MIMM_LO / MIMM_HI (imm_I of a load, imm_S of a store) and IS_SYS (looked up), the
 *             multiplicities M_MEM = IS_LOAD WR + IS_STORE ACTIVE and N_ECW (the words the row's ecall wrote) and
 *             EC_OP = 16 IS_SYS.  A row sends (MEM_OP, TSA, A, MIMM, B, RES) M_MEM times and (EC_OP, TSA) N_ECW times
 *   program   preprocessed RK_RV32MEM_PROGRAM_PREP_COLS columns: rv32im-elf's 41 fields, the six above, VALID (rv32im-elf's,
 *             and 0 on a LOAD / STORE word whose funct3 the executor traps); trace: the count
 *   register, byte, range, shift, muldiv   as for rv32im-elf (the counts include the lookups of memop and memory)
 *   memop     memop_rows x RK_RV32MEM_MEMOP_COLS: one row per recorded access (rk_exec_mem_accesses) in list order, then
 *             padding rows (ONE = 1, the rest 0): the op one-hot, the cpu row's tuple, the address sum with its carries and
 *             split into word address and byte offset, the bytes of the word before and after and of rs2, the selected
 *             byte / half, its sign bit, the previous access's timestamp and the difference's limbs
 *   memory    memory_rows x RK_RV32MEM_MEMORY_COLS: one row per distinct touched word in ascending address order: (WL, WH,
 *             INIT lo / hi, FINAL lo / hi, FTS, REAL, GL, GH, WL4, SAME, FINV), the word address as WL + 2^14 WH (WL, 4 WL and
 *             WH range-checked), the distance to the next row's address limb by limb (SAME and GL when the high limbs
 *             agree, GH otherwise) and the inverse of FTS (a real row was touched); then rows of zeros.  THE BOUNDARY
 *             TABLE: what a link between shards would bind
 * CONSTRAINED: everything rv32im-elf constrains; the value LB / LH / LW / LBU / LHU write and the word SB / SH / SW leave,
 * against one history per word inside the shard.  FREE: INIT of every touched word (the boundary to the previous shard
 * and to the ELF's data image; the link below binds it), what an ecall writes, the a0 it leaves (the io form below binds
 * both).
 * rk_exec_mem_accesses: the access list of segment `index` (needs record_trace): *n entries of four words (cycle within
 * the segment, word address addr >> 2, word before, word after) in cycle order -- one per store, one per load whose rd is
 * not x0 (after = before) and one per word an ecall READ wrote, at the ecall's cycle in ascending address order.
 * Instruction fetch and the reads of an ecall COMMIT are not recorded.  RK_ERR_CAPACITY with *n set when more than
 * `capacity` entries.
 * rk_exec_rv32mem_sizes: the rows of the memop and the memory table (2^max(RK_RV32MEM_MIN_LOG_ROWS, ceil(log2 count)));
 * RK_ERR_CAPACITY for a segment with more accesses than 2^(po2 + 1).  rk_rv32mem_prep_device: rk_rv32elf_prep_device
 * with the 48-column program matrix.  rk_exec_rv32mem_shard_device: rk_exec_rv32elf_shard_device with the two tables
 * more; memop_rows / memory_rows: a power of two from what rk_exec_rv32mem_sizes gives up to 2^(po2 + 1).
 * RK_ERR_INVALID, before any launch and with nothing written, for a buffer with fewer rows than that, more than
 * 2^(po2 + 1) or not a power of two, and for an access list that is not in cycle order. */
#define RK_RV32MEM_CPU_COLS 141
#define RK_RV32MEM_PROGRAM_PREP_COLS 48
#define RK_RV32MEM_MEMOP_COLS 64
#define RK_RV32MEM_MEMORY_COLS 13
#define RK_RV32MEM_MIN_LOG_ROWS 1
int rk_exec_mem_accesses(const rk_exec* ex, uint32_t index, uint32_t* out, size_t capacity, size_t* n);
int rk_exec_rv32mem_sizes(const rk_exec* ex, uint32_t index, size_t* memop_rows, size_t* memory_rows);
int rk_rv32mem_prep_device(rk_ctx* ctx, const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs,
                           const uint32_t* words, size_t n_words, uint32_t* d_program, size_t program_rows, uint32_t* d_byte,
                           uint32_t* d_range, uint32_t* d_shift);
int rk_exec_rv32mem_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, const uint32_t* seg_vaddr,
                                 const uint32_t* seg_words, uint32_t n_segs, const uint32_t* d_image_words, uint32_t* d_cpu,
                                 uint32_t* d_program_mult, size_t program_rows, uint32_t* d_register, uint32_t* d_byte_mult,
                                 uint32_t* d_range_mult, uint32_t* d_shift_mult, uint32_t* d_muldiv, size_t muldiv_rows,
                                 uint32_t* d_memop, size_t memop_rows, uint32_t* d_memory, size_t memory_rows);
/* THE IO FORM OF RV32IM-MEM: ecalls bound to the run's input and exit code (raiko_amd/rv32io.py builds the same tables in
 * numpy, names every column and writes the AIRs).  Ten tables, rv32im-mem's nine in their order, then io; a key of its
 * own: rk_rv32io_prep_device is rk_rv32mem_prep_device with the program tuple of the word 0x00000073 reading a0 and a1
 * (RS1 = 10, RS2 = 11, WREG = 10).  DECODE OF THE ECALL WORD IS TRUSTED TO SETUP, as all decode under rv32im-elf.
 *   cpu     2^po2 x RK_RV32IO_CPU_COLS: rv32im-mem's 141 columns (N_ECW = EC_OP = 0: no send to memop; an ecall row's A and B
 *           are a0 and a1), then T0_LO / T0_HI, PT_TS, DT_LO, DT_HI, R5 = 5 IS_SYS, T0Z: an ecall row reads x5 as a fourth
 *           register access at TSA and sends (TSA, T0, A, B, RES) on bus RK_RV32IO_BUS; no row is active after a HALT row
 *   memop   an ECW row obeys SW's constraints (A its address, MI = 0, B and BB the word it leaves); its tuple comes from an
 *           io word row
 *   io      io_rows x RK_RV32IO_IO_COLS: one head row per ecall in cycle order (HALT / READ / COMMIT one-hot from T0 in
 *           {0, 1, 2}; HALT and COMMIT leave a0; READ leaves GOT = min(a1, N_INPUT - POS), proven limb by limb in RANGE16
 *           with is-zero flags), after a READ head GOT word rows -- word k sends (16, TS, A + 4 k, 0, V, 0) to memop and the
 *           stream tuple (POS_WL, POS_WH, V_LO, V_HI, 0, 0) on bus RK_RV32IO_INPUT_BUS, which no table receives -- then
 *           padding; POS runs through every row
 * The io table's RK_RV32IO_PUBLICS public values: POS_START, POS_END, N_INPUT, HALTED, EXIT_LO, EXIT_HI, then 8 words no
 * constraint reads: the digest of input[POS_START .. POS_END) as stream tuples -- rk_rv32mem_journal_root of the journal
 * (position, word, 0) at the io table's height.  The verifier recomputes it from ITS input, adds the stream tuples as
 * receive claims (rk_p3_verify_claims: this is the caller's duty stated there) and chains POS over the shards.
 * CONSTRAINED: what READ stores and where, the a0 every call leaves, the exit code.  The bytes COMMIT appends to the
 * journal are bound by the commit form (rk_exec_rv32commit_shard_device, below), not by this one.  The rk_p3_fri_*
 * statements do not cover an io proof, as for linked proofs.
 * rk_exec_ecall_args: per ecall row of segment `index` (needs record_trace) five words -- cycle, t0, a0 before the call,
 * a1, input position before it -- in cycle order; *pos_start (may be NULL): the input position at the segment's start.
 * RK_ERR_CAPACITY with *n set when more than `capacity` entries.  TraceRow.a / .b of an ecall row stay 0.
 * rk_exec_rv32io_sizes: rk_exec_rv32mem_sizes and the io table's rows, 2^max(1, ceil(log2(ecalls + words read))).
 * rk_exec_rv32io_shard_device: rk_exec_rv32mem_shard_device in io form with the tenth table; h_publics receives the io
 * table's RK_RV32IO_PUBLICS public values (Montgomery; the digest is committed under ctx's parameter set).
 * RK_ERR_INVALID / RK_ERR_CAPACITY before any launch for NULL buffers, io_rows not a power of two >= 2, below what
 * rk_exec_rv32io_sizes gives or above 2^(po2 + 1), and a side list that is not the trace's ecall rows in cycle order. */
#define RK_RV32IO_CPU_COLS 148
#define RK_RV32IO_IO_COLS 47
#define RK_RV32IO_BUS 12
#define RK_RV32IO_INPUT_BUS 13
#define RK_RV32IO_PUBLICS 14
int rk_exec_ecall_args(const rk_exec* ex, uint32_t index, uint32_t* out, size_t capacity, size_t* n, uint32_t* pos_start);
int rk_rv32io_prep_device(rk_ctx* ctx, const uint32_t* seg_vaddr, const uint32_t* seg_words, uint32_t n_segs,
                          const uint32_t* words, size_t n_words, uint32_t* d_program, size_t program_rows, uint32_t* d_byte,
                          uint32_t* d_range, uint32_t* d_shift);
int rk_exec_rv32io_sizes(const rk_exec* ex, uint32_t index, size_t* memop_rows, size_t* memory_rows, size_t* io_rows);
int rk_exec_rv32io_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, const uint32_t* seg_vaddr,
                                const uint32_t* seg_words, uint32_t n_segs, const uint32_t* d_image_words, uint32_t* d_cpu,
                                uint32_t* d_program_mult, size_t program_rows, uint32_t* d_register, uint32_t* d_byte_mult,
                                uint32_t* d_range_mult, uint32_t* d_shift_mult, uint32_t* d_muldiv, size_t muldiv_rows,
                                uint32_t* d_memop, size_t memop_rows, uint32_t* d_memory, size_t memory_rows, uint32_t* d_io,
                                size_t io_rows, uint32_t h_publics[RK_RV32IO_PUBLICS]);
/* THE COMMIT FORM OF THE IO FORM: the COMMIT journal bound (raiko_amd/rv32commit.py builds the same tables in numpy, names
 * every column and writes the AIRs).  The io form's ten tables under the io form's key (rk_rv32io_prep_device); two differ:
 *   memop   memop_rows x RK_RV32COMMIT_MEMOP_COLS: rv32im-mem's 64 columns and ECR, the selector of a tenth row kind (op
 *           RK_RV32COMMIT_ECR_CODE) that obeys LW's constraints: one row per word a COMMIT reads, in the cycle-order merge
 *           of the access list and the commit reads (a COMMIT cycle holds only reads); the memory table is built over the
 *           same merged list
 *   io      io_rows x RK_RV32COMMIT_IO_COLS: the io form's 47 columns, then CW, S, S0, S1, CNT, C0, C1, T0B, T1B, BH7, RML,
 *           RMH, RMH7, JPOS, JL, JL4, JH.  After a COMMIT head with a1 != 0 come ((a0 & 3) + a1 + 3) >> 2 commit-word rows:
 *           row k sends (17, TS, (a0 & ~3) + 4 k, 0, 0, V) to memop -- V is memory's word -- and (JL, JH, V_LO, V_HI, S,
 *           CNT) on bus RK_RV32COMMIT_BUS, which no table receives: bytes S .. S + CNT - 1 of V go to the journal at byte
 *           offset JPOS = JL + 2^14 JH.  S is a0 & 3 on a call's first row and 0 later, S + CNT = 4 on every row but the
 *           call's last, and REM counts a1 down by CNT to 0.  JPOS runs through every row
 * The io table's RK_RV32COMMIT_PUBLICS public values: the io form's 14, JPOS_START, JPOS_END, then 8 words no constraint
 * reads: the digest of the shard's commit log -- rk_rv32mem_journal_root of the journal (jpos, word, S | CNT << 16) at the
 * io table's height.  The verifier is HANDED the log (as the link's verifier is handed the memory journal), checks its
 * shape, recomputes the digest, adds the log's tuples as receive claims (rk_p3_verify_claims) and cuts the journal's bytes
 * out of it; it chains JPOS over the shards.  The log shows the bytes of a COMMIT's first and last word that the call
 * does not select.  CONSTRAINED: every byte of the journal.  The rk_p3_fri_* statements do not cover a commit proof.
 * rk_exec_commit_reads: per word an ecall COMMIT of segment `index` reads (needs record_trace) three words -- cycle, word
 * address, word -- in cycle order and per call in ascending address order from a0 & ~3; *jpos_start (may be NULL): the
 * journal's length at the segment's start.  RK_ERR_CAPACITY with *n set when more than `capacity` entries.
 * rk_exec_mem_accesses holds none of these: it returns what it returned before.
 * rk_exec_rv32commit_sizes: rk_exec_rv32io_sizes over the merged list and with the commit-word rows counted.
 * rk_exec_rv32commit_shard_device: rk_exec_rv32io_shard_device in commit form; d_log (io_rows x 3 words) receives the
 * commit log, canonical, *n_log its rows.  Refusals before any launch as rk_exec_rv32io_shard_device's, the rule "no more
 * accesses than twice the cpu table's rows" over the merged list, and RK_ERR_INVALID for commit reads that are not the
 * words of the trace's COMMITs in cycle order or a COMMIT of 2^25 bytes and more. */
#define RK_RV32COMMIT_MEMOP_COLS 65
#define RK_RV32COMMIT_IO_COLS 64
#define RK_RV32COMMIT_BUS 14
#define RK_RV32COMMIT_ECR_CODE 17
#define RK_RV32COMMIT_PUBLICS 24
int rk_exec_commit_reads(const rk_exec* ex, uint32_t index, uint32_t* out, size_t capacity, size_t* n, uint32_t* jpos_start);
int rk_exec_rv32commit_sizes(const rk_exec* ex, uint32_t index, size_t* memop_rows, size_t* memory_rows, size_t* io_rows);
int rk_exec_rv32commit_shard_device(rk_ctx* ctx, const rk_exec* ex, uint32_t index, const uint32_t* seg_vaddr,
                                    const uint32_t* seg_words, uint32_t n_segs, const uint32_t* d_image_words, uint32_t* d_cpu,
                                    uint32_t* d_program_mult, size_t program_rows, uint32_t* d_register, uint32_t* d_byte_mult,
                                    uint32_t* d_range_mult, uint32_t* d_shift_mult, uint32_t* d_muldiv, size_t muldiv_rows,
                                    uint32_t* d_memop, size_t memop_rows, uint32_t* d_memory, size_t memory_rows, uint32_t* d_io,
                                    size_t io_rows, uint32_t h_publics[RK_RV32COMMIT_PUBLICS], uint32_t* d_log, size_t* n_log);
/* THE LINK BETWEEN SHARD MEMORIES (raiko_amd/rv32link.py; the first of the designs a boundary table admits: a digest).
 * With the link on, a real row of the memory table also SENDS (WL, WH, I_LO, I_HI, F_LO, F_HI) on bus RK_RV32LINK_BUS,
 * which no table receives, and the table carries 8 public values no constraint reads: the digest of the shard's JOURNAL,
 * one (word address, INIT, FINAL) per touched word, ascending.  The verifier is handed the journal, recomputes the digest
 * (rk_rv32mem_journal_root) against the public values, adds the receiving side itself (rk_p3_verify_claims with the
 * journal's limb tuples as receive claims) and replays the journals shard after shard from the ELF's memory image
 * (rk_exec_memory_image): INIT of a word must be what the image holds, then the image's word becomes FINAL.  Public values
 * are observed before the permutation challenges are sampled, so the journal is fixed (up to a collision of the digest)
 * before the challenges exist, and the LogUp identity makes the multiset of real boundary rows the journal.  STILL FREE:
 * what an ecall writes and the a0 it leaves (bound by the io form above; then the COMMIT journal remains).  The verifier's work is linear in the touched words.  The rk_p3_fri_*
 * captures of a linked proof replay rk_p3_verify_key and stop at reason 8: the FRI statements do not cover it.
 * The digest: the rk_mmcs_commit root of the memory_rows x RK_RV32LINK_TUPLE row-major Montgomery matrix of the limb
 * tuples, rows of zeros past the real ones.
 * rk_exec_memory_image: every PT_LOAD segment's file bytes, as the executor's loader stores them, merged into (word
 * address, word) pairs in ascending address order: a later segment overwrites an earlier one byte by byte, bytes of a
 * word outside every segment's file bytes are 0.  RK_ERR_CAPACITY with *n set when more than `capacity` words.  Host only.
 * rk_rv32mem_journal_device: from a finished device memory table (memory_rows x RK_RV32MEM_MEMORY_COLS, Montgomery) the
 * journal (canonical, 3 words per real row, in row order; capacity memory_rows rows), the link matrix (memory_rows x
 * RK_RV32LINK_TUPLE, Montgomery), the tree over it (d_nodes: 2 * memory_rows * 8 words, as rk_mmcs_commit) with its root
 * in h_root, and the count of real rows in *n_real.  RK_ERR_INVALID before any launch for NULL buffers or memory_rows
 * not a power of two >= 2; RK_ERR_INVALID after the run for a table whose real rows are not a prefix or which holds a
 * limb that is no 16-bit value (a 14-bit WL).
 * rk_rv32mem_journal_root: the same digest on the host from a journal of n rows (canonical) at table height
 * 2^log_rows.  RK_ERR_INVALID for n > 2^log_rows, an address >= 2^30 or addresses that do not strictly ascend. */
#define RK_RV32LINK_BUS 11
#define RK_RV32LINK_TUPLE 6
int rk_exec_memory_image(const uint8_t* elf, size_t elf_bytes, uint32_t* out_addr, uint32_t* out_words, size_t capacity, size_t* n);
int rk_rv32mem_journal_device(rk_ctx* ctx, const uint32_t* d_memory, size_t memory_rows, uint32_t* d_journal, uint32_t* d_link,
                              uint32_t* d_nodes, size_t* n_real, uint32_t h_root[8]);
int rk_rv32mem_journal_root(const rk_params* params, const uint32_t* journal, size_t n, uint32_t log_rows, uint32_t root[8]);
const char* rk_exec_error(const rk_exec* ex);
int rk_exec_free(rk_exec* ex);

/* ---- Plonky3-style STARK for AIRs handed over as data: the proof system behind SP1's `client.setup(ELF)` /
 * `client.prove(&pk, stdin)` (provers/sp1/driver/src/lib.rs:44-57; shard knobs docs/README_Sp1.md:19-32) as far as it
 * exists without SP1's chips -- p3-uni-stark prove / verify over p3-fri's TwoAdicFriPcs with a DuplexChallenger
 * (Plonky3@88ea2b8, Cargo.lock:4889-5127; RECALLED, the crates are outside the reference tree), for one or several
 * tables under shared challenges, the way sp1-core proves the chips of a shard, including the permutation (LogUp)
 * argument that ties the tables together (rk_air_create_lookup below).  NOT here: SP1's chips, its recursion / compress VM.
 *
 * An AIR is a step list, the shape `Air::eval` leaves in a symbolic builder: every step except ASSERT_ZERO pushes one
 * value; a, b name earlier values by their position in that list.
 *   CONST a              the canonical integer a
 *   LOCAL a / NEXT a     column a of the current / the next row (cyclic)
 *   PUBLIC a             public value a
 *   IS_FIRST_ROW, IS_LAST_ROW, IS_TRANSITION     the Lagrange selectors (unnormalised, as p3-commit domain.rs has them)
 *   ADD | SUB | MUL a b, NEG a
 *   ASSERT_ZERO a        ConstraintFolder::assert_zero: accumulator = accumulator * alpha + a
 *   PERM_LOCAL a / PERM_NEXT a   base column a of the table's permutation trace (rk_air_create_lookup), current / next row
 *   CHALLENGE a          base component a of the permutation challenges [alpha | beta^0 | beta^1 | ...] (4 words each)
 *   CUMSUM a             base component a of the table's cumulative sum
 *   PREP_LOCAL a / PREP_NEXT a   preprocessed column a (rk_air_create_prep), current / next row; symbolic degree 1
 * rk_air_create validates, derives the quotient degree from the symbolic degrees (get_log_quotient_degree: a cell and
 * is_first_row / is_last_row count 1, is_transition and constants 0) and translates the list into an rk_program whose
 * taps are the columns of the LDE, so the quotient is evaluated by the same GPU evaluator as risc0's eval_check;
 * rk_air_compile builds the straight-line kernel with hiprtc (optional, about 3x the interpreter). */
typedef enum {
    RK_AIR_CONST = 0, RK_AIR_LOCAL = 1, RK_AIR_NEXT = 2, RK_AIR_PUBLIC = 3, RK_AIR_IS_FIRST_ROW = 4, RK_AIR_IS_LAST_ROW = 5,
    RK_AIR_IS_TRANSITION = 6, RK_AIR_ADD = 7, RK_AIR_SUB = 8, RK_AIR_MUL = 9, RK_AIR_NEG = 10, RK_AIR_ASSERT_ZERO = 11,
    RK_AIR_PERM_LOCAL = 12, RK_AIR_PERM_NEXT = 13, RK_AIR_CHALLENGE = 14, RK_AIR_CUMSUM = 15,
    RK_AIR_PREP_LOCAL = 16, RK_AIR_PREP_NEXT = 17
} rk_air_op;
typedef struct { uint32_t op, a, b; } rk_air_step;
typedef struct rk_air rk_air;
typedef struct {
    uint64_t n_steps;              /* as given */
    uint64_t n_ops;                /* arithmetic steps a point of the quotient domain costs */
    uint32_t n_constraints;
    uint32_t max_degree;           /* symbolic degree of the highest constraint */
    uint32_t log_quotient_degree;  /* log2_ceil(max(max_degree, 2) - 1): the quotient has 2^this chunks */
    uint32_t n_fp_slots;           /* live intermediate values (rk_program_info) */
} rk_air_info;
int rk_air_create(const rk_air_step* steps, size_t n_steps, uint32_t width, uint32_t n_public, rk_air** out);
/* An AIR whose table takes part in lookups, in the shape sp1-core gives them (stark/permutation.rs, lookup/interaction.rs,
 * air/builder.rs send / receive; sp1-core is pulled by the reference's Cargo.lock, RECALLED): interaction i says "every
 * row sends (kind 0) or receives (kind 1) the tuple (bus, local[value_cols]...) `mult` times", mult a main-trace column
 * or -- mult_is_const -- a canonical constant.  Flat form: per interaction the words kind, bus, mult_is_const, mult,
 * n_values followed by its n_values column numbers (n_words in all); at most 64 values per tuple and 120 distinct
 * columns over all interactions of a table.
 * The prover (rk_p3_prove) then, after the main traces are committed, draws two extension challenges alpha, beta,
 * fills the table's permutation trace on the GPU -- one extension column per batch of two interactions holding
 * sum +-mult / (alpha + beta^0 bus + sum_j beta^(j+1) value_j), and a last column with the running sum of the row totals
 * (4 base columns each: 4 * (ceil(n / 2) + 1) in all) --, commits those traces as a second batch and observes root and
 * cumulative sums before the constraint challenge; the verifier also checks that the cumulative sums of all tables add
 * up to zero (reason 8): every tuple sent is received as often.  The constraints tying the permutation trace to the
 * main trace are AIR steps over PERM_LOCAL / PERM_NEXT / CHALLENGE / CUMSUM -- sp1-core's eval_permutation_constraints,
 * every extension identity as four base asserts: per batch entry * prod rlc_i = sum_i +-mult_i * prod_(j != i) rlc_j,
 * phi[0] = sum entries[0], phi' = phi + sum entries' on transitions, phi[last] = cumulative sum.  ext_w != 0: `steps`
 * holds the table's own constraints only (what a chip's Air::eval emits) and the library appends those steps for the
 * extension x^4 - ext_w (the canonical W of the parameter set the proofs will be made under: 11 for SP1's); ext_w = 0:
 * `steps` already contains them (raiko_amd/p3.py AirBuilder can write them itself).  rk_air_get_steps reads the full
 * list back.  A proof without any interaction keeps the bytes it had before this entry point existed. */
int rk_air_create_lookup(const rk_air_step* steps, size_t n_steps, uint32_t width, uint32_t n_public,
                         const uint32_t* interaction_words, uint32_t n_interactions, size_t n_words, uint32_t ext_w, rk_air** out);
/* An AIR over `width` trace columns and `prep_width` PREPROCESSED columns: columns fixed before any witness exists (a
 * range table's values, a program's instructions), committed once by rk_p3_setup and read by the steps through
 * PREP_LOCAL / PREP_NEXT a, a < prep_width.  Interactions as in rk_air_create_lookup (n_interactions = 0: none), over the
 * union of both: a column number c >= width in the flat words -- a value or a `mult` that is a column -- means
 * preprocessed column c - width; the limits (64 values per tuple, 120 distinct columns per table) count the union, and
 * the appended permutation constraints read such a column through PREP_LOCAL.  rk_air_create and rk_air_create_lookup
 * are this call with prep_width = 0, where PREP_* steps are refused.  Tables of such an AIR are proven with
 * rk_p3_prove_key and checked with rk_p3_verify_key only (see there). */
int rk_air_create_prep(const rk_air_step* steps, size_t n_steps, uint32_t width, uint32_t prep_width, uint32_t n_public,
                       const uint32_t* interaction_words, uint32_t n_interactions, size_t n_words, uint32_t ext_w, rk_air** out);
/* the AIR's preprocessed columns (0: none, or air NULL) */
uint32_t rk_air_prep_width(const rk_air* air);
/* the AIR's complete step list (with the appended lookup constraints); RK_ERR_CAPACITY with *n_steps set when it does not fit */
int rk_air_get_steps(const rk_air* air, rk_air_step* out, size_t capacity, size_t* n_steps);
int rk_air_destroy(rk_air* air);
int rk_air_get_info(const rk_air* air, rk_air_info* out);
int rk_air_compile(rk_air* air, rk_ctx* ctx);
/* The Poseidon2 chip: a table whose every row is one permutation of the parameter set's instance (width 16 or 24, either
 * 4x4 block) with the intermediate values a degree-3 AIR needs in columns -- the shape of sp1-recursion-core's Poseidon2
 * wide chip (RECALLED; outside the reference tree), the table a recursion / compress layer spends most of its rows on:
 * every Merkle path step and sponge block of a proof it verifies is one lookup (bus: in[0..W), out[0..8)) into it.
 * Columns: in W | external rounds 0..3: cube W, state after the round W | internal rounds: cube of cell 0 (R_P), cell 0
 * entering rounds 1.. (R_P - 1) | state after the internal rounds W | external rounds 4..7 | multiplicity; x^7 = cube *
 * cube * x, so every constraint has degree 3 (two quotient chunks).  314 columns for width 16, 474 for width 24.
 * rk_p2_chip_air: the AIR (step list written by the library, one receive interaction on `bus` with the multiplicity
 * column); rk_p2_chip_trace: the rows on the GPU under the context's parameter set, one lane per permutation -- d_inputs
 * n x W row-major Montgomery words, d_mult n multiplicities or NULL for ones, d_trace n x rk_p2_chip_width row-major:
 * ready to be an on_device rk_p3_table.  params NULL = the SP1 preset. */
uint32_t rk_p2_chip_width(const rk_params* params);
int rk_p2_chip_air(const rk_params* params, uint32_t bus, rk_air** out);
/* rk_p2_chip_air_ex: the same step list and width with the receive (in[0..W), out[0..n_out)), n_out 8 or 16: with 16 the
 * chip hands out the whole state after the permutation, what a sponge over more than one block carries from one
 * permutation to the next.  rk_p2_chip_air is n_out = 8; rk_p2_chip_trace writes the rows of either. */
int rk_p2_chip_air_ex(const rk_params* params, uint32_t bus, uint32_t n_out, rk_air** out);
int rk_p2_chip_trace(rk_ctx* ctx, const uint32_t* d_inputs, const uint32_t* d_mult, size_t n, uint32_t* d_trace);
/* The Keccak-f[1600] chip: the permutation behind Keccak-256 as a table, the first precompile-shaped chip -- the shape
 * of p3-keccak-air (pulled by the reference's Cargo.lock, the crate outside the reference tree: RECALLED, parity unpinned;
 * without its preimage / export columns, and the columns below are this project's).
 * One row per round, 25 rows per permutation: rows 0..23 are the 24 rounds, row 24 is an OUTPUT ROW -- a round with round
 * constant 0 whose results nobody reads; it exists so that the permutation's output stands in the same columns A its
 * input stood in, which keeps the interactions within the 120 distinct columns a table's interactions may read (input
 * plus output are 200 limbs).  Lane (x, y) has index x + 5 y; a lane is four 16-bit limbs, little endian, or 64 bits.
 * Columns (2537): STEP[25] one-hot round flags | A[25][4] the state entering the row, limbs | C[5][64] column parities,
 * bits | C'[5][64] = C[x] ^ C[x-1] ^ rol(C[x+1], 1), bits | A'[25][64] the state after theta, bits | A''[25][4] the state
 * after rho, pi, chi, limbs | the 64 bits of A''[0][0] | A'''[0][0] lane (0, 0) after iota, 4 limbs | ID | M | M_IN | M_OUT.
 * Constraints (degree <= 3, two quotient chunks): the flags are one-hot, STEP[0] on the first row, STEP[i] goes on to the
 * next row's STEP[i + 1 mod 25]; C, A' and the bits of A''[0][0] are boolean; C' is that xor; every limb of A is
 * recomposed from A' ^ C ^ C'; sum_y A'[y][x][z] - C'[x][z] is 0, 2 or 4; every limb of A'' is recomposed from
 * b ^ (~b1 & b2) over the rho / pi-permuted bits of A'; A'''[0][0] = A''[0][0] ^ rc with rc_z = sum_r STEP[r] RC[r]_z
 * (0 on row 24); unless STEP[24], the next row's A is this row's result (A'''[0][0], A'' elsewhere) and its ID and M are
 * this row's; M_IN = M STEP[0], M_OUT = M STEP[24].
 * Interactions: four receives.  bus, bus + 1: (ID, limbs 0..49 of A), (ID, limbs 50..99 of A) M_IN times -- the input;
 * bus + 2, bus + 3: the same columns M_OUT times -- the output (limb index = 4 (x + 5 y) + limb; 51 values per tuple, 103
 * distinct columns).  M is one column under all four and constant over a permutation's rows, so a permutation that
 * answers one of a sender's four tuples must have all four of its own matched; ID ties the halves and the two ends.  A
 * permutation cut off by the table's end must have M = 0 -- otherwise its input is received and its output never, and
 * the cumulative sums do not cancel (the verifier's reason 8); no constraint is needed for that.
 * rk_keccak_chip_air: the AIR (step list written by the library; params gives the extension's W, NULL = the SP1
 * preset; the buses bus .. bus + 3 must be canonical).  rk_keccak_chip_trace: the rows on the GPU, one wavefront per
 * permutation -- d_states n x 25 lanes (lane x + 5 y), d_ids / d_mult n Montgomery words each or NULL for 0 .. n - 1 /
 * ones, rows a power of two >= max(2, 25 n) and <= 2^24 (permutation slots past n, the cut-off last one included, are
 * the zero state with M = ID = 0), d_trace rows x rk_keccak_chip_width row-major Montgomery words, ready to be an
 * on_device rk_p3_table; d_out NULL or n x 25 lanes: the permutations' outputs.  RK_ERR_INVALID before any launch for a
 * NULL ctx / d_states / d_trace, n = 0, or rows that are no power of two, below 25 n or above 2^24.
 * Out of scope here: the chip as an ecall of the executor through the memory argument.  The sponge table over it
 * follows. */
uint32_t rk_keccak_chip_width(void);
int rk_keccak_chip_air(const rk_params* params, uint32_t bus, rk_air** out);
int rk_keccak_chip_trace(rk_ctx* ctx, const uint64_t* d_states, const uint32_t* d_ids, const uint32_t* d_mult, size_t n, size_t rows,
                         uint32_t* d_trace, uint64_t* d_out);
/* THE KECCAK-256 SPONGE TABLE over the chip: "the Keccak-256 of these blocks is this digest".  Rate 136 bytes = 17 lanes
 * = 68 limbs; the table absorbs WHOLE blocks: padding (0x01 .. 0x80) lies with whoever sends them -- the verifier for
 * public messages, later an ecall table --, the AIR has no padding constraints.  Three rows per block (a group), in this
 * order: the X row (V[0..67] = the block's limbs, V[68..99] = 0), the I row (V = the state entering the permutation =
 * PREV xor the block) and the O row (V = the permutation's output).  Everything the table sends stands in the one block
 * V of 100 limb columns on different rows, so its seven interactions read 108 distinct columns.  Columns
 * (rk_keccak_sponge_width = 2458; kc::KeccakSpongeLayout, raiko_amd/csrc/keccak_sponge.hpp): V[100] | PREV[100] (the state
 * before this block: 0 on a message's first, else the preceding O row's V; the same on a group's rows) | MB[17][64] the
 * bits of V's rate lanes | PB[17][64] those of PREV's | XR[68] = sum_k 2^k (mb + pb - 2 mb pb) | MSG BLK NBLK PID | KX KI KO
 * REAL | FIRST LAST | S_IN S_OUT S_MSG S_DIG.  MB, PB and XR are constrained on every row alike (an all-zero row satisfies
 * them); the X row's XR is what the I row's rate part must equal, its capacity part is PREV's -- both linear under IS_TRANSITION KX,
 * which keeps the degree at 3.
 * Constraints: the kinds are boolean, REAL their sum, X -> I -> O, an X row only after an O row (REAL falls once: real
 * groups, then padding, and a padding row is zero); the first row is an X row with FIRST and PID 0, or padding; the last
 * row is an O row or padding (a group the table's end cuts is not real); S_MSG = REAL KX, S_IN = REAL KI, S_OUT = REAL KO,
 * S_DIG = KO LAST (a real row cannot withhold a send); NBLK = BLK + REAL; FIRST => BLK = 0 and PREV = 0; within a group
 * PREV, MSG, BLK, PID, FIRST, LAST go on; PID rises by 1 a group; after an O row without LAST comes an X row of the same
 * MSG with BLK + 1, FIRST = 0 and PREV = this V, and such a row is not the table's last; after a LAST O row a real row
 * has FIRST.
 * Interactions, seven sends: (PID, V[0..49]) on bus and (PID, V[50..99]) on bus + 1 S_IN times, the same on bus + 2, bus + 3
 * S_OUT times -- the chip's four receives --; (MSG, BLK, V[0..33]) on bus + 4 and (MSG, BLK, V[34..67]) on bus + 5 S_MSG
 * times; (MSG, NBLK, V[0..15]) on bus + 6 S_DIG times: the digest and the message's block count.  No table receives
 * the last three: the verifier does, with claims (rk_p3_verify_claims) it binds itself.
 * rk_keccak_sponge_air: params NULL = the SP1 preset; bus .. bus + 6 must be canonical.  rk_keccak_sponge_trace: two
 * launches on the context's stream.  keccak_sponge_chain_kernel, one wavefront per message with lane i < 25 holding lane i
 * of the state, writes per block the permutation's input to d_states (n_blocks x 25 lanes: exactly rk_keccak_chip_trace's
 * d_states) and its output to d_outs, and four lanes per message to d_digests (n_msgs x 4); keccak_sponge_rows_kernel,
 * one wavefront per block, then writes d_trace (rows x rk_keccak_sponge_width Montgomery words; block slots past
 * n_blocks, the cut-off last one included, are zero rows).  d_blocks n_blocks x 17 lanes; d_first n_msgs + 1 words: the
 * first block of each message, then n_blocks -- it must start at 0, rise strictly and end in n_blocks: anything else is
 * THE CALLER'S ERROR and not detected (no access leaves the buffers, the rows are then not a valid witness); d_msg_ids
 * NULL for 0 .. n_msgs - 1, else n_msgs Montgomery words.  RK_ERR_INVALID before any launch for a NULL ctx or buffer
 * (d_msg_ids excepted), n_msgs = 0, n_blocks = 0, n_msgs > n_blocks, or rows that are no power of two, below
 * rk_keccak_sponge_rows_per_block x n_blocks or above 2^24.
 * Out of scope: the executor's ecall, SHA-3 padding and other rates, a digest binding of the claims in place of init_words. */
uint32_t rk_keccak_sponge_width(void);
uint32_t rk_keccak_sponge_rows_per_block(void);
int rk_keccak_sponge_air(const rk_params* params, uint32_t bus, rk_air** out);
int rk_keccak_sponge_trace(rk_ctx* ctx, const uint64_t* d_blocks, const uint32_t* d_first, const uint32_t* d_msg_ids, size_t n_msgs,
                           size_t n_blocks, size_t rows, uint32_t* d_trace, uint64_t* d_states, uint64_t* d_outs, uint64_t* d_digests);
/* THE KECCAK-256 PADDING TABLE under the sponge: "these 32-bit words, cut at this byte length and padded, are those
 * blocks".  It RECEIVES the sponge's three sends on bus + 4 .. bus + 6 and sends what a memory-argument table can answer:
 * one tuple a word and one a message.  The statement of [pad, sponge, chip]: for every message the sender supplies its
 * little-endian words w_0 .. w_(NW-1), NW = ceil(len / 4) (the bytes of the last word past len are arbitrary and do not
 * matter), len and a digest; the proof is accepted exactly when digest = Keccak-256(the first len bytes of the words).
 * One row per word slot, 34 rows a block (rk_keccak_pad_rows_per_block).  Columns (rk_keccak_pad_width = 167;
 * kc::KeccakPadLayout, raiko_amd/csrc/keccak_pad.hpp): B[68], a shift register of limbs -- B[66], B[67] the word PLACED on
 * this row, next.B[j] = B[j + 2] within a block, so the block's 34th row holds the whole block -- | STEP[34] one-hot word
 * position | W_LO W_HI the sender's word | WB[32] its bits | E[4] one-hot of len mod 4 on the END row | D[16] the digest's
 * limbs on a message's last row | MSG BLK NBLK IDX LEN | DATA END AFTER REAL | R S_END.  A row is DATA (a word before the
 * one that holds byte position len), END (that word) or AFTER; a padding row is zero.
 * Constraints: the phases are boolean, REAL their sum and boolean, REAL falls once; STEP is one-hot on real rows, STEP[0]
 * on the first row, cyclic; S_END = STEP[33] (END + AFTER) marks a message's last row, R = DATA + END - E[0] the rows that
 * carry a word, NBLK = BLK + REAL (a real row cannot withhold a tuple); sum E = END and END (LEN - 4 IDX) = E[1] + 2 E[2] +
 * 3 E[3]; WB boolean and recomposing W on every row, W = 0 where R = 0; the placed word B[66], B[67] = W on DATA, W's bytes
 * below e and 0x01 above them on END, 0 on AFTER, + 0x8000 in the high limb on a message's last row (0x01 + 0x80 = 0x81:
 * nothing carries); B[0..65] = 0 on STEP[0] and on padding rows and shifts after a real row without STEP[33]; D = 0 off a
 * message's last row; IDX = BLK = AFTER = 0 on the first row and after a message's last; a real row that is not its
 * message's last is followed by a real row with MSG and LEN unchanged, IDX + 1, BLK + STEP[33] and AFTER = END + AFTER (so
 * DATA* END AFTER*: one END a message, and LEN = 4 IDX + e places it), and is not the table's last row.  Degree 3.
 * Interactions (94 distinct columns): receives (MSG, BLK, B[0..33]) on bus + 4 and (MSG, BLK, B[34..67]) on bus + 5
 * STEP[33] times, (MSG, NBLK, D) on bus + 6 S_END times; sends (MSG, IDX, W_LO, W_HI) on bus + 7 R times and (MSG, LEN, D)
 * on bus + 8 S_END times.  No table receives the two sends: the verifier does, with claims (rk_p3_verify_claims).
 * rk_keccak_pad_air: params NULL = the SP1 preset; bus .. bus + 8 must be canonical.  rk_keccak_pad_trace: two launches on
 * the context's stream.  keccak_pad_blocks_kernel, one thread per word slot, writes d_blocks (n_blocks x 17 lanes: exactly
 * rk_keccak_sponge_trace's d_blocks -- the padded message is never formed on the host); keccak_pad_rows_kernel, one
 * wavefront per block slot of 34 rows, then writes d_trace (rows x rk_keccak_pad_width Montgomery words, D = 0; rows past 34 n_blocks are
 * zero).  d_words n_words words: the messages' words back to back, each message from a word boundary; d_word_first
 * n_msgs + 1: the first word of each message, then n_words; d_lens n_msgs byte lengths; d_first n_msgs + 1: the first block
 * of each message, then n_blocks, where message m has len / 136 + 1 blocks.  Tables that do not agree with each other are
 * THE CALLER'S ERROR and not detected: no access leaves the buffers (a word index is held below n_words, a block index
 * below n_blocks), the rows are then not a valid witness.  d_msg_ids NULL for 0 .. n_msgs - 1, else n_msgs Montgomery words.
 * rk_keccak_pad_digests: one launch that writes D from rk_keccak_sponge_trace's d_digests (n_msgs x 4 lanes), which exist
 * only after the sponge has run over d_blocks.  Both return RK_ERR_INVALID before any launch for a NULL ctx or buffer
 * (d_msg_ids excepted), n_msgs = 0, n_msgs > n_blocks, or rows that are no power of two, below 34 n_blocks or above 2^24.
 * Out of scope: RK_ECALL_KECCAK itself (the executor's ecall, io-table rows that send the words, the digest's write-back,
 * key and shard pool), sources that are not word-aligned, SHA-3's 0x06. */
uint32_t rk_keccak_pad_width(void);
uint32_t rk_keccak_pad_rows_per_block(void);
int rk_keccak_pad_air(const rk_params* params, uint32_t bus, rk_air** out);
int rk_keccak_pad_trace(rk_ctx* ctx, const uint32_t* d_words, size_t n_words, const uint32_t* d_word_first, const uint32_t* d_lens,
                        const uint32_t* d_first, const uint32_t* d_msg_ids, size_t n_msgs, size_t n_blocks, size_t rows, uint32_t* d_trace,
                        uint64_t* d_blocks);
int rk_keccak_pad_digests(rk_ctx* ctx, const uint64_t* d_digests, const uint32_t* d_first, size_t n_msgs, size_t n_blocks, size_t rows,
                          uint32_t* d_trace);
/* One table of a proof.  trace: row-major 2^log_height x width Montgomery words (Plonky3's RowMajorMatrix), in host
 * memory or -- on_device = 1 -- in the memory of the context's GPU (left untouched). */
typedef struct {
    const uint32_t* trace;
    uint32_t log_height;           /* 1 .. 24 - blowup_log2; verifier: 0 = read it from the proof, else the height required */
    uint32_t width;                /* = the AIR's */
    const rk_air* air;
    const uint32_t* public_values; /* host, Montgomery words */
    uint32_t n_public;             /* = the AIR's */
    uint32_t on_device;
} rk_p3_table;
/* p3-uni-stark `prove` under the context's parameter set (rk_set_params: field, coset shift = Val::generator(), Poseidon2
 * instance, blowup_log2 = FriConfig::log_blowup, queries, pow_bits; fri_fold_log2 / fri_min_degree are not used -- the
 * PCS folds by two down to a constant).  Every table's quotient degree must fit the blow-up.  Transcript:
 * observe(init_words) -- whatever binds the statement: SP1 observes the verifying key and pc_start there --,
 * observe(trace root), observe(public values of every table), [lookups: permutation alpha, beta, observe(permutation
 * root), observe(cumulative sums)], alpha, observe(quotient root), zeta, then the PCS's own challenges.
 * Proof = u32 words (field elements as Montgomery words):
 *   n_tables | log_height per table | trace root 8 | [permutation root 8 | cumulative sum 4 per table with lookups] |
 *   quotient root 8 |
 *   per table: opened trace row at zeta (4 words per column), at zeta * g, [the permutation trace's, likewise],
 *   2^log_quotient_degree chunks x 4 x 4 |
 *   n_rounds | n_rounds x 8 commit-phase roots | final polynomial 4 | proof-of-work witness (canonical integer) |
 *   per query: the trace batch (every table's LDE row, then the Merkle path), [the permutation batch], the quotient
 *   batch (every chunk's row, then the path), then per FRI round the sibling value (4) and its path.
 * RK_ERR_CAPACITY with *proof_words = the exact size when the buffer is too small.  A trace that breaks its AIR still
 * yields a proof (as in Plonky3's release builds); rk_p3_verify rejects it with reason 3. */
int rk_p3_prove(rk_ctx* ctx, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init_words, size_t n_init,
                uint32_t* h_proof, size_t capacity_words, size_t* proof_words);
/* PREPROCESSED COLUMNS: setup once, prove with a key -- the shape of SP1's `client.setup(ELF)` -> `prove(&pk, ..)` ->
 * `verify(.., &vk)` (provers/sp1/driver/src/lib.rs:44-57,116-120).  A fourth committed batch beside trace, permutation
 * and quotient: the preprocessed matrices of the tables whose AIR has prep_width > 0, committed ONCE, their root part of
 * the statement (the verifying key = that root plus the heights of those tables), opened at zeta and zeta * g like the
 * main trace and readable by the AIR and the interactions.  The protocol, as prover, verifier and the tests' reference
 * state it (this project's choice, modelled on sp1-core's machine, RECALLED; the pinned Plonky3 revision has no
 * preprocessed trace in uni-stark, so there is no upstream parity to pin):
 *   transcript   observe(init_words), observe(preprocessed root) IF the key has one, then the trace root and everything
 *                after it as in rk_p3_prove
 *   proof words  header, trace root, permutation part, quotient root unchanged -- the preprocessed root is NOT in the
 *                proof, the verifier's caller supplies it; per table the opened values are
 *                  local 4w | next 4w | [prep local 4c | prep next 4c] | [perm local | perm next] | chunks
 *                per query: the trace batch, [the preprocessed batch: every preprocessed table's LDE row in table order,
 *                then the Merkle path of its own tree, whose height is that of its tallest member], [the permutation
 *                batch], the quotient batch, the FRI rounds
 *   order of the opened matrices (batches hashed, powers of the PCS's alpha in the reduced openings): trace,
 *                preprocessed, permutation, quotient
 * A proof of tables without any preprocessed column keeps every byte rk_p3_prove gives it.
 *
 * rk_p3_setup: prep_traces[t] = the row-major 2^log_height x prep_width Montgomery matrix of table t (host memory, or
 * device memory where tables[t].on_device), NULL where the table's AIR has prep_width = 0; of `tables` the air,
 * log_height and on_device are read.  The key holds in the memory of the context's GPU (its own allocations, alive until
 * rk_p3_key_destroy, usable by any context of that GPU under the same parameter set): the column LDE of every
 * preprocessed matrix (2^(log_height + blowup_log2) x prep_width words), the tree over them (one rk_mmcs_commit in table
 * order), the root, the row-major matrix itself for the tables whose interactions read a preprocessed column, and every
 * table's (prep_width, log_height): a table with preprocessed columns has its height fixed by the key.  A key over
 * tables without any preprocessed column is legal and has no root (rk_p3_key_root: RK_ERR_INVALID). */
typedef struct rk_p3_key rk_p3_key;
int rk_p3_setup(rk_ctx* ctx, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* const* prep_traces, rk_p3_key** key);
int rk_p3_key_root(const rk_p3_key* key, uint32_t out[8]);
size_t rk_p3_key_bytes(const rk_p3_key* key);   /* device memory the key holds */
int rk_p3_key_destroy(rk_p3_key* key);
/* rk_p3_prove with a key (NULL: none -- rk_p3_prove is exactly that, and refuses AIRs with prep_width > 0).  The key must
 * come from a context of the same GPU under the same parameter set and from tables of the same count, prep_width and --
 * where prep_width > 0 -- log_height: anything else is RK_ERR_INVALID before a kernel is launched.  The quotient reads
 * the key's LDE in place (a fourth column group of the evaluator), the permutation trace its rows, the queries its tree:
 * nothing of the preprocessed data is copied or recomputed per proof. */
int rk_p3_prove_key(rk_ctx* ctx, const rk_p3_key* key, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init_words, size_t n_init,
                    uint32_t* h_proof, size_t capacity_words, size_t* proof_words);
/* exact proof size of rk_p3_prove_key for the tables' shapes; = rk_p3_proof_bound_words without preprocessed columns */
size_t rk_p3_proof_bound_words_key(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables);
/* rk_p3_verify against a verifying key: prep_root = the 8 words of rk_p3_key_root, NULL when no table has preprocessed
 * columns (then this is rk_p3_verify); every table with prep_width > 0 must come with its pinned log_height != 0.  A root
 * without such a table, such a table without a root or without its height: RK_ERR_INVALID.  A proof carrying another
 * height: reason 2; a preprocessed opening that does not lead to the caller's root: reason 5.
 * rk_p3_verify, rk_p3_verify_hashes, the four rk_p3_fri_* captures, rk_p3_prove and rk_p3_prove_shards refuse tables with
 * prep_width > 0 with RK_ERR_INVALID: they have no root to check the fourth batch against.  Keyed proofs go to the _key
 * twins instead: rk_p3_prove_key, rk_p3_verify_key, rk_p3_verify_hashes_key and the four rk_p3_fri_*_key captures below,
 * whose formats carry the preprocessed batch and which the rk_fri_* tables are written from in the same way. */
int rk_p3_verify_key(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* prep_root,
                     const uint32_t* init_words, size_t n_init, const uint32_t* proof, size_t proof_words);
/* p3-uni-stark `verify` on the host (no GPU): params NULL = the SP1 preset; trace / on_device of the tables are ignored;
 * log_height = 0 takes the table's height from the proof, any other value PINS it (the proof must carry that height: what
 * a statement with a fixed-size table -- all 2^16 values of a range check -- needs).  0 = accepted, RK_ERR_INVALID for malformed arguments, otherwise a reason: 1 malformed proof (short,
 * trailing or non-canonical words), 2 shape mismatch, 3 constraint identity (OodEvaluationMismatch), 4 proof of work,
 * 5 input opening, 6 commit-phase opening, 7 final polynomial, 8 the cumulative sums of the lookups do not cancel. */
int rk_p3_verify(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init_words, size_t n_init,
                 const uint32_t* proof, size_t proof_words);
/* CLAIMS: interactions the VERIFIER adds to the lookup argument of a proof.  A claim is n tuples of tuple_len Montgomery
 * words on one bus, each with multiplicity 1 (repeats allowed), sent (sign +1) or received (sign -1) by no table of the
 * proof.  rk_p3_verify_claims is rk_p3_verify (prep_root NULL) / rk_p3_verify_key with
 *     sum of the tables' cumulative sums + sum over the claims of sign / rlc(tuple) == 0
 * in place of a sum of zero, rlc = chal[0] + chal[1] bus + sum_j chal[2 + j] x_j under the proof's own permutation
 * challenges.  Reason 8: any other total, or a tuple whose rlc is zero.  RK_ERR_INVALID: a tuple longer than the tables'
 * challenges cover (4 (tuple_len + 2) > the largest n_chal of the tables), a non-canonical word, a sign that is not +-1,
 * NULL tuples with n != 0, or claims against tables without lookups.  n_claims == 0: exactly rk_p3_verify / rk_p3_verify_key.
 * THE CALLER'S DUTY: the challenges must not have been chosen knowing the tuples.  The tuples have to be bound into
 * init_words or into a public value of a table (both are observed before the challenges are sampled), e.g. by a digest
 * the caller recomputes; otherwise a prover picks the tuples after the challenges and the check is UNSOUND.  The function
 * does not do this itself. */
typedef struct {
    uint32_t bus;
    uint32_t tuple_len;
    int32_t sign;                  /* +1 the claim sends, -1 it receives */
    const uint32_t* tuples;        /* n x tuple_len Montgomery words, host */
    size_t n;
} rk_p3_claim;
int rk_p3_verify_claims(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* prep_root,
                        const uint32_t* init_words, size_t n_init, const uint32_t* proof, size_t proof_words,
                        const rk_p3_claim* claims, uint32_t n_claims);
/* rk_p3_verify that also hands back EVERY Poseidon2 permutation the check performed -- the transcript's, the leaf sponges
 * over the opened rows, the Merkle compressions, the proof of work's -- as input states (p2_width Montgomery words each,
 * in the order they happened): what the Poseidon2 chip of a recursion / compress layer has to prove for this proof
 * (rk_p2_chip_trace turns them into that chip's rows).  Returns the verifier's verdict (0 accepted, 1..8 the reason a
 * sequential check gives; the log then ends where the check stopped) or a negative status; RK_ERR_CAPACITY with
 * *n_permutations set when `states` holds fewer than that many: call again. */
int rk_p3_verify_hashes(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init_words, size_t n_init,
                        const uint32_t* proof, size_t proof_words, uint32_t* states, size_t capacity_permutations, size_t* n_permutations);
/* The commit phase of the FRI query check as lookup tables (one more piece of a recursion / compress layer; AIRs and host
 * witness: raiko_amd/fri_chip.py).  Parameter sets with the width-16 Poseidon2 and fri_fold_log2 = 1 (SP1's preset and
 * its blowup_log2 variants); any other is RK_ERR_INVALID.  L = log_max (tallest LDE), R = L - blowup_log2 rounds,
 * lfh(rd) = L - 1 - rd the height of round rd's commit-phase tree.
 * rk_p3_fri_openings: rk_p3_verify (same arguments, same verdict) that on verdict 0 also hands back, as Montgomery words,
 *   shape:   L, R, blowup_log2, queries
 *   publics: beta of every round (4 R) | commit-phase roots (8 R) | final polynomial (4)
 *   records: per query: the index | per round: the reduced opening that joins before it (rop[lfh + 1] when a table of
 *            that height exists, else zero) 4, the sibling value 4, its Merkle path 8 lfh
 * RK_ERR_CAPACITY with *publics_words / *records_words set when a buffer is too small: call again.  On any other verdict
 * nothing is written and both sizes are 0. */
int rk_p3_fri_openings(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init_words, size_t n_init,
                       const uint32_t* proof, size_t proof_words, uint32_t* shape, uint32_t* publics, size_t publics_capacity,
                       uint32_t* records, size_t records_capacity, size_t* publics_words, size_t* records_words);
/* The same calls over a proof under a verifying key: each _key function is its twin with prep_root as rk_p3_verify_key
 * takes it (the 8 words of rk_p3_key_root if and only if a table has prep_width > 0, whose log_height is then pinned;
 * otherwise RK_ERR_INVALID), returns rk_p3_verify_key's verdict, and with a NULL root and tables without preprocessed
 * columns hands back word for word what its twin does.  With a preprocessed batch:
 *   rk_p3_verify_hashes_key   the permutations of the keyed check: the observe of the root first in the transcript, the
 *                             fourth batch's leaf sponges and compressions per query behind the trace batch's
 *   rk_p3_fri_openings_key    the same format; the reduced openings include the preprocessed columns
 *   rk_p3_fri_inputs_key      layout: a preprocessed matrix carries batch 3 and points 2; the matrices stay in the
 *                             verifier's order, trace, preprocessed, permutation, quotient (the order of the alpha powers),
 *                             so the batch numbers run 0.., 3.., 1.., 2...  records: per query the index, then the opened
 *                             rows in that same order (a matrix's offset in a record is a running sum over the layout)
 *   rk_p3_fri_input_paths_key publics: the 25 words of rk_p3_fri_input_paths | the preprocessed root 8 (the caller's
 *                             prep_root) | log_kmax (the log LDE height of the preprocessed batch's tallest matrix): 34
 *                             words.  records: per query the paths in batch-number order: trace 8 L | permutation
 *                             8 log_pmax | quotient 8 L | preprocessed 8 log_kmax
 *   rk_p3_fri_transcript_key  the same format; `observed` holds the root between init and the trace root, where the
 *                             challenger observes it */
int rk_p3_verify_hashes_key(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* prep_root,
                            const uint32_t* init_words, size_t n_init, const uint32_t* proof, size_t proof_words, uint32_t* states,
                            size_t capacity_permutations, size_t* n_permutations);
int rk_p3_fri_openings_key(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* prep_root,
                           const uint32_t* init_words, size_t n_init, const uint32_t* proof, size_t proof_words, uint32_t* shape,
                           uint32_t* publics, size_t publics_capacity, uint32_t* records, size_t records_capacity, size_t* publics_words,
                           size_t* records_words);
int rk_p3_fri_inputs_key(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* prep_root,
                         const uint32_t* init_words, size_t n_init, const uint32_t* proof, size_t proof_words, uint32_t* shape, uint32_t* layout,
                         size_t layout_capacity, uint32_t* publics, size_t publics_capacity, uint32_t* records, size_t records_capacity,
                         size_t* layout_words, size_t* publics_words, size_t* records_words);
int rk_p3_fri_input_paths_key(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* prep_root,
                              const uint32_t* init_words, size_t n_init, const uint32_t* proof, size_t proof_words, uint32_t* shape,
                              uint32_t* publics, size_t publics_capacity, uint32_t* records, size_t records_capacity, size_t* publics_words,
                              size_t* records_words);
int rk_p3_fri_transcript_key(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* prep_root,
                             const uint32_t* init_words, size_t n_init, const uint32_t* proof, size_t proof_words, uint32_t* shape, uint32_t* ops,
                             size_t ops_capacity, uint32_t* observed, size_t observed_capacity, uint32_t* sampled, size_t sampled_capacity,
                             size_t* ops_words, size_t* observed_words, size_t* sampled_words);
/* The four tables of that statement for a shape: fold (one row per query and round), path (one row per Merkle step),
 * claims (query, round, index, reduced opening: free cells here; rk_fri_reduce_* below replaces them) and the Poseidon2 chip (one row per
 * leaf sponge and compression).  *_rows = rows in use, *_log_height = the power of two they are padded to (>= 1). */
typedef struct {
    uint32_t n_rounds;
    uint32_t fold_width, path_width, claims_width, chip_width;
    uint32_t fold_log_height, path_log_height, claims_log_height, chip_log_height;
    uint32_t reserved;
    uint64_t fold_rows, path_rows, chip_rows;
    uint64_t publics_words, records_words;
} rk_fri_chip_size_info;
int rk_fri_chip_sizes(uint32_t log_max, uint32_t blowup_log2, uint32_t queries, rk_fri_chip_size_info* out);
/* The rows of all four tables on the GPU from the uploaded publics and records (d_*, as rk_p3_fri_openings wrote them),
 * under the context's parameter set: a fold kernel (one lane per query walks its rounds: fold and claim rows), a path
 * kernel (one lane per query and round, round-major so that a wave's lanes share the path length: leaf sponge, lfh
 * compressions, path rows, the chip's inputs), then rk_p2_chip_trace over those inputs (padding inputs: multiplicity 0).
 * Each d_* table is 2^log_height x width Montgomery words row-major (rk_fri_chip_sizes), ready as an on_device
 * rk_p3_table; *_capacity in words.  A buffer smaller than its table: RK_ERR_CAPACITY before anything is launched. */
int rk_fri_chip_rows_device(rk_ctx* ctx, uint32_t log_max, uint32_t blowup_log2, uint32_t queries, const uint32_t* d_publics,
                            const uint32_t* d_records, uint32_t* d_fold, size_t fold_capacity, uint32_t* d_path, size_t path_capacity,
                            uint32_t* d_claims, size_t claims_capacity, uint32_t* d_chip, size_t chip_capacity);
/* The reduced openings of the FRI query check as a lookup table: a second, larger statement beside the one above (AIRs
 * and host witness: raiko_amd/fri_reduce.py; same scope).  Its four tables are fold' (the fold table with one more
 * column, the domain point X of the query in that round, which joins the claim it sends), path, reduce and the chip: the
 * claims table is gone, the reduced opening that joins the fold chain in a round is now the one the reduce table computes
 * from the rows the shard proof opened.  For one query and one LDE height the verifier's sum over every opened column,
 * sum_k alpha^k (p_k(x) - y_k) / (x - z_k), is grouped by (matrix, point) into (sum_k alpha^k p_k(x) - S) / (x - z) with
 * S = sum_k alpha^k y_k over the same absolute powers; S, the group's first power A and z do not depend on the query.
 * Still free in that statement: the query indices, the opened values themselves (one cell P per query and column: their
 * Merkle openings are not proven here; rk_fri_open_* below does) and the transcript-derived public values, which the host
 * binds to the shard proof.
 * rk_p3_fri_inputs: rk_p3_verify (same arguments, same verdict) that on verdict 0 also hands back, as Montgomery words,
 *   shape:   L, R, blowup_log2, queries
 *   layout:  per opened matrix, in the verifier's order (trace batch per table, then the permutation batch, then every
 *            quotient chunk): batch (0 trace, 1 permutation, 2 quotient), round L - lh, width, points (2: zeta and
 *            zeta gen(log_n); quotient chunks 1: zeta), log_n
 *   publics: alpha 4 | zeta 4 | per matrix, per point: A 4, S 4
 *   records: per query: the index | trace rows | permutation rows | quotient rows (no Merkle paths)
 * RK_ERR_CAPACITY with the three *_words set when a buffer is too small: call again.  On any other verdict nothing is
 * written and the sizes are 0. */
int rk_p3_fri_inputs(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init_words, size_t n_init,
                     const uint32_t* proof, size_t proof_words, uint32_t* shape, uint32_t* layout, size_t layout_capacity, uint32_t* publics,
                     size_t publics_capacity, uint32_t* records, size_t records_capacity, size_t* layout_words, size_t* publics_words,
                     size_t* records_words);
/* The four tables of that statement for a shape and a layout (n_matrices entries of 5 words, as rk_p3_fri_inputs wrote
 * them, or rk_p3_fri_inputs_key: batch 3 = preprocessed, points 2; the batches in the order 0, 3, 1, 2, a trace matrix
 * first; anything else is RK_ERR_INVALID).  The reduce table has one row per (query, slot, column): the slots are the
 * matrices ordered by round (the
 * layout's order within a round) and one single-row slot for every round without a matrix; rows_per_query = the sum of
 * their widths.  reduce_publics_words = 8 + 16 n_slots: alpha | zeta | per slot A, S of the first point, A, S of the
 * second (zero where the slot has no such point). */
typedef struct {
    uint32_t n_rounds, n_slots;
    uint32_t fold_width, path_width, reduce_width, chip_width;
    uint32_t fold_log_height, path_log_height, reduce_log_height, chip_log_height;
    uint64_t fold_rows, path_rows, reduce_rows, chip_rows, rows_per_query;
    uint64_t fold_publics_words, fold_records_words, reduce_publics_words, inputs_words;
} rk_fri_reduce_size_info;
int rk_fri_reduce_sizes(uint32_t log_max, uint32_t blowup_log2, uint32_t queries, const uint32_t* layout, uint32_t n_matrices,
                        rk_fri_reduce_size_info* out);
/* The rows of all four tables on the GPU: the fold and path kernels of rk_fri_chip_rows_device (the fold rows with the
 * extra column, no claim rows) over d_fold_publics / d_fold_records (as rk_p3_fri_openings wrote them), a reduce kernel
 * over d_reduce_publics (slot order, rk_fri_reduce_sizes) and d_inputs (the records of rk_p3_fri_inputs) -- a workgroup
 * per (query, round), its lanes along the columns of a matrix, running sums by wave scans --, then rk_p2_chip_trace.
 * `layout` is host memory.  A buffer smaller than its table (RK_ERR_CAPACITY), a layout that does not fit the shape or a
 * blow-up that is not the context's (RK_ERR_INVALID) is refused before anything is launched. */
int rk_fri_reduce_rows_device(rk_ctx* ctx, uint32_t log_max, uint32_t blowup_log2, uint32_t queries, const uint32_t* layout, uint32_t n_matrices,
                              const uint32_t* d_fold_publics, const uint32_t* d_fold_records, const uint32_t* d_reduce_publics,
                              const uint32_t* d_inputs, uint32_t* d_fold, size_t fold_capacity, uint32_t* d_path, size_t path_capacity,
                              uint32_t* d_reduce, size_t reduce_capacity, uint32_t* d_chip, size_t chip_capacity);
/* The input-batch Merkle openings of the FRI query check as lookup tables: a third statement beside the two above (AIRs
 * and host witness: raiko_amd/fri_open.py; the scope of the other two and p2_pad_free = 1).  Six tables: fold', path,
 * reduce'' (the reduce table with sponge columns: the opened cells P of the matrices of one (round, batch) are absorbed
 * in place, the group's digest is sent to ipath), ipath (one row per query, batch and Merkle level of the three input
 * trees: compress with the proof's sibling, and where shorter matrices join compress(node, their digest), up to the
 * batch's root, a public value), the chip, and a state chip (the same permutation AIR with all 16 output cells in its
 * receive, rk_p2_chip_air_ex) that the sponge's permutations are looked up in.
 * rk_p3_fri_input_paths: rk_p3_verify (same arguments, same verdict) that on verdict 0 also hands back, as Montgomery words,
 *   publics: trace root 8 | permutation root 8 (zeros when no table has lookups) | quotient root 8 | log_pmax (the log
 *            LDE height of the permutation batch's tallest matrix, 0 without one)
 *   records: per query: trace path 8 L | permutation path 8 log_pmax | quotient path 8 L
 * with the capacity protocol of rk_p3_fri_inputs. */
int rk_p3_fri_input_paths(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init_words, size_t n_init,
                          const uint32_t* proof, size_t proof_words, uint32_t* shape, uint32_t* publics, size_t publics_capacity,
                          uint32_t* records, size_t records_capacity, size_t* publics_words, size_t* records_words);
/* The six tables for a shape and a layout.  n_groups = the (round, batch) groups of a query, n_batches = the input trees
 * (2 to 4, in batch-number order: the preprocessed tree's ipath rows, chip inputs and paths come last); state_rows =
 * queries x the sponge permutations of a query, chip_rows = those of the reduce statement plus one per ipath row and
 * injection.  roots_words / paths_words: what rk_p3_fri_input_paths(_key) hands back -- roots_words is 34 exactly when the
 * layout has a batch-3 matrix, and d_roots must then be the 34-word form: the device cannot tell, the caller checks.
 * log_kmax: the log LDE height of the preprocessed batch's tallest matrix, 0 without one; a batch-3 matrix cannot be
 * taller than log_max, trace and quotient must reach it. */
typedef struct {
    uint32_t n_rounds, n_slots, n_groups, n_batches, log_pmax, log_kmax;
    uint32_t fold_width, path_width, reduce_width, ipath_width, chip_width, state_width;
    uint32_t fold_log_height, path_log_height, reduce_log_height, ipath_log_height, chip_log_height, state_log_height;
    uint64_t fold_rows, path_rows, reduce_rows, ipath_rows, chip_rows, state_rows, rows_per_query;
    uint64_t fold_publics_words, fold_records_words, reduce_publics_words, inputs_words, roots_words, paths_words;
} rk_fri_open_size_info;
int rk_fri_open_sizes(uint32_t log_max, uint32_t blowup_log2, uint32_t queries, const uint32_t* layout, uint32_t n_matrices,
                      rk_fri_open_size_info* out);
/* The rows of all six tables on the GPU: the kernels of rk_fri_reduce_rows_device (the reduce rows at the wider stride),
 * then a sponge kernel (one lane per query and group: the chain of permutations over the group's cells), a fill kernel
 * (one lane per reduce row: the sponge columns), an ipath kernel (one lane per query and batch over d_paths, the records
 * of rk_p3_fri_input_paths; d_roots = its publics) and rk_p2_chip_trace twice.  Refusals as rk_fri_reduce_rows_device,
 * and a context whose sponge pads (p2_pad_free = 0) is RK_ERR_INVALID; all before anything is launched. */
int rk_fri_open_rows_device(rk_ctx* ctx, uint32_t log_max, uint32_t blowup_log2, uint32_t queries, const uint32_t* layout, uint32_t n_matrices,
                            const uint32_t* d_fold_publics, const uint32_t* d_fold_records, const uint32_t* d_reduce_publics,
                            const uint32_t* d_inputs, const uint32_t* d_roots, const uint32_t* d_paths, uint32_t* d_fold, size_t fold_capacity,
                            uint32_t* d_path, size_t path_capacity, uint32_t* d_reduce, size_t reduce_capacity, uint32_t* d_ipath,
                            size_t ipath_capacity, uint32_t* d_chip, size_t chip_capacity, uint32_t* d_state, size_t state_capacity);
/* The Fiat-Shamir transcript of the FRI query check as lookup tables: a fourth statement beside the three above (AIRs and
 * host witness: raiko_amd/fri_transcript.py; the scope of rk_fri_open_* and pow_bits <= 27).  Eight tables: fold'' (fold'
 * with one more column FIRST, with which a query's first row receives (query, index) from the bits table), path,
 * reduce'', ipath, transcript (one row per duplex permutation of rk_p3_verify's challenger: what it absorbs and what is
 * sampled from it are public values, every cell it keeps is the row before's output), bits (one row per sample_bits: the
 * canonical 31-bit form of the sampled cell, its low bits the proof-of-work check and the query indices), the chip and the
 * state chip, which now also holds the transcript's permutations.
 * rk_p3_fri_transcript: rk_p3_verify (same arguments, same verdict) that on verdict 0 also hands back, as Montgomery words,
 *   ops:      the challenger's calls in order as pairs (kind, count): 0 observe `count` words (an empty observe is left
 *             out), 1 sample `count` field elements, 2 sample_bits(count)
 *   observed: every observed word, concatenated
 *   sampled:  every sampled field element in order, those behind sample_bits included
 * with the capacity protocol of rk_p3_fri_inputs. */
int rk_p3_fri_transcript(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables, const uint32_t* init_words, size_t n_init,
                         const uint32_t* proof, size_t proof_words, uint32_t* shape, uint32_t* ops, size_t ops_capacity, uint32_t* observed,
                         size_t observed_capacity, uint32_t* sampled, size_t sampled_capacity, size_t* ops_words, size_t* observed_words,
                         size_t* sampled_words);
/* The eight tables for a shape, a layout and the challenger's calls (n_ops pairs, as rk_p3_fri_transcript wrote them; host
 * memory).  The calls must end in queries + 1 sample_bits with nothing between them: the proof of work (pow_bits <= 27),
 * then one of log_max bits per query.  n_steps = the duplex permutations = transcript_rows; bits_rows = queries + 1;
 * state_rows = those of the open statement + n_steps; transcript_publics_words = observed_words + the field elements
 * sampled by kind 1. */
typedef struct {
    uint32_t n_rounds, n_slots, n_groups, n_batches, log_pmax, n_steps, pow_bits, log_kmax;
    uint32_t fold_width, path_width, reduce_width, ipath_width, transcript_width, bits_width, chip_width, state_width;
    uint32_t fold_log_height, path_log_height, reduce_log_height, ipath_log_height, transcript_log_height, bits_log_height, chip_log_height,
        state_log_height;
    uint64_t fold_rows, path_rows, reduce_rows, ipath_rows, transcript_rows, bits_rows, chip_rows, state_rows, rows_per_query;
    uint64_t fold_publics_words, fold_records_words, reduce_publics_words, inputs_words, roots_words, paths_words, observed_words,
        transcript_publics_words;
} rk_fri_transcript_size_info;
int rk_fri_transcript_sizes(uint32_t log_max, uint32_t blowup_log2, uint32_t queries, const uint32_t* layout, uint32_t n_matrices,
                            const uint32_t* ops, uint32_t n_ops, rk_fri_transcript_size_info* out);
/* The rows of all eight tables on the GPU: the kernels of rk_fri_open_rows_device (the fold rows with FIRST), then a chain
 * kernel (one wave: a half-wave walks the challenger's permutations one after the other, one lane per state cell, over
 * d_observed; it writes IN and OUT of every transcript row, the state chip's inputs behind the sponge's, and the cells
 * sample_bits consumed), a fill kernel (one lane per transcript row: step one-hot and helpers; one lane per bits row) and
 * rk_p2_chip_trace twice.  Refusals as rk_fri_open_rows_device, and calls that do not fit the shape are RK_ERR_INVALID;
 * all before anything is launched. */
int rk_fri_transcript_rows_device(rk_ctx* ctx, uint32_t log_max, uint32_t blowup_log2, uint32_t queries, const uint32_t* layout,
                                  uint32_t n_matrices, const uint32_t* ops, uint32_t n_ops, const uint32_t* d_fold_publics,
                                  const uint32_t* d_fold_records, const uint32_t* d_reduce_publics, const uint32_t* d_inputs,
                                  const uint32_t* d_roots, const uint32_t* d_paths, const uint32_t* d_observed, uint32_t* d_fold,
                                  size_t fold_capacity, uint32_t* d_path, size_t path_capacity, uint32_t* d_reduce, size_t reduce_capacity,
                                  uint32_t* d_ipath, size_t ipath_capacity, uint32_t* d_transcript, size_t transcript_capacity,
                                  uint32_t* d_bits, size_t bits_capacity, uint32_t* d_chip, size_t chip_capacity, uint32_t* d_state,
                                  size_t state_capacity);
/* exact proof size for the tables' shapes (log_height, width, air); 0 for shapes rk_p3_prove rejects */
size_t rk_p3_proof_bound_words(const rk_params* params, const rk_p3_table* tables, uint32_t n_tables);
/* Many independent proofs -- the shards of one SP1 execution -- with `batch` of them in flight per GPU: what SP1's
 * SHARD_BATCH_SIZE bounds (docs/README_Sp1.md:27-32; shards are proven from one work queue, the latency-bound parts of
 * one proof -- transcript round trips, the small FRI layers -- under the throughput-bound parts of the others).  One
 * worker thread and prover context per slot, kept per device for the life of the process like rk_prove_session's
 * (rk_session_release frees them too); proof i lands in shards[i].h_proof.  verify != 0: every proof is checked with
 * rk_p3_verify on host threads of their own while the GPU goes on.  Returns RK_OK or the first failure (RK_ERR_VERIFY for a
 * proof that does not verify) with the shard's index in *failed_index. */
typedef struct {
    const rk_p3_table* tables;
    uint32_t n_tables;
    const uint32_t* init_words;
    size_t n_init;
    uint32_t* h_proof;
    size_t capacity_words;
    size_t proof_words;            /* out */
} rk_p3_shard;
typedef struct {
    int device;                    /* the GPU, when n_devices == 0 */
    int batch;                     /* proofs in flight per GPU, 1..16 (SHARD_BATCH_SIZE) */
    int verify;
    const int* devices;            /* optional list of distinct GPUs sharing the work queue */
    int n_devices;
    const rk_params* params;       /* NULL = the SP1 preset */
} rk_p3_session_opts;
int rk_p3_prove_shards(const rk_p3_session_opts* opts, rk_p3_shard* shards, size_t n, size_t* failed_index);
/* rk_p3_prove_shards under a key (rk_p3_setup): the way shards whose tables have preprocessed columns go through the pool.
 * keys[d] = the key for the d-th device AS THE CALLER LISTED THEM in opts->devices (one entry, for opts->device, when
 * n_devices == 0); keys == NULL is rk_p3_prove_shards.  Workers prove with rk_p3_prove_key, verifiers check with
 * rk_p3_verify_key against the keys' root.  A key is read-only after rk_p3_setup, which drains its stream before it
 * returns: any number of contexts of its GPU may read one key concurrently, which is what the pool's slots do.
 * RK_ERR_INVALID before any context is created or configured: a NULL entry, a key of another GPU than its slot's, keys
 * whose roots differ from each other (or some with a root and some without), a key made under another parameter set
 * than opts->params, a shard whose table count, prep_width or -- where prep_width > 0 -- log_height is not the key's
 * (*failed_index = that shard).  A key over tables without preprocessed columns gives rk_p3_prove_shards' exact proofs. */
int rk_p3_prove_shards_key(const rk_p3_session_opts* opts, const rk_p3_key* const* keys, rk_p3_shard* shards, size_t n,
                           size_t* failed_index);
/* rk_p3_prove_shards / rk_p3_prove_shards_key (keys NULL: the former) whose verifier threads call rk_p3_verify_claims:
 * claims[i] / n_claims[i] are shard i's claims (see rk_p3_verify_claims, and the caller's duty there).  claims == NULL
 * behaves as rk_p3_prove_shards_key; with claims, n_claims must not be NULL.  rk_p3_shard keeps its layout. */
int rk_p3_prove_shards_claims(const rk_p3_session_opts* opts, const rk_p3_key* const* keys, rk_p3_shard* shards,
                              const rk_p3_claim* const* claims, const uint32_t* n_claims, size_t n, size_t* failed_index);
/* wall-clock per stage of the last rk_p3_prove on this ctx, milliseconds (the stream is drained at every boundary) */
typedef struct { float lde, commit, quotient, open, fri, query, total, perm /* permutation traces + their LDE */; } rk_p3_timing;
int rk_p3_last_timing(rk_ctx* ctx, rk_p3_timing* out);

/* per-stage device time of the last rk_prove_segment on this ctx, milliseconds (hipEvent) */
typedef struct { float ntt, hash, deep, fri, query, total, circuit /* time inside rk_circuit_hooks */; } rk_timing;
int rk_last_timing(rk_ctx* ctx, rk_timing* out);

/* ---- per-kernel-class timing (for bench.py's roofline object) ----
 * When enabled every launch of a class is bracketed by a hipEvent pair on the ctx stream;
 * rk_kernel_stats synchronises the stream and returns launches, total device milliseconds and
 * total ALGORITHMIC bytes (what the launch must read + write once) since the last reset. */
typedef enum {
    RK_KCLASS_HASH_ROWS = 0,   /* hash_rows_kernel */
    RK_KCLASS_HASH_FOLD = 1,   /* hash_fold_kernel */
    RK_KCLASS_NTT_PASS = 2,    /* ntt_pass_kernel<fwd|rev> */
    RK_KCLASS_BIT_REVERSE = 3, /* bit_reverse_kernel */
    RK_KCLASS_POLY = 4,        /* mix / eval / divide / fold / sum kernels */
    RK_KCLASS_COUNT = 5
} rk_kclass;
typedef struct { uint64_t launches; double ms; double bytes; } rk_kernel_stat;
int rk_set_kernel_timing(rk_ctx* ctx, int enabled);   /* also resets the counters */
int rk_kernel_stats(rk_ctx* ctx, int kclass, rk_kernel_stat* out);
const char* rk_kernel_class_name(int kclass);
/* the same for the prover contexts rk_prove_session keeps for `device`: enable / reset, then the
 * totals over all of them (what bench.py reads after timing the drop-in entry point) */
int rk_session_set_kernel_timing(int device, int enabled);
int rk_session_kernel_stats(int device, int kclass, rk_kernel_stat* out);

#ifdef __cplusplus
}
#endif
#endif /* RAIKO_HIP_H */
