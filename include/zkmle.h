/*
 * zkmle.h -- C ABI of libzkmle_amd.so: the MI355X (gfx950) implementation of the multilinear
 * hot path of casweeney/zk-cryptography-research-implementations.
 *
 * The reference has no FFI layer: its path is reached through generic Rust items.
 * Each entry point below replaces the reference item cited next to it; the Rust shim that binds
 * them is shown in INTEGRATION.md (rust_shim/ holds its source).
 *
 * Conventions
 *   - field elements: `limbs` little-endian u64 limbs in Montgomery form, R = 2^(64*limbs) -- the
 *     in-memory layout of an arkworks `Fp`, so `&[Fr]` / `Vec<F>` can be passed by pointer;
 *   - tables: contiguous arrays of elements; index bit (n-1-v) <-> variable v (variable 0 = MSB),
 *     evaluation_form.rs:76-80;
 *   - every function returns a zk_status; precondition failures that PANIC in the reference
 *     return the matching negative code and never abort (zk_status_message gives the
 *     reference's panic text);
 *   - `zk_table` handles own device (HBM) memory; host pointers stay owned by the caller;
 *   - a handle is used by one thread at a time; the library is re-entrant after zk_init.
 * The library NEVER falls back to a CPU path: without a usable HIP device every compute entry
 * point returns ZK_E_NO_DEVICE.
 */
#ifndef ZKMLE_H
#define ZKMLE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { ZK_FR381 = 0, ZK_FQ381 = 1, ZK_BN254_FQ = 2, ZK_BN254_FR = 3 } zk_field;

typedef enum {
    ZK_OK = 0,
    ZK_E_NOT_POW2 = -1,     /* "Evaluated values must be a power of 2"  evaluation_form.rs:13 */
    ZK_E_LEN_MISMATCH = -2, /* evaluation_form.rs:112,129-132,149-153 */
    ZK_E_NVARS = -3,        /* "different number of variables" product_polynomial.rs:16-21, sum_polynomial.rs:17-23 */
    ZK_E_NEED_TWO = -4,     /* product_polynomial.rs:59-62, sum_polynomial.rs:58-61 */
    ZK_E_KZG_LEN = -5,      /* multilinear_kzg.rs:29-33,55-64 */
    ZK_E_RANGE = -6,        /* implicit index / underflow panics */
    ZK_E_ARG = -7,          /* bad argument at the C boundary (no reference counterpart) */
    ZK_E_NOMEM = -8,
    ZK_E_NO_DEVICE = -9,    /* no usable HIP device: the product path has no CPU fallback */
    ZK_E_HIP = -10,         /* a HIP runtime call failed; see zk_last_error */
    ZK_E_NOT_INIT = -11,    /* "Can't prove without init" prover.rs:36 */
    ZK_E_COMM = -12         /* an RCCL call or a caller-supplied exchange callback failed; see zk_last_error */
} zk_status;

const char *zk_status_message(int status);
const char *zk_last_error(void);      /* thread-local detail for ZK_E_HIP */
const char *zk_version(void);

/* ---- device ------------------------------------------------------------------------------- */
int zk_device_count(int *count);
int zk_init(int device);              /* select the device for the calling thread's later calls */
int zk_field_limbs(int field);        /* u64 limbs per element (4 or 6), negative on bad field */
int zk_device_synchronize(void);
/* Streams and threads: every launch, copy and wait of the library runs on the CALLING THREAD's current stream -- the
 * default (NULL) stream unless zk_set_stream was called on that thread.  A handle is used by one thread at a time; threads
 * that set different streams run their calls concurrently on the device (scratch buffers, staging buffers and the *_stats
 * are per thread; cached scratch blocks are reused only on the stream they last served).  The `stream` argument of the
 * zk_mle_* calls, when not NULL, overrides the thread's stream for that call. */
int zk_set_stream(void *hip_stream);
void *zk_get_stream(void);
int zk_release_cached_memory(void);   /* frees the library's cached per-call scratch (MSM workspaces) on the current device */

/* ---- device-resident tables ----------------------------------------------------------------
 * MultilinearPolynomial<F>{evaluated_values: Vec<F>}  evaluation_form.rs:7-18 */
typedef struct zk_table zk_table;
int zk_table_alloc(int field, size_t len, zk_table **out);                 /* uninitialised */
int zk_table_upload(int field, const uint64_t *host, size_t len, zk_table **out);  /* MultilinearPolynomial::new :12 (asserts pow2) */
/* plain vector upload without the power-of-two assert (MSM scalars, W layers): any len >= 1 */
int zk_table_upload_raw(int field, const uint64_t *host, size_t len, zk_table **out);
int zk_table_download(const zk_table *t, uint64_t *host);
int zk_table_free(zk_table *t);
size_t zk_table_len(const zk_table *t);
int zk_table_field(const zk_table *t);
void *zk_table_device_ptr(zk_table *t);                                    /* raw HBM pointer */
int zk_table_wrap(int field, void *device_ptr, size_t len, zk_table **out); /* non-owning view of caller's HBM */
int zk_table_clone(const zk_table *t, zk_table **out);
/* synthetic benchmark data: element i = SplitMix64-derived 4 (6) words reduced mod p */
int zk_table_fill_random(zk_table *t, uint64_t seed);
/* local entry j <- element (first + j * stride) of the stream `seed`: rank g of G generates its low-bit shard of a global
 * table with (first, stride) = (g, G), its contiguous slice of an MSM's scalars with (g * n / G, 1) */
int zk_table_fill_random_strided(zk_table *t, uint64_t seed, size_t first, size_t stride);
/* host mirror of the generator (same bytes), for parity tests */
int zk_host_fill_random(int field, uint64_t seed, size_t first, size_t count, uint64_t *out);

/* ---- MLE operations on device tables --------------------------------------------------------
 * every `stream` argument is a hipStream_t (NULL = the null stream) */
/* partial_evaluate  evaluation_form.rs:61-106.  out: len/2 elements (out != in) */
int zk_mle_fold(const zk_table *in, size_t var, const uint64_t *value, zk_table *out, void *stream);
/* the same on raw device pointers (HBM-resident slices of a caller-managed buffer) */
int zk_mle_fold_ptr(int field, const void *d_in, size_t len, size_t var, const uint64_t *value,
                    void *d_out, void *stream);
/* evaluate  evaluation_form.rs:21-33 : nvalues successive var-0 folds, element 0 */
int zk_mle_evaluate(const zk_table *t, const uint64_t *values, size_t nvalues, uint64_t *out);
/* convert_to_bytes  :35-43 : canonical big-endian bytes, len*8*limbs */
int zk_mle_to_bytes(const zk_table *t, uint8_t *host_out);
/* scalar_mul :49, add_polynomials :145, polynomial_tensor_add :108, polynomial_tensor_mul :125 */
int zk_mle_scalar_mul(const zk_table *a, const uint64_t *scalar, zk_table *out, void *stream);
int zk_mle_add(const zk_table *a, const zk_table *b, zk_table *out, void *stream);
int zk_mle_sub_scalar(const zk_table *a, const uint64_t *scalar, zk_table *out, void *stream); /* multilinear_kzg.rs:74-78 */
/* out = sum_j coeffs[j] * tables[j]  (k tables of equal length, 1 <= k <= 64; coeffs: k elements, Montgomery): scalar_mul :49 and
 * add_polynomials :145 of k tables in one pass.  A table may be passed more than once; out must not overlap any of them.
 * ZK_E_NVARS: unequal lengths; ZK_E_ARG: k = 0, k > 64, mixed fields, out too short or overlapping.  Extension: no reference counterpart. */
int zk_mle_linear_combination(const zk_table *const *tables, size_t k, const uint64_t *coeffs, zk_table *out, void *stream);
int zk_mle_tensor_add(const zk_table *wb, const zk_table *wc, zk_table *out, void *stream);
int zk_mle_tensor_mul(const zk_table *wb, const zk_table *wc, zk_table *out, void *stream);
/* iter().sum()  prover.rs:28 ; and split_polynomial_and_sum_each prover.rs:74-89 (out2: 2 elements) */
int zk_mle_sum(const zk_table *t, uint64_t *out);
int zk_mle_half_sums(const zk_table *t, uint64_t *out2);
/* fused sumcheck round: fold by `value` AND return the folded table's two half sums (the next
 * round's univariate) in one pass over HBM */
int zk_mle_fold_half_sums(const zk_table *in, const uint64_t *value, zk_table *out, uint64_t *out2,
                          void *stream);

/* ---- stateless host-buffer conveniences (upload, compute on the GPU, download) --------------- */
int zk_host_partial_evaluate(int field, const uint64_t *poly, size_t len, size_t var,
                             const uint64_t *value, uint64_t *out);
int zk_host_evaluate(int field, const uint64_t *poly, size_t len, const uint64_t *values,
                     size_t nvalues, uint64_t *out);

/* ---- host-side helpers (CPU, tiny: control path) -------------------------------------------- */
int zk_fe_from_u64(int field, uint64_t v, uint64_t *out);
int zk_fe_to_bytes_be(int field, const uint64_t *a, uint8_t *out);
int zk_fe_from_le_bytes_mod_order(int field, const uint8_t *bytes, size_t n, uint64_t *out);
int zk_fe_add(int field, const uint64_t *a, const uint64_t *b, uint64_t *out);
int zk_fe_sub(int field, const uint64_t *a, const uint64_t *b, uint64_t *out);
int zk_fe_mul(int field, const uint64_t *a, const uint64_t *b, uint64_t *out);
int zk_fe_inv(int field, const uint64_t *a, uint64_t *out);
int zk_vec_from_canonical(int field, const uint64_t *canon, size_t n, uint64_t *mont);
int zk_vec_to_canonical(int field, const uint64_t *mont, size_t n, uint64_t *canon);

/* ---- Fiat-Shamir transcript (host; transcripts/src/fiat_shamir/fiat_shamir_transcript.rs:5-43) ---- */
typedef struct zk_transcript zk_transcript;
int zk_transcript_new(zk_transcript **out);                                        /* Transcript::new :12 */
int zk_transcript_free(zk_transcript *t);
int zk_transcript_append(zk_transcript *t, const uint8_t *data, size_t n);         /* append :22 */
int zk_transcript_sample(zk_transcript *t, uint8_t out32[32]);                     /* sample_random_challenge :29 */
int zk_transcript_challenge(zk_transcript *t, int field, uint64_t *out);           /* random_challenge_as_field_element :38 */
int zk_keccak256(const uint8_t *data, size_t n, uint8_t out32[32]);
/* the running sponge as 25 Keccak lanes + the fill of the open block: what one rank hands to the others after absorbing
 * input only it has seen (the whole-table absorb of a sharded Prover::prove) */
int zk_transcript_export_state(const zk_transcript *t, uint64_t lanes25[25], uint32_t *fill);
int zk_transcript_import_state(zk_transcript *t, const uint64_t lanes25[25], uint32_t fill);

/* ---- Merkle commitment of a table (extension: the reference's merkle_tree/ crate is empty; csrc/merkle.cuh) ----------
 * For a table of len = 2^d elements of any of the four fields:
 *   leaf_i = Keccak256(0x00 || bytes(e_i))      bytes = convert_to_bytes of ONE element (evaluation_form.rs:35-43): the canonical
 *                                               integer big-endian, 8 * limbs bytes (32 or 48)
 *   node   = Keccak256(0x01 || left || right)   node j of level l + 1 hashes nodes 2j and 2j + 1 of level l;
 *                                               level 0 = the leaves in table-index order
 *   root   = the single node of level d; a one-entry table's root is leaf_0.
 * Keccak256 is the transcript's: the ORIGINAL Keccak (pad 0x01 .. 0x80, rate 136), not SHA3-256.  Every input is 33, 49 or 65 bytes,
 * one block, so a hash is one permutation; the kernels run one hash per GPU lane.  A length that is not a power of two returns
 * ZK_E_NOT_POW2; NULL arguments and bad fields ZK_E_ARG.  Launches go on the calling thread's stream; one synchronisation per call.
 * zk_mle_merkle_root returns nothing but the root (what the committed provers call): its levels go through one scratch block of the
 * caching pool, 64 bytes x len (1 GiB for 2^24 entries), which the calling thread's pool keeps for the next call as it does every
 * per-call scratch (zk_release_cached_memory).  zk_merkle_build keeps every level in HBM (64 bytes x len), which is what openings
 * need; the tree is a long-lived allocation of its own (hipMalloc / hipFree), so zk_merkle_build and zk_merkle_free are NOT
 * stream-ordered: the free may wait for the whole device, and the build's time includes the allocation. */
int zk_mle_merkle_root(const zk_table *t, uint8_t root32[32]);
typedef struct zk_merkle_tree zk_merkle_tree;
int zk_merkle_build(const zk_table *t, zk_merkle_tree **out);
int zk_merkle_free(zk_merkle_tree *m);
size_t zk_merkle_depth(const zk_merkle_tree *m);
int zk_merkle_root(const zk_merkle_tree *m, uint8_t root32[32]);
/* the authentication paths of `nidx` entries, gathered by one kernel and one download: paths = nidx x depth x 32 bytes, for each
 * index the leaf's sibling first, the root's child last.  An index >= len returns ZK_E_RANGE (nothing is written). */
int zk_merkle_open(const zk_merkle_tree *m, const size_t *indices, size_t nidx, uint8_t *paths);
/* HOST only, O(depth) hashes, needs no device: *ok = 1 when `element` (Montgomery limbs) at `index` hashes up `path` to root32.
 * index >= 2^depth returns ZK_E_RANGE. */
int zk_merkle_verify(int field, const uint8_t root32[32], size_t depth, size_t index, const uint64_t *element,
                     const uint8_t *path, int *ok);
/* Merkle commitment with grouped leaves (csrc/merkle.cuh merkle_leaf_group_kernel).  For a table of len = 2^d elements of 32 bytes (the 48-byte
 * field is ZK_E_ARG) and log_group = g in {1, 2}, with part = len >> g:
 *   leaf_j = Keccak256(0x00 || bytes(e_j) || bytes(e_{j + part}) || .. || bytes(e_{j + (2^g - 1) part})),  j < part
 * -- the 2^g entries a FRI fold of arity 2^g reads together -- 65 bytes for g = 1, 129 bytes for g = 2: with the pad's two bytes still inside
 * the 136-byte rate, so a leaf over the group is the ONE permutation a leaf over one element is.  The pair leaf has a node's length but a
 * leaf's tag.  Nodes and root are as above over `part` leaves: the tree has 2 part - 1 digests and depth d - g, and zk_merkle_open (indices
 * below part), zk_merkle_root, zk_merkle_depth and zk_merkle_free work on it as they are.  log_group = 0 is zk_merkle_build /
 * zk_mle_merkle_root.  ZK_E_ARG for NULL, log_group > 2, a field whose elements are not 32 bytes or len < 2^log_group, then ZK_E_NOT_POW2,
 * all before the device is touched. */
int zk_merkle_build_grouped(const zk_table *t, uint32_t log_group, zk_merkle_tree **out);
int zk_mle_merkle_root_grouped(const zk_table *t, uint32_t log_group, uint8_t root32[32]);   /* root-only mode: scratch of 64 bytes x part */
/* HOST only: *ok = 1 when the 2^log_group `elements` (Montgomery limbs, in the leaf's order) of leaf `index` hash up `path` (depth digests)
 * to root32; an element that is not reduced gives *ok = 0.  log_group > 2 or a 48-byte field: ZK_E_ARG; index >= 2^depth: ZK_E_RANGE. */
int zk_merkle_verify_grouped(int field, const uint8_t root32[32], size_t depth, size_t index, uint32_t log_group, const uint64_t *elements,
                             const uint8_t *path, int *ok);
/* Merkle commitment of several columns (csrc/merkle_columns.cuh merkle_leaf_columns_kernel).  k tables ("columns") f_0 .. f_{k-1} of one
 * scalar field (ZK_FR381 or ZK_BN254_FR) and one length len = 2^d >= 4 under ONE tree, 1 <= k <= 32.  With part = len >> 2:
 *   leaf_j = Keccak256(0x00 || for c < k: for s < 4: bytes(f_c[j + s part])),  j < part
 * -- 1 + 128 k bytes: each column's quad in the order of the grouped leaf with log_group = 2, behind one tag; elements canonical big-endian;
 * the hash is the transcript's Keccak (rate 136, pad 0x01 .. 0x80), B(k) = floor((1 + 128 k) / 136) + 1 permutations a leaf.  k = 1 is the
 * grouped quad leaf byte for byte, so a one-column tree has zk_merkle_build_grouped(t, 2)'s root.  Nodes and root are as above over `part`
 * leaves: 2 part - 1 digests, depth d - 2, and zk_merkle_open (indices below part), zk_merkle_root, zk_merkle_depth and zk_merkle_free work
 * on the tree as they are.  ZK_E_ARG for NULL, k outside 1 .. 32, any other field, mixed fields or len < 4, then ZK_E_LEN_MISMATCH for unequal
 * lengths, then ZK_E_NOT_POW2, all before the device is touched. */
int zk_merkle_build_columns(const zk_table *const *tables, uint32_t k, zk_merkle_tree **out);
int zk_mle_merkle_root_columns(const zk_table *const *tables, uint32_t k, uint8_t root32[32]);   /* root-only mode: scratch of 64 bytes x part */
/* HOST only: *ok = 1 when the 4 k `elements` (Montgomery limbs, in the leaf's order: column, then side) of leaf `index` hash up `path` (depth
 * digests) to root32; an element that is not reduced gives *ok = 0.  k outside 1 .. 32 or another field: ZK_E_ARG; index >= 2^depth: ZK_E_RANGE. */
int zk_merkle_verify_columns(int field, const uint8_t root32[32], size_t depth, size_t index, uint32_t k, const uint64_t *elements,
                             const uint8_t *path, int *ok);

/* ---- number-theoretic transform (extension: the reference's fft/ crate is empty; csrc/ntt.cuh) -------------------------------
 * The definition is arkworks' Radix2EvaluationDomain.  p - 1 = 2^s t with t odd, g the field's multiplicative generator (7 for
 * BLS12-381 Fr, s = 32; 5 for BN254 Fr, s = 28): w_{2^s} = g^t and w_n = w_{2^s}^(2^s / n) for n = 2^log_n <= 2^s.  The two Fq
 * fields have s = 1 (w_2 = -1): lengths 1 and 2 work there.  With the coset shift c (non-zero; NULL = 1):
 *   forward  out[k] = sum_i in[i] c^i w_n^(i k)      the coefficient table evaluated at c w_n^k   (fft / coset_fft)
 *   inverse  the exact inverse map, n^-1 and c^-i included                                         (ifft / coset_ifft)
 * Input and output are in natural order; elements stay in the stored Montgomery form, fully reduced.  Status order: ZK_E_ARG (NULL
 * argument, bad field, zero coset), ZK_E_NOT_POW2, ZK_E_RANGE (log_n > s), all before ZK_E_NO_DEVICE.  Launches go on the calling
 * thread's stream, nothing is synchronised; the twiddle tables and, above 2^10 entries, a scratch table of the same length come from the
 * calling thread's caching pool (zk_release_cached_memory). */
int zk_ntt_two_adicity(int field, uint32_t *s);                                   /* host */
int zk_ntt_root_of_unity(int field, uint32_t log_n, uint64_t *omega);             /* host; w_n in the stored form, like zk_fe_* */
int zk_ntt(zk_table *t, int inverse, const uint64_t *coset);                      /* in place */
/* upload + zk_ntt + download, like zk_host_partial_evaluate */
int zk_host_ntt(int field, const uint64_t *in, size_t n, int inverse, const uint64_t *coset, uint64_t *out);
/* the Reed-Solomon codeword of a coefficient table: its len * 2^log_blowup evaluations at c w^k (a new table).  The zero part of the
 * padded input is never read from memory. */
int zk_uni_low_degree_extend(const zk_table *coeffs, uint32_t log_blowup, const uint64_t *coset, zk_table **out);
/* the product of two coefficient tables of equal length n: a new table of 2 n coefficients (two forward transforms of size 2 n,
 * zk_prodpoly_reduce, one inverse).  Unequal lengths: ZK_E_LEN_MISMATCH. */
int zk_uni_mul(const zk_table *a, const zk_table *b, zk_table **out);

/* ---- FRI low-degree proof (extension: the reference's fri/ crate is empty; csrc/fri.cuh, csrc/zkmle_fri.hip) -------------------
 * A hash-based commitment to a coefficient table on the NTT and the Merkle tree above: no trusted setup, no MSM.  Fields: ZK_FR381
 * and ZK_BN254_FR (the two Fq fields cannot hold a domain: every shape returns ZK_E_RANGE there).
 * Input: a coefficient table of n = 2^d entries; log_blowup = b, 1 <= b <= 8; log_final = f, 0 <= f < d; nqueries = Q,
 * 1 <= Q <= 4096; the coset shift c, non-zero, NULL = 1.  L = d + b, N = 2^L, R = d - f folds, m = 2^f; w = zk_ntt_root_of_unity(L).
 * Layer l has N_l = N >> l entries on the domain {c_l w_l^k}, c_l = c^(2^l), w_l = w^(2^l).  Layer 0 is f_0[k] = f(c w^k), the table
 * zk_uni_low_degree_extend(coeffs, b, c) returns.  The fold, for k < N_l / 2 and the challenge beta_l:
 *   f_{l+1}[k] = (f_l[k] + f_l[k + N_l/2]) / 2  +  beta_l (f_l[k] - f_l[k + N_l/2]) / (2 c_l w_l^k)
 * = f_even(x^2) + beta_l f_odd(x^2) on the squared domain: f_{l+1} is the extension, with shift c_{l+1}, of a'[i] = a[2i] + beta_l a[2i+1].
 * Layers 0 .. R - 1 are each committed by the Merkle tree above of the layer's table in natural order (root_l = zk_mle_merkle_root(f_l)).
 * Layer R is not committed: it is sent as the m low coefficients h_0 .. h_{m-1} of the polynomial of degree < N_R that interpolates
 * f_R on {c_R w_R^k} (the higher ones are zero for an honest input).
 * Transcript (t = NULL: a fresh Transcript::new()), plain appends in this order:
 *   1. 48 bytes in one append: d, b, f, Q as four big-endian u32, then c as the 32-byte canonical big-endian element;
 *   2. root_0 (32 bytes);
 *   3. for l = 0 .. R - 1: beta_l = random_challenge_as_field_element(); then, if l + 1 < R, append root_{l+1};
 *   4. h_0 .. h_{m-1}, each as the 32-byte canonical big-endian element;
 *   5. for q < Q: i_q = the little-endian integer of sample_random_challenge() mod N / 2 (duplicates are answered twice).
 * The answer to i = i_q holds, for each l < R with j_l = i mod N_l / 2, the two elements f_l[j_l] (low) and f_l[j_l + N_l/2] (high) and
 * their two authentication paths of L - l digests each, in zk_merkle_open's order.
 * Flat layouts: roots R x 32 bytes; final_coeffs m elements (Montgomery, like every element of this API);
 * query_values[(q R + l) 2 + side]; query_paths per q, per l, the low path then the high path (zk_fri_proof_sizes gives the counts).
 * Status order, as for zk_ntt: ZK_E_ARG (NULL, bad field, Q or b out of range, zero coset, and once the length is known to be a
 * power of two: f >= d, a codeword no longer than its blow-up), ZK_E_NOT_POW2, ZK_E_RANGE (d + b above the field's two-adicity),
 * all before ZK_E_NO_DEVICE.  The provers have no CPU path; the verifier is host code and never opens a device.
 * Everything runs on the calling thread's stream.  Tables, trees (one block: 64 bytes x 2 N for the R trees together) and the power
 * tables come from its caching pool (zk_release_cached_memory); beta_l depends on root_l, so a proof synchronises once per layer. */
/* one fold of a codeword of len >= 2 on {coset w_len^k} by `beta`: a new table of len / 2 entries */
int zk_fri_fold(const zk_table *codeword, const uint64_t *beta, const uint64_t *coset, zk_table **out);
/* host: the counts of the flat outputs; any pointer may be NULL.  ZK_E_ARG / ZK_E_RANGE (d + b > 32) as above */
int zk_fri_proof_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, size_t *nroots, size_t *nfinal,
                       size_t *nvalues, size_t *path_bytes);
/* betas (R elements) and query_indices (Q words) are diagnostic and may be NULL */
int zk_fri_prove(const zk_table *coeffs, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset,
                 zk_transcript *t, uint8_t *roots, uint64_t *final_coeffs, uint64_t *betas, uint64_t *query_indices,
                 uint64_t *query_values, uint8_t *query_paths);
/* the same from the N evaluations a caller already holds (d = log2 len - log_blowup): zk_fri_prove is zk_uni_low_degree_extend
 * followed by this.  A codeword that is not of low degree is not an error: its proof does not verify. */
int zk_fri_prove_codeword(const zk_table *codeword, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries,
                          const uint64_t *coset, zk_transcript *t, uint8_t *roots, uint64_t *final_coeffs, uint64_t *betas,
                          uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths);
/* HOST only.  Replays the transcript; for every query and layer checks both paths (zk_merkle_verify), folds the pair with beta_l at
 * x = c_l w_l^(j_l) and compares the result with the opened element of layer l + 1 at position j_l (the low one if j_l < N_{l+1} / 2,
 * else the high one), for l = R - 1 with sum_j h_j x'^j at x' = c_R w_R^(j_l).  Anything else -- an element that is not reduced
 * included -- gives *ok = 0.  `t` ends in the prover's state whenever the status is ZK_OK. */
int zk_fri_verify(int field, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset,
                  zk_transcript *t, const uint8_t *roots, const uint64_t *final_coeffs, const uint64_t *query_values,
                  const uint8_t *query_paths, int *ok);
/* HIP-event times of the calling thread's last zk_fri_prove / zk_fri_prove_codeword: the extension (0 for a codeword), the trees
 * (root downloads included), the folds, and the inverse transform of the last layer with the query gather and its downloads */
typedef struct {
    uint32_t layers, queries;
    float ms_extend, ms_trees, ms_folds, ms_queries, ms_total;
} zk_fri_stats;
int zk_fri_last_stats(zk_fri_stats *out);

/* ---- FRI polynomial commitment: opening at a point (extension; csrc/fri_pcs.cuh, csrc/zkmle_fri_pcs.hip) ------------------------
 * What turns the low-degree proof above into a polynomial commitment: commit to a coefficient table, later claim f(z) = y, and let a
 * verifier who holds only the root check the claim.  Batched from the start: k polynomials opened at ONE point with ONE proof
 * (zk_kzg_batch_open's counterpart); k = 1 is the plain opening.  Fields and parameters are FRI's: ZK_FR381 and ZK_BN254_FR; d, b, f, Q,
 * the coset c (NULL = 1), L = d + b, N = 2^L, w = zk_ntt_root_of_unity(L).
 * Commitment to a table a of n = 2^d coefficients: root = zk_mle_merkle_root(zk_uni_low_degree_extend(a, b, c)) -- byte for byte the
 * root_0 zk_fri_prove puts out for the same input.  The prover-side zk_fri_commitment owns a device copy of the coefficients, the
 * codeword and every level of its tree (64 bytes x N), long-lived allocations of their own like zk_merkle_build's.
 * Opening of f_0 .. f_{k-1}, 1 <= k <= 64, at z.  All commitments share field, d, b and c (else ZK_E_LEN_MISMATCH).  z must be a reduced
 * element outside the evaluation domain: (z / c)^N = 1 returns ZK_E_ARG, from prover and verifier alike, before the device check.
 *   1. y_j = f_j(z).
 *   2. Transcript (t = NULL: a fresh Transcript::new()), plain appends in this order: one append of 4 bytes, k as a big-endian u32; the k
 *      roots, 32 bytes each; z as its 32-byte canonical big-endian element; y_0 .. y_{k-1} likewise.  Then
 *      gamma = random_challenge_as_field_element().
 *   3. The quotient codeword, for i < N and x_i = c w^i:   q[i] = (sum_j gamma^j (f_j[i] - y_j)) / (x_i - z).
 *      For honest y_j every f_j - y_j vanishes at z, so q is the extension of a polynomial of degree < n - 1.  FRI proves degree < n:
 *      there is ONE degree of slack, i.e. the proof shows that sum_j gamma^j (f_j - y_j) agrees on the queried positions with (x - z) times
 *      a polynomial of degree <= n - 1, a product of degree <= n where the honest numerator has degree <= n - 1.  The slack is the usual
 *      one of a DEEP quotient proved at the committed degree bound; it costs the soundness analysis one unit of degree, not a query.
 *   4. zk_fri_prove_codeword(q, b, f, Q, c, t, ..) on the SAME transcript, unchanged: it appends its header, roots and final coefficients
 *      and samples i_0 .. i_{Q-1}.
 *   5. For every query q, side s in {0, 1} and j < k: the element f_j[i_q + s N/2] and its authentication path of L digests against
 *      root_j, in zk_merkle_open's order.  Flat layouts: opened_values[(q 2 + s) k + j]; opened_paths in the same order, L x 32 bytes each.
 * Verifier (HOST only, never opens a device): replays 2, runs the FRI verifier on the same transcript, checks every path of 5 with
 * zk_merkle_verify, and checks for every (q, s) that  sum_j gamma^j (v_j - y_j) = (x - z) (FRI's layer-0 value at that position),
 * x = c w^(i_q + s N/2).  Anything else -- an element that is not reduced included -- gives *ok = 0.  `t` ends in the prover's state
 * whenever the status is ZK_OK.
 * Status order as for FRI: ZK_E_ARG (NULL, bad field, k, b or Q out of range, zero coset, d < 1, f >= d, z in the domain or not reduced),
 * ZK_E_NOT_POW2, ZK_E_LEN_MISMATCH, ZK_E_RANGE (a field without a domain, d + b above the two-adicity), all before ZK_E_NO_DEVICE.
 * Everything runs on the calling thread's stream; the quotient, the power tables and the gather buffers come from its caching pool. */
typedef struct zk_fri_commitment zk_fri_commitment;
int zk_fri_commit(const zk_table *coeffs, uint32_t log_blowup, const uint64_t *coset, zk_fri_commitment **out);
int zk_fri_commitment_free(zk_fri_commitment *cm);
int zk_fri_commitment_root(const zk_fri_commitment *cm, uint8_t root32[32]);                 /* host copy, no device work */
/* the N evaluations f(c w^i): a BORROWED table that lives as long as the commitment (do not free it) */
int zk_fri_commitment_codeword(const zk_fri_commitment *cm, const zk_table **out);
/* The same commitment with its tree over grouped leaves.  log_group = 2: root = zk_mle_merkle_root_grouped(codeword, 2), a leaf per coset
 * {f[j], f[j + N/4], f[j + N/2], f[j + 3N/4]} of the first fold by 4, 2 (N / 4) - 1 digests (16 bytes x N); coefficients and codeword are
 * zk_fri_commit's.  log_group = 0 is zk_fri_commit byte for byte; anything else is ZK_E_ARG.  Such a commitment is opened by
 * zk_fri_ml_open_points_grouped only: zk_fri_pcs_open, zk_fri_ml_open, zk_fri_ml_open_points, zk_fri_ml_open_points_arity,
 * zk_sumcheck_basic_prove_succinct and zk_gkr_sparse_prove_succinct return ZK_E_ARG for it before any device work; zk_fri_pcs_quotient and
 * the root and codeword accessors do not read the tree and work as before. */
int zk_fri_commit_grouped(const zk_table *coeffs, uint32_t log_blowup, const uint64_t *coset, uint32_t log_group, zk_fri_commitment **out);
uint32_t zk_fri_commitment_log_group(const zk_fri_commitment *cm);                            /* 0 for NULL */
/* host: zk_fri_proof_sizes' four counts plus nopened = Q 2 k elements and opened_path_bytes = Q 2 k L 32; any pointer may be NULL */
int zk_fri_pcs_sizes(uint32_t k, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, size_t *nroots, size_t *nfinal,
                     size_t *nvalues, size_t *path_bytes, size_t *nopened, size_t *opened_path_bytes);
/* y = sum_i coeffs[i] z^i of a device table of 2^d coefficients (d >= 0), on the device: the element zk_uni_evaluate gives on the host.
 * One lane per run of 8 coefficients, the powers of z from a two-level table, two launches and one 32-byte download.  At most 512
 * workgroups; the environment's ZK_FRI_PCS_EVAL_BLOCKS, read per call and clamped to 1 .. 512, lowers that cap (tests: a short table then
 * takes the later trips of the kernel's loop).  y does not depend on it. */
int zk_uni_evaluate_device(const zk_table *coeffs, const uint64_t *z, uint64_t *y);
/* step 3 on its own (as zk_fri_fold is for the fold): a new table of N entries from the k codewords, ys (k elements) and gamma.  The N
 * inversions are Montgomery batch inversions of T entries per lane, T = N / 2^16 between 1 and 16;
 * the environment's ZK_FRI_PCS_BATCH = 1, 2, 4, 8 or 16, read per call, overrides the choice (tests, measurements).  The table does not
 * depend on T. */
int zk_fri_pcs_quotient(const zk_fri_commitment *const *cms, size_t k, const uint64_t *z, const uint64_t *ys, const uint64_t *gamma,
                        zk_table **out);
/* ys_out: k elements.  roots .. query_paths: the FRI proof of the quotient, as zk_fri_prove_codeword (betas and query_indices may be
 * NULL).  opened_values: Q 2 k elements; opened_paths: Q 2 k L 32 bytes. */
int zk_fri_pcs_open(const zk_fri_commitment *const *cms, size_t k, const uint64_t *z, uint32_t log_final, uint32_t nqueries, zk_transcript *t,
                    uint64_t *ys_out, uint8_t *roots, uint64_t *final_coeffs, uint64_t *betas, uint64_t *query_indices, uint64_t *query_values,
                    uint8_t *query_paths, uint64_t *opened_values, uint8_t *opened_paths);
/* HOST only.  roots_of_f: k x 32 bytes, in the prover's order. */
int zk_fri_pcs_verify(int field, size_t k, const uint8_t *roots_of_f, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries,
                      const uint64_t *coset, const uint64_t *z, const uint64_t *ys, zk_transcript *t, const uint8_t *roots,
                      const uint64_t *final_coeffs, const uint64_t *query_values, const uint8_t *query_paths, const uint64_t *opened_values,
                      const uint8_t *opened_paths, int *ok);
/* HIP-event times of the calling thread's last zk_fri_pcs_open: the k evaluations (download included), the quotient, the FRI proof of it
 * (zk_fri_last_stats splits that one further), the gather of the opened values and paths with its downloads; ms_total is the host clock
 * over the call.  After zk_fri_pcs_quotient: ms_quotient alone.  batch = the T of the quotient's batch inversion. */
typedef struct {
    uint32_t polys, batch;
    float ms_evals, ms_quotient, ms_fri, ms_gather, ms_total;
} zk_fri_pcs_stats;
int zk_fri_pcs_last_stats(zk_fri_pcs_stats *out);

/* ---- FRI commitment opened as a multilinear polynomial (extension; csrc/fri_ml.cuh, csrc/zkmle_fri_ml.hip) -----------------------
 * The same zk_fri_commitment, read the other way: the n = 2^d entries of an EVALUATION table T are committed as the coefficient table of
 * zk_fri_commit(T, b, c), and the claim opened is y = zk_mle_evaluate(T, z) at z = (z_0 .. z_{d-1}) in zk_mle_evaluate's order (variable 0 is
 * the most significant index bit).  This is the Basefold opening: a codeword folded with  f'(x^2) = (1 - r) f_even(x^2) + r f_odd(x^2)
 * instead of f_even + beta f_odd is the extension of a'[i] = (1 - r) a[2i] + r a[2i+1], the MLE fold of the coefficient table by r in its
 * LAST variable; a sumcheck of  sum_x T[x] eq(x, z) = y  that binds the variables last to first on the same challenges ends in the very
 * table the folded codeword ends in.  No basis change, no second tree of T: one commitment opens as a univariate (above) or as a multilinear.
 * Fields and parameters are FRI's: ZK_FR381 and ZK_BN254_FR; d, b, f, Q, c (NULL = 1), L = d + b, N = 2^L, R = d - f >= 1, m = 2^f.  Any
 * reduced elements are allowed in z; nothing is refused for lying in a domain.
 * Rounds.  T_0 = T; round l < R binds variable v = d - 1 - l, the lowest index bit of T_l.  E_l = the eq table of (z_0 .. z_{v-1}) over the
 * remaining v variables; A_l = prod_{l' < l} eq1(r_l', z_{d-1-l'}), eq1(a, b) = a b + (1 - a)(1 - b).  The round polynomial
 *   g_l(X) = A_l eq1(X, z_v) (S_0 + X (S_1 - S_0)),   S_X = sum_x' E_l[x'] T_l[2x' + X],
 * is sent as the three elements g_l(0), g_l(1), g_l(2).  Then T_{l+1} = zk_mle_fold(T_l, var = last, r_l) and
 *   f_{l+1}[k] = (1 - r_l) (f_l[k] + f_l[k + N_l/2]) / 2  +  r_l (f_l[k] - f_l[k + N_l/2]) / (2 c_l w_l^k)
 * = zk_uni_low_degree_extend(T_{l+1}, b, c_{l+1}), byte for byte.
 * Transcript (t = NULL: a fresh Transcript::new()), plain appends in this order:
 *   1. FRI's 48-byte header, unchanged;
 *   2. root_0, the commitment's root;
 *   3. z_0 .. z_{d-1}, then y, each as the 32-byte canonical big-endian element;
 *   4. for l = 0 .. R - 1: g_l(0), g_l(1), g_l(2) (96 bytes); r_l = random_challenge_as_field_element(); if l + 1 < R, root_{l+1} =
 *      zk_mle_merkle_root(f_{l+1});
 *   5. the m entries of T_R, 32 bytes each: at once the final table of the sumcheck and the final coefficients of the FRI layer;
 *   6. Q indices, exactly as FRI's step 5.
 * Answers: layout and counts are FRI's (zk_fri_proof_sizes; query_values[(q R + l) 2 + side], the paths in the same order); roots[0] is the
 * commitment's root.  Layer 0's values and paths are read from the commitment's own codeword and tree: nothing of T's codeword is hashed again.
 * Verifier (HOST only, never opens a device): replays the transcript; claim = y; per round the three elements must be reduced and
 * g_l(0) + g_l(1) = claim, then claim = g_l(r_l) by quadratic interpolation; at the end A_R (the MLE of T_R at (z_0 .. z_{f-1})) = claim.  For
 * every query and layer it checks both paths, folds the pair with r_l by the formula above and compares with the next layer's opened
 * element, for l = R - 1 with sum_j T_R[j] x'^j at x' = c_R w_R^(j_l).  It is FRI's verifier with the fold mode switched, not a copy.
 * Anything else -- an element that is not reduced included, z and y among them -- gives *ok = 0.  `t` ends in the prover's state whenever
 * the status is ZK_OK.
 * Status order is FRI's: ZK_E_ARG (NULL, bad field, Q, b or f out of range, zero coset; from the prover also a z_i that is not reduced), then
 * ZK_E_NOT_POW2, then ZK_E_RANGE, all before ZK_E_NO_DEVICE.  Everything runs on the calling thread's stream.  T_l, E_l, the layers
 * f_1 .. f_{R-1} and their R - 1 trees are ONE block of the caching pool (32 bytes x (2 n + 3 N) and a little); layer R is never built, since
 * T_R comes out of the sumcheck's side.  One host synchronisation per round: r_l depends on g_l, and root_{l+1} on r_l -- the fold of the
 * codeword, its tree and the next round's pass over T_l and E_l are enqueued behind one another and waited for once.  y needs no pass of
 * its own: y = g_0(0) + g_0(1). */
/* one Lagrange-form fold of a codeword of len >= 2 on {coset w_len^k} by r (as zk_fri_fold is for the monomial form): a new table of len / 2
 * entries = zk_uni_low_degree_extend(zk_mle_fold(T, last, r), b, coset^2) when the codeword is zk_uni_low_degree_extend(T, b, coset) */
int zk_fri_ml_fold(const zk_table *codeword, const uint64_t *r, const uint64_t *coset, zk_table **out);
/* host: zk_fri_proof_sizes' four counts plus nround = 3 R elements of round polynomials; any pointer may be NULL */
int zk_fri_ml_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, size_t *nroots, size_t *nfinal, size_t *nvalues,
                    size_t *path_bytes, size_t *nround);
/* z: d elements.  y_out: one element; round_polys: 3 R; roots: R x 32 bytes; final_table: m; challenges (R) and query_indices (Q) are
 * diagnostic and may be NULL.  The commitment's tables are only read. */
int zk_fri_ml_open(const zk_fri_commitment *cm, const uint64_t *z, uint32_t log_final, uint32_t nqueries, zk_transcript *t, uint64_t *y_out,
                   uint64_t *round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *challenges, uint64_t *query_indices,
                   uint64_t *query_values, uint8_t *query_paths);
/* HOST only.  root32: the commitment's root as the verifier holds it; roots[0] must be the same bytes. */
int zk_fri_ml_verify(int field, const uint8_t *root32, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries,
                     const uint64_t *coset, const uint64_t *z, const uint64_t *y, zk_transcript *t, const uint64_t *round_polys,
                     const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values, const uint8_t *query_paths, int *ok);
/* HIP-event times of the calling thread's last zk_fri_ml_open: the sumcheck's passes (E_0, the round kernels, their downloads and the last
 * fold of T), the folds of the codeword, the trees, the query gather with its downloads; ms_total is the host clock over the call */
typedef struct {
    uint32_t rounds, queries;
    float ms_sumcheck, ms_folds, ms_trees, ms_queries, ms_total;
} zk_fri_ml_stats;
int zk_fri_ml_last_stats(zk_fri_ml_stats *out);
/* ---- FRI commitment opened at several points (extension; csrc/fri_ml.cuh fri_ml_round_w_kernel, csrc/zkmle_fri_ml.hip) -----------------
 * ONE proof that y_p = zk_mle_evaluate(T, z^p) for P points z^0 .. z^{P-1} of the same commitment: the folded layers and their trees, the
 * larger part of an opening, are built once instead of P times.  Everything is as in "FRI commitment opened as a multilinear polynomial"
 * above: fields, d, b, f, Q, c, R = d - f >= 1, m = 2^f; a round binds the LAST variable; the codeword fold is zk_fri_ml_fold.
 * Points: 1 <= P <= 8, each of d reduced elements in zk_mle_evaluate's order; equal points are allowed.
 * Transcript (t = NULL: a fresh Transcript::new()), plain appends in this order:
 *   1. FRI's 48-byte header, unchanged;
 *   2. root_0;
 *   3. P as a 4-byte big-endian u32;
 *   4. the points, point-major: z^0_0 .. z^0_{d-1}, z^1_0 ..;
 *   5. y_0 .. y_{P-1} (points and claims each as the 32-byte canonical big-endian element);
 *   6. gamma = random_challenge_as_field_element();
 *   7. (nothing is appended) claim_0 = sum_p gamma^p y_p;
 *   8. for l = 0 .. R - 1: g_l(0), g_l(1), g_l(2); r_l = random_challenge_as_field_element(); root_{l+1} if l + 1 < R;
 *   9. the m entries of T_R;
 *  10. the Q indices.  Steps 8 to 10 are exactly steps 4 to 6 of the single-point protocol.
 * Round polynomial.  W_0[x] = sum_p gamma^p eq(x, z^p) and W_{l+1} = zk_mle_fold(W_l, last, r_l), as T_{l+1} from T_l:
 *   g_l(X) = sum_x' (W_l[2x'] + X (W_l[2x'+1] - W_l[2x'])) (T_l[2x'] + X (T_l[2x'+1] - T_l[2x'])).
 * Since W_l[2x' + X'] = sum_p gamma^p A^p_l E^p_l[x'] eq1(X', z^p_v) (v = d - 1 - l, A^p_l and E^p_l the single-point protocol's A_l and
 * E_l at z^p), this is the SAME polynomial as the per-point form  sum_p gamma^p A^p_l eq1(X, z^p_v) (S^p_0 + X (S^p_1 - S^p_0)),
 * S^p_X = sum_x' E^p_l[x'] T_l[2x' + X]; at P = 1 it is the single-point protocol's g_l.  The prover computes the first form -- one pass
 * over T_l and W_l whose cost does not depend on P -- and the verifier checks the second, which needs no table.
 * Answers: layouts and counts are zk_fri_ml_sizes'; they do not depend on P.  Layer 0 is answered from the commitment's own codeword and tree.
 * Verifier (HOST only): fri_verify_core with the FriMlClaim switch extended to P points and gamma, not a copy.  claim = claim_0; per round
 * g_l(0) + g_l(1) = claim, then claim = g_l(r_l); at the end  sum_{j<m} T_R[j] W_R[j] = claim  with
 * W_R[j] = sum_p gamma^p A^p_R eq(j; z^p_0 .. z^p_{f-1}),  A^p_R = prod_l eq1(r_l, z^p_{d-1-l}); then FRI's query checks with the Lagrange fold.
 * Anything unreduced -- a point's entry, a claim, any proof element -- gives *ok = 0.  Status order, and "t ends in the prover's state
 * whenever the status is ZK_OK", are zk_fri_ml_verify's; P outside 1 .. 8 is ZK_E_ARG (from the prover also an unreduced point entry).
 * Prover: y_p by zk_mle_evaluate (P passes, before gamma exists); W_0 from P eq tables combined in one pass (P = 1: built in place); then
 * one pass per round (fri_ml_round_w_kernel) that folds T_{l-1} and W_{l-1} by r_{l-1} and accumulates g_l at the nodes 0, 1 and infinity
 * (g_l(2) = 2 g_l(1) - g_l(0) + 2 g_l(inf) on the host).  One host synchronisation per round, as in the single-point opening.  T_l, W_l,
 * the layers, their trees and the P eq tables are ONE block of the caching pool (32 bytes x (3 n + 3 N + P n) and a little; no P n for P = 1). */
/* one round pass on its own (as zk_fri_ml_fold is for the fold).  r = NULL: round 0's form, nothing is folded or allocated, g3 = g(0), g(1),
 * g(2) of (T, W), len >= 2.  r != NULL: *T_out = zk_mle_fold(T, last, r), *W_out the same of W (new tables, len / 2), g3 of the folded pair;
 * len >= 4.  ZK_E_ARG (NULL, mixed or unsupported field, too short, r not reduced), ZK_E_LEN_MISMATCH, ZK_E_NOT_POW2, then ZK_E_NO_DEVICE. */
int zk_fri_ml_round(const zk_table *T, const zk_table *W, const uint64_t *r, zk_table **T_out, zk_table **W_out, uint64_t *g3);
/* points: npoints x d elements, point-major.  ys_out: npoints elements; gamma_out (one element) is diagnostic and may be NULL; the rest as
 * zk_fri_ml_open.  zk_fri_ml_last_stats reports this call too: the y_p and W_0 passes count in ms_sumcheck. */
int zk_fri_ml_open_points(const zk_fri_commitment *cm, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries,
                          zk_transcript *t, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *round_polys, uint8_t *roots, uint64_t *final_table,
                          uint64_t *challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths);
/* HOST only. */
int zk_fri_ml_verify_points(int field, const uint8_t *root32, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries,
                            const uint64_t *coset, const uint64_t *points, uint32_t npoints, const uint64_t *ys, zk_transcript *t,
                            const uint64_t *round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                            const uint8_t *query_paths, int *ok);
/* ---- FRI commitment opened with a fold arity (extension; csrc/fri_ml.cuh fri_ml_fold4_kernel, csrc/zkmle_fri_ml.hip) -----------------------
 * The opening at several points with every SECOND folded layer committed: half as many trees over a third of the leaves, and the codeword
 * read once per two folds.  Everything is as in "FRI commitment opened at several points" above; the additions hang on log_arity = a in {1, 2}.
 * a = 1 is that protocol byte for byte: same transcript, same layouts.  a = 2 requires R = d - f >= 2 (otherwise ZK_E_ARG).
 * Layers.  The committed layers are the even l < R: R' = ceil(R / 2) roots, roots[0] the commitment's, roots[s] the root of f_{2s}.  A STEP
 * starts at an even layer l: it folds by 4 to f_{l+2} if l + 2 <= R; otherwise (R odd, l = R - 1) it is the fold by 2 to the final layer.
 * Layer R is never built, and neither is any odd layer.
 * Transcript, plain appends in this order:
 *   1. FRI's 48-byte header, unchanged;
 *   2. ONLY when a = 2: a as a 4-byte big-endian u32 (domain separation from the a = 1 protocol);
 *   3. root_0, P, the points, y_0 .. y_{P-1}, gamma, as steps 2 to 6 above;
 *   4. for l = 0 .. R - 1: g_l(0), g_l(1), g_l(2); r_l = random_challenge_as_field_element(); and, only if l + 1 is even and l + 1 < R,
 *      root_{l+1} = zk_mle_merkle_root(f_{l+1});
 *   5. the m entries of T_R;
 *   6. Q indices i_q = the sample mod N / 4 (mod N / 2 for a = 1).
 * The sumcheck is unchanged: R rounds, one challenge each, the same round polynomials.
 * Fold by 4, k < N_l / 4, with x = c_l w_l^k, i = w_l^(N_l / 4) (the primitive fourth root of unity) and
 *   fold(a, b; r, x) = (1 - r) (a + b) / 2 + r (a - b) / (2 x):
 *   u0 = fold(f_l[k], f_l[k + N_l/2]; r_l, x),  u1 = fold(f_l[k + N_l/4], f_l[k + 3 N_l/4]; r_l, i x),  f_{l+2}[k] = fold(u0, u1; r_{l+1}, x^2)
 * -- canonical, and byte for byte what two zk_fri_ml_fold calls give (u0 = f_{l+1}[k], u1 = f_{l+1}[k + N_l/4]).
 * Answers.  For query i and a fold-4 step at layer l: j = i mod N_l / 4 and the four elements f_l[j + s N_l / 4], s = 0 .. 3, with their
 * four paths of L - l digests; for a final fold-2 step j = i mod N_l / 2, two elements and two paths.  Flat layout: per query, per step in
 * order, per s; the paths in the same order.  Counts (zk_fri_ml_sizes_arity): nroots = ceil(R / 2), nvalues = Q (4 floor(R / 2) + 2 (R mod 2)),
 * path_bytes = 32 Q sum over the steps of sides (L - l); nfinal and nround are unchanged.  The proof does NOT get smaller: four paths for half
 * as many layers.
 * Verifier (HOST only, never opens a device): fri_verify_core with FriMlClaim extended by the arity, not a copy; the sumcheck's checks are
 * unchanged.  Per fold-4 step it checks four paths, computes u0, u1 and the fold by r_{l+1} and compares with the NEXT step's opened
 * element at position j -- side j div (N_{l+2} / A'), A' the next step's number of sides -- and for the last step with sum_j T_R[j] x'^j,
 * x' = c_R w_R^j.  Unreduced elements give *ok = 0.  Status order is zk_fri_ml_verify_points'; a outside {1, 2}, or a = 2 with R < 2, is
 * ZK_E_ARG.  `t` ends in the prover's state whenever the status is ZK_OK.
 * Prover.  After r_l with l even and l + 1 < R only round l + 1's pass is enqueued and waited for; after r_{l+1} the fold by 4 f_l -> f_{l+2}
 * with (r_l, r_{l+1}), the tree of f_{l+2} and round l + 2's pass behind one another, and one wait for the root and the sums: still one host
 * synchronisation per round.  The pool block is 32 bytes x (3 n + 3 C + P n) and a little, C = the entries of the committed layers
 * f_a, f_2a, .. below R together: below N for a = 1, below N / 3 for a = 2. */
/* two Lagrange-form folds of a codeword of len >= 4 on {coset w_len^k} in one pass: a new table of len / 4 entries, byte for byte
 * zk_fri_ml_fold(zk_fri_ml_fold(codeword, r0, coset), r1, coset^2).  Statuses as zk_fri_ml_fold; len < 4 is ZK_E_ARG. */
int zk_fri_ml_fold4(const zk_table *codeword, const uint64_t *r0, const uint64_t *r1, const uint64_t *coset, zk_table **out);
/* host: zk_fri_ml_sizes' five counts for the arity; log_arity outside {1, 2}, or 2 with d - log_final < 2, is ZK_E_ARG */
int zk_fri_ml_sizes_arity(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, size_t *nroots,
                          size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nround);
/* zk_fri_ml_open_points with log_arity after nqueries; the outputs are sized by zk_fri_ml_sizes_arity (challenges: R elements as before).
 * zk_fri_ml_last_stats reports this call too. */
int zk_fri_ml_open_points_arity(const zk_fri_commitment *cm, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries,
                                uint32_t log_arity, zk_transcript *t, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *round_polys, uint8_t *roots,
                                uint64_t *final_table, uint64_t *challenges, uint64_t *query_indices, uint64_t *query_values,
                                uint8_t *query_paths);
/* HOST only: zk_fri_ml_verify_points with log_arity after nqueries. */
int zk_fri_ml_verify_points_arity(int field, const uint8_t *root32, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries,
                                  uint32_t log_arity, const uint64_t *coset, const uint64_t *points, uint32_t npoints, const uint64_t *ys,
                                  zk_transcript *t, const uint64_t *round_polys, const uint8_t *roots, const uint64_t *final_table,
                                  const uint64_t *query_values, const uint8_t *query_paths, int *ok);
/* ---- FRI commitment opened with grouped leaves (extension; csrc/merkle.cuh merkle_leaf_group_kernel, csrc/zkmle_fri_ml.hip) ---------------------
 * The opening with a fold arity at a = 2 in which every tree has ONE leaf per fold coset: a layer of n entries costs 2 (n / 4) - 1 permutations
 * instead of 2 n - 1, and a query one path of log n - 2 digests per step instead of four of log n.  It is "FRI commitment opened with a fold
 * arity" at a = 2 with these differences and no others:
 *   Commitment.  zk_fri_commit_grouped(.., log_group = 2); any other commitment is ZK_E_ARG.
 *   Transcript.  Step 2 appends 8 bytes: a = 2 as a big-endian u32, then the u32 1 (domain separation from the ungrouped protocol).  The header,
 *     root_0, P, the points, the claims, gamma, the rounds, the roots' positions, T_R and the Q indices mod N / 4 are unchanged.
 *   Leaves.  Every committed layer f_l is hashed with leaves grouped by the sides of the step that starts there: root_l =
 *     zk_mle_merkle_root_grouped(f_l, 2) for a fold-4 step and (f_l, 1) for the final fold-2 step at l = R - 1 when R is odd -- a pair leaf.
 *     Layer 0 always starts a fold-4 step (R >= 2).
 *   Answers.  The values as before: per query, per step, per side.  The paths: per query and step ONE path of L - l - log_sides digests, that
 *     of leaf j = i_q mod (N_l >> log_sides), the leaf's sibling first.
 *   Counts (zk_fri_ml_sizes_grouped).  nroots, nfinal, nvalues and nround are the arity's; path_bytes = 32 Q sum over the steps of
 *     (L - l - log_sides).  d = 24, b = 2, f = 6: 144 digests a query, where a = 1 has 630 and a = 2 ungrouped 648.
 *   Verifier (HOST only).  fri_verify_core with FriMlClaim extended by a flag, not a copy: per step it hashes the 2^log_sides opened values
 *     into the leaf (zk_merkle_verify_grouped), climbs the one path and compares with the step's root; the fold and sumcheck checks are unchanged.
 *   Prover.  The pool block is 32 bytes x (3 n + C + 2 G + P n) and a little: C as before (below N / 3), G = the leaves of the committed layers
 *     below R together, below C / 4 + 1 -- where the ungrouped block has 3 C.
 * Statuses are zk_fri_ml_open_points_arity's and zk_fri_ml_verify_points_arity's at log_arity = 2.  zk_fri_ml_last_stats reports this call too. */
int zk_fri_ml_sizes_grouped(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, size_t *nroots, size_t *nfinal, size_t *nvalues,
                            size_t *path_bytes, size_t *nround);
int zk_fri_ml_open_points_grouped(const zk_fri_commitment *cm, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries,
                                  zk_transcript *t, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *round_polys, uint8_t *roots,
                                  uint64_t *final_table, uint64_t *challenges, uint64_t *query_indices, uint64_t *query_values,
                                  uint8_t *query_paths);
int zk_fri_ml_verify_points_grouped(int field, const uint8_t *root32, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries,
                                    const uint64_t *coset, const uint64_t *points, uint32_t npoints, const uint64_t *ys, zk_transcript *t,
                                    const uint64_t *round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                                    const uint8_t *query_paths, int *ok);
/* ---- FRI commitments opened together (extension; csrc/fri_ml.cuh fri_ml_fold_batch_kernel, csrc/zkmle_fri_ml.hip) -------------------------------
 * k commitments cm_0 .. cm_{k-1}, 1 <= k <= ZK_FRI_ML_BATCH_MAX, opened at the same P <= 8 points with ONE proof: Reed-Solomon encoding is
 * linear, so the codeword of T = sum_j a_j T_j is sum_j a_j f_j, and one opening of T costs one pass over the k codewords plus k layer-0 answers
 * per query; every folded layer and every tree of a later layer is built once.  It is "FRI commitment opened at several points" with its arity
 * (a = log_arity in {1, 2}) and grouped-leaves variants, changed only as follows.
 *   Inputs.  The commitments share field, d, log_blowup, coset and log_group (0 or 2); anything else is ZK_E_ARG, before any device work.
 *     log_group = 2 needs a = 2; a = 2 needs R = d - f >= 2.  The claims are y_{j,p} = zk_mle_evaluate(T_j, z^p), laid out table-major.
 *   Transcript, plain appends in this order:
 *     1. FRI's 48-byte header;
 *     2. 16 bytes: the ASCII tag "BTCH", then a, then the grouped flag (0 or 1), then k, each a big-endian u32 -- always present, at a = 1 and
 *        k = 1 too, so no transcript of an earlier protocol is one of this protocol;
 *     3. the k roots, in order;
 *     4. P as a 4-byte big-endian u32, then the points, point-major;
 *     5. the k P claims, table-major, each 32 bytes canonical big-endian;
 *     6. ONE challenge gamma.  The coefficient of y_{j,p} is gamma^(j P + p).  With alpha = gamma^P:
 *          claim_0 = sum_j alpha^j sum_p gamma^p y_{j,p},   T = sum_j alpha^j T_j,   f_0 = sum_j alpha^j f_j,   W_0 = sum_p gamma^p eq(., z^p);
 *     7. the rounds, the later layers' roots, T_R and the Q indices exactly as in the single-table protocol of the same schedule, on T and f_0.
 *   Layer 0.  The combined f_0 has no tree and is never stored.  For step 0 a query answers with the step's `sides` values per commitment:
 *     values j-major, then side; paths j-major, `sides` paths each when ungrouped or one path each when grouped, every path from commitment
 *     j's own tree.  Steps s >= 1 are laid out as in the single-table protocol.
 *   Roots.  `roots` holds the k commitment roots first, then the roots of the committed layers of steps 1 and up.
 *   Counts (zk_fri_ml_sizes_batch).  nroots = k + (the single form's nroots - 1); nvalues and path_bytes = the single form's plus (k - 1) times
 *     step 0's share (Q sides_0 values; 32 Q sides_0 L bytes ungrouped, 32 Q (L - 2) grouped); nfinal and nround unchanged.
 *   Verifier (HOST only).  fri_verify_core with FriMlClaim extended by the number of tables, not a copy.  At step 0 it checks each commitment's
 *     path or paths against root_j, forms u_s = sum_j alpha^j v_{j,s} and carries on with u_s as the step's values; the sumcheck's checks are
 *     the several-point form's with the new claim_0.  Unreduced elements give *ok = 0; the proof's first k roots must be the verifier's own.
 *     Status order is zk_fri_ml_verify_points_arity's; k outside 1 .. 16, log_group outside {0, 2} or log_group = 2 with a = 1 is ZK_E_ARG.
 *   Prover.  k P zk_mle_evaluate passes; W_0 as in the several-point form; T_0 = T by one zk_mle_linear_combination pass into n further
 *     elements of the pool block; round 0 on (T_0, W_0).  The first step's fold reads the k codewords and forms f_0's entries in registers
 *     (fri_ml_fold_batch_kernel): k N elements read, N / sides_0 written.  Step 0's answers are gathered from the k commitments by the
 *     single-table gather kernels, once per commitment.  zk_fri_ml_last_stats reports the call: the evaluations and the combination count in
 *     ms_sumcheck, the fused first fold in ms_folds. */
#define ZK_FRI_ML_BATCH_MAX 16
/* the first step's fold on its own: zk_fri_ml_fold4(sum_j coeffs[j] codewords[j], r0, r1, coset) -- r1 = NULL: zk_fri_ml_fold(.., r0, coset) --
 * byte for byte, in one pass that never stores the sum.  coeffs: k elements.  ZK_E_ARG (NULL, k outside 1 .. 16, mixed fields),
 * ZK_E_LEN_MISMATCH (unequal lengths), then zk_fri_ml_fold4's statuses (zk_fri_ml_fold's when r1 = NULL) on codewords[0]. */
int zk_fri_ml_fold_batch(const zk_table *const *codewords, uint32_t k, const uint64_t *coeffs, const uint64_t *r0, const uint64_t *r1,
                         const uint64_t *coset, zk_table **out);
/* host: the five counts of an opening of k commitments; log_group = 2 selects the grouped form (needs log_arity = 2) */
int zk_fri_ml_sizes_batch(uint32_t k, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group,
                          size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nround);
/* ys_out: k x npoints elements, table-major; the other outputs as zk_fri_ml_open_points_arity, sized by zk_fri_ml_sizes_batch with the
 * commitments' log_group.  Statuses: ZK_E_ARG (NULL, k outside 1 .. 16, commitments that differ in field, d, log_blowup, coset or log_group,
 * grouped commitments with log_arity = 1, and zk_fri_ml_open_points_arity's), all before ZK_E_NO_DEVICE. */
int zk_fri_ml_open_batch(const zk_fri_commitment *const *cms, uint32_t k, const uint64_t *points, uint32_t npoints, uint32_t log_final,
                         uint32_t nqueries, uint32_t log_arity, zk_transcript *t, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *round_polys,
                         uint8_t *roots, uint64_t *final_table, uint64_t *challenges, uint64_t *query_indices, uint64_t *query_values,
                         uint8_t *query_paths);
/* HOST only.  roots_of_f: the k commitment roots the verifier holds, 32 bytes each, in the prover's order; ys: k x npoints elements. */
int zk_fri_ml_verify_batch(int field, const uint8_t *roots_of_f, uint32_t k, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries,
                           uint32_t log_arity, uint32_t log_group, const uint64_t *coset, const uint64_t *points, uint32_t npoints, const uint64_t *ys,
                           zk_transcript *t, const uint64_t *round_polys, const uint8_t *roots, const uint64_t *final_table,
                           const uint64_t *query_values, const uint8_t *query_paths, int *ok);
/* The basic sumcheck finished by a verifier who holds 32 bytes.  Prover::prove (prover.rs:35-71) with one change, as
 * zk_sumcheck_basic_prove_committed: the first append (:38-39) is the COMMITMENT's root (zk_fri_commitment_root: the root of the codeword of
 * the table, not zk_mle_merkle_root of the table).  The rounds run on the commitment's device table, which is only read; then
 * zk_fri_ml_open runs at z = the sumcheck's d challenges on the same transcript.  claimed_sum: one element; round_polys: d x 2; challenges:
 * d elements (required: they are the point); the rest as zk_fri_ml_open.  t = NULL: a fresh Transcript::new(). */
int zk_sumcheck_basic_prove_succinct(const zk_fri_commitment *cm, uint32_t log_final, uint32_t nqueries, zk_transcript *t,
                                     uint64_t *claimed_sum, uint64_t *round_polys, uint64_t *challenges, uint64_t *y_out,
                                     uint64_t *open_round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *open_challenges,
                                     uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths);
/* HOST only: no table, no device.  The checks of Verifier::verify (verifier.rs:23-71) on the root, with the final `evaluate` (:67) replaced by
 * y and the verified opening of y at the challenges.  Statuses as zk_fri_ml_verify, all before the transcript is touched. */
int zk_sumcheck_basic_verify_succinct(int field, const uint8_t *root32, uint32_t d, uint32_t log_blowup, uint32_t log_final,
                                      uint32_t nqueries, const uint64_t *coset, zk_transcript *t, const uint64_t *claimed_sum,
                                      const uint64_t *round_polys, const uint64_t *y, const uint64_t *open_round_polys, const uint8_t *roots,
                                      const uint64_t *final_table, const uint64_t *query_values, const uint8_t *query_paths, int *ok);

/* ---- Proof-of-work grinding (extension; csrc/grind.cuh fri_grind_kernel, csrc/grind_host.h, csrc/zkmle_grind.hip) --------------------------------
 * Lets a caller trade queries for prover work: before the query indices are drawn the prover must find a nonce whose hash with the transcript
 * has g leading zero bits, 1 <= g <= ZK_FRI_GRIND_MAX_BITS.  Each bit of g costs the prover a factor of two and, under the count commonly used
 * for FRI (b = log_blowup bits per query: an assumption about the protocol's soundness, not something this library proves), buys one bit of
 * query-phase soundness: (Q, g) and (Q', g') are equal under it when b Q + g = b Q' + g'.
 *   The step grind(t, g), plain appends on the transcript:
 *     1. 8 bytes in one append: the ASCII tag "GRND", then g as a big-endian u32 -- a proof made for one g is no proof for another;
 *     2. the nonce w is the SMALLEST unsigned 64-bit integer (at or above `start`, where there is one) such that
 *        Keccak256(everything absorbed so far || w as 8 big-endian bytes) has its first g bits zero: bit i of the digest is bit 7 - i mod 8 of byte
 *        i div 8.  In transcript terms the digest is what sample_random_challenge() returns after append(w).  w = 2^64 - 1 is never a candidate;
 *     3. append(w as 8 big-endian bytes), then sample_random_challenge(): the digest of step 2, absorbed back as always.
 *   The verifier appends the tag and g, appends w, samples the challenge and rejects unless its first g bits are zero.
 *   g = 0 means no step at all: nothing is appended, no nonce exists, and every _pow function below is its counterpart byte for byte.
 *   Placement.  zk_fri_prove_pow: between item 4 (the final coefficients) and item 5 (the indices) of zk_fri_prove's transcript.
 *     zk_fri_ml_open_batch_pow: after T_R is absorbed and before the Q indices.  Nothing else of either transcript changes.
 *     zk_fri_pcs_open, the single-commitment multilinear openers and the succinct sumcheck / GKR wrappers have no grinding form.
 *   Search (GPU).  One candidate per lane per iteration on the Merkle tree's one-hash-per-lane Keccak; the sponge (25 lanes and the fill of its
 *     open block, any of 0 .. 135) travels in the kernel's argument block.  One permutation per candidate while nonce and pad fit the open block
 *     (fill <= 127), two otherwise.  Ranges of 2^log_batch candidates are launched in ascending order and a hit lowers one 64-bit word by
 *     atomicMin, so the first range with a hit yields the smallest nonce.  The search gives up with ZK_E_RANGE once 2^(g + 6) candidates hold no
 *     nonce (an honest search fails there with probability e^-64); the transcript is then as it was.
 * Statuses: ZK_E_ARG (NULL, bits outside 1 .. 32, log_batch neither 0 nor 8 .. 30; grinding_bits > 32 for the _pow functions, or > 0 with a
 * NULL pow_nonce in a prover) before everything else, ZK_E_NO_DEVICE only from the GPU search and the provers. */
#define ZK_FRI_GRIND_MAX_BITS 32
/* GPU.  Steps 1 - 3 on t; *nonce = the smallest w >= start.  log_batch = 0 selects the default (2^22 candidates a launch, more above 24 bits),
 * else 8 .. 30.  start and log_batch exist for tests and measurements: the provers pass 0 and 0. */
int zk_transcript_grind(zk_transcript *t, uint32_t bits, uint64_t start, uint32_t log_batch, uint64_t *nonce);
/* HOST, one core: the same by the transcript's own Keccak256, cloned per candidate.  At most max_tries candidates (0: 2^(bits + 6)), then
 * ZK_E_RANGE with t as it was.  About 10^6 candidates a second. */
int zk_host_transcript_grind(zk_transcript *t, uint32_t bits, uint64_t start, uint64_t max_tries, uint64_t *nonce);
/* HOST: the verifier's step.  *ok = 1 iff the challenge's first `bits` bits are zero; t ends in the prover's state either way. */
int zk_transcript_grind_check(zk_transcript *t, uint32_t bits, uint64_t nonce, int *ok);
/* the calling thread's last zk_transcript_grind (the provers' included): candidates = those up to and including the nonce (all that were
 * covered when there was none) -- the lanes of the last launch hash somewhat more; launches; ms = HIP-event time of the launches with their
 * result reads */
typedef struct {
    uint64_t candidates;
    uint32_t launches;
    float ms;
} zk_grind_stats;
int zk_transcript_grind_last_stats(zk_grind_stats *out);
/* zk_fri_prove / zk_fri_verify with the step; pow_nonce: out (may be NULL at grinding_bits = 0, and is not written then) / in */
int zk_fri_prove_pow(const zk_table *coeffs, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset,
                     zk_transcript *t, uint8_t *roots, uint64_t *final_coeffs, uint64_t *betas, uint64_t *query_indices,
                     uint64_t *query_values, uint8_t *query_paths, uint32_t grinding_bits, uint64_t *pow_nonce);
int zk_fri_verify_pow(int field, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset,
                      zk_transcript *t, const uint8_t *roots, const uint64_t *final_coeffs, const uint64_t *query_values,
                      const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce, int *ok);
/* zk_fri_ml_open_batch / zk_fri_ml_verify_batch with the step: k commitments, P points, all three schedules (k = 1, P = 1 covers the simpler
 * forms' statements, under the batch protocol's transcript) */
int zk_fri_ml_open_batch_pow(const zk_fri_commitment *const *cms, uint32_t k, const uint64_t *points, uint32_t npoints, uint32_t log_final,
                             uint32_t nqueries, uint32_t log_arity, zk_transcript *t, uint64_t *ys_out, uint64_t *gamma_out,
                             uint64_t *round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *challenges, uint64_t *query_indices,
                             uint64_t *query_values, uint8_t *query_paths, uint32_t grinding_bits, uint64_t *pow_nonce);
int zk_fri_ml_verify_batch_pow(int field, const uint8_t *roots_of_f, uint32_t k, uint32_t d, uint32_t log_blowup, uint32_t log_final,
                               uint32_t nqueries, uint32_t log_arity, uint32_t log_group, const uint64_t *coset, const uint64_t *points,
                               uint32_t npoints, const uint64_t *ys, zk_transcript *t, const uint64_t *round_polys, const uint8_t *roots,
                               const uint64_t *final_table, const uint64_t *query_values, const uint8_t *query_paths, uint32_t grinding_bits,
                               uint64_t pow_nonce, int *ok);

/* ---- FRI commitments opened together, wide: up to 32 (extension; csrc/fri_ml.cuh fri_ml_fold_batch_wide_kernel, csrc/zkmle_fri_ml.hip) ------------
 * The protocol of "FRI commitments opened together" with the proof-of-work step of "Proof-of-work grinding", byte for byte, for
 * 1 <= k <= ZK_FRI_ML_WIDE_MAX.  Nothing in that transcript or its layout depends on the cap: the "BTCH" line carries k as a u32, the roots, the
 * claims and a query's step-0 answers are k of a kind.  So for k <= ZK_FRI_ML_BATCH_MAX each function below gives exactly the bytes, the
 * statuses and the launches of its narrow counterpart (the same instantiation of fri_ml_fold_batch_kernel), and for 17 <= k <= 32 it gives
 * what that protocol defines there.  k outside 1 .. 32 is ZK_E_ARG, where the narrow functions refuse k outside 1 .. 16.  The narrow
 * functions keep their cap: a caller who relied on the refusal of k = 17 still gets it.
 *   Prover.  The first step's fold takes a second argument block of 32 pointers and 32 coefficients (1284 bytes of kernel arguments) and a
 *     second set of instantiations, launched only when k > 16; one reduction per entry still covers the 32 terms.  Everything else is the
 *     narrow driver with its host arrays sized for 32.
 *   Verifier (HOST only).  fri_verify_core with the cap as a parameter. */
#define ZK_FRI_ML_WIDE_MAX 32
/* zk_fri_ml_fold_batch for k <= 32: the arguments, the statuses and the result of the narrow hook */
int zk_fri_ml_fold_batch_wide(const zk_table *const *codewords, uint32_t k, const uint64_t *coeffs, const uint64_t *r0, const uint64_t *r1,
                              const uint64_t *coset, zk_table **out);
/* host: zk_fri_ml_sizes_batch for k <= 32 */
int zk_fri_ml_sizes_batch_wide(uint32_t k, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                               uint32_t log_group, size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nround);
/* zk_fri_ml_open_batch_pow for k <= 32, sized by zk_fri_ml_sizes_batch_wide */
int zk_fri_ml_open_batch_wide_pow(const zk_fri_commitment *const *cms, uint32_t k, const uint64_t *points, uint32_t npoints, uint32_t log_final,
                                  uint32_t nqueries, uint32_t log_arity, zk_transcript *t, uint64_t *ys_out, uint64_t *gamma_out,
                                  uint64_t *round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *challenges, uint64_t *query_indices,
                                  uint64_t *query_values, uint8_t *query_paths, uint32_t grinding_bits, uint64_t *pow_nonce);
/* HOST only: zk_fri_ml_verify_batch_pow for k <= 32 */
int zk_fri_ml_verify_batch_wide_pow(int field, const uint8_t *roots_of_f, uint32_t k, uint32_t d, uint32_t log_blowup, uint32_t log_final,
                                    uint32_t nqueries, uint32_t log_arity, uint32_t log_group, const uint64_t *coset, const uint64_t *points,
                                    uint32_t npoints, const uint64_t *ys, zk_transcript *t, const uint64_t *round_polys, const uint8_t *roots,
                                    const uint64_t *final_table, const uint64_t *query_values, const uint8_t *query_paths,
                                    uint32_t grinding_bits, uint64_t pow_nonce, int *ok);

/* ---- Column commitments opened together (extension; csrc/merkle_columns.cuh, csrc/zkmle_fri_pcs.hip, csrc/zkmle_fri_ml.hip) -----------------------
 * A commitment to a MATRIX: k tables of one field and one length n = 2^d, 1 <= k <= ZK_FRI_COLUMNS_MAX, each extended to its own codeword f_c of
 * N = 2^(d + log_blowup) entries as zk_fri_commit does, and ONE tree over the k codewords ("Merkle commitment of several columns"): leaf j < N / 4
 * holds the first fold's coset of every column.  One path then answers all k columns at a queried position.  k = 1 has
 * zk_fri_commit_grouped(.., 2)'s root.
 *   Commitment.  zk_fri_commit_columns: k clones of the tables, k codewords by the transform zk_fri_commit uses, ONE device allocation of
 *     2 (N / 4) - 1 digests, one tree, one 32-byte download.  Statuses: ZK_E_ARG for NULL, k outside 1 .. 32, log_blowup outside 1 .. 8, a 48-byte
 *     field, mixed fields, len = 1 or a zero coset; ZK_E_LEN_MISMATCH for unequal lengths; ZK_E_NOT_POW2; ZK_E_RANGE for a field without a domain
 *     or d + log_blowup beyond its two-adicity; then the device.  The accessors give the device views (not owned by the caller) a prover runs
 *     its rounds on.
 *   Opening.  m column commitments of widths w_0 .. w_{m-1}, K = sum w_i <= ZK_FRI_ML_WIDE_MAX, one field, d, log_blowup and coset, all K columns
 *     opened as multilinear polynomials at the same P <= 8 points with one proof.  The protocol is "FRI commitments opened together" at
 *     log_arity = 2 with grouped leaves (R = d - log_final >= 2), changed only as follows.
 *     Transcript.  After the 48-byte header: the ASCII tag "COLS", then 2 (the arity), m and the m widths, each a big-endian u32, one append; then
 *       the m roots; then P, the points and the K P claims in global column order (commitment, then column, then point); gamma.  The coefficient
 *       of y_{c,p} is gamma^(c P + p) over the global column index c; alpha = gamma^P, T = sum_c alpha^c T_c, f_0 = sum_c alpha^c f_c.  The rounds,
 *       the later roots, T_R, the proof-of-work step and the indices (mod N / 4) are the grouped batch opening's.
 *     Step 0 of a query.  Values: 4 K elements, column-major then side.  Paths: m paths of d + log_blowup - 2 digests in commitment order, the
 *       sibling of leaf i_q first.  Later steps are unchanged.
 *     roots.  The m commitment roots first, then the later layers'.
 *     Counts.  nroots = m + (the single grouped form's - 1); nvalues = its + 4 Q (K - 1); path_bytes = its + 32 Q (L - 2)(m - 1); nfinal and nround
 *       are unchanged.
 *   Verifier (HOST only).  fri_verify_core: at step 0 it hashes each commitment's 4 w_i values into the leaf (zk_merkle_verify_columns), climbs
 *     its one path to root_i and forms u_s = sum_c alpha^c v_{c,s}; it carries on as the grouped batch verifier.  The proof's first m roots must
 *     be the verifier's own; anything unreduced gives *ok = 0 with ZK_OK; every status is decided before the transcript moves: ZK_E_ARG for NULL,
 *     m = 0, a zero width, K > 32, P outside 1 .. 8, R < 2 and zk_fri_ml_verify_batch_wide_pow's others, ZK_E_RANGE as there.
 *   Prover.  The batch driver with its table and codeword pointers taken from the columns; the first fold is the batch opening's kernel.  Step-0
 *     values are gathered per column, step-0 paths once per commitment.  All commitments must share field, d, log_blowup and coset (ZK_E_ARG).
 *     zk_fri_ml_last_stats reports the call. */
typedef struct zk_fri_columns zk_fri_columns;
#define ZK_FRI_COLUMNS_MAX 32
int zk_fri_commit_columns(const zk_table *const *tables, uint32_t k, uint32_t log_blowup, const uint64_t *coset, zk_fri_columns **out);
int zk_fri_columns_free(zk_fri_columns *cm);
int zk_fri_columns_root(const zk_fri_columns *cm, uint8_t root32[32]);                       /* host copy */
uint32_t zk_fri_columns_count(const zk_fri_columns *cm);                                     /* k; 0 for NULL */
int zk_fri_columns_table(const zk_fri_columns *cm, uint32_t j, const zk_table **out);        /* column j's table; j >= k: ZK_E_RANGE */
int zk_fri_columns_codeword(const zk_fri_columns *cm, uint32_t j, const zk_table **out);     /* column j's codeword */
typedef struct {
    uint32_t columns;
    float ms_extend, ms_leaves, ms_nodes;   /* the k transforms, the leaf launch, the node launches (events) */
    float ms_total;                         /* host wall clock of the call */
} zk_fri_columns_stats;
int zk_fri_columns_last_stats(zk_fri_columns_stats *out);
/* host: the counts above */
int zk_fri_ml_sizes_columns(const uint32_t *widths, uint32_t m, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, size_t *nroots,
                            size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nround);
/* ys_out: K x npoints elements; roots: nroots x 32 bytes; the other outputs as zk_fri_ml_open_batch_pow's, sized by zk_fri_ml_sizes_columns */
int zk_fri_ml_open_columns_pow(const zk_fri_columns *const *cms, uint32_t m, const uint64_t *points, uint32_t npoints, uint32_t log_final,
                               uint32_t nqueries, uint32_t grinding_bits, zk_transcript *t, uint64_t *ys_out, uint64_t *gamma_out,
                               uint64_t *round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *challenges, uint64_t *query_indices,
                               uint64_t *query_values, uint8_t *query_paths, uint64_t *pow_nonce);
/* HOST only.  roots_of_f: the m commitments' roots */
int zk_fri_ml_verify_columns_pow(int field, const uint8_t *roots_of_f, const uint32_t *widths, uint32_t m, uint32_t d, uint32_t log_blowup,
                                 uint32_t log_final, uint32_t nqueries, uint32_t grinding_bits, const uint64_t *coset, const uint64_t *points,
                                 uint32_t npoints, const uint64_t *ys, zk_transcript *t, const uint64_t *round_polys, const uint8_t *roots,
                                 const uint64_t *final_table, const uint64_t *query_values, const uint8_t *query_paths, uint64_t pow_nonce, int *ok);

/* ---- FRI commitment opened against a weight table (extension; csrc/fri_ml.cuh fri_ml_round_w_kernel, csrc/zkmle_fri_ml.hip) --------------------------
 * The proof of an inner product of a committed table with ANY table: for a commitment of 2^d entries T and a device table W_0 of 2^d entries,
 *     sum_x T[x] W_0[x] = c.
 * It is "FRI commitment opened at several points" with the points taken out: that protocol's sumcheck already runs on a weight table,
 * W_0 = sum_p gamma^p eq(., z^p), and here the caller hands W_0 over.  Everything else -- fields, d, b, f, Q, the coset, the rounds binding
 * the LAST variable, the three schedules (log_arity 1; 2; 2 on a commitment with grouped leaves), the proof-of-work step -- is as there, in
 * "... with a fold arity", "... with grouped leaves" and "Proof-of-work grinding".
 * Transcript (t = NULL: a fresh Transcript::new()): the several-point protocol's with its steps 3 to 7 replaced:
 *   1. FRI's 48-byte header; at log_arity 2 the 4-byte arity line (and its second word on grouped leaves), as in those protocols;
 *   2. root_0;
 *   3. the 4 ASCII bytes "WGHT";
 *   4. c as the 32-byte canonical big-endian element: c = g_0(0) + g_0(1) comes out of round 0's pass and is appended before g_0;
 *   5. for l = 0 .. R - 1: g_l(0), g_l(1), g_l(2); r_l; the next committed layer's root where the schedule has one;
 *   6. the m = 2^f entries of T_R; the proof-of-work step if grinding_bits > 0; the Q indices.
 * THE WEIGHT TABLE IS NOT ABSORBED.  The statement is only as binding as the caller makes it: W_0, or everything it is computed from, must be
 * in the transcript before the call (a prover whose rounds produce the table passes the transcript those rounds ran on).
 * Prover: W_0 is copied into the opening's block (the caller's table is not modified) and folded there beside T; the passes are the
 * several-point form's, fri_ml_round_w_kernel.  ZK_E_ARG: a NULL (challenges and, with grinding_bits > 0, pow_nonce are required), log_arity
 * outside 1 .. 2, grouped leaves without log_arity 2, R < 2 at log_arity 2, Q or f out of range, a table of another field;
 * ZK_E_LEN_MISMATCH: a table of another length; then ZK_E_NO_DEVICE.  Sizes: zk_fri_ml_sizes_weighted = zk_fri_ml_sizes_batch at k = 1.
 * Verifier (HOST only): zk_fri_ml_verify_points_arity's arguments (and log_group, grinding_bits, pow_nonce) with the points and claims replaced
 * by c, `challenges` (R elements, as the proof carries them) and w_final (m elements): the caller's W_R, that is W_0 folded over the last
 * variable R times by those challenges.  fri_verify_core's FriMlClaim switch is extended, not copied.  It replays the rounds and sets *ok = 0
 * if any replayed r_l differs from challenges[l] -- this is what makes a w_final computed from the proof's own copy of the challenges sound,
 * and no callback crosses the C ABI -- then checks g_0(0) + g_0(1) = c, the chain claim = g_l(r_l), and
 * sum_j T_R[j] w_final[j] = g_{R-1}(r_{R-1}), then FRI's query checks unchanged.  Anything unreduced gives *ok = 0; the statuses and "t ends in
 * the prover's state whenever the status is ZK_OK" are zk_fri_ml_verify's. */
int zk_fri_ml_sizes_weighted(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group,
                             size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nround);
int zk_fri_ml_open_weighted(const zk_fri_commitment *cm, const zk_table *weights, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                            uint32_t grinding_bits, zk_transcript *t, uint64_t *c_out, uint64_t *round_polys, uint8_t *roots, uint64_t *final_table,
                            uint64_t *challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths, uint64_t *pow_nonce);
/* HOST only. */
int zk_fri_ml_verify_weighted(int field, const uint8_t *root32, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries,
                              uint32_t log_arity, uint32_t log_group, const uint64_t *coset, const uint64_t *c, const uint64_t *challenges,
                              const uint64_t *w_final, zk_transcript *t, const uint64_t *round_polys, const uint8_t *roots,
                              const uint64_t *final_table, const uint64_t *query_values, const uint8_t *query_paths, uint32_t grinding_bits,
                              uint64_t pow_nonce, int *ok);

/* ---- Zerocheck of a product of committed tables (extension; csrc/zerocheck.cuh, csrc/zerocheck_host.h, csrc/zkmle_zerocheck.hip) --------------------
 * The simplest non-linear statement over the commitment above: three commitments cmA, cmB, cmC (zk_fri_commit / zk_fri_commit_grouped; one
 * field, d, log_blowup, coset and log_group) whose tables, read as evaluations over the cube {0,1}^d, satisfy  A[x] B[x] - C[x] = 0  for all x.
 * The prover shows  sum_x eq(x, tau) (A[x] B[x] - C[x]) = 0  at a random tau by a sumcheck and opens the three tables at the point the
 * sumcheck leaves, with ONE zk_fri_ml_open_batch_pow proof.  Transcript (t = NULL: a fresh Transcript::new()), plain appends in this order:
 *   1. 8 bytes in one append: the ASCII tag "ZCML", then d as a big-endian u32; then the 32-byte roots of A, B, C, one append each;
 *   2. tau_0 .. tau_{d-1} = d successive random_challenge_as_field_element();
 *   3. (nothing is appended) E_0[x] = eq(x, tau) = prod_i (x_i ? tau_i : 1 - tau_i), variable 0 the most significant index bit, as everywhere;
 *   4. for l = 0 .. d - 1, with X_{l+1} = zk_mle_fold(X_l, last, r_l) for X = A, B, C, E (a round binds the LAST variable, as zk_fri_ml_round):
 *        g_l(X) = sum_x' E_l(x', X) (A_l(x', X) B_l(x', X) - C_l(x', X)),   Y_l(x', X) = Y_l[2x'] + X (Y_l[2x'+1] - Y_l[2x']),
 *      a cubic, sent as g_l(0), g_l(1), g_l(2), g_l(3) (each the 32-byte canonical big-endian element); r_l = random_challenge_as_field_element();
 *   5. (nothing is appended) the point z with z[d - 1 - l] = r_l: zk_mle_evaluate(X, z) is the one entry the d folds leave of X;
 *   6. the whole protocol of zk_fri_ml_open_batch_pow on the transcript as step 4 left it: k = 3 (A, B, C in that order), npoints = 1, the point
 *      z, and the caller's log_final, nqueries, log_arity and grinding_bits -- byte for byte what that function writes when handed this
 *      transcript.  Its claims are yA, yB, yC.
 * The prover does not check the relation: on a false statement it returns ZK_OK and a proof the verifier rejects.
 * Verifier (HOST only: no table, no device; it holds the three roots).  It replays steps 1, 2 and 4 and checks  g_0(0) + g_0(1) = 0,
 *   g_l(0) + g_l(1) = g_{l-1}(r_{l-1})  (the cubic through the four nodes), and  g_{d-1}(r_{d-1}) = eq(z, tau) (yA yB - yC);  then
 *   zk_fri_ml_verify_batch_pow with ys = (yA, yB, yC).  *ok is the conjunction; anything unreduced gives *ok = 0.  Every status is decided
 *   before the transcript is touched (zk_fri_ml_verify_batch_pow's, in its order); t ends in the prover's state whenever the status is ZK_OK.
 * Prover.  E_0 by the eq-table builder (one or two launches); then one pass per round (zerocheck_mul_round_kernel) that folds the four tables of
 *   the round before by its challenge -- A, B, C, E in turn, each stored before the next is loaded -- and accumulates g_l at the nodes 0, 1, 2
 *   and infinity (the X^3 coefficient sum (E1 - E0)(A1 - A0)(B1 - B0), in which C has no share); the host forms
 *   g_l(3) = 3 g_l(2) - 3 g_l(1) + g_l(0) + 6 g_l(inf).  Sixteen reads and eight writes of 32 bytes per lane where zk_sumcheck_gkr_rounds on
 *   (E, A, B), (E, -C, 1) moves 36.  Round 0 reads the commitments' own coefficient tables, which are never written; E_0 and the two ping-pong
 *   halves of the folded tables are one block of the caching pool (32 bytes x 4 n).  One host synchronisation per round.
 * Not here: the eq factor taken out of the round (a degree-2 message), several rounds per pass or a device-side transcript, a sharded prover.
 *   Another gate: "Zerocheck of a Plonk gate over committed tables" below. */
/* one round pass on its own (as zk_fri_ml_round).  r = NULL: round 0's form, nothing is folded or allocated, g4 = g(0), g(1), g(2), g(3) of
 * (A, B, C, E), len >= 2.  r != NULL: outs[0 .. 3] = zk_mle_fold(X, last, r) for X = A, B, C, E (new tables, len / 2), g4 of the folded four;
 * len >= 4.  ZK_E_ARG (NULL, mixed or unsupported field, too short, r not reduced), ZK_E_LEN_MISMATCH, ZK_E_NOT_POW2, then ZK_E_NO_DEVICE. */
int zk_zerocheck_mul_round(const zk_table *A, const zk_table *B, const zk_table *C, const zk_table *E, const uint64_t *r, zk_table **outs, uint64_t *g4);
/* host: nzc_round = 4 d elements of round polynomials, then the five counts of zk_fri_ml_sizes_batch(3, ..); any pointer may be NULL */
int zk_zerocheck_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group, size_t *nzc_round,
                       size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nround);
/* round_polys: 4 d elements; challenges: d elements (r_0 .. r_{d-1}; the point is their reverse); tau_out (d elements) is diagnostic and may be
 * NULL; ys_out: 3 elements; from gamma_out on, the outputs of zk_fri_ml_open_batch_pow for k = 3 and one point, sized by zk_zerocheck_sizes.
 * Statuses: ZK_E_ARG (NULL, commitments that differ in field, d, log_blowup, coset or log_group, and zk_fri_ml_open_batch_pow's own), all
 * before ZK_E_NO_DEVICE and before the transcript moves. */
int zk_zerocheck_mul_prove(const zk_fri_commitment *cmA, const zk_fri_commitment *cmB, const zk_fri_commitment *cmC, uint32_t log_final, uint32_t nqueries,
                           uint32_t log_arity, uint32_t grinding_bits, zk_transcript *t, uint64_t *tau_out, uint64_t *round_polys, uint64_t *challenges,
                           uint64_t *ys_out, uint64_t *gamma_out, uint64_t *open_round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *open_challenges,
                           uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths, uint64_t *pow_nonce);
/* HOST only.  roots_of_abc: the roots of A, B, C as the verifier holds them, 96 bytes; ys: yA, yB, yC. */
int zk_zerocheck_mul_verify(int field, const uint8_t *roots_of_abc, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                            uint32_t log_group, const uint64_t *coset, zk_transcript *t, const uint64_t *round_polys, const uint64_t *ys,
                            const uint64_t *open_round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                            const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce, int *ok);
/* the calling thread's last zk_zerocheck_mul_prove or zk_zerocheck_gate_prove: HIP-event times of E_0's construction and of the d rounds (their passes, downloads and
 * the host's transcript steps between them); ms_opening = zk_fri_ml_last_stats' ms_total of the opening; ms_total is the host clock over the call */
typedef struct {
    uint32_t rounds;
    float ms_eq, ms_rounds, ms_opening, ms_total;
} zk_zerocheck_stats;
int zk_zerocheck_last_stats(zk_zerocheck_stats *out);

/* ---- Zerocheck of a Plonk gate over committed tables (extension; csrc/zerocheck.cuh, csrc/zerocheck_host.h, csrc/zkmle_zerocheck.hip) ----------------
 * The product's zerocheck with selectors: EIGHT commitments of one shape (one field, d, log_blowup, coset and log_group), in this order
 * everywhere: the wires A, B, C and the selectors qM, qL, qR, qO, qC.  Their tables, read as evaluations over the cube {0,1}^d, satisfy
 *     qM[x] A[x] B[x] + qL[x] A[x] + qR[x] B[x] + qO[x] C[x] + qC[x] = 0     for all x,
 * the vanilla Plonk gate: additions, multiplications, constants and public-constant rows in one relation.  Wiring (copy constraints) is not
 * part of it: see the block after this one.  Transcript (t = NULL: a fresh Transcript::new()), plain appends in this order:
 *   1. 8 bytes in one append: the ASCII tag "ZCPG", then d as a big-endian u32; then the eight 32-byte roots in the order above, one append each;
 *   2. tau_0 .. tau_{d-1} = d successive random_challenge_as_field_element();  E_0[x] = eq(x, tau), variable 0 the most significant index bit;
 *   3. for l = 0 .. d - 1, with X_{l+1} = zk_mle_fold(X_l, last, r_l) for the nine tables X (a round binds the LAST variable) and
 *      Y_l(x', X) = Y_l[2x'] + X (Y_l[2x'+1] - Y_l[2x']):
 *        g_l(X) = sum_x' E_l (qM_l A_l B_l + qL_l A_l + qR_l B_l + qO_l C_l + qC_l)   at (x', X),
 *      a quartic, sent as g_l(0), g_l(1), g_l(2), g_l(3), g_l(4) (each the 32-byte canonical big-endian element); then
 *      r_l = random_challenge_as_field_element();
 *   4. (nothing is appended) the point z with z[d - 1 - l] = r_l;
 *   5. the whole protocol of zk_fri_ml_open_batch_pow on the transcript as step 3 left it: k = 8 in the order above, npoints = 1, the point z,
 *      and the caller's log_final, nqueries, log_arity and grinding_bits.  Its claims are y_A, y_B, y_C, y_qM, y_qL, y_qR, y_qO, y_qC.
 * The prover does not check the relation: on a false statement it returns ZK_OK and a proof the verifier rejects.
 * Verifier (HOST only: no table, no device; it holds the eight roots, 256 bytes).  It replays steps 1 to 3 and checks  g_0(0) + g_0(1) = 0,
 *   g_l(0) + g_l(1) = g_{l-1}(r_{l-1})  (the quartic through the five nodes), and
 *   g_{d-1}(r_{d-1}) = eq(z, tau) (y_qM y_A y_B + y_qL y_A + y_qR y_B + y_qO y_C + y_qC);  then zk_fri_ml_verify_batch_pow on the eight claims.
 *   *ok is the conjunction; anything unreduced gives *ok = 0.  Every status is decided before the transcript is touched
 *   (zk_fri_ml_verify_batch_pow's, in its order); t ends in the prover's state whenever the status is ZK_OK.
 * Prover.  As the product's: E_0, then one pass per round (zerocheck_gate_round_kernel) that folds the nine tables of the round before by its
 *   challenge and accumulates g_l at the nodes 0, 1, 2, 3 and infinity (the X^4 coefficient sum (E1 - E0)(qM1 - qM0)(A1 - A0)(B1 - B0): only
 *   qM A B has a share in it); the host forms g_l(4) = 4 g_l(3) - 6 g_l(2) + 4 g_l(1) - g_l(0) + 24 g_l(inf).  36 reads and 18 writes of 32 bytes
 *   and 41 products per lane.  Round 0 reads the commitments' own coefficient tables, which are never written; E_0 and the two ping-pong halves
 *   of the folded nine are one block of the caching pool (32 bytes x 7.75 n).  One host synchronisation per round.
 * Not here: copy constraints ("Wiring: a permutation check over committed tables" below, a proof of its own) and public inputs (both with this gate in
 *   ONE sumcheck: "Plonk: gate, wiring and public inputs in one sumcheck" below), any lookup argument, custom or higher-degree gates, node 1 dropped from the pass
 *   by the known claimed sum, the eq factor taken out of the round, several rounds per pass, a sharded prover. */
/* one round pass on its own.  tables: A, B, C, qM, qL, qR, qO, qC, E.  r = NULL: round 0's form, nothing is folded or allocated,
 * g5 = g(0) .. g(4) of the nine, len >= 2.  r != NULL: outs[0 .. 8] = zk_mle_fold(X, last, r) of each (new tables, len / 2), g5 of the folded
 * nine; len >= 4.  Statuses and their order as zk_zerocheck_mul_round. */
int zk_zerocheck_gate_round(const zk_table *const tables[9], const uint64_t *r, zk_table **outs, uint64_t *g5);
/* host: nzc_round = 5 d elements of round polynomials, then the five counts of zk_fri_ml_sizes_batch(8, ..); any pointer may be NULL */
int zk_zerocheck_gate_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group, size_t *nzc_round,
                            size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nround);
/* As zk_zerocheck_mul_prove with cms[0 .. 7] = A, B, C, qM, qL, qR, qO, qC: round_polys 5 d elements, ys_out 8 elements, the opening's outputs
 * for k = 8 and one point, sized by zk_zerocheck_gate_sizes.  The same statuses, all before ZK_E_NO_DEVICE and before the transcript moves. */
int zk_zerocheck_gate_prove(const zk_fri_commitment *const cms[8], uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t grinding_bits, zk_transcript *t,
                            uint64_t *tau_out, uint64_t *round_polys, uint64_t *challenges, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *open_round_polys,
                            uint8_t *roots, uint64_t *final_table, uint64_t *open_challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths,
                            uint64_t *pow_nonce);
/* HOST only.  roots_of_eight: the eight roots as the verifier holds them, 256 bytes; ys: the eight claims. */
int zk_zerocheck_gate_verify(int field, const uint8_t *roots_of_eight, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                             uint32_t log_group, const uint64_t *coset, zk_transcript *t, const uint64_t *round_polys, const uint64_t *ys,
                             const uint64_t *open_round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                             const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce, int *ok);

/* ---- Wiring: a permutation check over committed tables (extension; csrc/wiring.cuh, csrc/wiring_host.h, csrc/zkmle_wiring.hip) -----------------------
 * Plonk's copy constraints beside the gate above: SIX commitments of one shape (one field, d, log_blowup, coset and log_group), in this order
 * everywhere: the wires A, B, C (W_0, W_1, W_2) and the permutation tables SA, SB, SC (S_0, S_1, S_2).  With n = 2^d the cell (j, x) has the
 * global index id_j(x) = j n + x, and S_j[x] is the field element of the global index the circuit's permutation sigma sends (j, x) to.  The
 * statement:  W(sigma(c)) = W(c)  for all 3 n cells c: W takes one value on every cycle of sigma.  The S tables belong to the circuit, as the
 * selectors do: the verifier holds their roots and trusts that they commit to a permutation.
 * The argument is the logarithmic-derivative one with three helper commitments.  Transcript (t = NULL: a fresh Transcript::new()), plain appends:
 *   1. 8 bytes in one append: the ASCII tag "ZCPW", then d as a big-endian u32; then the six 32-byte roots in the order above, one append each;
 *   2. beta, then gamma = two successive random_challenge_as_field_element();
 *   3. for j = 0, 1, 2 the helper table
 *        H_j[x] = inv0(Did_j[x]) - inv0(Dsig_j[x]),   Did_j[x] = beta + W_j[x] + gamma id_j(x),   Dsig_j[x] = beta + W_j[x] + gamma S_j[x],
 *      inv0(0) = 0 and inv0(a) = 1 / a otherwise (for that entry alone); each H_j is committed with the shape of the six (zk_fri_commit, or
 *      zk_fri_commit_grouped by the inputs' log_group) and the three 32-byte roots are appended, one append each.  They are part of the proof;
 *   4. alpha, then mu, then tau_0 .. tau_{d-1} = 2 + d successive challenges;  E_0[x] = eq(x, tau), variable 0 the most significant index bit;
 *   5. a sumcheck with the claimed sum 0 of
 *        mu (H_0 + H_1 + H_2)(x) + E(x) sum_j alpha^j ( H_j(x) Did_j(x) Dsig_j(x) - gamma (S_j(x) - id_j(x)) ):
 *      the second part is the zerocheck that every H_j is what step 3 says (1/Did - 1/Dsig = gamma (S - id) / (Did Dsig)), the first the multiset
 *      equality sum_j sum_x H_j(x) = 0.  For l = 0 .. d - 1, with X_{l+1} = zk_mle_fold(X_l, last, r_l) for the ten tables A, B, C, SA, SB, SC, H0,
 *      H1, H2, E (a round binds the LAST variable) and the id tables folded the same way -- they are never stored: after l folds
 *      ID_{j,l}[x'] = j 2^d + c_l + 2^l x' with c_l = sum_{i<l} 2^i r_i -- the quartic g_l(X) is sent as g_l(0) .. g_l(4) (each the 32-byte
 *      canonical big-endian element); then r_l = random_challenge_as_field_element();
 *   6. (nothing is appended) the point z with z[d - 1 - l] = r_l;
 *   7. the whole protocol of zk_fri_ml_open_batch_pow on the transcript as step 5 left it: k = 9 in the order A, B, C, SA, SB, SC, H0, H1, H2,
 *      npoints = 1, the point z, and the caller's log_final, nqueries, log_arity and grinding_bits.
 * The prover does not check the statement: on a false one it returns ZK_OK and a proof the verifier rejects.
 * Verifier (HOST only; it holds the six roots, 192 bytes).  It replays steps 1 to 5 with the H roots of the proof and checks g_0(0) + g_0(1) = 0,
 *   g_l(0) + g_l(1) = g_{l-1}(r_{l-1})  (the quartic through the five nodes), and
 *   g_{d-1}(r_{d-1}) = mu (yH0 + yH1 + yH2) + eq(z, tau) sum_j alpha^j ( yH_j (beta + yW_j + gamma id_j(z)) (beta + yW_j + gamma yS_j)
 *                                                                         - gamma (yS_j - id_j(z)) ),   id_j(z) = j 2^d + sum_i 2^(d-1-i) z_i;
 *   then zk_fri_ml_verify_batch_pow on the nine claims.  *ok is the conjunction; anything unreduced gives *ok = 0.  Every status is decided
 *   before the transcript is touched (zk_fri_ml_verify_batch_pow's, in its order); t ends in the prover's state whenever the status is ZK_OK.
 * Soundness, as a count and not a proof: the multiset equality by logarithmic derivatives needs the characteristic to exceed the 6 n fractions
 *   (both scalar fields: about 2^254 against d <= 28 or 32) and fails for a false statement with probability about 6 n / p over beta (with gamma:
 *   another 3 n / p for two cells meeting in beta + w + gamma id); the zerocheck adds d / p for tau and 2 / p for alpha, the sumcheck 4 d / p,
 *   mu 1 / p, and the opening its own error.
 * Prover.  Three launches of wiring_fractions_kernel (Montgomery's trick: one Fermat inversion for the sixteen denominators of a lane), three
 *   commitments, E_0, then one pass per round (wiring_round_kernel) that folds the ten tables and accumulates the quartic's zerocheck part at the
 *   nodes 0, 1, 2, 3 and infinity and the two plain sums of H_0 + H_1 + H_2 over the even and the odd entries; the host adds mu times the line
 *   through those two and forms g_l(4) by the fourth difference.  40 reads and 20 writes of 32 bytes and 75 products per lane (round 0: 20 reads,
 *   55 products).  No committed table is written; E_0 and the two ping-pong halves of the folded ten are one block of the caching pool
 *   (32 bytes x 8.5 n).  The helper commitments are freed before the call returns.  One host synchronisation per round.
 * Not here: gate and wiring in ONE sumcheck with one opening of A, B, C and public inputs (the block after this one: "Plonk: gate, wiring and
 *   public inputs in one sumcheck"), lookup arguments, more than three wire columns, a grand-product form, the eq factor taken out of the
 *   round, several rounds per pass, a sharded prover, and any check that the S tables commit to a permutation. */
/* the helper table of one wire on its own: *H (a new table) = inv0(beta + W[x] + gamma (first + x)) - inv0(beta + W[x] + gamma S[x]); len >= 2.
 * Statuses and their order as zk_zerocheck_mul_round (beta and gamma reduced). */
int zk_wiring_fractions(const zk_table *W, const zk_table *S, uint64_t first, const uint64_t *beta, const uint64_t *gamma, zk_table **H);
/* one round pass on its own.  tables: A, B, C, SA, SB, SC, H0, H1, H2, E.  r = NULL: round 0's form, nothing is folded or allocated, len >= 2.
 * r != NULL: outs[0 .. 9] = zk_mle_fold(X, last, r) of each (new tables, len / 2), the sums over the folded ten; len >= 4.  The id tables that
 * go with the tables the sums are taken over (with r != NULL: after the fold) are ID_j[x'] = j 2^d + id_base + 2^log_step x', d = log2 of
 * that length + log_step <= 32; id_base is a field element.  g5 = g(0) .. g(4), the message as sent (mu's line included).  Statuses and their
 * order as zk_zerocheck_mul_round; the five elements and r reduced. */
int zk_wiring_round(const zk_table *const tables[10], const uint64_t *beta, const uint64_t *gamma, const uint64_t *alpha, const uint64_t *mu, const uint64_t *id_base,
                    uint32_t log_step, const uint64_t *r, zk_table **outs, uint64_t *g5);
/* host: nround = 5 d elements of round polynomials, nhroots = 3, then the five counts of zk_fri_ml_sizes_batch(9, ..); any pointer may be NULL */
int zk_wiring_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group, size_t *nround, size_t *nhroots,
                    size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nopen_round);
/* cms[0 .. 5] = A, B, C, SA, SB, SC.  h_roots: 96 bytes; round_polys: 5 d elements; challenges: d elements (r_0 .. r_{d-1}; the point is their
 * reverse); chal_out (4 + d elements: beta, gamma, alpha, mu, tau) is diagnostic and may be NULL; ys_out: 9 elements; from gamma_out on, the
 * outputs of zk_fri_ml_open_batch_pow for k = 9 and one point, sized by zk_wiring_sizes.  Statuses: ZK_E_ARG (NULL, commitments that differ
 * in field, d, log_blowup, coset or log_group, and zk_fri_ml_open_batch_pow's own), all before ZK_E_NO_DEVICE and before the transcript moves. */
int zk_wiring_prove(const zk_fri_commitment *const cms[6], uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t grinding_bits, zk_transcript *t,
                    uint8_t *h_roots, uint64_t *chal_out, uint64_t *round_polys, uint64_t *challenges, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *open_round_polys,
                    uint8_t *roots, uint64_t *final_table, uint64_t *open_challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths,
                    uint64_t *pow_nonce);
/* HOST only.  roots_of_six: the six roots as the verifier holds them, 192 bytes; h_roots: the proof's three, 96 bytes; ys: the nine claims. */
int zk_wiring_verify(int field, const uint8_t *roots_of_six, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group,
                     const uint64_t *coset, zk_transcript *t, const uint8_t *h_roots, const uint64_t *round_polys, const uint64_t *ys, const uint64_t *open_round_polys,
                     const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values, const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce,
                     int *ok);
/* the calling thread's last zk_wiring_prove: HIP-event times of the three helper tables, their three commitments, E_0's construction and the d
 * rounds; ms_opening = zk_fri_ml_last_stats' ms_total of the opening; ms_total is the host clock over the call */
typedef struct {
    uint32_t rounds;
    float ms_fractions, ms_commit, ms_eq, ms_rounds, ms_opening, ms_total;
} zk_wiring_stats;
int zk_wiring_last_stats(zk_wiring_stats *out);

/* ---- Plonk: gate, wiring and public inputs in one sumcheck (extension; csrc/plonk.cuh, csrc/plonk_host.h, csrc/zkmle_plonk.hip) --------------------
 * The two blocks above as ONE proof, with public inputs: ELEVEN commitments of one shape (one field, d, log_blowup, coset and log_group), in this
 * order everywhere: the wires A, B, C, the selectors qM, qL, qR, qO, qC and the permutation tables SA, SB, SC.  The public inputs are
 * pi_0 .. pi_{l-1}, 0 <= l <= 2^d, reduced field elements in a host array (4 u64 limbs each, stored form); PI[x] = pi_x for x < l and 0 otherwise.
 * The statement has two parts:
 *     qM[x] A[x] B[x] + qL[x] A[x] + qR[x] B[x] + qO[x] C[x] + qC[x] - PI[x] = 0     for all x
 * (a row x < l with qL = 1 and the other selectors 0 says A[x] = pi_x), and the wiring's statement W(sigma(c)) = W(c) on A, B, C, SA, SB, SC.
 * Transcript (t = NULL: a fresh Transcript::new()), plain appends:
 *   1. 12 bytes in one append: the ASCII tag "ZCPK", then d as a big-endian u32, then l as a big-endian u32;
 *   2. the eleven 32-byte roots in the order above, one append each;
 *   3. the l public values, each the 32-byte canonical big-endian element, one append each;
 *   4. beta, then gamma = two successive random_challenge_as_field_element();
 *   5. the helper tables H_0, H_1, H_2 exactly as step 3 of the wiring (wiring_fractions_kernel, inv0, id_j(x) = j 2^d + x), each committed with
 *      the shape of the eleven; the three 32-byte roots are appended, one append each.  They are part of the proof;
 *   6. alpha, then mu, then tau_0 .. tau_{d-1} = 2 + d successive challenges;  E_0[x] = eq(x, tau), variable 0 the most significant index bit;
 *   7. ONE sumcheck of
 *        mu (H_0 + H_1 + H_2)(x) + E(x) [ sum_{j<3} alpha^j ( H_j Did_j Dsig_j - gamma (S_j - id_j) )(x) + alpha^3 (qM A B + qL A + qR B + qO C + qC)(x) ]
 *      with the claimed sum  c = alpha^3 PIeval(tau),  PIeval(tau) = sum_{x<l} pi_x eq(x, tau)  (0 when l = 0): the public inputs, taken to the
 *      other side of the gate's zerocheck, are in no table and in no kernel.  d rounds of a quartic sent as g_l(0) .. g_l(4) (each the 32-byte
 *      canonical big-endian element), then r_l; each round binds the LAST variable, all fifteen tables A, B, C, qM, qL, qR, qO, qC, SA, SB, SC, H0,
 *      H1, H2, E fold by r_l, and the id tables are implicit as in the wiring: ID_{j,l}[x'] = j 2^d + c_l + 2^l x', c_l = sum_{i<l} 2^i r_i;
 *   8. (nothing is appended) the point z with z[d - 1 - l] = r_l;
 *   9. the whole protocol of zk_fri_ml_open_batch_pow on the transcript as step 7 left it: k = 14 in the order A, B, C, qM, qL, qR, qO, qC, SA, SB,
 *      SC, H0, H1, H2, npoints = 1, the point z, and the caller's log_final, nqueries, log_arity and grinding_bits.
 * The prover does not check the statement: on a false one it returns ZK_OK and a proof the verifier rejects.
 * Verifier (HOST only: no table, no device; it holds the eleven roots, 352 bytes, and the public values).  It replays steps 1 to 7 with the H
 *   roots of the proof and checks  g_0(0) + g_0(1) = c,  g_l(0) + g_l(1) = g_{l-1}(r_{l-1})  (the quartic through the five nodes), and
 *   g_{d-1}(r_{d-1}) = mu (yH0 + yH1 + yH2) + eq(z, tau) [ sum_j alpha^j ( yH_j (beta + yW_j + gamma id_j(z)) (beta + yW_j + gamma yS_j)
 *                        - gamma (yS_j - id_j(z)) ) + alpha^3 (y_qM y_A y_B + y_qL y_A + y_qR y_B + y_qO y_C + y_qC) ],   id_j(z) = j 2^d + sum_i 2^(d-1-i) z_i;
 *   then zk_fri_ml_verify_batch_pow on the fourteen claims.  *ok is the conjunction; anything unreduced -- a public value >= p among it -- gives
 *   *ok = 0 with the status ZK_OK.  Every status is decided before the transcript is touched (zk_fri_ml_verify_batch_pow's, in its order, then
 *   npublic > 2^d and public_inputs == NULL with npublic > 0: ZK_E_ARG); the replay runs on a copy and t ends in the prover's state whenever the
 *   status is ZK_OK.
 * Prover.  The wiring's three launches of wiring_fractions_kernel and three commitments, E_0, then one pass per round (plonk_round_kernel) that
 *   folds the fifteen tables and accumulates the seven sums of the wiring's pass, the gate's share scaled by the line alpha^3 E going into the
 *   same five zerocheck sums (only qM A B has a share in the X^4 coefficient); the host forms the message as the wiring's does.  60 reads and 30
 *   writes of 32 bytes per lane that reach HBM, 6 more reads of entries the lane itself touched a phase earlier, and 110 products (round 0: 30 + 6
 *   reads, 80 products).  No committed table is written; E_0 and the two ping-pong halves of the folded fifteen are one block of the caching
 *   pool (32 bytes x 12.25 n).  The helper commitments are freed before the call returns.  One host synchronisation per round.
 * Not here: lookup arguments inside this sumcheck (a proof of its own on the same transcript: "Lookup: rows of a committed table" below), more
 *   than three wire columns, custom gates, a circuit-builder API, any check that the S tables commit to a permutation, several rounds per
 *   pass, a sharded prover, pooled memory for the helper trees. */
/* one round pass on its own.  tables: A, B, C, qM, qL, qR, qO, qC, SA, SB, SC, H0, H1, H2, E.  The contract of zk_wiring_round with fifteen
 * tables: r = NULL: round 0's form, nothing is folded or allocated, len >= 2; r != NULL: outs[0 .. 14] = zk_mle_fold(X, last, r) of each (new
 * tables, len / 2), the sums over the folded fifteen, len >= 4; the id tables ID_j[x'] = j 2^d + id_base + 2^log_step x', d = log2 of the
 * summed length + log_step <= 32; g5 = g(0) .. g(4), the message as sent.  The same statuses in the same order. */
int zk_plonk_round(const zk_table *const tables[15], const uint64_t *beta, const uint64_t *gamma, const uint64_t *alpha, const uint64_t *mu, const uint64_t *id_base,
                   uint32_t log_step, const uint64_t *r, zk_table **outs, uint64_t *g5);
/* host: *out = PIeval(tau) = sum_{x < npublic} public_inputs[x] eq(x, tau), tau: d elements, variable 0 the most significant index bit; at most
 * 2 npublic + d products and no table.  ZK_E_ARG: NULL (public_inputs may be NULL with npublic = 0), d outside 1 .. 32, npublic > 2^d, a field other than the two scalar
 * fields, anything unreduced. */
int zk_plonk_public_eval(int field, const uint64_t *public_inputs, uint32_t npublic, const uint64_t *tau, uint32_t d, uint64_t *out);
/* host: nround = 5 d elements of round polynomials, nhroots = 3, then the five counts of zk_fri_ml_sizes_batch(14, ..); any pointer may be NULL */
int zk_plonk_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group, size_t *nround, size_t *nhroots,
                   size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nopen_round);
/* cms[0 .. 10] = A, B, C, qM, qL, qR, qO, qC, SA, SB, SC; public_inputs: npublic elements (NULL with npublic = 0).  h_roots: 96 bytes;
 * round_polys: 5 d elements; challenges: d elements (the point is their reverse); chal_out (4 + d elements: beta, gamma, alpha, mu, tau) is
 * diagnostic and may be NULL; ys_out: 14 elements; from gamma_out on, the outputs of zk_fri_ml_open_batch_pow for k = 14 and one point, sized
 * by zk_plonk_sizes.  ZK_E_ARG, with nothing written and the transcript as it was: what zk_wiring_prove refuses, in each of the eleven places;
 * npublic > 2^d; public_inputs == NULL with npublic > 0; an unreduced public value.  All before ZK_E_NO_DEVICE. */
int zk_plonk_prove(const zk_fri_commitment *const cms[11], const uint64_t *public_inputs, uint32_t npublic, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                   uint32_t grinding_bits, zk_transcript *t, uint8_t *h_roots, uint64_t *chal_out, uint64_t *round_polys, uint64_t *challenges, uint64_t *ys_out,
                   uint64_t *gamma_out, uint64_t *open_round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *open_challenges, uint64_t *query_indices,
                   uint64_t *query_values, uint8_t *query_paths, uint64_t *pow_nonce);
/* HOST only.  roots_of_eleven: the eleven roots as the verifier holds them, 352 bytes; public_inputs: the verifier's own npublic values;
 * h_roots: the proof's three, 96 bytes; ys: the fourteen claims. */
int zk_plonk_verify(int field, const uint8_t *roots_of_eleven, const uint64_t *public_inputs, uint32_t npublic, uint32_t d, uint32_t log_blowup, uint32_t log_final,
                    uint32_t nqueries, uint32_t log_arity, uint32_t log_group, const uint64_t *coset, zk_transcript *t, const uint8_t *h_roots, const uint64_t *round_polys,
                    const uint64_t *ys, const uint64_t *open_round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                    const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce, int *ok);
/* the calling thread's last zk_plonk_prove: the fields of zk_wiring_stats */
typedef zk_wiring_stats zk_plonk_stats;
int zk_plonk_last_stats(zk_plonk_stats *out);

/* ---- Lookup: rows of a committed table (extension; csrc/lookup.cuh, csrc/lookup_host.h, csrc/zkmle_lookup.hip) --------------------------------------
 * A lookup argument beside the blocks above, a proof of its own on the caller's transcript: SEVEN commitments of one shape (one field, d,
 * log_blowup, coset and log_group), in this order everywhere: the wires A, B, C, the lookup selector qK and the table columns T0, T1, T2.  With
 * n = 2^d the statement:  for every row x with qK[x] = 1 there is a y with (A[x], B[x], C[x]) = (T0[y], T1[y], T2[y]).  qK and the T columns belong
 * to the circuit, as the selectors and the S tables do: the verifier holds the seven roots and trusts that qK holds only 0 and 1.  A table shorter
 * than n is padded by repeating a row; a table longer than the witness is not supported.
 * The argument is the logarithmic-derivative one (logUp) with two helper commitments.  Transcript (t = NULL: a fresh Transcript::new()), plain appends:
 *   1. 8 bytes in one append: the ASCII tag "ZCLK", then d as a big-endian u32; then the seven 32-byte roots in the order above, one append each;
 *   2. the multiplicity table M: M[y] = the number of rows x with qK[x] equal to the field's one whose triple (A[x], B[x], C[x]) equals the table's
 *      row y, credited to the SMALLEST y that holds that triple; every other index of a repeated row gets 0, and a row whose triple is nowhere in
 *      the table is counted nowhere.  M is a function of the inputs (no challenge has been drawn yet).  It is committed with the shape of the
 *      seven (zk_fri_commit, or zk_fri_commit_grouped by the inputs' log_group) and its 32-byte root is appended.  It is part of the proof;
 *   3. beta, then gamma = two successive random_challenge_as_field_element();
 *   4. the ONE helper table
 *        H[x] = qK[x] inv0(Dw[x]) - M[x] inv0(Dt[x]),   Dw = beta + A + gamma B + gamma^2 C,   Dt = beta + T0 + gamma T1 + gamma^2 T2,
 *      inv0(0) = 0 and inv0(a) = 1 / a otherwise (for that entry alone); committed with the shape of the seven, its 32-byte root appended.  It is
 *      part of the proof;
 *   5. mu, then tau_0 .. tau_{d-1} = 1 + d successive challenges;  E_0[x] = eq(x, tau), variable 0 the most significant index bit;
 *   6. ONE sumcheck with the claimed sum 0 of
 *        mu H(x) + E(x) ( H(x) Dw(x) Dt(x) - qK(x) Dt(x) + M(x) Dw(x) ):
 *      the second part is the zerocheck that H is what step 4 says, the first the equality sum_x qK / Dw = sum_y M / Dt.  For l = 0 .. d - 1, with
 *      X_{l+1} = zk_mle_fold(X_l, last, r_l) for the ten tables A, B, C, qK, T0, T1, T2, M, H, E (a round binds the LAST variable), the quartic
 *      g_l(X) is sent as g_l(0) .. g_l(4) (each the 32-byte canonical big-endian element); then r_l = random_challenge_as_field_element().  There
 *      is no alpha: there is one relation;
 *   7. (nothing is appended) the point z with z[d - 1 - l] = r_l;
 *   8. the whole protocol of zk_fri_ml_open_batch_pow on the transcript as step 6 left it: k = 9 in the order A, B, C, qK, T0, T1, T2, M, H,
 *      npoints = 1, the point z, and the caller's log_final, nqueries, log_arity and grinding_bits.
 * The prover does not check the statement: on a false one it returns ZK_OK and a proof the verifier rejects; the number of rows with qK = 1 whose
 * triple is in no table row is in zk_lookup_last_stats' `misses`.
 * Verifier (HOST only; it holds the seven roots, 224 bytes).  It replays steps 1 to 6 with the proof's two roots (M, then H) and checks
 *   g_0(0) + g_0(1) = 0,  g_l(0) + g_l(1) = g_{l-1}(r_{l-1})  (the quartic through the five nodes), and
 *   g_{d-1}(r_{d-1}) = mu yH + eq(z, tau) ( yH dw dt - yqK dt + yM dw ),   dw = beta + yA + gamma yB + gamma^2 yC,  dt = beta + yT0 + gamma yT1 + gamma^2 yT2;
 *   then zk_fri_ml_verify_batch_pow on the nine claims.  *ok is the conjunction; anything unreduced gives *ok = 0.  Every status is decided
 *   before the transcript is touched (zk_fri_ml_verify_batch_pow's, in its order); the replay runs on a copy and t ends in the prover's state
 *   whenever the status is ZK_OK.
 * Soundness, as a count and not a proof: the equality of the two sums of fractions as rational functions of beta needs the characteristic to
 *   exceed the 2 n fractions (every multiplicity is at most n; both scalar fields: about 2^254 against d <= 31) and fails for a false statement
 *   with probability about 2 n / p over beta; gamma adds 2 (2 n)^2 / p in the crudest count for two distinct triples among the 2 n meeting in one
 *   combined value; the zerocheck adds d / p for tau, the sumcheck 4 d / p, mu 1 / p, and the opening its own error.
 * Prover.  The multiplicities by a hash table of 2^(d+1) 32-bit slots holding table-row indices (open addressing, linear probing; three launches:
 *   a lane per table row inserts by atomicCAS and lowers an equal row's slot by atomicMin, a lane per witness row probes and counts by atomicAdd,
 *   and the counts become field elements); every probe loop is bounded by the capacity, and one that runs out gives ZK_E_HIP with
 *   zk_last_error naming it.  Then the two denominators' columns into pool memory (lookup_denominators_kernel), lookup_fractions_kernel
 *   (Montgomery's trick: one Fermat inversion for the sixteen denominators of a lane), the two commitments, E_0, then one pass per round
 *   (lookup_round_kernel) that folds the ten tables and accumulates the quartic's zerocheck part at the nodes 0, 1, 2, 3 and infinity and the two
 *   plain sums of H over the even and the odd entries; the host forms the message as the wiring's does.  40 reads and 20 writes of 32 bytes and
 *   47 products per lane (round 0: 20 reads, 27 products).  No committed table is written; E_0 and the two ping-pong halves of the folded ten are
 *   one block of the caching pool (32 bytes x 8.5 n); the hash table, the counts and the denominators come from the pool and go back to it.  The
 *   two helper commitments are freed before the call returns.  One host synchronisation per round and one for the miss count.
 * Not here: the lookup inside zk_plonk_prove's sumcheck and its one opening, a column count other than three, several tables or a table
 *   selector, a table of another length than the witness, a sharded prover, and any check that qK is boolean. */
/* the multiplicity table on its own.  tables: A, B, C, qK, T0, T1, T2 (len >= 2, at most 2^31: the counts are 32 bits); *M (a new table) as
 * step 2 says, *misses = the number of rows with qK = 1 whose triple is in no table row.  Statuses and their order as zk_wiring_fractions. */
int zk_lookup_multiplicities(const zk_table *const tables[7], zk_table **M, uint64_t *misses);
/* TEST HOOK: the hash table as the insert pass of zk_lookup_multiplicities and of the provers leaves it (the same set-up and launch).  T: T0,
 * T1, T2 (len = n >= 2, at most 2^31); slots: 2 n words of HOST memory.  Slot s holds the index of a table row or all ones (empty); a row's home
 * is murmur3_x86_32 (seed 0x5EED) of its 96 stored bytes, T0 then T1 then T2, masked with 2 n - 1, and it sits at the first slot from there, cyclically,
 * that was empty or held an equal row when it arrived; the slot of a repeated row ends at its smallest index.  Which row sits in which slot of a
 * chain depends on the arrival order; the set of occupied slots does not.  Statuses and their order as zk_lookup_multiplicities; nothing is
 * written unless the status is ZK_OK. */
int zk_lookup_hash_slots(const zk_table *const T[3], uint32_t *slots);
/* the helper table on its own.  tables: A, B, C, qK, T0, T1, T2, M; *H (a new table) as step 4 says; len >= 2.  Statuses and their order as
 * zk_wiring_fractions (beta and gamma reduced). */
int zk_lookup_fractions(const zk_table *const tables[8], const uint64_t *beta, const uint64_t *gamma, zk_table **H);
/* one round pass on its own.  tables: A, B, C, qK, T0, T1, T2, M, H, E.  r = NULL: round 0's form, nothing is folded or allocated, len >= 2.
 * r != NULL: outs[0 .. 9] = zk_mle_fold(X, last, r) of each (new tables, len / 2), the sums over the folded ten; len >= 4.  g5 = g(0) .. g(4),
 * the message as sent (mu's line included).  Statuses and their order as zk_wiring_round; the three elements and r reduced. */
int zk_lookup_round(const zk_table *const tables[10], const uint64_t *beta, const uint64_t *gamma, const uint64_t *mu, const uint64_t *r, zk_table **outs,
                    uint64_t *g5);
/* host: nround = 5 d elements of round polynomials, nhroots = 2, then the five counts of zk_fri_ml_sizes_batch(9, ..); any pointer may be NULL */
int zk_lookup_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group, size_t *nround, size_t *nhroots,
                    size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nopen_round);
/* cms[0 .. 6] = A, B, C, qK, T0, T1, T2.  h_roots: 64 bytes (M, then H); round_polys: 5 d elements; challenges: d elements (r_0 .. r_{d-1}; the
 * point is their reverse); chal_out (3 + d elements: beta, gamma, mu, tau) is diagnostic and may be NULL; ys_out: 9 elements; from gamma_out on,
 * the outputs of zk_fri_ml_open_batch_pow for k = 9 and one point, sized by zk_lookup_sizes.  Statuses: ZK_E_ARG (NULL, d > 31, commitments that
 * differ in field, d, log_blowup, coset or log_group, and zk_fri_ml_open_batch_pow's own), all before ZK_E_NO_DEVICE and before the transcript
 * moves. */
int zk_lookup_prove(const zk_fri_commitment *const cms[7], uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t grinding_bits, zk_transcript *t,
                    uint8_t *h_roots, uint64_t *chal_out, uint64_t *round_polys, uint64_t *challenges, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *open_round_polys,
                    uint8_t *roots, uint64_t *final_table, uint64_t *open_challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths,
                    uint64_t *pow_nonce);
/* HOST only.  roots_of_seven: the seven roots as the verifier holds them, 224 bytes; h_roots: the proof's two, 64 bytes; ys: the nine claims. */
int zk_lookup_verify(int field, const uint8_t *roots_of_seven, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group,
                     const uint64_t *coset, zk_transcript *t, const uint8_t *h_roots, const uint64_t *round_polys, const uint64_t *ys, const uint64_t *open_round_polys,
                     const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values, const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce,
                     int *ok);
/* the calling thread's last zk_lookup_prove: the rows with qK = 1 whose triple is in no table row; HIP-event times of the multiplicity count,
 * the helper table (denominators and fractions), the two commitments together, E_0's construction and the d rounds; ms_opening =
 * zk_fri_ml_last_stats' ms_total of the opening; ms_total is the host clock over the call */
typedef struct {
    uint32_t rounds;
    uint64_t misses;
    float ms_multiplicities, ms_fractions, ms_commit, ms_eq, ms_rounds, ms_opening, ms_total;
} zk_lookup_stats;
int zk_lookup_last_stats(zk_lookup_stats *out);

/* ---- Plonk with lookups: gate, wiring, public inputs and lookup rows in one sumcheck (extension; csrc/plonk_lookup.cuh, csrc/plonk_lookup_host.h,
 *      csrc/zkmle_plonk_lookup.hip) ------------------------------------------------------------------------------------------------------------------
 * zk_plonk_prove and zk_lookup_prove as ONE proof: one sumcheck, one point, one opening.  FIFTEEN commitments of one shape (field, d <= 31,
 * log_blowup, coset, log_group), in this order everywhere: A, B, C, qM, qL, qR, qO, qC, SA, SB, SC, qK, T0, T1, T2, and l <= 2^d public values.
 *   Statement.  That of "Plonk: gate, wiring and public inputs in one sumcheck" on the first eleven (the gate with the public inputs on the
 *     first l rows, and the wiring), and that of "Lookup: rows of a committed table" on A, B, C, qK, T0, T1, T2 (every row with qK = 1 is a
 *     row of the table).
 *   Transcript (t = NULL: a fresh Transcript::new()), plain appends in this order:
 *     1. 12 bytes in one append: the ASCII tag "ZCPL", then d, then l, each a big-endian u32;
 *     2. the fifteen roots, one append each;
 *     3. the l public values, each the 32-byte canonical big-endian element;
 *     4. the table M exactly as step 2 of the lookup (the same three kernels on A, B, C, qK, T0, T1, T2, a repeated table row credited at
 *        its smallest index), committed with the shape of the fifteen; its root;
 *     5. beta, then gamma: ONE pair, used by the wiring and by the lookup;
 *     6. the four helper tables with that beta and gamma: H0, H1, H2 exactly as the wiring's (wiring_fractions_kernel), HL exactly as the
 *        lookup's H (lookup_denominators_kernel, lookup_fractions_kernel); each is committed; the roots in the order H0, H1, H2, HL.  The
 *        proof's h_roots are M, H0, H1, H2, HL: 160 bytes;
 *     7. alpha, mu, tau_0 .. tau_{d-1}; E = eq(., tau);
 *     8. ONE sumcheck, d rounds that bind the LAST variable, each a quartic sent at the nodes 0 .. 4 and followed by its challenge, of
 *            mu (H0 + H1 + H2)(x) + mu^2 HL(x)
 *              + E(x) [ sum_{j<3} alpha^j ( H_j Did_j Dsig_j - gamma (S_j - id_j) )(x)
 *                       + alpha^3 (qM A B + qL A + qR B + qO C + qC)(x)
 *                       + alpha^4 ( HL Dw Dt - qK Dt + M Dw )(x) ]
 *        with Did_j, Dsig_j and the implicit id tables as in the wiring, Dw = beta + A + gamma B + gamma^2 C and
 *        Dt = beta + T0 + gamma T1 + gamma^2 T2.  The claimed sum is alpha^3 PIeval(tau) (zk_plonk_public_eval);
 *     9. the point z, z[d - 1 - l] = r_l;
 *    10. the whole protocol of zk_fri_ml_open_batch_wide_pow on the transcript as step 8 left it: k = 20 in the order of the fifteen, then M, H0,
 *        H1, H2, HL, npoints = 1, the point z.
 *   Soundness, as a count and not a proof.  Both arguments' counts hold unchanged because beta and gamma are drawn after EVERY
 *     witness-dependent commitment that either argument needs before them: the wiring (7n's count) needs A, B, C, SA, SB, SC fixed, the lookup
 *     (7p's count) needs A, B, C, qK, T0, T1, T2 and M fixed; here the fifteen and M all precede the pair.  The helpers H0, H1, H2, HL depend on
 *     beta and gamma in both originals too and precede alpha, mu and tau, as there.  The three zerochecks share E and are separated by powers of
 *     alpha (alpha^0 .. alpha^2 the wires, alpha^3 the gate, alpha^4 the lookup): one more power than 7o, so the batching term of the count is
 *     4 / p where 7o has 3 / p.  The two plain sums are separated by mu and mu^2: 2 / p where each original has 1 / p.  The rounds are d
 *     quartics as in both.  Nothing here is proved; DESIGN.md 7q repeats the count.
 *   Verifier (HOST only).  It replays steps 1 to 9 on a copy of the transcript, checks g_0(0) + g_0(1) = alpha^3 PIeval(tau),
 *     g_l(0) + g_l(1) = g_{l-1}(r_{l-1}) and, on the twenty claims with eq = eq(z, tau),
 *         g_{d-1}(r_{d-1}) = [the wiring's relation] + eq alpha^3 [the gate's relation] + eq alpha^4 (yHL dw dt - yqK dt + yM dw) + mu^2 yHL,
 *     then zk_fri_ml_verify_batch_wide_pow on the twenty claims.  *ok is the conjunction; anything unreduced -- a public value >= p among it --
 *     gives *ok = 0 with the status ZK_OK.  Every status is decided before the transcript is touched (zk_fri_ml_verify_batch_wide_pow's, in
 *     its order, then d > 31 and the public inputs' shape); t ends in the prover's state whenever the status is ZK_OK.
 *   Prover.  It does not check the statement: a false one gives ZK_OK, the rows with qK = 1 that are in no table row in the stats' `misses`,
 *     and a proof the verifier rejects.  The five helper commitments are freed before it returns; no committed table is written.  The
 *     rounds are one pass each (plonk_lookup_round_kernel: plonk_round_kernel with a fifth phase) over twenty-one tables folded into ONE pool
 *     block with E_0, 32 bytes x 16.75 n.
 * Not here: a column count other than three, several tables or a table selector, a table longer than the witness, a check that qK is boolean
 * or that the S tables commit to a permutation, more than three wires, custom gates, several rounds per pass, a sharded prover. */
/* one round pass on its own, for tests and measurements: zk_plonk_round's contract with the twenty-one tables A, B, C, qM, qL, qR, qO, qC, SA,
 * SB, SC, qK, T0, T1, T2, M, H0, H1, H2, HL, E.  r = NULL: g5 = the message of round 0's form on the tables as they are; otherwise the tables
 * folded by r in their last variable come back in outs (21 new tables) and g5 is the message on the folded ones.  The id tables are
 * id_base + 2^log_step x + j 2^(log2 of the tables a message is taken over + log_step). */
int zk_plonk_lookup_round(const zk_table *const tables[21], const uint64_t *beta, const uint64_t *gamma, const uint64_t *alpha, const uint64_t *mu,
                          const uint64_t *id_base, uint32_t log_step, const uint64_t *r, zk_table **outs, uint64_t *g5);
/* host: nround = 5 d, nhroots = 5, and zk_fri_ml_sizes_batch_wide's counts for k = 20 */
int zk_plonk_lookup_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group, size_t *nround,
                          size_t *nhroots, size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nopen_round);
/* h_roots: 160 bytes (M, H0, H1, H2, HL); chal_out (may be NULL): beta, gamma, alpha, mu, tau: 4 + d elements, diagnostic; round_polys: 5 d
 * elements; challenges: d; ys_out: 20 elements; from gamma_out on, the outputs of zk_fri_ml_open_batch_wide_pow for k = 20 and one point, sized
 * by zk_plonk_lookup_sizes.  ZK_E_ARG, with nothing written and the transcript as it was: what zk_plonk_prove refuses, in each of the fifteen
 * places and for the public inputs, and d > 31; all before ZK_E_NO_DEVICE. */
int zk_plonk_lookup_prove(const zk_fri_commitment *const cms[15], const uint64_t *public_inputs, uint32_t npublic, uint32_t log_final, uint32_t nqueries,
                          uint32_t log_arity, uint32_t grinding_bits, zk_transcript *t, uint8_t *h_roots, uint64_t *chal_out, uint64_t *round_polys,
                          uint64_t *challenges, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *open_round_polys, uint8_t *roots, uint64_t *final_table,
                          uint64_t *open_challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths, uint64_t *pow_nonce);
/* HOST only.  roots_of_fifteen: 480 bytes in the order above; the rest as zk_plonk_verify with twenty claims and five helper roots */
int zk_plonk_lookup_verify(int field, const uint8_t *roots_of_fifteen, const uint64_t *public_inputs, uint32_t npublic, uint32_t d, uint32_t log_blowup,
                           uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group, const uint64_t *coset, zk_transcript *t,
                           const uint8_t *h_roots, const uint64_t *round_polys, const uint64_t *ys, const uint64_t *open_round_polys, const uint8_t *roots,
                           const uint64_t *final_table, const uint64_t *query_values, const uint8_t *query_paths, uint32_t grinding_bits,
                           uint64_t pow_nonce, int *ok);
/* the calling thread's last zk_plonk_lookup_prove: the fields of zk_lookup_stats; ms_fractions covers all four helper tables, ms_commit the
 * five commitments together */
typedef zk_lookup_stats zk_plonk_lookup_stats;
int zk_plonk_lookup_last_stats(zk_plonk_lookup_stats *out);

/* ---- Plonk with lookups on column commitments (extension; csrc/plonk_helpers.cuh, csrc/plonk_lookup_columns_host.h,
 *      csrc/zkmle_plonk_lookup_columns.hip) --------------------------------------------------------------------------------------------------------
 * The proof of the block above for a circuit that was preprocessed ONCE into one commitment: the verifier holds TWO roots, 64 bytes.  Two
 * column commitments of one shape (field, d <= 31, log_blowup, coset), both made by zk_fri_commit_columns:
 *     witness   three columns   A, B, C
 *     circuit   twelve columns  qM, qL, qR, qO, qC, SA, SB, SC, qK, T0, T1, T2
 * and l <= 2^d public values.
 *   Statement.  That of "Plonk with lookups: gate, wiring, public inputs and lookup rows in one sumcheck" on the fifteen columns.
 *   Transcript (t = NULL: a fresh Transcript::new()), plain appends in this order:
 *     1. 12 bytes in one append: the ASCII tag "ZCLC", then d, then l, each a big-endian u32.  No other protocol here starts with these four
 *        bytes, so no earlier protocol's transcript is a prefix of this one's;
 *     2. the witness root, then the circuit root, one append each;
 *     3. the l public values, each the 32-byte canonical big-endian element;
 *     4. the table M exactly as step 4 above (the lookup's three kernels), committed as a ONE-column commitment of the same shape; its root;
 *     5. beta, then gamma: ONE pair;
 *     6. the four helper tables with that pair, in the SINGLE-DENOMINATOR form, inv0(0) = 0:
 *            H_j[x] = N_j[x] inv0(Did_j[x] Dsig_j[x]),  N_j = Dsig_j - Did_j = gamma (S_j - id_j),  Did_j = beta + W_j + gamma (j n + x),
 *                                                       Dsig_j = beta + W_j + gamma S_j,                                    j = 0, 1, 2
 *            HL[x]  = (qK[x] Dt[x] - M[x] Dw[x]) inv0(Dw[x] Dt[x]),  Dw = beta + A + gamma B + gamma^2 C,  Dt = beta + T0 + gamma T1 + gamma^2 T2
 *        made together by ONE kernel (plonk_lookup_helpers_kernel) and committed as ONE four-column commitment H0, H1, H2, HL; its one root.
 *        The proof's h_roots are M's root, then the helpers': 64 bytes.
 *        Where no denominator is zero these are, as field elements, the tables of step 6 above.  Where a product of two denominators is zero
 *        the entry is 0, which differs from inv0 per denominator only when exactly ONE of the pair is zero; there the verifier's relation for
 *        that entry, H Did Dsig - N = 0 (H Dw Dt - qK Dt + M Dw = 0), cannot hold for either definition, since the product is zero and the
 *        numerator is not.  When both are zero the numerator is zero too and 0 satisfies the relation;
 *     7. alpha, mu, tau_0 .. tau_{d-1}; E = eq(., tau);
 *     8. the sumcheck of step 8 above unchanged (plonk_lookup_round_kernel and its launcher as they are, on the columns' tables); the claimed
 *        sum is alpha^3 PIeval(tau);
 *     9. the point z, z[d - 1 - l] = r_l;
 *    10. the whole protocol of zk_fri_ml_open_columns_pow on the transcript as step 8 left it: m = 4 commitments of widths 3, 12, 1, 4 in the
 *        order witness, circuit, M, helpers, npoints = 1, the point z.  The global column order is A, B, C, qM, qL, qR, qO, qC, SA, SB, SC, qK,
 *        T0, T1, T2, M, H0, H1, H2, HL: the order of the twenty claims above, so the final relation is that block's on ys as they stand.
 *   Schedule.  The columns opening's only one: fold by 4 on grouped leaves, d - log_final >= 2.
 *   Soundness, as a count and not a proof.  The count of the block above holds unchanged: beta and gamma are drawn after the witness root, the
 *     circuit root and M's root, which between them fix every table that either argument needs before the pair (A, B, C, SA, SB, SC for the
 *     wiring; A, B, C, qK, T0, T1, T2 and M for the lookup), and nothing that the pair depends on moves after it; the helpers depend on the
 *     pair and precede alpha, mu and tau as there; alpha^0 .. alpha^4 separate the five zerocheck terms (4 / p), mu and mu^2 the two plain sums
 *     (2 / p), the rounds are d quartics (4 d / p), tau adds d / p, and the opening its own error.  That a column commitment binds each of its
 *     columns is the opening's statement ("Column commitments opened together").  Nothing here is proved; DESIGN.md 7s repeats the count.
 *   Verifier (HOST only).  It replays steps 1 to 9 on a copy of the transcript, checks g_0(0) + g_0(1) = alpha^3 PIeval(tau),
 *     g_l(0) + g_l(1) = g_{l-1}(r_{l-1}) and the final relation of the block above on the twenty claims, then zk_fri_ml_verify_columns_pow with
 *     the roots witness, circuit, M, helpers and the widths 3, 12, 1, 4.  *ok is the conjunction; anything unreduced -- a public value >= p
 *     among it -- gives *ok = 0 with the status ZK_OK.  Every status is decided before the transcript is touched (grinding_bits, a NULL, the
 *     field, d > 31, zk_fri_ml_sizes_columns' own, a zero coset, ZK_E_RANGE for a field or size without the roots of unity, the public inputs'
 *     shape); t ends in the prover's state whenever the status is ZK_OK.
 *   Prover.  It does not check the statement: a false one gives ZK_OK, the rows with qK = 1 that are in no table row in the stats' `misses`,
 *     and a proof the verifier rejects.  The two helper commitments ADOPT the tables the prover has just made (nothing is cloned) and are freed
 *     before it returns; no committed table is written.  ZK_E_ARG, with nothing written and the transcript as it was and before
 *     ZK_E_NO_DEVICE: a NULL, a witness that has not three columns or a circuit that has not twelve, d > 31, two commitments of different
 *     shape, d - log_final < 2 and the rest of zk_fri_ml_open_columns_pow's own, and the public inputs' shape or an unreduced public value.
 * Not here: the same move for zk_plonk_prove, zk_wiring_prove and zk_lookup_prove, M inside the witness commitment, a batched transform for
 * the k columns, several rounds per pass, a sharded prover, and the single-denominator helpers inside the provers above (their protocols define
 * inv0 per denominator). */
/* the four helper tables on their own.  tables: A, B, C, SA, SB, SC, qK, T0, T1, T2, M (2 <= len <= 2^31); H[0 .. 3] = H0, H1, H2, HL (new
 * tables) as step 6 says.  Statuses and their order as zk_lookup_fractions (beta and gamma reduced); ZK_E_ARG also when the four handles H lie
 * inside the array `tables` (an output that aliases an input). */
int zk_plonk_lookup_helpers(const zk_table *const tables[11], const uint64_t *beta, const uint64_t *gamma, zk_table *H[4]);
/* the rows a lane of plonk_lookup_helpers_kernel takes: its tile is 256 times as many */
uint32_t zk_plonk_lookup_helpers_batch(void);
/* host: nround = 5 d, nhroots = 2, and zk_fri_ml_sizes_columns' counts for the widths 3, 12, 1, 4 (nroots: the four commitments' first);
 * d > 31: ZK_E_ARG; any pointer may be NULL */
int zk_plonk_lookup_sizes_columns(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, size_t *nround, size_t *nhroots, size_t *nroots,
                                  size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nopen_round);
/* h_roots: 64 bytes (M, then the helpers); chal_out (may be NULL): beta, gamma, alpha, mu, tau: 4 + d elements, diagnostic; round_polys: 5 d
 * elements; challenges: d; ys_out: 20 elements; from gamma_out on, the outputs of zk_fri_ml_open_columns_pow for the four commitments and one
 * point, sized by zk_plonk_lookup_sizes_columns. */
int zk_plonk_lookup_prove_columns(const zk_fri_columns *witness, const zk_fri_columns *circuit, const uint64_t *public_inputs, uint32_t npublic,
                                  uint32_t log_final, uint32_t nqueries, uint32_t grinding_bits, zk_transcript *t, uint8_t *h_roots, uint64_t *chal_out,
                                  uint64_t *round_polys, uint64_t *challenges, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *open_round_polys, uint8_t *roots,
                                  uint64_t *final_table, uint64_t *open_challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths,
                                  uint64_t *pow_nonce);
/* HOST only.  witness_root, circuit_root: 32 bytes each, as the verifier holds them; h_roots: the proof's two, 64 bytes; ys: the twenty claims */
int zk_plonk_lookup_verify_columns(int field, const uint8_t *witness_root, const uint8_t *circuit_root, const uint64_t *public_inputs, uint32_t npublic, uint32_t d,
                                   uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset, zk_transcript *t, const uint8_t *h_roots,
                                   const uint64_t *round_polys, const uint64_t *ys, const uint64_t *open_round_polys, const uint8_t *roots,
                                   const uint64_t *final_table, const uint64_t *query_values, const uint8_t *query_paths, uint32_t grinding_bits,
                                   uint64_t pow_nonce, int *ok);
/* the calling thread's last zk_plonk_lookup_prove_columns: the fields of zk_plonk_lookup_stats; ms_fractions is the ONE helper kernel,
 * ms_commit the two helper commitments together */
int zk_plonk_lookup_columns_last_stats(zk_plonk_lookup_stats *out);

/* ---- R1CS instance: sparse matrices times a table (extension; csrc/r1cs.cuh, csrc/r1cs_host.h, csrc/zkmle_r1cs.hip) ----------------------------------
 * A rank-1 constraint system (A z) o (B z) = C z over ZK_FR381 or ZK_BN254_FR: three sparse matrices of 2^s rows and 2^d columns, s >= 1,
 * d >= 2, both at most 28.  The handle is what a Spartan prover and its verifier hold of a circuit; here it carries the two sparse passes such
 * a prover runs, each behind a function of its own: the products feed its first sumcheck (zk_zerocheck_mul_round's pass on A z, B z, C z), and
 * the bound rows are the weight table of its second, which "FRI commitment opened against a weight table" runs as the opening of the witness.
 * "R1CS satisfiability" below chains them.  A handle belongs to the device of its first pass (ZK_E_ARG on another).
 * z = (w || x): the witness w in the columns below 2^(d-1) -- the most significant index bit 0, variable 0 being the most
 * significant bit as everywhere -- and the public half x above.
 *
 * zk_r1cs_create takes, for each of A, B, C, nnz[k] entries in any order: row, column and the value as a reduced element in the host layout
 * (Montgomery limbs).  Zero values and empty matrices are allowed.  ZK_E_ARG, before any device work: a field other than the two, s or d out
 * of range, a row or column out of range, an unreduced value, the same (row, column) twice in one matrix, more than 2^32 - 1 entries.  The
 * handle sorts the entries by (row, column) and builds, on the host, a CSR form of the three matrices for the products and a CSC form (a
 * counting sort) for the bound rows, with the rows and columns binned by length: up to ZK_R1CS_ROW_SPLIT entries one to a lane, above it one
 * to a workgroup (a column's length is that of the three matrices together).  This is preprocessing, once per circuit.  Creating a handle
 * needs no device; the forms are copied to the device when zk_r1cs_matvec or zk_r1cs_bind_rows first needs them, and stay there.
 *
 * zk_r1cs_digest = Keccak-256 of: the 7 ASCII bytes "R1CSMAT"; the field id, s, d as big-endian u32; then for A, B, C in turn nnz as a
 * big-endian u64 and the entries sorted by (row, column), each as row (big-endian u32), column (big-endian u32) and the value as its 32
 * canonical big-endian bytes.  It does not depend on the order the entries were given in.
 * zk_r1cs_shape: any output may be NULL; block_items = how many rows (of the 3 2^s) and columns (of the 2^d) lie above ZK_R1CS_ROW_SPLIT.
 *
 * zk_r1cs_matvec: out[0 .. 3) = new tables of 2^s entries, A z, B z, C z for the device table z of 2^d entries: one launch sequence over
 * the rows of all three matrices.  ZK_E_ARG for another field, ZK_E_LEN_MISMATCH for another length, then ZK_E_NO_DEVICE.
 * zk_r1cs_bind_rows: with E = eq(rx, .) over the 2^s rows (rx: s reduced elements, rx[0] the most significant index bit) and rho (one reduced
 * element; unreduced: ZK_E_ARG),
 *     M[y] = sum over the entries (x, y) of A, B, C of rho^k val E[x],   k = 0, 1, 2 for A, B, C,
 * one pass over the three CSC forms that writes M once.  *out = a new table of the 2^(d-1) witness columns, or with full != 0 of all 2^d.
 * Every product val * operand of both passes is accumulated as a plain integer and reduced at the latest every 68 (ZK_FR381) or 168
 * (ZK_BN254_FR) terms; all results are canonical.  The grids are capped by ZK_R1CS_BLOCKS workgroups (1 .. 65536, read at every call). */
#define ZK_R1CS_ROW_SPLIT 32
typedef struct zk_r1cs zk_r1cs;
int zk_r1cs_create(int field, uint32_t log_rows, uint32_t log_cols, const uint32_t *const rows[3], const uint32_t *const cols[3],
                   const uint64_t *const vals[3], const size_t nnz[3], zk_r1cs **out);
int zk_r1cs_free(zk_r1cs *inst);
int zk_r1cs_digest(const zk_r1cs *inst, uint8_t digest32[32]);                                  /* HOST only */
int zk_r1cs_shape(const zk_r1cs *inst, int *field, uint32_t *log_rows, uint32_t *log_cols, uint64_t nnz[3], uint64_t block_items[2]);   /* HOST only */
int zk_r1cs_matvec(zk_r1cs *inst, const zk_table *z, zk_table *out[3]);
int zk_r1cs_bind_rows(zk_r1cs *inst, const uint64_t *rx, const uint64_t *rho, int full, zk_table **out);
/* ---- R1CS satisfiability: Spartan over a FRI commitment (extension; csrc/r1cs_host.h, csrc/zkmle_r1cs.hip) ------------------------------------------
 * The proof that (A z) o (B z) = C z for z = (w || x): w the table of 2^(d-1) entries that cmW commits to (cmW->d = d - 1, else ZK_E_ARG; any
 * leaf grouping the weighted opening accepts), x = (1, pi_1 .. pi_l, 0, ..) the public half, 0 <= l < 2^(d-1).  Two sumchecks from existing
 * parts: the product zerocheck's rounds over the tables A z, B z, C z, and the opening of w against the weight table of the bound rows, which
 * IS the second sumcheck sum_y M[y] z[y].  The prover does not check the relation: on a false statement it returns ZK_OK and a proof the
 * verifier rejects.  This is the Spartan-NIZK form: the verifier is linear in the circuit (no Spark), and nothing is zero knowledge.
 * Transcript (t = NULL: a fresh one), plain appends in this order:
 *   1. 16 bytes in one append: "R1CS", then s, d, l as big-endian u32; the 32-byte digest (zk_r1cs_digest); cmW's root; pi_1 .. pi_l, each as the
 *      32-byte canonical big-endian element, one append each;
 *   2. tau_0 .. tau_{s-1} by random_challenge_as_field_element();
 *   3. (nothing is appended) z on the device, the three products (zk_r1cs_matvec's launch), E_0 = eq(., tau);
 *   4. the s rounds of step 4 of zk_zerocheck_mul_prove on (A z, B z, C z, E): a cubic at the nodes 0 .. 3 per round, then r_l; rx[s-1-l] = r_l;
 *   5. va, vb, vc = zk_mle_evaluate(A z | B z | C z, rx), appended in that order;
 *   6. rho = random_challenge_as_field_element();
 *   7. (nothing is appended) M = zk_r1cs_bind_rows(rx, rho) over the witness half;
 *   8. the whole protocol of zk_fri_ml_open_weighted on the transcript as it stands, byte for byte: cmW, the weight table M, the caller's
 *      log_final, nqueries, log_arity, grinding_bits; its claim is c.
 * Verifier (HOST only; it holds the instance, the 32-byte root and the public values): replays 1, 2, 4, 6 and checks g_0(0) + g_0(1) = 0,
 * g_l(0) + g_l(1) = g_{l-1}(r_{l-1}), g_{s-1}(r_{s-1}) = eq(rx, tau) (va vb - vc); c = va + rho vb + rho^2 vc - c_pub with
 *   c_pub = sum over the entries (x, y), y >= 2^(d-1), of rho^k val eq(rx, x) x[y - 2^(d-1)];
 * then zk_fri_ml_verify_weighted with c, the proof's opening challenges and
 *   w_final[j] = sum over the entries with y < 2^(d-1), (y >> R) = j, of rho^k val eq(rx, x) prod_{l<R} eq1(r_l, bit l of y),  R = d - 1 - f,
 * bit 0 the least significant (round l of the opening binds the last variable): two host eq tables and one walk over the entries.  *ok is the
 * conjunction; anything unreduced gives *ok = 0.  Every status is decided before the transcript moves, and t ends in the prover's state
 * whenever the status is ZK_OK.  zk_r1cs_public_terms returns c_pub and (w_final not NULL) w_final on their own; nchallenges = R.
 * Sizes: nzc_round = 4 s elements of round polynomials; the rest zk_fri_ml_sizes_weighted at d - 1.  vs: three elements; tau_out (s elements)
 * and rho_out are diagnostic and may be NULL; challenges: the s r_l. */
int zk_r1cs_sizes(uint32_t log_rows, uint32_t log_cols, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group,
                  size_t *nzc_round, size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nround);
int zk_r1cs_prove(zk_r1cs *inst, const zk_fri_commitment *cmW, const uint64_t *public_inputs, uint32_t l, uint32_t log_final, uint32_t nqueries,
                  uint32_t log_arity, uint32_t grinding_bits, zk_transcript *t, uint64_t *tau_out, uint64_t *round_polys, uint64_t *challenges,
                  uint64_t *vs_out, uint64_t *rho_out, uint64_t *c_out, uint64_t *open_round_polys, uint8_t *roots, uint64_t *final_table,
                  uint64_t *open_challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths, uint64_t *pow_nonce);
/* HOST only. */
int zk_r1cs_verify(const zk_r1cs *inst, const uint8_t *root32, const uint64_t *public_inputs, uint32_t l, uint32_t log_blowup, uint32_t log_final,
                   uint32_t nqueries, uint32_t log_arity, uint32_t log_group, const uint64_t *coset, zk_transcript *t, const uint64_t *round_polys,
                   const uint64_t *vs, const uint64_t *c, const uint64_t *open_round_polys, const uint8_t *roots, const uint64_t *final_table,
                   const uint64_t *open_challenges, const uint64_t *query_values, const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce,
                   int *ok);
/* HOST only. */
int zk_r1cs_public_terms(const zk_r1cs *inst, const uint64_t *public_inputs, uint32_t l, const uint64_t *rx, const uint64_t *rho,
                         const uint64_t *open_challenges, uint32_t nchallenges, uint64_t *c_pub, uint64_t *w_final);
/* the calling thread's last zk_r1cs_prove: the products (with z's assembly), E_0, the rounds, the row binding (with eq(rx, .)), the opening and
 * the total, in ms.  zk_r1cs_matvec sets ms_products and zk_r1cs_bind_rows ms_eq (its table eq(rx, .)) and ms_bind: device events around the
 * launches alone */
typedef struct {
    float ms_products, ms_eq, ms_rounds, ms_bind, ms_opening, ms_total;
} zk_r1cs_stats;
int zk_r1cs_last_stats(zk_r1cs_stats *out);

/* ---- univariate helpers (host; polynomials/src/univariate/dense_univariate.rs) ------------------ */
int zk_uni_evaluate(int field, const uint64_t *coeffs, size_t n, const uint64_t *x, uint64_t *out);        /* :57 */
int zk_uni_lagrange_interpolate(int field, const uint64_t *xs, const uint64_t *ys, size_t n, uint64_t *out); /* :74 */

/* ---- basic sumcheck (sumcheck_protocol/src/basic_sumcheck) ------------------------------------- */
/* Host-clock split of the last zk_sumcheck_basic_prove / zk_sumcheck_gkr_prove / zk_sumcheck_gkr_rounds call made on the
 * calling thread: `ms_absorb` = the whole-table transcript absorb (prover.rs:38-39, sequential Keccak on the host),
 * `ms_rounds` = every round (kernels + device-side transcript) up to the single synchronisation. */
typedef struct {
    uint32_t rounds;
    float ms_absorb, ms_rounds;
} zk_sumcheck_stats;
int zk_sumcheck_last_stats(zk_sumcheck_stats *out);
/* Fault injection for tests: the NEXT proof (of any thread) whose transcript steps run on the host finds its host side deaf for
 * `milliseconds` -- as if the process had been descheduled.  The kernels waiting for their challenge give up after their spin
 * budget (2-3 s), every kernel still ends, and the proving call returns ZK_E_HIP with zk_last_error naming the cause; the
 * thread's next proof works.  The reference has no analogue (its prover cannot stall: it is one thread).  Process-global, so it is
 * inert -- returns ZK_E_ARG -- unless the process runs with ZK_ENABLE_FAULT_INJECTION=1 in its environment. */
int zk_debug_stall_service_once(int milliseconds);

/* Prover::init + Prover::prove  prover.rs:22-71.  The table stays in HBM; per round one fused
 * fold + half-sums kernel; after the table absorb the transcript lives on the device (one host
 * synchronisation per proof, csrc/dev_transcript.cuh).  round_polys: nvars*2 elements
 * (SumcheckProof.round_univariate_polynomials); challenges (nvars) is diagnostic, may be NULL. */
int zk_sumcheck_basic_prove(const zk_table *table, uint64_t *claimed_sum, uint64_t *round_polys,
                            uint64_t *challenges);
/* the same on the CALLER's transcript -- `Prover { transcript, .. }` is a public field of the reference's prover (prover.rs:7-13) that prove()
 * appends to (:38-58): the transcript ends in the state the reference's ends in, whatever it had absorbed before */
int zk_sumcheck_basic_prove_on(const zk_table *table, zk_transcript *transcript, uint64_t *claimed_sum, uint64_t *round_polys,
                               uint64_t *challenges);
/* Verifier::verify  verifier.rs:23-71 (its final `evaluate` is the same GPU fold); *ok = 1 / 0 */
int zk_sumcheck_basic_verify(const zk_table *table, const uint64_t *claimed_sum,
                             const uint64_t *round_polys, size_t nrounds, int *ok);
/* Prover::prove bound to the table's COMMITMENT (extension: no reference counterpart).  Exactly one change to prover.rs:35-71: the first
 * append (:38-39) is the 32-byte Merkle root of the table (zk_mle_merkle_root, returned in root32) instead of the table's bytes.
 * Claimed sum, round messages, challenges' derivation and the output layout are those of zk_sumcheck_basic_prove_on.  The sponge is
 * sequential, so the reference's binding costs one host core 0.7 GB/s; the root is a few milliseconds of GPU work at 2^24 entries.
 * transcript = NULL: a fresh Transcript::new().  zk_sumcheck_last_stats' ms_absorb reports the root's time. */
int zk_sumcheck_basic_prove_committed(const zk_table *table, zk_transcript *transcript, uint8_t root32[32], uint64_t *claimed_sum,
                                      uint64_t *round_polys, uint64_t *challenges);
/* Verifier::verify (verifier.rs:23-71) for the committed proof: recomputes the root from the table on the GPU, *ok = 0 if root32 is given
 * (it may be NULL) and differs, replays the transcript from the root and finishes with the GPU `evaluate`. */
int zk_sumcheck_basic_verify_committed(const zk_table *table, const uint8_t *root32, const uint64_t *claimed_sum,
                                       const uint64_t *round_polys, size_t nrounds, int *ok);

/* ---- composed polynomials + GKR sumcheck ----------------------------------------------------------
 * A SumPolynomial (polynomials/src/composed/sum_polynomial.rs:7-9) of `nprod` ProductPolynomials
 * (product_polynomial.rs:6-8) with `nfac` MLEs each is passed as tables[p * nfac + f].
 * SumPolynomial::new / ProductPolynomial::new assert equal variable counts (ZK_E_NVARS). */
int zk_sumpoly_evaluate(const zk_table *const *tables, size_t nprod, size_t nfac,
                        const uint64_t *values, size_t nvalues, uint64_t *out);    /* sum_polynomial.rs:30 */
int zk_sumpoly_reduce(const zk_table *const *tables, size_t nprod, size_t nfac, zk_table *out); /* :57 add_polynomials_element_wise */
/* ProductPolynomial::multiply_polynomials_element_wise (product_polynomial.rs:58-73): out[i] = prod_f tables[f][i]; nfac >= 2
 * (the reference asserts "more than one polynomial required for mul operation") */
int zk_prodpoly_reduce(const zk_table *const *tables, size_t nfac, zk_table *out);
/* generate_round_univariate sumcheck_gkr_protocol.rs:113-143 ; out: nfac+1 evaluations at 0..nfac.
 * out == NULL (here and in zk_sumpoly_fold_round_evals' out_evals): the pass over the tables is only ENQUEUED on the current
 * stream -- no reduction of the per-workgroup partials, no read-back -- which is how bench.py times the round kernels alone. */
int zk_sumpoly_round_evals(const zk_table *const *tables, size_t nprod, size_t nfac, uint64_t *out);
/* one fused prover round on caller-managed tables: fold every table of `in` by `value` into `out`
 * (len/2 each) and return the NEXT round's nfac+1 evaluations of the folded tables (len >= 4).
 * Building block of the multi-GPU prover, where the host combines per-shard evaluations. */
int zk_sumpoly_fold_round_evals(const zk_table *const *in, zk_table *const *out, size_t nprod, size_t nfac,
                                const uint64_t *value, uint64_t *out_evals);
/* prove  sumcheck_gkr_protocol.rs:24-67.  round_coeffs: nvars*(nfac+1) coefficients, challenges: nvars.
 * The caller's tables are not modified (the reference clones, :33). */
int zk_sumcheck_gkr_prove(const zk_table *const *tables, size_t nprod, size_t nfac,
                          const uint64_t *claimed_sum, zk_transcript *t, uint64_t *round_coeffs,
                          uint64_t *challenges);
/* the rounds of `prove` without the leading claimed-sum append (:37-60), for provers that run one
 * sumcheck in several phases on one transcript (the sparse GKR prover).  final_values (may be NULL):
 * the nprod*nfac one-entry tables left after the last fold. */
int zk_sumcheck_gkr_rounds(const zk_table *const *tables, size_t nprod, size_t nfac, zk_transcript *t,
                           uint64_t *round_coeffs, uint64_t *challenges, uint64_t *final_values);
/* the same rounds where the SECOND factor of some two-factor products is a constant: tables[p * 2 + 1] == NULL means
 * "const_factors[p] at every index" (nfac must be 2, const_factors: nprod elements).  A product with a constant factor is a
 * linear term sum_i c X(i); its table is never materialised, streamed or folded, and the proof is the one the rounds above give
 * with that table filled with the constant (tests/test_gpu_sumcheck.py).  The sparse GKR prover's phases W H1 + H0 * 1 and
 * C W + A * u run through it with three tables instead of four. */
int zk_sumcheck_gkr_rounds_cf(const zk_table *const *tables, size_t nprod, size_t nfac, const uint64_t *const_factors,
                              zk_transcript *t, uint64_t *round_coeffs, uint64_t *challenges, uint64_t *final_values);
/* verify :69-105 (host only: O(rounds) field operations) */
int zk_sumcheck_gkr_verify(int field, const uint64_t *claimed_sum, const uint64_t *round_coeffs,
                           size_t nrounds, size_t ncoef, zk_transcript *t, uint64_t *challenges,
                           uint64_t *last_claimed_sum, int *ok);

/* ---- device-resident rounds as a handle: sharded (one process per GPU) sumcheck provers ------------------
 * each GPU owns the table entries i == rank (mod G); a round is local except for the sum of 2 (basic) or
 * d + 1 (GKR) evaluations over the ranks.  With this handle that sum is ONE all-reduce(SUM) of `zk_rounds_limbs_len`
 * 64-bit words in device memory (RCCL; each word holds a 32-bit limb of a lazy sum, so element-wise integer
 * addition is exact), and the transcript step runs on every rank's device (csrc/dev_transcript.cuh): no host round
 * trip per round.  Sequence: zk_rounds_evals -> all-reduce -> zk_rounds_absorb, then per round zk_rounds_fold_evals
 * -> all-reduce -> zk_rounds_absorb; when one entry per rank is left, gather the G entries on every rank,
 * zk_rounds_evals + zk_rounds_absorb on the gathered tables (no all-reduce: replicated) and zk_rounds_tail.
 * mode 0 = basic sumcheck (prover.rs:35-71; nprod = nfac = 1, messages = the two half sums, the claimed sum is
 * absorbed before round 0), mode 1 = GKR sumcheck rounds (sumcheck_gkr_protocol.rs:37-60).  `t` is read at creation
 * (everything absorbed so far) and written back by zk_rounds_collect; keep it alive and untouched in between (by default the
 * transcript step of a round runs on the calling thread's host side, on `t` itself: the kernels post the summed evaluations to a
 * pinned mailbox and wait for the challenge -- ZK_HOST_TRANSCRIPT=0 keeps the step on the device). */
typedef struct zk_rounds zk_rounds;
int zk_rounds_new(int field, int mode, size_t nprod, size_t nfac, size_t nrounds, zk_transcript *t, zk_rounds **out);
int zk_rounds_free(zk_rounds *r);
size_t zk_rounds_limbs_len(const zk_rounds *r);                     /* capacity in words: (nfac + 1) * (limbs32 + 1); mode 0: 16 * (limbs32 + 1) */
/* evaluations of the next round from the CURRENT tables (no fold) -> limbs_dev (device memory) */
int zk_rounds_evals(zk_rounds *r, const zk_table *const *tables, uint64_t *limbs_dev);
/* fold every table by the last absorbed round's challenge (device-resident) into `out`, and the next round's
 * evaluations -> limbs_dev; tables of 2 entries are only folded (limbs_dev untouched, may be NULL) */
int zk_rounds_fold_evals(zk_rounds *r, const zk_table *const *in, zk_table *const *out, uint64_t *limbs_dev);
/* transcript step of the next round on the (summed) limbs: message, absorb, challenge */
int zk_rounds_absorb(zk_rounds *r, const uint64_t *limbs_dev);
/* every remaining round in one launch on tables every rank holds in full (<= 2048 entries); the last absorbed
 * round's challenge folds first */
int zk_rounds_tail(zk_rounds *r, const zk_table *const *tables);
/* Basic sumcheck (mode 0) with the host-assisted transcript step: SEVERAL rounds per pass and per all-reduce
 * (csrc/basic_multi.cuh).  The m rounds after a pass are the basic sumcheck on the table's 2^m segment sums (folding the top
 * variable commutes with summing out the low ones), so: zk_rounds_multi_evals (2^m segment sums -> 2^m * (limbs32 + 1) words)
 * -> all-reduce -> zk_rounds_multi_absorb (m transcript steps, one exchange) -> zk_rounds_multi_fold_evals (fold the k = m
 * variables just absorbed, prover.rs:61-63 k times, and the 2^m_next segment sums of the output; m_next = 0: none) -> ...;
 * once the global table has <= 2048 entries, gather it on every rank and zk_rounds_multi_tail runs every round left (none of
 * them started) in one launch.  zk_rounds_multi_max = the largest m accepted, 0 when the handle cannot do this (mode 1, or the
 * transcript step on the device): use the one-round sequence above then.  Same messages, same bytes absorbed.
 * limbs_dev == NULL in zk_rounds_multi_evals / zk_rounds_multi_fold_evals (with m_next > 0) means ONE rank: nothing is all-reduced, the
 * pass's last workgroup runs the exchange itself and the rounds count as absorbed (no zk_rounds_multi_absorb for them). */
unsigned zk_rounds_multi_max(const zk_rounds *r);
int zk_rounds_multi_evals(zk_rounds *r, const zk_table *table, unsigned m, uint64_t *limbs_dev);
int zk_rounds_multi_absorb(zk_rounds *r, const uint64_t *limbs_dev, unsigned m);
int zk_rounds_multi_fold_evals(zk_rounds *r, const zk_table *in, zk_table *out, unsigned k, unsigned m_next, uint64_t *limbs_dev);
int zk_rounds_multi_tail(zk_rounds *r, const zk_table *table);
/* the single synchronisation: messages (nrounds x (nfac + 1) elements), challenges (nrounds), the claimed sum
 * (mode 0) and, after zk_rounds_tail, the nprod * nfac fully folded values; any pointer may be NULL */
int zk_rounds_collect(zk_rounds *r, zk_transcript *t, uint64_t *claimed_sum, uint64_t *messages, uint64_t *challenges,
                      uint64_t *final_values);

/* ---- layered circuit + GKR prover (circuit/src/arithmetic_circuit.rs, gkr/src/gkr_protocol.rs) ----
 * Gate :9-15 (op 0 = Add, 1 = Mul); a circuit is `nlayers` layers (layer 0 = output layer), its
 * gates concatenated in `gates` with per-layer counts.  The reference ties width to depth: layer i
 * reads a 2^(i+1)-entry layer (:166-178); other shapes hit its asserts (ZK_E_NVARS / ZK_E_NOT_POW2). */
typedef struct { uint64_t left, right, out, op; } zk_gate;
size_t zk_num_of_layer_variables(size_t layer_index);                               /* :166 */
size_t zk_wiring_index(size_t layer_index, size_t a, size_t b, size_t c);            /* convert_to_binary_and_to_decimal :180 */
size_t zk_circuit_eval_size(const zk_gate *gates, const size_t *gate_counts, size_t nlayers, size_t ninputs);
/* Circuit::evaluate :65-109 ; layer_sizes[nlayers+1], evals = layer 0 .. inputs concatenated */
int zk_circuit_evaluate(int field, const zk_gate *gates, const size_t *gate_counts, size_t nlayers,
                        const uint64_t *inputs, size_t ninputs, size_t *layer_sizes, uint64_t *evals);
/* add_i_and_mul_i_mle :126-163 : dense wiring predicates, built in HBM */
int zk_circuit_add_mul_mle(int field, const zk_gate *layer_gates, size_t ngates, size_t layer_index,
                           zk_table **add_i, zk_table **mul_i);
/* gkr_protocol::prove  gkr_protocol.rs:26-143.  Flattened Proof (:17-23):
 *   circuit_output[*output_len]; claimed_sum[1]; layer_claims[nlayers] (each layer's
 *   SumcheckProverProof.claimed_sum); coeffs: per layer rounds(L)*3 coefficients, rounds(L)=2(L+1);
 *   challenges: per layer rounds(L); wb_evals / wc_evals [nlayers-1].
 * A well-formed circuit (layer i writes wires 0 .. 2^i - 1, no gate twice) is proved from its gate lists (zk_gkr_sparse_*): the same transcript and
 * the same proof bytes without the 2^(3 i + 2)-entry dense predicates; the gate lists of the calling thread's last circuit stay compiled on the device.
 * ZK_GKR_DENSE_TABLES=1 (environment, read per call) keeps the reference's dense representation, which also serves every other shape. */
size_t zk_gkr_rounds(size_t layer_index);
int zk_gkr_prove(int field, const zk_gate *gates, const size_t *gate_counts, size_t nlayers,
                 const uint64_t *inputs, size_t ninputs, uint64_t *circuit_output, size_t *output_len,
                 uint64_t *claimed_sum, uint64_t *layer_claims, uint64_t *coeffs, uint64_t *challenges,
                 uint64_t *wb_evals, uint64_t *wc_evals);
/* gkr_protocol::verify :146-236 ; *ok = 1 / 0 */
int zk_gkr_verify(int field, const zk_gate *gates, const size_t *gate_counts, size_t nlayers,
                  const uint64_t *inputs, size_t ninputs, const uint64_t *circuit_output, size_t output_len,
                  const uint64_t *layer_claims, const uint64_t *coeffs, const uint64_t *wb_evals,
                  const uint64_t *wc_evals, int *ok);

/* ---- BLS12-381 G1 bases, MSM and multilinear KZG (multilinear_kzg/src) ---------------------------
 * Affine point = 12 u64: x[6] | y[6], Fq Montgomery limbs; x = y = 0 encodes infinity.  Group
 * results are affine-normalised: compare them as (x, y) (a projective triple is not unique). */
typedef struct zk_g1_bases zk_g1_bases;                 /* HBM-resident affine bases (TrustedSetup.g1_powers_of_tau, trusted_setup.rs:5-8) */
int zk_g1_bases_upload(const uint64_t *affine, size_t n, zk_g1_bases **out);
int zk_g1_bases_download(const zk_g1_bases *b, uint64_t *affine);
int zk_g1_bases_free(zk_g1_bases *b);
size_t zk_g1_bases_len(const zk_g1_bases *b);
/* synthetic benchmark bases P_i = [a + i*d] G, generated on the device */
int zk_g1_bases_synthetic(size_t n, const uint64_t *a_fr, const uint64_t *d_fr, zk_g1_bases **out);
int zk_g1_generator(uint64_t *out12);
int zk_g1_is_on_curve(const uint64_t *p12);
/* host-side group helpers (control path: combining per-GPU partial results, a handful of points) */
int zk_g1_add(const uint64_t *p12, const uint64_t *q12, uint64_t *out12);
int zk_g1_mul_fr(const uint64_t *p12, const uint64_t *scalar_fr, uint64_t *out12);

typedef struct {
    int window_bits, windows;
    uint64_t terms, entries, segments;
    float ms_digits, ms_sort, ms_buckets, ms_reduce, ms_total;    /* HIP-event times of the phases */
} zk_msm_stats;
/* sum_i [s_i] B_i by Pippenger (window_bits = 0: chosen from n; 2 .. 24).  scalars: Fr table of n terms
 * (n = bases length, any n >= 1).  This is the dot product of multilinear_kzg.rs:37-42 / :100-107.
 * Windows of more than 16 bits sort their entries most-significant-digit first (csrc/msm_sort_wide.cuh). */
int zk_msm_g1(const zk_table *scalars, const zk_g1_bases *bases, int window_bits, uint64_t *out12,
              zk_msm_stats *stats /* may be NULL */);

/* Optional, once per setup (TrustedSetup.g1_powers_of_tau is fixed across commits, trusted_setup.rs:5-8): keep one copy of the
 * points per window, 2^(c w) B_i, so that every window of a later zk_msm_g1 / zk_kzg_commit on these bases feeds ONE bucket set:
 * ceil(256 / c) bucket additions per term with c = 22 (window_bits = 0: chosen from n), one bucket reduction, no window
 * combination.  Costs ceil(256 / c) x 128 bytes per point of HBM and (W - 1) c doublings per point to build; the group element
 * returned by the MSM is the same.  A later call with another window size rebuilds the copies. */
int zk_g1_bases_precompute(zk_g1_bases *b, int window_bits);
int zk_g1_bases_precomputed_window(const zk_g1_bases *b);      /* 0: none */

/* compute_lagrange_basis  trusted_setup.rs:24-49 : eq table of tau, built in HBM (O(2^n)) */
int zk_kzg_lagrange_basis(const uint64_t *taus, size_t ntaus, zk_table **out);
/* compute_g1_powers_of_tau :51-60 : [L_i(tau)] G for all i (fixed-base windowed scalar mul) */
int zk_kzg_setup_g1(const uint64_t *taus, size_t ntaus, zk_g1_bases **out);
/* commit_to_polynomial  multilinear_kzg.rs:25-45 */
int zk_kzg_commit(const zk_table *poly, const zk_g1_bases *g1_powers, uint64_t *out12);
/* open_and_prove :50-126.  The reference runs a full-size naive dot product per round over the
 * blown-up quotient; the same group elements are obtained here as MSMs of sizes 2^(n-1) .. 1
 * against pre-summed bases (zk_kzg_opening_key, built once per setup).  n_g2 = the setup's
 * g2_powers_of_tau length (only compared, :60-64).  proofs: nopen affine points.
 * The independent level MSMs of one call run on up to 3 library-owned host threads, each with its
 * own stream (environment ZK_KZG_OPEN_THREADS = 1 .. 4; 1 keeps everything on the caller's thread
 * and stream); the call returns when all of them have finished. */
typedef struct zk_kzg_opening_key zk_kzg_opening_key;
int zk_kzg_opening_key_new(const zk_g1_bases *g1_powers, zk_kzg_opening_key **out);
int zk_kzg_opening_key_free(zk_kzg_opening_key *k);
/* Optional, once per key: zk_g1_bases_precompute on every pre-summed level of at least `min_points` points (0: 2^18), so that
 * the level MSMs of later openings (multilinear_kzg.rs:96-107) run on one bucket set each.  window_bits = 0: chosen per level.
 * Costs as zk_g1_bases_precompute, summed over the levels (about as much again as for the setup itself); the proofs are the
 * same group elements. */
int zk_kzg_opening_key_precompute(zk_kzg_opening_key *k, int window_bits, size_t min_points);
int zk_kzg_open(const zk_table *poly, const zk_g1_bases *g1_powers, const zk_kzg_opening_key *key,
                const uint64_t *opening, size_t nopen, size_t n_g2, uint64_t *evaluation, uint64_t *proofs);
/* Open k polynomials (equal length 2^nopen, BLS12-381 Fr) at ONE point with ONE proof (extension: no reference counterpart).
 * Transcript (t = NULL: a fresh Transcript::new()), in this order, as plain appends:
 *   for j < k: x_j || y_j of commitment j, each the canonical 48-byte BIG-endian Fq integer (infinity: 96 zero bytes);
 *   for i < nopen: opening[i] as field_element_to_bytes (32-byte canonical big-endian, sumcheck_gkr_protocol.rs:152);
 *   for j < k: evaluations[j], same encoding;
 *   then gamma = random_challenge_as_field_element() (fiat_shamir_transcript.rs:38).
 * evaluations: k elements (f_j(opening)); proofs: nopen affine points = open_and_prove of sum_j gamma^j f_j;
 * gamma (may be NULL): the sampled challenge.  commitments12: k affine points (zk_kzg_commit of each polynomial), bound by the
 * transcript.  Preconditions and codes as zk_kzg_open, plus ZK_E_NVARS / ZK_E_ARG as zk_mle_linear_combination.  The first
 * level's combination, quotient and fold are one pass over the k tables; the level MSMs are those of one zk_kzg_open. */
int zk_kzg_batch_open(const zk_table *const *polys, size_t k, const uint64_t *commitments12,
                      const zk_g1_bases *g1_powers, const zk_kzg_opening_key *key,
                      const uint64_t *opening, size_t nopen, size_t n_g2, zk_transcript *t,
                      uint64_t *evaluations, uint64_t *gamma, uint64_t *proofs);

/* prove_succinct  gkr/src/succinct_gkr_protocol.rs:35-169 (BLS12-381 Fr): the GKR proof of
 * zk_gkr_prove plus commit(inputs) (:42-44) and the two openings at the last layer's rb / rc
 * (:154-157).  rb_proofs / rc_proofs: nlayers affine points each. */
int zk_gkr_prove_succinct(const zk_gate *gates, const size_t *gate_counts, size_t nlayers,
                          const uint64_t *inputs, size_t ninputs, const zk_g1_bases *g1_powers, size_t n_g2,
                          uint64_t *circuit_output, size_t *output_len, uint64_t *claimed_sum,
                          uint64_t *layer_claims, uint64_t *coeffs, uint64_t *challenges,
                          uint64_t *wb_evals, uint64_t *wc_evals, uint64_t *commitment12,
                          uint64_t *rb_evaluation, uint64_t *rb_proofs, uint64_t *rc_evaluation,
                          uint64_t *rc_proofs);

/* ---- verifier side of multilinear KZG: G2, pairings (HOST code: O(n) work on n + 2 points, csrc/pairing.h) ------------
 * G2 points: affine over Fq2, 24 limbs = x.c0, x.c1, y.c0, y.c1 (6 x u64 Montgomery each), all zero = infinity.
 * GT elements: 72 limbs = the Fq2 coefficients of w^0 .. w^5 in Fq12 = Fq2[w]/(w^6 - (1 + u)), (c0, c1) each. */
int zk_g2_generator(uint64_t *out24);
int zk_g2_is_on_curve(const uint64_t *p24);                                 /* 1 / 0 */
int zk_g2_add(const uint64_t *p24, const uint64_t *q24, uint64_t *out24);
int zk_g2_mul_fr(const uint64_t *p24, const uint64_t *scalar_fr, uint64_t *out24);          /* mul_bigint(into_bigint) */
int zk_pairing(const uint64_t *g1_12, const uint64_t *g2_24, uint64_t *gt72);               /* P::pairing */
int zk_pairing_product_is_one(const uint64_t *g1s, const uint64_t *g2s, size_t n, int *ok);
/* compute_g2_powers_of_tau  trusted_setup.rs:62-72 : out[i] = [tau_i] G2 (ntaus x 24 limbs) */
int zk_kzg_setup_g2(const uint64_t *taus, size_t ntaus, uint64_t *out);
/* MultilinearKZG::verify  multilinear_kzg.rs:131-158 ; *ok = 1 / 0.  nopen != nproofs -> ZK_E_KZG_LEN (:137-141), as is
 * ng2 > nproofs (the reference indexes proofs[i] for every G2 power, :149-154) */
int zk_kzg_verify(const uint64_t *commitment12, const uint64_t *opening_values, size_t nopen, const uint64_t *evaluation,
                  const uint64_t *proofs, size_t nproofs, const uint64_t *g2_powers, size_t ng2, int *ok);
/* The verifier of zk_kzg_batch_open: replays the same transcript steps, then MultilinearKZG::verify (multilinear_kzg.rs:131-158)
 * on C = sum gamma^j C_j, v = sum gamma^j v_j.  *ok = 1 / 0.  Length codes as zk_kzg_verify; k = 0 -> ZK_E_ARG.  Every status is
 * returned before the transcript is touched.  Extension: no reference counterpart. */
int zk_kzg_batch_verify(const uint64_t *commitments12, size_t k, const uint64_t *opening, size_t nopen,
                        const uint64_t *evaluations, const uint64_t *proofs, size_t nproofs,
                        const uint64_t *g2_powers, size_t ng2, zk_transcript *t, int *ok);

/* verify_succinct  gkr/src/succinct_gkr_protocol.rs:172-285 (BLS12-381 Fr): GKR verification without the inputs, then the
 * two KZG openings of the committed input polynomial at the last layer's challenges */
int zk_gkr_verify_succinct(const zk_gate *gates, const size_t *gate_counts, size_t nlayers, const uint64_t *circuit_output,
                           size_t output_len, const uint64_t *layer_claims, const uint64_t *coeffs, const uint64_t *wb_evals,
                           const uint64_t *wc_evals, const uint64_t *commitment12, const uint64_t *rb_evaluation,
                           const uint64_t *rb_proofs, size_t n_rb_proofs, const uint64_t *rc_evaluation, const uint64_t *rc_proofs,
                           size_t n_rc_proofs, const uint64_t *g2_powers, size_t ng2, int *ok);

/* ---- sparse (linear-time) GKR prover: the generalisation BASELINE config 4 needs -------------------------
 * The reference materialises dense wiring predicates add_i / mul_i of 2^(3i+2) entries and a dense f(b,c) of
 * 2^(2i+2) entries (arithmetic_circuit.rs:126-163, utils.rs:8-21) and ties a layer's width to its index
 * (:166-178).  Here a layer is a gate LIST (out, left, right, op) with its own widths: layer l has
 * 2^out_bits[l] outputs and reads the 2^out_bits[l+1] wires of the next layer (the inputs for the last one).
 * Each layer's 2k-round sumcheck is run in two phases (b then c) on tables built from the gate list in
 * O(#gates + 2^k):   phase 1  f = W(b) H1(b) + H0(b),   phase 2  f = A(c)(u + W(c)) + M(c) u W(c).
 * The round polynomials are the SAME polynomials as the dense definition's, so on circuits of the
 * reference's shape the proof is bit-identical to zk_gkr_prove / gkr_protocol::prove (tests/test_gpu_gkr_sparse.py).
 * With out_bits[0] = k0 > 1 the output claim uses k0 successive challenges (the reference has k0 = 1).
 * Proof layout as zk_gkr_prove with rounds(l) = 2 * in_bits(l). */
int zk_gkr_sparse_prove(int field, const zk_gate *gates, const size_t *gate_counts, size_t nlayers,
                        const uint32_t *out_bits, const uint64_t *inputs, size_t ninputs,
                        uint64_t *circuit_output, uint64_t *claimed_sum, uint64_t *layer_claims,
                        uint64_t *coeffs, uint64_t *challenges, uint64_t *wb_evals, uint64_t *wc_evals,
                        uint64_t *output_challenges /* out_bits[0] elements */, float *ms_layers /* nlayers, may be NULL */);
/* a circuit compiled once (gate lists uploaded and grouped by left / right / output index) and reused by
 * any number of proofs: the per-circuit preprocessing is O(#gates) host work that does not belong in a proof */
typedef struct zk_sparse_circuit zk_sparse_circuit;
int zk_sparse_circuit_new(const zk_gate *gates, const size_t *gate_counts, size_t nlayers, const uint32_t *out_bits,
                          size_t ninputs, zk_sparse_circuit **out);
int zk_sparse_circuit_free(zk_sparse_circuit *c);
int zk_gkr_sparse_prove_compiled(int field, const zk_sparse_circuit *c, const uint64_t *inputs, size_t ninputs,
                                 uint64_t *circuit_output, uint64_t *claimed_sum, uint64_t *layer_claims,
                                 uint64_t *coeffs, uint64_t *challenges, uint64_t *wb_evals, uint64_t *wc_evals,
                                 uint64_t *output_challenges, float *ms_layers);
/* the same proof with the output layer bound by its COMMITMENT (extension): the transcript's first append (gkr_protocol.rs:49) is the
 * Merkle root of the output layer (zk_mle_merkle_root, returned in output_root32) instead of its bytes; the output challenges and
 * everything after them follow from the transcript as before. */
int zk_gkr_sparse_prove_committed(int field, const zk_sparse_circuit *c, const uint64_t *inputs, size_t ninputs,
                                  uint64_t *circuit_output, uint64_t *claimed_sum, uint64_t *layer_claims,
                                  uint64_t *coeffs, uint64_t *challenges, uint64_t *wb_evals, uint64_t *wc_evals,
                                  uint64_t *output_challenges, float *ms_layers, uint8_t output_root32[32]);
/* Succinct sparse GKR without a trusted setup, for ZK_FR381 and ZK_BN254_FR (extension): the inputs are the table `cm` commits to
 * (zk_fri_commit; 2^in_bits(last layer) entries, else ZK_E_LEN_MISMATCH; no host copy is passed), and the verifier holds the gate lists, the
 * output layer and the commitment's 32-byte root.  The GKR transcript's FIRST append is that root (returned in input_root32); every append
 * of zk_gkr_sparse_prove_compiled follows unchanged, so the last layer's challenges rb and rc depend on the commitment.  Then
 * zk_fri_ml_open_points opens the commitment at z^0 = rb, z^1 = rc (P = 2; the last layer's first and second k = in_bits challenges) on a
 * FRESH Transcript::new(): the opening absorbs its whole statement -- header, root, points, values -- itself, and the GKR sponge lives in
 * device slots, so nothing is gained by continuing it.  input_evals (2 elements) = the opening's y_0, y_1: they take the place of the last
 * layer's W(rb), W(rc) in the verifier's final check.  The proof outputs are zk_gkr_sparse_prove_compiled's, the opening outputs
 * zk_fri_ml_open's (sizes: zk_fri_ml_sizes(in_bits, cm's b, log_final, nqueries)). */
int zk_gkr_sparse_prove_succinct(int field, const zk_sparse_circuit *c, const zk_fri_commitment *cm, uint32_t log_final, uint32_t nqueries,
                                 uint64_t *circuit_output, uint64_t *claimed_sum, uint64_t *layer_claims, uint64_t *coeffs,
                                 uint64_t *challenges, uint64_t *wb_evals, uint64_t *wc_evals, uint64_t *output_challenges, float *ms_layers,
                                 uint8_t input_root32[32], uint64_t *input_evals, uint64_t *open_round_polys, uint8_t *roots,
                                 uint64_t *final_table, uint64_t *open_challenges, uint64_t *query_indices, uint64_t *query_values,
                                 uint8_t *query_paths);
/* independent evaluation of the wiring predicates at a point (the verifier's O(#gates) work):
 * add_r = sum_{add gates} w_g eq(rb, left_g) eq(rc, right_g), same for mul, with
 * w_g = alpha eq(pa, out_g) + beta eq(pb, out_g)  (layer 0: alpha = 1, beta = 0, pa = output challenges). */
int zk_gkr_sparse_wiring_eval(int field, const zk_gate *layer_gates, size_t ngates, uint32_t out_bits, uint32_t in_bits,
                              const uint64_t *alpha, const uint64_t *pa, const uint64_t *beta, const uint64_t *pb,
                              const uint64_t *rb, const uint64_t *rc, uint64_t *add_r, uint64_t *mul_r);
/* one phase's table kernel on its own, on tables the caller chooses (a hook for tests: it runs the functions the prover runs per layer --
 * the conversion of half tables to the products' internal form, the grid, the choice of kernel -- after the same grouping of the gate list).
 * phase 1: *x = H1, *y = H0 over the left index b,  H1(b) = sum_{g: left_g = b} w_g ([add] + [mul] other[right_g]),  H0(b) = sum_{g add: left_g = b}
 * w_g other[right_g];  phase 2: *x = C = A + u M, *y = A over the right index c,  A / M(c) = sum_{g add / mul: right_g = c} w_g other[left_g].
 * Both are new tables of 2^in_bits entries.  The weight w_g of a gate comes either from half tables, w_g = ah[o >> lbits] al[o & (2^lbits - 1)]
 * (+ bh[..] bl[..]; bh = bl = NULL: one product) at its output index o, with ah, bh of 2^(out_bits - lbits) and al, bl of 2^lbits entries and
 * 1 <= lbits < out_bits -- any reduced elements, not only eq tables; the kernels then run in the internal form, as the prover's do for layers
 * of more than 12 output bits -- or from w, ngates weights in gate order (ah .. bl NULL; ngates = 0: w is not read and may be NULL).  The other
 * table is `other`, 2^in_bits entries (phase 1: the next layer's values; phase 2: eq(rb*, .)), or in phase 2 its halves other_hi of
 * 2^(in_bits - other_lbits) and other_lo of 2^other_lbits entries, 1 <= other_lbits < in_bits (`other` NULL), which run in the internal form with
 * weights from half tables and in the stored form with w: the four combinations the prover reaches.  u: one reduced element, phase 2 only.
 * ZK_E_ARG, with nothing written: a phase other than 1 or 2, half tables AND w or neither (but for ngates = 0), half tables with ngates = 0, bh
 * without bl, halves of the other table in phase 1 or together with `other`, lbits or other_lbits out of range, out_bits or in_bits outside
 * 1 .. 30, a table of another field or length, u NULL in phase 2.  Then ZK_E_NO_DEVICE; ZK_E_RANGE for a gate index that does not fit.  The
 * inputs are not modified.  Extension: no reference counterpart. */
int zk_gkr_sparse_phase_tables(int field, int phase /* 1 | 2 */, const zk_gate *gates, size_t ngates, uint32_t out_bits, uint32_t in_bits,
                               const zk_table *ah, const zk_table *al, const zk_table *bh, const zk_table *bl, uint32_t lbits,
                               const zk_table *w, const zk_table *other, const zk_table *other_hi, const zk_table *other_lo,
                               uint32_t other_lbits, const uint64_t *u, zk_table **x, zk_table **y);
/* layer-by-layer evaluation of a sparse circuit on the GPU; evals = layer 0 .. inputs concatenated */
int zk_sparse_circuit_evaluate(int field, const zk_gate *gates, const size_t *gate_counts, size_t nlayers,
                               const uint32_t *out_bits, const uint64_t *inputs, size_t ninputs, uint64_t *evals);

/* ---- multi-GPU provers: one process per GPU, RCCL over xGMI -------------------------------------
 * A zk_comm is this rank's end of the node's communicator.  zk_comm_init_rccl creates an RCCL communicator on the calling
 * thread's device (ncclCommInitRank; librccl.so.1 is opened at first use): rank 0 calls zk_comm_unique_id and ships the 128
 * bytes to the other ranks out of band (file, MPI, torch.distributed store ...).  Every collective of the provers below is
 * enqueued on the calling thread's current stream between the kernels it separates -- the device never waits for the host
 * inside a sumcheck.  zk_comm_from_host_ops is the same interface over caller-supplied HOST-memory exchange callbacks (the
 * library stages device <-> pinned host and synchronises around each call): for hosts that own another transport, and for
 * the multi-rank tests on one GPU (RCCL refuses two ranks on one device).
 * The tables of the reference's provers shard by the LOW index bits: rank g of G = 2^k holds the entries i == g (mod G) as a
 * contiguous local table (local index i >> k), so that every round that folds variable 0 (prover.rs:62,
 * sumcheck_gkr_protocol.rs:57) is local; MSM terms shard by contiguous slices. */
typedef struct zk_comm zk_comm;
typedef struct {
    void *ctx;
    /* in-place element-wise sum over the ranks of `count` int64 words */
    int (*all_reduce_sum_i64)(void *ctx, int64_t *host_buf, size_t count);
    /* recv = send buffers of all ranks in rank order (bytes each) */
    int (*all_gather)(void *ctx, const void *host_send, void *host_recv, size_t bytes);
    /* root's recv = send buffers of all ranks in rank order; recv is NULL on the other ranks */
    int (*gather)(void *ctx, const void *host_send, void *host_recv, size_t bytes, int root);
    int (*broadcast)(void *ctx, void *host_buf, size_t bytes, int root);
} zk_comm_host_ops;                                               /* every callback returns 0 on success */
int zk_comm_unique_id(uint8_t out128[128]);                       /* ncclGetUniqueId */
int zk_comm_init_rccl(const uint8_t id128[128], int nranks, int rank, zk_comm **out);
int zk_comm_from_host_ops(const zk_comm_host_ops *ops, int nranks, int rank, zk_comm **out);
/* The ranks as THREADS of one process (one thread per GPU, or several ranks sharing one GPU in tests and rehearsals): a
 * group of `nranks` ends that exchange through the process's own host memory.  Every rank's thread creates its end with
 * zk_comm_from_local_group (backend "local-threads") and calls the provers concurrently, each on its own stream; the group
 * outlives its ends and is freed by the caller after them.  zk_comm_local_group_abort wakes every rank that waits in an
 * exchange (they return ZK_E_COMM): what a rank calls when its own proof failed, so that nobody hangs. */
typedef struct zk_comm_local_group zk_comm_local_group;
int zk_comm_local_group_new(int nranks, zk_comm_local_group **out);
int zk_comm_local_group_free(zk_comm_local_group *g);
int zk_comm_local_group_abort(zk_comm_local_group *g);
int zk_comm_from_local_group(zk_comm_local_group *g, int rank, zk_comm **out);
int zk_comm_free(zk_comm *c);
int zk_comm_rank(const zk_comm *c);
int zk_comm_size(const zk_comm *c);
const char *zk_comm_backend(const zk_comm *c);                    /* "rccl", "host-ops" or "local-threads" */
/* payload bytes this rank has received through the communicator so far (all-reduce: the buffer; all-gather / gather at the
 * root: the other ranks' parts; broadcast: the buffer on non-root ranks) and the number of collectives issued */
int zk_comm_stats(const zk_comm *c, uint64_t *bytes_received, uint64_t *collectives);
/* primitives, on device buffers, enqueued on the current stream (what the provers below are made of) */
int zk_comm_all_reduce_sum_i64(zk_comm *c, void *dev_buf, size_t count);
int zk_comm_all_gather(zk_comm *c, const void *dev_send, void *dev_recv, size_t bytes);
int zk_comm_broadcast(zk_comm *c, void *dev_buf, size_t bytes, int root);
/* the same exchanges on HOST buffers, for the callback kinds only ("host-ops", "local-threads"; ZK_E_ARG on an RCCL
 * communicator): op 0 = all-reduce(SUM) of n int64 words in place, 1 = all-gather of n bytes per rank into host_recv,
 * 2 = gather to `root` (host_recv on the root only), 3 = broadcast of n bytes from `root`.  Needs no device. */
int zk_comm_host_exchange(zk_comm *c, int op, void *host_buf, void *host_recv, size_t n, int root);

/* Prover::prove (prover.rs:35-71) of the global table whose low-bit shard is `shard` (local length 2^m, global 2^(m+k)).
 * Same proof bytes on every rank as zk_sumcheck_basic_prove on the interleaved table.  Per local round: one fused kernel,
 * ONE all-reduce of 18 int64 words, the transcript step on every rank's device.  absorb_table != 0 hashes the whole table
 * first (:38-39): the ranks stream their canonical bytes to rank 0 in chunks (gather), rank 0 absorbs them in global index
 * order and broadcasts the 208-byte sponge (25 lanes + fill) -- non-root ranks receive 208 bytes for the absorb. */
int zk_sharded_sumcheck_basic_prove(zk_comm *c, const zk_table *shard, int absorb_table, uint64_t *claimed_sum,
                                    uint64_t *round_polys /* (m + k) x 2 */, uint64_t *challenges /* m + k, may be NULL */);
/* sumcheck_gkr_protocol::prove (:24-67) on low-bit shards of the nprod x nfac tables; `t` must hold the same state on every
 * rank and is advanced identically.  final_values (nprod * nfac elements, may be NULL) = the fully folded tables. */
int zk_sharded_sumcheck_gkr_prove(zk_comm *c, const zk_table *const *shards, size_t nprod, size_t nfac,
                                  const uint64_t *claimed_sum, zk_transcript *t, uint64_t *round_coeffs, uint64_t *challenges,
                                  uint64_t *final_values);
/* MultilinearPolynomial::evaluate (evaluation_form.rs:21-33) of the sharded table at nvalues = m + k points: m local fold
 * rounds, one all-gather of G elements, k replicated rounds */
int zk_sharded_mle_evaluate(zk_comm *c, const zk_table *shard, const uint64_t *values, size_t nvalues, uint64_t *out);
/* commit_to_polynomial (multilinear_kzg.rs:37-42) with the terms sliced over the ranks: one Pippenger per rank, one
 * all-gather of G affine points (96 B each), G - 1 additions.  Same point on every rank. */
int zk_sharded_msm_g1(zk_comm *c, const zk_table *scalars_slice, const zk_g1_bases *bases_slice, int window_bits,
                      uint64_t *out12, zk_msm_stats *stats /* this rank's local MSM, may be NULL */);
/* open_and_prove (multilinear_kzg.rs:50-126) of the low-bit-sharded table (local length 2^m, G = 2^k ranks, nopen = m + k opening
 * values).  bases_local = the rank's own powers P_{j G + g} (the same low-bit shard of g1_powers_of_tau), key_local = the opening key
 * of bases_local (zk_kzg_opening_key_new; NULL: built for the call).  The first m proofs are sums over the ranks of local MSMs, the
 * last k are computed replicated from the G leftover entries and the G per-rank base totals: ONE all-gather of (m + 1) points + one
 * element per rank.  evaluation and the m + k proofs are the single-device ones, on every rank. */
int zk_sharded_kzg_open(zk_comm *c, const zk_table *shard, const zk_g1_bases *bases_local, const zk_kzg_opening_key *key_local,
                        const uint64_t *opening, size_t nopen, uint64_t *evaluation, uint64_t *proofs /* (m + k) x 12 */);

#ifdef __cplusplus
}
#endif
#endif
