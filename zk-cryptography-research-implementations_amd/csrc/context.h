// context.h -- library-internal: status helpers, HIP error capture, per-device scratch, tables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>

#include "../../include/zkmle.h"

namespace zk {

void set_last_error(const std::string &s);

#define ZK_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t e__ = (call);                                                              \
        if (e__ != hipSuccess) {                                                              \
            ::zk::set_last_error(std::string(#call) + ": " + hipGetErrorString(e__));         \
            return (e__ == hipErrorNoDevice || e__ == hipErrorInvalidDevice ||                \
                    e__ == hipErrorInsufficientDriver) ? ZK_E_NO_DEVICE : ZK_E_HIP;           \
        }                                                                                     \
    } while (0)

#define ZK_TRY(expr)                         \
    do {                                     \
        int rc__ = (expr);                   \
        if (rc__ != ZK_OK) return rc__;      \
    } while (0)

// Fails loudly (ZK_E_NO_DEVICE) when there is no GPU: there is no CPU fallback in this library.
int require_device();
// The calling thread's current stream (zk_set_stream; the null stream by default).  Every kernel launch, copy and
// synchronisation of the library goes through it, so threads that set different streams run their calls concurrently on
// the device.  Scratch buffers, the caching pool and the statistics are per thread as well.
hipStream_t cur_stream();
hipError_t memcpy_on_stream(void *dst, const void *src, size_t bytes, hipMemcpyKind kind);   // async copy + stream sync
hipError_t memset_on_stream(void *dst, int value, size_t bytes);
// wait until the current stream has drained, polling hipStreamQuery for the first ~0.3 ms (a blocking hipStreamSynchronize wakes up
// 20-30 us after the last kernel has ended: a quarter of a small proof) before falling back to it
hipError_t stream_wait_idle();
// one block of words per thread and device, zero when handed out: the arrival counter (first 64 bytes) and the segment accumulators of
// the passes that run their exchange themselves (basic_multi.cuh MultiFin).  Whoever uses it leaves it zero; sync_words_reset() after a
// proof that may not have.
constexpr size_t kSyncCounterBytes = 64 * (1 + 256);        // the pass's counter and one per segment, 64 bytes apart
constexpr size_t kSyncWordsBytes = kSyncCounterBytes + (size_t)256 * 12 * 128;   // + one 128-byte line per (segment, limb) accumulator word
int sync_words(void **out);
int sync_words_reset();
// device scratch for reduction partials: at least `bytes` bytes, owned per device, reused
int scratch(size_t bytes, void **out);
// pinned host staging for small results (a few field elements)
int host_staging(size_t bytes, void **out);
// one block (16 KiB) of pinned, COHERENT (fine-grained) host memory per thread and device, mapped into the device: the mailbox of the
// host-assisted transcript step (dev_transcript.cuh HostMailbox).  *host and *dev address the same memory.
int host_mailbox(void **host, void **dev);

// Caching device allocator for per-call scratch (the MSM allocates several GB per call; hipMalloc / hipFree of
// such blocks costs milliseconds).  Freed blocks are kept per THREAD and device and reused by that thread's later calls of
// similar size (stream-ordered: a thread's work runs on its current stream, and changing the stream synchronises the
// old one first); zk_release_cached_memory() returns the calling thread's blocks to the driver.
int pool_alloc(size_t bytes, void **out);
void pool_free(void *p);

inline bool is_pow2(size_t x) { return x && !(x & (x - 1)); }
inline unsigned ilog2(size_t x) { unsigned k = 0; while (x >>= 1) k++; return k; }
// ZK_PROOF_TRACE=1 (measurement only): host clock and in-kernel stamps of a proof's phases on stderr
inline bool proof_trace() {
    static const bool v = [] { const char *e = getenv("ZK_PROOF_TRACE"); return e && e[0] == '1'; }();
    return v;
}
inline int field_limbs64(int field) { return field == ZK_FQ381 ? 6 : (field >= 0 && field <= 3 ? 4 : -1); }

}  // namespace zk

struct zk_table {
    int field;
    size_t len;
    void *dptr;
    int owned;      // 0 = view of caller memory (zk_table_wrap), 1 = hipMalloc, 2 = block of the scratch pool
};
// the prover's side of a FRI commitment (zkmle_fri_pcs.hip makes and frees it; zkmle_fri_ml.hip opens it as a multilinear polynomial)
struct zk_fri_commitment {
    int field;
    unsigned d, b;
    bool has_coset;
    uint64_t coset[4];
    zk_table *coeffs, *codeword;     // long-lived tables of their own (zk_table_clone, zk_table_alloc)
    uint64_t *levels;                // 2 N - 1 digests (hipMalloc), zk_merkle_build's layout; log_group != 0: 2 (N >> log_group) - 1, zk_merkle_build_grouped's
    uint8_t root[32];
    unsigned log_group;              // 0, or 2: a leaf per coset of the first fold by 4 (zk_fri_commit_grouped).  Who walks `levels` as 2 N - 1 digests refuses the latter
};

// the prover's side of a commitment to k columns under ONE tree (zkmle_fri_pcs.hip makes and frees it; zkmle_fri_ml.hip opens several together)
struct zk_fri_columns {
    int field;
    unsigned d, b, k;
    bool has_coset;
    uint64_t coset[4];
    zk_table *coeffs[ZK_FRI_COLUMNS_MAX], *codeword[ZK_FRI_COLUMNS_MAX];   // long-lived tables of their own, k of each
    uint64_t *levels;                // 2 (N / 4) - 1 digests (ONE hipMalloc), zk_merkle_build_columns' layout
    uint8_t root[32];
};

namespace zk {
class Transcript;
// transcript.append(convert_to_bytes(table)) (evaluation_form.rs:35-43, prover.rs:38-39): the GPU converts Montgomery ->
// canonical big-endian chunk by chunk into pinned host buffers while the host hashes the previous chunk (zkmle_sumcheck.hip)
int transcript_absorb_table(Transcript &t, const zk_table *table);
// the table's Keccak-256 Merkle root, root-only mode (zkmle_merkle.hip): what the committed provers append in place of the table's bytes
int merkle_root_device(const zk_table *t, uint8_t root32[32]);
// every level of the table's tree into the caller's device block of 2 len - 1 digests, laid out as zk_merkle_build's; launches only, no
// checks (the FRI prover: one block for the trees of all its layers)
int merkle_levels_device(const zk_table *t, uint64_t *levels);
// the same with grouped leaves (merkle.cuh; log_group <= 2, 32-byte elements, len >= 2^log_group): 2 (len >> log_group) - 1 digests, zk_merkle_build_grouped's
// layout; launches only, no checks.  log_group = 0 is merkle_levels_device
int merkle_levels_grouped_device(const zk_table *t, unsigned log_group, uint64_t *levels);
// several columns under one tree (merkle_columns.cuh; the two scalar fields): merkle_columns_check gives the statuses that need no device --
// ZK_E_ARG for a null, k outside 1 .. 32, another field, mixed fields or len < min_len, ZK_E_LEN_MISMATCH, ZK_E_NOT_POW2 -- the others are launches
// only, no checks: the len >> 2 leaves into `levels`, the nodes above `leaves` digests (zk_merkle_build_grouped's layout), and both
int merkle_columns_check(const zk_table *const *tables, uint32_t k, size_t min_len = 4);
int merkle_leaves_columns_device(const zk_table *const *tables, uint32_t k, uint64_t *levels);
int merkle_nodes_device(uint64_t *levels, size_t leaves);
int merkle_levels_columns_device(const zk_table *const *tables, uint32_t k, uint64_t *levels);
// zk_uni_low_degree_extend into a table the caller allocated (out->len = coeffs->len << log_blowup); launches only, no checks (zkmle_ntt.hip)
int ntt_extend_into(const zk_table *coeffs, const uint64_t *coset, zk_table *out);
// zk_fri_verify's checks and body on a caller's Transcript; indices_out (nqueries words, may be null) receives the sampled query indices
// (zkmle_fri.hip; the opening verifier of zkmle_fri_pcs.hip checks the committed polynomials at the same positions)
// `ml` (may be null) switches the fold mode: the proof is the multilinear opening of include/zkmle.h (zkmle_fri_ml.hip) -- z and y are appended
// after root_0, every round's three evaluations before its challenge, the layers fold in Lagrange form, `final_coeffs` is the final table T_R
// and the sumcheck's checks are made beside FRI's.  roots[0] is then the verifier's own copy of the commitment's root.
// npoints > 0: the opening at SEVERAL points ("... opened at several points"): z holds npoints x d elements (point-major), y npoints elements;
// after root_0 the transcript takes npoints (4 bytes), the points, the claims, then gamma is drawn; the sumcheck's first claim is
// sum_p gamma^p y_p and its last check is sum_p gamma^p A^p_R MLE(T_R)(z^p_0 .. z^p_{f-1}) = claim.  npoints = 0: the single-point form, as before.
struct FriMlClaim {
    const uint64_t *z, *y, *round_polys;                     // d elements, one element, R x 3 elements
    uint32_t npoints = 0;
    uint32_t log_arity = 1;                                  // 2: the opening folded by 4 (include/zkmle.h "... opened with a fold arity"); needs npoints >= 1
    uint32_t grouped = 0;                                    // 1: every layer's leaves hold a step's sides ("... with grouped leaves"); needs log_arity = 2
    // k > 0: k commitments opened together ("FRI commitments opened together"; needs npoints >= 1).  y holds k x npoints claims table-major and
    // `roots` starts with the k commitments' roots (the verifier's own copies), the later layers' behind them; a query's step 0 holds the k
    // commitments' values and paths, j-major, and the step's values are their alpha-combination, alpha = gamma^npoints.  0: one table, as before
    uint32_t ntables = 0;
    // ncommit > 0: COLUMN commitments opened together ("Column commitments opened together"; needs log_arity = 2, grouped and ntables = the sum
    // of the widths): `widths` holds the ncommit widths, `roots` starts with the ncommit roots, the statement carries "COLS", and a query's step 0
    // holds the ntables columns' values as ever but ONE path per commitment, whose leaf is hashed from that commitment's 4 w_i values
    const uint32_t *widths = nullptr;
    uint32_t ncommit = 0;
    // weighted_c != null: the opening against a caller's weight table ("FRI commitment opened against a weight table"; needs npoints = 0 and
    // ntables = 0; z and y are not read): "WGHT" and the claim c follow root_0 (and the arity line), the sumcheck starts from c and ends in
    // sum_j T_R[j] w_final[j], and every replayed r_l must equal challenges[l] (R elements, as the proof carries them)
    const uint64_t *weighted_c = nullptr, *challenges = nullptr, *w_final = nullptr;
};
// zk_fri_ml_open_columns_pow's own statuses (zkmle_fri_ml.hip), every ZK_E_ARG and then ZK_E_NO_DEVICE, as fri_ml_open_batch_check for a prover
// that runs rounds of its own before it opens column commitments
int fri_ml_open_columns_check(const zk_fri_columns *const *cms, uint32_t m, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries,
                              const uint64_t *ys_out, uint64_t *round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *query_values,
                              uint8_t *query_paths, uint32_t grinding_bits, const uint64_t *pow_nonce);
// zk_fri_commit_columns on k device tables that the caller owns (zk_table_alloc or the pool; not zk_table_wrap) and hands over: with ZK_OK they are
// the commitment's own tables, freed with it, and nothing is cloned; with any other status they stay the caller's.  The statuses are
// zk_fri_commit_columns' (zkmle_fri_pcs.hip; the prover on column commitments commits the helper tables it has just made)
int fri_commit_columns_adopt(zk_table *const *tables, uint32_t k, uint32_t log_blowup, const uint64_t *coset, zk_fri_columns **out);
// grind_bits > 0: the proof-of-work step (include/zkmle.h "Proof-of-work grinding") with the nonce pow_nonce stands between the final
// coefficients and the indices; a nonce that fails it gives *ok = 0.  grind_bits > ZK_FRI_GRIND_MAX_BITS: ZK_E_ARG
int fri_verify_core(int field, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset, Transcript &tr,
                    const uint8_t *roots, const uint64_t *final_coeffs, const uint64_t *query_values, const uint8_t *query_paths, int *ok,
                    uint64_t *indices_out, const FriMlClaim *ml = nullptr, uint32_t grind_bits = 0, uint64_t pow_nonce = 0,
                    uint32_t max_tables = ZK_FRI_ML_BATCH_MAX);   // the most commitments opened together: the wide verifier passes ZK_FRI_ML_WIDE_MAX
// zk_fri_ml_open_batch_pow's own statuses (zkmle_fri_ml.hip), every ZK_E_ARG and then ZK_E_NO_DEVICE, for a prover that runs rounds of its own on
// the transcript before it calls that opener at a point those rounds produce (zkmle_zerocheck.hip): `points` is then any reduced stand-in
int fri_ml_open_batch_check(const zk_fri_commitment *const *cms, uint32_t k, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries,
                            uint32_t log_arity, const uint64_t *ys_out, uint64_t *round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *query_values,
                            uint8_t *query_paths, uint32_t grinding_bits, const uint64_t *pow_nonce, uint32_t max_tables = ZK_FRI_ML_BATCH_MAX);   // ZK_FRI_ML_WIDE_MAX: zk_fri_ml_open_batch_wide_pow's
// zk_fri_ml_open_weighted's own statuses (zkmle_fri_ml.hip), every ZK_E_ARG, ZK_E_LEN_MISMATCH and then ZK_E_NO_DEVICE, for a prover that runs
// rounds of its own on the transcript before it opens against a weight table those rounds produce
int fri_ml_open_weighted_check(const zk_fri_commitment *cm, const zk_table *weights, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                               const uint64_t *c_out, uint64_t *round_polys, uint8_t *roots, uint64_t *final_table, const uint64_t *challenges,
                               uint64_t *query_values, uint8_t *query_paths, uint32_t grinding_bits, const uint64_t *pow_nonce);
// steps 1-3 of the proof-of-work step on `tr` with the search on the GPU (zkmle_grind.hip): zk_transcript_grind's checks and body
int transcript_grind(Transcript &tr, uint32_t bits, uint64_t start, uint32_t log_batch, uint64_t *nonce);
// Prover::prove (prover.rs:35-71) on a caller's Transcript whose binding append (:38-39) is the 32 bytes `bound` -- a commitment the caller
// holds -- instead of the table's bytes; no checks (zkmle_sumcheck.hip; the succinct sumcheck of zkmle_fri_ml.hip)
int sumcheck_basic_prove_bound(const zk_table *table, Transcript &tr, const uint8_t bound[32], uint64_t *claimed_sum, uint64_t *round_polys,
                               uint64_t *challenges);
// Proof slots shared by a proof made of several sumchecks (zkmle_sumcheck.hip): the sponge, the interpolation basis and every slot
// (coefficients, challenges, final values, layer links) live in ONE device block; rounds() and link() only enqueue kernels on the
// current stream, collect() is the single download.  Slot layout of rounds(): round k's nfac + 1 coefficients at s0 + per k, its
// challenge at s0 + per k + nfac + 1, then the nprod * nfac final values (per = nfac + 2).
struct ProofSlotsBase {
    virtual ~ProofSlotsBase() {}
    virtual void *slot_ptr(size_t s) const = 0;                    // device address of slot s
    virtual int upload_slot(size_t s, const uint64_t *el) = 0;
    // enqueue the rounds of a sum-of-products sumcheck (constant second factors: tables[p * 2 + 1] == null, value from const_host
    // (nprod elements) or const_dev[p] (device memory)); with_claim: proof[claim_slot] is absorbed in front of round 0's message
    virtual int rounds(size_t s0, const zk_table *const *tables, size_t nprod, size_t nfac, const uint64_t *const_host, const void *const *const_dev,
                       int with_claim, size_t claim_slot) = 0;
    // gkr_protocol.rs:109-133 on the device: append wb, alpha, append wc, beta, claim = alpha wb + beta wc
    // every sumcheck enqueued through rounds() proves a sum the prover computed itself; the first one's is told here (the later ones' are the
    // running claim of the previous phase or link), so that round 0 may derive e(1) = claim - e(0)
    virtual void set_claim(const uint64_t *el) = 0;
    virtual int link(size_t wb_src, size_t wc_src, size_t wb_slot, size_t wc_slot, size_t alpha_slot, size_t beta_slot, size_t claim_slot) = 0;
    virtual int collect(Transcript &tr, uint64_t *host_slots) = 0;   // every slot (field elements, u64 limbs) + the sponge back into tr
};
int proof_slots_new(int field, Transcript &tr, size_t npts, size_t nslots, ProofSlotsBase **out);
// open_and_prove's body with the subtracted value and the leftover entry exposed (zkmle_kzg.hip; the sharded opening builds on it)
int kzg_open_core(const zk_table *poly, const zk_g1_bases *g1_powers, const zk_kzg_opening_key *key, const uint64_t *opening, size_t nopen,
                  const uint64_t *v_given, uint64_t *evaluation, uint64_t *proofs, uint64_t *last);
int kzg_key_total(const zk_kzg_opening_key *k, const zk_g1_bases *g1, uint64_t *out12);
// two pinned host staging buffers of at least `bytes` each, owned per device
int pinned_pair(size_t bytes, void *out[2]);
// a temporary table backed by the caching pool (internal provers: dozens of same-sized temporaries per proof)
int table_alloc_pooled(int field, size_t len, zk_table **out);
// the argument checks of a linear combination of k tables (zk_mle_linear_combination, zk_kzg_batch_open), all before any device check:
// ZK_E_ARG for a null table, k = 0, k > 64 or mixed fields, ZK_E_NVARS for unequal lengths; with `out`, ZK_E_ARG for a field or length that does
// not fit or for memory that overlaps an input's
int lincomb_check(const zk_table *const *tables, size_t k, const zk_table *out);
// alpha fold(in, rb) + beta fold(in, rc) over the k <= 8 top variables in one pass (gkr/src/utils.rs:23-68; zkmle_core.hip)
int mle_fold_alpha_beta(const zk_table *in, size_t k, const uint64_t *alpha, const uint64_t *beta, const uint64_t *rb, const uint64_t *rc, zk_table *out);
}
