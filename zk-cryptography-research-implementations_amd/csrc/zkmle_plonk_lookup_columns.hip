// zkmle_plonk_lookup_columns.hip -- C ABI of the Plonk proof with lookup rows on COLUMN commitments (plonk_helpers.cuh,
// plonk_lookup_columns_host.h): the four helper tables in one pass on their own, the prover (the multiplicities as a one-column commitment,
// the four helper tables by ONE kernel as a four-column commitment, zkmle_plonk_lookup.hip's sumcheck unchanged on the twenty columns and E,
// then zk_fri_ml_open_columns_pow of the four commitments at the point the rounds leave, on the same transcript) and its host verifier.  The
// rounds are plonk_lookup_driver.cuh's on zerocheck_driver.cuh's round loop, whose table checks and shells' shared checks it uses too.
// Extension: the protocol is defined in include/zkmle.h "Plonk with lookups on column commitments".
#include <string.h>

#include <chrono>
#include <vector>

#include "lookup_driver.cuh"
#include "plonk_helpers.cuh"
#include "plonk_lookup_columns_host.h"
#include "plonk_lookup_driver.cuh"

using namespace zk;
using namespace zk::host;

namespace {

thread_local zk_plonk_lookup_stats g_stats{};

// the places of the helper kernel's eleven inputs (A, B, C, SA, SB, SC, qK, T0, T1, T2) among the fifteen given; M is the sixteenth
constexpr int kHelpersPlace[kPlonkHelpersIn - 1] = {0, 1, 2, 8, 9, 10, 11, 12, 13, 14};

// the prover's two helper commitments (M; H0, H1, H2, HL): freed with the call
struct HelperColumns {
    zk_fri_columns *m = nullptr, *h = nullptr;
    ~HelperColumns() {
        zk_fri_columns_free(m);
        zk_fri_columns_free(h);
    }
};
// tables that are the caller's until a commitment adopts them
struct Owned {
    zk_table *t[kPlonkHelpersOut] = {};
    ~Owned() { for (zk_table *x : t) zk_table_free(x); }
    void release() { for (zk_table *&x : t) x = nullptr; }
};

// H0, H1, H2, HL (n entries each, device) from the eleven tables.  Launches only.
template <class F> int launch_helpers(const void *const *in, void *const *out, size_t n, const Fe<F> &beta, const Fe<F> &gamma) {
    PlonkHelpersTables tb{};
    for (int j = 0; j < kPlonkHelpersIn; j++) tb.in[j] = in[j];
    for (int j = 0; j < kPlonkHelpersOut; j++) tb.out[j] = out[j];
    PlonkHelpersConsts<F> c;
    c.beta = beta;
    c.gamma = gamma;
    c.gamma2 = fe_mul<F>(gamma, gamma);
    c.gn = fe_mul<F>(gamma, fe_from_u64<F>((uint64_t)n));
    c.g256 = fe_mul<F>(gamma, fe_from_u64<F>((uint64_t)kPcsBlock));
    const size_t per = (size_t)kPlonkHelpersBatch * kPcsBlock;
    plonk_lookup_helpers_kernel<F><<<(unsigned)((n + per - 1) / per), kPcsBlock, 0, cur_stream()>>>(tb, n, c);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class F> int helpers_once(const zk_table *const *in, const uint64_t *beta, const uint64_t *gamma, zk_table **H) {
    Owned o;
    const void *ip[kPlonkHelpersIn];
    void *op[kPlonkHelpersOut];
    for (int j = 0; j < kPlonkHelpersIn; j++) ip[j] = in[j]->dptr;
    for (int j = 0; j < kPlonkHelpersOut; j++) {
        ZK_TRY(zk_table_alloc(in[0]->field, in[0]->len, &o.t[j]));
        op[j] = o.t[j]->dptr;
    }
    ZK_TRY(launch_helpers<F>(ip, op, in[0]->len, load_host<F>(beta), load_host<F>(gamma)));
    ZK_HIP(hipStreamSynchronize(cur_stream()));
    for (int j = 0; j < kPlonkHelpersOut; j++) H[j] = o.t[j];
    o.release();
    return ZK_OK;
}

// steps 1 to 9 on `tr`: the statement, M and its one-column commitment, the four helper tables and their four-column commitment (hc; h_roots: M's
// root, then the helpers'), then E_0 and zkmle_plonk_lookup.hip's d rounds on the columns' tables by plonk_lookup_driver.cuh; z (d elements) =
// the point the opening is made at.  One host synchronisation for the miss count beside the rounds'.
template <class F> int prove_steps(const zk_fri_columns *wit, const zk_fri_columns *cir, const uint64_t *pub, uint32_t npublic, Transcript &tr, HelperColumns &hc,
                                   uint8_t *h_roots, uint64_t *chal_out, uint64_t *round_polys, uint64_t *challenges, uint64_t *z, zk_plonk_lookup_stats &st) {
    constexpr int W = F::N / 2, K = kPlonkLookupOpened, G = kPlonkLookupGiven;
    const unsigned d = wit->d;
    const size_t n = (size_t)1 << d;
    const uint64_t *coset = wit->has_coset ? wit->coset : nullptr;
    const void *given[G];                                    // the fifteen in the order of the twenty claims
    for (int j = 0; j < G; j++) given[j] = (j < (int)kPlonkColumnsWitness ? wit->coeffs[j] : cir->coeffs[j - kPlonkColumnsWitness])->dptr;
    const void *lk[kLookupGiven];                            // the lookup's seven in its own order: A, B, C, qK, T0, T1, T2
    for (int j = 0; j < kLookupGiven; j++) lk[j] = given[kPlonkLookupLookupPlace[j]];
    WiringChallenges<F> ch;
    plonk_lookup_columns_statement<F>(tr, wit->root, cir->root, d, pub, npublic);

    Events ev;
    size_t e0, e1, e2, e3, e4;
    ZK_TRY(ev.mark(&e0));
    {
        Owned m;
        ZK_TRY(table_alloc_pooled(wit->field, n, &m.t[0]));
        ZK_TRY(multiplicities_into<F>(lk, n, m.t[0]->dptr, &st.misses));
        ZK_TRY(ev.mark(&e1));
        ZK_TRY(fri_commit_columns_adopt(m.t, 1, wit->b, coset, &hc.m));
        m.release();
    }
    memcpy(h_roots, hc.m->root, 32);
    ZK_TRY(ev.mark(&e2));
    plonk_lookup_multiplicity_root<F>(tr, h_roots, ch);
    {
        Owned h;
        const void *ip[kPlonkHelpersIn];
        void *op[kPlonkHelpersOut];
        for (int j = 0; j < kPlonkHelpersIn - 1; j++) ip[j] = given[kHelpersPlace[j]];
        ip[PH_M] = hc.m->coeffs[0]->dptr;
        for (int j = 0; j < kPlonkHelpersOut; j++) {
            ZK_TRY(table_alloc_pooled(wit->field, n, &h.t[j]));
            op[j] = h.t[j]->dptr;
        }
        ZK_TRY(launch_helpers<F>(ip, op, n, ch.beta, ch.gamma));
        ZK_TRY(ev.mark(&e3));
        ZK_TRY(fri_commit_columns_adopt(h.t, kPlonkHelpersOut, wit->b, coset, &hc.h));
        h.release();
    }
    memcpy(h_roots + 32, hc.h->root, 32);
    ZK_TRY(ev.mark(&e4));
    plonk_lookup_columns_helpers<F>(tr, h_roots + 32, d, ch);
    if (chal_out) {
        store_host<F>(chal_out, ch.beta);
        store_host<F>(chal_out + W, ch.gamma);
        store_host<F>(chal_out + 2 * W, ch.alpha);
        store_host<F>(chal_out + 3 * W, ch.mu);
        memcpy(chal_out + 4 * W, ch.tau.data(), ch.tau.size() * 8);
    }

    const void *opened[K];
    for (int j = 0; j < K; j++) opened[j] = j < G ? given[j] : j == G ? hc.m->coeffs[0]->dptr : hc.h->coeffs[j - G - 1]->dptr;
    ZK_TRY(plonk_lookup_rounds<F>(opened, d, ch, tr, round_polys, challenges, z, ev, &e4, &st.ms_eq, &st.ms_rounds));
    st.rounds = d;
    st.ms_multiplicities = ev.ms(e0, e1);
    st.ms_fractions = ev.ms(e2, e3);
    st.ms_commit = ev.ms(e1, e2) + ev.ms(e3, e4);
    return ZK_OK;
}

}  // namespace

extern "C" {

uint32_t zk_plonk_lookup_helpers_batch(void) { return kPlonkHelpersBatch; }

int zk_plonk_lookup_helpers(const zk_table *const tables[11], const uint64_t *beta, const uint64_t *gamma, zk_table *H[4]) {
    if (!beta || !gamma || !H || !tables) return ZK_E_ARG;
    {                                                        // the four handles are written: they may not lie in the array that is read
        const char *a = (const char *)tables, *b = (const char *)H;
        if (a < b + kPlonkHelpersOut * sizeof(zk_table *) && b < a + kPlonkHelpersIn * sizeof(zk_table *)) return ZK_E_ARG;
    }
    ZK_TRY(check_tables(tables, kPlonkHelpersIn, 2));
    const int field = tables[0]->field;
    if (tables[0]->len > ((size_t)1 << kLookupMaxLog)) return ZK_E_ARG;
    if (!all_reduced(field, beta, 1) || !all_reduced(field, gamma, 1)) return ZK_E_ARG;
    ZK_TRY(require_device());
    FRI_DISPATCH(field, return helpers_once<F>(tables, beta, gamma, H));
    return ZK_OK;
}

int zk_plonk_lookup_sizes_columns(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, size_t *nround, size_t *nhroots, size_t *nroots, size_t *nfinal,
                                  size_t *nvalues, size_t *path_bytes, size_t *nopen_round) {
    if (d > kLookupMaxLog) return ZK_E_ARG;
    ZK_TRY(zk_fri_ml_sizes_columns(kPlonkColumnsWidths, kPlonkColumnsCommits, d, log_blowup, log_final, nqueries, nroots, nfinal, nvalues, path_bytes, nopen_round));
    if (nround) *nround = (size_t)kPlonkNodes * d;
    if (nhroots) *nhroots = 2;
    return ZK_OK;
}

int zk_plonk_lookup_prove_columns(const zk_fri_columns *witness, const zk_fri_columns *circuit, const uint64_t *public_inputs, uint32_t npublic, uint32_t log_final,
                                  uint32_t nqueries, uint32_t grinding_bits, zk_transcript *t, uint8_t *h_roots, uint64_t *chal_out, uint64_t *round_polys,
                                  uint64_t *challenges, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *open_round_polys, uint8_t *roots, uint64_t *final_table,
                                  uint64_t *open_challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths, uint64_t *pow_nonce) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!witness || !circuit || !h_roots || !round_polys || !challenges) return ZK_E_ARG;
    if (witness->k != kPlonkColumnsWitness || circuit->k != kPlonkColumnsCircuit) return ZK_E_ARG;
    if (witness->d < 1 || witness->d > kLookupMaxLog) return ZK_E_ARG;   // what sizes the point below, and the lookup's 32-bit counts
    // the point and the two helper commitments do not exist yet: the columns opener's statuses are taken on the two given, on stand-ins of the
    // witness's shape with one and four columns, and on a point of zeros, before the transcript moves
    zk_fri_columns stand_m = *witness, stand_h = *witness;
    stand_m.k = 1;
    stand_h.k = kPlonkColumnsHelpers;
    const zk_fri_columns *shape[kPlonkColumnsCommits] = {witness, circuit, &stand_m, &stand_h};
    std::vector<uint64_t> z((size_t)witness->d * 4, 0);
    ZK_TRY(fri_ml_open_columns_check(shape, kPlonkColumnsCommits, z.data(), 1, log_final, nqueries, ys_out, open_round_polys, roots, final_table, query_values, query_paths,
                                     grinding_bits, pow_nonce));
    if (!plonk_public_shape_ok(public_inputs, npublic, witness->d) || !all_reduced(witness->field, public_inputs, npublic)) return ZK_E_ARG;
    zk_transcript own;
    zk_transcript *tt = t ? t : &own;
    zk_plonk_lookup_stats st{};
    HelperColumns hc;
    FRI_DISPATCH(witness->field, ZK_TRY((prove_steps<F>(witness, circuit, public_inputs, npublic, tt->t, hc, h_roots, chal_out, round_polys, challenges, z.data(), st))));
    const zk_fri_columns *all[kPlonkColumnsCommits] = {witness, circuit, hc.m, hc.h};
    const int opened = zk_fri_ml_open_columns_pow(all, kPlonkColumnsCommits, z.data(), 1, log_final, nqueries, grinding_bits, tt, ys_out, gamma_out, open_round_polys, roots,
                                                  final_table, open_challenges, query_indices, query_values, query_paths, pow_nonce);
    return prove_finish(opened, t0, st, g_stats);
}

int zk_plonk_lookup_verify_columns(int field, const uint8_t *witness_root, const uint8_t *circuit_root, const uint64_t *public_inputs, uint32_t npublic, uint32_t d,
                                   uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset, zk_transcript *t, const uint8_t *h_roots,
                                   const uint64_t *round_polys, const uint64_t *ys, const uint64_t *open_round_polys, const uint8_t *roots, const uint64_t *final_table,
                                   const uint64_t *query_values, const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce, int *ok) {
    const bool have_all = witness_root && circuit_root && h_roots && round_polys && ys && open_round_polys && roots && final_table && query_values && query_paths && ok;
    ZK_TRY(verify_check(field, d, log_blowup, coset, grinding_bits, have_all, [&]() -> int {
        if (d > kLookupMaxLog) return ZK_E_ARG;
        return zk_fri_ml_sizes_columns(kPlonkColumnsWidths, kPlonkColumnsCommits, d, log_blowup, log_final, nqueries, nullptr, nullptr, nullptr, nullptr, nullptr);
    }));
    if (!plonk_public_shape_ok(public_inputs, npublic, d)) return ZK_E_ARG;
    uint8_t all[32 * kPlonkColumnsCommits];
    memcpy(all, witness_root, 32);
    memcpy(all + 32, circuit_root, 32);
    memcpy(all + 64, h_roots, 64);
    zk_transcript work;
    if (t) work.t = t->t;
    std::vector<uint64_t> z((size_t)d * 4);
    bool good = false;
    FRI_DISPATCH(field, (plonk_lookup_columns_replay<F>(work.t, witness_root, circuit_root, d, public_inputs, npublic, h_roots, round_polys, ys, z.data(), &good)));
    int open_ok = 0;
    ZK_TRY(zk_fri_ml_verify_columns_pow(field, all, kPlonkColumnsWidths, kPlonkColumnsCommits, d, log_blowup, log_final, nqueries, grinding_bits, coset, z.data(), 1, ys,
                                        &work, open_round_polys, roots, final_table, query_values, query_paths, pow_nonce, &open_ok));
    if (t) t->t = work.t;
    *ok = good && open_ok ? 1 : 0;
    return ZK_OK;
}

int zk_plonk_lookup_columns_last_stats(zk_plonk_lookup_stats *out) {
    if (!out) return ZK_E_ARG;
    *out = g_stats;
    return ZK_OK;
}

}  // extern "C"
