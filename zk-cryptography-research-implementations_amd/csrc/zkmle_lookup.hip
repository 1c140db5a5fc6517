// zkmle_lookup.hip -- C ABI of the lookup argument over FRI commitments (lookup.cuh, lookup_host.h): the multiplicity table, the helper table
// and one round pass on their own, the prover (the multiplicities and their commitment, the helper table and its commitment, the sumcheck of
// the logarithmic-derivative relation on the nine coefficient tables and E, then zk_fri_ml_open_batch_pow of the nine commitments at the
// point the rounds leave, on the same transcript) and its host verifier.  The round loop, the hook's pass, the hooks' table checks and the shells'
// shared checks are zerocheck_driver.cuh's, by wiring_driver.cuh.  Extension: the protocol is defined in include/zkmle.h "Lookup: rows
// of a committed table".
#include <string.h>

#include <chrono>
#include <vector>

#include "lookup.cuh"
#include "lookup_driver.cuh"
#include "lookup_host.h"
#include "wiring_driver.cuh"

using namespace zk;
using namespace zk::host;

namespace {

thread_local zk_lookup_stats g_lookup_stats{};

constexpr int kTables = LOOKUP_TABLES;                       // A, B, C, qK, T0, T1, T2, M, H, E
// sums (device, 7 elements) of a pass over q pairs; the ten folded to out0 + j ostride.  Launches only.
template <class F>
int launch_round(bool fold, const void *const *in, void *out0, size_t ostride, size_t q, const Fe<F> &r, const LookupChallenges<F> &ch, void *partials, void *sums) {
    LookupTables t{};
    for (int j = 0; j < kTables; j++) t.in[j] = in[j];
    t.out0 = out0;
    t.ostride = ostride;
    const int grid = reduce_grid_for(q);
    LookupConsts<F> c;
    c.beta = ch.beta;
    c.gamma = ch.gamma;
    c.gamma2 = fe_mul<F>(ch.gamma, ch.gamma);
    if (fold) lookup_round_kernel<F, true><<<grid, kBlock, 0, cur_stream()>>>(t, q, r, c, partials);
    else lookup_round_kernel<F, false><<<grid, kBlock, 0, cur_stream()>>>(t, q, r, c, partials);
    ZK_HIP(hipGetLastError());
    finish_sums_kernel<F><<<1, kBlock, 0, cur_stream()>>>(partials, (size_t)grid, kWiringSums, sums);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class F> int multiplicities_once(const zk_table *const *in, zk_table **M, uint64_t *misses) {
    zk_table *m = nullptr;
    ZK_TRY(zk_table_alloc(in[0]->field, in[0]->len, &m));
    const void *p[kLookupGiven];
    for (int j = 0; j < kLookupGiven; j++) p[j] = in[j]->dptr;
    uint64_t lost = 0;
    const int rc = multiplicities_into<F>(p, in[0]->len, m->dptr, &lost);
    if (rc != ZK_OK) { zk_table_free(m); return rc; }
    *M = m;
    *misses = lost;
    return ZK_OK;
}

template <class F> int fractions_once(const zk_table *const *in, const uint64_t *beta, const uint64_t *gamma, zk_table **H) {
    zk_table *h = nullptr;
    ZK_TRY(zk_table_alloc(in[0]->field, in[0]->len, &h));
    const void *p[kLookupGiven + 1];
    for (int j = 0; j <= kLookupGiven; j++) p[j] = in[j]->dptr;
    int rc = launch_fractions_lookup<F>(p, in[0]->len, h->dptr, load_host<F>(beta), load_host<F>(gamma));
    if (rc == ZK_OK && hipStreamSynchronize(cur_stream()) != hipSuccess) rc = ZK_E_HIP;
    if (rc != ZK_OK) { zk_table_free(h); return rc; }
    *H = h;
    return ZK_OK;
}

// zerocheck_driver.cuh's launch and message with the lookup's challenges
template <class F> auto launch_with(const LookupChallenges<F> &ch) {
    return [&ch](bool fold, const void *const *in, void *out0, size_t ostride, size_t q, const Fe<F> &r, unsigned, void *partials, void *sums) {
        return launch_round<F>(fold, in, out0, ostride, q, r, ch, partials, sums);
    };
}
template <class F> auto message_with(const LookupChallenges<F> &ch) {
    return [&ch](const Fe<F> *S, Fe<F> *g) { wiring_message<F>(S, ch.mu, g); };
}

// steps 1 to 7 on `tr`: the statement, M and H with their commitments (hc.cm[0], hc.cm[1]; h_roots), then E_0 and the d rounds by
// zerocheck_driver.cuh; z (d elements) = the point the opening is made at.  One host synchronisation for the miss count beside the rounds'.
template <class F> int prove_steps(const zk_fri_commitment *const *cms, Transcript &tr, CommitHolder &hc, uint8_t *h_roots, uint64_t *chal_out, uint64_t *round_polys,
                                   uint64_t *challenges, uint64_t *z, zk_lookup_stats &st) {
    constexpr int W = F::N / 2, K = kLookupOpened;
    const zk_fri_commitment *c0 = cms[0];
    const unsigned d = c0->d;
    const size_t n = (size_t)1 << d;
    uint8_t roots[32 * kLookupGiven];
    const void *in[kLookupGiven + 1];
    for (int j = 0; j < kLookupGiven; j++) {
        memcpy(roots + 32 * j, cms[j]->root, 32);
        in[j] = cms[j]->coeffs->dptr;
    }
    lookup_statement(tr, roots, d);
    LookupChallenges<F> ch;

    Events ev;
    size_t e0, e1, e2, e3, e4;
    ZK_TRY(ev.mark(&e0));
    {
        TableHolder th;
        zk_table *M = nullptr, *H = nullptr;
        ZK_TRY(th.alloc(c0->field, n, &M));
        ZK_TRY(multiplicities_into<F>(in, n, M->dptr, &st.misses));
        ZK_TRY(ev.mark(&e1));
        ZK_TRY(commit_like(c0, M, &hc.cm[0]));
        memcpy(h_roots, hc.cm[0]->root, 32);
        ZK_TRY(ev.mark(&e2));
        lookup_multiplicity_root<F>(tr, h_roots, ch);
        in[kLookupGiven] = hc.cm[0]->coeffs->dptr;
        ZK_TRY(th.alloc(c0->field, n, &H));
        ZK_TRY(launch_fractions_lookup<F>(in, n, H->dptr, ch.beta, ch.gamma));
        ZK_TRY(ev.mark(&e3));
        ZK_TRY(commit_like(c0, H, &hc.cm[1]));
        memcpy(h_roots + 32, hc.cm[1]->root, 32);
        ZK_TRY(ev.mark(&e4));
    }
    lookup_helper_root<F>(tr, h_roots + 32, d, ch);
    if (chal_out) {
        store_host<F>(chal_out, ch.beta);
        store_host<F>(chal_out + W, ch.gamma);
        store_host<F>(chal_out + 2 * W, ch.mu);
        memcpy(chal_out + 3 * W, ch.tau.data(), ch.tau.size() * 8);
    }

    const void *opened[K];
    for (int j = 0; j < K; j++) opened[j] = (j < kLookupGiven ? cms[j] : hc.cm[j - kLookupGiven])->coeffs->dptr;
    ZK_TRY((prove_rounds<F, kTables, kWiringSums, kWiringNodes>(opened, d, ch.tau.data(), tr, launch_with<F>(ch), message_with<F>(ch), round_polys, challenges, z, ev, &e4,
                                                                &st.ms_eq, &st.ms_rounds)));
    st.rounds = d;
    st.ms_multiplicities = ev.ms(e0, e1);
    st.ms_fractions = ev.ms(e2, e3);
    st.ms_commit = ev.ms(e1, e2) + ev.ms(e3, e4);
    return ZK_OK;
}

}  // namespace

extern "C" {

int zk_lookup_multiplicities(const zk_table *const tables[7], zk_table **M, uint64_t *misses) {
    if (!M || !misses) return ZK_E_ARG;
    ZK_TRY(check_tables(tables, kLookupGiven, 2));
    if (tables[0]->len > ((size_t)1 << kLookupMaxLog)) return ZK_E_ARG;
    ZK_TRY(require_device());
    FRI_DISPATCH(tables[0]->field, return multiplicities_once<F>(tables, M, misses));
    return ZK_OK;
}

int zk_lookup_hash_slots(const zk_table *const T[3], uint32_t *slots) {
    if (!slots) return ZK_E_ARG;
    ZK_TRY(check_tables(T, 3, 2));
    if (T[0]->len > ((size_t)1 << kLookupMaxLog)) return ZK_E_ARG;
    ZK_TRY(require_device());
    const void *p[3] = {T[0]->dptr, T[1]->dptr, T[2]->dptr};
    FRI_DISPATCH(T[0]->field, return hash_slots_into<F>(p, T[0]->len, slots));
    return ZK_OK;
}

int zk_lookup_fractions(const zk_table *const tables[8], const uint64_t *beta, const uint64_t *gamma, zk_table **H) {
    if (!beta || !gamma || !H) return ZK_E_ARG;
    ZK_TRY(check_tables(tables, kLookupGiven + 1, 2));
    if (!all_reduced(tables[0]->field, beta, 1) || !all_reduced(tables[0]->field, gamma, 1)) return ZK_E_ARG;
    ZK_TRY(require_device());
    FRI_DISPATCH(tables[0]->field, return fractions_once<F>(tables, beta, gamma, H));
    return ZK_OK;
}

int zk_lookup_round(const zk_table *const tables[10], const uint64_t *beta, const uint64_t *gamma, const uint64_t *mu, const uint64_t *r, zk_table **outs, uint64_t *g5) {
    if (!beta || !gamma || !mu || !g5 || (r && !outs)) return ZK_E_ARG;
    ZK_TRY(check_tables(tables, kTables, r ? 4 : 2));
    const int field = tables[0]->field;
    if (r && !all_reduced(field, r, 1)) return ZK_E_ARG;
    for (const uint64_t *e : {beta, gamma, mu})
        if (!all_reduced(field, e, 1)) return ZK_E_ARG;
    ZK_TRY(require_device());
    FRI_DISPATCH(field, {
        LookupChallenges<F> ch;
        ch.beta = load_host<F>(beta);
        ch.gamma = load_host<F>(gamma);
        ch.mu = load_host<F>(mu);
        return round_once<F, kTables, kWiringSums, kWiringNodes>(tables, r, outs, g5, launch_with<F>(ch), message_with<F>(ch));
    });
    return ZK_OK;
}

int zk_lookup_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group, size_t *nround, size_t *nhroots,
                    size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nopen_round) {
    ZK_TRY(zk_fri_ml_sizes_batch(kLookupOpened, d, log_blowup, log_final, nqueries, log_arity, log_group, nroots, nfinal, nvalues, path_bytes, nopen_round));
    if (nround) *nround = (size_t)kWiringNodes * d;
    if (nhroots) *nhroots = kLookupHelpers;
    return ZK_OK;
}

int zk_lookup_prove(const zk_fri_commitment *const cms[7], uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t grinding_bits, zk_transcript *t,
                    uint8_t *h_roots, uint64_t *chal_out, uint64_t *round_polys, uint64_t *challenges, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *open_round_polys,
                    uint8_t *roots, uint64_t *final_table, uint64_t *open_challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths,
                    uint64_t *pow_nonce) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!cms) return ZK_E_ARG;
    for (int j = 0; j < kLookupGiven; j++)
        if (!cms[j]) return ZK_E_ARG;
    if (!h_roots || !round_polys || !challenges) return ZK_E_ARG;
    if (cms[0]->d < 1 || cms[0]->d > kLookupMaxLog) return ZK_E_ARG;   // what sizes the point below, and the 32-bit counts; no commitment is made outside it
    // the point and the helper commitments do not exist yet: the opener's statuses are taken on the seven and a stand-in of zeros, before the
    // transcript moves (the helpers get the shape of the seven, and nine is within the opener's count)
    std::vector<uint64_t> z((size_t)cms[0]->d * 4, 0);
    ZK_TRY(fri_ml_open_batch_check(cms, kLookupGiven, z.data(), 1, log_final, nqueries, log_arity, ys_out, open_round_polys, roots, final_table, query_values, query_paths,
                                   grinding_bits, pow_nonce));
    zk_transcript own;
    zk_transcript *tt = t ? t : &own;
    zk_lookup_stats st{};
    CommitHolder hc;
    FRI_DISPATCH(cms[0]->field, ZK_TRY((prove_steps<F>(cms, tt->t, hc, h_roots, chal_out, round_polys, challenges, z.data(), st))));
    const zk_fri_commitment *all[kLookupOpened];
    for (int j = 0; j < kLookupOpened; j++) all[j] = j < kLookupGiven ? cms[j] : hc.cm[j - kLookupGiven];
    const int opened = zk_fri_ml_open_batch_pow(all, kLookupOpened, z.data(), 1, log_final, nqueries, log_arity, tt, ys_out, gamma_out, open_round_polys, roots, final_table,
                                                open_challenges, query_indices, query_values, query_paths, grinding_bits, pow_nonce);
    return prove_finish(opened, t0, st, g_lookup_stats);
}

int zk_lookup_verify(int field, const uint8_t *roots_of_seven, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group,
                     const uint64_t *coset, zk_transcript *t, const uint8_t *h_roots, const uint64_t *round_polys, const uint64_t *ys, const uint64_t *open_round_polys,
                     const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values, const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce,
                     int *ok) {
    const bool have_all = roots_of_seven && h_roots && round_polys && ys && open_round_polys && roots && final_table && query_values && query_paths && ok;
    ZK_TRY(verify_check(field, d, log_blowup, coset, grinding_bits, have_all, [&] {
        return zk_fri_ml_sizes_batch(kLookupOpened, d, log_blowup, log_final, nqueries, log_arity, log_group, nullptr, nullptr, nullptr, nullptr, nullptr);
    }));
    uint8_t nine[32 * kLookupOpened];
    memcpy(nine, roots_of_seven, 32 * kLookupGiven);
    memcpy(nine + 32 * kLookupGiven, h_roots, 32 * kLookupHelpers);
    zk_transcript work;
    if (t) work.t = t->t;
    std::vector<uint64_t> z((size_t)d * 4);
    bool good = false;
    FRI_DISPATCH(field, (lookup_replay<F>(work.t, roots_of_seven, d, h_roots, round_polys, ys, z.data(), &good)));
    int open_ok = 0;
    ZK_TRY(zk_fri_ml_verify_batch_pow(field, nine, kLookupOpened, d, log_blowup, log_final, nqueries, log_arity, log_group, coset, z.data(), 1, ys, &work, open_round_polys,
                                      roots, final_table, query_values, query_paths, grinding_bits, pow_nonce, &open_ok));
    if (t) t->t = work.t;
    *ok = good && open_ok ? 1 : 0;
    return ZK_OK;
}

int zk_lookup_last_stats(zk_lookup_stats *out) {
    if (!out) return ZK_E_ARG;
    *out = g_lookup_stats;
    return ZK_OK;
}

}  // extern "C"
