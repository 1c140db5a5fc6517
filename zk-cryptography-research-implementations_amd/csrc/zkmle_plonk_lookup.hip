// zkmle_plonk_lookup.hip -- C ABI of the Plonk proof with lookup rows over FRI commitments (plonk_lookup.cuh, plonk_lookup_host.h): one round pass
// on its own, the prover (the multiplicities and their commitment, the wiring's three helper tables and the lookup's one with their commitments,
// ONE sumcheck of the gate, the wiring and the lookup on the twenty coefficient tables and E whose claimed sum carries the public inputs, then
// zk_fri_ml_open_batch_wide_pow of the twenty commitments at the point the rounds leave, on the same transcript) and its host verifier.  The
// rounds are plonk_lookup_driver.cuh's on zerocheck_driver.cuh's round loop, whose hook's pass and shells' shared checks it uses too.
// Extension: the protocol is defined in include/zkmle.h "Plonk with lookups: gate, wiring, public inputs and lookup rows in one sumcheck".
#include <string.h>

#include <chrono>
#include <vector>

#include "lookup_driver.cuh"
#include "plonk_lookup.cuh"
#include "plonk_lookup_driver.cuh"
#include "plonk_lookup_host.h"

using namespace zk;
using namespace zk::host;

// plonk_lookup_driver.cuh's launcher.  Sums (device, 7 elements) of a pass over q pairs whose id tables are c_l + 2^l x + j 2^d.  Launches only.
template <class F> int zk::host::plonk_lookup_launch_round(bool fold, const PlonkLookupTables &t, size_t q, const Fe<F> &r, const WiringChallenges<F> &ch, const Fe<F> &id_base, unsigned log_step,
                                    unsigned d, void *partials, void *sums) {
    const int grid = reduce_grid_for(q);
    PlonkLookupConsts<F> c;
    c.beta = ch.beta;
    c.gamma = ch.gamma;
    c.alpha = ch.alpha;
    c.alpha2 = fe_mul<F>(ch.alpha, ch.alpha);
    c.alpha3 = fe_mul<F>(ch.alpha, c.alpha2);
    c.gamma2 = fe_mul<F>(ch.gamma, ch.gamma);
    c.mu = ch.mu;
    c.gstep = fe_mul<F>(ch.gamma, fe_from_u64<F>((uint64_t)1 << log_step));
    c.gwire = fe_mul<F>(ch.gamma, fe_from_u64<F>((uint64_t)1 << d));
    c.gid0 = fe_mul<F>(ch.gamma, id_base);
    c.gnext = fe_sub<F>(fe_mul<F>(fe_dbl<F>(c.gstep), fe_from_u64<F>((uint64_t)grid * kBlock)), fe_dbl<F>(c.gwire));
    if (fold) plonk_lookup_round_kernel<F, true><<<grid, kBlock, 0, cur_stream()>>>(t, q, r, c, partials);
    else plonk_lookup_round_kernel<F, false><<<grid, kBlock, 0, cur_stream()>>>(t, q, r, c, partials);
    ZK_HIP(hipGetLastError());
    finish_sums_kernel<F><<<1, kBlock, 0, cur_stream()>>>(partials, (size_t)grid, kWiringSums, sums);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template int zk::host::plonk_lookup_launch_round<Fr381>(bool, const PlonkLookupTables &, size_t, const Fe<Fr381> &, const WiringChallenges<Fr381> &, const Fe<Fr381> &, unsigned, unsigned, void *, void *);
template int zk::host::plonk_lookup_launch_round<Bn254Fr>(bool, const PlonkLookupTables &, size_t, const Fe<Bn254Fr> &, const WiringChallenges<Bn254Fr> &, const Fe<Bn254Fr> &, unsigned, unsigned, void *, void *);

namespace {

thread_local zk_plonk_lookup_stats g_stats{};

constexpr int kTables = kPlonkLookupTables;                  // the twenty opened and E
static_assert(kTables == kPlonkLookupOpened + 1, "the pass folds the opened tables and E");

// the prover's five helper commitments (M, H0, H1, H2, HL): freed with the call
struct HelperCommits {
    zk_fri_commitment *cm[kPlonkLookupHelpers] = {};
    ~HelperCommits() { for (zk_fri_commitment *c : cm) zk_fri_commitment_free(c); }
};

template <class F> int hook_round(const zk_table *const *in, const WiringChallenges<F> &ch, const uint64_t *id_base, unsigned log_step, const uint64_t *r, zk_table **outs,
                                  uint64_t *gout) {
    const Fe<F> id0 = load_host<F>(id_base);
    const auto launch = [&](bool fold, const void *const *ip, void *out0, size_t ostride, size_t q, const Fe<F> &rr, unsigned, void *partials, void *sums) {
        return plonk_lookup_pass<F>(fold, ip, out0, ostride, q, rr, ch, id0, log_step, ilog2(2 * q) + log_step, partials, sums);
    };
    return round_once<F, kTables, kWiringSums, kPlonkNodes>(in, r, outs, gout, launch, [&](const Fe<F> *S, Fe<F> *g) { wiring_message<F>(S, ch.mu, g); });
}

// steps 1 to 9 on `tr`: the statement, M, the four helper tables and the five commitments (hc: M, H0, H1, H2, HL; h_roots), then E_0 and the d
// rounds by plonk_lookup_driver.cuh; z (d elements) = the point the opening is made at.  One host synchronisation for the miss count beside the rounds'.
template <class F> int prove_steps(const zk_fri_commitment *const *cms, const uint64_t *pub, uint32_t npublic, Transcript &tr, HelperCommits &hc, uint8_t *h_roots,
                                   uint64_t *chal_out, uint64_t *round_polys, uint64_t *challenges, uint64_t *z, zk_plonk_lookup_stats &st) {
    constexpr int W = F::N / 2, K = kPlonkLookupOpened, G = kPlonkLookupGiven;
    const zk_fri_commitment *c0 = cms[0];
    const unsigned d = c0->d;
    const size_t n = (size_t)1 << d;
    uint8_t roots[32 * G];
    for (int j = 0; j < G; j++) memcpy(roots + 32 * j, cms[j]->root, 32);
    // the lookup's eight in its own order: A, B, C, qK, T0, T1, T2, then M
    const void *lk[kLookupGiven + 1];
    for (int j = 0; j < kLookupGiven; j++) lk[j] = cms[kPlonkLookupLookupPlace[j]]->coeffs->dptr;
    WiringChallenges<F> ch;
    plonk_lookup_statement<F>(tr, roots, d, pub, npublic);

    Events ev;
    size_t e0, e1, e2, e3, e4;
    ZK_TRY(ev.mark(&e0));
    {
        TableHolder th;
        zk_table *M = nullptr, *H[kWiringWires + 1];
        ZK_TRY(th.alloc(c0->field, n, &M));
        ZK_TRY(multiplicities_into<F>(lk, n, M->dptr, &st.misses));
        ZK_TRY(ev.mark(&e1));
        ZK_TRY(commit_like(c0, M, &hc.cm[0]));
        memcpy(h_roots, hc.cm[0]->root, 32);
        ZK_TRY(ev.mark(&e2));
        plonk_lookup_multiplicity_root<F>(tr, h_roots, ch);
        lk[kLookupGiven] = hc.cm[0]->coeffs->dptr;
        for (int j = 0; j < kWiringWires; j++) {
            ZK_TRY(th.alloc(c0->field, n, &H[j]));
            ZK_TRY(launch_fractions<F>(cms[j]->coeffs->dptr, cms[PLONK_S + j]->coeffs->dptr, H[j]->dptr, n, (uint64_t)j * n, ch.beta, ch.gamma));
        }
        ZK_TRY(th.alloc(c0->field, n, &H[kWiringWires]));
        ZK_TRY(launch_fractions_lookup<F>(lk, n, H[kWiringWires]->dptr, ch.beta, ch.gamma));
        ZK_TRY(ev.mark(&e3));
        for (int j = 0; j <= kWiringWires; j++) {
            ZK_TRY(commit_like(c0, H[j], &hc.cm[1 + j]));
            memcpy(h_roots + 32 * (1 + j), hc.cm[1 + j]->root, 32);
        }
        ZK_TRY(ev.mark(&e4));
    }
    plonk_lookup_helpers<F>(tr, h_roots + 32, d, ch);
    if (chal_out) {
        store_host<F>(chal_out, ch.beta);
        store_host<F>(chal_out + W, ch.gamma);
        store_host<F>(chal_out + 2 * W, ch.alpha);
        store_host<F>(chal_out + 3 * W, ch.mu);
        memcpy(chal_out + 4 * W, ch.tau.data(), ch.tau.size() * 8);
    }

    const void *opened[K];
    for (int j = 0; j < K; j++) opened[j] = (j < G ? cms[j] : hc.cm[j - G])->coeffs->dptr;
    ZK_TRY(plonk_lookup_rounds<F>(opened, d, ch, tr, round_polys, challenges, z, ev, &e4, &st.ms_eq, &st.ms_rounds));
    st.rounds = d;
    st.ms_multiplicities = ev.ms(e0, e1);
    st.ms_fractions = ev.ms(e2, e3);
    st.ms_commit = ev.ms(e1, e2) + ev.ms(e3, e4);
    return ZK_OK;
}

}  // namespace

extern "C" {

int zk_plonk_lookup_round(const zk_table *const tables[21], const uint64_t *beta, const uint64_t *gamma, const uint64_t *alpha, const uint64_t *mu, const uint64_t *id_base,
                          uint32_t log_step, const uint64_t *r, zk_table **outs, uint64_t *g5) {
    ZK_TRY(wiring_round_check(tables, kTables, beta, gamma, alpha, mu, id_base, log_step, r, outs, g5));
    FRI_DISPATCH(tables[0]->field, return hook_round<F>(tables, wiring_challenges<F>(beta, gamma, alpha, mu), id_base, log_step, r, outs, g5));
    return ZK_OK;
}

int zk_plonk_lookup_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group, size_t *nround, size_t *nhroots,
                          size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nopen_round) {
    ZK_TRY(zk_fri_ml_sizes_batch_wide(kPlonkLookupOpened, d, log_blowup, log_final, nqueries, log_arity, log_group, nroots, nfinal, nvalues, path_bytes, nopen_round));
    if (nround) *nround = (size_t)kPlonkNodes * d;
    if (nhroots) *nhroots = kPlonkLookupHelpers;
    return ZK_OK;
}

int zk_plonk_lookup_prove(const zk_fri_commitment *const cms[15], const uint64_t *public_inputs, uint32_t npublic, uint32_t log_final, uint32_t nqueries,
                          uint32_t log_arity, uint32_t grinding_bits, zk_transcript *t, uint8_t *h_roots, uint64_t *chal_out, uint64_t *round_polys, uint64_t *challenges,
                          uint64_t *ys_out, uint64_t *gamma_out, uint64_t *open_round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *open_challenges,
                          uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths, uint64_t *pow_nonce) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!cms) return ZK_E_ARG;
    for (int j = 0; j < kPlonkLookupGiven; j++)
        if (!cms[j]) return ZK_E_ARG;
    if (!h_roots || !round_polys || !challenges) return ZK_E_ARG;
    if (cms[0]->d < 1 || cms[0]->d > kLookupMaxLog) return ZK_E_ARG;   // what sizes the point below, and the lookup's 32-bit counts
    // the point and the helper commitments do not exist yet: the wide opener's statuses are taken on the fifteen and a stand-in of zeros, before
    // the transcript moves (the helpers get the shape of the fifteen, and twenty is within the wide opener's count)
    std::vector<uint64_t> z((size_t)cms[0]->d * 4, 0);
    ZK_TRY(fri_ml_open_batch_check(cms, kPlonkLookupGiven, z.data(), 1, log_final, nqueries, log_arity, ys_out, open_round_polys, roots, final_table, query_values,
                                   query_paths, grinding_bits, pow_nonce));
    if (!plonk_public_shape_ok(public_inputs, npublic, cms[0]->d) || !all_reduced(cms[0]->field, public_inputs, npublic)) return ZK_E_ARG;
    zk_transcript own;
    zk_transcript *tt = t ? t : &own;
    zk_plonk_lookup_stats st{};
    HelperCommits hc;
    FRI_DISPATCH(cms[0]->field, ZK_TRY((prove_steps<F>(cms, public_inputs, npublic, tt->t, hc, h_roots, chal_out, round_polys, challenges, z.data(), st))));
    const zk_fri_commitment *all[kPlonkLookupOpened];
    for (int j = 0; j < kPlonkLookupOpened; j++) all[j] = j < kPlonkLookupGiven ? cms[j] : hc.cm[j - kPlonkLookupGiven];
    const int opened = zk_fri_ml_open_batch_wide_pow(all, kPlonkLookupOpened, z.data(), 1, log_final, nqueries, log_arity, tt, ys_out, gamma_out, open_round_polys, roots,
                                                     final_table, open_challenges, query_indices, query_values, query_paths, grinding_bits, pow_nonce);
    return prove_finish(opened, t0, st, g_stats);
}

int zk_plonk_lookup_verify(int field, const uint8_t *roots_of_fifteen, const uint64_t *public_inputs, uint32_t npublic, uint32_t d, uint32_t log_blowup,
                           uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group, const uint64_t *coset, zk_transcript *t, const uint8_t *h_roots,
                           const uint64_t *round_polys, const uint64_t *ys, const uint64_t *open_round_polys, const uint8_t *roots, const uint64_t *final_table,
                           const uint64_t *query_values, const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce, int *ok) {
    const bool have_all = roots_of_fifteen && h_roots && round_polys && ys && open_round_polys && roots && final_table && query_values && query_paths && ok;
    ZK_TRY(verify_check(field, d, log_blowup, coset, grinding_bits, have_all, [&]() -> int {
        ZK_TRY(zk_fri_ml_sizes_batch_wide(kPlonkLookupOpened, d, log_blowup, log_final, nqueries, log_arity, log_group, nullptr, nullptr, nullptr, nullptr, nullptr));
        return d > kLookupMaxLog ? ZK_E_ARG : ZK_OK;
    }));
    if (!plonk_public_shape_ok(public_inputs, npublic, d)) return ZK_E_ARG;
    uint8_t all[32 * kPlonkLookupOpened];
    memcpy(all, roots_of_fifteen, 32 * kPlonkLookupGiven);
    memcpy(all + 32 * kPlonkLookupGiven, h_roots, 32 * kPlonkLookupHelpers);
    zk_transcript work;
    if (t) work.t = t->t;
    std::vector<uint64_t> z((size_t)d * 4);
    bool good = false;
    FRI_DISPATCH(field, (plonk_lookup_replay<F>(work.t, roots_of_fifteen, d, public_inputs, npublic, h_roots, round_polys, ys, z.data(), &good)));
    int open_ok = 0;
    ZK_TRY(zk_fri_ml_verify_batch_wide_pow(field, all, kPlonkLookupOpened, d, log_blowup, log_final, nqueries, log_arity, log_group, coset, z.data(), 1, ys, &work,
                                           open_round_polys, roots, final_table, query_values, query_paths, grinding_bits, pow_nonce, &open_ok));
    if (t) t->t = work.t;
    *ok = good && open_ok ? 1 : 0;
    return ZK_OK;
}

int zk_plonk_lookup_last_stats(zk_plonk_lookup_stats *out) {
    if (!out) return ZK_E_ARG;
    *out = g_stats;
    return ZK_OK;
}

}  // extern "C"
