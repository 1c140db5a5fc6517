// zkmle_wiring.hip -- C ABI of the permutation check over FRI commitments (wiring.cuh, wiring_host.h): the helper tables of one wire and one
// round pass on their own, the prover (the three helper tables and their commitments, the sumcheck of the logarithmic-derivative relation on
// the nine coefficient tables and E, then zk_fri_ml_open_batch_pow of the nine commitments at the point the rounds leave, on the same
// transcript) and its host verifier.  The round loop, the hook's pass and the shells' shared checks are zerocheck_driver.cuh's, by
// wiring_driver.cuh.  Extension: the protocol is defined in include/zkmle.h "Wiring: a permutation check over committed tables".
#include <string.h>

#include <chrono>
#include <vector>

#include "wiring_driver.cuh"

using namespace zk;
using namespace zk::host;

namespace {

thread_local zk_wiring_stats g_wiring_stats{};

constexpr int kTables = kWiringOpened + 1;                   // A, B, C, SA, SB, SC, H0, H1, H2, E

// sums (device, 7 elements) of a pass over q pairs whose id tables are c_l + 2^l x + j 2^d; the ten folded to out0 + j ostride.  Launches only.
template <class F> int launch_round(bool fold, const void *const *in, void *out0, size_t ostride, size_t q, const Fe<F> &r, const WiringChallenges<F> &ch, const Fe<F> &id_base,
                                    unsigned log_step, unsigned d, void *partials, void *sums) {
    WiringTables t{};
    for (int j = 0; j < kTables; j++) t.in[j] = in[j];
    t.out0 = out0;
    t.ostride = ostride;
    const int grid = reduce_grid_for(q);
    WiringConsts<F> c;
    c.beta = ch.beta;
    c.gamma = ch.gamma;
    c.alpha = ch.alpha;
    c.gstep = fe_mul<F>(ch.gamma, fe_from_u64<F>((uint64_t)1 << log_step));
    c.gwire = fe_mul<F>(ch.gamma, fe_from_u64<F>((uint64_t)1 << d));
    c.gid0 = fe_mul<F>(ch.gamma, id_base);
    c.gnext = fe_sub<F>(fe_mul<F>(fe_dbl<F>(c.gstep), fe_from_u64<F>((uint64_t)grid * kBlock)), fe_dbl<F>(c.gwire));
    if (fold) wiring_round_kernel<F, true><<<grid, kBlock, 0, cur_stream()>>>(t, q, r, c, partials);
    else wiring_round_kernel<F, false><<<grid, kBlock, 0, cur_stream()>>>(t, q, r, c, partials);
    ZK_HIP(hipGetLastError());
    finish_sums_kernel<F><<<1, kBlock, 0, cur_stream()>>>(partials, (size_t)grid, kWiringSums, sums);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class F> int fractions_once(const zk_table *W, const zk_table *S, uint64_t first, const uint64_t *beta, const uint64_t *gamma, zk_table **H) {
    zk_table *h = nullptr;
    ZK_TRY(zk_table_alloc(W->field, W->len, &h));
    int rc = launch_fractions<F>(W->dptr, S->dptr, h->dptr, W->len, first, load_host<F>(beta), load_host<F>(gamma));
    if (rc == ZK_OK && hipStreamSynchronize(cur_stream()) != hipSuccess) rc = ZK_E_HIP;
    if (rc != ZK_OK) { zk_table_free(h); return rc; }
    *H = h;
    return ZK_OK;
}

template <class F> int hook_round(const zk_table *const *in, const WiringChallenges<F> &ch, const uint64_t *id_base, unsigned log_step, const uint64_t *r, zk_table **outs,
                                  uint64_t *gout) {
    const Fe<F> id0 = load_host<F>(id_base);
    const auto launch = [&](bool fold, const void *const *ip, void *out0, size_t ostride, size_t q, const Fe<F> &rr, unsigned, void *partials, void *sums) {
        return launch_round<F>(fold, ip, out0, ostride, q, rr, ch, id0, log_step, ilog2(2 * q) + log_step, partials, sums);
    };
    return round_once<F, kTables, kWiringSums, kWiringNodes>(in, r, outs, gout, launch, [&](const Fe<F> *S, Fe<F> *g) { wiring_message<F>(S, ch.mu, g); });
}

// steps 1 to 6 on `tr`: the statement, the helper tables and their commitments (hc, h_roots), then E_0 and the d rounds by zerocheck_driver.cuh;
// z (d elements) = the point the opening is made at.
template <class F> int prove_steps(const zk_fri_commitment *const *cms, Transcript &tr, CommitHolder &hc, uint8_t *h_roots, uint64_t *chal_out, uint64_t *round_polys,
                                   uint64_t *challenges, uint64_t *z, zk_wiring_stats &st) {
    constexpr int W = F::N / 2, K = kWiringOpened;
    const zk_fri_commitment *c0 = cms[0];
    const unsigned d = c0->d;
    const size_t n = (size_t)1 << d;
    uint8_t roots[32 * kWiringGiven];
    for (int j = 0; j < kWiringGiven; j++) memcpy(roots + 32 * j, cms[j]->root, 32);
    WiringChallenges<F> ch;
    wiring_statement<F>(tr, roots, d, ch);

    Events ev;
    size_t e0, e1, e2;
    ZK_TRY(ev.mark(&e0));
    {
        TableHolder th;
        zk_table *H[kWiringWires];
        for (int j = 0; j < kWiringWires; j++) {
            ZK_TRY(th.alloc(c0->field, n, &H[j]));
            ZK_TRY(launch_fractions<F>(cms[j]->coeffs->dptr, cms[3 + j]->coeffs->dptr, H[j]->dptr, n, (uint64_t)j * n, ch.beta, ch.gamma));
        }
        ZK_TRY(ev.mark(&e1));
        for (int j = 0; j < kWiringWires; j++) {
            const uint64_t *coset = c0->has_coset ? c0->coset : nullptr;
            ZK_TRY(c0->log_group ? zk_fri_commit_grouped(H[j], c0->b, coset, c0->log_group, &hc.cm[j]) : zk_fri_commit(H[j], c0->b, coset, &hc.cm[j]));
            memcpy(h_roots + 32 * j, hc.cm[j]->root, 32);
        }
        ZK_TRY(ev.mark(&e2));
    }
    wiring_helpers<F>(tr, h_roots, d, ch);
    if (chal_out) {
        store_host<F>(chal_out, ch.beta);
        store_host<F>(chal_out + W, ch.gamma);
        store_host<F>(chal_out + 2 * W, ch.alpha);
        store_host<F>(chal_out + 3 * W, ch.mu);
        memcpy(chal_out + 4 * W, ch.tau.data(), ch.tau.size() * 8);
    }

    const void *opened[K];
    for (int j = 0; j < K; j++) opened[j] = (j < kWiringGiven ? cms[j] : hc.cm[j - kWiringGiven])->coeffs->dptr;
    IdBase<F> idb;
    const auto launch = [&](bool fold, const void *const *in, void *out0, size_t ostride, size_t q, const Fe<F> &r, unsigned l, void *partials, void *sums) {
        return launch_round<F>(fold, in, out0, ostride, q, r, ch, idb.at(l, r), l, d, partials, sums);
    };
    ZK_TRY((prove_rounds<F, kTables, kWiringSums, kWiringNodes>(opened, d, ch.tau.data(), tr, launch, [&](const Fe<F> *S, Fe<F> *g) { wiring_message<F>(S, ch.mu, g); },
                                                                round_polys, challenges, z, ev, &e2, &st.ms_eq, &st.ms_rounds)));
    st.rounds = d;
    st.ms_fractions = ev.ms(e0, e1);
    st.ms_commit = ev.ms(e1, e2);
    return ZK_OK;
}

}  // namespace

extern "C" {

int zk_wiring_fractions(const zk_table *W, const zk_table *S, uint64_t first, const uint64_t *beta, const uint64_t *gamma, zk_table **H) {
    if (!W || !S || !beta || !gamma || !H || W->field != S->field || (W->field != ZK_FR381 && W->field != ZK_BN254_FR)) return ZK_E_ARG;
    if (W->len != S->len) return ZK_E_LEN_MISMATCH;
    if (!is_pow2(W->len)) return ZK_E_NOT_POW2;
    if (W->len < 2 || !all_reduced(W->field, beta, 1) || !all_reduced(W->field, gamma, 1)) return ZK_E_ARG;
    ZK_TRY(require_device());
    FRI_DISPATCH(W->field, return fractions_once<F>(W, S, first, beta, gamma, H));
    return ZK_OK;
}

int zk_wiring_round(const zk_table *const tables[10], const uint64_t *beta, const uint64_t *gamma, const uint64_t *alpha, const uint64_t *mu, const uint64_t *id_base,
                    uint32_t log_step, const uint64_t *r, zk_table **outs, uint64_t *g5) {
    ZK_TRY(wiring_round_check(tables, kTables, beta, gamma, alpha, mu, id_base, log_step, r, outs, g5));
    FRI_DISPATCH(tables[0]->field, return hook_round<F>(tables, wiring_challenges<F>(beta, gamma, alpha, mu), id_base, log_step, r, outs, g5));
    return ZK_OK;
}

int zk_wiring_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group, size_t *nround, size_t *nhroots,
                    size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nopen_round) {
    ZK_TRY(zk_fri_ml_sizes_batch(kWiringOpened, d, log_blowup, log_final, nqueries, log_arity, log_group, nroots, nfinal, nvalues, path_bytes, nopen_round));
    if (nround) *nround = (size_t)kWiringNodes * d;
    if (nhroots) *nhroots = kWiringWires;
    return ZK_OK;
}

int zk_wiring_prove(const zk_fri_commitment *const cms[6], uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t grinding_bits, zk_transcript *t,
                    uint8_t *h_roots, uint64_t *chal_out, uint64_t *round_polys, uint64_t *challenges, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *open_round_polys,
                    uint8_t *roots, uint64_t *final_table, uint64_t *open_challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths,
                    uint64_t *pow_nonce) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!cms) return ZK_E_ARG;
    for (int j = 0; j < kWiringGiven; j++)
        if (!cms[j]) return ZK_E_ARG;
    if (!h_roots || !round_polys || !challenges) return ZK_E_ARG;
    if (cms[0]->d < 1 || cms[0]->d > 32) return ZK_E_ARG;     // what sizes the point below; no commitment is made outside it
    // the point and the helper commitments do not exist yet: the opener's statuses are taken on the six and a stand-in of zeros, before the
    // transcript moves (the helpers get the shape of the six, and nine is within the opener's count)
    std::vector<uint64_t> z((size_t)cms[0]->d * 4, 0);
    ZK_TRY(fri_ml_open_batch_check(cms, kWiringGiven, z.data(), 1, log_final, nqueries, log_arity, ys_out, open_round_polys, roots, final_table, query_values, query_paths,
                                   grinding_bits, pow_nonce));
    zk_transcript own;
    zk_transcript *tt = t ? t : &own;
    zk_wiring_stats st{};
    CommitHolder hc;
    FRI_DISPATCH(cms[0]->field, ZK_TRY((prove_steps<F>(cms, tt->t, hc, h_roots, chal_out, round_polys, challenges, z.data(), st))));
    const zk_fri_commitment *all[kWiringOpened];
    for (int j = 0; j < kWiringOpened; j++) all[j] = j < kWiringGiven ? cms[j] : hc.cm[j - kWiringGiven];
    const int opened = zk_fri_ml_open_batch_pow(all, kWiringOpened, z.data(), 1, log_final, nqueries, log_arity, tt, ys_out, gamma_out, open_round_polys, roots, final_table,
                                                open_challenges, query_indices, query_values, query_paths, grinding_bits, pow_nonce);
    return prove_finish(opened, t0, st, g_wiring_stats);
}

int zk_wiring_verify(int field, const uint8_t *roots_of_six, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group,
                     const uint64_t *coset, zk_transcript *t, const uint8_t *h_roots, const uint64_t *round_polys, const uint64_t *ys, const uint64_t *open_round_polys,
                     const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values, const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce,
                     int *ok) {
    const bool have_all = roots_of_six && h_roots && round_polys && ys && open_round_polys && roots && final_table && query_values && query_paths && ok;
    ZK_TRY(verify_check(field, d, log_blowup, coset, grinding_bits, have_all, [&] {
        return zk_fri_ml_sizes_batch(kWiringOpened, d, log_blowup, log_final, nqueries, log_arity, log_group, nullptr, nullptr, nullptr, nullptr, nullptr);
    }));
    uint8_t nine[32 * kWiringOpened];
    memcpy(nine, roots_of_six, 32 * kWiringGiven);
    memcpy(nine + 32 * kWiringGiven, h_roots, 32 * kWiringWires);
    zk_transcript work;
    if (t) work.t = t->t;
    std::vector<uint64_t> z((size_t)d * 4);
    bool good = false;
    FRI_DISPATCH(field, (wiring_replay<F>(work.t, roots_of_six, d, h_roots, round_polys, ys, z.data(), &good)));
    int open_ok = 0;
    ZK_TRY(zk_fri_ml_verify_batch_pow(field, nine, kWiringOpened, d, log_blowup, log_final, nqueries, log_arity, log_group, coset, z.data(), 1, ys, &work, open_round_polys,
                                      roots, final_table, query_values, query_paths, grinding_bits, pow_nonce, &open_ok));
    if (t) t->t = work.t;
    *ok = good && open_ok ? 1 : 0;
    return ZK_OK;
}

int zk_wiring_last_stats(zk_wiring_stats *out) {
    if (!out) return ZK_E_ARG;
    *out = g_wiring_stats;
    return ZK_OK;
}

}  // extern "C"
