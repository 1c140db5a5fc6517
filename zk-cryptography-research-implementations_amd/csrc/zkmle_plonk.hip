// zkmle_plonk.hip -- C ABI of the Plonk proof over FRI commitments (plonk.cuh, plonk_host.h): one round pass on its own, the public inputs' value
// at a point, the prover (the wiring's three helper tables and their commitments, ONE sumcheck of the gate and the wiring on the fourteen
// coefficient tables and E whose claimed sum carries the public inputs, then zk_fri_ml_open_batch_pow of the fourteen commitments at the point the
// rounds leave, on the same transcript) and its host verifier.  The round loop, the hook's pass and the shells' shared checks are
// zerocheck_driver.cuh's, by wiring_driver.cuh.  Extension: the protocol is defined in include/zkmle.h "Plonk: gate, wiring and
// public inputs in one sumcheck".
#include <string.h>

#include <chrono>
#include <vector>

#include "plonk.cuh"
#include "plonk_host.h"
#include "wiring_driver.cuh"

using namespace zk;
using namespace zk::host;

namespace {

thread_local zk_plonk_stats g_plonk_stats{};

constexpr int kTables = kPlonkTables;                        // the fourteen opened and E
static_assert(kTables == kPlonkOpened + 1, "the pass folds the opened tables and E");

// sums (device, 7 elements) of a pass over q pairs whose id tables are c_l + 2^l x + j 2^d; the fifteen folded to out0 + j ostride.  Launches only.
template <class F> int launch_round(bool fold, const void *const *in, void *out0, size_t ostride, size_t q, const Fe<F> &r, const WiringChallenges<F> &ch, const Fe<F> &id_base,
                                    unsigned log_step, unsigned d, void *partials, void *sums) {
    PlonkTables t{};
    for (int j = 0; j < kTables; j++) t.in[j] = in[j];
    t.out0 = out0;
    t.ostride = ostride;
    const int grid = reduce_grid_for(q);
    PlonkConsts<F> c;
    c.beta = ch.beta;
    c.gamma = ch.gamma;
    c.alpha = ch.alpha;
    c.alpha3 = fe_mul<F>(ch.alpha, fe_mul<F>(ch.alpha, ch.alpha));
    c.gstep = fe_mul<F>(ch.gamma, fe_from_u64<F>((uint64_t)1 << log_step));
    c.gwire = fe_mul<F>(ch.gamma, fe_from_u64<F>((uint64_t)1 << d));
    c.gid0 = fe_mul<F>(ch.gamma, id_base);
    c.gnext = fe_sub<F>(fe_mul<F>(fe_dbl<F>(c.gstep), fe_from_u64<F>((uint64_t)grid * kBlock)), fe_dbl<F>(c.gwire));
    if (fold) plonk_round_kernel<F, true><<<grid, kBlock, 0, cur_stream()>>>(t, q, r, c, partials);
    else plonk_round_kernel<F, false><<<grid, kBlock, 0, cur_stream()>>>(t, q, r, c, partials);
    ZK_HIP(hipGetLastError());
    finish_sums_kernel<F><<<1, kBlock, 0, cur_stream()>>>(partials, (size_t)grid, kWiringSums, sums);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class F> int hook_round(const zk_table *const *in, const WiringChallenges<F> &ch, const uint64_t *id_base, unsigned log_step, const uint64_t *r, zk_table **outs,
                                  uint64_t *gout) {
    const Fe<F> id0 = load_host<F>(id_base);
    const auto launch = [&](bool fold, const void *const *ip, void *out0, size_t ostride, size_t q, const Fe<F> &rr, unsigned, void *partials, void *sums) {
        return launch_round<F>(fold, ip, out0, ostride, q, rr, ch, id0, log_step, ilog2(2 * q) + log_step, partials, sums);
    };
    return round_once<F, kTables, kWiringSums, kPlonkNodes>(in, r, outs, gout, launch, [&](const Fe<F> *S, Fe<F> *g) { wiring_message<F>(S, ch.mu, g); });
}

// steps 1 to 8 on `tr`: the statement, the helper tables and their commitments (hc, h_roots), then E_0 and the d rounds by zerocheck_driver.cuh;
// z (d elements) = the point the opening is made at.
template <class F> int prove_steps(const zk_fri_commitment *const *cms, const uint64_t *pub, uint32_t npublic, Transcript &tr, CommitHolder &hc, uint8_t *h_roots,
                                   uint64_t *chal_out, uint64_t *round_polys, uint64_t *challenges, uint64_t *z, zk_plonk_stats &st) {
    constexpr int W = F::N / 2, K = kPlonkOpened;
    const zk_fri_commitment *c0 = cms[0];
    const unsigned d = c0->d;
    const size_t n = (size_t)1 << d;
    uint8_t roots[32 * kPlonkGiven];
    for (int j = 0; j < kPlonkGiven; j++) memcpy(roots + 32 * j, cms[j]->root, 32);
    WiringChallenges<F> ch;
    plonk_statement<F>(tr, roots, d, pub, npublic, ch);

    Events ev;
    size_t e0, e1, e2;
    ZK_TRY(ev.mark(&e0));
    {
        TableHolder th;
        zk_table *H[kWiringWires];
        for (int j = 0; j < kWiringWires; j++) {
            ZK_TRY(th.alloc(c0->field, n, &H[j]));
            ZK_TRY(launch_fractions<F>(cms[j]->coeffs->dptr, cms[PLONK_S + j]->coeffs->dptr, H[j]->dptr, n, (uint64_t)j * n, ch.beta, ch.gamma));
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
    for (int j = 0; j < K; j++) opened[j] = (j < kPlonkGiven ? cms[j] : hc.cm[j - kPlonkGiven])->coeffs->dptr;
    IdBase<F> idb;
    const auto launch = [&](bool fold, const void *const *in, void *out0, size_t ostride, size_t q, const Fe<F> &r, unsigned l, void *partials, void *sums) {
        return launch_round<F>(fold, in, out0, ostride, q, r, ch, idb.at(l, r), l, d, partials, sums);
    };
    ZK_TRY((prove_rounds<F, kTables, kWiringSums, kPlonkNodes>(opened, d, ch.tau.data(), tr, launch, [&](const Fe<F> *S, Fe<F> *g) { wiring_message<F>(S, ch.mu, g); },
                                                               round_polys, challenges, z, ev, &e2, &st.ms_eq, &st.ms_rounds)));
    st.rounds = d;
    st.ms_fractions = ev.ms(e0, e1);
    st.ms_commit = ev.ms(e1, e2);
    return ZK_OK;
}

}  // namespace

extern "C" {

int zk_plonk_round(const zk_table *const tables[15], const uint64_t *beta, const uint64_t *gamma, const uint64_t *alpha, const uint64_t *mu, const uint64_t *id_base,
                   uint32_t log_step, const uint64_t *r, zk_table **outs, uint64_t *g5) {
    ZK_TRY(wiring_round_check(tables, kTables, beta, gamma, alpha, mu, id_base, log_step, r, outs, g5));
    FRI_DISPATCH(tables[0]->field, return hook_round<F>(tables, wiring_challenges<F>(beta, gamma, alpha, mu), id_base, log_step, r, outs, g5));
    return ZK_OK;
}

int zk_plonk_public_eval(int field, const uint64_t *public_inputs, uint32_t npublic, const uint64_t *tau, uint32_t d, uint64_t *out) {
    if (!tau || !out || d < 1 || d > 32 || (field != ZK_FR381 && field != ZK_BN254_FR) || !plonk_public_shape_ok(public_inputs, npublic, d)) return ZK_E_ARG;
    if (!all_reduced(field, public_inputs, npublic) || !all_reduced(field, tau, d)) return ZK_E_ARG;
    FRI_DISPATCH(field, store_host<F>(out, plonk_public_eval<F>(public_inputs, npublic, tau, d)));
    return ZK_OK;
}

int zk_plonk_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group, size_t *nround, size_t *nhroots,
                   size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nopen_round) {
    ZK_TRY(zk_fri_ml_sizes_batch(kPlonkOpened, d, log_blowup, log_final, nqueries, log_arity, log_group, nroots, nfinal, nvalues, path_bytes, nopen_round));
    if (nround) *nround = (size_t)kPlonkNodes * d;
    if (nhroots) *nhroots = kWiringWires;
    return ZK_OK;
}

int zk_plonk_prove(const zk_fri_commitment *const cms[11], const uint64_t *public_inputs, uint32_t npublic, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                   uint32_t grinding_bits, zk_transcript *t, uint8_t *h_roots, uint64_t *chal_out, uint64_t *round_polys, uint64_t *challenges, uint64_t *ys_out,
                   uint64_t *gamma_out, uint64_t *open_round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *open_challenges, uint64_t *query_indices,
                   uint64_t *query_values, uint8_t *query_paths, uint64_t *pow_nonce) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!cms) return ZK_E_ARG;
    for (int j = 0; j < kPlonkGiven; j++)
        if (!cms[j]) return ZK_E_ARG;
    if (!h_roots || !round_polys || !challenges) return ZK_E_ARG;
    if (cms[0]->d < 1 || cms[0]->d > 32) return ZK_E_ARG;     // what sizes the point below; no commitment is made outside it
    // the point and the helper commitments do not exist yet: the opener's statuses are taken on the eleven and a stand-in of zeros, before the
    // transcript moves (the helpers get the shape of the eleven, and fourteen is within the opener's count)
    std::vector<uint64_t> z((size_t)cms[0]->d * 4, 0);
    ZK_TRY(fri_ml_open_batch_check(cms, kPlonkGiven, z.data(), 1, log_final, nqueries, log_arity, ys_out, open_round_polys, roots, final_table, query_values, query_paths,
                                   grinding_bits, pow_nonce));
    if (!plonk_public_shape_ok(public_inputs, npublic, cms[0]->d) || !all_reduced(cms[0]->field, public_inputs, npublic)) return ZK_E_ARG;
    zk_transcript own;
    zk_transcript *tt = t ? t : &own;
    zk_plonk_stats st{};
    CommitHolder hc;
    FRI_DISPATCH(cms[0]->field, ZK_TRY((prove_steps<F>(cms, public_inputs, npublic, tt->t, hc, h_roots, chal_out, round_polys, challenges, z.data(), st))));
    const zk_fri_commitment *all[kPlonkOpened];
    for (int j = 0; j < kPlonkOpened; j++) all[j] = j < kPlonkGiven ? cms[j] : hc.cm[j - kPlonkGiven];
    const int opened = zk_fri_ml_open_batch_pow(all, kPlonkOpened, z.data(), 1, log_final, nqueries, log_arity, tt, ys_out, gamma_out, open_round_polys, roots, final_table,
                                                open_challenges, query_indices, query_values, query_paths, grinding_bits, pow_nonce);
    return prove_finish(opened, t0, st, g_plonk_stats);
}

int zk_plonk_verify(int field, const uint8_t *roots_of_eleven, const uint64_t *public_inputs, uint32_t npublic, uint32_t d, uint32_t log_blowup, uint32_t log_final,
                    uint32_t nqueries, uint32_t log_arity, uint32_t log_group, const uint64_t *coset, zk_transcript *t, const uint8_t *h_roots, const uint64_t *round_polys,
                    const uint64_t *ys, const uint64_t *open_round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                    const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce, int *ok) {
    const bool have_all = roots_of_eleven && h_roots && round_polys && ys && open_round_polys && roots && final_table && query_values && query_paths && ok;
    ZK_TRY(verify_check(field, d, log_blowup, coset, grinding_bits, have_all, [&] {
        return zk_fri_ml_sizes_batch(kPlonkOpened, d, log_blowup, log_final, nqueries, log_arity, log_group, nullptr, nullptr, nullptr, nullptr, nullptr);
    }));
    if (!plonk_public_shape_ok(public_inputs, npublic, d)) return ZK_E_ARG;
    uint8_t all[32 * kPlonkOpened];
    memcpy(all, roots_of_eleven, 32 * kPlonkGiven);
    memcpy(all + 32 * kPlonkGiven, h_roots, 32 * kWiringWires);
    zk_transcript work;
    if (t) work.t = t->t;
    std::vector<uint64_t> z((size_t)d * 4);
    bool good = false;
    FRI_DISPATCH(field, (plonk_replay<F>(work.t, roots_of_eleven, d, public_inputs, npublic, h_roots, round_polys, ys, z.data(), &good)));
    int open_ok = 0;
    ZK_TRY(zk_fri_ml_verify_batch_pow(field, all, kPlonkOpened, d, log_blowup, log_final, nqueries, log_arity, log_group, coset, z.data(), 1, ys, &work, open_round_polys,
                                      roots, final_table, query_values, query_paths, grinding_bits, pow_nonce, &open_ok));
    if (t) t->t = work.t;
    *ok = good && open_ok ? 1 : 0;
    return ZK_OK;
}

int zk_plonk_last_stats(zk_plonk_stats *out) {
    if (!out) return ZK_E_ARG;
    *out = g_plonk_stats;
    return ZK_OK;
}

}  // extern "C"
