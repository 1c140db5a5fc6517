// zkmle_zerocheck.hip -- C ABI of the zerochecks over FRI commitments (zerocheck.cuh, zerocheck_host.h): the product A o B = C over three
// commitments and the Plonk gate qM A B + qL A + qR B + qO C + qC = 0 over eight.  For each: one round pass on its own, the prover (the
// sumcheck of sum_x eq(x, tau) relation(x) = 0 on the commitments' coefficient tables, then zk_fri_ml_open_batch_pow of the K commitments at
// the point the rounds leave, on the same transcript) and its host verifier.  One launch, one prover and one verifier serve both, parametrised
// by zerocheck_host.h's statement; the round loop, the hook's pass and the shells' shared checks are zerocheck_driver.cuh's.  Extension: the protocols are defined in include/zkmle.h "Zerocheck of a product of
// committed tables" and "Zerocheck of a Plonk gate over committed tables".
#include <string.h>

#include <chrono>
#include <vector>

#include "zerocheck.cuh"
#include "zerocheck_driver.cuh"

using namespace zk;
using namespace zk::host;

namespace {

thread_local zk_zerocheck_stats g_zc_stats{};

// the pass of a statement: its tables (the K commitments' in the statement's order, then E) and its kernel
template <class St> struct Pass;
template <> struct Pass<ZerocheckMul> {
    using Tables = ZerocheckTables;
    template <class F, bool FOLD> static void launch(int grid, const Tables &t, size_t q, const Fe<F> &r, void *partials) {
        zerocheck_mul_round_kernel<F, FOLD><<<grid, kBlock, 0, cur_stream()>>>(t, q, r, partials);
    }
};
template <> struct Pass<ZerocheckGate> {
    using Tables = ZerocheckGateTables;
    template <class F, bool FOLD> static void launch(int grid, const Tables &t, size_t q, const Fe<F> &r, void *partials) {
        zerocheck_gate_round_kernel<F, FOLD><<<grid, kBlock, 0, cur_stream()>>>(t, q, r, partials);
    }
};

// zerocheck_driver.cuh's launch for the statement: sums (device, NODES elements) = the pass's sums at the nodes 0 .. NODES - 2 and infinity.
// The kernels take one output per table: out0 + j ostride, as the driver lays them out.  Launches only.
template <class F, class St>
int launch_round(bool fold, const void *const *in, void *out0, size_t ostride, size_t q, const Fe<F> &r, unsigned, void *partials, void *sums) {
    typename Pass<St>::Tables t{};
    for (int j = 0; j < St::K + 1; j++) {
        t.in[j] = in[j];
        if (fold) t.out[j] = (char *)out0 + (size_t)j * ostride;
    }
    const int grid = reduce_grid_for(q);
    if (fold) Pass<St>::template launch<F, true>(grid, t, q, r, partials);
    else Pass<St>::template launch<F, false>(grid, t, q, r, partials);
    ZK_HIP(hipGetLastError());
    finish_sums_kernel<F><<<1, kBlock, 0, cur_stream()>>>(partials, (size_t)grid, St::NODES, sums);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

// the checks of a round hook on its T = K + 1 tables, in the order of zk_zerocheck_mul_round's statuses
inline int round_check(const zk_table *const *in, int T, const uint64_t *r, zk_table **outs, const uint64_t *g) {
    if (!g || (r && !outs)) return ZK_E_ARG;
    ZK_TRY(check_tables(in, T, r ? 4 : 2));
    if (r && !all_reduced(in[0]->field, r, 1)) return ZK_E_ARG;
    return require_device();
}

template <class F, class St> int hook_round(const zk_table *const *in, const uint64_t *r, zk_table **outs, uint64_t *gout) {
    return round_once<F, St::K + 1, St::NODES, St::NODES>(in, r, outs, gout, launch_round<F, St>, St::template message<F>);
}

// the statement and, by zerocheck_driver.cuh, E_0 and the d rounds on `tr`; z (d elements) = the point the opening is made at
template <class F, class St> int prove_steps(const zk_fri_commitment *const *cms, Transcript &tr, uint64_t *tau_out, uint64_t *round_polys, uint64_t *challenges,
                                             uint64_t *z, zk_zerocheck_stats &st) {
    constexpr int K = St::K;
    const unsigned d = cms[0]->d;
    uint8_t roots[32 * K];
    const void *opened[K];
    for (int j = 0; j < K; j++) {
        memcpy(roots + 32 * j, cms[j]->root, 32);
        opened[j] = cms[j]->coeffs->dptr;
    }
    std::vector<uint64_t> tau((size_t)d * (F::N / 2));
    zerocheck_statement<F, St>(tr, roots, d, tau.data());
    if (tau_out) memcpy(tau_out, tau.data(), tau.size() * 8);
    Events ev;
    st.rounds = d;
    return prove_rounds<F, K + 1, St::NODES, St::NODES>(opened, d, tau.data(), tr, launch_round<F, St>, St::template message<F>, round_polys, challenges, z, ev, nullptr,
                                                        &st.ms_eq, &st.ms_rounds);
}

// zk_zerocheck_mul_prove / zk_zerocheck_gate_prove on the statement's K commitments
template <class St> int prove(const zk_fri_commitment *const *cms, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t grinding_bits, zk_transcript *t,
                              uint64_t *tau_out, uint64_t *round_polys, uint64_t *challenges, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *open_round_polys,
                              uint8_t *roots, uint64_t *final_table, uint64_t *open_challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths,
                              uint64_t *pow_nonce) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int j = 0; j < St::K; j++)
        if (!cms[j]) return ZK_E_ARG;
    if (!round_polys || !challenges) return ZK_E_ARG;
    if (cms[0]->d < 1 || cms[0]->d > 32) return ZK_E_ARG;     // what sizes the point below; no commitment is made outside it
    // the point does not exist yet: the opener's statuses are taken on a stand-in of zeros, before the transcript moves
    std::vector<uint64_t> z((size_t)cms[0]->d * 4, 0);
    ZK_TRY(fri_ml_open_batch_check(cms, St::K, z.data(), 1, log_final, nqueries, log_arity, ys_out, open_round_polys, roots, final_table, query_values, query_paths,
                                   grinding_bits, pow_nonce));
    zk_transcript own;
    zk_transcript *tt = t ? t : &own;
    zk_zerocheck_stats st{};
    FRI_DISPATCH(cms[0]->field, ZK_TRY((prove_steps<F, St>(cms, tt->t, tau_out, round_polys, challenges, z.data(), st))));
    const int opened = zk_fri_ml_open_batch_pow(cms, St::K, z.data(), 1, log_final, nqueries, log_arity, tt, ys_out, gamma_out, open_round_polys, roots, final_table,
                                                open_challenges, query_indices, query_values, query_paths, grinding_bits, pow_nonce);
    return prove_finish(opened, t0, st, g_zc_stats);
}

// zk_zerocheck_mul_verify / zk_zerocheck_gate_verify; own_roots: the statement's K roots as the verifier holds them
template <class St> int verify(int field, const uint8_t *own_roots, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                               uint32_t log_group, const uint64_t *coset, zk_transcript *t, const uint64_t *round_polys, const uint64_t *ys,
                               const uint64_t *open_round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                               const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce, int *ok) {
    const bool have_all = own_roots && round_polys && ys && open_round_polys && roots && final_table && query_values && query_paths && ok;
    ZK_TRY(verify_check(field, d, log_blowup, coset, grinding_bits, have_all, [&] {
        return zk_fri_ml_sizes_batch(St::K, d, log_blowup, log_final, nqueries, log_arity, log_group, nullptr, nullptr, nullptr, nullptr, nullptr);
    }));
    zk_transcript work;
    if (t) work.t = t->t;
    std::vector<uint64_t> z((size_t)d * 4);
    bool good = false;
    FRI_DISPATCH(field, (zerocheck_replay<F, St>(work.t, own_roots, d, round_polys, ys, z.data(), &good)));
    int open_ok = 0;
    ZK_TRY(zk_fri_ml_verify_batch_pow(field, own_roots, St::K, d, log_blowup, log_final, nqueries, log_arity, log_group, coset, z.data(), 1, ys, &work, open_round_polys,
                                      roots, final_table, query_values, query_paths, grinding_bits, pow_nonce, &open_ok));
    if (t) t->t = work.t;
    *ok = good && open_ok ? 1 : 0;
    return ZK_OK;
}

}  // namespace

extern "C" {

int zk_zerocheck_mul_round(const zk_table *A, const zk_table *B, const zk_table *C, const zk_table *E, const uint64_t *r, zk_table **outs, uint64_t *g4) {
    const zk_table *in[4] = {A, B, C, E};
    ZK_TRY(round_check(in, 4, r, outs, g4));
    FRI_DISPATCH(A->field, return (hook_round<F, ZerocheckMul>(in, r, outs, g4)));
    return ZK_OK;
}

int zk_zerocheck_gate_round(const zk_table *const tables[9], const uint64_t *r, zk_table **outs, uint64_t *g5) {
    ZK_TRY(round_check(tables, 9, r, outs, g5));
    FRI_DISPATCH(tables[0]->field, return (hook_round<F, ZerocheckGate>(tables, r, outs, g5)));
    return ZK_OK;
}

int zk_zerocheck_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group, size_t *nzc_round,
                       size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nround) {
    ZK_TRY(zk_fri_ml_sizes_batch(ZerocheckMul::K, d, log_blowup, log_final, nqueries, log_arity, log_group, nroots, nfinal, nvalues, path_bytes, nround));
    if (nzc_round) *nzc_round = (size_t)ZerocheckMul::NODES * d;
    return ZK_OK;
}

int zk_zerocheck_gate_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group, size_t *nzc_round,
                            size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nround) {
    ZK_TRY(zk_fri_ml_sizes_batch(ZerocheckGate::K, d, log_blowup, log_final, nqueries, log_arity, log_group, nroots, nfinal, nvalues, path_bytes, nround));
    if (nzc_round) *nzc_round = (size_t)ZerocheckGate::NODES * d;
    return ZK_OK;
}

int zk_zerocheck_mul_prove(const zk_fri_commitment *cmA, const zk_fri_commitment *cmB, const zk_fri_commitment *cmC, uint32_t log_final, uint32_t nqueries,
                           uint32_t log_arity, uint32_t grinding_bits, zk_transcript *t, uint64_t *tau_out, uint64_t *round_polys, uint64_t *challenges,
                           uint64_t *ys_out, uint64_t *gamma_out, uint64_t *open_round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *open_challenges,
                           uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths, uint64_t *pow_nonce) {
    const zk_fri_commitment *cms[3] = {cmA, cmB, cmC};
    return prove<ZerocheckMul>(cms, log_final, nqueries, log_arity, grinding_bits, t, tau_out, round_polys, challenges, ys_out, gamma_out, open_round_polys, roots,
                               final_table, open_challenges, query_indices, query_values, query_paths, pow_nonce);
}

int zk_zerocheck_gate_prove(const zk_fri_commitment *const cms[8], uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t grinding_bits, zk_transcript *t,
                            uint64_t *tau_out, uint64_t *round_polys, uint64_t *challenges, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *open_round_polys,
                            uint8_t *roots, uint64_t *final_table, uint64_t *open_challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths,
                            uint64_t *pow_nonce) {
    if (!cms) return ZK_E_ARG;
    return prove<ZerocheckGate>(cms, log_final, nqueries, log_arity, grinding_bits, t, tau_out, round_polys, challenges, ys_out, gamma_out, open_round_polys, roots,
                                final_table, open_challenges, query_indices, query_values, query_paths, pow_nonce);
}

int zk_zerocheck_mul_verify(int field, const uint8_t *roots_of_abc, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                            uint32_t log_group, const uint64_t *coset, zk_transcript *t, const uint64_t *round_polys, const uint64_t *ys,
                            const uint64_t *open_round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                            const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce, int *ok) {
    return verify<ZerocheckMul>(field, roots_of_abc, d, log_blowup, log_final, nqueries, log_arity, log_group, coset, t, round_polys, ys, open_round_polys, roots,
                                final_table, query_values, query_paths, grinding_bits, pow_nonce, ok);
}

int zk_zerocheck_gate_verify(int field, const uint8_t *roots_of_eight, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                             uint32_t log_group, const uint64_t *coset, zk_transcript *t, const uint64_t *round_polys, const uint64_t *ys,
                             const uint64_t *open_round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                             const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce, int *ok) {
    return verify<ZerocheckGate>(field, roots_of_eight, d, log_blowup, log_final, nqueries, log_arity, log_group, coset, t, round_polys, ys, open_round_polys, roots,
                                 final_table, query_values, query_paths, grinding_bits, pow_nonce, ok);
}

int zk_zerocheck_last_stats(zk_zerocheck_stats *out) {
    if (!out) return ZK_E_ARG;
    *out = g_zc_stats;
    return ZK_OK;
}

}  // extern "C"
