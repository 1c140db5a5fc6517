// zkmle_zerocheck.hip -- C ABI of the zerochecks over FRI commitments (zerocheck.cuh, zerocheck_host.h): the product A o B = C over three
// commitments and the Plonk gate qM A B + qL A + qR B + qO C + qC = 0 over eight.  For each: one round pass on its own, the prover (the
// sumcheck of sum_x eq(x, tau) relation(x) = 0 on the commitments' coefficient tables, then zk_fri_ml_open_batch_pow of the K commitments at
// the point the rounds leave, on the same transcript) and its host verifier.  One round driver, one prover and one verifier serve both,
// parametrised by zerocheck_host.h's statement.  Extension: the protocols are defined in include/zkmle.h "Zerocheck of a product of
// committed tables" and "Zerocheck of a Plonk gate over committed tables".
#include <string.h>

#include <chrono>
#include <vector>

#include "eq_table.cuh"
#include "fri_host.h"
#include "zerocheck.cuh"
#include "zerocheck_host.h"

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

// sums (device, NODES elements) = the pass's sums at the nodes 0 .. NODES - 2 and infinity.  Launches only.
template <class F, class St> int launch_round(bool fold, const typename Pass<St>::Tables &t, size_t q, const Fe<F> &r, void *partials, void *sums) {
    const int grid = reduce_grid_for(q);
    if (fold) Pass<St>::template launch<F, true>(grid, t, q, r, partials);
    else Pass<St>::template launch<F, false>(grid, t, q, r, partials);
    ZK_HIP(hipGetLastError());
    finish_sums_kernel<F><<<1, kBlock, 0, cur_stream()>>>(partials, (size_t)grid, St::NODES, sums);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

// room for the workgroups' partial sums and the `nsums` sums behind them
struct SumsBuf {
    DevBuf buf;
    void *sums = nullptr;
    int alloc(size_t esz, size_t nsums) {
        const size_t cap = (size_t)reduce_block_cap();
        ZK_TRY(buf.alloc((nsums * cap + nsums) * esz));
        sums = (char *)buf.p + nsums * cap * esz;
        return ZK_OK;
    }
};

// the checks of a round hook on its T = K + 1 tables, in the order of zk_zerocheck_mul_round's statuses
inline int round_check(const zk_table *const *in, int T, const uint64_t *r, zk_table **outs, const uint64_t *g) {
    for (int j = 0; j < T; j++)
        if (!in[j]) return ZK_E_ARG;
    if (!g || (r && !outs) || (in[0]->field != ZK_FR381 && in[0]->field != ZK_BN254_FR)) return ZK_E_ARG;
    for (int j = 1; j < T; j++)
        if (in[j]->field != in[0]->field) return ZK_E_ARG;
    for (int j = 1; j < T; j++)
        if (in[j]->len != in[0]->len) return ZK_E_LEN_MISMATCH;
    if (!is_pow2(in[0]->len)) return ZK_E_NOT_POW2;
    if (in[0]->len < (r ? 4u : 2u) || (r && !all_reduced(in[0]->field, r, 1))) return ZK_E_ARG;
    return require_device();
}

template <class F, class St> int round_once(const zk_table *const *in, const uint64_t *r, zk_table **outs, uint64_t *gout) {
    constexpr size_t ESZ = sizeof(Fe<F>);
    constexpr int W = F::N / 2, T = St::K + 1, NS = St::NODES;
    const bool fold = r != nullptr;
    const size_t len = in[0]->len, q = fold ? len / 4 : len / 2;
    SumsBuf sb;
    ZK_TRY(sb.alloc(ESZ, NS));
    zk_table *o[T] = {};
    const auto drop = [&] { for (zk_table *t : o) zk_table_free(t); };
    typename Pass<St>::Tables t{};
    for (int j = 0; j < T; j++) {
        t.in[j] = in[j]->dptr;
        if (!fold) continue;
        const int rc = zk_table_alloc(in[0]->field, len / 2, &o[j]);
        if (rc != ZK_OK) { drop(); return rc; }
        t.out[j] = o[j]->dptr;
    }
    Fe<F> S[NS], g[NS];
    int rc = launch_round<F, St>(fold, t, q, fold ? load_host<F>(r) : fe_one<F>(), sb.buf.p, sb.sums);
    if (rc == ZK_OK && zk::memcpy_on_stream(S, sb.sums, NS * ESZ, hipMemcpyDeviceToHost) != hipSuccess) rc = ZK_E_HIP;
    if (rc != ZK_OK) { drop(); return rc; }
    St::template message<F>(S, g);
    for (int k = 0; k < NS; k++) store_host<F>(gout + (size_t)k * W, g[k]);
    for (int j = 0; fold && j < T; j++) outs[j] = o[j];
    return ZK_OK;
}

// the statement, E_0 and the d rounds on `tr`; z (d elements) = the point the opening is made at.  One host synchronisation per round: the
// sums down, the transcript's step on the host, r_l up as the next pass's argument.
template <class F, class St> int prove_rounds(const zk_fri_commitment *const *cms, Transcript &tr, uint64_t *tau_out, uint64_t *round_polys, uint64_t *challenges,
                                              uint64_t *z, zk_zerocheck_stats &st) {
    constexpr size_t ESZ = sizeof(Fe<F>);
    constexpr int W = F::N / 2, K = St::K, T = St::K + 1, NS = St::NODES;
    const unsigned d = cms[0]->d;
    const size_t n = (size_t)1 << d;
    uint8_t roots[32 * K];
    for (int j = 0; j < K; j++) memcpy(roots + 32 * j, cms[j]->root, 32);
    std::vector<uint64_t> tau((size_t)d * W);
    zerocheck_statement<F, St>(tr, roots, d, tau.data());
    if (tau_out) memcpy(tau_out, tau.data(), tau.size() * 8);

    // one block: E_0 (n elements), then the two ping-pong halves: the T tables of an odd round (n / 2 entries each at round 1) and of an
    // even one (n / 4 each at round 2); a round's tables never outgrow the half they first had
    DevBuf blk;
    SumsBuf sb;
    ZK_TRY(blk.alloc((n + T * (n / 2) + T * (n / 4) + 1) * ESZ));
    ZK_TRY(sb.alloc(ESZ, NS));
    char *E0 = (char *)blk.p, *half[2] = {E0 + n * ESZ, E0 + (n + T * (n / 2)) * ESZ};
    const auto tables_at = [&](unsigned l, const void **out) {   // the K tables and E at round l: n >> l entries each
        for (int j = 0; j < T; j++) out[j] = l == 0 ? (j < K ? cms[j]->coeffs->dptr : (void *)E0) : half[(l - 1) & 1] + (size_t)j * (n >> l) * ESZ;
    };
    Events ev;
    size_t e0, e1, e2;
    ZK_TRY(ev.mark(&e0));
    EqBuilder<F> eqb;
    ZK_TRY(eqb.build(tau.data(), d, E0));
    ZK_TRY(ev.mark(&e1));
    Fe<F> r = fe_one<F>();
    for (unsigned l = 0; l < d; l++) {
        typename Pass<St>::Tables t{};
        if (l == 0) {
            tables_at(0, t.in);
        } else {
            const void *to[T];
            tables_at(l - 1, t.in);
            tables_at(l, to);
            for (int j = 0; j < T; j++) t.out[j] = const_cast<void *>(to[j]);
        }
        ZK_TRY((launch_round<F, St>(l != 0, t, n >> (l + 1), r, sb.buf.p, sb.sums)));
        Fe<F> S[NS], g[NS];
        ZK_HIP(zk::memcpy_on_stream(S, sb.sums, NS * ESZ, hipMemcpyDeviceToHost));   // the round's synchronisation
        if (l == 0) eqb.release();
        St::template message<F>(S, g);
        for (int k = 0; k < NS; k++) {
            store_host<F>(round_polys + ((size_t)l * NS + k) * W, g[k]);
            tr.append_be<F>(g[k]);
        }
        r = tr.random_challenge_as_field_element<F>();
        store_host<F>(challenges + (size_t)l * W, r);
        store_host<F>(z + (size_t)(d - 1 - l) * W, r);
    }
    ZK_TRY(ev.mark(&e2));
    ZK_HIP(hipEventSynchronize(ev.ev[e2]));
    st.rounds = d;
    st.ms_eq = ev.ms(e0, e1);
    st.ms_rounds = ev.ms(e1, e2);
    return ZK_OK;
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
    FRI_DISPATCH(cms[0]->field, ZK_TRY((prove_rounds<F, St>(cms, tt->t, tau_out, round_polys, challenges, z.data(), st))));
    ZK_TRY(zk_fri_ml_open_batch_pow(cms, St::K, z.data(), 1, log_final, nqueries, log_arity, tt, ys_out, gamma_out, open_round_polys, roots, final_table, open_challenges,
                                    query_indices, query_values, query_paths, grinding_bits, pow_nonce));
    zk_fri_ml_stats ml{};
    (void)zk_fri_ml_last_stats(&ml);
    st.ms_opening = ml.ms_total;
    st.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g_zc_stats = st;
    return ZK_OK;
}

// zk_zerocheck_mul_verify / zk_zerocheck_gate_verify; own_roots: the statement's K roots as the verifier holds them
template <class St> int verify(int field, const uint8_t *own_roots, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                               uint32_t log_group, const uint64_t *coset, zk_transcript *t, const uint64_t *round_polys, const uint64_t *ys,
                               const uint64_t *open_round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                               const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce, int *ok) {
    if (grinding_bits > ZK_FRI_GRIND_MAX_BITS) return ZK_E_ARG;
    if (!own_roots || !round_polys || !ys || !open_round_polys || !roots || !final_table || !query_values || !query_paths || !ok) return ZK_E_ARG;
    // every status before the transcript is touched: the opening's own on an empty replay, as zk_sumcheck_basic_verify_succinct; and the replay
    // and the opening's verifier run on a copy that becomes the caller's transcript only with ZK_OK
    if (field_limbs64(field) < 0) return ZK_E_ARG;
    ZK_TRY(zk_fri_ml_sizes_batch(St::K, d, log_blowup, log_final, nqueries, log_arity, log_group, nullptr, nullptr, nullptr, nullptr, nullptr));
    if (coset && is_zero_element(field, coset)) return ZK_E_ARG;
    if ((field != ZK_FR381 && field != ZK_BN254_FR) || d + log_blowup > two_adicity(field)) return ZK_E_RANGE;
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
    FRI_DISPATCH(A->field, return (round_once<F, ZerocheckMul>(in, r, outs, g4)));
    return ZK_OK;
}

int zk_zerocheck_gate_round(const zk_table *const tables[9], const uint64_t *r, zk_table **outs, uint64_t *g5) {
    if (!tables) return ZK_E_ARG;
    ZK_TRY(round_check(tables, 9, r, outs, g5));
    FRI_DISPATCH(tables[0]->field, return (round_once<F, ZerocheckGate>(tables, r, outs, g5)));
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
