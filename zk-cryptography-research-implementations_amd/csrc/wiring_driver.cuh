// wiring_driver.cuh -- what the drivers of the wiring's sumcheck (zkmle_wiring.hip), of the Plonk proofs (zkmle_plonk.hip, zkmle_plonk_lookup.hip,
// zkmle_plonk_lookup_columns.hip) and of the lookup (zkmle_lookup.hip) share beyond zerocheck_driver.cuh's round driver, which it includes: the
// holder of the three helper commitments, the launch of the helper tables' kernel, the id tables' base along the rounds, and the round hooks'
// checks and challenges.  Library-internal; included by .hip files only.
#pragma once
#include "wiring.cuh"
#include "wiring_host.h"
#include "zerocheck_driver.cuh"

namespace zk {
namespace host {

// the prover's helper commitments: freed with the call
struct CommitHolder {
    zk_fri_commitment *cm[kWiringWires] = {};
    ~CommitHolder() { for (zk_fri_commitment *c : cm) zk_fri_commitment_free(c); }
};

// H (n entries, device) of one wire with id[x] = first + x.  Launches only.
template <class F> int launch_fractions(const void *W, const void *S, void *H, size_t n, uint64_t first, const Fe<F> &beta, const Fe<F> &gamma) {
    const size_t per = (size_t)kWiringBatch * kPcsBlock;
    const Fe<F> gfirst = fe_mul<F>(gamma, fe_from_u64<F>(first)), g256 = fe_mul<F>(gamma, fe_from_u64<F>((uint64_t)kPcsBlock));
    wiring_fractions_kernel<F><<<(unsigned)((n + per - 1) / per), kPcsBlock, 0, cur_stream()>>>(W, S, H, n, beta, gamma, gfirst, g256);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

// c_l = sum_{i < l} 2^i r_i, the base of the id tables c_l + 2^l x + j 2^d at round l: a prover's launch steps it with the r it is given.  at()
// changes the base, so it counts on the driver calling launch exactly once per round, in the order of the rounds, with r = r_{l-1}: a driver
// that folds two rounds in a pass has to step it twice
template <class F> struct IdBase {
    Fe<F> c = fe_zero<F>();
    const Fe<F> &at(unsigned l, const Fe<F> &r) {
        if (l != 0) c = fe_add<F>(c, fe_mul<F>(fe_from_u64<F>((uint64_t)1 << (l - 1)), r));
        return c;
    }
};

// the checks of zk_wiring_round, zk_plonk_round and zk_plonk_lookup_round on their T tables and arguments, in the order of their statuses
inline int wiring_round_check(const zk_table *const *tables, int T, const uint64_t *beta, const uint64_t *gamma, const uint64_t *alpha, const uint64_t *mu,
                              const uint64_t *id_base, uint32_t log_step, const uint64_t *r, zk_table **outs, const uint64_t *g5) {
    if (!beta || !gamma || !alpha || !mu || !id_base || !g5 || (r && !outs)) return ZK_E_ARG;
    ZK_TRY(check_tables(tables, T, r ? 4 : 2));
    const int field = tables[0]->field;
    if (r && !all_reduced(field, r, 1)) return ZK_E_ARG;
    for (const uint64_t *e : {beta, gamma, alpha, mu, id_base})
        if (!all_reduced(field, e, 1)) return ZK_E_ARG;
    const size_t len = tables[0]->len;
    if (log_step > 32 || ilog2(r ? len / 2 : len) + log_step > 32) return ZK_E_ARG;
    return require_device();
}

template <class F> WiringChallenges<F> wiring_challenges(const uint64_t *beta, const uint64_t *gamma, const uint64_t *alpha, const uint64_t *mu) {
    WiringChallenges<F> ch;
    ch.beta = load_host<F>(beta);
    ch.gamma = load_host<F>(gamma);
    ch.alpha = load_host<F>(alpha);
    ch.mu = load_host<F>(mu);
    return ch;
}

}  // namespace host
}  // namespace zk
