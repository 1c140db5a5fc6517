// plonk_lookup_driver.cuh -- what the two provers of the Plonk proof with lookup rows share (zkmle_plonk_lookup.hip on fifteen commitments,
// zkmle_plonk_lookup_columns.hip on column commitments): the launch of the round pass, defined and instantiated for the two scalar fields in
// zkmle_plonk_lookup.hip, so plonk_lookup_round_kernel is compiled once; and their rounds on zerocheck_driver.cuh's driver.  Library-internal;
// included by .hip files only.
#pragma once
#include "plonk_host.h"
#include "plonk_lookup.cuh"
#include "wiring_driver.cuh"

namespace zk {
namespace host {

// sums (device, 7 elements) of a pass over q pairs whose id tables are c_l + 2^l x + j 2^d.  Launches only.
template <class F> int plonk_lookup_launch_round(bool fold, const PlonkLookupTables &t, size_t q, const Fe<F> &r, const WiringChallenges<F> &ch, const Fe<F> &id_base,
                                                 unsigned log_step, unsigned d, void *partials, void *sums);

// zerocheck_driver.cuh's launch on the twenty-one tables, folded to out0 + j ostride
template <class F> int plonk_lookup_pass(bool fold, const void *const *in, void *out0, size_t ostride, size_t q, const Fe<F> &r, const WiringChallenges<F> &ch, const Fe<F> &id_base,
                                         unsigned log_step, unsigned d, void *partials, void *sums) {
    PlonkLookupTables t{};
    for (int j = 0; j < kPlonkLookupTables; j++) t.in[j] = in[j];
    t.out0 = out0;
    t.ostride = ostride;
    return plonk_lookup_launch_round<F>(fold, t, q, r, ch, id_base, log_step, d, partials, sums);
}

// E_0 and the d rounds of either prover on the twenty tables `opened` (A .. T2, M, H0, H1, H2, HL) and E: zerocheck_driver.cuh's prove_rounds
template <class F> int plonk_lookup_rounds(const void *const *opened, unsigned d, const WiringChallenges<F> &ch, Transcript &tr, uint64_t *round_polys, uint64_t *challenges,
                                           uint64_t *z, Events &ev, const size_t *from, float *ms_eq, float *ms_rounds) {
    IdBase<F> idb;
    const auto launch = [&](bool fold, const void *const *in, void *out0, size_t ostride, size_t q, const Fe<F> &r, unsigned l, void *partials, void *sums) {
        return plonk_lookup_pass<F>(fold, in, out0, ostride, q, r, ch, idb.at(l, r), l, d, partials, sums);
    };
    return prove_rounds<F, kPlonkLookupTables, kWiringSums, kPlonkNodes>(opened, d, ch.tau.data(), tr, launch, [&](const Fe<F> *S, Fe<F> *g) { wiring_message<F>(S, ch.mu, g); },
                                                                         round_polys, challenges, z, ev, from, ms_eq, ms_rounds);
}

}  // namespace host
}  // namespace zk
