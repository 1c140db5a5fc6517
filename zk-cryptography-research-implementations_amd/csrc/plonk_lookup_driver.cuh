// plonk_lookup_driver.cuh -- what the two provers of the Plonk proof with lookup rows share (zkmle_plonk_lookup.hip on fifteen commitments,
// zkmle_plonk_lookup_columns.hip on column commitments): the launch of the round pass.  Defined and instantiated for the two scalar fields in
// zkmle_plonk_lookup.hip, so plonk_lookup_round_kernel is compiled once.  Library-internal; included by .hip files only.
#pragma once
#include "plonk_lookup.cuh"
#include "wiring_host.h"

namespace zk {
namespace host {

// sums (device, 7 elements) of a pass over q pairs whose id tables are c_l + 2^l x + j 2^d.  Launches only.
template <class F> int plonk_lookup_launch_round(bool fold, const PlonkLookupTables &t, size_t q, const Fe<F> &r, const WiringChallenges<F> &ch, const Fe<F> &id_base,
                                                 unsigned log_step, unsigned d, void *partials, void *sums);

}  // namespace host
}  // namespace zk
