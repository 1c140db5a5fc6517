// plonk_lookup_columns_host.h -- the host side of the Plonk proof with lookup rows on COLUMN commitments (include/zkmle.h "Plonk with lookups
// on column commitments") that prover and verifier share: the statement's absorption (a tag of its own, the witness root, the circuit root, the
// public values), the root of M and the ONE root of the four helpers with the challenges behind them, and the verifier's replay.  The final
// relation is plonk_lookup_host.h's on the twenty claims as they stand: the global column order of the four commitments (3, 12, 1, 4) is the
// order of that proof's twenty; the rounds' replay is zerocheck_host.h's.  It touches no device; tools/plonk_lookup_columns_selftest.hip runs it under a sanitizer.  Library-internal;
// included by .hip files only.
#pragma once
#include "plonk_lookup_host.h"

namespace zk {
namespace host {

// the four commitments opened together: the witness (A, B, C), the circuit (qM, qL, qR, qO, qC, SA, SB, SC, qK, T0, T1, T2), M, the helpers
// (H0, H1, H2, HL)
constexpr uint32_t kPlonkColumnsCommits = 4, kPlonkColumnsWitness = 3, kPlonkColumnsCircuit = 12, kPlonkColumnsHelpers = 4;
constexpr uint32_t kPlonkColumnsWidths[kPlonkColumnsCommits] = {kPlonkColumnsWitness, kPlonkColumnsCircuit, 1, kPlonkColumnsHelpers};
static_assert(kPlonkColumnsWitness + kPlonkColumnsCircuit == kPlonkLookupGiven && kPlonkColumnsWitness + kPlonkColumnsCircuit + 1 + kPlonkColumnsHelpers == kPlonkLookupOpened,
              "the columns in global order are the twenty of plonk_lookup_host.h");

// steps 1 to 3: the tag, d and l in one append ("ZCLC": no other protocol of the library starts with these four bytes, so none's transcript is
// a prefix of this one's); the witness root, then the circuit root; the l public values
template <class F> void plonk_lookup_columns_statement(Transcript &tr, const uint8_t *witness_root, const uint8_t *circuit_root, uint32_t d, const uint64_t *pub,
                                                       uint32_t npublic) {
    uint8_t tag[12];
    memcpy(tag, "ZCLC", 4);
    put_be32(tag + 4, d);
    put_be32(tag + 8, npublic);
    tr.append(tag, sizeof tag);
    tr.append(witness_root, 32);
    tr.append(circuit_root, 32);
    for (uint32_t x = 0; x < npublic; x++) tr.append_be<F>(load_host<F>(pub + (size_t)x * (F::N / 2)));
}

// the end of step 6 and step 7: the ONE root of the four helper columns; then alpha, mu, tau_0 .. tau_{d-1}
template <class F> void plonk_lookup_columns_helpers(Transcript &tr, const uint8_t *h_root, uint32_t d, WiringChallenges<F> &ch) {
    tr.append(h_root, 32);
    ch.alpha = tr.random_challenge_as_field_element<F>();
    ch.mu = tr.random_challenge_as_field_element<F>();
    ch.tau.resize((size_t)d * (F::N / 2));
    for (uint32_t i = 0; i < d; i++) store_host<F>(ch.tau.data() + (size_t)i * (F::N / 2), tr.random_challenge_as_field_element<F>());
}

// plonk_lookup_replay with this protocol's statement and roots: h_roots: 64 bytes (M, then the helpers' one root); round_polys: 5 d elements,
// ys: 20.  z (d elements) receives the point, z[d - 1 - l] = r_l; *good = every check held and every element read is reduced.  The transcript
// advances the same way whatever *good is.  d <= 32.
template <class F> void plonk_lookup_columns_replay(Transcript &tr, const uint8_t *witness_root, const uint8_t *circuit_root, uint32_t d, const uint64_t *pub,
                                                    uint32_t npublic, const uint8_t *h_roots, const uint64_t *round_polys, const uint64_t *ys, uint64_t *z, bool *good) {
    constexpr int W = F::N / 2;
    WiringChallenges<F> ch;
    bool ok = true;
    for (uint32_t x = 0; x < npublic; x++) ok = ok && is_reduced<F>(pub + (size_t)x * W);
    plonk_lookup_columns_statement<F>(tr, witness_root, circuit_root, d, pub, npublic);
    plonk_lookup_multiplicity_root<F>(tr, h_roots, ch);
    plonk_lookup_columns_helpers<F>(tr, h_roots + 32, d, ch);
    const Fe<F> a3 = fe_mul<F>(ch.alpha, fe_mul<F>(ch.alpha, ch.alpha));
    const Fe<F> claim0 = fe_mul<F>(a3, plonk_public_eval<F>(pub, npublic, ch.tau.data(), d));
    const Fe<F> last = replay_rounds<F, kPlonkNodes>(tr, d, claim0, round_polys, z, ok);
    const Fe<F> eq = eq_at<F>(z, ch.tau.data(), d);
    Fe<F> y[kPlonkLookupOpened];
    load_claims<F>(ys, kPlonkLookupOpened, y, ok);
    *good = ok && fe_eq<F>(last, plonk_lookup_relation<F>(ch, y, eq, wiring_id_at<F>(z, d), d));
}

}  // namespace host
}  // namespace zk
