// plonk_lookup_host.h -- the host side of the Plonk proof with lookup rows (include/zkmle.h "Plonk with lookups: gate, wiring, public inputs and
// lookup rows in one sumcheck") that prover and verifier share: the statement's absorption, the roots of M and of the four helper tables with the
// challenges behind them, the final relation and the verifier's replay.  The public inputs' value, the gate's and the wiring's relation are
// plonk_host.h's, the lookup's relation lookup_host.h's, the round message wiring_host.h's, the rounds' replay
// zerocheck_host.h's.  It touches no device; tools/plonk_lookup_selftest.hip runs it under a sanitizer.  Library-internal; included by .hip files only.
#pragma once
#include "lookup_host.h"
#include "plonk_host.h"

namespace zk {
namespace host {

// A, B, C, qM, qL, qR, qO, qC, SA, SB, SC, qK, T0, T1, T2;  M, H0, H1, H2, HL
constexpr int kPlonkLookupGiven = 15, kPlonkLookupHelpers = 5, kPlonkLookupOpened = 20;
// the places of the plonk proof's fourteen (.., SA, SB, SC, H0, H1, H2) and of the lookup's nine (A, B, C, qK, T0, T1, T2, M, H) among the twenty
constexpr int kPlonkLookupPlonkPlace[kPlonkOpened] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16, 17, 18};
constexpr int kPlonkLookupLookupPlace[kLookupOpened] = {0, 1, 2, 11, 12, 13, 14, 15, 19};

// steps 1 to 3: the tag, d and l in one append; the fifteen roots; the l public values
template <class F> void plonk_lookup_statement(Transcript &tr, const uint8_t *roots, uint32_t d, const uint64_t *pub, uint32_t npublic) {
    uint8_t tag[12];
    memcpy(tag, "ZCPL", 4);
    put_be32(tag + 4, d);
    put_be32(tag + 8, npublic);
    tr.append(tag, sizeof tag);
    for (int j = 0; j < kPlonkLookupGiven; j++) tr.append(roots + 32 * j, 32);
    for (uint32_t x = 0; x < npublic; x++) tr.append_be<F>(load_host<F>(pub + (size_t)x * (F::N / 2)));
}

// the end of step 4 and step 5: the root of M; then beta, gamma -- ONE pair for the wiring and the lookup
template <class F> void plonk_lookup_multiplicity_root(Transcript &tr, const uint8_t *m_root, WiringChallenges<F> &ch) {
    tr.append(m_root, 32);
    ch.beta = tr.random_challenge_as_field_element<F>();
    ch.gamma = tr.random_challenge_as_field_element<F>();
}

// the end of step 6 and step 7: the roots of H0, H1, H2, HL (128 bytes); then alpha, mu, tau_0 .. tau_{d-1}
template <class F> void plonk_lookup_helpers(Transcript &tr, const uint8_t *h4_roots, uint32_t d, WiringChallenges<F> &ch) {
    for (int j = 0; j < kWiringWires + 1; j++) tr.append(h4_roots + 32 * j, 32);
    ch.alpha = tr.random_challenge_as_field_element<F>();
    ch.mu = tr.random_challenge_as_field_element<F>();
    ch.tau.resize((size_t)d * (F::N / 2));
    for (uint32_t i = 0; i < d; i++) store_host<F>(ch.tau.data() + (size_t)i * (F::N / 2), tr.random_challenge_as_field_element<F>());
}

// plonk_relation on the fourteen + eq alpha^4 (the lookup's bracket) + mu^2 yHL, on the twenty claims: lookup_relation is called with mu^2 in
// mu's place and eq alpha^4 in eq's
template <class F> Fe<F> plonk_lookup_relation(const WiringChallenges<F> &ch, const Fe<F> *y, const Fe<F> &eq, const Fe<F> &id0, uint32_t d) {
    Fe<F> fourteen[kPlonkOpened], nine[kLookupOpened];
    for (int j = 0; j < kPlonkOpened; j++) fourteen[j] = y[kPlonkLookupPlonkPlace[j]];
    for (int j = 0; j < kLookupOpened; j++) nine[j] = y[kPlonkLookupLookupPlace[j]];
    const Fe<F> a2 = fe_mul<F>(ch.alpha, ch.alpha);
    LookupChallenges<F> lc;
    lc.beta = ch.beta;
    lc.gamma = ch.gamma;
    lc.mu = fe_mul<F>(ch.mu, ch.mu);
    return fe_add<F>(plonk_relation<F>(ch, fourteen, eq, id0, d), lookup_relation<F>(lc, nine, fe_mul<F>(eq, fe_mul<F>(a2, a2))));
}

// The verifier's replay of steps 1 to 9 on `tr` and its checks: g_0(0) + g_0(1) = alpha^3 PIeval(tau), g_l(0) + g_l(1) = g_{l-1}(r_{l-1}), and
// g_{d-1}(r_{d-1}) = the relation on the twenty claims.  round_polys: 5 d elements, ys: 20, h_roots: 160 bytes (M, H0, H1, H2, HL), pub: npublic
// <= 2^d elements.  z (d elements) receives the point, z[d - 1 - l] = r_l; *good = every check held and every element read is reduced, the
// public values among them.  The transcript advances the same way whatever *good is.  d <= 32.
template <class F> void plonk_lookup_replay(Transcript &tr, const uint8_t *roots, uint32_t d, const uint64_t *pub, uint32_t npublic, const uint8_t *h_roots,
                                            const uint64_t *round_polys, const uint64_t *ys, uint64_t *z, bool *good) {
    constexpr int W = F::N / 2;
    WiringChallenges<F> ch;
    bool ok = true;
    for (uint32_t x = 0; x < npublic; x++) ok = ok && is_reduced<F>(pub + (size_t)x * W);
    plonk_lookup_statement<F>(tr, roots, d, pub, npublic);
    plonk_lookup_multiplicity_root<F>(tr, h_roots, ch);
    plonk_lookup_helpers<F>(tr, h_roots + 32, d, ch);
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
