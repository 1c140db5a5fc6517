// lookup_host.h -- the host side of the lookup argument over FRI commitments (include/zkmle.h "Lookup: rows of a committed table") that prover
// and verifier share: the statement's absorption, the two helper roots and the challenges behind them, the final relation, and the verifier's
// replay.  The round message is wiring_host.h's (the same seven sums), the interpolation and the rounds' replay zerocheck_host.h's.  It touches no device;
// tools/lookup_selftest.hip runs it under a sanitizer.  Library-internal; included by .hip files only.
#pragma once
#include "wiring_host.h"

namespace zk {
namespace host {

constexpr int kLookupGiven = 7, kLookupHelpers = 2, kLookupOpened = 9;   // A, B, C, qK, T0, T1, T2; M, H

template <class F> struct LookupChallenges {
    Fe<F> beta, gamma, mu;
    std::vector<uint64_t> tau;                               // d elements, u64 limbs
};

// step 1: the tag, d, the seven roots (A, B, C, qK, T0, T1, T2)
inline void lookup_statement(Transcript &tr, const uint8_t *roots, uint32_t d) {
    uint8_t tag[8];
    memcpy(tag, "ZCLK", 4);
    put_be32(tag + 4, d);
    tr.append(tag, sizeof tag);
    for (int j = 0; j < kLookupGiven; j++) tr.append(roots + 32 * j, 32);
}

// the end of step 2 and step 3: the root of M; then beta, gamma
template <class F> void lookup_multiplicity_root(Transcript &tr, const uint8_t *m_root, LookupChallenges<F> &ch) {
    tr.append(m_root, 32);
    ch.beta = tr.random_challenge_as_field_element<F>();
    ch.gamma = tr.random_challenge_as_field_element<F>();
}

// the end of step 4 and step 5: the root of H; then mu, tau_0 .. tau_{d-1}
template <class F> void lookup_helper_root(Transcript &tr, const uint8_t *h_root, uint32_t d, LookupChallenges<F> &ch) {
    tr.append(h_root, 32);
    ch.mu = tr.random_challenge_as_field_element<F>();
    ch.tau.resize((size_t)d * (F::N / 2));
    for (uint32_t i = 0; i < d; i++) store_host<F>(ch.tau.data() + (size_t)i * (F::N / 2), tr.random_challenge_as_field_element<F>());
}

// mu yH + eq (yH dw dt - yqK dt + yM dw);  y: the nine claims A, B, C, qK, T0, T1, T2, M, H
template <class F> Fe<F> lookup_relation(const LookupChallenges<F> &ch, const Fe<F> *y, const Fe<F> &eq) {
    const Fe<F> g2 = fe_mul<F>(ch.gamma, ch.gamma);
    const Fe<F> dw = fe_add<F>(fe_add<F>(ch.beta, y[0]), fe_add<F>(fe_mul<F>(ch.gamma, y[1]), fe_mul<F>(g2, y[2])));
    const Fe<F> dt = fe_add<F>(fe_add<F>(ch.beta, y[4]), fe_add<F>(fe_mul<F>(ch.gamma, y[5]), fe_mul<F>(g2, y[6])));
    const Fe<F> zc = fe_add<F>(fe_mul<F>(dt, fe_sub<F>(fe_mul<F>(y[8], dw), y[3])), fe_mul<F>(y[7], dw));
    return fe_add<F>(fe_mul<F>(ch.mu, y[8]), fe_mul<F>(eq, zc));
}

// The verifier's replay of steps 1 to 6 on `tr` and its checks: g_0(0) + g_0(1) = 0, g_l(0) + g_l(1) = g_{l-1}(r_{l-1}), and g_{d-1}(r_{d-1}) =
// the relation on the nine claims.  round_polys: 5 d elements, ys: 9, h_roots: 64 bytes (M, then H).  z (d elements) receives the point,
// z[d - 1 - l] = r_l; *good = every check held and every element read is reduced.  The transcript advances the same way whatever *good is.
template <class F> void lookup_replay(Transcript &tr, const uint8_t *roots, uint32_t d, const uint8_t *h_roots, const uint64_t *round_polys, const uint64_t *ys, uint64_t *z,
                                      bool *good) {
    LookupChallenges<F> ch;
    lookup_statement(tr, roots, d);
    lookup_multiplicity_root<F>(tr, h_roots, ch);
    lookup_helper_root<F>(tr, h_roots + 32, d, ch);
    bool ok = true;
    const Fe<F> last = replay_rounds<F, kWiringNodes>(tr, d, fe_zero<F>(), round_polys, z, ok);
    const Fe<F> eq = eq_at<F>(z, ch.tau.data(), d);
    Fe<F> y[kLookupOpened];
    load_claims<F>(ys, kLookupOpened, y, ok);
    *good = ok && fe_eq<F>(last, lookup_relation<F>(ch, y, eq));
}

}  // namespace host
}  // namespace zk
