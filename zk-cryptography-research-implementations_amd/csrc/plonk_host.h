// plonk_host.h -- the host side of the Plonk proof (include/zkmle.h "Plonk: gate, wiring and public inputs in one sumcheck") that prover and
// verifier share: the statement's absorption, the public inputs' value at tau (the claimed sum), the final relation and the verifier's replay.
// The helper step, the round message, the id tables' closed form and the wiring's relation are wiring_host.h's, the gate's relation, the
// interpolation and the rounds' replay zerocheck_host.h's.  It touches no device; tools/plonk_selftest.hip runs it under a sanitizer.  Library-internal; included by
// .hip files only.
#pragma once
#include "wiring_host.h"

namespace zk {
namespace host {

constexpr int kPlonkGiven = 11, kPlonkOpened = 14, kPlonkNodes = kWiringNodes;
// the places of the wiring's nine (A, B, C, SA, SB, SC, H0, H1, H2) among the fourteen (A, B, C, qM, qL, qR, qO, qC, SA, SB, SC, H0, H1, H2)
constexpr int kPlonkWiringPlace[kWiringOpened] = {0, 1, 2, 8, 9, 10, 11, 12, 13};

// the public inputs' shape, which prover and verifier refuse alike: npublic <= 2^d, a NULL array only with npublic = 0
inline bool plonk_public_shape_ok(const uint64_t *pub, uint32_t npublic, uint32_t d) { return (d >= 32 || npublic <= ((uint32_t)1 << d)) && (pub || npublic == 0); }

// steps 1 to 4: the tag, d and l; the eleven roots; the l public values (each the 32-byte canonical big-endian element); then beta, gamma
template <class F> void plonk_statement(Transcript &tr, const uint8_t *roots, uint32_t d, const uint64_t *pub, uint32_t npublic, WiringChallenges<F> &ch) {
    uint8_t tag[12];
    memcpy(tag, "ZCPK", 4);
    put_be32(tag + 4, d);
    put_be32(tag + 8, npublic);
    tr.append(tag, sizeof tag);
    for (int j = 0; j < kPlonkGiven; j++) tr.append(roots + 32 * j, 32);
    for (uint32_t x = 0; x < npublic; x++) tr.append_be<F>(load_host<F>(pub + (size_t)x * (F::N / 2)));
    ch.beta = tr.random_challenge_as_field_element<F>();
    ch.gamma = tr.random_challenge_as_field_element<F>();
}

// sum_{lo <= x < min(l, lo + 2^(d-i))} pi_x eq(x, tau) / eq of the i variables already walked: the subtree below the first i index bits.  A
// subtree that starts at or past l is zero and is not entered, so 2 l + d nodes are visited: one product each, d frames deep.
template <class F> Fe<F> plonk_public_walk(const uint64_t *pub, uint64_t l, const uint64_t *tau, uint32_t d, uint32_t i, uint64_t lo) {
    if (lo >= l) return fe_zero<F>();
    if (i == d) return load_host<F>(pub + (size_t)lo * (F::N / 2));
    const Fe<F> left = plonk_public_walk<F>(pub, l, tau, d, i + 1, lo);
    const Fe<F> right = plonk_public_walk<F>(pub, l, tau, d, i + 1, lo + ((uint64_t)1 << (d - 1 - i)));
    return fe_add<F>(left, fe_mul<F>(load_host<F>(tau + (size_t)i * (F::N / 2)), fe_sub<F>(right, left)));
}
// PIeval(tau) = sum_{x < l} pi_x eq(x, tau), variable 0 the most significant index bit; l <= 2^d, d <= 32.  O(l + d) products.
template <class F> Fe<F> plonk_public_eval(const uint64_t *pub, uint64_t l, const uint64_t *tau, uint32_t d) { return plonk_public_walk<F>(pub, l, tau, d, 0, 0); }

// mu (yH0 + yH1 + yH2) + eq [ the wiring's bracket + alpha^3 (y_qM y_A y_B + y_qL y_A + y_qR y_B + y_qO y_C + y_qC) ] on the fourteen claims
template <class F> Fe<F> plonk_relation(const WiringChallenges<F> &ch, const Fe<F> *y, const Fe<F> &eq, const Fe<F> &id0, uint32_t d) {
    Fe<F> nine[kWiringOpened];
    for (int j = 0; j < kWiringOpened; j++) nine[j] = y[kPlonkWiringPlace[j]];
    const Fe<F> a3 = fe_mul<F>(ch.alpha, fe_mul<F>(ch.alpha, ch.alpha));
    return fe_add<F>(wiring_relation<F>(ch, nine, eq, id0, d), fe_mul<F>(eq, fe_mul<F>(a3, ZerocheckGate::relation<F>(y))));
}

// The verifier's replay of steps 1 to 7 on `tr` and its checks: g_0(0) + g_0(1) = alpha^3 PIeval(tau), g_l(0) + g_l(1) = g_{l-1}(r_{l-1}), and
// g_{d-1}(r_{d-1}) = the relation on the fourteen claims.  round_polys: 5 d elements, ys: 14, h_roots: 96 bytes, pub: npublic <= 2^d elements.
// z (d elements) receives the point, z[d - 1 - l] = r_l; *good = every check held and every element read is reduced, the public values among them.
// The transcript advances the same way whatever *good is.  d <= 32.
template <class F> void plonk_replay(Transcript &tr, const uint8_t *roots, uint32_t d, const uint64_t *pub, uint32_t npublic, const uint8_t *h_roots,
                                     const uint64_t *round_polys, const uint64_t *ys, uint64_t *z, bool *good) {
    constexpr int W = F::N / 2;
    WiringChallenges<F> ch;
    bool ok = true;
    for (uint32_t x = 0; x < npublic; x++) ok = ok && is_reduced<F>(pub + (size_t)x * W);
    plonk_statement<F>(tr, roots, d, pub, npublic, ch);
    wiring_helpers<F>(tr, h_roots, d, ch);
    const Fe<F> a3 = fe_mul<F>(ch.alpha, fe_mul<F>(ch.alpha, ch.alpha));
    const Fe<F> claim0 = fe_mul<F>(a3, plonk_public_eval<F>(pub, npublic, ch.tau.data(), d));
    const Fe<F> last = replay_rounds<F, kPlonkNodes>(tr, d, claim0, round_polys, z, ok);
    const Fe<F> eq = eq_at<F>(z, ch.tau.data(), d);
    Fe<F> y[kPlonkOpened];
    load_claims<F>(ys, kPlonkOpened, y, ok);
    *good = ok && fe_eq<F>(last, plonk_relation<F>(ch, y, eq, wiring_id_at<F>(z, d), d));
}

}  // namespace host
}  // namespace zk
