// wiring_host.h -- the host side of the permutation check over FRI commitments (include/zkmle.h "Wiring: a permutation check over committed
// tables") that prover and verifier share: the statement's absorption and its challenges, the round message from the pass's seven sums, the
// closed form of the id tables at a point, the final relation, and the verifier's replay.  The round message, the interpolation and the
// replay of the rounds themselves (replay_rounds, eq_at, load_claims) are zerocheck_host.h's.  It touches no device; tools/wiring_selftest.hip runs it under a sanitizer.  Library-internal; included by .hip files only.
#pragma once
#include "zerocheck_host.h"

namespace zk {
namespace host {

constexpr int kWiringWires = 3, kWiringGiven = 6, kWiringOpened = 9, kWiringNodes = 5, kWiringSums = 7;

template <class F> struct WiringChallenges {
    Fe<F> beta, gamma, alpha, mu;
    std::vector<uint64_t> tau;                               // d elements, u64 limbs
};

// step 1 and 2: the tag, d, the six roots (A, B, C, SA, SB, SC); then beta, gamma
template <class F> void wiring_statement(Transcript &tr, const uint8_t *roots, uint32_t d, WiringChallenges<F> &ch) {
    uint8_t tag[8];
    memcpy(tag, "ZCPW", 4);
    put_be32(tag + 4, d);
    tr.append(tag, sizeof tag);
    for (int j = 0; j < kWiringGiven; j++) tr.append(roots + 32 * j, 32);
    ch.beta = tr.random_challenge_as_field_element<F>();
    ch.gamma = tr.random_challenge_as_field_element<F>();
}

// the end of step 3 and step 4: the three roots of H0, H1, H2; then alpha, mu, tau_0 .. tau_{d-1}
template <class F> void wiring_helpers(Transcript &tr, const uint8_t *h_roots, uint32_t d, WiringChallenges<F> &ch) {
    for (int j = 0; j < kWiringWires; j++) tr.append(h_roots + 32 * j, 32);
    ch.alpha = tr.random_challenge_as_field_element<F>();
    ch.mu = tr.random_challenge_as_field_element<F>();
    ch.tau.resize((size_t)d * (F::N / 2));
    for (uint32_t i = 0; i < d; i++) store_host<F>(ch.tau.data() + (size_t)i * (F::N / 2), tr.random_challenge_as_field_element<F>());
}

// g(0) .. g(4) from the pass's sums s_0, s_1, s_2, s_3, s_inf, s_ev, s_od: mu times the line through (0, s_ev), (1, s_od) joins the node
// values; a line has no share in the fourth difference
template <class F> void wiring_message(const Fe<F> S[kWiringSums], const Fe<F> &mu, Fe<F> g[kWiringNodes]) {
    Fe<F> T[kWiringNodes], line = fe_mul<F>(mu, S[5]);
    const Fe<F> step = fe_mul<F>(mu, fe_sub<F>(S[6], S[5]));
    for (int k = 0; k < 4; k++) {
        T[k] = fe_add<F>(S[k], line);
        line = fe_add<F>(line, step);
    }
    T[4] = S[4];
    zerocheck_g5<F>(T, g);
}

// the multilinear extension of id_0[x] = x at z: sum_i 2^(d-1-i) z_i (variable 0 is the most significant index bit); id_j = j 2^d + id_0
template <class F> Fe<F> wiring_id_at(const uint64_t *z, uint32_t d) {
    Fe<F> acc = fe_zero<F>();
    for (uint32_t i = 0; i < d; i++) acc = fe_add<F>(fe_dbl<F>(acc), load_host<F>(z + (size_t)i * (F::N / 2)));
    return acc;
}

// mu (yH0 + yH1 + yH2) + eq sum_j alpha^j (yH_j (beta + yW_j + gamma id_j) (beta + yW_j + gamma yS_j) - gamma (yS_j - id_j));
// y: the nine claims A, B, C, SA, SB, SC, H0, H1, H2; id0 = wiring_id_at(z)
template <class F> Fe<F> wiring_relation(const WiringChallenges<F> &ch, const Fe<F> *y, const Fe<F> &eq, const Fe<F> &id0, uint32_t d) {
    const Fe<F> wire = fe_from_u64<F>((uint64_t)1 << d);
    Fe<F> id = id0, apow = fe_one<F>(), zc = fe_zero<F>(), hs = fe_zero<F>();
    for (int j = 0; j < kWiringWires; j++) {
        const Fe<F> bw = fe_add<F>(ch.beta, y[j]), gs = fe_mul<F>(ch.gamma, y[3 + j]), gi = fe_mul<F>(ch.gamma, id);
        const Fe<F> term = fe_sub<F>(fe_mul<F>(y[6 + j], fe_mul<F>(fe_add<F>(bw, gi), fe_add<F>(bw, gs))), fe_sub<F>(gs, gi));
        zc = fe_add<F>(zc, fe_mul<F>(apow, term));
        hs = fe_add<F>(hs, y[6 + j]);
        apow = fe_mul<F>(apow, ch.alpha);
        id = fe_add<F>(id, wire);
    }
    return fe_add<F>(fe_mul<F>(ch.mu, hs), fe_mul<F>(eq, zc));
}

// The verifier's replay of steps 1 to 5 on `tr` and its checks: g_0(0) + g_0(1) = 0, g_l(0) + g_l(1) = g_{l-1}(r_{l-1}), and g_{d-1}(r_{d-1}) =
// the relation on the nine claims.  round_polys: 5 d elements, ys: 9, h_roots: 96 bytes.  z (d elements) receives the point, z[d - 1 - l] = r_l;
// *good = every check held and every element read is reduced.  The transcript advances the same way whatever *good is.  d <= 32.
template <class F> void wiring_replay(Transcript &tr, const uint8_t *roots, uint32_t d, const uint8_t *h_roots, const uint64_t *round_polys, const uint64_t *ys, uint64_t *z,
                                      bool *good) {
    WiringChallenges<F> ch;
    wiring_statement<F>(tr, roots, d, ch);
    wiring_helpers<F>(tr, h_roots, d, ch);
    bool ok = true;
    const Fe<F> last = replay_rounds<F, kWiringNodes>(tr, d, fe_zero<F>(), round_polys, z, ok);
    const Fe<F> eq = eq_at<F>(z, ch.tau.data(), d);
    Fe<F> y[kWiringOpened];
    load_claims<F>(ys, kWiringOpened, y, ok);
    *good = ok && fe_eq<F>(last, wiring_relation<F>(ch, y, eq, wiring_id_at<F>(z, d), d));
}

}  // namespace host
}  // namespace zk
