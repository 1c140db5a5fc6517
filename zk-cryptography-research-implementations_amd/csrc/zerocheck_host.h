// zerocheck_host.h -- the host side of the zerochecks over FRI commitments (include/zkmle.h "Zerocheck of a product of committed tables" and
// "Zerocheck of a Plonk gate over committed tables") that prover and verifier share: the statement's absorption, the round message from the
// pass's sums, and the verifier's replay of the sumcheck.  The replay's three parts that do not depend on the protocol (replay_rounds, eq_at,
// load_claims) serve the whole family: wiring_host.h, plonk_host.h, lookup_host.h, plonk_lookup_host.h and plonk_lookup_columns_host.h call
// them between their own statement and their own relation.  The two protocols here differ in a statement (ZerocheckMul, ZerocheckGate): the tag, the
// number of commitments K, the number of nodes a round message is sent at, how the message comes from the pass's sums, and the relation the
// last check evaluates on the K claims.  It touches no device; tools/zerocheck_selftest.hip runs it under a sanitizer.  Library-internal;
// included by .hip files only.
#pragma once
#include <string.h>

#include <vector>

#include "host_util.h"
#include "transcript.h"

namespace zk {
namespace host {

// g(0), g(1), g(2), g(3) from the pass's sums at the nodes 0, 1, 2 and infinity: g(3) = 3 g(2) - 3 g(1) + g(0) + 6 s_inf
template <class F> void zerocheck_g4(const Fe<F> S[4], Fe<F> g[4]) {
    g[0] = S[0];
    g[1] = S[1];
    g[2] = S[2];
    const Fe<F> t = fe_add<F>(fe_sub<F>(S[2], S[1]), fe_dbl<F>(S[3]));   // g(2) - g(1) + 2 s_inf
    g[3] = fe_add<F>(fe_add<F>(fe_dbl<F>(t), t), S[0]);
}

// g(0) .. g(4) from the pass's sums at the nodes 0, 1, 2, 3 and infinity: g(4) = 4 g(3) - 6 g(2) + 4 g(1) - g(0) + 24 s_inf
template <class F> void zerocheck_g5(const Fe<F> S[5], Fe<F> g[5]) {
    for (int k = 0; k < 4; k++) g[k] = S[k];
    const Fe<F> a = fe_add<F>(S[3], S[1]), s4 = fe_dbl<F>(fe_dbl<F>(S[4]));                     // g(3) + g(1); 4 s_inf
    const Fe<F> s12 = fe_add<F>(fe_dbl<F>(s4), s4), g2x3 = fe_add<F>(fe_dbl<F>(S[2]), S[2]);
    const Fe<F> t = fe_sub<F>(fe_add<F>(fe_dbl<F>(a), s12), g2x3);                              // 2 (g(3) + g(1)) - 3 g(2) + 12 s_inf
    g[4] = fe_sub<F>(fe_dbl<F>(t), S[0]);
}

// the polynomial of degree NODES - 1 through (0, g[0]) .. (NODES - 1, g[NODES - 1]) at r, by Lagrange's formula
template <class F, int NODES> Fe<F> zerocheck_interpolate_at(const Fe<F> *g, const Fe<F> &r) {
    Fe<F> node[NODES], out = fe_zero<F>();
    for (int j = 0; j < NODES; j++) node[j] = fe_from_u64<F>((uint64_t)j);
    for (int i = 0; i < NODES; i++) {
        Fe<F> num = g[i], den = fe_one<F>();
        for (int j = 0; j < NODES; j++) {
            if (j == i) continue;
            num = fe_mul<F>(num, fe_sub<F>(r, node[j]));
            den = fe_mul<F>(den, fe_sub<F>(node[i], node[j]));
        }
        out = fe_add<F>(out, fe_mul<F>(num, fe_inv<F>(den)));
    }
    return out;
}

// A o B = C over (A, B, C): a cubic at the nodes 0 .. 3
struct ZerocheckMul {
    static constexpr int K = 3, NODES = 4;
    static constexpr const char *tag = "ZCML";
    template <class F> static void message(const Fe<F> *S, Fe<F> *g) { zerocheck_g4<F>(S, g); }
    template <class F> static Fe<F> relation(const Fe<F> *y) { return fe_sub<F>(fe_mul<F>(y[0], y[1]), y[2]); }
};

// qM A B + qL A + qR B + qO C + qC = 0 over (A, B, C, qM, qL, qR, qO, qC): a quartic at the nodes 0 .. 4
struct ZerocheckGate {
    static constexpr int K = 8, NODES = 5;
    static constexpr const char *tag = "ZCPG";
    template <class F> static void message(const Fe<F> *S, Fe<F> *g) { zerocheck_g5<F>(S, g); }
    template <class F> static Fe<F> relation(const Fe<F> *y) {
        const Fe<F> ab = fe_add<F>(fe_mul<F>(fe_add<F>(fe_mul<F>(y[3], y[1]), y[4]), y[0]), fe_mul<F>(y[5], y[1]));   // (qM B + qL) A + qR B
        return fe_add<F>(fe_add<F>(ab, fe_mul<F>(y[6], y[2])), y[7]);
    }
};

// steps 1 and 2: the tag, d, the K roots; then tau_0 .. tau_{d-1} (tau: d elements, u64 limbs)
template <class F, class St> void zerocheck_statement(Transcript &tr, const uint8_t *roots, uint32_t d, uint64_t *tau) {
    uint8_t tag[8];
    memcpy(tag, St::tag, 4);
    put_be32(tag + 4, d);
    tr.append(tag, sizeof tag);
    for (int j = 0; j < St::K; j++) tr.append(roots + 32 * j, 32);
    for (uint32_t i = 0; i < d; i++) store_host<F>(tau + (size_t)i * (F::N / 2), tr.random_challenge_as_field_element<F>());
}

// The verifier's replay of the d rounds on `tr`, for every protocol of the family: each round's NODES elements are read, checked for reducedness
// and absorbed, g_l(0) + g_l(1) is checked against the running claim (claim0 at round 0), r_l is drawn and the claim becomes g_l(r_l).  z (d
// elements) receives the point, z[d - 1 - l] = r_l; a failed check clears `ok`.  Returns g_{d-1}(r_{d-1}).  The transcript advances the same
// way whatever `ok` is.
template <class F, int NODES> Fe<F> replay_rounds(Transcript &tr, uint32_t d, const Fe<F> &claim0, const uint64_t *round_polys, uint64_t *z, bool &ok) {
    constexpr int W = F::N / 2;
    Fe<F> cur = claim0;
    for (uint32_t l = 0; l < d; l++) {
        Fe<F> g[NODES];
        for (int k = 0; k < NODES; k++) {
            const uint64_t *src = round_polys + ((size_t)l * NODES + k) * W;
            ok = ok && is_reduced<F>(src);
            g[k] = load_host<F>(src);
            tr.append_be<F>(g[k]);
        }
        ok = ok && fe_eq<F>(fe_add<F>(g[0], g[1]), cur);
        const Fe<F> r = tr.random_challenge_as_field_element<F>();
        store_host<F>(z + (size_t)(d - 1 - l) * W, r);
        cur = zerocheck_interpolate_at<F, NODES>(g, r);
    }
    return cur;
}

// eq(z, tau) = prod_i (z_i tau_i + (1 - z_i)(1 - tau_i)); z, tau: d elements, u64 limbs
template <class F> Fe<F> eq_at(const uint64_t *z, const uint64_t *tau, uint32_t d) {
    constexpr int W = F::N / 2;
    const Fe<F> one = fe_one<F>();
    Fe<F> eq = one;
    for (uint32_t i = 0; i < d; i++) {
        const Fe<F> a = load_host<F>(z + (size_t)i * W), b = load_host<F>(tau + (size_t)i * W);
        eq = fe_mul<F>(eq, fe_add<F>(fe_mul<F>(a, b), fe_mul<F>(fe_sub<F>(one, a), fe_sub<F>(one, b))));
    }
    return eq;
}

// y = the K claims ys; one that is not reduced clears `ok`
template <class F> void load_claims(const uint64_t *ys, int K, Fe<F> *y, bool &ok) {
    for (int j = 0; j < K; j++) {
        ok = ok && is_reduced<F>(ys + (size_t)j * (F::N / 2));
        y[j] = load_host<F>(ys + (size_t)j * (F::N / 2));
    }
}

// The verifier's replay of the statement and the rounds on `tr` and its three checks: g_0(0) + g_0(1) = 0, g_l(0) + g_l(1) = g_{l-1}(r_{l-1}),
// and g_{d-1}(r_{d-1}) = eq(z, tau) relation(ys).  round_polys: NODES d elements, ys: K.  z (d elements) receives the point,
// z[d - 1 - l] = r_l; *good = every check held and every element read is reduced.  The transcript advances the same way whatever *good is.
template <class F, class St> void zerocheck_replay(Transcript &tr, const uint8_t *roots, uint32_t d, const uint64_t *round_polys, const uint64_t *ys, uint64_t *z, bool *good) {
    std::vector<uint64_t> tau((size_t)d * (F::N / 2));
    zerocheck_statement<F, St>(tr, roots, d, tau.data());
    bool ok = true;
    const Fe<F> last = replay_rounds<F, St::NODES>(tr, d, fe_zero<F>(), round_polys, z, ok);
    const Fe<F> eq = eq_at<F>(z, tau.data(), d);
    Fe<F> y[St::K];
    load_claims<F>(ys, St::K, y, ok);
    *good = ok && fe_eq<F>(last, fe_mul<F>(eq, St::template relation<F>(y)));
}

}  // namespace host
}  // namespace zk
