// zerocheck_host.h -- the host side of the zerocheck of a product (include/zkmle.h "Zerocheck of a product of committed tables") that prover
// and verifier share: the statement's absorption, the round message from the pass's sums, and the verifier's replay of the sumcheck.  It
// touches no device; tools/zerocheck_selftest.hip runs it under a sanitizer.  Library-internal; included by .hip files only.
#pragma once
#include "host_util.h"
#include "transcript.h"

namespace zk {
namespace host {

// steps 1 and 2: "ZCML", d, the roots of A, B, C; then tau_0 .. tau_{d-1} (tau: d elements, u64 limbs)
template <class F> void zerocheck_statement(Transcript &tr, const uint8_t *roots96, uint32_t d, uint64_t *tau) {
    uint8_t tag[8] = {'Z', 'C', 'M', 'L'};
    put_be32(tag + 4, d);
    tr.append(tag, sizeof tag);
    for (int j = 0; j < 3; j++) tr.append(roots96 + 32 * j, 32);
    for (uint32_t i = 0; i < d; i++) store_host<F>(tau + (size_t)i * (F::N / 2), tr.random_challenge_as_field_element<F>());
}

// g(0), g(1), g(2), g(3) from the pass's sums at the nodes 0, 1, 2 and infinity: g(3) = 3 g(2) - 3 g(1) + g(0) + 6 s_inf
template <class F> void zerocheck_g4(const Fe<F> S[4], Fe<F> g[4]) {
    g[0] = S[0];
    g[1] = S[1];
    g[2] = S[2];
    const Fe<F> t = fe_add<F>(fe_sub<F>(S[2], S[1]), fe_dbl<F>(S[3]));   // g(2) - g(1) + 2 s_inf
    g[3] = fe_add<F>(fe_add<F>(fe_dbl<F>(t), t), S[0]);
}

// the cubic through (0, g[0]) .. (3, g[3]) at r
template <class F> Fe<F> zerocheck_cubic_at(const Fe<F> g[4], const Fe<F> &r) {
    const Fe<F> one = fe_one<F>(), r1 = fe_sub<F>(r, one), r2 = fe_sub<F>(r1, one), r3 = fe_sub<F>(r2, one);
    const Fe<F> inv2 = fe_inv<F>(fe_from_u64<F>(2)), inv6 = fe_inv<F>(fe_from_u64<F>(6));
    const Fe<F> l0 = fe_mul<F>(fe_mul<F>(r1, fe_mul<F>(r2, r3)), inv6), l1 = fe_mul<F>(fe_mul<F>(r, fe_mul<F>(r2, r3)), inv2);
    const Fe<F> l2 = fe_mul<F>(fe_mul<F>(r, fe_mul<F>(r1, r3)), inv2), l3 = fe_mul<F>(fe_mul<F>(r, fe_mul<F>(r1, r2)), inv6);
    return fe_add<F>(fe_sub<F>(fe_mul<F>(g[1], l1), fe_mul<F>(g[0], l0)), fe_sub<F>(fe_mul<F>(g[3], l3), fe_mul<F>(g[2], l2)));
}

// The verifier's steps 1, 2 and 4 on `tr` and its three checks: g_0(0) + g_0(1) = 0, g_l(0) + g_l(1) = g_{l-1}(r_{l-1}), and
// g_{d-1}(r_{d-1}) = eq(z, tau) (yA yB - yC).  round_polys: 4 d elements, ys: 3.  z (d elements) receives the point, z[d - 1 - l] = r_l;
// *good = every check held and every element read is reduced.  The transcript advances the same way whatever *good is.
template <class F> void zerocheck_replay(Transcript &tr, const uint8_t *roots96, uint32_t d, const uint64_t *round_polys, const uint64_t *ys, uint64_t *z, bool *good) {
    constexpr int W = F::N / 2;
    std::vector<uint64_t> tau((size_t)d * W);
    zerocheck_statement<F>(tr, roots96, d, tau.data());
    bool ok = true;
    Fe<F> cur = fe_zero<F>();
    for (uint32_t l = 0; l < d; l++) {
        Fe<F> g[4];
        for (int k = 0; k < 4; k++) {
            const uint64_t *src = round_polys + ((size_t)l * 4 + k) * W;
            ok = ok && is_reduced<F>(src);
            g[k] = load_host<F>(src);
            tr.append_be<F>(g[k]);
        }
        ok = ok && fe_eq<F>(fe_add<F>(g[0], g[1]), cur);
        const Fe<F> r = tr.random_challenge_as_field_element<F>();
        store_host<F>(z + (size_t)(d - 1 - l) * W, r);
        cur = zerocheck_cubic_at<F>(g, r);
    }
    const Fe<F> one = fe_one<F>();
    Fe<F> eq = one;
    for (uint32_t i = 0; i < d; i++) {
        const Fe<F> a = load_host<F>(z + (size_t)i * W), b = load_host<F>(tau.data() + (size_t)i * W);
        eq = fe_mul<F>(eq, fe_add<F>(fe_mul<F>(a, b), fe_mul<F>(fe_sub<F>(one, a), fe_sub<F>(one, b))));
    }
    for (int j = 0; j < 3; j++) ok = ok && is_reduced<F>(ys + (size_t)j * W);
    const Fe<F> gate = fe_sub<F>(fe_mul<F>(load_host<F>(ys), load_host<F>(ys + W)), load_host<F>(ys + 2 * W));
    *good = ok && fe_eq<F>(cur, fe_mul<F>(eq, gate));
}

}  // namespace host
}  // namespace zk
