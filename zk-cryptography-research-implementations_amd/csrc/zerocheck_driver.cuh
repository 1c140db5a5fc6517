// zerocheck_driver.cuh -- the driver that the six provers of the zerocheck family share (zkmle_zerocheck.hip, zkmle_wiring.hip, zkmle_plonk.hip,
// zkmle_lookup.hip, zkmle_plonk_lookup.hip, zkmle_plonk_lookup_columns.hip): the room for a pass's sums, the block the rounds fold in, the ONE
// round loop (prove_rounds) and the one-pass test hook (round_once), both over a protocol's `launch` and `message`; and what their C-ABI shells
// do alike: the hooks' table checks, the verifiers' statuses before the transcript is touched, the provers' end after the opening.  A protocol
// keeps its kernel launch, its statement and helper phase and its extern "C" functions.  Library-internal; included by .hip files only.
//
//   launch(fold, in, out0, ostride, q, r, l, partials, sums) -> status.  One pass over q pairs of the T tables in[0 .. T) (E last): its NS sums
//       to `sums` (device) and, when `fold`, table j folded at r to out0 + j ostride.  l is the round (0 in a hook).  Launches only.
//   message(S, g): the round message g[0 .. NODES) from the pass's sums S[0 .. NS), on the host.
#pragma once
#include <chrono>

#include "eq_table.cuh"
#include "fri_host.h"
#include "zerocheck_host.h"

namespace zk {
namespace host {

// room for the workgroups' partial sums and the `nsums` sums behind them
struct SumsBuf {
    DevBuf buf;
    void *sums = nullptr;
    int alloc(size_t esz, size_t nsums) {
        const size_t cap = (size_t)reduce_block_cap();
        ZK_TRY(buf.alloc((nsums * cap + nsums) * esz));
        sums = (char *)buf.p + nsums * cap * esz;
        return ZK_OK;
    }
};

// One block for a prover's rounds over T tables of n = 2^d elements of esz bytes: E_0 (n elements), then the two ping-pong halves: the T tables
// of an odd round (n / 2 entries each at round 1) and of an even one (n / 4 each at round 2); a round's tables never outgrow the half they first
// had.  At round 0 the tables are the caller's T - 1 opened ones and E_0.
template <int T> struct RoundBlock {
    DevBuf blk;
    const void *first[T];
    char *half[2];
    size_t n, esz;
    int alloc(const void *const *opened, unsigned d, size_t esz_) {
        n = (size_t)1 << d;
        esz = esz_;
        ZK_TRY(blk.alloc((n + T * (n / 2) + T * (n / 4) + 1) * esz));
        for (int j = 0; j < T; j++) first[j] = j < T - 1 ? opened[j] : blk.p;
        half[0] = (char *)blk.p + n * esz;
        half[1] = half[0] + T * (n / 2) * esz;
        return ZK_OK;
    }
    void *E0() const { return blk.p; }
    void *out0(unsigned l) const { return half[(l - 1) & 1]; }          // where round l's tables lie, l >= 1: table j at out0 + j ostride
    size_t ostride(unsigned l) const { return (n >> l) * esz; }
    void tables_at(unsigned l, const void **out) const {                // the T tables at round l: n >> l entries each
        for (int j = 0; j < T; j++) out[j] = l == 0 ? first[j] : (char *)out0(l) + (size_t)j * ostride(l);
    }
};

// E_0 from tau and the d rounds on `tr` over the T - 1 tables `opened` (device, 2^d elements each) and E: round_polys (NODES d elements),
// challenges (d) and z (d elements, z[d - 1 - l] = r_l: the point the opening is made at).  One host synchronisation per round: the sums down,
// the transcript's step on the host, r_l up as the next pass's argument.  ms_eq = from the caller's mark *from to E_0 built (the wiring kinds and
// the lookup: their last commitment's mark, the allocations inside the span) or, with from = NULL, from a mark of the driver's own after the
// allocations (the two zerochecks: E_0's construction alone); ms_rounds = the rounds.  The stream is idle on return.
template <class F, int T, int NS, int NODES, class Launch, class Message>
int prove_rounds(const void *const *opened, unsigned d, const uint64_t *tau, Transcript &tr, Launch &&launch, Message &&message, uint64_t *round_polys,
                 uint64_t *challenges, uint64_t *z, Events &ev, const size_t *from, float *ms_eq, float *ms_rounds) {
    constexpr size_t ESZ = sizeof(Fe<F>);
    constexpr int W = F::N / 2;
    RoundBlock<T> blk;
    SumsBuf sb;
    ZK_TRY(blk.alloc(opened, d, ESZ));
    ZK_TRY(sb.alloc(ESZ, NS));
    size_t e0, e1, e2;
    if (from) e0 = *from;
    else ZK_TRY(ev.mark(&e0));
    EqBuilder<F> eqb;
    ZK_TRY(eqb.build(tau, d, blk.E0()));
    ZK_TRY(ev.mark(&e1));
    Fe<F> r = fe_one<F>();
    for (unsigned l = 0; l < d; l++) {
        const void *in[T];
        blk.tables_at(l == 0 ? 0 : l - 1, in);
        ZK_TRY(launch(l != 0, in, l == 0 ? nullptr : blk.out0(l), l == 0 ? 0 : blk.ostride(l), blk.n >> (l + 1), r, l, sb.buf.p, sb.sums));
        Fe<F> S[NS], g[NODES];
        ZK_HIP(zk::memcpy_on_stream(S, sb.sums, NS * ESZ, hipMemcpyDeviceToHost));   // the round's synchronisation
        if (l == 0) eqb.release();
        message(S, g);
        for (int k = 0; k < NODES; k++) {
            store_host<F>(round_polys + ((size_t)l * NODES + k) * W, g[k]);
            tr.append_be<F>(g[k]);
        }
        r = tr.random_challenge_as_field_element<F>();
        store_host<F>(challenges + (size_t)l * W, r);
        store_host<F>(z + (size_t)(d - 1 - l) * W, r);
    }
    ZK_TRY(ev.mark(&e2));
    ZK_HIP(hipEventSynchronize(ev.ev[e2]));
    *ms_eq = ev.ms(e0, e1);
    *ms_rounds = ev.ms(e1, e2);
    return ZK_OK;
}

// The test hook of one pass over the T tables `in` (checked by the caller): gout (NODES elements) = its message; with r, outs[0 .. T) = new
// tables of half the length, folded at r.  The pass writes the folded T into one block; the caller's new tables are copies of its parts.
template <class F, int T, int NS, int NODES, class Launch, class Message>
int round_once(const zk_table *const *in, const uint64_t *r, zk_table **outs, uint64_t *gout, Launch &&launch, Message &&message) {
    constexpr size_t ESZ = sizeof(Fe<F>);
    const bool fold = r != nullptr;
    const size_t len = in[0]->len, q = fold ? len / 4 : len / 2, ostride = fold ? (len / 2) * ESZ : 0;
    SumsBuf sb;
    ZK_TRY(sb.alloc(ESZ, NS));
    zk_table *o[T] = {};
    const auto drop = [&] { for (zk_table *t : o) zk_table_free(t); };
    DevBuf folded;
    const void *ip[T];
    for (int j = 0; j < T; j++) ip[j] = in[j]->dptr;
    if (fold) {
        ZK_TRY(folded.alloc(T * ostride));
        for (int j = 0; j < T; j++) {
            const int rc = zk_table_alloc(in[0]->field, len / 2, &o[j]);
            if (rc != ZK_OK) { drop(); return rc; }
        }
    }
    Fe<F> S[NS], g[NODES];
    int rc = launch(fold, ip, folded.p, ostride, q, fold ? load_host<F>(r) : fe_one<F>(), 0u, sb.buf.p, sb.sums);
    for (int j = 0; fold && rc == ZK_OK && j < T; j++)
        if (hipMemcpyAsync(o[j]->dptr, (char *)folded.p + (size_t)j * ostride, ostride, hipMemcpyDeviceToDevice, cur_stream()) != hipSuccess) rc = ZK_E_HIP;
    if (rc == ZK_OK && zk::memcpy_on_stream(S, sb.sums, NS * ESZ, hipMemcpyDeviceToHost) != hipSuccess) rc = ZK_E_HIP;
    if (rc != ZK_OK) { drop(); return rc; }
    message(S, g);
    for (int k = 0; k < NODES; k++) store_host<F>(gout + (size_t)k * (F::N / 2), g[k]);
    for (int j = 0; fold && j < T; j++) outs[j] = o[j];
    return ZK_OK;
}

// what the hooks check alike: `count` tables, none NULL, one of the two scalar fields, one length, a power of two of at least `least`
inline int check_tables(const zk_table *const *tables, int count, size_t least) {
    if (!tables) return ZK_E_ARG;
    for (int j = 0; j < count; j++)
        if (!tables[j]) return ZK_E_ARG;
    const int field = tables[0]->field;
    if (field != ZK_FR381 && field != ZK_BN254_FR) return ZK_E_ARG;
    for (int j = 1; j < count; j++)
        if (tables[j]->field != field) return ZK_E_ARG;
    for (int j = 1; j < count; j++)
        if (tables[j]->len != tables[0]->len) return ZK_E_LEN_MISMATCH;
    if (!is_pow2(tables[0]->len)) return ZK_E_NOT_POW2;
    if (tables[0]->len < least) return ZK_E_ARG;
    return ZK_OK;
}

// Every status of a verifier before the transcript is touched, in the order the six keep: the grinding bound, the caller's pointers (have_all),
// the field's limbs, the opening's own statuses on an empty replay (`sizes`: the protocol's sizes call, and whatever bound it sets beside it),
// a zero coset, and ZK_E_RANGE for the field and its two-adicity.  The replay and the opening's verifier then run on a copy that becomes the
// caller's transcript only with ZK_OK.
template <class Sizes> int verify_check(int field, uint32_t d, uint32_t log_blowup, const uint64_t *coset, uint32_t grinding_bits, bool have_all, Sizes &&sizes) {
    if (grinding_bits > ZK_FRI_GRIND_MAX_BITS || !have_all || field_limbs64(field) < 0) return ZK_E_ARG;
    ZK_TRY(sizes());
    if (coset && is_zero_element(field, coset)) return ZK_E_ARG;
    if ((field != ZK_FR381 && field != ZK_BN254_FR) || d + log_blowup > two_adicity(field)) return ZK_E_RANGE;
    return ZK_OK;
}

// a prover's end: `opened` is the status of the opening it has just made at the rounds' point; st becomes the thread's last stats
template <class Stats> int prove_finish(int opened, std::chrono::steady_clock::time_point t0, Stats &st, Stats &last) {
    ZK_TRY(opened);
    zk_fri_ml_stats ml{};
    (void)zk_fri_ml_last_stats(&ml);
    st.ms_opening = ml.ms_total;
    st.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    last = st;
    return ZK_OK;
}

}  // namespace host
}  // namespace zk
