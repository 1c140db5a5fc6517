// zkmle_fri_ml.hip -- C ABI of the multilinear opening of a FRI commitment (fri_ml.cuh): one Lagrange-form fold, the opening (a sumcheck
// of sum_x T[x] eq(x, z) interleaved with the folds of the codeword, on the same challenges), its host verifier, and the basic sumcheck
// that ends in such an opening; and the opening at several points with one proof (a sumcheck against the gamma-combination of the points'
// eq tables: "FRI commitment opened at several points").  Extension: the reference leaves `fri/` empty; the protocol is defined in
// include/zkmle.h "FRI commitment opened as a multilinear polynomial".
#include <string.h>

#include <chrono>
#include <vector>

#include "eq_table.cuh"
#include "fri_host.h"
#include "fri_ml.cuh"

using namespace zk;
using namespace zk::host;

namespace {

thread_local zk_fri_ml_stats g_ml_stats{};

// eq1(a, b) = a b + (1 - a)(1 - b)
template <class F> Fe<F> eq1(const Fe<F> &a, const Fe<F> &b) {
    const Fe<F> one = fe_one<F>();
    return fe_add<F>(fe_mul<F>(a, b), fe_mul<F>(fe_sub<F>(one, a), fe_sub<F>(one, b)));
}

// out[k], k < len / 2, from in[0 .. len): gamma = r / (2 c_l), `shift` = the layer's number, c = c_l (null: 1)
template <class F> int launch_fold(const void *in, void *out, size_t len, unsigned shift, const FoldTables<F> &tb, const Fe<F> &gamma, const Fe<F> *c) {
    const FriUni g = fri_uni<F>(gamma);
    const size_t half = len / 2;
    const unsigned blocks = (unsigned)((half + kFriBlock - 1) / kFriBlock);
    if (c) fri_ml_fold_kernel<F, true><<<blocks, kFriBlock, 0, cur_stream()>>>(in, out, half, tb.lo, tb.hi, shift, FriMlShift<F, true>{*c}, g);
    else fri_ml_fold_kernel<F, false><<<blocks, kFriBlock, 0, cur_stream()>>>(in, out, half, tb.lo, tb.hi, shift, FriMlShift<F, false>{}, g);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class F> int fold_once(const zk_table *cw, const uint64_t *r, const uint64_t *coset, zk_table **out) {
    FoldTables<F> tb;
    ZK_TRY(tb.build(ilog2(cw->len)));
    Fe<F> den = fe_from_u64<F>(2), c = fe_one<F>();
    if (coset) { c = load_host<F>(coset); den = fe_mul<F>(den, c); }
    zk_table *o = nullptr;
    ZK_TRY(zk_table_alloc(cw->field, cw->len / 2, &o));
    const int rc = launch_fold<F>(cw->dptr, o->dptr, cw->len, 0, tb, fe_mul<F>(load_host<F>(r), fe_inv<F>(den)), coset ? &c : nullptr);
    if (rc != ZK_OK) { zk_table_free(o); return rc; }
    *out = o;
    return ZK_OK;
}

// out[k], k < len / 4, from in[0 .. len): two folds in one pass.  g0 = r0 / (2 c_l), g1 = r1 / (2 c_l^2), `shift` = the layer's number, c = c_l (null: 1)
template <class F> int launch_fold4(const void *in, void *out, size_t len, unsigned shift, const FoldTables<F> &tb, const Fe<F> &g0, const Fe<F> &g1, const Fe<F> *c) {
    const FriUni g = fri_uni<F>(g0);
    const size_t quarter = len / 4;
    const unsigned blocks = (unsigned)((quarter + kFriBlock - 1) / kFriBlock);
    if (c) fri_ml_fold4_kernel<F, true><<<blocks, kFriBlock, 0, cur_stream()>>>(in, out, quarter, tb.lo, tb.hi, shift, FriMlShift2<F, true>{*c, fe_sqr<F>(*c)}, g1, g);
    else fri_ml_fold4_kernel<F, false><<<blocks, kFriBlock, 0, cur_stream()>>>(in, out, quarter, tb.lo, tb.hi, shift, FriMlShift2<F, false>{}, g1, g);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class F> int fold4_once(const zk_table *cw, const uint64_t *r0, const uint64_t *r1, const uint64_t *coset, zk_table **out) {
    FoldTables<F> tb;
    ZK_TRY(tb.build(ilog2(cw->len)));
    const Fe<F> two = fe_from_u64<F>(2), c = coset ? load_host<F>(coset) : fe_one<F>();
    const Fe<F> g0 = fe_mul<F>(load_host<F>(r0), fe_inv<F>(fe_mul<F>(two, c))), g1 = fe_mul<F>(load_host<F>(r1), fe_inv<F>(fe_mul<F>(two, fe_sqr<F>(c))));
    zk_table *o = nullptr;
    ZK_TRY(zk_table_alloc(cw->field, cw->len / 4, &o));
    const int rc = launch_fold4<F>(cw->dptr, o->dptr, cw->len, 0, tb, g0, g1, coset ? &c : nullptr);
    if (rc != ZK_OK) { zk_table_free(o); return rc; }
    *out = o;
    return ZK_OK;
}

// out[i], i < len / sides, from the k codewords of `len` entries each: the fold (g1 null) or fold4 of sum_j coef_j f_j at layer 0, one pass.
// coef: k stored-form elements.  g0 = r0 / (2 c), g1 = r1 / (2 c^2), c = the coset's shift (null: 1)
// `Args`: FriMlBatchArgs<F> with fri_ml_fold_batch_kernel, or the 32-slot block with fri_ml_fold_batch_wide_kernel
template <class F, class Args, bool WIDE> int launch_fold_batch_as(const void *const *cws, unsigned k, const Fe<F> *coef, void *out, size_t len, const FoldTables<F> &tb,
                                                                  const Fe<F> &g0, const Fe<F> *g1, const Fe<F> *c) {
    Args a{};
    for (unsigned j = 0; j < k; j++) {
        a.t[j] = cws[j];
        a.c[j] = lincomb_coeff<F>(coef[j]);
    }
    a.k = (int)k;
    const size_t part = g1 ? len / 4 : len / 2, want = (part + kFriBlock - 1) / kFriBlock;
    const unsigned blocks = (unsigned)(want < (size_t)kFriMlBatchBlocks ? want : (size_t)kFriMlBatchBlocks);
    const Fe<F> gg1 = g1 ? *g1 : fe_one<F>();
    if constexpr (WIDE) {
        constexpr int CAP = kFriMlWideMax;
        if (c) {
            const FriMlShift2<F, true> sh{*c, fe_sqr<F>(*c)};
            if (g1) fri_ml_fold_batch_wide_kernel<F, CAP, 4, true><<<blocks, kFriBlock, 0, cur_stream()>>>(a, out, part, tb.lo, tb.hi, sh, g0, gg1);
            else fri_ml_fold_batch_wide_kernel<F, CAP, 2, true><<<blocks, kFriBlock, 0, cur_stream()>>>(a, out, part, tb.lo, tb.hi, sh, g0, gg1);
        } else {
            if (g1) fri_ml_fold_batch_wide_kernel<F, CAP, 4, false><<<blocks, kFriBlock, 0, cur_stream()>>>(a, out, part, tb.lo, tb.hi, FriMlShift2<F, false>{}, g0, gg1);
            else fri_ml_fold_batch_wide_kernel<F, CAP, 2, false><<<blocks, kFriBlock, 0, cur_stream()>>>(a, out, part, tb.lo, tb.hi, FriMlShift2<F, false>{}, g0, gg1);
        }
    } else {
        if (c) {
            const FriMlShift2<F, true> sh{*c, fe_sqr<F>(*c)};
            if (g1) fri_ml_fold_batch_kernel<F, 4, true><<<blocks, kFriBlock, 0, cur_stream()>>>(a, out, part, tb.lo, tb.hi, sh, g0, gg1);
            else fri_ml_fold_batch_kernel<F, 2, true><<<blocks, kFriBlock, 0, cur_stream()>>>(a, out, part, tb.lo, tb.hi, sh, g0, gg1);
        } else {
            if (g1) fri_ml_fold_batch_kernel<F, 4, false><<<blocks, kFriBlock, 0, cur_stream()>>>(a, out, part, tb.lo, tb.hi, FriMlShift2<F, false>{}, g0, gg1);
            else fri_ml_fold_batch_kernel<F, 2, false><<<blocks, kFriBlock, 0, cur_stream()>>>(a, out, part, tb.lo, tb.hi, FriMlShift2<F, false>{}, g0, gg1);
        }
    }
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}
// k <= kFriMlBatchMax: the 16-slot block and its kernel, whichever entry point asks; above (the wide entry points only, k <= kFriMlWideMax): the 32-slot one
template <class F> int launch_fold_batch(const void *const *cws, unsigned k, const Fe<F> *coef, void *out, size_t len, const FoldTables<F> &tb, const Fe<F> &g0,
                                         const Fe<F> *g1, const Fe<F> *c) {
    if (k > (unsigned)kFriMlWideMax) return ZK_E_ARG;
    if (k > (unsigned)kFriMlBatchMax) return launch_fold_batch_as<F, FriMlBatchArgsCap<F, kFriMlWideMax>, true>(cws, k, coef, out, len, tb, g0, g1, c);
    return launch_fold_batch_as<F, FriMlBatchArgs<F>, false>(cws, k, coef, out, len, tb, g0, g1, c);
}

template <class F> int fold_batch_once(const zk_table *const *cws, unsigned k, const uint64_t *coeffs, const uint64_t *r0, const uint64_t *r1, const uint64_t *coset,
                                       zk_table **out) {
    constexpr int W = F::N / 2;
    const size_t len = cws[0]->len;
    FoldTables<F> tb;
    ZK_TRY(tb.build(ilog2(len)));
    const Fe<F> two = fe_from_u64<F>(2), c = coset ? load_host<F>(coset) : fe_one<F>();
    const Fe<F> g0 = fe_mul<F>(load_host<F>(r0), fe_inv<F>(fe_mul<F>(two, c)));
    Fe<F> g1 = fe_one<F>();
    if (r1) g1 = fe_mul<F>(load_host<F>(r1), fe_inv<F>(fe_mul<F>(two, fe_sqr<F>(c))));
    const void *ptrs[kFriMlWideMax];
    Fe<F> coef[kFriMlWideMax];
    for (unsigned j = 0; j < k; j++) {
        ptrs[j] = cws[j]->dptr;
        coef[j] = load_host<F>(coeffs + (size_t)j * W);
    }
    zk_table *o = nullptr;
    ZK_TRY(zk_table_alloc(cws[0]->field, r1 ? len / 4 : len / 2, &o));
    const int rc = launch_fold_batch<F>(ptrs, k, coef, o->dptr, len, tb, g0, r1 ? &g1 : nullptr, coset ? &c : nullptr);
    if (rc != ZK_OK) { zk_table_free(o); return rc; }
    *out = o;
    return ZK_OK;
}

// ---- the passes ----------------------------------------------------------------------------------------------------------------
// sums (device, 2 elements) = S_0, S_1 of the pass; FOLD: see fri_ml_round_kernel.  Launches only.
template <class F> int launch_round(bool fold, const void *tin, const void *ein, void *tout, void *eout, size_t q, const Fe<F> &r, void *partials, void *sums) {
    const int grid = reduce_grid_for(q);
    if (fold) fri_ml_round_kernel<F, true><<<grid, kBlock, 0, cur_stream()>>>(tin, ein, tout, eout, q, r, partials);
    else fri_ml_round_kernel<F, false><<<grid, kBlock, 0, cur_stream()>>>(tin, ein, tout, eout, q, r, partials);
    ZK_HIP(hipGetLastError());
    finish_sums_kernel<F><<<1, kBlock, 0, cur_stream()>>>(partials, (size_t)grid, 2, sums);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

// sums (device, 3 elements) = the pass's sums at the nodes 0, 1, infinity (fri_ml_round_w_kernel).  Launches only.
template <class F> int launch_round_w(bool fold, const void *tin, const void *win, void *tout, void *wout, size_t q, const Fe<F> &r, void *partials, void *sums) {
    const int grid = reduce_grid_for(q);
    if (fold) fri_ml_round_w_kernel<F, true><<<grid, kBlock, 0, cur_stream()>>>(tin, win, tout, wout, q, r, partials);
    else fri_ml_round_w_kernel<F, false><<<grid, kBlock, 0, cur_stream()>>>(tin, win, tout, wout, q, r, partials);
    ZK_HIP(hipGetLastError());
    finish_sums_kernel<F><<<1, kBlock, 0, cur_stream()>>>(partials, (size_t)grid, 3, sums);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}
// g(0), g(1), g(2) from the sums at 0, 1, infinity: g(2) = 2 g(1) - g(0) + 2 g(inf)
template <class F> void nodes_to_g3(const Fe<F> S[3], Fe<F> g[3]) {
    g[0] = S[0];
    g[1] = S[1];
    const Fe<F> t = fe_add<F>(S[1], S[2]);
    g[2] = fe_sub<F>(fe_add<F>(t, t), S[0]);
}

template <class F> int round_once(const zk_table *T, const zk_table *Wt, const uint64_t *r, zk_table **T_out, zk_table **W_out, uint64_t *g3) {
    constexpr size_t ESZ = sizeof(Fe<F>);
    constexpr int W = F::N / 2;
    const bool fold = r != nullptr;
    const size_t q = fold ? T->len / 4 : T->len / 2;
    DevBuf scr;
    const size_t cap = (size_t)reduce_block_cap();
    ZK_TRY(scr.alloc((3 * cap + 3) * ESZ));
    void *sums = (char *)scr.p + 3 * cap * ESZ;
    zk_table *to = nullptr, *wo = nullptr;
    if (fold) {
        ZK_TRY(zk_table_alloc(T->field, T->len / 2, &to));
        const int rc = zk_table_alloc(T->field, T->len / 2, &wo);
        if (rc != ZK_OK) { zk_table_free(to); return rc; }
    }
    Fe<F> S[3], g[3];
    int rc = launch_round_w<F>(fold, T->dptr, Wt->dptr, fold ? to->dptr : nullptr, fold ? wo->dptr : nullptr, q, fold ? load_host<F>(r) : fe_one<F>(), scr.p, sums);
    if (rc == ZK_OK && zk::memcpy_on_stream(S, sums, 3 * ESZ, hipMemcpyDeviceToHost) != hipSuccess) rc = ZK_E_HIP;
    if (rc != ZK_OK) { zk_table_free(to); zk_table_free(wo); return rc; }
    nodes_to_g3<F>(S, g);
    for (int k = 0; k < 3; k++) store_host<F>(g3 + (size_t)k * W, g[k]);
    if (fold) { *T_out = to; *W_out = wo; }
    return ZK_OK;
}

// ---- the prover ----------------------------------------------------------------------------------------------------------------
struct OpenOut {
    uint64_t *round_polys;
    uint8_t *roots;
    uint64_t *final_table, *challenges, *query_indices, *query_values;
    uint8_t *query_paths;
};
// what a form's passes work on: the commitment's table T_0, the form's weight tables, the workgroups' partial sums and the pass's sums
struct PassMem {
    const void *T0;
    char *weights;
    void *partials, *sums;
};

// The three forms of the opening.  The driver (open_with) owns everything they share; a form supplies what defines its protocol:
//   kSums                      the sums a pass leaves
//   weight_room / weight_off   the elements its weight tables take for a table of n entries, and where round l's table starts
//   absorb                     what enters the transcript between root_0 and round 0
//   start                      the rest of what precedes round 0, and round 0's pass (launched, not waited for); release() follows the wait
//   pass                       a round's launches
//   round_poly                 g_l(0), g_l(1), g_l(2) from the last pass's sums S
//   bind                       the challenge's effect on the form's own state
//   kBatch                     ManyTables only, which then also supplies: statement (the tag and the k roots in place of the arity line and
//                              the single root), ntables, fold0 (the first step's fold, of the k codewords) and layer0 (where a query's
//                              step-0 answers come from)

// one point z: an eq table of (z_0 .. z_{d-2}) with the last variable summed out, S_0 and S_1, and g_l formed here from A_l, eq1 and the sums
template <class F> struct OnePoint {
    static constexpr int W = F::N / 2;
    static constexpr unsigned kSums = 2;
    static constexpr bool kBatch = false;
    const uint64_t *z;
    uint64_t *y_out;
    unsigned d;
    Fe<F> A = fe_one<F>();                                    // A_l
    EqBuilder<F> eqb;

    size_t weight_room(size_t n) const { return n; }          // E_0 .. E_{R-1}
    size_t weight_off(size_t n, unsigned l) const { return n - (n >> l); }   // E_l: n >> (l + 1) entries
    void absorb(Transcript &tr) const {
        for (unsigned i = 0; i < d; i++) tr.append_be<F>(load_host<F>(z + (size_t)i * W));
    }
    // E_0 = the eq table of (z_0 .. z_{d-2}); the pass reads the commitment's own coefficient table and writes nothing
    int start(const zk_fri_commitment *, Transcript &, const PassMem &m) {
        ZK_TRY(eqb.build(z, d - 1, m.weights));
        return pass(false, m.T0, m.weights, nullptr, nullptr, ((size_t)1 << d) / 2, fe_one<F>(), m.partials, m.sums);
    }
    void release() { eqb.release(); }
    static int pass(bool fold, const void *tin, const void *win, void *tout, void *wout, size_t q, const Fe<F> &r, void *partials, void *sums) {
        return launch_round<F>(fold, tin, win, tout, wout, q, r, partials, sums);
    }
    // g_l(X) = A_l eq1(X, z_v) (S_0 + X (S_1 - S_0)) at 0, 1, 2: eq1(0, z) = 1 - z, eq1(1, z) = z, eq1(2, z) = 3 z - 1
    void round_poly(unsigned l, const Fe<F> *S, Transcript &tr, Fe<F> g[3]) const {
        const Fe<F> one = fe_one<F>(), two = fe_from_u64<F>(2), three = fe_from_u64<F>(3), zv = load_host<F>(z + (size_t)(d - 1 - l) * W);
        g[0] = fe_mul<F>(A, fe_mul<F>(fe_sub<F>(one, zv), S[0]));
        g[1] = fe_mul<F>(A, fe_mul<F>(zv, S[1]));
        g[2] = fe_mul<F>(A, fe_mul<F>(fe_sub<F>(fe_mul<F>(three, zv), one), fe_sub<F>(fe_mul<F>(two, S[1]), S[0])));
        if (l == 0) {                                        // y = g_0(0) + g_0(1): the claim comes out of round 0's pass
            const Fe<F> y = fe_add<F>(g[0], g[1]);
            store_host<F>(y_out, y);
            tr.append_be<F>(y);
        }
    }
    void bind(unsigned l, const Fe<F> &r) { A = fe_mul<F>(A, eq1<F>(r, load_host<F>(z + (size_t)(d - 1 - l) * W))); }
};

// P points: a weight table W_0 = sum_p gamma^p eq(., z^p) of n entries folded beside T, the sums at the nodes 0, 1, infinity
template <class F> struct ManyPoints {
    static constexpr int W = F::N / 2;
    static constexpr unsigned kSums = 3;
    static constexpr bool kBatch = false;
    const uint64_t *pts;
    uint32_t P;
    uint64_t *ys_out, *gamma_out;
    unsigned d;
    std::vector<EqBuilder<F>> eqb;

    size_t weight_room(size_t n) const { return 2 * n + (P > 1 ? (size_t)P * n : 0); }   // W_0 .. W_{R-1}, then the P eq tables W_0 is combined from
    size_t weight_off(size_t n, unsigned l) const { return 2 * n - ((2 * n) >> l); }      // W_l: n >> l entries
    void absorb(Transcript &tr) const {
        uint8_t pbe[4];
        put_be32(pbe, P);
        tr.append(pbe, 4);
        for (size_t i = 0; i < (size_t)P * d; i++) tr.append_be<F>(load_host<F>(pts + i * W));
    }
    int start(const zk_fri_commitment *cm, Transcript &tr, const PassMem &m) {
        const size_t n = (size_t)1 << d;
        // y_p = zk_mle_evaluate(T, z^p), a pass each; they are absorbed before gamma exists
        for (unsigned p = 0; p < P; p++) {
            ZK_TRY(zk_mle_evaluate(cm->coeffs, pts + (size_t)p * d * W, d, ys_out + (size_t)p * W));
            tr.append_be<F>(load_host<F>(ys_out + (size_t)p * W));
        }
        const Fe<F> gamma = tr.random_challenge_as_field_element<F>();
        if (gamma_out) store_host<F>(gamma_out, gamma);
        ZK_TRY(weights(gamma, m));
        // round 0's pass reads the commitment's own coefficient table and W_0 and writes neither
        return pass(false, m.T0, m.weights, nullptr, nullptr, n / 2, fe_one<F>(), m.partials, m.sums);
    }
    // W_0 = sum_p gamma^p eq(., z^p) into m.weights: one point's table is built in place, several are combined in one pass
    int weights(const Fe<F> &gamma, const PassMem &m) {
        constexpr size_t ESZ = sizeof(Fe<F>);
        const size_t n = (size_t)1 << d;
        eqb.resize(P);
        if (P == 1) {
            ZK_TRY(eqb[0].build(pts, d, m.weights));
        } else {
            const void *tabs[8];
            uint64_t coef[8 * W];
            Fe<F> gp = fe_one<F>();
            for (unsigned p = 0; p < P; p++) {
                tabs[p] = m.weights + (2 * n + (size_t)p * n) * ESZ;
                ZK_TRY(eqb[p].build(pts + (size_t)p * d * W, d, (void *)tabs[p]));
                store_host<F>(coef + (size_t)p * W, gp);
                gp = fe_mul<F>(gp, gamma);
            }
            ZK_HIP((lincomb_launch<F, false>(tabs, P, coef, m.weights, n, fe_zero<F>(), fe_zero<F>(), nullptr, cur_stream())));
        }
        return ZK_OK;
    }
    void release() { for (auto &e : eqb) e.release(); }
    static int pass(bool fold, const void *tin, const void *win, void *tout, void *wout, size_t q, const Fe<F> &r, void *partials, void *sums) {
        return launch_round_w<F>(fold, tin, win, tout, wout, q, r, partials, sums);
    }
    void round_poly(unsigned, const Fe<F> *S, Transcript &, Fe<F> g[3]) const { nodes_to_g3<F>(S, g); }
    void bind(unsigned, const Fe<F> &) {}
};

// a caller's weight table W_0 of n entries ("FRI commitment opened against a weight table"): ManyPoints without points.  Nothing of the table
// enters the transcript; the claim c = g_0(0) + g_0(1) comes out of round 0's pass and is appended before g_0, as OnePoint's y is
template <class F> struct Weighted {
    static constexpr int W = F::N / 2;
    static constexpr unsigned kSums = 3;
    static constexpr bool kBatch = false;
    const void *w0;                                          // device, n elements; not modified
    uint64_t *c_out;
    unsigned d;

    size_t weight_room(size_t n) const { return 2 * n; }     // W_0 .. W_{R-1}
    size_t weight_off(size_t n, unsigned l) const { return 2 * n - ((2 * n) >> l); }
    void absorb(Transcript &tr) const { tr.append((const uint8_t *)"WGHT", 4); }
    // W_0 = the caller's table, copied into the weights' room (the later rounds fold it there); round 0's pass writes nothing
    int start(const zk_fri_commitment *, Transcript &, const PassMem &m) {
        const size_t n = (size_t)1 << d;
        ZK_HIP(hipMemcpyAsync(m.weights, w0, n * sizeof(Fe<F>), hipMemcpyDeviceToDevice, cur_stream()));
        return pass(false, m.T0, m.weights, nullptr, nullptr, n / 2, fe_one<F>(), m.partials, m.sums);
    }
    void release() {}
    static int pass(bool fold, const void *tin, const void *win, void *tout, void *wout, size_t q, const Fe<F> &r, void *partials, void *sums) {
        return launch_round_w<F>(fold, tin, win, tout, wout, q, r, partials, sums);
    }
    void round_poly(unsigned l, const Fe<F> *S, Transcript &tr, Fe<F> g[3]) const {
        nodes_to_g3<F>(S, g);
        if (l == 0) {
            const Fe<F> c = fe_add<F>(g[0], g[1]);
            store_host<F>(c_out, c);
            tr.append_be<F>(c);
        }
    }
    void bind(unsigned, const Fe<F> &) {}
};

// k commitments at the same P points ("FRI commitments opened together"): ManyPoints on T = sum_j alpha^j T_j, alpha = gamma^P.  T_0 is
// written into n further elements behind the weights (round 1 reads it anyway); f_0 = sum_j alpha^j f_j is never stored: the first step's
// fold forms it in registers (fri_ml_fold_batch_kernel), and a query's step-0 answers come from the k commitments' own codewords and trees.
template <class F> struct ManyTables : ManyPoints<F> {
    using Base = ManyPoints<F>;
    static constexpr int W = F::N / 2;
    static constexpr bool kBatch = true;
    // the k tables and their codewords; the m trees they sit under and their roots: m = k, one each, for k commitments; for m COLUMN
    // commitments ("Column commitments opened together") the k columns of all of them in order, and `widths` (else null) = the m widths
    const zk_table *tabs[kFriMlWideMax];
    const void *cws[kFriMlWideMax];
    const uint64_t *trees[kFriMlWideMax];
    const uint8_t *own_roots[kFriMlWideMax];
    uint32_t k, m;
    const uint32_t *widths = nullptr;
    Fe<F> coef[kFriMlWideMax];                               // alpha^j
    void *table0 = nullptr;                                  // T_0's n elements of the pool block: the driver sets it before start

    ManyTables(const zk_fri_commitment *const *cms_, uint32_t k_, const uint64_t *pts_, uint32_t P_, uint64_t *ys, uint64_t *gamma, unsigned d_)
        : Base{pts_, P_, ys, gamma, d_, {}}, k(k_), m(k_) {
        for (uint32_t j = 0; j < k; j++) {
            tabs[j] = cms_[j]->coeffs;
            cws[j] = cms_[j]->codeword->dptr;
            trees[j] = cms_[j]->levels;
            own_roots[j] = cms_[j]->root;
        }
    }
    // widths_: m words that outlive the form
    ManyTables(const zk_fri_columns *const *cols, uint32_t m_, const uint32_t *widths_, const uint64_t *pts_, uint32_t P_, uint64_t *ys, uint64_t *gamma, unsigned d_)
        : Base{pts_, P_, ys, gamma, d_, {}}, k(0), m(m_), widths(widths_) {
        for (uint32_t i = 0; i < m; i++) {
            trees[i] = cols[i]->levels;
            own_roots[i] = cols[i]->root;
            for (uint32_t c = 0; c < cols[i]->k; c++, k++) {
                tabs[k] = cols[i]->coeffs[c];
                cws[k] = cols[i]->codeword[c]->dptr;
            }
        }
    }
    unsigned ntables() const { return k; }
    unsigned nroots() const { return m; }
    size_t weight_room(size_t n) const { return Base::weight_room(n) + n; }   // the base's, then T_0
    size_t table0_off(size_t n) const { return Base::weight_room(n); }        // in elements from the weights
    // "BTCH", a, the grouped flag, k -- columns: "COLS", a, m, the m widths -- then the m roots, which are also the proof's first m
    void statement(Transcript &tr, unsigned la, bool grouped, uint8_t *roots) const {
        uint8_t tag[12 + 4 * kFriMlWideMax] = {'B', 'T', 'C', 'H'};
        size_t len = 16;
        put_be32(tag + 4, la);
        if (widths) {
            memcpy(tag, "COLS", 4);
            put_be32(tag + 8, m);
            for (uint32_t i = 0; i < m; i++) put_be32(tag + 12 + 4 * i, widths[i]);
            len = 12 + 4 * (size_t)m;
        } else {
            put_be32(tag + 8, grouped ? 1 : 0);
            put_be32(tag + 12, k);
        }
        tr.append(tag, len);
        for (uint32_t j = 0; j < m; j++) {
            memcpy(roots + 32 * (size_t)j, own_roots[j], 32);
            tr.append(own_roots[j], 32);
        }
    }
    // y_{j,p} table-major, a pass each; gamma; W_0; T_0 = sum_j alpha^j T_j in one pass; round 0's pass on T_0 and W_0
    int start(const zk_fri_commitment *, Transcript &tr, const PassMem &mem) {
        const unsigned P = this->P, d = this->d;
        const size_t n = (size_t)1 << d;
        for (uint32_t j = 0; j < k; j++) {
            for (unsigned p = 0; p < P; p++) {
                uint64_t *y = this->ys_out + ((size_t)j * P + p) * W;
                ZK_TRY(zk_mle_evaluate(tabs[j], this->pts + (size_t)p * d * W, d, y));
                tr.append_be<F>(load_host<F>(y));
            }
        }
        const Fe<F> gamma = tr.random_challenge_as_field_element<F>();
        if (this->gamma_out) store_host<F>(this->gamma_out, gamma);
        Fe<F> alpha = fe_one<F>();
        for (unsigned p = 0; p < P; p++) alpha = fe_mul<F>(alpha, gamma);
        const void *src[kFriMlWideMax];
        uint64_t cw[kFriMlWideMax * W];
        Fe<F> aj = fe_one<F>();
        for (uint32_t j = 0; j < k; j++) {
            coef[j] = aj;
            store_host<F>(cw + (size_t)j * W, aj);
            src[j] = tabs[j]->dptr;
            aj = fe_mul<F>(aj, alpha);
        }
        ZK_TRY(this->weights(gamma, mem));
        ZK_HIP((lincomb_launch<F, false>(src, k, cw, table0, n, fe_zero<F>(), fe_zero<F>(), nullptr, cur_stream())));
        return Base::pass(false, mem.T0, mem.weights, nullptr, nullptr, n / 2, fe_one<F>(), mem.partials, mem.sums);
    }
    // layer 0 -> the layer of step 1: out gets len / 2 entries (g1 null) or len / 4
    int fold0(void *out, size_t len, const FoldTables<F> &tb, const Fe<F> &g0, const Fe<F> *g1, const Fe<F> *shift) const {
        return launch_fold_batch<F>(cws, k, coef, out, len, tb, g0, g1, shift);
    }
};

// The queries of an opening of k tables under m trees (k commitments: m = k, a tree each; column commitments: the k columns of m trees, whose
// leaves hold every column of theirs, so step 0 has k tables' values and m paths).  Step 0 has no table and no tree of its own: its answers are the k commitments', gathered by
// the existing kernels once per commitment over a one-step view of the schedule, and once more over the steps from 1 up; every launch
// writes its own part of one device block and the host lays a query's answer out as the protocol orders it (j-major for step 0, then the
// later steps).  The alternative, a table of layer-0 sources inside FriLayers, would add 32 pointers to the argument block of both kernels
// and a branch to every lane of the single-table provers for the sake of k - 1 small launches here.
template <class F> int answer_queries_batch(Transcript &tr, const void *const *cws, unsigned k, const uint64_t *const *trees, unsigned m, const FriLayers &fl, const FriSchedule &sc, uint32_t Q,
                                            uint64_t *indices_out, uint64_t *values, uint8_t *paths, Events &ev, float *ms, uint32_t grind_bits = 0,
                                            uint64_t *nonce_out = nullptr) {
    constexpr size_t ESZ = sizeof(Fe<F>);
    std::vector<uint64_t> idx;
    ZK_TRY(draw_indices(tr, sc, Q, idx, grind_bits, nonce_out));
    if (indices_out) memcpy(indices_out, idx.data(), Q * 8);
    // the two views: step 0 alone (its table and tree set per commitment), and the steps from 1 up with their offsets counted from step 1
    const size_t v0 = sc.nsteps > 1 ? sc.step[1].val_off : sc.nvalues, d0 = sc.nsteps > 1 ? sc.step[1].path_off : sc.ndigests;
    const size_t v1 = sc.nvalues - v0, d1 = sc.ndigests - d0;
    FriLayers first = sc.layers(0, 1), rest{};
    if (sc.nsteps > 1) rest = sc.layers(1);
    for (unsigned s = 1; s < sc.nsteps; s++) {
        rest.table[s - 1] = fl.table[s];
        rest.tree[s - 1] = fl.tree[s];
    }
    const size_t nval = (size_t)Q * (k * v0 + v1), ndig = (size_t)Q * (m * d0 + d1);
    DevBuf didx, dval, dpath;
    ZK_TRY(didx.alloc(Q * 8));
    ZK_TRY(dval.alloc(nval * ESZ));
    ZK_TRY(dpath.alloc(ndig * 32));
    std::vector<uint64_t> hval(nval * (ESZ / 8));
    std::vector<uint8_t> hpath(ndig * 32);
    size_t q0, q1;
    ZK_TRY(ev.mark(&q0));
    ZK_HIP(hipMemcpyAsync(didx.p, idx.data(), Q * 8, hipMemcpyHostToDevice, cur_stream()));
    // nv or nd = 0: that kernel is not launched
    const auto gather = [&](const FriLayers &view, size_t nv, size_t nd, size_t voff, size_t doff) -> int {
        if (nv) fri_query_values_kernel<F><<<(unsigned)((nv + kFriBlock - 1) / kFriBlock), kFriBlock, 0, cur_stream()>>>(view, (const uint64_t *)didx.p, Q, (char *)dval.p + voff * ESZ);
        ZK_HIP(hipGetLastError());
        if (nd) fri_query_paths_kernel<<<(unsigned)((nd + kFriBlock - 1) / kFriBlock), kFriBlock, 0, cur_stream()>>>(view, (const uint64_t *)didx.p, Q, (uint64_t *)((char *)dpath.p + doff * 32));
        ZK_HIP(hipGetLastError());
        return ZK_OK;
    };
    // the downloads land in this function's own buffers: whatever fails below, the stream is drained before they go
    const auto run = [&]() -> int {
        for (unsigned j = 0; j < k; j++) {                    // m <= k: table j's values, and tree j's paths while there is one
            first.table[0] = cws[j];
            first.tree[0] = trees[j < m ? j : 0];
            ZK_TRY(gather(first, (size_t)Q * v0, j < m ? (size_t)Q * d0 : 0, (size_t)j * Q * v0, (size_t)j * Q * d0));
        }
        if (sc.nsteps > 1) ZK_TRY(gather(rest, (size_t)Q * v1, (size_t)Q * d1, (size_t)k * Q * v0, (size_t)m * Q * d0));
        ZK_HIP(hipMemcpyAsync(hval.data(), dval.p, nval * ESZ, hipMemcpyDeviceToHost, cur_stream()));
        ZK_HIP(zk::memcpy_on_stream(hpath.data(), dpath.p, ndig * 32, hipMemcpyDeviceToHost));
        ZK_TRY(ev.mark(&q1));
        ZK_HIP(hipEventSynchronize(ev.ev[q1]));
        return ZK_OK;
    };
    const int rc = run();
    if (rc != ZK_OK) {
        (void)hipStreamSynchronize(cur_stream());
        return rc;
    }
    if (ms) *ms = ev.ms(q0, q1);
    const size_t pv = k * v0 + v1, pd = m * d0 + d1;          // of one query's answer
    for (size_t q = 0; q < Q; q++) {
        for (unsigned j = 0; j < k; j++) memcpy((char *)values + (q * pv + j * v0) * ESZ, (const char *)hval.data() + ((size_t)j * Q + q) * v0 * ESZ, v0 * ESZ);
        for (unsigned j = 0; j < m; j++) memcpy(paths + (q * pd + j * d0) * 32, hpath.data() + ((size_t)j * Q + q) * d0 * 32, d0 * 32);
        memcpy((char *)values + (q * pv + k * v0) * ESZ, (const char *)hval.data() + ((size_t)k * Q * v0 + q * v1) * ESZ, v1 * ESZ);
        memcpy(paths + (q * pd + m * d0) * 32, hpath.data() + ((size_t)m * Q * d0 + q * d1) * 32, d1 * 32);
    }
    return ZK_OK;
}

// The opening: the sumcheck's rounds interleaved with the folds of the codeword, on the same challenges.  la = log_arity.  1: every layer
// f_1 .. f_{R-1} is committed.  2 (R >= 2): the even ones are; after r_l with l even only round l + 1's pass runs, after r_{l+1} the fold by 4
// f_l -> f_{l+2}, its tree and round l + 2's pass.  One host synchronisation per round either way.  A layer that is not committed is never built.
// `grouped` (la = 2, a commitment with log_group = 2): every layer's leaves hold the sides of the step that starts there, so its tree is a quarter
// (the final fold-2 step's: half) as large and a step opens one path.
// grind_bits > 0: the proof-of-work step between T_R and the indices, its nonce into *nonce_out.
template <class F, class Form> int open_with(const zk_fri_commitment *cm, Form &form, uint32_t f, uint32_t Q, unsigned la, bool grouped, Transcript &tr, const OpenOut &o,
                                             uint32_t grind_bits = 0, uint64_t *nonce_out = nullptr) {
    constexpr size_t ESZ = sizeof(Fe<F>);
    constexpr int W = F::N / 2;
    constexpr unsigned K = Form::kSums;
    const auto t0 = std::chrono::steady_clock::now();
    const unsigned d = cm->d, b = cm->b, L = d + b, R = d - f;
    const size_t n = (size_t)1 << d, N = (size_t)1 << L, m = (size_t)1 << f;
    const Fe<F> one = fe_one<F>(), c = cm->has_coset ? load_host<F>(cm->coset) : one;
    const FriSchedule sc(L, R, la, grouped);

    // the header, (the arity when it is not 1,) root_0, the form's claim; several tables: the header, the form's tag and roots, its claim
    uint8_t cbe[32], abe[8];
    host_to_bytes_be<F>(c, cbe);
    transcript_header(tr, d, b, f, Q, cbe);
    unsigned root_shift = 0;                                  // the roots in front of the later layers' beyond root_0
    if constexpr (Form::kBatch) {
        form.statement(tr, la, grouped, o.roots);
        root_shift = form.nroots() - 1;
    } else {
        if (la == 2) {
            put_be32(abe, la);
            put_be32(abe + 4, 1);
            tr.append(abe, grouped ? 8 : 4);
        }
        memcpy(o.roots, cm->root, 32);
        tr.append(cm->root, 32);
    }
    form.absorb(tr);

    // one block: T_1 .. T_R (below n elements), the form's weights, the committed layers below R (C = their N >> l entries together: below N
    // for la = 1, below N / 3 for la = 2), their trees (2 G digests: G = C, or grouped the layers' leaves together, below C / 4 + 1), the
    // workgroups' partial sums and the K sums
    const size_t cap = (size_t)reduce_block_cap();
    size_t f_off[kFriMaxLayers] = {0}, t_off[kFriMaxLayers] = {0}, C = 0, G = 0;   // of step s's layer, in entries from off_f; of its tree, in digests from off_tree
    for (unsigned s = 1; s < sc.nsteps; s++) {
        f_off[s] = C;
        t_off[s] = 2 * G;
        C += N >> sc.step[s].layer;
        G += (N >> sc.step[s].layer) >> sc.leaf_group(s);
    }
    const size_t off_w = n, off_f = off_w + form.weight_room(n), off_tree = off_f + C, off_part = off_tree + 2 * G, total = off_part + K * cap + K;   // in elements (a digest is 32 bytes too)
    static_assert(ESZ == 32, "the block is laid out in 32-byte units");
    DevBuf blk;
    ZK_TRY(blk.alloc(total * ESZ));
    char *base = (char *)blk.p;
    void *T0 = cm->coeffs->dptr;                              // several tables: their combination, behind the weights
    if constexpr (Form::kBatch) T0 = form.table0 = base + (off_w + form.table0_off(n)) * ESZ;
    auto T_at = [&](unsigned l) -> void * { return l == 0 ? T0 : base + (n - (n >> (l - 1))) * ESZ; };          // n >> l entries
    auto w_at = [&](unsigned l) -> void * { return base + (off_w + form.weight_off(n, l)) * ESZ; };
    auto f_at = [&](unsigned s) -> void * { return s == 0 ? cm->codeword->dptr : base + (off_f + f_off[s]) * ESZ; };          // step s's layer
    auto tree_at = [&](unsigned s) -> uint64_t * { return s == 0 ? cm->levels : (uint64_t *)(base + (off_tree + t_off[s]) * ESZ); };   // twice its leaves in digests of room
    const PassMem mem{T0, base + off_w * ESZ, base + off_part * ESZ, base + (off_part + K * cap) * ESZ};

    Events ev;
    std::vector<size_t> ta(R), tb_(R), tc(R), td(R);
    size_t e0, e1;
    FoldTables<F> pw;
    ZK_TRY(pw.build(L));
    FriLayers fl = sc.layers();
    for (unsigned s = 0; s < sc.nsteps; s++) {
        fl.table[s] = f_at(s);
        fl.tree[s] = tree_at(s);
    }

    ZK_TRY(ev.mark(&e0));
    ZK_TRY(form.start(cm, tr, mem));
    Fe<F> S[K];
    ZK_HIP(zk::memcpy_on_stream(S, mem.sums, K * ESZ, hipMemcpyDeviceToHost));   // round 0's synchronisation
    form.release();
    ZK_TRY(ev.mark(&e1));

    Fe<F> cl = c, gscale = fe_inv<F>(fe_mul<F>(fe_from_u64<F>(2), c)), cinv = fe_inv<F>(c);   // c_l, 1 / (2 c_l), c_l^-1
    Fe<F> r_s = one, c_s = c, gscale_s = gscale;              // the same at the layer of step s, and the challenge drawn there
    unsigned s = 0;                                           // the last step whose layer exists
    for (unsigned l = 0; l < R; l++) {
        Fe<F> g[3];
        form.round_poly(l, S, tr, g);
        for (int k = 0; k < 3; k++) {
            store_host<F>(o.round_polys + ((size_t)l * 3 + k) * W, g[k]);
            tr.append_be<F>(g[k]);
        }
        const Fe<F> r = tr.random_challenge_as_field_element<F>();
        if (o.challenges) store_host<F>(o.challenges + (size_t)l * W, r);
        form.bind(l, r);
        if (l == sc.step[s].layer) {
            r_s = r;
            c_s = cl;
            gscale_s = gscale;
        }
        ZK_TRY(ev.mark(&ta[l]));
        if (l + 1 < R) {
            // the challenge that ends step s: the next committed layer (step s's folded by 2 or by 4), its tree, and round l + 1's pass (which folds
            // T_l and the weights by r_l) behind one another; one wait for the root and the sums.  The first challenge of a fold by 4: the pass alone.
            const bool commit = s + 1 < sc.nsteps && sc.step[s + 1].layer == l + 1;
            const size_t len = N >> (l + 1);
            uint64_t *tree = nullptr;
            uint8_t *root = nullptr;
            if (commit) {
                tree = tree_at(s + 1);
                root = o.roots + 32 * (size_t)(sc.step[s + 1].root + root_shift);
                const Fe<F> *shift = cm->has_coset ? &c_s : nullptr;
                const Fe<F> g_s = fe_mul<F>(r_s, gscale_s);
                const Fe<F> g_1 = fe_mul<F>(r, gscale);         // a fold by 4's second multiplier
                bool folded = false;
                if constexpr (Form::kBatch) {                 // layer 0 is the form's: k codewords, combined as they are folded
                    if (s == 0) {
                        ZK_TRY(form.fold0(f_at(1), N, pw, g_s, sc.step[0].log_sides == 2 ? &g_1 : nullptr, shift));
                        folded = true;
                    }
                }
                if (!folded) {
                    if (sc.step[s].log_sides == 2) ZK_TRY((launch_fold4<F>(f_at(s), f_at(s + 1), 4 * len, l - 1, pw, g_s, g_1, shift)));
                    else ZK_TRY((launch_fold<F>(f_at(s), f_at(s + 1), 2 * len, l, pw, g_s, shift)));
                }
            }
            ZK_TRY(ev.mark(&tb_[l]));
            if (commit) {
                const zk_table layer{cm->field, len, f_at(s + 1), 0};
                ZK_TRY(merkle_levels_grouped_device(&layer, sc.leaf_group(s + 1), tree));
            }
            ZK_TRY(ev.mark(&tc[l]));
            ZK_TRY(Form::pass(true, T_at(l), w_at(l), T_at(l + 1), w_at(l + 1), n >> (l + 2), r, mem.partials, mem.sums));
            if (commit) ZK_HIP(hipMemcpyAsync(root, tree + 4 * (2 * (len >> sc.leaf_group(s + 1)) - 2), 32, hipMemcpyDeviceToHost, cur_stream()));
            ZK_HIP(zk::memcpy_on_stream(S, mem.sums, K * ESZ, hipMemcpyDeviceToHost));   // the round's synchronisation
            if (commit) {
                tr.append(root, 32);
                s++;
            }
        } else {
            // the last challenge: T_R = the final table of the sumcheck and the final coefficients of the codeword at once; layer R itself is
            // never needed (nothing queries it), so its fold is not run
            ZK_TRY(ev.mark(&tb_[l]));
            ZK_TRY(ev.mark(&tc[l]));
            uint64_t r64[W];
            store_host<F>(r64, r);
            ZK_TRY(zk_mle_fold_ptr(cm->field, T_at(l), n >> l, d - l - 1, r64, T_at(R), cur_stream()));
            ZK_HIP(zk::memcpy_on_stream(o.final_table, T_at(R), m * ESZ, hipMemcpyDeviceToHost));
        }
        ZK_TRY(ev.mark(&td[l]));
        gscale = fe_mul<F>(gscale, cinv);                     // 1 / (2 c_{l+1}) = (1 / (2 c_l)) c_l^-1
        cinv = fe_sqr<F>(cinv);
        cl = fe_sqr<F>(cl);
    }
    for (size_t j = 0; j < m; j++) tr.append_be<F>(load_host<F>(o.final_table + j * W));

    zk_fri_ml_stats st{};
    if constexpr (Form::kBatch) ZK_TRY((answer_queries_batch<F>(tr, form.cws, form.ntables(), form.trees, form.nroots(), fl, sc, Q, o.query_indices, o.query_values, o.query_paths, ev, &st.ms_queries, grind_bits, nonce_out)));
    else ZK_TRY((answer_queries<F>(tr, fl, sc, Q, o.query_indices, o.query_values, o.query_paths, ev, &st.ms_queries, grind_bits, nonce_out)));
    st.rounds = R;
    st.queries = Q;
    st.ms_sumcheck = ev.ms(e0, e1);                           // what precedes round 0, and round 0's pass
    for (unsigned l = 0; l < R; l++) {
        st.ms_folds += ev.ms(ta[l], tb_[l]);
        st.ms_trees += ev.ms(tb_[l], tc[l]);
        st.ms_sumcheck += ev.ms(tc[l], td[l]);
    }
    st.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g_ml_stats = st;
    return ZK_OK;
}

// the statuses of an opening of `cm` that need no device: ZK_E_ARG for Q or f out of range or a z_i that is not reduced, and for a commitment
// whose leaves are not grouped by `log_group` (the ungrouped openers walk cm->levels as 2 N - 1 digests)
int open_check(const zk_fri_commitment *cm, const uint64_t *z, uint32_t f, uint32_t Q, unsigned log_group = 0) {
    if (Q < 1 || Q > 4096 || f >= cm->d || cm->log_group != log_group) return ZK_E_ARG;
    if (z && !all_reduced(cm->field, z, cm->d)) return ZK_E_ARG;
    return ZK_OK;
}

// ---- the succinct basic sumcheck's verifier (host) -----------------------------------------------------------------------------------
// verifier.rs:23-71 on the root; *good = the rounds hold and end in y; challenges: d elements
template <class F> void sumcheck_replay(Transcript &tr, const uint8_t *root32, unsigned d, const uint64_t *claimed_sum, const uint64_t *round_polys,
                                        const uint64_t *y, uint64_t *challenges, bool *good) {
    constexpr int W = F::N / 2;
    tr.append(root32, 32);                                   // :34-35, the commitment in place of the table's bytes
    Fe<F> cur = load_host<F>(claimed_sum);
    *good = is_reduced<F>(claimed_sum) && is_reduced<F>(y);
    tr.append_be<F>(cur);                                    // :36-37
    for (unsigned i = 0; i < d; i++) {                       // :47
        const uint64_t *p0 = round_polys + (size_t)2 * i * W, *p1 = p0 + W;
        const Fe<F> e0 = load_host<F>(p0), e1 = load_host<F>(p1);
        *good = *good && is_reduced<F>(p0) && is_reduced<F>(p1) && fe_eq<F>(fe_add<F>(e0, e1), cur);   // :53-56
        tr.append_be<F>(e0);                                 // :58-59
        tr.append_be<F>(e1);
        const Fe<F> r = tr.random_challenge_as_field_element<F>();   // :61
        store_host<F>(challenges + (size_t)i * W, r);
        cur = fe_add<F>(e0, fe_mul<F>(r, fe_sub<F>(e1, e0)));        // :64
    }
    *good = *good && fe_eq<F>(cur, load_host<F>(y));         // :67-70 with `evaluate` replaced by the opened value
}

int open_one(const zk_fri_commitment *cm, const uint64_t *z, uint32_t f, uint32_t Q, Transcript &tr, uint64_t *y_out, const OpenOut &o) {
    FRI_DISPATCH(cm->field, OnePoint<F> form{z, y_out, cm->d}; return open_with<F>(cm, form, f, Q, 1, false, tr, o));
    return ZK_OK;
}

// the public verifiers' body: the statuses that precede fri_verify_core's, and root_0.  roots[0] is the verifier's own, so the proof's copy
// must be the same bytes and the core gets a copy of the roots that starts with the caller's
int verify_opening(int field, const uint8_t *root32, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset,
                   const FriMlClaim &ml, zk_transcript *t, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                   const uint8_t *query_paths, int *ok, uint32_t grind_bits = 0, uint64_t pow_nonce = 0, uint32_t max_tables = ZK_FRI_ML_BATCH_MAX) {
    if (grind_bits > ZK_FRI_GRIND_MAX_BITS) return ZK_E_ARG;
    if (ml.weighted_c ? (!ml.challenges || !ml.w_final) : (!ml.z || !ml.y)) return ZK_E_ARG;
    if (!root32 || !ml.round_polys || !roots || !final_table || !query_values || !query_paths || !ok) return ZK_E_ARG;
    if (field_limbs64(field) < 0 || log_blowup < 1 || log_blowup > 8 || nqueries < 1 || nqueries > 4096 || d < 1 || log_final >= d) return ZK_E_ARG;
    if (ml.log_arity == 2 && d - log_final < 2) return ZK_E_ARG;
    if (coset && is_zero_element(field, coset)) return ZK_E_ARG;
    if (d > 32) return ZK_E_RANGE;                           // what sizes the copy below; fri_verify_core repeats these and checks the rest
    const size_t own = ml.ncommit ? ml.ncommit : ml.ntables ? ml.ntables : 1;   // the roots the verifier holds itself: root32 has that many
    std::vector<uint8_t> rs(roots, roots + (size_t)32 * (own - 1 + FriSchedule(d + log_blowup, d - log_final, ml.log_arity).nsteps));
    const bool same_root = memcmp(roots, root32, 32 * own) == 0;
    memcpy(rs.data(), root32, 32 * own);
    Transcript fresh;
    int good = 0;
    ZK_TRY(fri_verify_core(field, d, log_blowup, log_final, nqueries, coset, t ? t->t : fresh, rs.data(), final_table, query_values, query_paths, &good, nullptr, &ml, grind_bits, pow_nonce, max_tables));
    *ok = good && same_root ? 1 : 0;
    return ZK_OK;
}

// what the several-point openers of one commitment and of k check alike, every ZK_E_ARG before the device is asked for: the outputs, P, the
// arity, open_check on the (first) commitment with the leaf grouping its protocol needs, R >= 2 at log_arity 2, reduced points
int open_points_check(const zk_fri_commitment *cm, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                      unsigned log_group, const uint64_t *ys_out, const OpenOut &o) {
    if (!cm || !points || !ys_out || !o.round_polys || !o.roots || !o.final_table || !o.query_values || !o.query_paths) return ZK_E_ARG;
    if (npoints < 1 || npoints > 8 || log_arity < 1 || log_arity > 2) return ZK_E_ARG;
    ZK_TRY(open_check(cm, nullptr, log_final, nqueries, log_group));
    if (log_arity == 2 && cm->d - log_final < 2) return ZK_E_ARG;
    if (!all_reduced(cm->field, points, (size_t)npoints * cm->d)) return ZK_E_ARG;
    return require_device();
}

// zk_fri_ml_open_batch_pow's statuses, every ZK_E_ARG and then the device check: the step's arguments, k, one field, size, blow-up, coset and
// leaf grouping, the grouping's arity, and open_points_check on the first commitment
int open_batch_check(const zk_fri_commitment *const *cms, uint32_t k, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries,
                     uint32_t log_arity, const uint64_t *ys_out, const OpenOut &o, uint32_t grinding_bits, const uint64_t *pow_nonce,
                     uint32_t max_tables = ZK_FRI_ML_BATCH_MAX) {
    if (grinding_bits > ZK_FRI_GRIND_MAX_BITS || (grinding_bits && !pow_nonce)) return ZK_E_ARG;
    if (!cms || k < 1 || k > max_tables || !cms[0]) return ZK_E_ARG;
    const zk_fri_commitment *c0 = cms[0];
    for (uint32_t j = 1; j < k; j++) {                        // one field, size, blow-up, coset and leaf grouping
        const zk_fri_commitment *cj = cms[j];
        if (!cj || cj->field != c0->field || cj->d != c0->d || cj->b != c0->b || cj->log_group != c0->log_group || cj->has_coset != c0->has_coset) return ZK_E_ARG;
        if (c0->has_coset && memcmp(cj->coset, c0->coset, sizeof c0->coset) != 0) return ZK_E_ARG;
    }
    if ((c0->log_group != 0 && c0->log_group != 2) || (c0->log_group == 2 && log_arity != 2)) return ZK_E_ARG;
    return open_points_check(c0, points, npoints, log_final, nqueries, log_arity, c0->log_group, ys_out, o);
}

// the several-point verifiers' claim; ntables = 0: one table
FriMlClaim claim_of(const uint64_t *points, uint32_t npoints, const uint64_t *ys, const uint64_t *round_polys, uint32_t log_arity, bool grouped,
                    uint32_t ntables) {
    FriMlClaim ml{points, ys, round_polys};
    ml.npoints = npoints;
    ml.log_arity = log_arity;
    ml.grouped = grouped;
    ml.ntables = ntables;
    return ml;
}

// zk_fri_ml_open_columns_pow's statuses, every ZK_E_ARG and then the device check; *view (may be null) = the first commitment's shape as the
// driver reads it (d, b, coset; its table, codeword and tree stand for layer 0, which the form supplies), *K = the columns together
int open_columns_check(const zk_fri_columns *const *cms, uint32_t m, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries,
                       const uint64_t *ys_out, const OpenOut &o, uint32_t grinding_bits, const uint64_t *pow_nonce, zk_fri_commitment *view, uint32_t *K) {
    if (grinding_bits > ZK_FRI_GRIND_MAX_BITS || (grinding_bits && !pow_nonce)) return ZK_E_ARG;
    if (!cms || m < 1 || m > ZK_FRI_ML_WIDE_MAX || !cms[0]) return ZK_E_ARG;
    const zk_fri_columns *c0 = cms[0];
    uint32_t total = 0;
    for (uint32_t j = 0; j < m; j++) {                        // one field, size, blow-up and coset; at most ZK_FRI_ML_WIDE_MAX columns
        const zk_fri_columns *cj = cms[j];
        if (!cj || cj->field != c0->field || cj->d != c0->d || cj->b != c0->b || cj->has_coset != c0->has_coset) return ZK_E_ARG;
        if (c0->has_coset && memcmp(cj->coset, c0->coset, sizeof c0->coset) != 0) return ZK_E_ARG;
        total += cj->k;
        if (total > ZK_FRI_ML_WIDE_MAX) return ZK_E_ARG;
    }
    zk_fri_commitment v{};
    v.field = c0->field;
    v.d = c0->d;
    v.b = c0->b;
    v.has_coset = c0->has_coset;
    memcpy(v.coset, c0->coset, sizeof v.coset);
    v.coeffs = c0->coeffs[0];
    v.codeword = c0->codeword[0];
    v.levels = c0->levels;
    v.log_group = 2;
    if (view) *view = v;
    if (K) *K = total;
    return open_points_check(&v, points, npoints, log_final, nqueries, 2, 2, ys_out, o);
}

}  // namespace

int zk::fri_ml_open_columns_check(const zk_fri_columns *const *cms, uint32_t m, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries,
                                  const uint64_t *ys_out, uint64_t *round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *query_values,
                                  uint8_t *query_paths, uint32_t grinding_bits, const uint64_t *pow_nonce) {
    return open_columns_check(cms, m, points, npoints, log_final, nqueries, ys_out, OpenOut{round_polys, roots, final_table, nullptr, nullptr, query_values, query_paths},
                              grinding_bits, pow_nonce, nullptr, nullptr);
}

int zk::fri_ml_open_batch_check(const zk_fri_commitment *const *cms, uint32_t k, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries,
                                uint32_t log_arity, const uint64_t *ys_out, uint64_t *round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *query_values,
                                uint8_t *query_paths, uint32_t grinding_bits, const uint64_t *pow_nonce, uint32_t max_tables) {
    return open_batch_check(cms, k, points, npoints, log_final, nqueries, log_arity, ys_out, OpenOut{round_polys, roots, final_table, nullptr, nullptr, query_values, query_paths},
                            grinding_bits, pow_nonce, max_tables);
}

int zk::fri_ml_open_weighted_check(const zk_fri_commitment *cm, const zk_table *weights, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                                   const uint64_t *c_out, uint64_t *round_polys, uint8_t *roots, uint64_t *final_table, const uint64_t *challenges,
                                   uint64_t *query_values, uint8_t *query_paths, uint32_t grinding_bits, const uint64_t *pow_nonce) {
    if (grinding_bits > ZK_FRI_GRIND_MAX_BITS || (grinding_bits && !pow_nonce)) return ZK_E_ARG;
    if (!cm || !weights || !c_out || !round_polys || !roots || !final_table || !challenges || !query_values || !query_paths) return ZK_E_ARG;
    if (log_arity < 1 || log_arity > 2 || (cm->log_group != 0 && cm->log_group != 2) || (cm->log_group == 2 && log_arity != 2)) return ZK_E_ARG;
    ZK_TRY(open_check(cm, nullptr, log_final, nqueries, cm->log_group));
    if (log_arity == 2 && cm->d - log_final < 2) return ZK_E_ARG;
    if (weights->field != cm->field) return ZK_E_ARG;
    if (weights->len != (size_t)1 << cm->d) return ZK_E_LEN_MISMATCH;
    return require_device();
}

extern "C" {

int zk_fri_ml_fold(const zk_table *codeword, const uint64_t *r, const uint64_t *coset, zk_table **out) {
    ZK_TRY(fold_check(codeword, r && out, coset, 1));
    FRI_DISPATCH(codeword->field, return fold_once<F>(codeword, r, coset, out));
    return ZK_OK;
}

int zk_fri_ml_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, size_t *nroots, size_t *nfinal, size_t *nvalues,
                    size_t *path_bytes, size_t *nround) {
    ZK_TRY(zk_fri_proof_sizes(d, log_blowup, log_final, nqueries, nroots, nfinal, nvalues, path_bytes));
    if (nround) *nround = (size_t)3 * (d - log_final);
    return ZK_OK;
}

int zk_fri_ml_open(const zk_fri_commitment *cm, const uint64_t *z, uint32_t log_final, uint32_t nqueries, zk_transcript *t, uint64_t *y_out,
                   uint64_t *round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *challenges, uint64_t *query_indices, uint64_t *query_values,
                   uint8_t *query_paths) {
    if (!cm || !z || !y_out || !round_polys || !roots || !final_table || !query_values || !query_paths) return ZK_E_ARG;
    ZK_TRY(open_check(cm, z, log_final, nqueries));
    ZK_TRY(require_device());
    Transcript fresh;
    return open_one(cm, z, log_final, nqueries, t ? t->t : fresh, y_out, OpenOut{round_polys, roots, final_table, challenges, query_indices, query_values, query_paths});
}

int zk_fri_ml_verify(int field, const uint8_t *root32, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset,
                     const uint64_t *z, const uint64_t *y, zk_transcript *t, const uint64_t *round_polys, const uint8_t *roots, const uint64_t *final_table,
                     const uint64_t *query_values, const uint8_t *query_paths, int *ok) {
    return verify_opening(field, root32, d, log_blowup, log_final, nqueries, coset, FriMlClaim{z, y, round_polys}, t, roots, final_table, query_values, query_paths, ok);
}

int zk_fri_ml_round(const zk_table *T, const zk_table *W, const uint64_t *r, zk_table **T_out, zk_table **W_out, uint64_t *g3) {
    if (!T || !W || !g3 || (r && (!T_out || !W_out)) || T->field != W->field || (T->field != ZK_FR381 && T->field != ZK_BN254_FR)) return ZK_E_ARG;
    if (T->len != W->len) return ZK_E_LEN_MISMATCH;
    if (!is_pow2(T->len)) return ZK_E_NOT_POW2;
    if (T->len < (r ? 4u : 2u) || (r && !all_reduced(T->field, r, 1))) return ZK_E_ARG;
    ZK_TRY(require_device());
    FRI_DISPATCH(T->field, return round_once<F>(T, W, r, T_out, W_out, g3));
    return ZK_OK;
}

int zk_fri_ml_open_points(const zk_fri_commitment *cm, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries, zk_transcript *t,
                          uint64_t *ys_out, uint64_t *gamma_out, uint64_t *round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *challenges,
                          uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths) {
    return zk_fri_ml_open_points_arity(cm, points, npoints, log_final, nqueries, 1, t, ys_out, gamma_out, round_polys, roots, final_table, challenges, query_indices,
                                       query_values, query_paths);
}

int zk_fri_ml_open_points_arity(const zk_fri_commitment *cm, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                                zk_transcript *t, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *round_polys, uint8_t *roots, uint64_t *final_table,
                                uint64_t *challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths) {
    const OpenOut o{round_polys, roots, final_table, challenges, query_indices, query_values, query_paths};
    ZK_TRY(open_points_check(cm, points, npoints, log_final, nqueries, log_arity, 0, ys_out, o));
    Transcript fresh;
    FRI_DISPATCH(cm->field, ManyPoints<F> form{points, npoints, ys_out, gamma_out, cm->d}; return open_with<F>(cm, form, log_final, nqueries, log_arity, false, t ? t->t : fresh, o));
    return ZK_OK;
}

int zk_fri_ml_verify_points_arity(int field, const uint8_t *root32, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                                  const uint64_t *coset, const uint64_t *points, uint32_t npoints, const uint64_t *ys, zk_transcript *t,
                                  const uint64_t *round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                                  const uint8_t *query_paths, int *ok) {
    if (npoints < 1 || npoints > 8 || log_arity < 1 || log_arity > 2) return ZK_E_ARG;
    return verify_opening(field, root32, d, log_blowup, log_final, nqueries, coset, claim_of(points, npoints, ys, round_polys, log_arity, false, 0), t, roots,
                          final_table, query_values, query_paths, ok);
}

int zk_fri_ml_fold4(const zk_table *codeword, const uint64_t *r0, const uint64_t *r1, const uint64_t *coset, zk_table **out) {
    ZK_TRY(fold_check(codeword, r0 && r1 && out, coset, 2));
    FRI_DISPATCH(codeword->field, return fold4_once<F>(codeword, r0, r1, coset, out));
    return ZK_OK;
}

int zk_fri_ml_sizes_arity(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, size_t *nroots, size_t *nfinal,
                          size_t *nvalues, size_t *path_bytes, size_t *nround) {
    if (log_arity < 1 || log_arity > 2) return ZK_E_ARG;
    ZK_TRY(zk_fri_ml_sizes(d, log_blowup, log_final, nqueries, nroots, nfinal, nvalues, path_bytes, nround));
    if (log_arity == 1) return ZK_OK;
    if (d - log_final < 2) return ZK_E_ARG;
    const FriSchedule sc(d + log_blowup, d - log_final, log_arity);
    if (nroots) *nroots = sc.nsteps;
    if (nvalues) *nvalues = (size_t)nqueries * sc.nvalues;
    if (path_bytes) *path_bytes = (size_t)nqueries * sc.ndigests * 32;
    return ZK_OK;
}

// the hook's statuses and body for k <= max_tables
static int fold_batch_capped(const zk_table *const *codewords, uint32_t k, uint32_t max_tables, const uint64_t *coeffs, const uint64_t *r0, const uint64_t *r1,
                             const uint64_t *coset, zk_table **out) {
    if (!codewords || k < 1 || k > max_tables || !codewords[0]) return ZK_E_ARG;
    for (uint32_t j = 1; j < k; j++) {
        if (!codewords[j] || codewords[j]->field != codewords[0]->field) return ZK_E_ARG;
        if (codewords[j]->len != codewords[0]->len) return ZK_E_LEN_MISMATCH;
    }
    ZK_TRY(fold_check(codewords[0], coeffs && r0 && out, coset, r1 ? 2 : 1));
    FRI_DISPATCH(codewords[0]->field, return fold_batch_once<F>(codewords, k, coeffs, r0, r1, coset, out));
    return ZK_OK;
}
int zk_fri_ml_fold_batch(const zk_table *const *codewords, uint32_t k, const uint64_t *coeffs, const uint64_t *r0, const uint64_t *r1, const uint64_t *coset,
                         zk_table **out) {
    return fold_batch_capped(codewords, k, ZK_FRI_ML_BATCH_MAX, coeffs, r0, r1, coset, out);
}
int zk_fri_ml_fold_batch_wide(const zk_table *const *codewords, uint32_t k, const uint64_t *coeffs, const uint64_t *r0, const uint64_t *r1, const uint64_t *coset,
                              zk_table **out) {
    return fold_batch_capped(codewords, k, ZK_FRI_ML_WIDE_MAX, coeffs, r0, r1, coset, out);
}

static int sizes_batch_capped(uint32_t k, uint32_t max_tables, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                              uint32_t log_group, size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nround) {
    if (k < 1 || k > max_tables || (log_group != 0 && log_group != 2) || (log_group == 2 && log_arity != 2)) return ZK_E_ARG;
    size_t nr = 0, nv = 0, pb = 0;
    if (log_group) ZK_TRY(zk_fri_ml_sizes_grouped(d, log_blowup, log_final, nqueries, &nr, nfinal, &nv, &pb, nround));
    else ZK_TRY(zk_fri_ml_sizes_arity(d, log_blowup, log_final, nqueries, log_arity, &nr, nfinal, &nv, &pb, nround));
    const FriSchedule sc(d + log_blowup, d - log_final, log_arity, log_group != 0);
    const size_t v0 = sc.nsteps > 1 ? sc.step[1].val_off : sc.nvalues, d0 = sc.nsteps > 1 ? sc.step[1].path_off : sc.ndigests;   // step 0's share
    if (nroots) *nroots = k + nr - 1;
    if (nvalues) *nvalues = nv + (size_t)(k - 1) * nqueries * v0;
    if (path_bytes) *path_bytes = pb + (size_t)(k - 1) * nqueries * d0 * 32;
    return ZK_OK;
}
int zk_fri_ml_sizes_batch(uint32_t k, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group,
                          size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nround) {
    return sizes_batch_capped(k, ZK_FRI_ML_BATCH_MAX, d, log_blowup, log_final, nqueries, log_arity, log_group, nroots, nfinal, nvalues, path_bytes, nround);
}
int zk_fri_ml_sizes_batch_wide(uint32_t k, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group,
                               size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nround) {
    return sizes_batch_capped(k, ZK_FRI_ML_WIDE_MAX, d, log_blowup, log_final, nqueries, log_arity, log_group, nroots, nfinal, nvalues, path_bytes, nround);
}

int zk_fri_ml_open_batch(const zk_fri_commitment *const *cms, uint32_t k, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries,
                         uint32_t log_arity, zk_transcript *t, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *round_polys, uint8_t *roots, uint64_t *final_table,
                         uint64_t *challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths) {
    return zk_fri_ml_open_batch_pow(cms, k, points, npoints, log_final, nqueries, log_arity, t, ys_out, gamma_out, round_polys, roots, final_table, challenges,
                                    query_indices, query_values, query_paths, 0, nullptr);
}

static int open_batch_capped(const zk_fri_commitment *const *cms, uint32_t k, uint32_t max_tables, const uint64_t *points, uint32_t npoints, uint32_t log_final,
                             uint32_t nqueries, uint32_t log_arity, zk_transcript *t, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *round_polys, uint8_t *roots,
                             uint64_t *final_table, uint64_t *challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths,
                             uint32_t grinding_bits, uint64_t *pow_nonce) {
    const OpenOut o{round_polys, roots, final_table, challenges, query_indices, query_values, query_paths};
    ZK_TRY(open_batch_check(cms, k, points, npoints, log_final, nqueries, log_arity, ys_out, o, grinding_bits, pow_nonce, max_tables));
    const zk_fri_commitment *c0 = cms[0];
    Transcript fresh;
    FRI_DISPATCH(c0->field, ManyTables<F> form(cms, k, points, npoints, ys_out, gamma_out, c0->d);
                 return open_with<F>(c0, form, log_final, nqueries, log_arity, c0->log_group == 2, t ? t->t : fresh, o, grinding_bits, pow_nonce));
    return ZK_OK;
}
int zk_fri_ml_open_batch_pow(const zk_fri_commitment *const *cms, uint32_t k, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries,
                             uint32_t log_arity, zk_transcript *t, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *round_polys, uint8_t *roots,
                             uint64_t *final_table, uint64_t *challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths,
                             uint32_t grinding_bits, uint64_t *pow_nonce) {
    return open_batch_capped(cms, k, ZK_FRI_ML_BATCH_MAX, points, npoints, log_final, nqueries, log_arity, t, ys_out, gamma_out, round_polys, roots, final_table,
                             challenges, query_indices, query_values, query_paths, grinding_bits, pow_nonce);
}
int zk_fri_ml_open_batch_wide_pow(const zk_fri_commitment *const *cms, uint32_t k, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries,
                                  uint32_t log_arity, zk_transcript *t, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *round_polys, uint8_t *roots,
                                  uint64_t *final_table, uint64_t *challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths,
                                  uint32_t grinding_bits, uint64_t *pow_nonce) {
    return open_batch_capped(cms, k, ZK_FRI_ML_WIDE_MAX, points, npoints, log_final, nqueries, log_arity, t, ys_out, gamma_out, round_polys, roots, final_table,
                             challenges, query_indices, query_values, query_paths, grinding_bits, pow_nonce);
}

int zk_fri_ml_verify_batch(int field, const uint8_t *roots_of_f, uint32_t k, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries,
                           uint32_t log_arity, uint32_t log_group, const uint64_t *coset, const uint64_t *points, uint32_t npoints, const uint64_t *ys,
                           zk_transcript *t, const uint64_t *round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                           const uint8_t *query_paths, int *ok) {
    return zk_fri_ml_verify_batch_pow(field, roots_of_f, k, d, log_blowup, log_final, nqueries, log_arity, log_group, coset, points, npoints, ys, t, round_polys,
                                      roots, final_table, query_values, query_paths, 0, 0, ok);
}

static int verify_batch_capped(int field, const uint8_t *roots_of_f, uint32_t k, uint32_t max_tables, uint32_t d, uint32_t log_blowup, uint32_t log_final,
                               uint32_t nqueries, uint32_t log_arity, uint32_t log_group, const uint64_t *coset, const uint64_t *points, uint32_t npoints,
                               const uint64_t *ys, zk_transcript *t, const uint64_t *round_polys, const uint8_t *roots, const uint64_t *final_table,
                               const uint64_t *query_values, const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce, int *ok) {
    if (grinding_bits > ZK_FRI_GRIND_MAX_BITS) return ZK_E_ARG;
    if (k < 1 || k > max_tables || npoints < 1 || npoints > 8 || log_arity < 1 || log_arity > 2) return ZK_E_ARG;
    if ((log_group != 0 && log_group != 2) || (log_group == 2 && log_arity != 2)) return ZK_E_ARG;
    return verify_opening(field, roots_of_f, d, log_blowup, log_final, nqueries, coset, claim_of(points, npoints, ys, round_polys, log_arity, log_group == 2, k), t,
                          roots, final_table, query_values, query_paths, ok, grinding_bits, pow_nonce, max_tables);
}
int zk_fri_ml_verify_batch_pow(int field, const uint8_t *roots_of_f, uint32_t k, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries,
                               uint32_t log_arity, uint32_t log_group, const uint64_t *coset, const uint64_t *points, uint32_t npoints, const uint64_t *ys,
                               zk_transcript *t, const uint64_t *round_polys, const uint8_t *roots, const uint64_t *final_table,
                               const uint64_t *query_values, const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce, int *ok) {
    return verify_batch_capped(field, roots_of_f, k, ZK_FRI_ML_BATCH_MAX, d, log_blowup, log_final, nqueries, log_arity, log_group, coset, points, npoints, ys, t,
                               round_polys, roots, final_table, query_values, query_paths, grinding_bits, pow_nonce, ok);
}
int zk_fri_ml_verify_batch_wide_pow(int field, const uint8_t *roots_of_f, uint32_t k, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries,
                                    uint32_t log_arity, uint32_t log_group, const uint64_t *coset, const uint64_t *points, uint32_t npoints, const uint64_t *ys,
                                    zk_transcript *t, const uint64_t *round_polys, const uint8_t *roots, const uint64_t *final_table,
                                    const uint64_t *query_values, const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce, int *ok) {
    return verify_batch_capped(field, roots_of_f, k, ZK_FRI_ML_WIDE_MAX, d, log_blowup, log_final, nqueries, log_arity, log_group, coset, points, npoints, ys, t,
                               round_polys, roots, final_table, query_values, query_paths, grinding_bits, pow_nonce, ok);
}

// ---- column commitments opened together --------------------------------------------------------------------------------------------
// m >= 1 widths, each >= 1, together at most ZK_FRI_ML_WIDE_MAX; *K = their sum
static int widths_check(const uint32_t *widths, uint32_t m, uint32_t *K) {
    if (!widths || m < 1 || m > ZK_FRI_ML_WIDE_MAX) return ZK_E_ARG;
    uint32_t total = 0;
    for (uint32_t i = 0; i < m; i++) {
        if (widths[i] < 1 || widths[i] > ZK_FRI_COLUMNS_MAX) return ZK_E_ARG;
        total += widths[i];
        if (total > ZK_FRI_ML_WIDE_MAX) return ZK_E_ARG;
    }
    *K = total;
    return ZK_OK;
}
int zk_fri_ml_sizes_columns(const uint32_t *widths, uint32_t m, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, size_t *nroots,
                            size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nround) {
    uint32_t K = 0;
    ZK_TRY(widths_check(widths, m, &K));
    size_t nr = 0, nv = 0, pb = 0;
    ZK_TRY(zk_fri_ml_sizes_grouped(d, log_blowup, log_final, nqueries, &nr, nfinal, &nv, &pb, nround));
    const FriSchedule sc(d + log_blowup, d - log_final, 2, true);
    const size_t v0 = sc.nsteps > 1 ? sc.step[1].val_off : sc.nvalues, d0 = sc.nsteps > 1 ? sc.step[1].path_off : sc.ndigests;   // step 0's share: 4 values, L - 2 digests
    if (nroots) *nroots = m + nr - 1;
    if (nvalues) *nvalues = nv + (size_t)(K - 1) * nqueries * v0;
    if (path_bytes) *path_bytes = pb + (size_t)(m - 1) * nqueries * d0 * 32;
    return ZK_OK;
}

int zk_fri_ml_open_columns_pow(const zk_fri_columns *const *cms, uint32_t m, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries,
                               uint32_t grinding_bits, zk_transcript *t, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *round_polys, uint8_t *roots,
                               uint64_t *final_table, uint64_t *challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths,
                               uint64_t *pow_nonce) {
    const OpenOut o{round_polys, roots, final_table, challenges, query_indices, query_values, query_paths};
    zk_fri_commitment view{};
    uint32_t K = 0, widths[ZK_FRI_ML_WIDE_MAX];
    ZK_TRY(open_columns_check(cms, m, points, npoints, log_final, nqueries, ys_out, o, grinding_bits, pow_nonce, &view, &K));
    for (uint32_t i = 0; i < m; i++) widths[i] = cms[i]->k;
    Transcript fresh;
    FRI_DISPATCH(view.field, ManyTables<F> form(cms, m, widths, points, npoints, ys_out, gamma_out, view.d);
                 return open_with<F>(&view, form, log_final, nqueries, 2, true, t ? t->t : fresh, o, grinding_bits, pow_nonce));
    return ZK_OK;
}

int zk_fri_ml_verify_columns_pow(int field, const uint8_t *roots_of_f, const uint32_t *widths, uint32_t m, uint32_t d, uint32_t log_blowup, uint32_t log_final,
                                 uint32_t nqueries, uint32_t grinding_bits, const uint64_t *coset, const uint64_t *points, uint32_t npoints, const uint64_t *ys,
                                 zk_transcript *t, const uint64_t *round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                                 const uint8_t *query_paths, uint64_t pow_nonce, int *ok) {
    if (grinding_bits > ZK_FRI_GRIND_MAX_BITS || npoints < 1 || npoints > 8) return ZK_E_ARG;
    uint32_t K = 0;
    ZK_TRY(widths_check(widths, m, &K));
    FriMlClaim ml = claim_of(points, npoints, ys, round_polys, 2, true, K);
    ml.widths = widths;
    ml.ncommit = m;
    return verify_opening(field, roots_of_f, d, log_blowup, log_final, nqueries, coset, ml, t, roots, final_table, query_values, query_paths, ok, grinding_bits,
                          pow_nonce, ZK_FRI_ML_WIDE_MAX);
}

int zk_fri_ml_sizes_grouped(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, size_t *nroots, size_t *nfinal, size_t *nvalues,
                            size_t *path_bytes, size_t *nround) {
    ZK_TRY(zk_fri_ml_sizes_arity(d, log_blowup, log_final, nqueries, 2, nroots, nfinal, nvalues, path_bytes, nround));
    if (path_bytes) *path_bytes = (size_t)nqueries * FriSchedule(d + log_blowup, d - log_final, 2, true).ndigests * 32;
    return ZK_OK;
}

int zk_fri_ml_open_points_grouped(const zk_fri_commitment *cm, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries, zk_transcript *t,
                                  uint64_t *ys_out, uint64_t *gamma_out, uint64_t *round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *challenges,
                                  uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths) {
    const OpenOut o{round_polys, roots, final_table, challenges, query_indices, query_values, query_paths};
    ZK_TRY(open_points_check(cm, points, npoints, log_final, nqueries, 2, 2, ys_out, o));
    Transcript fresh;
    FRI_DISPATCH(cm->field, ManyPoints<F> form{points, npoints, ys_out, gamma_out, cm->d}; return open_with<F>(cm, form, log_final, nqueries, 2, true, t ? t->t : fresh, o));
    return ZK_OK;
}

int zk_fri_ml_verify_points_grouped(int field, const uint8_t *root32, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset,
                                    const uint64_t *points, uint32_t npoints, const uint64_t *ys, zk_transcript *t, const uint64_t *round_polys,
                                    const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values, const uint8_t *query_paths, int *ok) {
    if (npoints < 1 || npoints > 8) return ZK_E_ARG;
    return verify_opening(field, root32, d, log_blowup, log_final, nqueries, coset, claim_of(points, npoints, ys, round_polys, 2, true, 0), t, roots, final_table,
                          query_values, query_paths, ok);
}

int zk_fri_ml_verify_points(int field, const uint8_t *root32, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset,
                            const uint64_t *points, uint32_t npoints, const uint64_t *ys, zk_transcript *t, const uint64_t *round_polys, const uint8_t *roots,
                            const uint64_t *final_table, const uint64_t *query_values, const uint8_t *query_paths, int *ok) {
    return zk_fri_ml_verify_points_arity(field, root32, d, log_blowup, log_final, nqueries, 1, coset, points, npoints, ys, t, round_polys, roots, final_table,
                                         query_values, query_paths, ok);
}

// ---- the opening against a weight table ----------------------------------------------------------------------------------------------
int zk_fri_ml_sizes_weighted(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group, size_t *nroots,
                             size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nround) {
    return zk_fri_ml_sizes_batch(1, d, log_blowup, log_final, nqueries, log_arity, log_group, nroots, nfinal, nvalues, path_bytes, nround);
}

int zk_fri_ml_open_weighted(const zk_fri_commitment *cm, const zk_table *weights, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t grinding_bits,
                            zk_transcript *t, uint64_t *c_out, uint64_t *round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *challenges,
                            uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths, uint64_t *pow_nonce) {
    const OpenOut o{round_polys, roots, final_table, challenges, query_indices, query_values, query_paths};
    ZK_TRY(zk::fri_ml_open_weighted_check(cm, weights, log_final, nqueries, log_arity, c_out, round_polys, roots, final_table, challenges, query_values, query_paths,
                                          grinding_bits, pow_nonce));
    Transcript fresh;
    FRI_DISPATCH(cm->field, Weighted<F> form{weights->dptr, c_out, cm->d};
                 return open_with<F>(cm, form, log_final, nqueries, log_arity, cm->log_group == 2, t ? t->t : fresh, o, grinding_bits, pow_nonce));
    return ZK_OK;
}

int zk_fri_ml_verify_weighted(int field, const uint8_t *root32, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                              uint32_t log_group, const uint64_t *coset, const uint64_t *c, const uint64_t *challenges, const uint64_t *w_final, zk_transcript *t,
                              const uint64_t *round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                              const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce, int *ok) {
    if (!c || log_arity < 1 || log_arity > 2 || (log_group != 0 && log_group != 2) || (log_group == 2 && log_arity != 2)) return ZK_E_ARG;
    FriMlClaim ml{nullptr, nullptr, round_polys};
    ml.log_arity = log_arity;
    ml.grouped = log_group == 2;
    ml.weighted_c = c;
    ml.challenges = challenges;
    ml.w_final = w_final;
    return verify_opening(field, root32, d, log_blowup, log_final, nqueries, coset, ml, t, roots, final_table, query_values, query_paths, ok, grinding_bits, pow_nonce);
}

int zk_fri_ml_last_stats(zk_fri_ml_stats *out) {
    if (!out) return ZK_E_ARG;
    *out = g_ml_stats;
    return ZK_OK;
}

int zk_sumcheck_basic_prove_succinct(const zk_fri_commitment *cm, uint32_t log_final, uint32_t nqueries, zk_transcript *t, uint64_t *claimed_sum,
                                     uint64_t *round_polys, uint64_t *challenges, uint64_t *y_out, uint64_t *open_round_polys, uint8_t *roots,
                                     uint64_t *final_table, uint64_t *open_challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths) {
    if (!cm || !claimed_sum || !round_polys || !challenges || !y_out || !open_round_polys || !roots || !final_table || !query_values || !query_paths) return ZK_E_ARG;
    ZK_TRY(open_check(cm, nullptr, log_final, nqueries));
    ZK_TRY(require_device());
    Transcript fresh;
    Transcript &tr = t ? t->t : fresh;
    ZK_TRY(sumcheck_basic_prove_bound(cm->coeffs, tr, cm->root, claimed_sum, round_polys, challenges));
    return open_one(cm, challenges, log_final, nqueries, tr, y_out, OpenOut{open_round_polys, roots, final_table, open_challenges, query_indices, query_values, query_paths});
}

int zk_sumcheck_basic_verify_succinct(int field, const uint8_t *root32, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries,
                                      const uint64_t *coset, zk_transcript *t, const uint64_t *claimed_sum, const uint64_t *round_polys, const uint64_t *y,
                                      const uint64_t *open_round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                                      const uint8_t *query_paths, int *ok) {
    if (!root32 || !claimed_sum || !round_polys || !y || !open_round_polys || !roots || !final_table || !query_values || !query_paths || !ok) return ZK_E_ARG;
    // every status before the transcript is touched: the opening's own checks on an empty replay
    size_t nroots = 0;
    if (field_limbs64(field) < 0) return ZK_E_ARG;
    ZK_TRY(zk_fri_proof_sizes(d, log_blowup, log_final, nqueries, &nroots, nullptr, nullptr, nullptr));
    if (coset && is_zero_element(field, coset)) return ZK_E_ARG;
    if ((field != ZK_FR381 && field != ZK_BN254_FR) || d + log_blowup > two_adicity(field)) return ZK_E_RANGE;
    Transcript fresh;
    Transcript &tr = t ? t->t : fresh;
    std::vector<uint64_t> chal((size_t)d * 4);
    bool good = false;
    FRI_DISPATCH(field, sumcheck_replay<F>(tr, root32, d, claimed_sum, round_polys, y, chal.data(), &good));
    int open_ok = 0;
    zk_transcript *tt = t;
    zk_transcript own;
    if (!tt) { own.t = tr; tt = &own; }
    ZK_TRY(zk_fri_ml_verify(field, root32, d, log_blowup, log_final, nqueries, coset, chal.data(), y, tt, open_round_polys, roots, final_table, query_values,
                            query_paths, &open_ok));
    *ok = good && open_ok ? 1 : 0;
    return ZK_OK;
}

}  // extern "C"
