// zkmle_fri_ml.hip -- C ABI of the multilinear opening of a FRI commitment (fri_ml.cuh): one Lagrange-form fold, the opening (a sumcheck
// of sum_x T[x] eq(x, z) interleaved with the folds of the codeword, on the same challenges), its host verifier, and the basic sumcheck
// that ends in such an opening; and the opening at several points with one proof (a sumcheck against the gamma-combination of the points'
// eq tables: "FRI commitment opened at several points").  Extension: the reference leaves `fri/` empty; the protocol is defined in
// include/zkmle.h "FRI commitment opened as a multilinear polynomial".
#include <string.h>

#include <chrono>
#include <vector>

#include "context.h"
#include "eq_table.cuh"
#include "fri_ml.cuh"
#include "transcript.h"

using namespace zk;

namespace {

struct DevBuf {   // RAII block of the caching pool
    void *p = nullptr;
    ~DevBuf() { pool_free(p); }
    int alloc(size_t bytes) { return pool_alloc(bytes, &p); }
};
struct Events {
    std::vector<hipEvent_t> ev;
    ~Events() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    int mark(size_t *id) {
        hipEvent_t e;
        ZK_HIP(hipEventCreate(&e));
        ev.push_back(e);
        ZK_HIP(hipEventRecord(e, cur_stream()));
        *id = ev.size() - 1;
        return ZK_OK;
    }
    float ms(size_t a, size_t b) const {
        float v = 0.f;
        return hipEventElapsedTime(&v, ev[a], ev[b]) == hipSuccess ? v : 0.f;
    }
};

thread_local zk_fri_ml_stats g_ml_stats{};

#define ML_DISPATCH(field_id, ...)                                         \
    switch (field_id) {                                                    \
        case ZK_FR381: { using F = ::zk::Fr381; __VA_ARGS__; } break;      \
        case ZK_BN254_FR: { using F = ::zk::Bn254Fr; __VA_ARGS__; } break; \
        default: return ZK_E_RANGE;                                        \
    }

template <class F> Fe<F> load_host(const uint64_t *src) {
    Fe<F> e;
    memcpy(e.l, src, sizeof(uint32_t) * F::N);
    return e;
}
template <class F> void store_host(uint64_t *dst, const Fe<F> &e) { memcpy(dst, e.l, sizeof(uint32_t) * F::N); }
template <class F> bool is_reduced(const uint64_t *el) {
    const Fe<F> x = load_host<F>(el);
    for (int i = F::N - 1; i >= 0; i--)
        if (x.l[i] != F::p(i)) return x.l[i] < F::p(i);
    return false;
}
bool all_reduced(int field, const uint64_t *els, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!(field == ZK_FR381 ? is_reduced<Fr381>(els + i * 4) : is_reduced<Bn254Fr>(els + i * 4))) return false;
    return true;
}
bool is_zero_element(int field, const uint64_t *x) {
    uint64_t v = 0;
    for (int k = 0; k < field_limbs64(field); k++) v |= x[k];
    return v == 0;
}
unsigned two_adicity(int field) {
    uint32_t s = 0;
    return zk_ntt_two_adicity(field, &s) == ZK_OK ? s : 0;
}
template <class F> Fe<F> root_of_unity(unsigned log_n) {
    uint64_t w[F::N / 2];
    (void)zk_ntt_root_of_unity(F::ID, log_n, w);
    return load_host<F>(w);
}
void put_be32(uint8_t *out, uint32_t v) {
    for (int k = 0; k < 4; k++) out[k] = (uint8_t)(v >> (24 - 8 * k));
}
// eq1(a, b) = a b + (1 - a)(1 - b)
template <class F> Fe<F> eq1(const Fe<F> &a, const Fe<F> &b) {
    const Fe<F> one = fe_one<F>();
    return fe_add<F>(fe_mul<F>(a, b), fe_mul<F>(fe_sub<F>(one, a), fe_sub<F>(one, b)));
}

// the powers of w_N^-1 below N / 2, N = 2^log_n, as ntt_pow2t reads them (zkmle_fri.hip FoldTables): layer l indexes them with k << l
template <class F> struct FoldTables {
    DevBuf buf;
    const void *lo = nullptr, *hi = nullptr;
    int build(unsigned log_n) {
        const size_t half = (size_t)1 << (log_n - 1);
        const bool two = half > ((size_t)1 << kNttLoBits);
        const size_t lo_count = two ? (size_t)1 << kNttLoBits : half, hi_count = two ? half >> kNttLoBits : 0;
        const size_t off_hi = (lo_count * sizeof(Ufe<F>) + 63) / 64 * 64;
        ZK_TRY(buf.alloc(off_hi + (hi_count + 1) * sizeof(Fe<F>)));
        const Fe<F> winv = fe_inv<F>(root_of_unity<F>(log_n)), one = fe_one<F>();
        const size_t blocks = (lo_count + kNttBlock - 1) / kNttBlock;
        ntt_pow_table_kernel<F, true><<<(unsigned)blocks, kNttBlock, 0, cur_stream()>>>(winv, one, (uint32_t)lo_count, buf.p);
        ZK_HIP(hipGetLastError());
        lo = buf.p;
        if (two) {
            Fe<F> step = winv;
            for (unsigned k = 0; k < kNttLoBits; k++) step = fe_sqr<F>(step);
            const size_t hb = (hi_count + kNttBlock - 1) / kNttBlock;
            ntt_pow_table_kernel<F, false><<<(unsigned)(hb < 1024 ? hb : 1024), kNttBlock, 0, cur_stream()>>>(step, one, (uint32_t)hi_count, (char *)buf.p + off_hi);
            ZK_HIP(hipGetLastError());
            hi = (char *)buf.p + off_hi;
        }
        return ZK_OK;
    }
};
// out[k], k < len / 2, from in[0 .. len): gamma = r / (2 c_l), `shift` = the layer's number, c = c_l (null: 1)
template <class F> int launch_fold(const void *in, void *out, size_t len, unsigned shift, const FoldTables<F> &tb, const Fe<F> &gamma, const Fe<F> *c) {
    UniMul<F> um;
    unimul_from<F>(um, gamma);
    FriUni g;
    memcpy(g.t, um.t, sizeof g.t);
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
    UniMul<F> um;
    unimul_from<F>(um, g0);
    FriUni g;
    memcpy(g.t, um.t, sizeof g.t);
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

// ---- the prover ----------------------------------------------------------------------------------------------------------------
struct OpenOut {
    uint64_t *y, *round_polys;
    uint8_t *roots;
    uint64_t *final_table, *challenges, *query_indices, *query_values;
    uint8_t *query_paths;
};

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

// the queries: FRI's step 5 and FRI's gather over the layers of `fl` (layer 0 = the commitment's codeword and tree); *ms = the gather with
// its downloads.  Ends with the stream drained.  fl.wide (the opening folded by 4): the layers are steps of four or two sides and the
// indices are taken mod N / 4.
template <class F> int answer_queries(Transcript &tr, const FriLayers &fl, unsigned L, unsigned R, uint32_t Q, const OpenOut &o, Events &ev, float *ms) {
    constexpr size_t ESZ = sizeof(Fe<F>);
    std::vector<uint64_t> idx(Q);
    for (unsigned q = 0; q < Q; q++) {
        uint8_t dg[32];
        tr.sample_random_challenge(dg);
        uint64_t v = 0;
        for (int k = 0; k < 8; k++) v |= (uint64_t)dg[k] << (8 * k);
        idx[q] = v & (((uint64_t)1 << (L - (fl.wide ? 2 : 1))) - 1);
    }
    if (o.query_indices) memcpy(o.query_indices, idx.data(), Q * 8);
    const size_t nval = (size_t)Q * (fl.wide ? fl.val_off[fl.nlayers] : R * 2), ndig = (size_t)Q * fl.path_off[fl.nlayers];
    DevBuf didx, dval, dpath;
    ZK_TRY(didx.alloc(Q * 8));
    ZK_TRY(dval.alloc(nval * ESZ));
    ZK_TRY(dpath.alloc(ndig * 32));
    size_t q0, q1;
    ZK_TRY(ev.mark(&q0));
    ZK_HIP(hipMemcpyAsync(didx.p, idx.data(), Q * 8, hipMemcpyHostToDevice, cur_stream()));
    fri_query_values_kernel<F><<<(unsigned)((nval + kFriBlock - 1) / kFriBlock), kFriBlock, 0, cur_stream()>>>(fl, (const uint64_t *)didx.p, Q, dval.p);
    ZK_HIP(hipGetLastError());
    fri_query_paths_kernel<<<(unsigned)((ndig + kFriBlock - 1) / kFriBlock), kFriBlock, 0, cur_stream()>>>(fl, (const uint64_t *)didx.p, Q, (uint64_t *)dpath.p);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(o.query_values, dval.p, nval * ESZ, hipMemcpyDeviceToHost, cur_stream()));   // one download each, one wait for both
    ZK_HIP(zk::memcpy_on_stream(o.query_paths, dpath.p, ndig * 32, hipMemcpyDeviceToHost));
    ZK_TRY(ev.mark(&q1));
    ZK_HIP(hipEventSynchronize(ev.ev[q1]));
    *ms = ev.ms(q0, q1);
    return ZK_OK;
}

template <class F> int open_any(const zk_fri_commitment *cm, const uint64_t *z, uint32_t f, uint32_t Q, Transcript &tr, const OpenOut &o) {
    constexpr size_t ESZ = sizeof(Fe<F>);
    constexpr int W = F::N / 2;
    const auto t0 = std::chrono::steady_clock::now();
    const unsigned d = cm->d, b = cm->b, L = d + b, R = d - f;
    const size_t n = (size_t)1 << d, N = (size_t)1 << L, m = (size_t)1 << f;
    const Fe<F> one = fe_one<F>(), c = cm->has_coset ? load_host<F>(cm->coset) : one;

    // steps 1 to 3 up to y: the header, root_0, the point
    uint8_t hdr[48];
    put_be32(hdr, d);
    put_be32(hdr + 4, b);
    put_be32(hdr + 8, f);
    put_be32(hdr + 12, Q);
    host_to_bytes_be<F>(c, hdr + 16);
    tr.append(hdr, sizeof hdr);
    memcpy(o.roots, cm->root, 32);
    tr.append(cm->root, 32);
    for (unsigned i = 0; i < d; i++) tr.append_be<F>(load_host<F>(z + (size_t)i * W));

    // one block: T_1 .. T_R (below n elements), E_0 .. E_{R-1} (below n), f_1 .. f_{R-1} (below N), their trees (below 2 N digests), the
    // workgroups' partial sums and the two sums
    const size_t cap = (size_t)reduce_block_cap();
    const size_t off_e = n, off_f = 2 * n, off_tree = off_f + N, off_part = off_tree + 2 * N, total = off_part + 2 * cap + 2;   // in elements (a digest is 32 bytes too)
    static_assert(ESZ == 32, "the block is laid out in 32-byte units");
    DevBuf blk;
    ZK_TRY(blk.alloc(total * ESZ));
    char *base = (char *)blk.p;
    auto T_at = [&](unsigned l) -> void * { return l == 0 ? cm->coeffs->dptr : base + (n - (n >> (l - 1))) * ESZ; };          // n >> l entries
    auto E_at = [&](unsigned l) -> void * { return base + (off_e + n - (n >> l)) * ESZ; };                                   // n >> (l + 1) entries
    auto f_at = [&](unsigned l) -> void * { return l == 0 ? cm->codeword->dptr : base + (off_f + N - (N >> (l - 1))) * ESZ; };   // N >> l entries
    auto tree_at = [&](unsigned l) -> uint64_t * { return l == 0 ? cm->levels : (uint64_t *)(base + (off_tree + 2 * N - ((4 * N) >> l)) * ESZ); };   // 2 N >> l digests of room
    void *partials = base + off_part * ESZ, *sums = base + (off_part + 2 * cap) * ESZ;

    Events ev;
    std::vector<size_t> ta(R), tb_(R), tc(R), td(R);
    size_t e0, e1;
    FoldTables<F> pw;
    ZK_TRY(pw.build(L));
    FriLayers fl{};
    fl.log_len0 = L;
    fl.nlayers = R;

    // round 0's pass: E_0 = the eq table of (z_0 .. z_{d-2}), S_0 and S_1 from the commitment's own coefficient table, which is only read
    ZK_TRY(ev.mark(&e0));
    EqBuilder<F> eqb;
    ZK_TRY(eqb.build(z, d - 1, E_at(0)));
    ZK_TRY((launch_round<F>(false, T_at(0), E_at(0), nullptr, nullptr, n / 2, one, partials, sums)));
    Fe<F> S[2];
    ZK_HIP(zk::memcpy_on_stream(S, sums, 2 * ESZ, hipMemcpyDeviceToHost));      // round 0's synchronisation
    eqb.release();
    ZK_TRY(ev.mark(&e1));

    Fe<F> A = one, cl = c, gscale = fe_inv<F>(fe_mul<F>(fe_from_u64<F>(2), c)), cinv = fe_inv<F>(c);   // A_l, c_l, 1 / (2 c_l), c_l^-1
    const Fe<F> two = fe_from_u64<F>(2), three = fe_from_u64<F>(3);
    for (unsigned l = 0; l < R; l++) {
        const Fe<F> zv = load_host<F>(z + (size_t)(d - 1 - l) * W);
        // g_l(X) = A_l eq1(X, z_v) (S_0 + X (S_1 - S_0)) at 0, 1, 2: eq1(0, z) = 1 - z, eq1(1, z) = z, eq1(2, z) = 3 z - 1
        const Fe<F> g0 = fe_mul<F>(A, fe_mul<F>(fe_sub<F>(one, zv), S[0])), g1 = fe_mul<F>(A, fe_mul<F>(zv, S[1]));
        const Fe<F> g2 = fe_mul<F>(A, fe_mul<F>(fe_sub<F>(fe_mul<F>(three, zv), one), fe_sub<F>(fe_mul<F>(two, S[1]), S[0])));
        if (l == 0) {                                        // y = g_0(0) + g_0(1): the claim comes out of round 0's pass
            const Fe<F> y = fe_add<F>(g0, g1);
            store_host<F>(o.y, y);
            tr.append_be<F>(y);
        }
        store_host<F>(o.round_polys + ((size_t)l * 3) * W, g0);
        store_host<F>(o.round_polys + ((size_t)l * 3 + 1) * W, g1);
        store_host<F>(o.round_polys + ((size_t)l * 3 + 2) * W, g2);
        tr.append_be<F>(g0);
        tr.append_be<F>(g1);
        tr.append_be<F>(g2);
        const Fe<F> r = tr.random_challenge_as_field_element<F>();
        if (o.challenges) store_host<F>(o.challenges + (size_t)l * W, r);
        A = fe_mul<F>(A, eq1<F>(r, zv));

        fl.table[l] = f_at(l);
        fl.tree[l] = tree_at(l);
        fl.path_off[l + 1] = fl.path_off[l] + 2 * (L - l);
        ZK_TRY(ev.mark(&ta[l]));
        if (l + 1 < R) {
            // f_{l+1}, its tree, and round l + 1's pass (which folds T_l by r_l) behind one another; one wait for the root and the sums
            ZK_TRY((launch_fold<F>(f_at(l), f_at(l + 1), N >> l, l, pw, fe_mul<F>(r, gscale), cm->has_coset ? &cl : nullptr)));
            ZK_TRY(ev.mark(&tb_[l]));
            const zk_table layer{cm->field, N >> (l + 1), f_at(l + 1), 0};
            uint64_t *tree = tree_at(l + 1);
            ZK_TRY(merkle_levels_device(&layer, tree));
            ZK_TRY(ev.mark(&tc[l]));
            ZK_TRY((launch_round<F>(true, T_at(l), E_at(l), T_at(l + 1), E_at(l + 1), n >> (l + 2), r, partials, sums)));
            uint8_t *root = o.roots + 32 * (l + 1);
            ZK_HIP(hipMemcpyAsync(root, tree + 4 * (2 * layer.len - 2), 32, hipMemcpyDeviceToHost, cur_stream()));
            ZK_HIP(zk::memcpy_on_stream(S, sums, 2 * ESZ, hipMemcpyDeviceToHost));   // the round's synchronisation
            tr.append(root, 32);
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

    float ms_queries = 0.f;
    ZK_TRY((answer_queries<F>(tr, fl, L, R, Q, o, ev, &ms_queries)));

    zk_fri_ml_stats st{};
    st.rounds = R;
    st.queries = Q;
    st.ms_sumcheck = ev.ms(e0, e1);
    for (unsigned l = 0; l < R; l++) {
        st.ms_folds += ev.ms(ta[l], tb_[l]);
        st.ms_trees += ev.ms(tb_[l], tc[l]);
        st.ms_sumcheck += ev.ms(tc[l], td[l]);
    }
    st.ms_queries = ms_queries;
    st.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g_ml_stats = st;
    return ZK_OK;
}

// the statuses of an opening of `cm` that need no device: ZK_E_ARG for Q or f out of range or a z_i that is not reduced
int open_check(const zk_fri_commitment *cm, const uint64_t *z, uint32_t f, uint32_t Q) {
    if (Q < 1 || Q > 4096 || f >= cm->d) return ZK_E_ARG;
    if (z && !all_reduced(cm->field, z, cm->d)) return ZK_E_ARG;
    return ZK_OK;
}

// ---- the opening at several points ----------------------------------------------------------------------------------------------------
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

// la = log_arity.  1: every layer f_1 .. f_{R-1} is committed.  2 (R >= 2): the even ones are; after r_l with l even only round l + 1's pass
// runs, after r_{l+1} the fold by 4 f_l -> f_{l+2}, its tree and round l + 2's pass.  One host synchronisation per round either way.
template <class F> int open_points_any(const zk_fri_commitment *cm, const uint64_t *pts, uint32_t P, uint32_t f, uint32_t Q, unsigned la, Transcript &tr,
                                       uint64_t *ys_out, uint64_t *gamma_out, const OpenOut &o) {
    constexpr size_t ESZ = sizeof(Fe<F>);
    constexpr int W = F::N / 2;
    const auto t0 = std::chrono::steady_clock::now();
    const unsigned d = cm->d, b = cm->b, L = d + b, R = d - f;
    const size_t n = (size_t)1 << d, N = (size_t)1 << L, m = (size_t)1 << f;
    const Fe<F> one = fe_one<F>(), c = cm->has_coset ? load_host<F>(cm->coset) : one;

    // steps 1 to 4: the header, (the arity when it is not 1,) root_0, P, the points
    uint8_t hdr[48], pbe[4];
    put_be32(hdr, d);
    put_be32(hdr + 4, b);
    put_be32(hdr + 8, f);
    put_be32(hdr + 12, Q);
    host_to_bytes_be<F>(c, hdr + 16);
    tr.append(hdr, sizeof hdr);
    if (la == 2) {
        put_be32(pbe, la);
        tr.append(pbe, 4);
    }
    memcpy(o.roots, cm->root, 32);
    tr.append(cm->root, 32);
    put_be32(pbe, P);
    tr.append(pbe, 4);
    for (size_t i = 0; i < (size_t)P * d; i++) tr.append_be<F>(load_host<F>(pts + i * W));

    // one block: T_1 .. T_R (below n elements), W_0 .. W_{R-1} (below 2 n), the committed layers f_la, f_2la, .. below R (C = their N >> l
    // entries together: below N for la = 1, below N / 3 for la = 2), their trees (2 C digests), the workgroups' partial sums and the three sums,
    // and -- for P > 1 -- the P eq tables W_0 is combined from: 32 bytes x (3 n + 3 C + P n) and a little.  A layer that is not committed is
    // never built.
    const size_t cap = (size_t)reduce_block_cap();
    std::vector<size_t> f_off(R + 1, 0);                      // of the committed layer l, in entries from off_f; its tree at twice that from off_tree
    size_t C = 0;
    for (unsigned l = la; l < R; l += la) {
        f_off[l] = C;
        C += N >> l;
    }
    const size_t off_w = n, off_f = 3 * n, off_tree = off_f + C, off_part = off_tree + 2 * C, off_eq = off_part + 3 * cap + 3;
    const size_t total = off_eq + (P > 1 ? (size_t)P * n : 0);   // in elements (a digest is 32 bytes too)
    static_assert(ESZ == 32, "the block is laid out in 32-byte units");
    DevBuf blk;
    ZK_TRY(blk.alloc(total * ESZ));
    char *base = (char *)blk.p;
    auto T_at = [&](unsigned l) -> void * { return l == 0 ? cm->coeffs->dptr : base + (n - (n >> (l - 1))) * ESZ; };          // n >> l entries
    auto W_at = [&](unsigned l) -> void * { return base + (off_w + 2 * n - ((2 * n) >> l)) * ESZ; };                         // n >> l entries
    auto f_at = [&](unsigned l) -> void * { return l == 0 ? cm->codeword->dptr : base + (off_f + f_off[l]) * ESZ; };          // N >> l entries, l committed
    auto tree_at = [&](unsigned l) -> uint64_t * { return l == 0 ? cm->levels : (uint64_t *)(base + (off_tree + 2 * f_off[l]) * ESZ); };   // 2 N >> l digests of room
    void *partials = base + off_part * ESZ, *sums = base + (off_part + 3 * cap) * ESZ;

    Events ev;
    std::vector<size_t> ta(R), tb_(R), tc(R), td(R);
    size_t e0, e1;
    FoldTables<F> pw;
    ZK_TRY(pw.build(L));
    FriLayers fl{};
    fl.log_len0 = L;
    fl.nlayers = la == 2 ? (R + 1) / 2 : R;
    fl.wide = la == 2;

    // step 5: y_p = zk_mle_evaluate(T, z^p), a pass each; they are absorbed before gamma exists
    ZK_TRY(ev.mark(&e0));
    for (unsigned p = 0; p < P; p++) {
        ZK_TRY(zk_mle_evaluate(cm->coeffs, pts + (size_t)p * d * W, d, ys_out + (size_t)p * W));
        tr.append_be<F>(load_host<F>(ys_out + (size_t)p * W));
    }
    const Fe<F> gamma = tr.random_challenge_as_field_element<F>();
    if (gamma_out) store_host<F>(gamma_out, gamma);
    // W_0 = sum_p gamma^p eq(., z^p): one point's table is built in place, several are combined in one pass
    std::vector<EqBuilder<F>> eqb(P);
    if (P == 1) {
        ZK_TRY(eqb[0].build(pts, d, W_at(0)));
    } else {
        const void *tabs[8];
        uint64_t coef[8 * W];
        Fe<F> gp = one;
        for (unsigned p = 0; p < P; p++) {
            tabs[p] = base + (off_eq + (size_t)p * n) * ESZ;
            ZK_TRY(eqb[p].build(pts + (size_t)p * d * W, d, (void *)tabs[p]));
            store_host<F>(coef + (size_t)p * W, gp);
            gp = fe_mul<F>(gp, gamma);
        }
        ZK_HIP((lincomb_launch<F, false>(tabs, P, coef, W_at(0), n, fe_zero<F>(), fe_zero<F>(), nullptr, cur_stream())));
    }
    // round 0's pass reads the commitment's own coefficient table and W_0 and writes neither
    ZK_TRY((launch_round_w<F>(false, T_at(0), W_at(0), nullptr, nullptr, n / 2, one, partials, sums)));
    Fe<F> S[3];
    ZK_HIP(zk::memcpy_on_stream(S, sums, 3 * ESZ, hipMemcpyDeviceToHost));      // round 0's synchronisation
    for (auto &e : eqb) e.release();
    ZK_TRY(ev.mark(&e1));

    Fe<F> cl = c, gscale = fe_inv<F>(fe_mul<F>(fe_from_u64<F>(2), c)), cinv = fe_inv<F>(c);   // c_l, 1 / (2 c_l), c_l^-1
    Fe<F> r_prev = one, cl_prev = c, gscale_prev = gscale;    // la = 2, l odd: r_{l-1}, c_{l-1}, 1 / (2 c_{l-1})
    for (unsigned l = 0; l < R; l++) {
        Fe<F> g[3];
        nodes_to_g3<F>(S, g);
        for (int k = 0; k < 3; k++) {
            store_host<F>(o.round_polys + ((size_t)l * 3 + k) * W, g[k]);
            tr.append_be<F>(g[k]);
        }
        const Fe<F> r = tr.random_challenge_as_field_element<F>();
        if (o.challenges) store_host<F>(o.challenges + (size_t)l * W, r);

        if (la == 1) {
            fl.table[l] = f_at(l);
            fl.tree[l] = tree_at(l);
            fl.path_off[l + 1] = fl.path_off[l] + 2 * (L - l);
        } else if (l % 2 == 0) {                              // a step starts here: four sides if layer l + 2 exists, else the fold by 2 to layer R
            const unsigned s = l / 2, ls = l + 2 <= R ? 2 : 1;
            fl.table[s] = f_at(l);
            fl.tree[s] = tree_at(l);
            fl.log_len[s] = (uint8_t)(L - l);
            fl.log_sides[s] = (uint8_t)ls;
            fl.val_off[s + 1] = fl.val_off[s] + (1u << ls);
            fl.path_off[s + 1] = fl.path_off[s] + (L - l) * (1u << ls);
        }
        ZK_TRY(ev.mark(&ta[l]));
        if (la == 2 && l + 1 < R && l % 2 == 0) {
            // the first challenge of a step: nothing is committed for it; round l + 1's pass alone, and the wait for its sums
            ZK_TRY(ev.mark(&tb_[l]));
            ZK_TRY(ev.mark(&tc[l]));
            ZK_TRY((launch_round_w<F>(true, T_at(l), W_at(l), T_at(l + 1), W_at(l + 1), n >> (l + 2), r, partials, sums)));
            ZK_HIP(zk::memcpy_on_stream(S, sums, 3 * ESZ, hipMemcpyDeviceToHost));   // the round's synchronisation
            r_prev = r;
            cl_prev = cl;
            gscale_prev = gscale;
        } else if (la == 2 && l + 1 < R) {
            // the second: f_{l+1} = the fold by 4 of f_{l-1} by (r_{l-1}, r_l), its tree, and round l + 1's pass behind one another; one wait
            ZK_TRY((launch_fold4<F>(f_at(l - 1), f_at(l + 1), N >> (l - 1), l - 1, pw, fe_mul<F>(r_prev, gscale_prev), fe_mul<F>(r, gscale),
                                    cm->has_coset ? &cl_prev : nullptr)));
            ZK_TRY(ev.mark(&tb_[l]));
            const zk_table layer{cm->field, N >> (l + 1), f_at(l + 1), 0};
            uint64_t *tree = tree_at(l + 1);
            ZK_TRY(merkle_levels_device(&layer, tree));
            ZK_TRY(ev.mark(&tc[l]));
            ZK_TRY((launch_round_w<F>(true, T_at(l), W_at(l), T_at(l + 1), W_at(l + 1), n >> (l + 2), r, partials, sums)));
            uint8_t *root = o.roots + 32 * ((l + 1) / 2);
            ZK_HIP(hipMemcpyAsync(root, tree + 4 * (2 * layer.len - 2), 32, hipMemcpyDeviceToHost, cur_stream()));
            ZK_HIP(zk::memcpy_on_stream(S, sums, 3 * ESZ, hipMemcpyDeviceToHost));   // the round's synchronisation
            tr.append(root, 32);
        } else if (l + 1 < R) {
            // f_{l+1}, its tree, and round l + 1's pass (which folds T_l and W_l by r_l) behind one another; one wait for the root and the sums
            ZK_TRY((launch_fold<F>(f_at(l), f_at(l + 1), N >> l, l, pw, fe_mul<F>(r, gscale), cm->has_coset ? &cl : nullptr)));
            ZK_TRY(ev.mark(&tb_[l]));
            const zk_table layer{cm->field, N >> (l + 1), f_at(l + 1), 0};
            uint64_t *tree = tree_at(l + 1);
            ZK_TRY(merkle_levels_device(&layer, tree));
            ZK_TRY(ev.mark(&tc[l]));
            ZK_TRY((launch_round_w<F>(true, T_at(l), W_at(l), T_at(l + 1), W_at(l + 1), n >> (l + 2), r, partials, sums)));
            uint8_t *root = o.roots + 32 * (l + 1);
            ZK_HIP(hipMemcpyAsync(root, tree + 4 * (2 * layer.len - 2), 32, hipMemcpyDeviceToHost, cur_stream()));
            ZK_HIP(zk::memcpy_on_stream(S, sums, 3 * ESZ, hipMemcpyDeviceToHost));   // the round's synchronisation
            tr.append(root, 32);
        } else {
            // the last challenge: T_R alone is needed (W_R is the verifier's to compute); layer R is never built
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

    float ms_queries = 0.f;
    ZK_TRY((answer_queries<F>(tr, fl, L, R, Q, o, ev, &ms_queries)));

    zk_fri_ml_stats st{};
    st.rounds = R;
    st.queries = Q;
    st.ms_sumcheck = ev.ms(e0, e1);                           // the y_p passes, W_0 and round 0's pass
    for (unsigned l = 0; l < R; l++) {
        st.ms_folds += ev.ms(ta[l], tb_[l]);
        st.ms_trees += ev.ms(tb_[l], tc[l]);
        st.ms_sumcheck += ev.ms(tc[l], td[l]);
    }
    st.ms_queries = ms_queries;
    st.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g_ml_stats = st;
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

}  // namespace

extern "C" {

int zk_fri_ml_fold(const zk_table *codeword, const uint64_t *r, const uint64_t *coset, zk_table **out) {
    if (!codeword || !r || !out || field_limbs64(codeword->field) < 0 || codeword->len == 1) return ZK_E_ARG;
    if (coset && is_zero_element(codeword->field, coset)) return ZK_E_ARG;
    if (!is_pow2(codeword->len)) return ZK_E_NOT_POW2;
    if ((codeword->field != ZK_FR381 && codeword->field != ZK_BN254_FR) || ilog2(codeword->len) > two_adicity(codeword->field)) return ZK_E_RANGE;
    ZK_TRY(require_device());
    ML_DISPATCH(codeword->field, return fold_once<F>(codeword, r, coset, out));
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
    const OpenOut o{y_out, round_polys, roots, final_table, challenges, query_indices, query_values, query_paths};
    ML_DISPATCH(cm->field, return open_any<F>(cm, z, log_final, nqueries, t ? t->t : fresh, o));
    return ZK_OK;
}

int zk_fri_ml_verify(int field, const uint8_t *root32, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset,
                     const uint64_t *z, const uint64_t *y, zk_transcript *t, const uint64_t *round_polys, const uint8_t *roots, const uint64_t *final_table,
                     const uint64_t *query_values, const uint8_t *query_paths, int *ok) {
    if (!root32 || !z || !y || !round_polys || !roots || !final_table || !query_values || !query_paths || !ok) return ZK_E_ARG;
    if (field_limbs64(field) < 0 || log_blowup < 1 || log_blowup > 8 || nqueries < 1 || nqueries > 4096 || d < 1 || log_final >= d) return ZK_E_ARG;
    if (coset && is_zero_element(field, coset)) return ZK_E_ARG;
    if (d > 32) return ZK_E_RANGE;                           // what sizes the copy below; fri_verify_core repeats these and checks the rest
    // root_0 is the verifier's own: the proof's copy must be the same bytes
    std::vector<uint8_t> rs(roots, roots + (size_t)32 * (d - log_final));
    const bool same_root = memcmp(roots, root32, 32) == 0;
    memcpy(rs.data(), root32, 32);
    Transcript fresh;
    const FriMlClaim ml{z, y, round_polys};
    int good = 0;
    ZK_TRY(fri_verify_core(field, d, log_blowup, log_final, nqueries, coset, t ? t->t : fresh, rs.data(), final_table, query_values, query_paths, &good, nullptr, &ml));
    *ok = good && same_root ? 1 : 0;
    return ZK_OK;
}

int zk_fri_ml_round(const zk_table *T, const zk_table *W, const uint64_t *r, zk_table **T_out, zk_table **W_out, uint64_t *g3) {
    if (!T || !W || !g3 || (r && (!T_out || !W_out)) || T->field != W->field || (T->field != ZK_FR381 && T->field != ZK_BN254_FR)) return ZK_E_ARG;
    if (T->len != W->len) return ZK_E_LEN_MISMATCH;
    if (!is_pow2(T->len)) return ZK_E_NOT_POW2;
    if (T->len < (r ? 4u : 2u) || (r && !all_reduced(T->field, r, 1))) return ZK_E_ARG;
    ZK_TRY(require_device());
    ML_DISPATCH(T->field, return round_once<F>(T, W, r, T_out, W_out, g3));
    return ZK_OK;
}

int zk_fri_ml_open_points(const zk_fri_commitment *cm, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries, zk_transcript *t,
                          uint64_t *ys_out, uint64_t *gamma_out, uint64_t *round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *challenges,
                          uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths) {
    if (!cm || !points || !ys_out || !round_polys || !roots || !final_table || !query_values || !query_paths) return ZK_E_ARG;
    if (npoints < 1 || npoints > 8) return ZK_E_ARG;
    ZK_TRY(open_check(cm, nullptr, log_final, nqueries));
    if (!all_reduced(cm->field, points, (size_t)npoints * cm->d)) return ZK_E_ARG;
    ZK_TRY(require_device());
    Transcript fresh;
    const OpenOut o{nullptr, round_polys, roots, final_table, challenges, query_indices, query_values, query_paths};
    ML_DISPATCH(cm->field, return open_points_any<F>(cm, points, npoints, log_final, nqueries, 1, t ? t->t : fresh, ys_out, gamma_out, o));
    return ZK_OK;
}

int zk_fri_ml_open_points_arity(const zk_fri_commitment *cm, const uint64_t *points, uint32_t npoints, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                                zk_transcript *t, uint64_t *ys_out, uint64_t *gamma_out, uint64_t *round_polys, uint8_t *roots, uint64_t *final_table,
                                uint64_t *challenges, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths) {
    if (!cm || !points || !ys_out || !round_polys || !roots || !final_table || !query_values || !query_paths) return ZK_E_ARG;
    if (npoints < 1 || npoints > 8 || log_arity < 1 || log_arity > 2) return ZK_E_ARG;
    ZK_TRY(open_check(cm, nullptr, log_final, nqueries));
    if (log_arity == 2 && cm->d - log_final < 2) return ZK_E_ARG;
    if (!all_reduced(cm->field, points, (size_t)npoints * cm->d)) return ZK_E_ARG;
    ZK_TRY(require_device());
    Transcript fresh;
    const OpenOut o{nullptr, round_polys, roots, final_table, challenges, query_indices, query_values, query_paths};
    ML_DISPATCH(cm->field, return open_points_any<F>(cm, points, npoints, log_final, nqueries, log_arity, t ? t->t : fresh, ys_out, gamma_out, o));
    return ZK_OK;
}

int zk_fri_ml_verify_points_arity(int field, const uint8_t *root32, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                                  const uint64_t *coset, const uint64_t *points, uint32_t npoints, const uint64_t *ys, zk_transcript *t,
                                  const uint64_t *round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *query_values,
                                  const uint8_t *query_paths, int *ok) {
    if (!root32 || !points || !ys || !round_polys || !roots || !final_table || !query_values || !query_paths || !ok) return ZK_E_ARG;
    if (npoints < 1 || npoints > 8 || log_arity < 1 || log_arity > 2) return ZK_E_ARG;
    if (field_limbs64(field) < 0 || log_blowup < 1 || log_blowup > 8 || nqueries < 1 || nqueries > 4096 || d < 1 || log_final >= d) return ZK_E_ARG;
    if (log_arity == 2 && d - log_final < 2) return ZK_E_ARG;
    if (coset && is_zero_element(field, coset)) return ZK_E_ARG;
    if (d > 32) return ZK_E_RANGE;                           // what sizes the copy below; fri_verify_core repeats these and checks the rest
    const unsigned R = d - log_final;
    std::vector<uint8_t> rs(roots, roots + (size_t)32 * (log_arity == 2 ? (R + 1) / 2 : R));
    const bool same_root = memcmp(roots, root32, 32) == 0;
    memcpy(rs.data(), root32, 32);
    Transcript fresh;
    FriMlClaim ml{points, ys, round_polys};
    ml.npoints = npoints;
    ml.log_arity = log_arity;
    int good = 0;
    ZK_TRY(fri_verify_core(field, d, log_blowup, log_final, nqueries, coset, t ? t->t : fresh, rs.data(), final_table, query_values, query_paths, &good, nullptr, &ml));
    *ok = good && same_root ? 1 : 0;
    return ZK_OK;
}

int zk_fri_ml_fold4(const zk_table *codeword, const uint64_t *r0, const uint64_t *r1, const uint64_t *coset, zk_table **out) {
    if (!codeword || !r0 || !r1 || !out || field_limbs64(codeword->field) < 0 || codeword->len == 1 || codeword->len == 2) return ZK_E_ARG;
    if (coset && is_zero_element(codeword->field, coset)) return ZK_E_ARG;
    if (!is_pow2(codeword->len)) return ZK_E_NOT_POW2;
    if ((codeword->field != ZK_FR381 && codeword->field != ZK_BN254_FR) || ilog2(codeword->len) > two_adicity(codeword->field)) return ZK_E_RANGE;
    ZK_TRY(require_device());
    ML_DISPATCH(codeword->field, return fold4_once<F>(codeword, r0, r1, coset, out));
    return ZK_OK;
}

int zk_fri_ml_sizes_arity(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, size_t *nroots, size_t *nfinal,
                          size_t *nvalues, size_t *path_bytes, size_t *nround) {
    if (log_arity < 1 || log_arity > 2) return ZK_E_ARG;
    ZK_TRY(zk_fri_ml_sizes(d, log_blowup, log_final, nqueries, nroots, nfinal, nvalues, path_bytes, nround));
    if (log_arity == 1) return ZK_OK;
    const unsigned R = d - log_final, L = d + log_blowup;
    if (R < 2) return ZK_E_ARG;
    size_t digests = 0;
    for (unsigned l = 0; l < R; l += 2) digests += (size_t)(l + 2 <= R ? 4 : 2) * (L - l);
    if (nroots) *nroots = (R + 1) / 2;
    if (nvalues) *nvalues = (size_t)nqueries * (4 * (size_t)(R / 2) + 2 * (R % 2));
    if (path_bytes) *path_bytes = (size_t)nqueries * digests * 32;
    return ZK_OK;
}

int zk_fri_ml_verify_points(int field, const uint8_t *root32, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset,
                            const uint64_t *points, uint32_t npoints, const uint64_t *ys, zk_transcript *t, const uint64_t *round_polys, const uint8_t *roots,
                            const uint64_t *final_table, const uint64_t *query_values, const uint8_t *query_paths, int *ok) {
    if (!root32 || !points || !ys || !round_polys || !roots || !final_table || !query_values || !query_paths || !ok) return ZK_E_ARG;
    if (npoints < 1 || npoints > 8) return ZK_E_ARG;
    if (field_limbs64(field) < 0 || log_blowup < 1 || log_blowup > 8 || nqueries < 1 || nqueries > 4096 || d < 1 || log_final >= d) return ZK_E_ARG;
    if (coset && is_zero_element(field, coset)) return ZK_E_ARG;
    if (d > 32) return ZK_E_RANGE;                           // what sizes the copy below; fri_verify_core repeats these and checks the rest
    std::vector<uint8_t> rs(roots, roots + (size_t)32 * (d - log_final));
    const bool same_root = memcmp(roots, root32, 32) == 0;
    memcpy(rs.data(), root32, 32);
    Transcript fresh;
    FriMlClaim ml{points, ys, round_polys};
    ml.npoints = npoints;
    int good = 0;
    ZK_TRY(fri_verify_core(field, d, log_blowup, log_final, nqueries, coset, t ? t->t : fresh, rs.data(), final_table, query_values, query_paths, &good, nullptr, &ml));
    *ok = good && same_root ? 1 : 0;
    return ZK_OK;
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
    const OpenOut o{y_out, open_round_polys, roots, final_table, open_challenges, query_indices, query_values, query_paths};
    ML_DISPATCH(cm->field, return open_any<F>(cm, challenges, log_final, nqueries, tr, o));
    return ZK_OK;
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
    ML_DISPATCH(field, sumcheck_replay<F>(tr, root32, d, claimed_sum, round_polys, y, chal.data(), &good));
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
