// zkmle_fri.hip -- C ABI of the FRI low-degree proof (fri.cuh): one fold, the prover from a coefficient table or from a codeword, the
// host verifier.  Extension: the reference leaves `fri/` empty; layers, transcript and layouts are defined in include/zkmle.h.
#include <string.h>

#include <chrono>
#include <vector>

#include "fri_host.h"
#include "grind_host.h"
#include "univariate.h"

using namespace zk;
using namespace zk::host;

namespace {

thread_local zk_fri_stats g_fri_stats{};

// the checks on (b, f, Q) that need no length, then those that need d = the coefficient table's log2 length
int params_check(uint32_t b, uint32_t Q) { return b >= 1 && b <= 8 && Q >= 1 && Q <= 4096 ? ZK_OK : ZK_E_ARG; }

// ---- the fold ------------------------------------------------------------------------------------------------------------------
// out[k], k < len / 2, from in[0 .. len): gamma = beta / (2 c) of this layer, `shift` = the layer's number
template <class F> int launch_fold(const void *in, void *out, size_t len, unsigned shift, const FoldTables<F> &tb, const Fe<F> &gamma) {
    const size_t half = len / 2;
    fri_fold_kernel<F><<<(unsigned)((half + kFriBlock - 1) / kFriBlock), kFriBlock, 0, cur_stream()>>>(in, out, half, tb.lo, tb.hi, shift, fri_uni<F>(gamma));
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class F> int fold_once(const zk_table *cw, const uint64_t *beta, const uint64_t *coset, zk_table **out) {
    FoldTables<F> tb;
    ZK_TRY(tb.build(ilog2(cw->len)));
    Fe<F> den = fe_from_u64<F>(2);
    if (coset) den = fe_mul<F>(den, load_host<F>(coset));
    zk_table *o = nullptr;
    ZK_TRY(zk_table_alloc(cw->field, cw->len / 2, &o));
    const int rc = launch_fold<F>(cw->dptr, o->dptr, cw->len, 0, tb, fe_mul<F>(load_host<F>(beta), fe_inv<F>(den)));
    if (rc != ZK_OK) { zk_table_free(o); return rc; }
    *out = o;
    return ZK_OK;
}

// ---- the prover ----------------------------------------------------------------------------------------------------------------
struct ProofOut {
    uint8_t *roots;
    uint64_t *final_coeffs, *betas, *query_indices, *query_values;
    uint8_t *query_paths;
};

// `cw` = layer 0 (N = 2^L entries, L = d + b); events: `ev0` was recorded before the extension (or is the proof's first event)
template <class F> int prove_layers(const zk_table *cw, unsigned b, unsigned f, unsigned Q, const uint64_t *coset, Transcript &tr, const ProofOut &o,
                                    Events &ev, float *ms_trees, float *ms_folds, float *ms_queries, uint32_t grind_bits, uint64_t *nonce_out) {
    constexpr size_t ESZ = sizeof(Fe<F>);
    const unsigned L = ilog2(cw->len), d = L - b, R = d - f;
    const size_t N = cw->len, m = (size_t)1 << f;
    const Fe<F> c = coset ? load_host<F>(coset) : fe_one<F>();
    uint8_t cbe[32];
    host_to_bytes_be<F>(c, cbe);
    transcript_header(tr, d, b, f, Q, cbe);

    FoldTables<F> tb;
    ZK_TRY(tb.build(L));
    DevBuf trees;                                             // layer l's levels at digest offset 4 N - (4 N >> l): 2 N_l digests of room each
    ZK_TRY(trees.alloc(4 * N * 32));
    TableHolder layers;
    const FriSchedule sc(L, R, 1);
    FriLayers fl = sc.layers();

    std::vector<size_t> ta(R + 1), tf(R);
    const zk_table *cur = cw;
    Fe<F> gscale = fe_inv<F>(fe_mul<F>(fe_from_u64<F>(2), c)), cinv_sq = fe_inv<F>(c);   // 1 / (2 c_l), and c_l^-1 to step it: 1 / (2 c_{l+1}) = (1 / (2 c_l)) c_l^-1
    for (unsigned l = 0; l < R; l++) {
        uint64_t *tree = (uint64_t *)trees.p + 4 * (4 * N - ((4 * N) >> l));
        fl.table[l] = cur->dptr;
        fl.tree[l] = tree;
        ZK_TRY(ev.mark(&ta[l]));
        ZK_TRY(merkle_levels_device(cur, tree));
        uint8_t *root = o.roots + 32 * l;
        ZK_HIP(zk::memcpy_on_stream(root, tree + 4 * (2 * cur->len - 2), 32, hipMemcpyDeviceToHost));   // the layer's synchronisation
        tr.append(root, 32);
        const Fe<F> beta = tr.random_challenge_as_field_element<F>();
        if (o.betas) memcpy(o.betas + l * (F::N / 2), beta.l, ESZ);
        zk_table *next = nullptr;
        ZK_TRY(layers.alloc(cw->field, cur->len / 2, &next));
        ZK_TRY(ev.mark(&tf[l]));
        ZK_TRY((launch_fold<F>(cur->dptr, next->dptr, cur->len, l, tb, fe_mul<F>(beta, gscale))));
        gscale = fe_mul<F>(gscale, cinv_sq);
        cinv_sq = fe_sqr<F>(cinv_sq);
        cur = next;
    }
    ZK_TRY(ev.mark(&ta[R]));

    // layer R as coefficients: the inverse coset transform of its N >> R entries, of which the m low ones are sent
    zk_table *last = layers.v.back();
    Fe<F> cR = c;
    for (unsigned l = 0; l < R; l++) cR = fe_sqr<F>(cR);
    uint64_t cR64[F::N / 2];
    memcpy(cR64, cR.l, ESZ);
    ZK_TRY(zk_ntt(last, 1, coset ? cR64 : nullptr));
    ZK_HIP(zk::memcpy_on_stream(o.final_coeffs, last->dptr, m * ESZ, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < m; j++) tr.append_be<F>(load_host<F>(o.final_coeffs + j * (F::N / 2)));

    ZK_TRY((answer_queries<F>(tr, fl, sc, Q, o.query_indices, o.query_values, o.query_paths, ev, nullptr, grind_bits, nonce_out)));
    *ms_trees = *ms_folds = 0.f;
    for (unsigned l = 0; l < R; l++) {
        *ms_trees += ev.ms(ta[l], tf[l]);
        *ms_folds += ev.ms(tf[l], ta[l + 1]);
    }
    *ms_queries = ev.since(ta[R]);                            // the last layer's transform and download, then the gather
    return ZK_OK;
}

// the statuses of a proof over a layer 0 of 2^L entries, before the device check (the length is a power of two here)
int shape_check(int field, unsigned L, uint32_t b, uint32_t f) {
    if (L <= b || f >= L - b) return ZK_E_ARG;               // d = L - b >= 1 and f < d
    if (field != ZK_FR381 && field != ZK_BN254_FR) return ZK_E_RANGE;
    return L > two_adicity(field) ? ZK_E_RANGE : ZK_OK;
}

// grind_bits > 0: the proof-of-work step in front of the indices, its nonce into *nonce_out
int prove_any(const zk_table *in, bool is_codeword, uint32_t b, uint32_t f, uint32_t Q, const uint64_t *coset, zk_transcript *t, const ProofOut &o,
              uint32_t grind_bits = 0, uint64_t *nonce_out = nullptr) {
    if (!in || !o.roots || !o.final_coeffs || !o.query_values || !o.query_paths || field_limbs64(in->field) < 0) return ZK_E_ARG;
    if (grind_bits > ZK_FRI_GRIND_MAX_BITS || (grind_bits && !nonce_out)) return ZK_E_ARG;
    ZK_TRY(params_check(b, Q));
    if (coset && is_zero_element(in->field, coset)) return ZK_E_ARG;
    if (!is_pow2(in->len)) return ZK_E_NOT_POW2;
    ZK_TRY(shape_check(in->field, ilog2(in->len) + (is_codeword ? 0 : b), b, f));
    ZK_TRY(require_device());
    const auto t0 = std::chrono::steady_clock::now();
    Transcript fresh;
    Transcript &tr = t ? t->t : fresh;
    Events ev;
    size_t e0, e1;
    TableHolder ext;
    const zk_table *cw = in;
    ZK_TRY(ev.mark(&e0));
    if (!is_codeword) {
        zk_table *x = nullptr;
        ZK_TRY(ext.alloc(in->field, in->len << b, &x));
        ZK_TRY(ntt_extend_into(in, coset, x));
        cw = x;
    }
    ZK_TRY(ev.mark(&e1));
    zk_fri_stats st{};
    int rc = ZK_OK;
    FRI_DISPATCH(in->field, rc = prove_layers<F>(cw, b, f, Q, coset, tr, o, ev, &st.ms_trees, &st.ms_folds, &st.ms_queries, grind_bits, nonce_out));
    ZK_TRY(rc);
    st.layers = ilog2(cw->len) - b - f;
    st.queries = Q;
    st.ms_extend = is_codeword ? 0.f : ev.ms(e0, e1);
    st.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g_fri_stats = st;
    return ZK_OK;
}

// ---- the verifier (host) -------------------------------------------------------------------------------------------------------
// what the transcript gives back: `good` = every element absorbed so far was a reduced one
template <class F> struct Replayed {
    bool good;
    Fe<F> gamma = fe_one<F>();                                // the several-point form's batching challenge
    std::vector<Fe<F>> beta, h;                               // the R fold challenges; the final coefficients (or table)
    std::vector<uint64_t> idx;                                // the Q query indices
};

// the prover's transcript over again.  `ml`: the claim and round polynomials of the multilinear forms (context.h FriMlClaim), null = zk_fri_verify
template <class F> Replayed<F> replay(uint32_t d, uint32_t b, uint32_t f, uint32_t Q, const uint64_t *coset, Transcript &tr, const FriSchedule &sc,
                                      const uint8_t *roots, const uint64_t *final_coeffs, const FriMlClaim *ml, uint32_t grind_bits = 0,
                                      uint64_t pow_nonce = 0) {
    constexpr int W = F::N / 2;
    const unsigned R = d - f;
    Replayed<F> rp;
    rp.good = !coset || is_reduced<F>(coset);
    const auto absorb = [&](const uint64_t *el) {
        rp.good = rp.good && is_reduced<F>(el);
        const Fe<F> e = load_host<F>(el);
        tr.append_be<F>(e);
        return e;
    };
    uint8_t cbe[32], be[16] = {'B', 'T', 'C', 'H'};
    const unsigned nt = ml ? ml->ntables : 0;                 // commitments opened together: their roots lead `roots`
    const unsigned nc = ml ? ml->ncommit : 0;                 // column commitments: nc roots lead, over nt columns
    const unsigned lead = nc ? nc : nt;
    host_to_bytes_be<F>(coset ? load_host<F>(coset) : fe_one<F>(), cbe);
    transcript_header(tr, d, b, f, Q, cbe);
    if (nc) {                                                // "COLS", the arity, m, the m widths; the m roots
        std::vector<uint8_t> line(12 + 4 * (size_t)nc);
        memcpy(line.data(), "COLS", 4);
        put_be32(line.data() + 4, sc.log_arity);
        put_be32(line.data() + 8, nc);
        for (unsigned i = 0; i < nc; i++) put_be32(line.data() + 12 + 4 * i, ml->widths[i]);
        tr.append(line.data(), line.size());
        tr.append(roots, (size_t)32 * nc);
    } else if (nt) {                                         // the tag, the arity, the grouped flag, k; the k roots
        put_be32(be + 4, sc.log_arity);
        put_be32(be + 8, sc.grouped ? 1 : 0);
        put_be32(be + 12, nt);
        tr.append(be, 16);
        tr.append(roots, (size_t)32 * nt);
    } else {
        if (sc.log_arity == 2) {                             // the arity, and behind it a 1 when the leaves are grouped
            put_be32(be, sc.log_arity);
            put_be32(be + 4, 1);
            tr.append(be, sc.grouped ? 8 : 4);
        }
        tr.append(roots, 32);
    }
    if (ml && ml->weighted_c) {                              // "WGHT", then the claim c; the weight table is the caller's to bind
        tr.append((const uint8_t *)"WGHT", 4);
        absorb(ml->weighted_c);
    } else if (ml && ml->npoints == 0) {                     // z_0 .. z_{d-1}, then y
        for (unsigned i = 0; i < d; i++) absorb(ml->z + (size_t)i * W);
        absorb(ml->y);
    } else if (ml) {                                         // P, the points (point-major), the claims, then gamma
        const size_t P = ml->npoints;
        put_be32(be, ml->npoints);
        tr.append(be, 4);
        for (size_t i = 0; i < P * d; i++) absorb(ml->z + i * W);
        for (size_t p = 0; p < P * (nt ? nt : 1); p++) absorb(ml->y + p * W);   // several tables: table-major
        rp.gamma = tr.random_challenge_as_field_element<F>();
    }
    rp.beta.resize(R);
    for (unsigned l = 0, s = 0; l < R; l++) {
        for (unsigned k = 0; ml && k < 3; k++) absorb(ml->round_polys + ((size_t)l * 3 + k) * W);   // g_l(0), g_l(1), g_l(2)
        rp.beta[l] = tr.random_challenge_as_field_element<F>();
        if (s + 1 < sc.nsteps && sc.step[s + 1].layer == l + 1) tr.append(roots + 32 * (size_t)(sc.step[++s].root + (lead ? lead - 1 : 0)), 32);   // layer l + 1 is committed
    }
    for (size_t j = 0; j < (size_t)1 << f; j++) rp.h.push_back(absorb(final_coeffs + j * W));
    if (grind_bits) {                                        // the proof-of-work step: the tag, the nonce, the challenge and its leading bits
        const bool pow_ok = grind_check(tr, grind_bits, pow_nonce);
        rp.good = rp.good && pow_ok;
    }
    for (unsigned q = 0; q < Q; q++) rp.idx.push_back(sample_index(tr, sc.index_bits()));
    return rp;
}

// the sumcheck of sum_x T[x] W[x] = sum_p gamma^p y_p beside the folds, on the same challenges; the single-point form is one point with gamma^0.
// k tables together: T = sum_j alpha^j T_j, alpha = gamma^P, so only the first claim differs: sum_j sum_p gamma^(j P + p) y_{j,p}
// g(r) from g's values at 0, 1, 2:  g0 (r - 1)(r - 2) / 2 - g1 r (r - 2) + g2 r (r - 1) / 2
template <class F> Fe<F> g3_at(const Fe<F> &g0, const Fe<F> &g1, const Fe<F> &g2, const Fe<F> &r) {
    const Fe<F> one = fe_one<F>(), two = fe_from_u64<F>(2), r1 = fe_sub<F>(r, one), r2 = fe_sub<F>(r, two);
    const Fe<F> outer = fe_mul<F>(fe_inv<F>(two), fe_add<F>(fe_mul<F>(g0, fe_mul<F>(r1, r2)), fe_mul<F>(g2, fe_mul<F>(r, r1))));
    return fe_sub<F>(outer, fe_mul<F>(g1, fe_mul<F>(r, r2)));
}

// the same sumcheck against a caller's weight table (ml.weighted_c): the first claim is c, every r_l must be the challenge the proof carries --
// the caller folded its table by those -- and the end is sum_j T_R[j] w_final[j]
template <class F> bool weighted_sumcheck_holds(uint32_t d, uint32_t f, const FriMlClaim &ml, const Replayed<F> &rp) {
    constexpr int W = F::N / 2;
    const unsigned R = d - f;
    const size_t m = (size_t)1 << f;
    for (size_t i = 0; i < R + m; i++)                        // the carried challenges, then w_final: reduced
        if (!is_reduced<F>(i < R ? ml.challenges + i * W : ml.w_final + (i - R) * W)) return false;
    Fe<F> claim = load_host<F>(ml.weighted_c);
    for (unsigned l = 0; l < R; l++) {
        const uint64_t *g = ml.round_polys + (size_t)l * 3 * W;
        const Fe<F> g0 = load_host<F>(g), g1 = load_host<F>(g + W), g2 = load_host<F>(g + 2 * W);
        if (!fe_eq<F>(rp.beta[l], load_host<F>(ml.challenges + (size_t)l * W)) || !fe_eq<F>(fe_add<F>(g0, g1), claim)) return false;
        claim = g3_at<F>(g0, g1, g2, rp.beta[l]);
    }
    Fe<F> end = fe_zero<F>();
    for (size_t j = 0; j < m; j++) end = fe_add<F>(end, fe_mul<F>(rp.h[j], load_host<F>(ml.w_final + j * W)));
    return fe_eq<F>(end, claim);
}

template <class F> bool sumcheck_holds(uint32_t d, uint32_t f, const FriMlClaim &ml, const Replayed<F> &rp) {
    constexpr int W = F::N / 2;
    if (ml.weighted_c) return weighted_sumcheck_holds<F>(d, f, ml, rp);
    const unsigned R = d - f, np = ml.npoints ? ml.npoints : 1;
    const size_t m = (size_t)1 << f;
    const Fe<F> one = fe_one<F>(), two = fe_from_u64<F>(2);
    std::vector<Fe<F>> A(np, one);                            // per point p: gamma^p A^p_l
    Fe<F> claim = fe_zero<F>();
    for (unsigned p = 1; p < np; p++) A[p] = fe_mul<F>(A[p - 1], rp.gamma);
    Fe<F> gp = one;                                           // gamma^(j P + p)
    for (size_t t = 0; t < (size_t)np * (ml.ntables ? ml.ntables : 1); t++) {
        claim = fe_add<F>(claim, fe_mul<F>(gp, load_host<F>(ml.y + t * W)));
        gp = fe_mul<F>(gp, rp.gamma);
    }
    for (unsigned l = 0; l < R; l++) {
        const uint64_t *g = ml.round_polys + (size_t)l * 3 * W;
        const Fe<F> g0 = load_host<F>(g), g1 = load_host<F>(g + W), g2 = load_host<F>(g + 2 * W), r = rp.beta[l];
        if (!fe_eq<F>(fe_add<F>(g0, g1), claim)) return false;
        claim = g3_at<F>(g0, g1, g2, r);
        for (unsigned p = 0; p < np; p++) {
            const Fe<F> zv = load_host<F>(ml.z + ((size_t)p * d + d - 1 - l) * W);   // eq1(r_l, z_v) = 1 - r - z + 2 r z
            A[p] = fe_mul<F>(A[p], fe_add<F>(fe_sub<F>(fe_sub<F>(one, r), zv), fe_mul<F>(two, fe_mul<F>(r, zv))));
        }
    }
    // sum_j T_R[j] W_R[j] = sum_p gamma^p A^p_R (the MLE of T_R at (z^p_0 .. z^p_{f-1})): f folds of variable 0 per point
    Fe<F> end = fe_zero<F>();
    for (unsigned p = 0; p < np; p++) {
        std::vector<Fe<F>> t(rp.h);
        for (unsigned i = 0; i < f; i++) {
            const size_t half = m >> (i + 1);
            const Fe<F> zi = load_host<F>(ml.z + ((size_t)p * d + i) * W);
            for (size_t j = 0; j < half; j++) t[j] = fe_add<F>(t[j], fe_mul<F>(zi, fe_sub<F>(t[j + half], t[j])));
        }
        end = fe_add<F>(end, fe_mul<F>(A[p], t[0]));
    }
    return fe_eq<F>(end, claim);
}

// every query: its steps' paths (grouped: each step's one path from the leaf over its sides), and each step's fold against the next step's value (the last against the final polynomial).  `lagrange`: the
// fold of the multilinear forms, (1 - r) (a + b) / 2 + r (a - b) / (2 x); else the monomial (a + b) / 2 + r (a - b) / (2 x)
// `nt` > 0 (commitments opened together): step 0 of a query holds the nt commitments' values and paths one commitment after the other, each
// checked against its own root (roots[j]); the step's values are u_side = sum_j alpha^j v_{j,side}; the later steps' roots follow the nt
// `widths` (nc of them, together nt; column commitments opened together): step 0 holds the nt columns' values but ONE path per commitment, whose
// leaf is hashed from that commitment's columns' values (zk_merkle_verify_columns), and nc roots lead
template <class F> int queries_hold(const FriSchedule &sc, unsigned R, bool lagrange, const Fe<F> &c, const Replayed<F> &rp, const uint8_t *roots,
                                    const uint64_t *values, const uint8_t *paths, int *ok, unsigned nt = 0, const Fe<F> &alpha = fe_one<F>(),
                                    const uint32_t *widths = nullptr, unsigned nc = 0) {
    constexpr int W = F::N / 2;
    const unsigned L = sc.step[0].log_len;
    const Fe<F> w = root_of_unity<F>(L), winv = fe_inv<F>(w), inv2 = fe_inv<F>(fe_from_u64<F>(2));
    const Fe<F> iinv = fe_pow<F>(winv, (uint64_t)1 << (L - 2));   // i^-1, i = w_l^(N_l / 4) = the primitive fourth root w^(N / 4) at every layer
    std::vector<Fe<F>> cinv(R);                               // c_l^-1
    Fe<F> cR = c, ci = fe_inv<F>(c);
    for (unsigned l = 0; l < R; l++) {
        cinv[l] = ci;
        ci = fe_sqr<F>(ci);
        cR = fe_sqr<F>(cR);
    }
    const auto fold = [&](const Fe<F> &a, const Fe<F> &bb, const Fe<F> &r, const Fe<F> &xinv) {
        Fe<F> even = fe_add<F>(a, bb);
        if (lagrange) even = fe_mul<F>(fe_sub<F>(fe_one<F>(), r), even);
        return fe_mul<F>(inv2, fe_add<F>(even, fe_mul<F>(fe_mul<F>(r, xinv), fe_sub<F>(a, bb))));
    };
    // step 0's share of one query's answer, and what the further commitments add in front of the later steps
    const size_t v0 = sc.nsteps > 1 ? sc.step[1].val_off : sc.nvalues, d0 = sc.nsteps > 1 ? sc.step[1].path_off : sc.ndigests;
    const size_t more = nt ? nt - 1 : 0, more_r = nc ? nc - 1 : more, more_v = more * v0, more_d = more_r * d0;
    for (size_t q = 0; q < rp.idx.size(); q++) {
        const uint64_t *vq = values + q * (sc.nvalues + more_v) * W;
        const uint8_t *pq = paths + q * (sc.ndigests + more_d) * 32;
        for (unsigned s = 0; s < sc.nsteps; s++) {
            const FriStep &st = sc.step[s];
            const unsigned l = st.layer, sides = 1u << st.log_sides;
            const size_t part = ((size_t)1 << st.log_len) >> st.log_sides, j = rp.idx[q] & (part - 1);
            Fe<F> e[4] = {fe_zero<F>(), fe_zero<F>(), fe_zero<F>(), fe_zero<F>()}, aj = fe_one<F>();
            if (nc && s == 0) {                               // each commitment's leaf over its columns' values, and its one path
                size_t col = 0;
                for (unsigned i = 0; i < nc; col += widths[i], i++) {
                    int ok_s = 0;
                    ZK_TRY(zk_merkle_verify_columns(F::ID, roots + 32 * (size_t)i, st.log_len - st.log_sides, j, widths[i], vq + col * v0 * W, pq + 32 * i * d0, &ok_s));
                    if (!ok_s) return ZK_OK;
                }
            }
            for (size_t tb = 0; tb < (s == 0 ? more + 1 : 1); tb++) {   // the commitments of step 0; one table otherwise
                const uint64_t *v = vq + (st.val_off + (s ? more_v : tb * v0)) * W;
                const uint8_t *pt = pq + 32 * (st.path_off + (s ? more_d : tb * d0)), *root = roots + 32 * (s ? st.root + more_r : tb);
                if (sc.grouped && !(nc && s == 0)) {                             // one leaf over the step's sides, one path
                    int ok_s = 0;
                    ZK_TRY(zk_merkle_verify_grouped(F::ID, root, st.log_len - st.log_sides, j, st.log_sides, v, pt, &ok_s));
                    if (!ok_s) return ZK_OK;
                }
                for (unsigned side = 0; side < sides; side++) {
                    int ok_s = sc.grouped;
                    if (!sc.grouped) ZK_TRY(zk_merkle_verify(F::ID, root, st.log_len, j + side * part, v + (size_t)side * W, pt + 32 * (size_t)side * st.log_len, &ok_s));
                    if (!ok_s) return ZK_OK;
                    const Fe<F> x = load_host<F>(v + (size_t)side * W);
                    e[side] = nt ? fe_add<F>(e[side], fe_mul<F>(aj, x)) : x;
                }
                if (nt) aj = fe_mul<F>(aj, alpha);
            }
            const Fe<F> xinv = fe_mul<F>(cinv[l], fe_pow<F>(winv, (uint64_t)j << l));
            Fe<F> got;
            if (sides == 4) got = fold(fold(e[0], e[2], rp.beta[l], xinv), fold(e[1], e[3], rp.beta[l], fe_mul<F>(xinv, iinv)), rp.beta[l + 1], fe_sqr<F>(xinv));
            else got = fold(e[0], e[1], rp.beta[l], xinv);
            Fe<F> want;                                       // the step lands in layer l + log_sides: j is a position of it
            if (s + 1 < sc.nsteps) {
                const FriStep &nx = sc.step[s + 1];
                want = load_host<F>(vq + (nx.val_off + more_v + j / (((size_t)1 << nx.log_len) >> nx.log_sides)) * W);
            } else want = uni_evaluate<F>(rp.h, fe_mul<F>(cR, fe_pow<F>(w, (uint64_t)j << R)));
            if (!fe_eq<F>(got, want)) return ZK_OK;
        }
    }
    *ok = 1;
    return ZK_OK;
}

// `indices_out` (Q words, may be null): the sampled i_q, for a caller that checks more at the queried positions (zkmle_fri_pcs.hip)
template <class F> int verify_host(uint32_t d, uint32_t b, uint32_t f, uint32_t Q, const uint64_t *coset, Transcript &tr, const uint8_t *roots,
                                   const uint64_t *final_coeffs, const uint64_t *values, const uint8_t *paths, int *ok, uint64_t *indices_out,
                                   const FriMlClaim *ml, uint32_t grind_bits, uint64_t pow_nonce) {
    const FriSchedule sc(d + b, d - f, ml ? ml->log_arity : 1, ml && ml->grouped);
    Replayed<F> rp = replay<F>(d, b, f, Q, coset, tr, sc, roots, final_coeffs, ml, grind_bits, pow_nonce);
    if (indices_out) memcpy(indices_out, rp.idx.data(), Q * 8);
    *ok = 0;
    const unsigned nt = ml ? ml->ntables : 0;
    const size_t per = sc.nvalues + (nt ? nt - 1 : 0) * (sc.nsteps > 1 ? sc.step[1].val_off : sc.nvalues);   // values of one query's answer
    for (size_t k = 0; rp.good && k < (size_t)Q * per; k++) rp.good = is_reduced<F>(values + k * (F::N / 2));
    if (!rp.good || (ml && !sumcheck_holds<F>(d, f, *ml, rp))) return ZK_OK;
    Fe<F> alpha = fe_one<F>();                                // gamma^P
    for (unsigned p = 0; nt && p < ml->npoints; p++) alpha = fe_mul<F>(alpha, rp.gamma);
    return queries_hold<F>(sc, d - f, ml != nullptr, coset ? load_host<F>(coset) : fe_one<F>(), rp, roots, values, paths, ok, nt, alpha, ml ? ml->widths : nullptr,
                           ml ? ml->ncommit : 0);
}

}  // namespace

namespace zk {
int fri_verify_core(int field, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset, Transcript &tr,
                    const uint8_t *roots, const uint64_t *final_coeffs, const uint64_t *query_values, const uint8_t *query_paths, int *ok,
                    uint64_t *indices_out, const FriMlClaim *ml, uint32_t grind_bits, uint64_t pow_nonce, uint32_t max_tables) {
    if (grind_bits > ZK_FRI_GRIND_MAX_BITS) return ZK_E_ARG;
    const bool weighted = ml && ml->weighted_c;               // a weight table stands where the points do
    if (weighted && (!ml->challenges || !ml->w_final || !ml->round_polys || ml->npoints || ml->ntables)) return ZK_E_ARG;
    if (ml && !weighted && (!ml->z || !ml->y || !ml->round_polys || ml->npoints > 8)) return ZK_E_ARG;
    if (ml && (ml->log_arity < 1 || ml->log_arity > 2 || (ml->log_arity == 2 && ((ml->npoints < 1 && !weighted) || log_final >= d || d - log_final < 2)))) return ZK_E_ARG;
    if (ml && ml->grouped && ml->log_arity != 2) return ZK_E_ARG;
    if (ml && (ml->ntables > max_tables || (ml->ntables && ml->npoints < 1))) return ZK_E_ARG;
    if (ml && ml->ncommit) {                                 // column commitments: grouped leaves, and the widths make up the tables
        if (!ml->widths || !ml->grouped || ml->ncommit > ml->ntables) return ZK_E_ARG;
        size_t total = 0;
        for (uint32_t i = 0; i < ml->ncommit; i++) {
            if (ml->widths[i] < 1 || ml->widths[i] > ZK_FRI_COLUMNS_MAX) return ZK_E_ARG;
            total += ml->widths[i];
        }
        if (total != ml->ntables) return ZK_E_ARG;
    }
    if (!roots || !final_coeffs || !query_values || !query_paths || !ok || field_limbs64(field) < 0) return ZK_E_ARG;
    ZK_TRY(params_check(log_blowup, nqueries));
    if (coset && is_zero_element(field, coset)) return ZK_E_ARG;
    if (d < 1 || log_final >= d) return ZK_E_ARG;
    if (d > 32) return ZK_E_RANGE;
    ZK_TRY(shape_check(field, d + log_blowup, log_blowup, log_final));
    FRI_DISPATCH(field, return verify_host<F>(d, log_blowup, log_final, nqueries, coset, tr, roots, final_coeffs, query_values, query_paths, ok, indices_out, ml, grind_bits, pow_nonce));
    return ZK_OK;
}
}  // namespace zk

extern "C" {

int zk_fri_fold(const zk_table *codeword, const uint64_t *beta, const uint64_t *coset, zk_table **out) {
    ZK_TRY(fold_check(codeword, beta && out, coset, 1));
    FRI_DISPATCH(codeword->field, return fold_once<F>(codeword, beta, coset, out));
    return ZK_OK;
}

int zk_fri_proof_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, size_t *nroots, size_t *nfinal, size_t *nvalues,
                       size_t *path_bytes) {
    ZK_TRY(params_check(log_blowup, nqueries));
    if (d < 1 || log_final >= d) return ZK_E_ARG;
    if (d > 32 || d + log_blowup > 32) return ZK_E_RANGE;
    const FriSchedule sc(d + log_blowup, d - log_final, 1);
    if (nroots) *nroots = sc.nsteps;
    if (nfinal) *nfinal = (size_t)1 << log_final;
    if (nvalues) *nvalues = (size_t)nqueries * sc.nvalues;
    if (path_bytes) *path_bytes = (size_t)nqueries * sc.ndigests * 32;
    return ZK_OK;
}

int zk_fri_prove(const zk_table *coeffs, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset, zk_transcript *t,
                 uint8_t *roots, uint64_t *final_coeffs, uint64_t *betas, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths) {
    return prove_any(coeffs, false, log_blowup, log_final, nqueries, coset, t, ProofOut{roots, final_coeffs, betas, query_indices, query_values, query_paths});
}
int zk_fri_prove_codeword(const zk_table *codeword, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset, zk_transcript *t,
                          uint8_t *roots, uint64_t *final_coeffs, uint64_t *betas, uint64_t *query_indices, uint64_t *query_values,
                          uint8_t *query_paths) {
    return prove_any(codeword, true, log_blowup, log_final, nqueries, coset, t, ProofOut{roots, final_coeffs, betas, query_indices, query_values, query_paths});
}

int zk_fri_verify(int field, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset, zk_transcript *t,
                  const uint8_t *roots, const uint64_t *final_coeffs, const uint64_t *query_values, const uint8_t *query_paths, int *ok) {
    Transcript fresh;
    return fri_verify_core(field, d, log_blowup, log_final, nqueries, coset, t ? t->t : fresh, roots, final_coeffs, query_values, query_paths, ok, nullptr);
}

int zk_fri_prove_pow(const zk_table *coeffs, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset, zk_transcript *t,
                     uint8_t *roots, uint64_t *final_coeffs, uint64_t *betas, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths,
                     uint32_t grinding_bits, uint64_t *pow_nonce) {
    return prove_any(coeffs, false, log_blowup, log_final, nqueries, coset, t, ProofOut{roots, final_coeffs, betas, query_indices, query_values, query_paths},
                     grinding_bits, pow_nonce);
}

int zk_fri_verify_pow(int field, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset, zk_transcript *t,
                      const uint8_t *roots, const uint64_t *final_coeffs, const uint64_t *query_values, const uint8_t *query_paths,
                      uint32_t grinding_bits, uint64_t pow_nonce, int *ok) {
    Transcript fresh;
    return fri_verify_core(field, d, log_blowup, log_final, nqueries, coset, t ? t->t : fresh, roots, final_coeffs, query_values, query_paths, ok, nullptr,
                           nullptr, grinding_bits, pow_nonce);
}

int zk_fri_last_stats(zk_fri_stats *out) {
    if (!out) return ZK_E_ARG;
    *out = g_fri_stats;
    return ZK_OK;
}

}  // extern "C"
