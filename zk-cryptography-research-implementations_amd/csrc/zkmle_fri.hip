// zkmle_fri.hip -- C ABI of the FRI low-degree proof (fri.cuh): one fold, the prover from a coefficient table or from a codeword, the
// host verifier.  Extension: the reference leaves `fri/` empty; layers, transcript and layouts are defined in include/zkmle.h.
#include <string.h>

#include <chrono>
#include <vector>

#include "context.h"
#include "fri.cuh"
#include "transcript.h"
#include "univariate.h"

using namespace zk;

namespace {

struct DevBuf {   // RAII block of the caching pool
    void *p = nullptr;
    ~DevBuf() { pool_free(p); }
    int alloc(size_t bytes) { return pool_alloc(bytes, &p); }
};
struct TableHolder {   // tables of the pool, freed with the proof
    std::vector<zk_table *> v;
    ~TableHolder() { for (zk_table *t : v) zk_table_free(t); }
};
// HIP events along the calling thread's stream; elapsed times are read after the proof's last synchronisation
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

thread_local zk_fri_stats g_fri_stats{};

// the two scalar fields: the only ones with a domain (every shape of the Fq fields is out of range)
#define FRI_DISPATCH(field_id, ...)                                        \
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
template <class F> Fe<F> fe_pow(Fe<F> b, uint64_t e) {
    Fe<F> acc = fe_one<F>();
    for (; e; e >>= 1) {
        if (e & 1) acc = fe_mul<F>(acc, b);
        b = fe_sqr<F>(b);
    }
    return acc;
}
template <class F> bool is_reduced(const uint64_t *el) {
    const Fe<F> x = load_host<F>(el);
    for (int i = F::N - 1; i >= 0; i--)
        if (x.l[i] != F::p(i)) return x.l[i] < F::p(i);
    return false;
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
// w_{2^log_n}; log_n within the field's two-adicity
template <class F> Fe<F> root_of_unity(unsigned log_n) {
    uint64_t w[F::N / 2];
    (void)zk_ntt_root_of_unity(F::ID, log_n, w);
    return load_host<F>(w);
}
void put_be32(uint8_t *out, uint32_t v) {
    for (int k = 0; k < 4; k++) out[k] = (uint8_t)(v >> (24 - 8 * k));
}
// the checks on (b, f, Q) that need no length, then those that need d = the coefficient table's log2 length
int params_check(uint32_t b, uint32_t Q) { return b >= 1 && b <= 8 && Q >= 1 && Q <= 4096 ? ZK_OK : ZK_E_ARG; }
size_t path_digests(unsigned L, unsigned R) {             // of one query's answer
    size_t n = 0;
    for (unsigned l = 0; l < R; l++) n += 2 * (size_t)(L - l);
    return n;
}

// ---- the fold ------------------------------------------------------------------------------------------------------------------
// the powers of w_N^-1 below N / 2, N = 2^log_n, as ntt_pow2t reads them: built once per proof, layer l indexes them with k << l
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
// out[k], k < len / 2, from in[0 .. len): gamma = beta / (2 c) of this layer, `shift` = the layer's number
template <class F> int launch_fold(const void *in, void *out, size_t len, unsigned shift, const FoldTables<F> &tb, const Fe<F> &gamma) {
    UniMul<F> um;
    unimul_from<F>(um, gamma);
    FriUni g;
    memcpy(g.t, um.t, sizeof g.t);
    const size_t half = len / 2;
    fri_fold_kernel<F><<<(unsigned)((half + kFriBlock - 1) / kFriBlock), kFriBlock, 0, cur_stream()>>>(in, out, half, tb.lo, tb.hi, shift, g);
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

void transcript_header(Transcript &tr, uint32_t d, uint32_t b, uint32_t f, uint32_t Q, const uint8_t coset_be[32]) {
    uint8_t hdr[48];
    put_be32(hdr, d);
    put_be32(hdr + 4, b);
    put_be32(hdr + 8, f);
    put_be32(hdr + 12, Q);
    memcpy(hdr + 16, coset_be, 32);
    tr.append(hdr, sizeof hdr);
}
// i_q = the little-endian integer of a sampled digest mod 2^bits, bits <= 31
uint64_t sample_index(Transcript &tr, unsigned bits) {
    uint8_t dg[32];
    tr.sample_random_challenge(dg);
    uint64_t v = 0;
    for (int k = 0; k < 8; k++) v |= (uint64_t)dg[k] << (8 * k);
    return v & (((uint64_t)1 << bits) - 1);
}

// `cw` = layer 0 (N = 2^L entries, L = d + b); events: `ev0` was recorded before the extension (or is the proof's first event)
template <class F> int prove_layers(const zk_table *cw, unsigned b, unsigned f, unsigned Q, const uint64_t *coset, Transcript &tr, const ProofOut &o,
                                    Events &ev, float *ms_trees, float *ms_folds, float *ms_queries) {
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
    FriLayers fl{};
    fl.log_len0 = L;
    fl.nlayers = R;

    std::vector<size_t> ta(R + 1), tf(R);
    const zk_table *cur = cw;
    Fe<F> gscale = fe_inv<F>(fe_mul<F>(fe_from_u64<F>(2), c)), cinv_sq = fe_inv<F>(c);   // 1 / (2 c_l), and c_l^-1 to step it: 1 / (2 c_{l+1}) = (1 / (2 c_l)) c_l^-1
    for (unsigned l = 0; l < R; l++) {
        uint64_t *tree = (uint64_t *)trees.p + 4 * (4 * N - ((4 * N) >> l));
        fl.table[l] = cur->dptr;
        fl.tree[l] = tree;
        fl.path_off[l + 1] = fl.path_off[l] + 2 * (L - l);
        ZK_TRY(ev.mark(&ta[l]));
        ZK_TRY(merkle_levels_device(cur, tree));
        uint8_t *root = o.roots + 32 * l;
        ZK_HIP(zk::memcpy_on_stream(root, tree + 4 * (2 * cur->len - 2), 32, hipMemcpyDeviceToHost));   // the layer's synchronisation
        tr.append(root, 32);
        const Fe<F> beta = tr.random_challenge_as_field_element<F>();
        if (o.betas) memcpy(o.betas + l * (F::N / 2), beta.l, ESZ);
        zk_table *next = nullptr;
        ZK_TRY(table_alloc_pooled(cw->field, cur->len / 2, &next));
        layers.v.push_back(next);
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

    std::vector<uint64_t> idx(Q);
    for (unsigned q = 0; q < Q; q++) idx[q] = sample_index(tr, L - 1);
    if (o.query_indices) memcpy(o.query_indices, idx.data(), Q * 8);
    const size_t nval = (size_t)Q * R * 2, ndig = (size_t)Q * fl.path_off[R];
    DevBuf didx, dval, dpath;
    ZK_TRY(didx.alloc(Q * 8));
    ZK_TRY(dval.alloc(nval * ESZ));
    ZK_TRY(dpath.alloc(ndig * 32));
    ZK_HIP(hipMemcpyAsync(didx.p, idx.data(), Q * 8, hipMemcpyHostToDevice, cur_stream()));
    fri_query_values_kernel<F><<<(unsigned)((nval + kFriBlock - 1) / kFriBlock), kFriBlock, 0, cur_stream()>>>(fl, (const uint64_t *)didx.p, Q, dval.p);
    ZK_HIP(hipGetLastError());
    fri_query_paths_kernel<<<(unsigned)((ndig + kFriBlock - 1) / kFriBlock), kFriBlock, 0, cur_stream()>>>(fl, (const uint64_t *)didx.p, Q, (uint64_t *)dpath.p);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(o.query_values, dval.p, nval * ESZ, hipMemcpyDeviceToHost, cur_stream()));   // one download each, one wait for both
    ZK_HIP(zk::memcpy_on_stream(o.query_paths, dpath.p, ndig * 32, hipMemcpyDeviceToHost));
    size_t end;
    ZK_TRY(ev.mark(&end));
    ZK_HIP(hipEventSynchronize(ev.ev[end]));
    *ms_trees = *ms_folds = 0.f;
    for (unsigned l = 0; l < R; l++) {
        *ms_trees += ev.ms(ta[l], tf[l]);
        *ms_folds += ev.ms(tf[l], ta[l + 1]);
    }
    *ms_queries = ev.ms(ta[R], end);
    return ZK_OK;
}

// the statuses of a proof over a layer 0 of 2^L entries, before the device check (the length is a power of two here)
int shape_check(int field, unsigned L, uint32_t b, uint32_t f) {
    if (L <= b || f >= L - b) return ZK_E_ARG;               // d = L - b >= 1 and f < d
    if (field != ZK_FR381 && field != ZK_BN254_FR) return ZK_E_RANGE;
    return L > two_adicity(field) ? ZK_E_RANGE : ZK_OK;
}

int prove_any(const zk_table *in, bool is_codeword, uint32_t b, uint32_t f, uint32_t Q, const uint64_t *coset, zk_transcript *t, const ProofOut &o) {
    if (!in || !o.roots || !o.final_coeffs || !o.query_values || !o.query_paths || field_limbs64(in->field) < 0) return ZK_E_ARG;
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
        ZK_TRY(table_alloc_pooled(in->field, in->len << b, &x));
        ext.v.push_back(x);
        ZK_TRY(ntt_extend_into(in, coset, x));
        cw = x;
    }
    ZK_TRY(ev.mark(&e1));
    zk_fri_stats st{};
    int rc = ZK_OK;
    FRI_DISPATCH(in->field, rc = prove_layers<F>(cw, b, f, Q, coset, tr, o, ev, &st.ms_trees, &st.ms_folds, &st.ms_queries));
    ZK_TRY(rc);
    st.layers = ilog2(cw->len) - b - f;
    st.queries = Q;
    st.ms_extend = is_codeword ? 0.f : ev.ms(e0, e1);
    st.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g_fri_stats = st;
    return ZK_OK;
}

// ---- the verifier (host) -------------------------------------------------------------------------------------------------------
// `indices_out` (Q words, may be null): the sampled i_q, for a caller that checks more at the queried positions (zkmle_fri_pcs.hip)
// `ml`: the fold mode of the multilinear opening (context.h FriMlClaim); null = the monomial fold of zk_fri_verify, byte for byte as before
template <class F> int verify_host(uint32_t d, uint32_t b, uint32_t f, uint32_t Q, const uint64_t *coset, Transcript &tr, const uint8_t *roots,
                                   const uint64_t *final_coeffs, const uint64_t *values, const uint8_t *paths, int *ok, uint64_t *indices_out,
                                   const FriMlClaim *ml) {
    constexpr int W = F::N / 2;
    const unsigned L = d + b, R = d - f;
    const size_t m = (size_t)1 << f;
    const Fe<F> c = coset ? load_host<F>(coset) : fe_one<F>();
    bool good = !coset || is_reduced<F>(coset);
    uint8_t cbe[32];
    host_to_bytes_be<F>(c, cbe);
    transcript_header(tr, d, b, f, Q, cbe);
    const unsigned la = ml ? ml->log_arity : 1;              // 2: every second layer is committed and a query opens four entries of it
    if (la == 2) {
        uint8_t abe[4];
        put_be32(abe, la);
        tr.append(abe, 4);
    }
    tr.append(roots, 32);
    const unsigned P = ml ? ml->npoints : 0;                 // 0: the single-point form
    Fe<F> gamma = fe_one<F>();
    if (ml && P == 0) {
        for (unsigned i = 0; i <= d; i++) {                  // z_0 .. z_{d-1}, then y
            const uint64_t *el = i < d ? ml->z + (size_t)i * W : ml->y;
            good = good && is_reduced<F>(el);
            tr.append_be<F>(load_host<F>(el));
        }
    } else if (ml) {                                         // P, the points (point-major), the claims, then gamma
        uint8_t pbe[4];
        for (int k = 0; k < 4; k++) pbe[k] = (uint8_t)(P >> (24 - 8 * k));
        tr.append(pbe, 4);
        for (size_t i = 0; i < (size_t)P * d + P; i++) {
            const uint64_t *el = i < (size_t)P * d ? ml->z + i * W : ml->y + (i - (size_t)P * d) * W;
            good = good && is_reduced<F>(el);
            tr.append_be<F>(load_host<F>(el));
        }
        gamma = tr.random_challenge_as_field_element<F>();
    }
    std::vector<Fe<F>> beta(R);
    for (unsigned l = 0; l < R; l++) {
        for (unsigned k = 0; ml && k < 3; k++) {             // g_l(0), g_l(1), g_l(2)
            const uint64_t *el = ml->round_polys + ((size_t)l * 3 + k) * W;
            good = good && is_reduced<F>(el);
            tr.append_be<F>(load_host<F>(el));
        }
        beta[l] = tr.random_challenge_as_field_element<F>();
        if (la == 2) {
            if (l + 1 < R && (l + 1) % 2 == 0) tr.append(roots + 32 * ((l + 1) / 2), 32);
        } else if (l + 1 < R) tr.append(roots + 32 * (l + 1), 32);
    }
    std::vector<Fe<F>> h(m);
    for (size_t j = 0; j < m; j++) {
        good = good && is_reduced<F>(final_coeffs + j * W);
        h[j] = load_host<F>(final_coeffs + j * W);
        tr.append_be<F>(h[j]);
    }
    std::vector<uint64_t> idx(Q);
    for (unsigned q = 0; q < Q; q++) idx[q] = sample_index(tr, L - la);
    if (indices_out) memcpy(indices_out, idx.data(), Q * 8);
    *ok = 0;
    const size_t vper = la == 2 ? 4 * (size_t)(R / 2) + 2 * (R % 2) : (size_t)R * 2;   // opened values of one query
    for (size_t k = 0; good && k < (size_t)Q * vper; k++) good = is_reduced<F>(values + k * W);
    if (!good) return ZK_OK;

    const Fe<F> w = root_of_unity<F>(L), winv = fe_inv<F>(w), inv2 = fe_inv<F>(fe_from_u64<F>(2));
    if (ml) {                                                // the sumcheck of sum_x T[x] eq(x, z) = y beside the folds, on the same challenges
        const Fe<F> one = fe_one<F>(), two = fe_from_u64<F>(2);
        const unsigned np = P ? P : 1;                        // per point p: gamma^p A^p_l; the single-point form is np = 1 with gamma^0
        std::vector<Fe<F>> A(np, one);
        Fe<F> claim = fe_zero<F>();
        for (unsigned p = 0; p < np; p++) {
            if (p) A[p] = fe_mul<F>(A[p - 1], gamma);
            claim = fe_add<F>(claim, fe_mul<F>(A[p], load_host<F>(ml->y + (size_t)p * W)));
        }
        for (unsigned l = 0; l < R; l++) {
            const uint64_t *g = ml->round_polys + (size_t)l * 3 * W;
            const Fe<F> g0 = load_host<F>(g), g1 = load_host<F>(g + W), g2 = load_host<F>(g + 2 * W), r = beta[l];
            if (!fe_eq<F>(fe_add<F>(g0, g1), claim)) return ZK_OK;
            // g_l(r) from its values at 0, 1, 2:  g0 (r - 1)(r - 2) / 2 - g1 r (r - 2) + g2 r (r - 1) / 2
            const Fe<F> r1 = fe_sub<F>(r, one), r2 = fe_sub<F>(r, two);
            const Fe<F> outer = fe_mul<F>(inv2, fe_add<F>(fe_mul<F>(g0, fe_mul<F>(r1, r2)), fe_mul<F>(g2, fe_mul<F>(r, r1))));
            claim = fe_sub<F>(outer, fe_mul<F>(g1, fe_mul<F>(r, r2)));
            for (unsigned p = 0; p < np; p++) {
                const Fe<F> zv = load_host<F>(ml->z + ((size_t)p * d + d - 1 - l) * W);   // eq1(r_l, z_v) = 1 - r - z + 2 r z
                A[p] = fe_mul<F>(A[p], fe_add<F>(fe_sub<F>(fe_sub<F>(one, r), zv), fe_mul<F>(two, fe_mul<F>(r, zv))));
            }
        }
        // sum_j T_R[j] W_R[j] = sum_p gamma^p A^p_R (the MLE of T_R at (z^p_0 .. z^p_{f-1})): f folds of variable 0 per point
        Fe<F> end = fe_zero<F>();
        for (unsigned p = 0; p < np; p++) {
            std::vector<Fe<F>> t(h);
            for (unsigned i = 0; i < f; i++) {
                const size_t half = m >> (i + 1);
                const Fe<F> zi = load_host<F>(ml->z + ((size_t)p * d + i) * W);
                for (size_t j = 0; j < half; j++) t[j] = fe_add<F>(t[j], fe_mul<F>(zi, fe_sub<F>(t[j + half], t[j])));
            }
            end = fe_add<F>(end, fe_mul<F>(A[p], t[0]));
        }
        if (!fe_eq<F>(end, claim)) return ZK_OK;
    }
    std::vector<Fe<F>> cinv(R);                               // c_l^-1
    Fe<F> cl = c, ci = fe_inv<F>(c);
    for (unsigned l = 0; l < R; l++) {
        cinv[l] = ci;
        ci = fe_sqr<F>(ci);
        cl = fe_sqr<F>(cl);
    }
    const Fe<F> cR = cl;
    if (la == 2) {
        // steps start at the even layers: a fold by 4 to layer l + 2 <= R, or (R odd, l = R - 1) the fold by 2 to layer R
        const auto fold = [&](const Fe<F> &a, const Fe<F> &bb, const Fe<F> &r, const Fe<F> &xinv) {   // (1 - r) (a + b) / 2 + r (a - b) / (2 x)
            const Fe<F> even = fe_mul<F>(fe_sub<F>(fe_one<F>(), r), fe_add<F>(a, bb));
            return fe_mul<F>(inv2, fe_add<F>(even, fe_mul<F>(fe_mul<F>(r, xinv), fe_sub<F>(a, bb))));
        };
        const Fe<F> iinv = fe_pow<F>(winv, (uint64_t)1 << (L - 2));   // i^-1, i = w_l^(N_l / 4) = the primitive fourth root w^(N / 4) at every layer
        const uint8_t *pp = paths;
        for (unsigned q = 0; q < Q; q++) {
            const uint64_t *vq = values + (size_t)q * vper * W;
            for (unsigned l = 0; l < R; l += 2) {
                const unsigned sides = l + 2 <= R ? 4 : 2, depth = L - l;
                const size_t part = ((size_t)1 << depth) / sides, j = idx[q] & (part - 1);
                const uint64_t *v = vq + (size_t)(l / 2) * 4 * W;
                Fe<F> e[4];
                for (unsigned s = 0; s < sides; s++) {
                    int ok_s = 0;
                    ZK_TRY(zk_merkle_verify(F::ID, roots + 32 * (l / 2), depth, j + s * part, v + (size_t)s * W, pp, &ok_s));
                    pp += 32 * (size_t)depth;
                    if (!ok_s) return ZK_OK;
                    e[s] = load_host<F>(v + (size_t)s * W);
                }
                const Fe<F> xinv = fe_mul<F>(cinv[l], fe_pow<F>(winv, (uint64_t)j << l));
                Fe<F> got;
                if (sides == 4) got = fold(fold(e[0], e[2], beta[l], xinv), fold(e[1], e[3], beta[l], fe_mul<F>(xinv, iinv)), beta[l + 1], fe_sqr<F>(xinv));
                else got = fold(e[0], e[1], beta[l], xinv);
                const unsigned ln = l + (sides == 4 ? 2 : 1);  // the layer the step lands in: j is a position of it
                Fe<F> want;
                if (ln < R) {
                    const size_t npart = ((size_t)1 << (L - ln)) / (ln + 2 <= R ? 4 : 2);
                    want = load_host<F>(vq + ((size_t)(ln / 2) * 4 + j / npart) * W);
                } else want = uni_evaluate<F>(h, fe_mul<F>(cR, fe_pow<F>(w, (uint64_t)j << R)));
                if (!fe_eq<F>(got, want)) return ZK_OK;
            }
        }
        *ok = 1;
        return ZK_OK;
    }
    const size_t per = path_digests(L, R);
    for (unsigned q = 0; q < Q; q++) {
        const uint8_t *pp = paths + (size_t)q * per * 32;
        for (unsigned l = 0; l < R; l++) {
            const size_t half = ((size_t)1 << (L - l)) >> 1, j = idx[q] & (half - 1);
            const uint64_t *lo = values + ((size_t)q * R + l) * 2 * W, *hi = lo + W;
            int ok_lo = 0, ok_hi = 0;
            ZK_TRY(zk_merkle_verify(F::ID, roots + 32 * l, L - l, j, lo, pp, &ok_lo));
            ZK_TRY(zk_merkle_verify(F::ID, roots + 32 * l, L - l, j + half, hi, pp + 32 * (L - l), &ok_hi));
            pp += 64 * (size_t)(L - l);
            if (!ok_lo || !ok_hi) return ZK_OK;
            const Fe<F> a = load_host<F>(lo), bb = load_host<F>(hi);
            const Fe<F> xinv = fe_mul<F>(cinv[l], fe_pow<F>(winv, (uint64_t)j << l));
            Fe<F> v;
            if (ml) {                                         // (1 - r) (a + b) / 2 + r (a - b) / (2 x)
                const Fe<F> even = fe_mul<F>(fe_sub<F>(fe_one<F>(), beta[l]), fe_add<F>(a, bb));
                v = fe_mul<F>(inv2, fe_add<F>(even, fe_mul<F>(fe_mul<F>(beta[l], xinv), fe_sub<F>(a, bb))));
            } else v = fe_mul<F>(inv2, fe_add<F>(fe_add<F>(a, bb), fe_mul<F>(fe_mul<F>(beta[l], xinv), fe_sub<F>(a, bb))));
            Fe<F> want;
            if (l + 1 < R) want = load_host<F>(values + (((size_t)q * R + l + 1) * 2 + (j >= half / 2 ? 1 : 0)) * W);
            else want = uni_evaluate<F>(h, fe_mul<F>(cR, fe_pow<F>(w, (uint64_t)j << R)));
            if (!fe_eq<F>(v, want)) return ZK_OK;
        }
    }
    *ok = 1;
    return ZK_OK;
}

}  // namespace

namespace zk {
int fri_verify_core(int field, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, const uint64_t *coset, Transcript &tr,
                    const uint8_t *roots, const uint64_t *final_coeffs, const uint64_t *query_values, const uint8_t *query_paths, int *ok,
                    uint64_t *indices_out, const FriMlClaim *ml) {
    if (ml && (!ml->z || !ml->y || !ml->round_polys || ml->npoints > 8)) return ZK_E_ARG;
    if (ml && (ml->log_arity < 1 || ml->log_arity > 2 || (ml->log_arity == 2 && (ml->npoints < 1 || log_final >= d || d - log_final < 2)))) return ZK_E_ARG;
    if (!roots || !final_coeffs || !query_values || !query_paths || !ok || field_limbs64(field) < 0) return ZK_E_ARG;
    ZK_TRY(params_check(log_blowup, nqueries));
    if (coset && is_zero_element(field, coset)) return ZK_E_ARG;
    if (d < 1 || log_final >= d) return ZK_E_ARG;
    if (d > 32) return ZK_E_RANGE;
    ZK_TRY(shape_check(field, d + log_blowup, log_blowup, log_final));
    FRI_DISPATCH(field, return verify_host<F>(d, log_blowup, log_final, nqueries, coset, tr, roots, final_coeffs, query_values, query_paths, ok, indices_out, ml));
    return ZK_OK;
}
}  // namespace zk

extern "C" {

int zk_fri_fold(const zk_table *codeword, const uint64_t *beta, const uint64_t *coset, zk_table **out) {
    if (!codeword || !beta || !out || field_limbs64(codeword->field) < 0 || codeword->len == 1) return ZK_E_ARG;
    if (coset && is_zero_element(codeword->field, coset)) return ZK_E_ARG;
    if (!is_pow2(codeword->len)) return ZK_E_NOT_POW2;
    if ((codeword->field != ZK_FR381 && codeword->field != ZK_BN254_FR) || ilog2(codeword->len) > two_adicity(codeword->field)) return ZK_E_RANGE;
    ZK_TRY(require_device());
    FRI_DISPATCH(codeword->field, return fold_once<F>(codeword, beta, coset, out));
    return ZK_OK;
}

int zk_fri_proof_sizes(uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, size_t *nroots, size_t *nfinal, size_t *nvalues,
                       size_t *path_bytes) {
    ZK_TRY(params_check(log_blowup, nqueries));
    if (d < 1 || log_final >= d) return ZK_E_ARG;
    if (d > 32 || d + log_blowup > 32) return ZK_E_RANGE;
    const unsigned R = d - log_final;
    if (nroots) *nroots = R;
    if (nfinal) *nfinal = (size_t)1 << log_final;
    if (nvalues) *nvalues = (size_t)nqueries * R * 2;
    if (path_bytes) *path_bytes = (size_t)nqueries * path_digests(d + log_blowup, R) * 32;
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

int zk_fri_last_stats(zk_fri_stats *out) {
    if (!out) return ZK_E_ARG;
    *out = g_fri_stats;
    return ZK_OK;
}

}  // extern "C"
