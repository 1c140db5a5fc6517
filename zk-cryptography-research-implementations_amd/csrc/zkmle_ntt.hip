// zkmle_ntt.hip -- C ABI of the number-theoretic transform (ntt.cuh): roots of unity, the in-place transform of a table with an optional
// coset shift, the low-degree extension and the product of two coefficient tables.  Extension: the reference leaves `fft/` empty; the
// definition is arkworks' Radix2EvaluationDomain (include/zkmle.h).
#include <stdlib.h>
#include <string.h>

#include "host_util.h"
#include "ntt.cuh"

using namespace zk;
using host::DevBuf;
using host::load_host;

namespace {

// w_{2^S} = g^t, t = (p - 1) >> S; -1 where S = 1
template <class F> Fe<F> top_root() {
    constexpr unsigned S = NttField<F>::S;
    if (S == 1) return fe_neg<F>(fe_one<F>());
    uint32_t pm1[F::N + 2] = {0};
    for (int i = 0; i < F::N; i++) pm1[i] = F::p(i);
    pm1[0] -= 1;                                                        // p is odd
    Fe<F> acc = fe_one<F>(), b = fe_from_u64<F>(NttField<F>::G);
    for (unsigned bit = S; bit < 32u * F::N; bit++) {
        if ((pm1[bit >> 5] >> (bit & 31)) & 1) acc = fe_mul<F>(acc, b);
        b = fe_sqr<F>(b);
    }
    return acc;
}
template <class F> Fe<F> domain_root(unsigned log_n) {                  // w_{2^log_n}, log_n <= S
    static const Fe<F> top = top_root<F>();
    if (log_n == 0) return fe_one<F>();
    Fe<F> w = top;
    for (unsigned k = NttField<F>::S; k > log_n; k--) w = fe_sqr<F>(w);
    return w;
}
template <class F> Fe<F> sqr_times(Fe<F> x, unsigned k) {
    while (k--) x = fe_sqr<F>(x);
    return x;
}

// ZK_NTT_MAX_DIGIT_BITS = 3 .. 8 (environment, read per call; tests and measurements): the most levels one pass takes, which is also the
// largest transform done in one launch then.  Unset: 8 levels a pass, one launch up to 2^10 entries, three passes from 2^16.
unsigned digit_cap() {
    const char *e = getenv("ZK_NTT_MAX_DIGIT_BITS");
    const int v = e ? atoi(e) : 0;
    return v >= 3 && v <= (int)kNttDigitMax ? (unsigned)v : 0;
}
struct Plan {
    unsigned ndig;
    uint8_t dig[kNttMaxDigits];
};
Plan make_plan(unsigned log_n) {
    Plan pl{};
    const unsigned cap = digit_cap();
    if (log_n <= (cap ? cap : kNttTileLog)) {
        pl.ndig = 1;
        pl.dig[0] = (uint8_t)log_n;
        return pl;
    }
    const unsigned b = cap ? cap : kNttDigitMax;
    unsigned d = (log_n + b - 1) / b;
    if (!cap && log_n >= 16 && d < 3) d = 3;
    pl.ndig = d;
    for (unsigned k = 0; k < d; k++) pl.dig[k] = (uint8_t)(log_n / d + (k < log_n % d ? 1 : 0));
    return pl;
}

template <class F, bool UFORM> int pow_table(const Fe<F> &base, const Fe<F> &pre, size_t count, void *out) {
    const size_t blocks = (count + kNttBlock - 1) / kNttBlock;
    ntt_pow_table_kernel<F, UFORM><<<(unsigned)(blocks < 1024 ? blocks : 1024), kNttBlock, 0, cur_stream()>>>(base, pre, (uint32_t)count, out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

// dst[k] = sum_i src[i] c^i w^(i k) over n = 2^log_n entries (src entries from src_len on count as zero), or the inverse map; src may be dst.
// Every launch goes on the calling thread's stream; tables and the n-entry scratch of a transform of several passes come from its pool.
template <class F> int ntt_run(const void *src, size_t src_len, void *dst, unsigned log_n, bool inverse, const uint64_t *coset) {
    const size_t n = (size_t)1 << log_n;
    const Plan pl = make_plan(log_n);
    unsigned tw_log = 0;
    for (unsigned d = 0; d < pl.ndig; d++) tw_log = pl.dig[d] > tw_log ? pl.dig[d] : tw_log;
    Fe<F> wn = domain_root<F>(log_n);
    if (inverse) wn = fe_inv<F>(wn);
    const bool two = log_n > kNttLoBits;                                  // the powers need their second table
    const size_t lo_count = two ? (size_t)1 << kNttLoBits : n, hi_count = two ? n >> kNttLoBits : 0;
    const size_t usz = (sizeof(Ufe<F>) + 63) / 64 * 64;                   // table offsets stay 64-byte aligned
    const size_t tw_count = tw_log ? (size_t)1 << (tw_log - 1) : 1;
    const bool scaled = coset || inverse;
    const size_t off_tw = 0, off_tl = off_tw + tw_count * usz, off_th = off_tl + lo_count * usz, off_sl = off_th + (hi_count + 1) * sizeof(Fe<F>),
                 off_sh = off_sl + lo_count * usz, total = off_sh + (hi_count + 1) * sizeof(Fe<F>);
    DevBuf tabs, scratch;
    ZK_TRY(tabs.alloc(total));
    char *tb = (char *)tabs.p;
    const Fe<F> one = fe_one<F>();
    ZK_TRY((pow_table<F, true>(sqr_times<F>(wn, log_n - tw_log), one, tw_count, tb + off_tw)));
    if (pl.ndig > 1) {
        ZK_TRY((pow_table<F, true>(wn, one, lo_count, tb + off_tl)));
        if (two) ZK_TRY((pow_table<F, false>(sqr_times<F>(wn, kNttLoBits), one, hi_count, tb + off_th)));
        ZK_TRY(scratch.alloc(n * sizeof(Fe<F>)));
    }
    uint32_t scale_mask = 0;
    if (scaled) {
        Fe<F> pre = one, sb = one;
        if (inverse) pre = fe_inv<F>(fe_from_u64<F>((uint64_t)n));
        if (coset) {
            sb = load_host<F>(coset);
            if (inverse) sb = fe_inv<F>(sb);
            scale_mask = 0xffffffffu;
            ZK_TRY((pow_table<F, true>(sb, pre, lo_count, tb + off_sl)));
            if (two) ZK_TRY((pow_table<F, false>(sqr_times<F>(sb, kNttLoBits), one, hi_count, tb + off_sh)));
        } else {
            ZK_TRY((pow_table<F, true>(one, pre, 1, tb + off_sl)));          // n^-1 for every entry
        }
    }
    unsigned t_log = 0, s_log = log_n;
    for (unsigned d = 0; d < pl.ndig; d++) {
        const bool last = d + 1 == pl.ndig;
        const unsigned log_p = pl.dig[d];
        s_log -= log_p;
        NttPassArgs a{};
        a.src = d == 0 ? src : scratch.p;
        a.dst = last ? dst : scratch.p;
        a.src_len = d == 0 ? src_len : n;
        a.tw = tb + off_tw;
        a.tw_log = tw_log;
        a.log_n = log_n;
        a.log_p = log_p;
        a.log_s = s_log;
        a.log_t = t_log;
        a.ndig = pl.ndig;
        unsigned acc = 0;
        for (unsigned k = 0; k < pl.ndig; k++) { a.dig_log[k] = pl.dig[k]; a.t_log[k] = (uint8_t)acc; acc += pl.dig[k]; }
        a.log_k0 = pl.ndig > 1 ? pl.dig[0] : 0;
        const unsigned room = kNttTileLog > log_p ? kNttTileLog - log_p : 0, lim = last ? a.log_k0 : s_log;
        a.log_c = room < lim ? room : lim;
        if (!last) {
            a.twist_lo = tb + off_tl;
            a.twist_hi = two ? tb + off_th : nullptr;
        }
        if (scaled && (inverse ? last : d == 0)) {
            a.scale_mode = inverse ? 2 : 1;
            a.scale_mask = scale_mask;
            a.scale_lo = tb + off_sl;
            a.scale_hi = coset && two ? tb + off_sh : nullptr;
        }
        const size_t tiles = n >> (log_p + a.log_c);
        const size_t lds = (sizeof(Fe<F>) << (log_p + a.log_c)) + (((size_t)1 << log_p) / 2) * sizeof(uint32_t) * UParams<F>::L;
        if (last) ntt_pass_kernel<F, true><<<(unsigned)tiles, kNttBlock, lds, cur_stream()>>>(a);
        else ntt_pass_kernel<F, false><<<(unsigned)tiles, kNttBlock, lds, cur_stream()>>>(a);
        ZK_HIP(hipGetLastError());
        t_log += log_p;
    }
    return ZK_OK;
}

bool coset_is_zero(int field, const uint64_t *coset) {
    uint64_t x = 0;
    for (int k = 0; k < field_limbs64(field); k++) x |= coset[k];
    return x == 0;
}
unsigned two_adicity(int field) { return field == ZK_FR381 ? NttField<Fr381>::S : field == ZK_BN254_FR ? NttField<Bn254Fr>::S : 1; }

// the statuses of a transform of `len` entries that come before the device check
int ntt_check(int field, size_t len, const uint64_t *coset) {
    if (field_limbs64(field) < 0 || (coset && coset_is_zero(field, coset))) return ZK_E_ARG;
    if (!is_pow2(len)) return ZK_E_NOT_POW2;
    if (ilog2(len) > two_adicity(field)) return ZK_E_RANGE;
    return ZK_OK;
}

}  // namespace

namespace zk {
int ntt_extend_into(const zk_table *coeffs, const uint64_t *coset, zk_table *out) {
    ZK_DISPATCH_FIELD(coeffs->field, return ntt_run<F>(coeffs->dptr, coeffs->len, out->dptr, ilog2(out->len), false, coset));
    return ZK_OK;
}
}  // namespace zk

extern "C" {

int zk_ntt_two_adicity(int field, uint32_t *s) {
    if (!s || field_limbs64(field) < 0) return ZK_E_ARG;
    *s = two_adicity(field);
    return ZK_OK;
}
int zk_ntt_root_of_unity(int field, uint32_t log_n, uint64_t *omega) {
    if (!omega || field_limbs64(field) < 0) return ZK_E_ARG;
    if (log_n > two_adicity(field)) return ZK_E_RANGE;
    ZK_DISPATCH_FIELD(field, { const Fe<F> w = domain_root<F>(log_n); memcpy(omega, w.l, 4 * F::N); });
    return ZK_OK;
}
int zk_ntt(zk_table *t, int inverse, const uint64_t *coset) {
    if (!t) return ZK_E_ARG;
    ZK_TRY(ntt_check(t->field, t->len, coset));
    ZK_TRY(require_device());
    ZK_DISPATCH_FIELD(t->field, return ntt_run<F>(t->dptr, t->len, t->dptr, ilog2(t->len), inverse != 0, coset));
    return ZK_OK;
}
int zk_host_ntt(int field, const uint64_t *in, size_t n, int inverse, const uint64_t *coset, uint64_t *out) {
    if (!in || !out) return ZK_E_ARG;
    ZK_TRY(ntt_check(field, n, coset));
    zk_table *t = nullptr;
    ZK_TRY(zk_table_upload_raw(field, in, n, &t));
    int rc = zk_ntt(t, inverse, coset);
    if (rc == ZK_OK) rc = zk_table_download(t, out);
    zk_table_free(t);
    return rc;
}
int zk_uni_low_degree_extend(const zk_table *coeffs, uint32_t log_blowup, const uint64_t *coset, zk_table **out) {
    if (!coeffs || !out) return ZK_E_ARG;
    ZK_TRY(ntt_check(coeffs->field, coeffs->len, coset));
    if (log_blowup > 32 || ilog2(coeffs->len) + log_blowup > two_adicity(coeffs->field)) return ZK_E_RANGE;
    zk_table *o = nullptr;
    ZK_TRY(zk_table_alloc(coeffs->field, coeffs->len << log_blowup, &o));
    int rc = ZK_OK;
    ZK_DISPATCH_FIELD(coeffs->field, rc = ntt_run<F>(coeffs->dptr, coeffs->len, o->dptr, ilog2(o->len), false, coset));
    if (rc != ZK_OK) { zk_table_free(o); return rc; }
    *out = o;
    return ZK_OK;
}
int zk_uni_mul(const zk_table *a, const zk_table *b, zk_table **out) {
    if (!a || !b || !out || a->field != b->field) return ZK_E_ARG;
    if (a->len != b->len) return ZK_E_LEN_MISMATCH;
    ZK_TRY(ntt_check(a->field, a->len, nullptr));
    if (ilog2(a->len) + 1 > two_adicity(a->field)) return ZK_E_RANGE;
    const size_t n2 = 2 * a->len;
    zk_table *o = nullptr, *tmp = nullptr;
    ZK_TRY(zk_table_alloc(a->field, n2, &o));
    int rc = table_alloc_pooled(a->field, n2, &tmp);
    if (rc == ZK_OK) ZK_DISPATCH_FIELD(a->field, {
        rc = ntt_run<F>(a->dptr, a->len, o->dptr, ilog2(n2), false, nullptr);
        if (rc == ZK_OK) rc = ntt_run<F>(b->dptr, b->len, tmp->dptr, ilog2(n2), false, nullptr);
    });
    const zk_table *fac[2] = {o, tmp};
    if (rc == ZK_OK) rc = zk_prodpoly_reduce(fac, 2, o);
    if (rc == ZK_OK) rc = zk_ntt(o, 1, nullptr);
    zk_table_free(tmp);
    if (rc != ZK_OK) { zk_table_free(o); return rc; }
    *out = o;
    return ZK_OK;
}

}  // extern "C"
