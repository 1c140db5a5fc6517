// zkmle_fri_pcs.hip -- C ABI of the evaluation opening of FRI-committed polynomials (fri_pcs.cuh): the commitment object (coefficients,
// codeword and every level of its tree, resident in HBM), the evaluation of a coefficient table at a point, the DEEP quotient, the batched
// opening of k polynomials at one point and its host verifier.  Extension: the reference leaves `fri/` empty; the protocol is defined in
// include/zkmle.h "FRI polynomial commitment".
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "fri_host.h"
#include "fri_pcs.cuh"

using namespace zk;
using namespace zk::host;

namespace {

thread_local zk_fri_pcs_stats g_pcs_stats{};

template <class F> Fe<F> sqr_times(Fe<F> x, unsigned k) {
    while (k--) x = fe_sqr<F>(x);
    return x;
}
bool scalar_field(int field) { return field == ZK_FR381 || field == ZK_BN254_FR; }
// 1: z (reduced) lies in {c w^i}: (z / c)^N = 1
template <class F> bool in_domain(const uint64_t *z, const uint64_t *coset, unsigned L) {
    Fe<F> r = load_host<F>(z);
    if (coset) r = fe_mul<F>(r, fe_inv<F>(load_host<F>(coset)));
    return fe_eq<F>(sqr_times<F>(r, L), fe_one<F>());
}
// ZK_E_ARG for a point that is not a reduced element or lies in the evaluation domain of 2^L entries (scalar field, L within its two-adicity)
int point_check(int field, const uint64_t *z, const uint64_t *coset, unsigned L) {
    FRI_DISPATCH(field, return is_reduced<F>(z) && !in_domain<F>(z, coset, L) ? ZK_OK : ZK_E_ARG);
    return ZK_OK;
}
// the statuses of (field, d, b) that a commitment, and every proof on it, need before the device check
int shape_check(int field, uint64_t d, uint32_t b) {
    if (field_limbs64(field) < 0 || b < 1 || b > 8 || d < 1) return ZK_E_ARG;
    if (!scalar_field(field) || d + b > two_adicity(field)) return ZK_E_RANGE;
    return ZK_OK;
}
// base^e, e < n, as ntt_pow2t reads them (pre times base^lo as 29-bit limbs, base^(4096 hi)): hi stays null when n <= 4096
template <class F> struct PowTables {
    DevBuf buf;
    const void *lo = nullptr, *hi = nullptr;
    int build(const Fe<F> &base, const Fe<F> &pre, size_t n) {
        const bool two = n > ((size_t)1 << kNttLoBits);
        const size_t lo_count = two ? (size_t)1 << kNttLoBits : n, hi_count = two ? n >> kNttLoBits : 0;
        const size_t off_hi = (lo_count * sizeof(Ufe<F>) + 63) / 64 * 64;
        ZK_TRY(buf.alloc(off_hi + (hi_count + 1) * sizeof(Fe<F>)));
        const size_t blocks = (lo_count + kNttBlock - 1) / kNttBlock;
        ntt_pow_table_kernel<F, true><<<(unsigned)blocks, kNttBlock, 0, cur_stream()>>>(base, pre, (uint32_t)lo_count, buf.p);
        ZK_HIP(hipGetLastError());
        lo = buf.p;
        if (two) {
            const size_t hb = (hi_count + kNttBlock - 1) / kNttBlock;
            ntt_pow_table_kernel<F, false><<<(unsigned)(hb < 1024 ? hb : 1024), kNttBlock, 0, cur_stream()>>>(sqr_times<F>(base, kNttLoBits), fe_one<F>(),
                                                                                                              (uint32_t)hi_count, (char *)buf.p + off_hi);
            ZK_HIP(hipGetLastError());
            hi = (char *)buf.p + off_hi;
        }
        return ZK_OK;
    }
};

// ---- evaluation ----------------------------------------------------------------------------------------------------------------
// the grid cap of the evaluation: kPcsEvalMaxBlocks.  ZK_FRI_PCS_EVAL_BLOCKS (environment, read per call; tests) lowers it, clamped to
// 1 .. kPcsEvalMaxBlocks, so that a short table takes the later trips of the kernel's stride loop.
unsigned eval_block_cap() {
    const char *e = getenv("ZK_FRI_PCS_EVAL_BLOCKS");
    if (!e || !*e) return kPcsEvalMaxBlocks;
    const long v = atol(e);
    return v < 1 ? 1u : (v > (long)kPcsEvalMaxBlocks ? kPcsEvalMaxBlocks : (unsigned)v);
}
// out[slot] (device) = sum_i coeffs[i] z^i: launches only.  `partials`: room for kPcsEvalMaxBlocks elements.
template <class F> int launch_evaluate(const zk_table *coeffs, const Fe<F> &z, const PowTables<F> &pw, void *partials, void *out, unsigned slot) {
    const size_t nruns = (coeffs->len + kPcsEvalRun - 1) / kPcsEvalRun, want = (nruns + kPcsBlock - 1) / kPcsBlock, cap = eval_block_cap();
    const unsigned blocks = (unsigned)(want < cap ? want : cap);
    pcs_eval_kernel<F><<<blocks, kPcsBlock, 0, cur_stream()>>>(coeffs->dptr, coeffs->len, pw.lo, pw.hi, z, partials);
    ZK_HIP(hipGetLastError());
    pcs_eval_finish_kernel<F><<<1, kPcsBlock, 0, cur_stream()>>>(partials, blocks, out, slot);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}
// ys (host) = the k tables (equal length) at z: one power table, 2 k launches, one download
template <class F> int evaluate_many(const zk_table *const *tables, size_t k, const uint64_t *z64, uint64_t *ys) {
    const Fe<F> z = load_host<F>(z64);
    PowTables<F> pw;
    ZK_TRY(pw.build(z, fe_one<F>(), tables[0]->len));
    DevBuf work;
    ZK_TRY(work.alloc((kPcsEvalMaxBlocks + k) * sizeof(Fe<F>)));
    void *res = (char *)work.p + kPcsEvalMaxBlocks * sizeof(Fe<F>);
    for (size_t j = 0; j < k; j++) ZK_TRY((launch_evaluate<F>(tables[j], z, pw, work.p, res, (unsigned)j)));
    ZK_HIP(zk::memcpy_on_stream(ys, res, k * sizeof(Fe<F>), hipMemcpyDeviceToHost));
    return ZK_OK;
}

// ---- the quotient --------------------------------------------------------------------------------------------------------------
// T of the batch inversion for a domain of n entries.  A lane's chain is one Fermat inversion (about 380 products) plus 3 (T - 1), and the
// pass is bound by those products, not by memory: measured (profiles/fri_pcs/) T = 4 and 8 beat 2 and 1 at n = 2^18, T = 16 beats 8 at
// 2^22.  What a longer chain costs is lanes, so T grows only once every CU has a block: T = n / 2^16, between 1 and 16 (16 is the variant that
// parks its prefixes in the output).  ZK_FRI_PCS_BATCH = 1, 2, 4, 8, 16 (environment, read per call; tests and measurements) overrides it.
unsigned pick_batch(size_t n) {
    const char *e = getenv("ZK_FRI_PCS_BATCH");
    const int v = e ? atoi(e) : 0;
    if (v == 1 || v == 2 || v == 4 || v == 8 || v == kPcsMemBatch) return (unsigned)v;
    unsigned t = 1;
    while (t < (unsigned)kPcsMemBatch && (n / t) > ((size_t)1 << 16)) t *= 2;
    return t;
}
template <class F, int T, bool MEM> int launch_quotient_t(const PcsTables &tb, unsigned k, void *out, size_t n, const PowTables<F> &x, const Fe<F> &z,
                                                          const Fe<F> &csum, const FriUni &g) {
    const size_t per = (size_t)T * kPcsBlock;
    pcs_quotient_kernel<F, T, MEM><<<(unsigned)((n + per - 1) / per), kPcsBlock, 0, cur_stream()>>>(tb, k, out, n, x.lo, x.hi, z, csum, g);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}
// out[i] = (sum_j gamma^j (f_j[i] - y_j)) / (c w^i - z) over the k codewords; launches only.  *batch: the T used.
template <class F> int launch_quotient(const zk_fri_commitment *const *cms, size_t k, const uint64_t *z64, const uint64_t *ys, const Fe<F> &gamma,
                                       zk_table *out, unsigned *batch) {
    const zk_fri_commitment *c0 = cms[0];
    const unsigned L = c0->d + c0->b;
    const size_t n = (size_t)1 << L;
    PowTables<F> x;
    ZK_TRY(x.build(root_of_unity<F>(L), c0->has_coset ? load_host<F>(c0->coset) : fe_one<F>(), n));
    Fe<F> csum = fe_zero<F>(), gp = fe_one<F>();              // sum_j gamma^j y_j
    PcsTables tb{};
    for (size_t j = 0; j < k; j++) {
        csum = fe_add<F>(csum, fe_mul<F>(gp, load_host<F>(ys + j * (F::N / 2))));
        gp = fe_mul<F>(gp, gamma);
        tb.cw[j] = cms[j]->codeword->dptr;
    }
    const FriUni g = fri_uni<F>(gamma);
    const Fe<F> z = load_host<F>(z64);
    const unsigned T = pick_batch(n);
    *batch = T;
    switch (T) {
        case 1: return launch_quotient_t<F, 1, false>(tb, (unsigned)k, out->dptr, n, x, z, csum, g);
        case 2: return launch_quotient_t<F, 2, false>(tb, (unsigned)k, out->dptr, n, x, z, csum, g);
        case 4: return launch_quotient_t<F, 4, false>(tb, (unsigned)k, out->dptr, n, x, z, csum, g);
        case 8: return launch_quotient_t<F, 8, false>(tb, (unsigned)k, out->dptr, n, x, z, csum, g);
        default: return launch_quotient_t<F, kPcsMemBatch, true>(tb, (unsigned)k, out->dptr, n, x, z, csum, g);
    }
}

// the checks on a set of commitments and a point shared by the quotient and the opening
int set_check(const zk_fri_commitment *const *cms, size_t k, const uint64_t *z) {
    if (!cms || !z || k < 1 || k > kPcsMaxPolys) return ZK_E_ARG;
    for (size_t j = 0; j < k; j++)
        if (!cms[j]) return ZK_E_ARG;
    const zk_fri_commitment *c0 = cms[0];
    ZK_TRY(point_check(c0->field, z, c0->has_coset ? c0->coset : nullptr, c0->d + c0->b));
    for (size_t j = 1; j < k; j++) {
        const zk_fri_commitment *c = cms[j];
        if (c->field != c0->field || c->d != c0->d || c->b != c0->b || c->has_coset != c0->has_coset || memcmp(c->coset, c0->coset, 32)) return ZK_E_LEN_MISMATCH;
    }
    return ZK_OK;
}

// ---- transcript ----------------------------------------------------------------------------------------------------------------
// step 2 of the protocol, shared by prover and verifier: k, the roots, z, the evaluations; then gamma
template <class F> Fe<F> opening_challenge(Transcript &tr, size_t k, const uint8_t *const *roots, const uint64_t *z, const uint64_t *ys) {
    uint8_t kb[4];
    put_be32(kb, (uint32_t)k);
    tr.append(kb, 4);
    for (size_t j = 0; j < k; j++) tr.append(roots[j], 32);
    tr.append_be<F>(load_host<F>(z));
    for (size_t j = 0; j < k; j++) tr.append_be<F>(load_host<F>(ys + j * (F::N / 2)));
    return tr.random_challenge_as_field_element<F>();
}

struct OpenOut {
    uint64_t *ys;
    uint8_t *roots;
    uint64_t *final_coeffs, *betas, *query_indices, *query_values;
    uint8_t *query_paths;
    uint64_t *opened_values;
    uint8_t *opened_paths;
};

template <class F> int open_any(const zk_fri_commitment *const *cms, size_t k, const uint64_t *z, uint32_t f, uint32_t Q, zk_transcript *t, const OpenOut &o) {
    constexpr size_t ESZ = sizeof(Fe<F>);
    const auto t0 = std::chrono::steady_clock::now();
    const zk_fri_commitment *c0 = cms[0];
    const unsigned L = c0->d + c0->b;
    const size_t n = (size_t)1 << L;
    Events ev;
    size_t e0, e1, e2, e3, e4;
    zk_fri_pcs_stats st{};
    st.polys = (uint32_t)k;

    ZK_TRY(ev.mark(&e0));
    std::vector<const zk_table *> coeffs(k);
    std::vector<const uint8_t *> roots(k);
    for (size_t j = 0; j < k; j++) { coeffs[j] = cms[j]->coeffs; roots[j] = cms[j]->root; }
    ZK_TRY((evaluate_many<F>(coeffs.data(), k, z, o.ys)));
    ZK_TRY(ev.mark(&e1));

    zk_transcript fresh;
    zk_transcript *tt = t ? t : &fresh;
    const Fe<F> gamma = opening_challenge<F>(tt->t, k, roots.data(), z, o.ys);
    TableHolder hold;
    zk_table *quot = nullptr;
    ZK_TRY(hold.alloc(c0->field, n, &quot));
    ZK_TRY((launch_quotient<F>(cms, k, z, o.ys, gamma, quot, &st.batch)));
    ZK_TRY(ev.mark(&e2));

    std::vector<uint64_t> idx_own;
    uint64_t *idx = o.query_indices;
    if (!idx) { idx_own.resize(Q); idx = idx_own.data(); }
    ZK_TRY(zk_fri_prove_codeword(quot, c0->b, f, Q, c0->has_coset ? c0->coset : nullptr, tt, o.roots, o.final_coeffs, o.betas, idx, o.query_values, o.query_paths));
    ZK_TRY(ev.mark(&e3));

    PcsTrees tr{};
    for (size_t j = 0; j < k; j++) { tr.cw[j] = cms[j]->codeword->dptr; tr.tree[j] = cms[j]->levels; }
    const size_t nval = (size_t)Q * 2 * k, ndig = nval * L;
    DevBuf didx, dval, dpath;
    ZK_TRY(didx.alloc(Q * 8));
    ZK_TRY(dval.alloc(nval * ESZ));
    ZK_TRY(dpath.alloc(ndig * 32));
    ZK_HIP(hipMemcpyAsync(didx.p, idx, Q * 8, hipMemcpyHostToDevice, cur_stream()));
    pcs_open_values_kernel<F><<<(unsigned)((nval + kPcsBlock - 1) / kPcsBlock), kPcsBlock, 0, cur_stream()>>>(tr, (unsigned)k, n, (const uint64_t *)didx.p, Q, dval.p);
    ZK_HIP(hipGetLastError());
    const size_t pb = (ndig + kPcsBlock - 1) / kPcsBlock;
    pcs_open_paths_kernel<<<(unsigned)(pb < 4096 ? pb : 4096), kPcsBlock, 0, cur_stream()>>>(tr, (unsigned)k, L, (const uint64_t *)didx.p, Q, (uint64_t *)dpath.p);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(o.opened_values, dval.p, nval * ESZ, hipMemcpyDeviceToHost, cur_stream()));   // one download each, one wait for both
    ZK_HIP(zk::memcpy_on_stream(o.opened_paths, dpath.p, ndig * 32, hipMemcpyDeviceToHost));
    ZK_TRY(ev.mark(&e4));
    ZK_HIP(hipEventSynchronize(ev.ev[e4]));
    st.ms_evals = ev.ms(e0, e1);
    st.ms_quotient = ev.ms(e1, e2);
    st.ms_fri = ev.ms(e2, e3);
    st.ms_gather = ev.ms(e3, e4);
    st.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g_pcs_stats = st;
    return ZK_OK;
}

// ---- the verifier (host) -------------------------------------------------------------------------------------------------------
template <class F> int verify_host(size_t k, const uint8_t *roots_f, uint32_t d, uint32_t b, uint32_t f, uint32_t Q, const uint64_t *coset, const uint64_t *z64,
                                   const uint64_t *ys, Transcript &tr, const uint8_t *roots, const uint64_t *final_coeffs, const uint64_t *values,
                                   const uint8_t *paths, const uint64_t *opened, const uint8_t *opened_paths, int *ok) {
    constexpr int W = F::N / 2;
    const unsigned L = d + b;
    const size_t half = ((size_t)1 << L) >> 1, R = d - f;
    bool good = is_reduced<F>(z64);
    for (size_t j = 0; good && j < k; j++) good = is_reduced<F>(ys + j * W);
    for (size_t e = 0; good && e < (size_t)Q * 2 * k; e++) good = is_reduced<F>(opened + e * W);
    std::vector<const uint8_t *> rp(k);
    for (size_t j = 0; j < k; j++) rp[j] = roots_f + 32 * j;
    const Fe<F> gamma = opening_challenge<F>(tr, k, rp.data(), z64, ys);
    std::vector<uint64_t> idx(Q);
    int fri_ok = 0;
    ZK_TRY(fri_verify_core(F::ID, d, b, f, Q, coset, tr, roots, final_coeffs, values, paths, &fri_ok, idx.data()));
    *ok = 0;
    if (!good || !fri_ok) return ZK_OK;

    const Fe<F> z = load_host<F>(z64), c = coset ? load_host<F>(coset) : fe_one<F>(), w = root_of_unity<F>(L);
    for (unsigned q = 0; q < Q; q++) {
        for (unsigned s = 0; s < 2; s++) {
            const size_t pos = idx[q] + s * half, e0 = ((size_t)q * 2 + s) * k;
            Fe<F> num = fe_zero<F>();
            for (size_t j = k; j-- > 0;) {                     // Horner in gamma
                const uint64_t *v = opened + (e0 + j) * W;
                int path_ok = 0;
                ZK_TRY(zk_merkle_verify(F::ID, rp[j], L, pos, v, opened_paths + (e0 + j) * L * 32, &path_ok));
                if (!path_ok) return ZK_OK;
                num = fe_add<F>(fe_mul<F>(num, gamma), fe_sub<F>(load_host<F>(v), load_host<F>(ys + j * W)));
            }
            const Fe<F> x = fe_mul<F>(c, fe_pow<F>(w, pos));
            const Fe<F> q0 = load_host<F>(values + ((size_t)q * R * 2 + s) * W);       // FRI's layer 0 at the same position
            if (!fe_eq<F>(num, fe_mul<F>(fe_sub<F>(x, z), q0))) return ZK_OK;
        }
    }
    *ok = 1;
    return ZK_OK;
}

// zk_fri_commit (lg = 0) and zk_fri_commit_grouped (lg = 2): the tree has N >> lg leaves
int commit_any(const zk_table *coeffs, uint32_t log_blowup, const uint64_t *coset, unsigned lg, zk_fri_commitment **out) {
    if (!coeffs || !out || field_limbs64(coeffs->field) < 0 || log_blowup < 1 || log_blowup > 8) return ZK_E_ARG;
    if (coset && is_zero_element(coeffs->field, coset)) return ZK_E_ARG;
    if (coeffs->len == 1) return ZK_E_ARG;
    if (!is_pow2(coeffs->len)) return ZK_E_NOT_POW2;
    ZK_TRY(shape_check(coeffs->field, ilog2(coeffs->len), log_blowup));
    ZK_TRY(require_device());
    zk_fri_commitment *cm = new zk_fri_commitment{};
    cm->field = coeffs->field;
    cm->d = ilog2(coeffs->len);
    cm->b = log_blowup;
    cm->log_group = lg;
    cm->has_coset = coset != nullptr;
    if (coset) memcpy(cm->coset, coset, 32);
    const size_t n = coeffs->len << log_blowup, leaves = n >> lg;         // N >= 4: d >= 1 and b >= 1
    int rc = zk_table_clone(coeffs, &cm->coeffs);
    if (rc == ZK_OK) rc = zk_table_alloc(coeffs->field, n, &cm->codeword);
    if (rc == ZK_OK) {
        void *lv = nullptr;
        if (hipMalloc(&lv, (2 * leaves - 1) * 32) != hipSuccess) { set_last_error("zk_fri_commit: no memory for the tree"); rc = ZK_E_NOMEM; }
        cm->levels = (uint64_t *)lv;
    }
    if (rc == ZK_OK) rc = ntt_extend_into(cm->coeffs, coset, cm->codeword);
    if (rc == ZK_OK) rc = merkle_levels_grouped_device(cm->codeword, lg, cm->levels);
    if (rc == ZK_OK && zk::memcpy_on_stream(cm->root, cm->levels + 4 * (2 * leaves - 2), 32, hipMemcpyDeviceToHost) != hipSuccess) {
        set_last_error("zk_fri_commit: the transform or the hash kernels failed");
        rc = ZK_E_HIP;
    }
    if (rc != ZK_OK) { zk_fri_commitment_free(cm); return rc; }
    *out = cm;
    return ZK_OK;
}

thread_local zk_fri_columns_stats g_columns_stats{};

// zk_fri_commit_columns: commit_any's statuses over k tables, then k transforms and ONE tree over the k codewords.  adopt (else null): k device
// tables the caller owns and hands over, the same objects as `tables`: they become the commitment's own in place of clones when the status is
// ZK_OK and stay the caller's otherwise
int commit_columns(const zk_table *const *tables, uint32_t k, uint32_t log_blowup, const uint64_t *coset, zk_fri_columns **out, zk_table *const *adopt = nullptr) {
    if (!tables || !out || k < 1 || k > ZK_FRI_COLUMNS_MAX || !tables[0] || log_blowup < 1 || log_blowup > 8) return ZK_E_ARG;
    const int field = tables[0]->field;
    if (field_limbs64(field) != 4) return ZK_E_ARG;
    for (uint32_t c = 1; c < k; c++)
        if (!tables[c] || tables[c]->field != field) return ZK_E_ARG;
    if (coset && is_zero_element(field, coset)) return ZK_E_ARG;
    for (uint32_t c = 0; c < k; c++)
        if (tables[c]->len == 1) return ZK_E_ARG;
    for (uint32_t c = 1; c < k; c++)
        if (tables[c]->len != tables[0]->len) return ZK_E_LEN_MISMATCH;
    if (!is_pow2(tables[0]->len)) return ZK_E_NOT_POW2;
    ZK_TRY(shape_check(field, ilog2(tables[0]->len), log_blowup));
    ZK_TRY(require_device());
    const auto t0 = std::chrono::steady_clock::now();
    zk_fri_columns *cm = new zk_fri_columns{};
    cm->field = field;
    cm->d = ilog2(tables[0]->len);
    cm->b = log_blowup;
    cm->k = k;
    cm->has_coset = coset != nullptr;
    if (coset) memcpy(cm->coset, coset, 32);
    const size_t n = tables[0]->len << log_blowup, leaves = n >> 2;       // N >= 4: d >= 1 and b >= 1
    int rc = ZK_OK;
    for (uint32_t c = 0; c < k && rc == ZK_OK; c++) {
        if (adopt) cm->coeffs[c] = adopt[c];
        else rc = zk_table_clone(tables[c], &cm->coeffs[c]);
        if (rc == ZK_OK) rc = zk_table_alloc(field, n, &cm->codeword[c]);
    }
    if (rc == ZK_OK) {
        void *lv = nullptr;
        if (hipMalloc(&lv, (2 * leaves - 1) * 32) != hipSuccess) { set_last_error("zk_fri_commit_columns: no memory for the tree"); rc = ZK_E_NOMEM; }
        cm->levels = (uint64_t *)lv;
    }
    Events ev;
    size_t e0 = 0, e1 = 0, e2 = 0, e3 = 0;
    const auto run = [&]() -> int {
        ZK_TRY(ev.mark(&e0));
        for (uint32_t c = 0; c < k; c++) ZK_TRY(ntt_extend_into(cm->coeffs[c], coset, cm->codeword[c]));
        ZK_TRY(ev.mark(&e1));
        ZK_TRY(merkle_leaves_columns_device(cm->codeword, k, cm->levels));
        ZK_TRY(ev.mark(&e2));
        ZK_TRY(merkle_nodes_device(cm->levels, leaves));
        ZK_TRY(ev.mark(&e3));
        return ZK_OK;
    };
    if (rc == ZK_OK) rc = run();
    if (rc == ZK_OK && zk::memcpy_on_stream(cm->root, cm->levels + 4 * (2 * leaves - 2), 32, hipMemcpyDeviceToHost) != hipSuccess) {
        set_last_error("zk_fri_commit_columns: the transforms or the hash kernels failed");
        rc = ZK_E_HIP;
    }
    if (rc != ZK_OK) {
        (void)hipStreamSynchronize(cur_stream());
        for (uint32_t c = 0; adopt && c < k; c++) cm->coeffs[c] = nullptr;   // still the caller's
        zk_fri_columns_free(cm);
        return rc;
    }
    zk_fri_columns_stats st{};
    st.columns = k;
    st.ms_extend = ev.ms(e0, e1);
    st.ms_leaves = ev.ms(e1, e2);
    st.ms_nodes = ev.ms(e2, e3);
    st.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g_columns_stats = st;
    *out = cm;
    return ZK_OK;
}

}  // namespace

int zk::fri_commit_columns_adopt(zk_table *const *tables, uint32_t k, uint32_t log_blowup, const uint64_t *coset, zk_fri_columns **out) {
    for (uint32_t c = 0; tables && c < k && c < ZK_FRI_COLUMNS_MAX; c++)
        if (tables[c] && (tables[c]->owned == 0 || !tables[c]->dptr)) return ZK_E_ARG;      // a view of the caller's memory cannot change hands
    return commit_columns(tables, k, log_blowup, coset, out, tables);
}

extern "C" {

int zk_fri_commit_columns(const zk_table *const *tables, uint32_t k, uint32_t log_blowup, const uint64_t *coset, zk_fri_columns **out) {
    return commit_columns(tables, k, log_blowup, coset, out);
}
int zk_fri_columns_free(zk_fri_columns *cm) {
    if (!cm) return ZK_OK;
    for (uint32_t c = 0; c < ZK_FRI_COLUMNS_MAX; c++) {
        zk_table_free(cm->coeffs[c]);
        zk_table_free(cm->codeword[c]);
    }
    if (cm->levels) (void)hipFree(cm->levels);
    delete cm;
    return ZK_OK;
}
int zk_fri_columns_root(const zk_fri_columns *cm, uint8_t root32[32]) {
    if (!cm || !root32) return ZK_E_ARG;
    memcpy(root32, cm->root, 32);
    return ZK_OK;
}
uint32_t zk_fri_columns_count(const zk_fri_columns *cm) { return cm ? cm->k : 0; }
int zk_fri_columns_table(const zk_fri_columns *cm, uint32_t j, const zk_table **out) {
    if (!cm || !out) return ZK_E_ARG;
    if (j >= cm->k) return ZK_E_RANGE;
    *out = cm->coeffs[j];
    return ZK_OK;
}
int zk_fri_columns_codeword(const zk_fri_columns *cm, uint32_t j, const zk_table **out) {
    if (!cm || !out) return ZK_E_ARG;
    if (j >= cm->k) return ZK_E_RANGE;
    *out = cm->codeword[j];
    return ZK_OK;
}
int zk_fri_columns_last_stats(zk_fri_columns_stats *out) {
    if (!out) return ZK_E_ARG;
    *out = g_columns_stats;
    return ZK_OK;
}

int zk_fri_commit(const zk_table *coeffs, uint32_t log_blowup, const uint64_t *coset, zk_fri_commitment **out) {
    return commit_any(coeffs, log_blowup, coset, 0, out);
}
int zk_fri_commit_grouped(const zk_table *coeffs, uint32_t log_blowup, const uint64_t *coset, uint32_t log_group, zk_fri_commitment **out) {
    if (log_group != 0 && log_group != 2) return ZK_E_ARG;
    return commit_any(coeffs, log_blowup, coset, log_group, out);
}
uint32_t zk_fri_commitment_log_group(const zk_fri_commitment *cm) { return cm ? cm->log_group : 0; }
int zk_fri_commitment_free(zk_fri_commitment *cm) {
    if (!cm) return ZK_OK;
    zk_table_free(cm->coeffs);
    zk_table_free(cm->codeword);
    if (cm->levels) (void)hipFree(cm->levels);
    delete cm;
    return ZK_OK;
}
int zk_fri_commitment_root(const zk_fri_commitment *cm, uint8_t root32[32]) {
    if (!cm || !root32) return ZK_E_ARG;
    memcpy(root32, cm->root, 32);
    return ZK_OK;
}
int zk_fri_commitment_codeword(const zk_fri_commitment *cm, const zk_table **out) {
    if (!cm || !out) return ZK_E_ARG;
    *out = cm->codeword;
    return ZK_OK;
}

int zk_fri_pcs_sizes(uint32_t k, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, size_t *nroots, size_t *nfinal, size_t *nvalues,
                     size_t *path_bytes, size_t *nopened, size_t *opened_path_bytes) {
    if (k < 1 || k > kPcsMaxPolys) return ZK_E_ARG;
    ZK_TRY(zk_fri_proof_sizes(d, log_blowup, log_final, nqueries, nroots, nfinal, nvalues, path_bytes));
    if (nopened) *nopened = (size_t)nqueries * 2 * k;
    if (opened_path_bytes) *opened_path_bytes = (size_t)nqueries * 2 * k * (d + log_blowup) * 32;
    return ZK_OK;
}

int zk_uni_evaluate_device(const zk_table *coeffs, const uint64_t *z, uint64_t *y) {
    if (!coeffs || !z || !y || field_limbs64(coeffs->field) < 0 || coeffs->len == 0) return ZK_E_ARG;
    if (!is_pow2(coeffs->len)) return ZK_E_NOT_POW2;
    if (!scalar_field(coeffs->field) || ilog2(coeffs->len) > 32) return ZK_E_RANGE;
    ZK_TRY(require_device());
    FRI_DISPATCH(coeffs->field, return evaluate_many<F>(&coeffs, 1, z, y));
    return ZK_OK;
}

int zk_fri_pcs_quotient(const zk_fri_commitment *const *cms, size_t k, const uint64_t *z, const uint64_t *ys, const uint64_t *gamma, zk_table **out) {
    if (!ys || !gamma || !out) return ZK_E_ARG;
    ZK_TRY(set_check(cms, k, z));
    ZK_TRY(require_device());
    zk_table *o = nullptr;
    ZK_TRY(zk_table_alloc(cms[0]->field, (size_t)1 << (cms[0]->d + cms[0]->b), &o));
    Events ev;
    size_t e0, e1;
    zk_fri_pcs_stats st{};
    st.polys = (uint32_t)k;
    int rc = ev.mark(&e0);
    if (rc == ZK_OK) FRI_DISPATCH(cms[0]->field, rc = launch_quotient<F>(cms, k, z, ys, load_host<F>(gamma), o, &st.batch));
    if (rc == ZK_OK) rc = ev.mark(&e1);
    if (rc == ZK_OK && hipEventSynchronize(ev.ev[e1]) != hipSuccess) { set_last_error("zk_fri_pcs_quotient: the kernel failed"); rc = ZK_E_HIP; }
    if (rc != ZK_OK) { zk_table_free(o); return rc; }
    st.ms_quotient = st.ms_total = ev.ms(e0, e1);
    g_pcs_stats = st;
    *out = o;
    return ZK_OK;
}

int zk_fri_pcs_open(const zk_fri_commitment *const *cms, size_t k, const uint64_t *z, uint32_t log_final, uint32_t nqueries, zk_transcript *t, uint64_t *ys_out,
                    uint8_t *roots, uint64_t *final_coeffs, uint64_t *betas, uint64_t *query_indices, uint64_t *query_values, uint8_t *query_paths,
                    uint64_t *opened_values, uint8_t *opened_paths) {
    if (!ys_out || !roots || !final_coeffs || !query_values || !query_paths || !opened_values || !opened_paths) return ZK_E_ARG;
    if (nqueries < 1 || nqueries > 4096) return ZK_E_ARG;
    ZK_TRY(set_check(cms, k, z));
    if (log_final >= cms[0]->d) return ZK_E_ARG;
    for (size_t j = 0; j < k; j++)
        if (cms[j]->log_group != 0) return ZK_E_ARG;         // the gather walks trees of 2 N - 1 digests
    ZK_TRY(require_device());
    const OpenOut o{ys_out, roots, final_coeffs, betas, query_indices, query_values, query_paths, opened_values, opened_paths};
    FRI_DISPATCH(cms[0]->field, return open_any<F>(cms, k, z, log_final, nqueries, t, o));
    return ZK_OK;
}

int zk_fri_pcs_verify(int field, size_t k, const uint8_t *roots_of_f, uint32_t d, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries,
                      const uint64_t *coset, const uint64_t *z, const uint64_t *ys, zk_transcript *t, const uint8_t *roots, const uint64_t *final_coeffs,
                      const uint64_t *query_values, const uint8_t *query_paths, const uint64_t *opened_values, const uint8_t *opened_paths, int *ok) {
    if (!roots_of_f || !z || !ys || !roots || !final_coeffs || !query_values || !query_paths || !opened_values || !opened_paths || !ok) return ZK_E_ARG;
    if (field_limbs64(field) < 0 || k < 1 || k > kPcsMaxPolys || nqueries < 1 || nqueries > 4096) return ZK_E_ARG;
    if (log_blowup < 1 || log_blowup > 8 || d < 1 || log_final >= d) return ZK_E_ARG;
    if (coset && is_zero_element(field, coset)) return ZK_E_ARG;
    ZK_TRY(shape_check(field, d, log_blowup));
    {                                                        // a point in the domain is refused; one that is not reduced is just no proof
        bool reduced = false;
        FRI_DISPATCH(field, reduced = is_reduced<F>(z) && (!coset || is_reduced<F>(coset)));
        if (reduced) ZK_TRY(point_check(field, z, coset, d + log_blowup));
    }
    Transcript fresh;
    FRI_DISPATCH(field, return verify_host<F>(k, roots_of_f, d, log_blowup, log_final, nqueries, coset, z, ys, t ? t->t : fresh, roots, final_coeffs,
                                               query_values, query_paths, opened_values, opened_paths, ok));
    return ZK_OK;
}

int zk_fri_pcs_last_stats(zk_fri_pcs_stats *out) {
    if (!out) return ZK_E_ARG;
    *out = g_pcs_stats;
    return ZK_OK;
}

}  // extern "C"
