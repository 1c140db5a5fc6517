// zkmle_r1cs.hip -- C ABI of the R1CS instance (r1cs.cuh, r1cs_host.h): the handle of three sparse matrices, its digest, and the two sparse
// passes a Spartan prover runs on it, each behind a hook of its own: the products A z, B z, C z and the rows bound at a point,
// M[y] = sum_x eq(rx, x) (A + rho B + rho^2 C)[x, y]; and that prover and its host verifier ("R1CS satisfiability: Spartan over a FRI commitment").  Extension: defined in include/zkmle.h "R1CS instance: sparse matrices times a table".
#include <string.h>

#include <new>

#include <chrono>

#include "r1cs.cuh"
#include "r1cs_host.h"
#include "zerocheck.cuh"
#include "zerocheck_driver.cuh"

using namespace zk;
using namespace zk::host;

namespace {

thread_local zk_r1cs_stats g_r1cs_stats{};

// what both hooks need before they launch: the device and the instance's copy on it
int r1cs_ready(zk_r1cs *inst) {
    ZK_TRY(require_device());
    return r1cs_upload(*inst);
}

// the products: out[k] (device, 2^s elements each) = matrix k times z (device, 2^d elements).  Launches only.
template <class F> int matvec_launch(const zk_r1cs &in, const void *z, void *const out[3]) {
    const R1csOut3 o{{out[0], out[1], out[2]}};
    const int cap = r1cs_block_cap();
    if (const size_t n = in.row_lane.size()) {
        r1cs_matvec_lane_kernel<F><<<grid_for(n, cap), kBlock, 0, cur_stream()>>>(in.dcsr, in.d_row_lane, n, in.s, z, o);
        ZK_HIP(hipGetLastError());
    }
    if (const size_t n = in.row_block.size()) {
        r1cs_matvec_block_kernel<F><<<(unsigned)(n < (size_t)cap ? n : (size_t)cap), kBlock, 0, cur_stream()>>>(in.dcsr, in.d_row_block, n, in.s, z, o);
        ZK_HIP(hipGetLastError());
    }
    return ZK_OK;
}

// the bound rows: M[y] for the columns below 2^(d-1), or (full) for all 2^d, from E = eq(rx, .) (device, 2^s elements).  Launches only.
template <class F> int bind_launch(const zk_r1cs &in, const void *E, const Fe<F> &rho, bool full, void *M) {
    const Fe<F> rho2 = fe_mul<F>(rho, rho);
    const size_t ncols = (size_t)1 << in.d;
    const int cap = r1cs_block_cap();
    if (const size_t n = full ? in.col_lane.size() : in.col_lane_half) {
        r1cs_bind_lane_kernel<F><<<grid_for(n, cap), kBlock, 0, cur_stream()>>>(in.dcsc, in.d_col_lane, n, ncols, E, rho, rho2, M);
        ZK_HIP(hipGetLastError());
    }
    if (const size_t n = full ? in.col_block.size() : in.col_block_half) {
        r1cs_bind_block_kernel<F><<<(unsigned)(n < (size_t)cap ? n : (size_t)cap), kBlock, 0, cur_stream()>>>(in.dcsc, in.d_col_block, n, ncols, E, rho, rho2, M);
        ZK_HIP(hipGetLastError());
    }
    return ZK_OK;
}

template <class F> int bind_rows(zk_r1cs &in, const uint64_t *rx, const uint64_t *rho, bool full, zk_table *out) {
    DevBuf E;
    ZK_TRY(E.alloc(sizeof(Fe<F>) << in.s));
    Events ev;
    size_t e0, e1, e2;
    ZK_TRY(ev.mark(&e0));
    EqBuilder<F> eqb;
    ZK_TRY(eqb.build(rx, in.s, E.p));
    ZK_TRY(ev.mark(&e1));
    ZK_TRY(bind_launch<F>(in, E.p, load_host<F>(rho), full, out->dptr));
    ZK_TRY(ev.mark(&e2));
    ZK_HIP(hipEventSynchronize(ev.ev[e2]));                   // E and the builder's halves go back to the pool behind the pass
    g_r1cs_stats.ms_eq = ev.ms(e0, e1);
    g_r1cs_stats.ms_bind = ev.ms(e1, e2);
    return ZK_OK;
}

// the zerocheck's pass over (Az, Bz, Cz, E) as zerocheck_driver.cuh's `launch` (zkmle_zerocheck.hip passes the same kernel and finish)
template <class F> int mul_round_launch(bool fold, const void *const *in, void *out0, size_t ostride, size_t q, const Fe<F> &r, unsigned, void *partials, void *sums) {
    ZerocheckTables t{};
    for (int j = 0; j < 4; j++) {
        t.in[j] = in[j];
        if (fold) t.out[j] = (char *)out0 + (size_t)j * ostride;
    }
    const int grid = reduce_grid_for(q);
    if (fold) zerocheck_mul_round_kernel<F, true><<<grid, kBlock, 0, cur_stream()>>>(t, q, r, partials);
    else zerocheck_mul_round_kernel<F, false><<<grid, kBlock, 0, cur_stream()>>>(t, q, r, partials);
    ZK_HIP(hipGetLastError());
    finish_sums_kernel<F><<<1, kBlock, 0, cur_stream()>>>(partials, (size_t)grid, ZerocheckMul::NODES, sums);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

struct ProveOut {
    uint64_t *tau, *round_polys, *challenges, *vs, *rho;
};

// steps 1 to 7 on `tr`: the statement, z, the products, the s rounds, va vb vc, rho, and M (device, 2^(d-1) elements, the caller's room)
template <class F> int prove_steps(zk_r1cs &in, const zk_fri_commitment *cmW, const uint64_t *pub, uint32_t l, Transcript &tr, const ProveOut &o, void *M, zk_r1cs_stats &st) {
    constexpr size_t ESZ = sizeof(Fe<F>);
    constexpr int W = F::N / 2;
    const unsigned s = in.s, d = in.d;
    const size_t rows = (size_t)1 << s, half = (size_t)1 << (d - 1);
    std::vector<uint64_t> tau((size_t)s * W), rx((size_t)s * W);
    r1cs_statement<F>(tr, in, cmW->root, pub, l, tau.data());
    if (o.tau) memcpy(o.tau, tau.data(), tau.size() * 8);
    // z = (w || 1, pi_1 .. pi_l, 0 ..) and the three products behind one another
    DevBuf zb, prod;
    ZK_TRY(zb.alloc(2 * half * ESZ));
    ZK_TRY(prod.alloc(3 * rows * ESZ));
    std::vector<uint64_t> x((size_t)(l + 1) * W);
    store_host<F>(x.data(), fe_one<F>());
    if (l) memcpy(x.data() + W, pub, (size_t)l * W * 8);
    Events ev;
    size_t e0, e1, e2, e3;
    ZK_TRY(ev.mark(&e0));
    ZK_HIP(hipMemcpyAsync(zb.p, cmW->coeffs->dptr, half * ESZ, hipMemcpyDeviceToDevice, cur_stream()));
    ZK_HIP(hipMemsetAsync((char *)zb.p + half * ESZ, 0, half * ESZ, cur_stream()));
    ZK_HIP(zk::memcpy_on_stream((char *)zb.p + half * ESZ, x.data(), x.size() * 8, hipMemcpyHostToDevice));
    void *op[3];
    const void *opened[3];
    for (int k = 0; k < 3; k++) opened[k] = op[k] = (char *)prod.p + (size_t)k * rows * ESZ;
    ZK_TRY(matvec_launch<F>(in, zb.p, op));
    ZK_TRY(ev.mark(&e1));
    ZK_TRY((prove_rounds<F, 4, 4, 4>(opened, s, tau.data(), tr, mul_round_launch<F>, ZerocheckMul::message<F>, o.round_polys, o.challenges, rx.data(), ev, nullptr,
                                     &st.ms_eq, &st.ms_rounds)));
    for (int k = 0; k < 3; k++) {
        const zk_table t{in.field, rows, op[k], 0};
        ZK_TRY(zk_mle_evaluate(&t, rx.data(), s, o.vs + (size_t)k * W));
        tr.append_be<F>(load_host<F>(o.vs + (size_t)k * W));
    }
    const Fe<F> rho = tr.random_challenge_as_field_element<F>();
    if (o.rho) store_host<F>(o.rho, rho);
    DevBuf E;
    ZK_TRY(E.alloc(rows * ESZ));
    ZK_TRY(ev.mark(&e2));
    EqBuilder<F> eqb;
    ZK_TRY(eqb.build(rx.data(), s, E.p));
    ZK_TRY(bind_launch<F>(in, E.p, rho, false, M));
    ZK_TRY(ev.mark(&e3));
    ZK_HIP(hipEventSynchronize(ev.ev[e3]));                   // z, the products, E and the builder's halves go back to the pool behind the pass
    st.ms_products = ev.ms(e0, e1);
    st.ms_bind = ev.ms(e2, e3);
    return ZK_OK;
}

}  // namespace

extern "C" {

int zk_r1cs_create(int field, uint32_t log_rows, uint32_t log_cols, const uint32_t *const rows[3], const uint32_t *const cols[3], const uint64_t *const vals[3],
                   const size_t nnz[3], zk_r1cs **out) {
    if (!rows || !cols || !vals || !nnz || !out) return ZK_E_ARG;
    if (field != ZK_FR381 && field != ZK_BN254_FR) return ZK_E_ARG;
    if (log_rows < 1 || log_cols < 2 || log_rows > kR1csMaxLog || log_cols > kR1csMaxLog) return ZK_E_ARG;
    uint64_t total = 0;
    for (int k = 0; k < 3; k++) {
        if (nnz[k] >> 32) return ZK_E_ARG;
        total += nnz[k];
    }
    if (total >> 32) return ZK_E_ARG;                         // the forms' offsets are 32 bits
    zk_r1cs *in = new (std::nothrow) zk_r1cs;
    if (!in) return ZK_E_NOMEM;
    in->field = field;
    in->s = log_rows;
    in->d = log_cols;
    for (int k = 0; k < 3; k++) {
        const int rc = r1cs_sort_matrix(field, log_rows, log_cols, rows[k], cols[k], vals[k], nnz[k], in->mat[k]);
        if (rc != ZK_OK) {
            delete in;
            return rc;
        }
    }
    FRI_DISPATCH(field, r1cs_digest<F>(*in, in->digest); r1cs_compress<F>(*in));
    *out = in;
    return ZK_OK;
}

int zk_r1cs_free(zk_r1cs *inst) {
    delete inst;
    return ZK_OK;
}

int zk_r1cs_digest(const zk_r1cs *inst, uint8_t digest32[32]) {
    if (!inst || !digest32) return ZK_E_ARG;
    memcpy(digest32, inst->digest, 32);
    return ZK_OK;
}

int zk_r1cs_shape(const zk_r1cs *inst, int *field, uint32_t *log_rows, uint32_t *log_cols, uint64_t nnz[3], uint64_t block_items[2]) {
    if (!inst) return ZK_E_ARG;
    if (field) *field = inst->field;
    if (log_rows) *log_rows = inst->s;
    if (log_cols) *log_cols = inst->d;
    for (int k = 0; nnz && k < 3; k++) nnz[k] = inst->mat[k].row.size();
    if (block_items) {
        block_items[0] = inst->row_block.size();
        block_items[1] = inst->col_block.size();
    }
    return ZK_OK;
}

int zk_r1cs_matvec(zk_r1cs *inst, const zk_table *z, zk_table *out[3]) {
    if (!inst || !z || !out || z->field != inst->field) return ZK_E_ARG;
    if (z->len != (size_t)1 << inst->d) return ZK_E_LEN_MISMATCH;
    ZK_TRY(r1cs_ready(inst));
    zk_table *o[3] = {};
    void *op[3];
    int rc = ZK_OK;
    for (int k = 0; k < 3 && rc == ZK_OK; k++) {
        rc = zk_table_alloc(inst->field, (size_t)1 << inst->s, &o[k]);
        if (rc == ZK_OK) op[k] = o[k]->dptr;
    }
    if (rc == ZK_OK) {
        rc = [&]() -> int {
            Events ev;
            size_t e0, e1;
            ZK_TRY(ev.mark(&e0));
            FRI_DISPATCH(inst->field, ZK_TRY(matvec_launch<F>(*inst, z->dptr, op)));
            ZK_TRY(ev.mark(&e1));
            ZK_HIP(hipEventSynchronize(ev.ev[e1]));
            g_r1cs_stats.ms_products = ev.ms(e0, e1);
            return ZK_OK;
        }();
    }
    if (rc != ZK_OK) {
        for (zk_table *t : o) zk_table_free(t);
        return rc;
    }
    for (int k = 0; k < 3; k++) out[k] = o[k];
    return ZK_OK;
}

int zk_r1cs_bind_rows(zk_r1cs *inst, const uint64_t *rx, const uint64_t *rho, int full, zk_table **out) {
    if (!inst || !rx || !rho || !out) return ZK_E_ARG;
    if (!all_reduced(inst->field, rx, inst->s) || !all_reduced(inst->field, rho, 1)) return ZK_E_ARG;
    ZK_TRY(r1cs_ready(inst));
    zk_table *M = nullptr;
    ZK_TRY(zk_table_alloc(inst->field, (size_t)1 << (full ? inst->d : inst->d - 1), &M));
    const int rc = [&]() -> int {
        FRI_DISPATCH(inst->field, ZK_TRY(bind_rows<F>(*inst, rx, rho, full != 0, M)));
        return ZK_OK;
    }();
    if (rc != ZK_OK) {
        zk_table_free(M);
        return rc;
    }
    *out = M;
    return ZK_OK;
}

int zk_r1cs_sizes(uint32_t log_rows, uint32_t log_cols, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries, uint32_t log_arity, uint32_t log_group,
                  size_t *nzc_round, size_t *nroots, size_t *nfinal, size_t *nvalues, size_t *path_bytes, size_t *nround) {
    if (log_rows < 1 || log_cols < 2 || log_rows > kR1csMaxLog || log_cols > kR1csMaxLog) return ZK_E_ARG;
    ZK_TRY(zk_fri_ml_sizes_weighted(log_cols - 1, log_blowup, log_final, nqueries, log_arity, log_group, nroots, nfinal, nvalues, path_bytes, nround));
    if (nzc_round) *nzc_round = (size_t)ZerocheckMul::NODES * log_rows;
    return ZK_OK;
}

int zk_r1cs_public_terms(const zk_r1cs *inst, const uint64_t *public_inputs, uint32_t l, const uint64_t *rx, const uint64_t *rho, const uint64_t *open_challenges,
                         uint32_t nchallenges, uint64_t *c_pub, uint64_t *w_final) {
    if (!inst || (l && !public_inputs) || !rx || !rho || !c_pub || (w_final && nchallenges && !open_challenges)) return ZK_E_ARG;
    if (nchallenges > inst->d - 1 || (uint64_t)l >= (uint64_t)1 << (inst->d - 1)) return ZK_E_ARG;
    if (!all_reduced(inst->field, public_inputs, l) || !all_reduced(inst->field, rx, inst->s) || !all_reduced(inst->field, rho, 1)) return ZK_E_ARG;
    if (w_final && !all_reduced(inst->field, open_challenges, nchallenges)) return ZK_E_ARG;
    FRI_DISPATCH(inst->field, Fe<F> cp; r1cs_public_terms<F>(*inst, public_inputs, l, rx, load_host<F>(rho), open_challenges, nchallenges, &cp, w_final);
                 store_host<F>(c_pub, cp));
    return ZK_OK;
}

int zk_r1cs_prove(zk_r1cs *inst, const zk_fri_commitment *cmW, const uint64_t *public_inputs, uint32_t l, uint32_t log_final, uint32_t nqueries, uint32_t log_arity,
                  uint32_t grinding_bits, zk_transcript *t, uint64_t *tau_out, uint64_t *round_polys, uint64_t *challenges, uint64_t *vs_out, uint64_t *rho_out,
                  uint64_t *c_out, uint64_t *open_round_polys, uint8_t *roots, uint64_t *final_table, uint64_t *open_challenges, uint64_t *query_indices,
                  uint64_t *query_values, uint8_t *query_paths, uint64_t *pow_nonce) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!inst || !cmW || !round_polys || !challenges || !vs_out || (l && !public_inputs)) return ZK_E_ARG;
    if (cmW->field != inst->field || cmW->d != inst->d - 1 || (uint64_t)l >= (uint64_t)1 << (inst->d - 1)) return ZK_E_ARG;
    if (!all_reduced(inst->field, public_inputs, l)) return ZK_E_ARG;
    // M does not exist yet: the opener's statuses are taken on a stand-in of its shape, before the transcript moves
    const zk_table shape{inst->field, (size_t)1 << (inst->d - 1), nullptr, 0};
    ZK_TRY(fri_ml_open_weighted_check(cmW, &shape, log_final, nqueries, log_arity, c_out, open_round_polys, roots, final_table, open_challenges, query_values, query_paths,
                                      grinding_bits, pow_nonce));
    ZK_TRY(r1cs_upload(*inst));
    DevBuf M;
    ZK_TRY(M.alloc((size_t)32 << (inst->d - 1)));
    zk_transcript own;
    zk_transcript *tt = t ? t : &own;
    zk_r1cs_stats st{};
    const ProveOut o{tau_out, round_polys, challenges, vs_out, rho_out};
    FRI_DISPATCH(inst->field, ZK_TRY(prove_steps<F>(*inst, cmW, public_inputs, l, tt->t, o, M.p, st)));
    const zk_table Mt{inst->field, (size_t)1 << (inst->d - 1), M.p, 0};
    ZK_TRY(zk_fri_ml_open_weighted(cmW, &Mt, log_final, nqueries, log_arity, grinding_bits, tt, c_out, open_round_polys, roots, final_table, open_challenges,
                                   query_indices, query_values, query_paths, pow_nonce));
    zk_fri_ml_stats ml{};
    (void)zk_fri_ml_last_stats(&ml);
    st.ms_opening = ml.ms_total;
    st.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g_r1cs_stats = st;
    return ZK_OK;
}

int zk_r1cs_verify(const zk_r1cs *inst, const uint8_t *root32, const uint64_t *public_inputs, uint32_t l, uint32_t log_blowup, uint32_t log_final, uint32_t nqueries,
                   uint32_t log_arity, uint32_t log_group, const uint64_t *coset, zk_transcript *t, const uint64_t *round_polys, const uint64_t *vs, const uint64_t *c,
                   const uint64_t *open_round_polys, const uint8_t *roots, const uint64_t *final_table, const uint64_t *open_challenges, const uint64_t *query_values,
                   const uint8_t *query_paths, uint32_t grinding_bits, uint64_t pow_nonce, int *ok) {
    if (!inst || (l && !public_inputs) || (uint64_t)l >= (uint64_t)1 << (inst->d - 1)) return ZK_E_ARG;
    const bool have_all = root32 && round_polys && vs && c && open_round_polys && roots && final_table && open_challenges && query_values && query_paths && ok;
    const uint32_t dw = inst->d - 1;
    ZK_TRY(verify_check(inst->field, dw, log_blowup, coset, grinding_bits, have_all, [&] {
        return zk_fri_ml_sizes_weighted(dw, log_blowup, log_final, nqueries, log_arity, log_group, nullptr, nullptr, nullptr, nullptr, nullptr);
    }));
    zk_transcript work;
    if (t) work.t = t->t;
    std::vector<uint64_t> w_final((size_t)4 << log_final, 0);
    bool good = false;
    FRI_DISPATCH(inst->field, r1cs_replay<F>(work.t, *inst, root32, public_inputs, l, round_polys, vs, c, open_challenges, dw - log_final, w_final.data(), &good));
    int open_ok = 0;
    ZK_TRY(zk_fri_ml_verify_weighted(inst->field, root32, dw, log_blowup, log_final, nqueries, log_arity, log_group, coset, c, open_challenges, w_final.data(), &work,
                                     open_round_polys, roots, final_table, query_values, query_paths, grinding_bits, pow_nonce, &open_ok));
    if (t) t->t = work.t;
    *ok = good && open_ok ? 1 : 0;
    return ZK_OK;
}

int zk_r1cs_last_stats(zk_r1cs_stats *out) {
    if (!out) return ZK_E_ARG;
    *out = g_r1cs_stats;
    return ZK_OK;
}

}  // extern "C"
