// r1cs_host.h -- the host side of an R1CS instance (include/zkmle.h "R1CS instance: sparse matrices times a table"): the checks of
// zk_r1cs_create, the entries sorted by (row, column), the digest, the compressed forms r1cs.cuh's kernels read and their bins.  All of it is
// preprocessing, done once per circuit on the host; the device copy is made when a device function first needs it, so a verifier holds an
// instance without a GPU.  Library-internal; included by .hip files only.
#pragma once
#include <mutex>
#include <vector>

#include "host_field.h"
#include "host_util.h"
#include "r1cs.cuh"
#include "transcript.h"
#include "zerocheck_host.h"

struct zk_r1cs {
    int field;
    unsigned s, d;                                            // 2^s rows, 2^d columns
    struct Matrix {                                           // sorted by (row, column)
        std::vector<uint32_t> row, col;
        std::vector<uint64_t> val;                            // 4 words an entry: the stored element
    } mat[3];
    uint8_t digest[32];
    // the forms of r1cs.cuh on the host: CSR over the items k 2^s + row, CSC over the items k 2^d + column; values as v R_u mod p
    std::vector<uint32_t> csr_off, csr_idx, csc_off, csc_idx;
    std::vector<uint64_t> csr_val, csc_val;
    // the bins, each ascending: rows by their own length, columns by their length in the three matrices together.  col_*_half = how many of
    // the list lie in the witness half y < 2^(d-1)
    std::vector<uint32_t> row_lane, row_block, col_lane, col_block;
    size_t col_lane_half = 0, col_block_half = 0;
    // the device copy: one block on the device that was current at the first pass; the host copies of the forms' values and indices are
    // dropped once it is made (mat[] stays: the digest's and the verifier's form)
    std::mutex mu;
    void *dev = nullptr;
    int device = -1;
    zk::R1csSparse dcsr{}, dcsc{};
    const uint32_t *d_row_lane = nullptr, *d_row_block = nullptr, *d_col_lane = nullptr, *d_col_block = nullptr;
    ~zk_r1cs() {
        if (dev) (void)hipFree(dev);
    }
};

namespace zk {
namespace host {

constexpr unsigned kR1csMaxLog = 28;                          // an item k 2^log + index fits 32 bits

// `keys[order[i]]` ascending after the call, equal keys in their order before it (one pass of a counting sort over nkeys keys)
inline void r1cs_counting_sort(const uint32_t *keys, size_t nkeys, std::vector<uint32_t> &order) {
    std::vector<size_t> at(nkeys + 1, 0);
    for (uint32_t e : order) at[keys[e] + 1]++;
    for (size_t k = 0; k < nkeys; k++) at[k + 1] += at[k];
    std::vector<uint32_t> out(order.size());
    for (uint32_t e : order) out[at[keys[e]]++] = e;
    order.swap(out);
}

// v R_std -> the 32-bit limbs of v R_u mod p (r1cs.cuh "values")
template <class F> void r1cs_value_for_scan(const uint64_t *stored, uint64_t *out) {
    store_host<F>(out, u_to_limbs32<F>(u_reduce_once<F>(u_from_std<F>(load_host<F>(stored)))));
}

// one matrix's checks and its entries sorted by (row, column); ZK_E_ARG for an index out of range, an unreduced value or a duplicate
inline int r1cs_sort_matrix(int field, unsigned s, unsigned d, const uint32_t *rows, const uint32_t *cols, const uint64_t *vals, size_t nnz, zk_r1cs::Matrix &m) {
    if (nnz && (!rows || !cols || !vals)) return ZK_E_ARG;
    for (size_t e = 0; e < nnz; e++)
        if (rows[e] >> s || cols[e] >> d) return ZK_E_ARG;
    if (!all_reduced(field, vals, nnz)) return ZK_E_ARG;
    std::vector<uint32_t> order(nnz);
    for (size_t e = 0; e < nnz; e++) order[e] = (uint32_t)e;
    r1cs_counting_sort(cols, (size_t)1 << d, order);
    r1cs_counting_sort(rows, (size_t)1 << s, order);
    m.row.resize(nnz);
    m.col.resize(nnz);
    m.val.resize(4 * nnz);
    for (size_t i = 0; i < nnz; i++) {
        const uint32_t e = order[i];
        m.row[i] = rows[e];
        m.col[i] = cols[e];
        memcpy(&m.val[4 * i], vals + 4 * (size_t)e, 32);
        if (i && m.row[i] == m.row[i - 1] && m.col[i] == m.col[i - 1]) return ZK_E_ARG;
    }
    return ZK_OK;
}

// Keccak-256 of "R1CSMAT", the field id, s and d (big-endian u32), then per matrix nnz (big-endian u64) and its sorted entries as row, column
// (big-endian u32) and the value's 32 canonical big-endian bytes
template <class F> void r1cs_digest(const zk_r1cs &in, uint8_t out[32]) {
    Keccak256 h;
    uint8_t head[7 + 12];
    memcpy(head, "R1CSMAT", 7);
    put_be32(head + 7, (uint32_t)in.field);
    put_be32(head + 11, in.s);
    put_be32(head + 15, in.d);
    h.update(head, sizeof head);
    for (const zk_r1cs::Matrix &m : in.mat) {
        uint8_t b[40];
        const uint64_t nnz = m.row.size();
        put_be32(b, (uint32_t)(nnz >> 32));
        put_be32(b + 4, (uint32_t)nnz);
        h.update(b, 8);
        for (size_t i = 0; i < nnz; i++) {
            put_be32(b, m.row[i]);
            put_be32(b + 4, m.col[i]);
            host_to_bytes_be<F>(load_host<F>(&m.val[4 * i]), b + 8);
            h.update(b, 40);
        }
    }
    h.finalize_copy(out);
}

// the compressed forms and the bins from the sorted entries
template <class F> void r1cs_compress(zk_r1cs &in) {
    const size_t R = (size_t)1 << in.s, Cn = (size_t)1 << in.d;
    size_t total = 0;
    for (const zk_r1cs::Matrix &m : in.mat) total += m.row.size();
    in.csr_off.assign(3 * R + 1, 0);
    in.csc_off.assign(3 * Cn + 1, 0);
    in.csr_idx.resize(total);
    in.csc_idx.resize(total);
    in.csr_val.resize(4 * total);
    in.csc_val.resize(4 * total);
    size_t base = 0;
    for (int k = 0; k < 3; k++) {
        const zk_r1cs::Matrix &m = in.mat[k];
        const size_t nnz = m.row.size();
        std::vector<uint32_t> by_col(nnz);
        for (size_t i = 0; i < nnz; i++) by_col[i] = (uint32_t)i;
        r1cs_counting_sort(m.col.data(), Cn, by_col);            // stable: rows ascending inside a column
        for (size_t i = 0; i < nnz; i++) {
            in.csr_off[k * R + m.row[i] + 1]++;
            in.csc_off[k * Cn + m.col[i] + 1]++;
            in.csr_idx[base + i] = m.col[i];
            r1cs_value_for_scan<F>(&m.val[4 * i], &in.csr_val[4 * (base + i)]);
        }
        for (size_t i = 0; i < nnz; i++) {
            in.csc_idx[base + i] = m.row[by_col[i]];
            memcpy(&in.csc_val[4 * (base + i)], &in.csr_val[4 * (base + by_col[i])], 32);
        }
        base += nnz;
    }
    for (size_t g = 0; g < 3 * R; g++) in.csr_off[g + 1] += in.csr_off[g];
    for (size_t g = 0; g < 3 * Cn; g++) in.csc_off[g + 1] += in.csc_off[g];
    for (size_t g = 0; g < 3 * R; g++) (in.csr_off[g + 1] - in.csr_off[g] > ZK_R1CS_ROW_SPLIT ? in.row_block : in.row_lane).push_back((uint32_t)g);
    for (size_t y = 0; y < Cn; y++) {
        size_t len = 0;
        for (size_t k = 0; k < 3; k++) len += in.csc_off[k * Cn + y + 1] - in.csc_off[k * Cn + y];
        if (y == Cn / 2) in.col_lane_half = in.col_lane.size(), in.col_block_half = in.col_block.size();
        (len > ZK_R1CS_ROW_SPLIT ? in.col_block : in.col_lane).push_back((uint32_t)y);
    }
}

// ---- the Spartan chain's host side (include/zkmle.h "R1CS satisfiability: Spartan over a FRI commitment"), shared by prover and verifier -------
// step 1 and 2: "R1CS" s d l, the digest, the witness commitment's root, pi_1 .. pi_l; then tau_0 .. tau_{s-1} (tau: s elements)
template <class F> void r1cs_statement(Transcript &tr, const zk_r1cs &in, const uint8_t *root32, const uint64_t *pub, uint32_t l, uint64_t *tau) {
    constexpr int W = F::N / 2;
    uint8_t head[16];
    memcpy(head, "R1CS", 4);
    put_be32(head + 4, in.s);
    put_be32(head + 8, in.d);
    put_be32(head + 12, l);
    tr.append(head, sizeof head);
    tr.append(in.digest, 32);
    tr.append(root32, 32);
    for (uint32_t i = 0; i < l; i++) tr.append_be<F>(load_host<F>(pub + (size_t)i * W));
    for (uint32_t i = 0; i < in.s; i++) store_host<F>(tau + (size_t)i * W, tr.random_challenge_as_field_element<F>());
}

// eq(point, x) for x < 2^n on the host; msb_first: point[0] is the most significant index bit, else the least
template <class F> std::vector<Fe<F>> r1cs_host_eq(const uint64_t *point, uint32_t n, bool msb_first) {
    constexpr int W = F::N / 2;
    std::vector<Fe<F>> t((size_t)1 << n);
    t[0] = fe_one<F>();
    for (uint32_t i = 0; i < n; i++) {                        // after step i the first 2^(i+1) entries hold the table of i + 1 variables
        const Fe<F> r = load_host<F>(point + (size_t)(msb_first ? i : n - 1 - i) * W);
        for (size_t x = (size_t)1 << i; x-- > 0;) {           // the new variable becomes the LEAST significant bit of the index so far
            const Fe<F> hi = fe_mul<F>(t[x], r);
            t[2 * x] = fe_sub<F>(t[x], hi);
            t[2 * x + 1] = hi;
        }
    }
    return t;
}

// c_pub = sum over the entries (x, y) with y >= 2^(d-1) of rho^k val eq(rx, x) xvec[y - 2^(d-1)], xvec = (1, pi_1 .. pi_l, 0, ..), and (w_final
// not null) w_final[j] = sum over the entries with y < 2^(d-1) and (y >> R) = j of rho^k val eq(rx, x) prod_{l<R} eq1(r_l, bit l of y), bit 0 the
// least significant; rs: the R opening challenges.  O(nnz + 2^s + 2^R) products
template <class F> void r1cs_public_terms(const zk_r1cs &in, const uint64_t *pub, uint32_t l, const uint64_t *rx, const Fe<F> &rho, const uint64_t *rs, uint32_t R,
                                          Fe<F> *c_pub, uint64_t *w_final) {
    constexpr int W = F::N / 2;
    const size_t half = (size_t)1 << (in.d - 1), m = half >> R, low = ((size_t)1 << R) - 1;
    const std::vector<Fe<F>> E = r1cs_host_eq<F>(rx, in.s, true);
    std::vector<Fe<F>> P, wf(w_final ? m : 0, fe_zero<F>());
    if (w_final) P = r1cs_host_eq<F>(rs, R, false);
    Fe<F> cp = fe_zero<F>(), w = fe_one<F>();
    for (const zk_r1cs::Matrix &mt : in.mat) {
        for (size_t i = 0; i < mt.row.size(); i++) {
            const size_t y = mt.col[i];
            const Fe<F> term = fe_mul<F>(w, fe_mul<F>(load_host<F>(&mt.val[4 * i]), E[mt.row[i]]));
            if (y >= half) {
                const size_t xi = y - half;
                if (xi == 0) cp = fe_add<F>(cp, term);
                else if (xi <= l) cp = fe_add<F>(cp, fe_mul<F>(term, load_host<F>(pub + (xi - 1) * W)));
            } else if (w_final) {
                wf[y >> R] = fe_add<F>(wf[y >> R], fe_mul<F>(term, P[y & low]));
            }
        }
        w = fe_mul<F>(w, rho);
    }
    *c_pub = cp;
    for (size_t j = 0; j < wf.size(); j++) store_host<F>(w_final + j * W, wf[j]);
}

// the verifier's replay up to the opening: *good = the zerocheck chain and c = va + rho vb + rho^2 vc - c_pub hold and everything read is
// reduced; w_final (2^f elements) for the opening's verifier.  vs: va, vb, vc.  The transcript advances the same way whatever *good is.
template <class F> void r1cs_replay(Transcript &tr, const zk_r1cs &in, const uint8_t *root32, const uint64_t *pub, uint32_t l, const uint64_t *round_polys,
                                    const uint64_t *vs, const uint64_t *c, const uint64_t *open_challenges, uint32_t R, uint64_t *w_final, bool *good) {
    constexpr int W = F::N / 2;
    std::vector<uint64_t> tau((size_t)in.s * W), rx((size_t)in.s * W);
    bool ok = all_reduced(in.field, pub, l) && all_reduced(in.field, open_challenges, R) && is_reduced<F>(c);
    r1cs_statement<F>(tr, in, root32, pub, l, tau.data());
    const Fe<F> last = replay_rounds<F, ZerocheckMul::NODES>(tr, in.s, fe_zero<F>(), round_polys, rx.data(), ok);
    Fe<F> v[3];
    load_claims<F>(vs, 3, v, ok);
    ok = ok && fe_eq<F>(last, fe_mul<F>(eq_at<F>(rx.data(), tau.data(), in.s), ZerocheckMul::relation<F>(v)));
    for (int k = 0; k < 3; k++) tr.append_be<F>(v[k]);
    const Fe<F> rho = tr.random_challenge_as_field_element<F>();
    Fe<F> c_pub;
    if (ok) r1cs_public_terms<F>(in, pub, l, rx.data(), rho, open_challenges, R, &c_pub, w_final);
    else c_pub = fe_zero<F>();
    const Fe<F> want = fe_sub<F>(fe_add<F>(v[0], fe_mul<F>(rho, fe_add<F>(v[1], fe_mul<F>(rho, v[2])))), c_pub);
    *good = ok && fe_eq<F>(want, load_host<F>(c));
}

// the device copy of the forms and bins, made once: values first (16-byte loads), then the 32-bit arrays.  A handle belongs to the device of
// its first pass: ZK_E_ARG when another one is current
inline int r1cs_upload(zk_r1cs &in) {
    std::lock_guard<std::mutex> lock(in.mu);
    int cur = 0;
    ZK_HIP(hipGetDevice(&cur));
    if (in.dev) return in.device == cur ? ZK_OK : ZK_E_ARG;
    const std::vector<uint64_t> *vals[2] = {&in.csr_val, &in.csc_val};
    const std::vector<uint32_t> *words[8] = {&in.csr_off, &in.csr_idx, &in.csc_off, &in.csc_idx, &in.row_lane, &in.row_block, &in.col_lane, &in.col_block};
    size_t bytes = 0, at[10];
    for (int j = 0; j < 2; j++) { at[j] = bytes; bytes += (vals[j]->size() * 8 + 15) / 16 * 16; }
    for (int j = 0; j < 8; j++) { at[2 + j] = bytes; bytes += (words[j]->size() * 4 + 15) / 16 * 16; }
    void *blk = nullptr;
    ZK_HIP(hipMalloc(&blk, bytes ? bytes : 16));
    hipError_t e = hipSuccess;
    for (int j = 0; j < 2 && e == hipSuccess; j++)
        if (!vals[j]->empty()) e = hipMemcpy((char *)blk + at[j], vals[j]->data(), vals[j]->size() * 8, hipMemcpyHostToDevice);
    for (int j = 0; j < 8 && e == hipSuccess; j++)
        if (!words[j]->empty()) e = hipMemcpy((char *)blk + at[2 + j], words[j]->data(), words[j]->size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(blk);
        ZK_HIP(e);
    }
    const auto w = [&](int j) { return (const uint32_t *)((char *)blk + at[2 + j]); };
    in.dcsr = R1csSparse{w(0), w(1), (char *)blk + at[0]};
    in.dcsc = R1csSparse{w(2), w(3), (char *)blk + at[1]};
    in.d_row_lane = w(4);
    in.d_row_block = w(5);
    in.d_col_lane = w(6);
    in.d_col_block = w(7);
    in.dev = blk;
    in.device = cur;
    for (std::vector<uint64_t> *v : {&in.csr_val, &in.csc_val}) std::vector<uint64_t>().swap(*v);
    for (std::vector<uint32_t> *v : {&in.csr_idx, &in.csc_idx}) std::vector<uint32_t>().swap(*v);
    return ZK_OK;
}

}  // namespace host
}  // namespace zk
