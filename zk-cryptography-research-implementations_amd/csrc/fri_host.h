// fri_host.h -- host code shared by the translation units of the FRI family (zkmle_fri.hip, zkmle_fri_pcs.hip, zkmle_fri_ml.hip), beside
// host_util.h's holders and loaders: the field dispatch, the domain's roots, the power tables of the fold, the transcript's header and index
// sampling, the step schedule of a proof, and the query phase.  Library-internal; included by .hip files only.
#pragma once
#include "fri.cuh"
#include "host_util.h"
#include "transcript.h"

namespace zk {
namespace host {

// the two scalar fields: the only ones with a domain (every shape of the Fq fields is out of range)
#define FRI_DISPATCH(field_id, ...)                                        \
    switch (field_id) {                                                    \
        case ZK_FR381: { using F = ::zk::Fr381; __VA_ARGS__; } break;      \
        case ZK_BN254_FR: { using F = ::zk::Bn254Fr; __VA_ARGS__; } break; \
        default: return ZK_E_RANGE;                                        \
    }

inline unsigned two_adicity(int field) {
    uint32_t s = 0;
    return zk_ntt_two_adicity(field, &s) == ZK_OK ? s : 0;
}
// w_{2^log_n}; log_n within the field's two-adicity
template <class F> Fe<F> root_of_unity(unsigned log_n) {
    uint64_t w[F::N / 2];
    (void)zk_ntt_root_of_unity(F::ID, log_n, w);
    return load_host<F>(w);
}
// the statuses of one fold of `cw` by 2^log_arity on its own, up to the device check; `args`: the caller's other pointers are all there
inline int fold_check(const zk_table *cw, bool args, const uint64_t *coset, unsigned log_arity) {
    if (!cw || !args || field_limbs64(cw->field) < 0 || cw->len == 1 || (log_arity == 2 && cw->len == 2)) return ZK_E_ARG;
    if (coset && is_zero_element(cw->field, coset)) return ZK_E_ARG;
    if (!is_pow2(cw->len)) return ZK_E_NOT_POW2;
    if ((cw->field != ZK_FR381 && cw->field != ZK_BN254_FR) || ilog2(cw->len) > two_adicity(cw->field)) return ZK_E_RANGE;
    return require_device();
}

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
// a fold's uniform multiplier as the kernels take it
template <class F> FriUni fri_uni(const Fe<F> &gamma) {
    UniMul<F> um;
    unimul_from<F>(um, gamma);
    FriUni g;
    memcpy(g.t, um.t, sizeof g.t);
    return g;
}

inline void transcript_header(Transcript &tr, uint32_t d, uint32_t b, uint32_t f, uint32_t Q, const uint8_t coset_be[32]) {
    uint8_t hdr[48];
    put_be32(hdr, d);
    put_be32(hdr + 4, b);
    put_be32(hdr + 8, f);
    put_be32(hdr + 12, Q);
    memcpy(hdr + 16, coset_be, 32);
    tr.append(hdr, sizeof hdr);
}
// i_q = the little-endian integer of a sampled digest mod 2^bits, bits <= 31
inline uint64_t sample_index(Transcript &tr, unsigned bits) {
    uint8_t dg[32];
    tr.sample_random_challenge(dg);
    uint64_t v = 0;
    for (int k = 0; k < 8; k++) v |= (uint64_t)dg[k] << (8 * k);
    return v & (((uint64_t)1 << bits) - 1);
}

// ---- the step schedule ---------------------------------------------------------------------------------------------------------
// What a query opens, for a proof of R folds over a layer 0 of 2^L entries: one source for the sizes, the provers' FriLayers and the
// verifier.  log_arity 1: a step per layer l < R, two sides.  2 (R >= 2): a step per even layer, four sides where layer l + 2 <= R exists
// (a fold by 4), else (R odd, l = R - 1) two (the fold by 2 to layer R).  A step's sides are its layer's entries j + side (len >> log_sides),
// j = i_q mod (len >> log_sides); one query's answer holds the steps' values, and their paths of log_len digests, one after the other.
// `grouped` (log_arity 2 only): every layer's tree has a leaf per j over the step's sides (merkle.cuh), so a step has ONE path, of
// log_len - log_sides digests.
struct FriStep {
    unsigned layer, log_len, log_sides, root;                 // the layer opened, its log2 length, of its sides, the index of its root
    size_t val_off, path_off;                                 // values and digests of one query's answer before this step
};
struct FriSchedule {
    unsigned log_arity, nsteps = 0;
    bool grouped;
    size_t nvalues = 0, ndigests = 0;                         // of one query's answer
    FriStep step[kFriMaxLayers];
    FriSchedule(unsigned L, unsigned R, unsigned log_arity_, bool grouped_ = false) : log_arity(log_arity_), grouped(grouped_) {
        for (unsigned l = 0; l < R; l += log_arity) {
            const unsigned ls = l + log_arity <= R ? log_arity : 1;
            step[nsteps] = FriStep{l, L - l, ls, nsteps, nvalues, ndigests};
            nvalues += (size_t)1 << ls;
            ndigests += grouped ? (size_t)L - l - ls : ((size_t)L - l) << ls;
            nsteps++;
        }
    }
    unsigned leaf_group(unsigned s) const { return grouped ? step[s].log_sides : 0; }   // the log_group of step s's tree
    unsigned index_bits() const { return step[0].log_len - log_arity; }   // every i_q is a position of the first step's part
    // the gather kernels' view of the steps first .. first + count - 1 (all of them by default; first < nsteps), offsets counted from step
    // `first`; the caller adds each step's table and tree.  wide stays 0 at arity 1: its three arrays are not read then, and step s is layer
    // s, whose length the kernels take from log_len0
    FriLayers layers(unsigned first = 0, unsigned count = kFriMaxLayers) const {
        if (count > nsteps - first) count = nsteps - first;
        const unsigned end = first + count;
        const size_t v0 = step[first].val_off, d0 = step[first].path_off;
        FriLayers fl{};
        fl.log_len0 = step[first].log_len;
        fl.nlayers = count;
        fl.wide = log_arity == 2;
        fl.grouped = grouped;
        for (unsigned s = 0; s < count; s++) {
            fl.path_off[s] = (uint32_t)(step[first + s].path_off - d0);
            if (!fl.wide) continue;
            fl.val_off[s] = (uint32_t)(step[first + s].val_off - v0);
            fl.log_len[s] = (uint8_t)step[first + s].log_len;
            fl.log_sides[s] = (uint8_t)step[first + s].log_sides;
        }
        fl.path_off[count] = (uint32_t)((end < nsteps ? step[end].path_off : ndigests) - d0);
        if (fl.wide) fl.val_off[count] = (uint32_t)((end < nsteps ? step[end].val_off : nvalues) - v0);
        return fl;
    }
};

// where every prover draws its Q indices.  grind_bits > 0: the proof-of-work step comes first (include/zkmle.h "Proof-of-work grinding";
// the search runs on the GPU, zkmle_grind.hip) and *nonce_out, which is required then, receives its nonce
inline int draw_indices(Transcript &tr, const FriSchedule &sc, uint32_t Q, std::vector<uint64_t> &idx, uint32_t grind_bits, uint64_t *nonce_out) {
    if (grind_bits) ZK_TRY(transcript_grind(tr, grind_bits, 0, 0, nonce_out));
    idx.resize(Q);
    for (unsigned q = 0; q < Q; q++) idx[q] = sample_index(tr, sc.index_bits());
    return ZK_OK;
}

// the queries: Q indices from the transcript, then every opened value and path of the steps of `fl` (= sc.layers() with its tables and
// trees) with one launch each, one download each and one wait for both.  *ms (may be null) = the gather with its downloads; ends with the stream drained and its end as the latest event.
template <class F> int answer_queries(Transcript &tr, const FriLayers &fl, const FriSchedule &sc, uint32_t Q, uint64_t *indices_out, uint64_t *values,
                                      uint8_t *paths, Events &ev, float *ms, uint32_t grind_bits = 0, uint64_t *nonce_out = nullptr) {
    constexpr size_t ESZ = sizeof(Fe<F>);
    std::vector<uint64_t> idx;
    ZK_TRY(draw_indices(tr, sc, Q, idx, grind_bits, nonce_out));
    if (indices_out) memcpy(indices_out, idx.data(), Q * 8);
    const size_t nval = (size_t)Q * sc.nvalues, ndig = (size_t)Q * sc.ndigests;
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
    ZK_HIP(hipMemcpyAsync(values, dval.p, nval * ESZ, hipMemcpyDeviceToHost, cur_stream()));
    ZK_HIP(zk::memcpy_on_stream(paths, dpath.p, ndig * 32, hipMemcpyDeviceToHost));
    ZK_TRY(ev.mark(&q1));
    ZK_HIP(hipEventSynchronize(ev.ev[q1]));
    if (ms) *ms = ev.ms(q0, q1);
    return ZK_OK;
}

}  // namespace host
}  // namespace zk
