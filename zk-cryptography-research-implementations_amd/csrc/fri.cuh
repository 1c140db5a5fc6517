// fri.cuh -- kernels of the FRI low-degree prover (include/zkmle.h "FRI"): the fold of a codeword in half and the gather of every
// query's opened values and authentication paths.  The trees are merkle.cuh's (built by zkmle_merkle.hip: its kernels are not templates and
// live in that translation unit alone), the domain powers ntt.cuh's two-level tables.
//
//   fold    g[k] = (f[k] + f[k + h]) / 2 + beta (f[k] - f[k + h]) / (2 c w^k),  k < h = len / 2, on the domain {c w^k}
//
// Per output: two contiguous 32-byte reads and one write (the traffic of mle_kernels.cuh fold0_kernel) and
//   - the halving of the sum as an add of p (when odd) and a shift: no product;
//   - w^-k from the tables of w_N^-1 of the WHOLE proof (base^lo as 29-bit limbs, base^(4096 hi)), indexed with k << layer: one product
//     once the domain is longer than 2 x 4096 entries, a table read below;
//   - (f[k] - f[k + h]) w^-k: one product by that multiplier;
//   - beta / (2 c), the same for every lane, as a uniform multiplier (ufield.cuh UniMul: 81 words of the kernel's arguments, scalar
//     registers): 99 multiply-adds instead of a scan's 162, and the sum with the halved term comes out of the same two reduction rows.
// Every result is canonical, so the table is the one a big-integer model gives, byte for byte.
#pragma once
#include "ntt.cuh"

namespace zk {

constexpr int kFriBlock = 256;
constexpr unsigned kFriMaxLayers = 32;                       // the largest two-adicity: no proof commits more layers

// the rows of a UniMul of a nine-limb field, as a kernel argument
struct FriUni {
    uint32_t t[81];
};

// x / 2 for a canonical x: (x + p) / 2 when x is odd; p < 2^(32 N - 1), so the sum fits the limbs
template <class F> ZK_HD Fe<F> fe_halve(const Fe<F> &x) {
    const uint32_t mask = 0u - (x.l[0] & 1u);
    Fe<F> s;
    unsigned c = 0;
#pragma unroll
    for (int i = 0; i < F::N; i++) s.l[i] = __builtin_addc(x.l[i], F::p(i) & mask, c, &c);
#pragma unroll
    for (int i = 0; i < F::N; i++) s.l[i] = (s.l[i] >> 1) | (i + 1 < F::N ? s.l[i + 1] << 31 : 0u);
    return s;
}

// a + r t for the uniform multiplier r: ufold's columns (ufield.cuh) with the digits of t in place of those of a difference.  a, t:
// normalized limbs of canonical elements.  Output: normalized limbs of a value congruent to a + r t, below a + p (1 + 2^-24).
template <class F> ZK_HD Ufe<F> uni_muladd(const UniMul<F> &m, const Ufe<F> &a, const Ufe<F> &t) {
    constexpr int L = UParams<F>::L;
    uint64_t T[L];
    T[0] = 0;
    T[1] = 0;
#pragma unroll
    for (int j = 2; j < L; j++) T[j] = a.l[j - 2];
#pragma unroll
    for (int i = 0; i < L; i++) {
#pragma unroll
        for (int j = 0; j < L; j++) T[j] += (uint64_t)t.l[i] * m.t[i][j];
    }
#pragma unroll
    for (int row = 0; row < 2; row++) {
        const uint32_t q = ((uint32_t)T[0] * UParams<F>::INV) & UMASK;
#pragma unroll
        for (int j = 0; j < L; j++) T[j] += (uint64_t)q * UParams<F>::p(j);
        const uint64_t carry = T[0] >> UB;
#pragma unroll
        for (int j = 0; j + 1 < L; j++) T[j] = T[j + 1];
        T[L - 1] = a.l[L - 2 + row];
        T[0] += carry;
    }
    return u_normalize_columns<F>(T);
}

// pw_lo / pw_hi: the powers of w_N^-1 (ntt_pow2t), N = the proof's first domain; this layer's w^-k is entry k << shift.  g = beta / (2 c).
template <class F> __global__ void __launch_bounds__(kFriBlock) fri_fold_kernel(const void *__restrict__ in, void *__restrict__ out, size_t half,
                                                                               const void *__restrict__ pw_lo, const void *__restrict__ pw_hi,
                                                                               unsigned shift, FriUni g) {
    constexpr int L = UParams<F>::L;
    static_assert(L * L == 81, "FriUni holds the rows of a nine-limb field");
    const size_t k = (size_t)blockIdx.x * kFriBlock + threadIdx.x;
    if (k >= half) return;
    UniMul<F> m;
#pragma unroll
    for (int i = 0; i < L; i++) {
#pragma unroll
        for (int j = 0; j < L; j++) m.t[i][j] = g.t[i * L + j];
    }
    const Fe<F> a = fe_load<F>(in, k), b = fe_load<F>(in, k + half);
    const Fe<F> s = fe_halve<F>(fe_add<F>(a, b));
    const Fe<F> t = fe_mul_u_pre<F>(ntt_pow2t<F>(pw_lo, pw_hi, (uint64_t)k << shift), fe_sub<F>(a, b));
    fe_store<F>(out, k, fe_from_u_below_2p<F>(uni_muladd<F>(m, u_from_limbs32<F>(s), u_from_limbs32<F>(t))));
}

// The committed layers of one proof: layer l has len0 >> l entries; its tree holds every level as zk_merkle_build lays them out (level
// v at digest offset 2 len - (2 len >> v)).  path_off[l] = digests of one query's answer before layer l (2 (log_len0 - l') for each l' < l).
// `wide` != 0 (the multilinear opening folded by 4, fri_ml.cuh): the nlayers entries are STEPS; step s opens 2^log_sides[s] entries of a
// layer of 2^log_len[s] entries, a part = len >> log_sides apart; val_off[s] = values of one query's answer before step s, path_off[s] its
// digests (2^log_sides paths of log_len digests per step).  wide == 0: step s is layer s with two sides and the three arrays are not read.
// `grouped` != 0 (needs wide): step s's tree has len >> log_sides leaves, leaf j over the step's sides (merkle_leaf_group_kernel), and the
// answer holds ONE path of log_len - log_sides digests per step.
struct FriLayers {
    const void *table[kFriMaxLayers];
    const uint64_t *tree[kFriMaxLayers];
    uint32_t path_off[kFriMaxLayers + 1];
    uint32_t log_len0, nlayers;
    uint32_t wide, grouped;
    uint32_t val_off[kFriMaxLayers + 1];
    uint8_t log_len[kFriMaxLayers], log_sides[kFriMaxLayers];
};

// every opened value with one launch: out[(q R + l) 2 + side] = f_l[(i_q mod len_l / 2) + side len_l / 2]; wide: out[q per + val_off[s] + side]
template <class F> __global__ void __launch_bounds__(kFriBlock) fri_query_values_kernel(FriLayers a, const uint64_t *__restrict__ indices, size_t nq,
                                                                                       void *__restrict__ out) {
    const size_t per = a.wide ? a.val_off[a.nlayers] : 2 * (size_t)a.nlayers, total = nq * per, stride = (size_t)gridDim.x * kFriBlock;
    for (size_t t = (size_t)blockIdx.x * kFriBlock + threadIdx.x; t < total; t += stride) {
        const size_t q = t / per;
        const uint32_t r = (uint32_t)(t % per);
        unsigned l = r >> 1, side = r & 1, depth = a.log_len0 - l, ls = 1;
        if (a.wide) {
            l = 0;
            while (l + 1 < a.nlayers && a.val_off[l + 1] <= r) l++;
            side = r - a.val_off[l];
            depth = a.log_len[l];
            ls = a.log_sides[l];
        }
        const size_t part = ((size_t)1 << depth) >> ls;
        fe_store<F>(out, t, fe_load<F>(a.table[l], (indices[q] & (part - 1)) + side * part));
    }
}

// every authentication path with one launch (merkle_open_kernel over the layers): per query and layer the low entry's path, then the
// high entry's, log_len0 - l digests each, the leaf's sibling first; wide: per step the 2^log_sides paths in the order of the sides;
// grouped: per step the one path of leaf j = i_q mod part in the tree of `part` leaves
static __global__ void __launch_bounds__(kFriBlock) fri_query_paths_kernel(FriLayers a, const uint64_t *__restrict__ indices, size_t nq, uint64_t *__restrict__ paths) {
    const uint32_t per = a.path_off[a.nlayers];
    const size_t total = nq * per, stride = (size_t)gridDim.x * kFriBlock;
    for (size_t t = (size_t)blockIdx.x * kFriBlock + threadIdx.x; t < total; t += stride) {
        const size_t q = t / per;
        const uint32_t r = (uint32_t)(t % per);
        unsigned l = 0;
        while (l + 1 < a.nlayers && a.path_off[l + 1] <= r) l++;
        if (a.grouped) {
            const size_t part = ((size_t)1 << a.log_len[l]) >> a.log_sides[l];
            const unsigned v = r - a.path_off[l];
            const uint4 *src = reinterpret_cast<const uint4 *>(a.tree[l]) + 2 * (2 * part - ((2 * part) >> v) + (((indices[q] & (part - 1)) >> v) ^ 1));
            uint4 *dst = reinterpret_cast<uint4 *>(paths) + 2 * t;
            const uint4 d0 = src[0], d1 = src[1];
            dst[0] = d0;
            dst[1] = d1;
            continue;
        }
        const unsigned depth = a.wide ? a.log_len[l] : a.log_len0 - l, side = (r - a.path_off[l]) / depth, v = (r - a.path_off[l]) % depth;
        const size_t len = (size_t)1 << depth, part = len >> (a.wide ? a.log_sides[l] : 1);
        const size_t pos = (indices[q] & (part - 1)) + side * part;
        const uint4 *src = reinterpret_cast<const uint4 *>(a.tree[l]) + 2 * (2 * len - ((2 * len) >> v) + ((pos >> v) ^ 1));   // a digest: 32 bytes
        uint4 *dst = reinterpret_cast<uint4 *>(paths) + 2 * t;
        const uint4 d0 = src[0], d1 = src[1];
        dst[0] = d0;
        dst[1] = d1;
    }
}

}  // namespace zk
