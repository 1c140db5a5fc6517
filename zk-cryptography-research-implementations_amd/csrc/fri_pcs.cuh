// fri_pcs.cuh -- kernels of the evaluation opening of FRI-committed polynomials (include/zkmle.h "FRI polynomial commitment"): the
// evaluation of a coefficient table at a point, the DEEP quotient of k codewords, and the gather of the opened values and paths.
//
//   evaluate   y = sum_i a_i z^i.  A lane runs Horner over kPcsEvalRun contiguous coefficients and scales by z^(run start), read from
//              the two-level power table of z (ntt.cuh: base^lo as 29-bit limbs, base^(4096 hi)); the lanes' terms are summed in LDS, the
//              blocks' sums by a second one-block launch.  Field addition is exact: the order of the sum does not show.
//   quotient   q[i] = (sum_j gamma^j f_j[i] - sum_j gamma^j y_j) / (c w^i - z), one pass: k reads and one write per entry.
//              - the numerator by Horner in gamma, f_0 + gamma (f_1 + gamma (f_2 + ..)): ONE uniform multiplier (ufield.cuh UniMul, 81
//                words of the kernel's arguments) whatever k is, a uni_muladd (fri.cuh) per further polynomial; the constant is folded
//                by the host;
//              - c w^i from the forward power tables (lo = c w^e, hi = w^(4096 h)): one product above 4096 entries, a table read below;
//              - the N inverses by Montgomery's trick per lane: a lane takes the T entries base + 256 t of its block's tile of 256 T (every
//                access of a wave is contiguous), keeps the prefix products d_0 .. d_t in registers (T <= 8) or parks them in the output
//                table, which nobody else reads (T = 16), inverts the full product once by Fermat (255 squarings, the multiplications of
//                p - 2: the exponent's bits are compile-time constants and the same for every lane) and walks back.  3 (T - 1) products
//                and one inversion per T entries.  Slots past the table's end count as the denominator 1.
//              Every product ends canonical, so q is the table of the big-integer model whatever T is.
//   gather     out[((q 2 + s) k + j)] = f_j[i_q + s N / 2] and its L digests of tree j, the leaf's sibling first (fri.cuh's query
//              kernels over k trees of one depth): one launch each.
#pragma once
#include <utility>

#include "fri.cuh"

namespace zk {

constexpr int kPcsBlock = 256;
constexpr unsigned kPcsEvalRun = 8;                          // coefficients per lane and Horner run: 256 contiguous bytes
constexpr unsigned kPcsEvalMaxBlocks = 512;                  // partial sums the second launch adds
constexpr unsigned kPcsMaxPolys = 64;
constexpr int kPcsMemBatch = 16;                             // T of the variant that parks its prefix products in the output table

struct PcsTables {
    const void *cw[kPcsMaxPolys];
};
struct PcsTrees {
    const void *cw[kPcsMaxPolys];
    const uint64_t *tree[kPcsMaxPolys];                      // zk_merkle_build's layout: level v at digest offset 2 N - (2 N >> v)
};

// fn(integral_constant<int, 0>) .. fn(integral_constant<int, N - 1>): a loop hipcc cannot leave rolled (a rolled one would index the
// register array of prefix products at run time, which sends it to scratch memory)
template <int... Is, class Fn> __device__ __forceinline__ void pcs_static_for(std::integer_sequence<int, Is...>, Fn &&fn) {
    (fn(std::integral_constant<int, Is>{}), ...);
}

// the block's sum of one element per lane, in lane 0
template <class F> __device__ __forceinline__ Fe<F> pcs_block_sum(Fe<F> v, Fe<F> *sh) {
    const unsigned tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (unsigned st = kPcsBlock / 2; st; st >>= 1) {
        if (tid < st) sh[tid] = fe_add<F>(sh[tid], sh[tid + st]);
        __syncthreads();
    }
    return sh[0];
}

// partials[block] = the sum over the block's runs of z^s Horner(a[s .. s + run), z); pw_lo / pw_hi: the powers of z below n (ntt_pow2t)
template <class F> __global__ void __launch_bounds__(kPcsBlock) pcs_eval_kernel(const void *__restrict__ coeffs, size_t n, const void *__restrict__ pw_lo,
                                                                               const void *__restrict__ pw_hi, Fe<F> z, void *__restrict__ partials) {
    __shared__ Fe<F> sh[kPcsBlock];
    const Ufe<F> zu = u_from_limbs32<F>(z);
    const size_t nruns = (n + kPcsEvalRun - 1) / kPcsEvalRun, stride = (size_t)gridDim.x * kPcsBlock;
    Fe<F> sum = fe_zero<F>();
    for (size_t r = (size_t)blockIdx.x * kPcsBlock + threadIdx.x; r < nruns; r += stride) {
        const size_t s = r * kPcsEvalRun, e = s + kPcsEvalRun < n ? s + kPcsEvalRun : n;
        Fe<F> acc = fe_load<F>(coeffs, e - 1);
        for (size_t j = e - 1; j-- > s;) acc = fe_add<F>(fe_mul_u_pre<F>(zu, acc), fe_load<F>(coeffs, j));
        if (s) acc = fe_mul_u_pre<F>(ntt_pow2t<F>(pw_lo, pw_hi, s), acc);
        sum = fe_add<F>(sum, acc);
    }
    sum = pcs_block_sum<F>(sum, sh);
    if (threadIdx.x == 0) fe_store<F>(partials, blockIdx.x, sum);
}
// out[slot] = the sum of `count` partials (one block)
template <class F> __global__ void __launch_bounds__(kPcsBlock) pcs_eval_finish_kernel(const void *__restrict__ partials, unsigned count, void *__restrict__ out,
                                                                                      unsigned slot) {
    __shared__ Fe<F> sh[kPcsBlock];
    Fe<F> sum = fe_zero<F>();
    for (unsigned j = threadIdx.x; j < count; j += kPcsBlock) sum = fe_add<F>(sum, fe_load<F>(partials, j));
    sum = pcs_block_sum<F>(sum, sh);
    if (threadIdx.x == 0) fe_store<F>(out, slot, sum);
}

// a^(p - 2), a != 0, left to right: the outer loop is unrolled, so a limb of the exponent is a constant and every branch is uniform
template <class F> __device__ __forceinline__ Fe<F> pcs_inverse(const Fe<F> &a) {
    const Ufe<F> au = u_from_limbs32<F>(a);
    Fe<F> acc = fe_one<F>();
#pragma unroll
    for (int i = F::N - 1; i >= 0; i--) {
        uint32_t e = F::p(i), borrow = 2;                    // limb i of p - 2
#pragma unroll
        for (int k = 0; k <= i; k++) {
            const uint32_t pk = F::p(k);
            e = pk - borrow;
            borrow = pk < borrow ? 1u : 0u;
        }
#pragma unroll 1
        for (int bit = 31; bit >= 0; bit--) {
            acc = fe_mul_u<F>(acc, acc);
            if ((e >> bit) & 1u) acc = fe_mul_u_pre<F>(au, acc);
        }
    }
    return acc;
}

// c w^i, canonical: x_lo[e] = c w^e as 29-bit limbs (e < 4096 or the whole domain), x_hi[h] = w^(4096 h) (null when the domain fits x_lo)
template <class F> __device__ __forceinline__ Fe<F> pcs_domain_point(const void *x_lo, const void *x_hi, size_t i) {
    const Ufe<F> l = reinterpret_cast<const Ufe<F> *>(x_lo)[i & ((1u << kNttLoBits) - 1)];
    if (!x_hi) return u_to_limbs32<F>(l);
    return fe_mul_u_pre<F>(l, fe_load<F>(x_hi, i >> kNttLoBits));
}

// sum_j gamma^j f_j[i] - csum, canonical; g = the rows of gamma's UniMul
template <class F> __device__ __forceinline__ Fe<F> pcs_numerator(const PcsTables &tb, unsigned k, size_t i, const UniMul<F> &m, const Fe<F> &csum) {
    Fe<F> acc = fe_load<F>(tb.cw[k - 1], i);
    for (unsigned j = k - 1; j-- > 0;)
        acc = fe_from_u_below_2p<F>(uni_muladd<F>(m, u_from_limbs32<F>(fe_load<F>(tb.cw[j], i)), u_from_limbs32<F>(acc)));
    return fe_sub<F>(acc, csum);
}

// T entries per lane; MEM: the prefix products wait in out[] instead of registers.  z is outside the domain: no denominator is zero.
template <class F, int T, bool MEM> __global__ void __launch_bounds__(kPcsBlock) pcs_quotient_kernel(PcsTables tb, unsigned k, void *__restrict__ out, size_t n,
                                                                                                    const void *__restrict__ x_lo, const void *__restrict__ x_hi,
                                                                                                    Fe<F> z, Fe<F> csum, FriUni g) {
    constexpr int L = UParams<F>::L;
    static_assert(L * L == 81, "FriUni holds the rows of a nine-limb field");
    const size_t base = (size_t)blockIdx.x * (T * kPcsBlock) + threadIdx.x;
    if (base >= n) return;
    UniMul<F> m;
#pragma unroll
    for (int i = 0; i < L; i++) {
#pragma unroll
        for (int j = 0; j < L; j++) m.t[i][j] = g.t[i * L + j];
    }
    Fe<F> pre[MEM ? 1 : T];
    Fe<F> acc = fe_sub<F>(pcs_domain_point<F>(x_lo, x_hi, base), z);
    if (MEM) fe_store<F>(out, base, acc); else pre[0] = acc;
    if (MEM) {
#pragma unroll 1
        for (int t = 1; t < T; t++) {
            const size_t i = base + (size_t)t * kPcsBlock;
            if (i >= n) break;
            acc = fe_mul_u<F>(acc, fe_sub<F>(pcs_domain_point<F>(x_lo, x_hi, i), z));
            fe_store<F>(out, i, acc);
        }
    } else {
        pcs_static_for(std::make_integer_sequence<int, T - 1>{}, [&](auto tc) {
            constexpr int t = decltype(tc)::value + 1;
            const size_t i = base + (size_t)t * kPcsBlock;
            if (i < n) acc = fe_mul_u<F>(acc, fe_sub<F>(pcs_domain_point<F>(x_lo, x_hi, i), z));
            pre[MEM ? 0 : t] = acc;
        });
    }
    Fe<F> inv = pcs_inverse<F>(acc);                         // 1 / (d_0 .. d_t') for the last valid slot t'
    if (MEM) {
#pragma unroll 1
        for (int t = T - 1; t >= 1; t--) {
            const size_t i = base + (size_t)t * kPcsBlock;
            if (i >= n) continue;
            const Fe<F> dinv = fe_mul_u<F>(inv, fe_load<F>(out, i - kPcsBlock));
            fe_store<F>(out, i, fe_mul_u<F>(pcs_numerator<F>(tb, k, i, m, csum), dinv));
            inv = fe_mul_u<F>(inv, fe_sub<F>(pcs_domain_point<F>(x_lo, x_hi, i), z));
        }
    } else {
        pcs_static_for(std::make_integer_sequence<int, T - 1>{}, [&](auto tc) {
            constexpr int t = T - 1 - decltype(tc)::value;
            const size_t i = base + (size_t)t * kPcsBlock;
            if (i < n) {
                const Fe<F> dinv = fe_mul_u<F>(inv, pre[MEM ? 0 : t - 1]);
                fe_store<F>(out, i, fe_mul_u<F>(pcs_numerator<F>(tb, k, i, m, csum), dinv));
                inv = fe_mul_u<F>(inv, fe_sub<F>(pcs_domain_point<F>(x_lo, x_hi, i), z));
            }
        });
    }
    fe_store<F>(out, base, fe_mul_u<F>(pcs_numerator<F>(tb, k, base, m, csum), inv));
}

// every opened value with one launch: out[(q 2 + s) k + j] = f_j[i_q + s n / 2]
template <class F> __global__ void __launch_bounds__(kPcsBlock) pcs_open_values_kernel(PcsTrees a, unsigned k, size_t n, const uint64_t *__restrict__ indices,
                                                                                      size_t nq, void *__restrict__ out) {
    const size_t total = nq * 2 * k, stride = (size_t)gridDim.x * kPcsBlock;
    for (size_t t = (size_t)blockIdx.x * kPcsBlock + threadIdx.x; t < total; t += stride) {
        const unsigned j = (unsigned)(t % k);
        const size_t qs = t / k;
        fe_store<F>(out, t, fe_load<F>(a.cw[j], (indices[qs >> 1] & (n / 2 - 1)) + (qs & 1) * (n / 2)));
    }
}
// every authentication path with one launch: per (q, s, j) the `depth` digests of tree j above entry i_q + s n / 2, the leaf's sibling first
static __global__ void __launch_bounds__(kPcsBlock) pcs_open_paths_kernel(PcsTrees a, unsigned k, unsigned depth, const uint64_t *__restrict__ indices, size_t nq,
                                                                  uint64_t *__restrict__ paths) {
    const size_t n = (size_t)1 << depth, total = nq * 2 * k * depth, stride = (size_t)gridDim.x * kPcsBlock;
    for (size_t t = (size_t)blockIdx.x * kPcsBlock + threadIdx.x; t < total; t += stride) {
        const unsigned v = (unsigned)(t % depth);
        const size_t e = t / depth, qs = e / k;
        const unsigned j = (unsigned)(e % k);
        const size_t pos = (indices[qs >> 1] & (n / 2 - 1)) + (qs & 1) * (n / 2);
        const uint4 *src = reinterpret_cast<const uint4 *>(a.tree[j]) + 2 * (2 * n - ((2 * n) >> v) + ((pos >> v) ^ 1));   // a digest: 32 bytes
        uint4 *dst = reinterpret_cast<uint4 *>(paths) + 2 * t;
        const uint4 d0 = src[0], d1 = src[1];
        dst[0] = d0;
        dst[1] = d1;
    }
}

}  // namespace zk
