// fri_ml.cuh -- kernels of the multilinear opening of a FRI commitment (include/zkmle.h "FRI commitment opened as a multilinear
// polynomial"): the Lagrange-form fold of a codeword and the round pass of the sumcheck that runs beside it.  The gather of the queries is
// fri.cuh's, the trees are merkle.cuh's.
//
//   fold    g[k] = (1 - r) (f[k] + f[k + h]) / 2 + r (f[k] - f[k + h]) / (2 c w^k),  k < h = len / 2, on the domain {c w^k}
//                = u + (r / 2c) ((f[k] - f[k + h]) w^-k - c (f[k] + f[k + h])),       u = (f[k] + f[k + h]) / 2
//           fri_fold_kernel's traffic and products, with the sum s = f[k] + f[k + h] leaving the product's other operand too: ONE uniform
//           multiplier (r / 2c, the 81 argument words of fri.cuh's FriUni) as before.  c s is one product more by a lane-uniform value;
//           c travels as a plain element (8 argument words, a Multiplier in registers), not as a second set of 81 rows, and with c = 1
//           (no coset: COSET = false) the product is not there at all.  Every result is canonical.
//   round   one pass per sumcheck round over the table T_{l-1} of 4 q entries and the eq table E_{l-1} of 2 q entries (FOLD), lane i < q:
//             T_l[2i + X] = T_{l-1}[4i + 2X] + r (T_{l-1}[4i + 2X + 1] - T_{l-1}[4i + 2X])     the MLE fold of the LAST variable
//             E_l[i]      = E_{l-1}[2i] + E_{l-1}[2i + 1]                                       the eq table with its last variable summed out
//             S_X        += E_l[i] T_l[2i + X]
//           four contiguous reads of T and two of E, two writes of T and one of E per lane.  Round 0 (FOLD = false) reads T_0 and E_0 and
//           writes neither.  S_0 and S_1 are mle_kernels.cuh's lazy sums (Wide: a carry chain per term, one reduction per workgroup); the
//           workgroups' sums are added by finish_sums_kernel, a second launch of one block.
#pragma once
#include "fri.cuh"
#include "mle_kernels.cuh"

namespace zk {

// the coset shift c_l as a kernel argument: an element with a coset, nothing without one
template <class F, bool COSET> struct FriMlShift {
    Fe<F> c;
};
template <class F> struct FriMlShift<F, false> {};

// pw_lo / pw_hi, shift: as fri_fold_kernel.  g = the rows of r / (2 c_l); c = c_l.
template <class F, bool COSET> __global__ void __launch_bounds__(kFriBlock) fri_ml_fold_kernel(const void *__restrict__ in, void *__restrict__ out, size_t half,
                                                                                              const void *__restrict__ pw_lo, const void *__restrict__ pw_hi,
                                                                                              unsigned shift, FriMlShift<F, COSET> c, FriUni g) {
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
    const Fe<F> s = fe_add<F>(a, b);
    Fe<F> t = fe_mul_u_pre<F>(ntt_pow2t<F>(pw_lo, pw_hi, (uint64_t)k << shift), fe_sub<F>(a, b));
    if constexpr (COSET) t = fe_sub<F>(t, Multiplier<F>(c.c).times(s));
    else t = fe_sub<F>(t, s);
    fe_store<F>(out, k, fe_from_u_below_2p<F>(uni_muladd<F>(m, u_from_limbs32<F>(fe_halve<F>(s)), u_from_limbs32<F>(t))));
}

// q = the number of (T_l pair, E_l entry) a launch covers; partials[X * gridDim.x + block] = the block's share of S_X.
// FOLD: tin has 4 q entries, ein 2 q, tout 2 q, eout q.  !FOLD: tin has 2 q entries, ein q; tout, eout and r are not used.
template <class F, bool FOLD> __global__ void __launch_bounds__(kBlock) fri_ml_round_kernel(const void *__restrict__ tin, const void *__restrict__ ein,
                                                                                          void *__restrict__ tout, void *__restrict__ eout, size_t q, Fe<F> r,
                                                                                          void *__restrict__ partials) {
    __shared__ Wide<F> sh[2 * kBlock / 64];
    const size_t stride = (size_t)gridDim.x * kBlock;
    Wide<F> sum[2] = {wide_zero<F>(), wide_zero<F>()};
    const Multiplier<F> mr(r);
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < q; i += stride) {
        Fe<F> t0, t1, e;
        if (FOLD) {
            const Fe<F> a0 = fe_load<F>(tin, 4 * i), a1 = fe_load<F>(tin, 4 * i + 1), b0 = fe_load<F>(tin, 4 * i + 2), b1 = fe_load<F>(tin, 4 * i + 3);
            t0 = fe_add<F>(a0, mr.times(fe_sub<F>(a1, a0)));
            t1 = fe_add<F>(b0, mr.times(fe_sub<F>(b1, b0)));
            e = fe_add<F>(fe_load<F>(ein, 2 * i), fe_load<F>(ein, 2 * i + 1));
            fe_store<F>(tout, 2 * i, t0);
            fe_store<F>(tout, 2 * i + 1, t1);
            fe_store<F>(eout, i, e);
        } else {
            t0 = fe_load<F>(tin, 2 * i);
            t1 = fe_load<F>(tin, 2 * i + 1);
            e = fe_load<F>(ein, i);
        }
        const Multiplier<F> me(e);
        wide_add_fe<F>(sum[0], me.times(t0));
        wide_add_fe<F>(sum[1], me.times(t1));
    }
    Fe<F> tot;
    if (block_reduce_wide<F, 2>(sum, sh, tot)) fe_store<F>(partials, (size_t)threadIdx.x * gridDim.x + blockIdx.x, tot);
}

}  // namespace zk
