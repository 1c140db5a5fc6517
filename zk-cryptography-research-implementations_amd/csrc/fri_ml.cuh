// fri_ml.cuh -- kernels of the multilinear opening of a FRI commitment (include/zkmle.h "FRI commitment opened as a multilinear
// polynomial"): the Lagrange-form fold of a codeword and the round pass of the sumcheck that runs beside it, in its single-point form (an
// eq table summed out) and its several-point form (a weight table folded beside T: fri_ml_round_w_kernel, at the end).  The gather of the
// queries is fri.cuh's, the trees are merkle.cuh's.
//
//   fold    g[k] = (1 - r) (f[k] + f[k + h]) / 2 + r (f[k] - f[k + h]) / (2 c w^k),  k < h = len / 2, on the domain {c w^k}
//                = u + (r / 2c) ((f[k] - f[k + h]) w^-k - c (f[k] + f[k + h])),       u = (f[k] + f[k + h]) / 2
//           fri_fold_kernel's traffic and products, with the sum s = f[k] + f[k + h] leaving the product's other operand too: ONE uniform
//           multiplier (r / 2c, the 81 argument words of fri.cuh's FriUni) as before.  c s is one product more by a lane-uniform value;
//           c travels as a plain element (8 argument words, a Multiplier in registers), not as a second set of 81 rows, and with c = 1
//           (no coset: COSET = false) the product is not there at all.  Every result is canonical.
//   fold4   two folds in one pass (the opening folded by 4: include/zkmle.h "FRI commitment opened with a fold arity"), lane k < q = len / 4:
//             u0 = fold(f[k], f[k + 2q]; r0, x),  u1 = fold(f[k + q], f[k + 3q]; r0, i x),  g[k] = fold(u0, u1; r1, x^2),  x = c w^k, i = w^q
//           four coalesced reads at the quarter strides and one write where two fold launches read four, write three and read two of
//           them again.  Stage 1 is the fold above twice with the ONE uniform multiplier r0 / 2c (w^-(k+q) = (i x / c)^-1 is the table's
//           entry k + q); stage 2 multiplies by r1 / 2c^2 as a Multiplier in registers (8 argument words): a second set of 81 rows
//           does not fit the scalar registers.  (w^-k)^2 is the table's entry 2k.  Every result is canonical, so g is the table two
//           fri_ml_fold_kernel launches leave, byte for byte.
//   round   one pass per sumcheck round over the table T_{l-1} of 4 q entries and the eq table E_{l-1} of 2 q entries (FOLD), lane i < q:
//             T_l[2i + X] = T_{l-1}[4i + 2X] + r (T_{l-1}[4i + 2X + 1] - T_{l-1}[4i + 2X])     the MLE fold of the LAST variable
//             E_l[i]      = E_{l-1}[2i] + E_{l-1}[2i + 1]                                       the eq table with its last variable summed out
//             S_X        += E_l[i] T_l[2i + X]
//           four contiguous reads of T and two of E, two writes of T and one of E per lane.  Round 0 (FOLD = false) reads T_0 and E_0 and
//           writes neither.  S_0 and S_1 are mle_kernels.cuh's lazy sums (Wide: a carry chain per term, one reduction per workgroup); the
//           workgroups' sums are added by finish_sums_kernel, a second launch of one block.
//   fold_batch  the first step of an opening of k commitments together (include/zkmle.h "FRI commitments opened together"): the fold or
//           fold4 above on u = sum_j alpha^j f_j, with the combination formed in registers (fri_ml_fold_batch_kernel, at the end).
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

// the shifts of a fold by 4: c_l and c_{l+1} = c_l^2 with a coset, nothing without one
template <class F, bool COSET> struct FriMlShift2 {
    Fe<F> c, c2;
};
template <class F> struct FriMlShift2<F, false> {};

// one stage-1 fold: s / 2 + g (w (a - b) - c s), s = a + b; g = the rows of r0 / (2 c)
template <class F, bool COSET> __device__ __forceinline__ Fe<F> fri_ml_fold4_stage1(const UniMul<F> &m, const Ufe<F> &w, const Fe<F> &a, const Fe<F> &b,
                                                                                   const FriMlShift2<F, COSET> &c) {
    const Fe<F> s = fe_add<F>(a, b);
    Fe<F> t = fe_mul_u_pre<F>(w, fe_sub<F>(a, b));
    if constexpr (COSET) t = fe_sub<F>(t, Multiplier<F>(c.c).times(s));
    else t = fe_sub<F>(t, s);
    return fe_from_u_below_2p<F>(uni_muladd<F>(m, u_from_limbs32<F>(fe_halve<F>(s)), u_from_limbs32<F>(t)));
}

// pw_lo / pw_hi, shift: as fri_ml_fold_kernel (the layer's w^-k is entry k << shift; 2 quarter entries of it exist).  g0 = the rows of
// r0 / (2 c_l); g1 = r1 / (2 c_l^2); c = c_l and c_l^2.  in: 4 quarter entries, out: quarter.
template <class F, bool COSET> __global__ void __launch_bounds__(kFriBlock) fri_ml_fold4_kernel(const void *__restrict__ in, void *__restrict__ out, size_t quarter,
                                                                                               const void *__restrict__ pw_lo, const void *__restrict__ pw_hi,
                                                                                               unsigned shift, FriMlShift2<F, COSET> c, Fe<F> g1, FriUni g0) {
    constexpr int L = UParams<F>::L;
    static_assert(L * L == 81, "FriUni holds the rows of a nine-limb field");
    const size_t k = (size_t)blockIdx.x * kFriBlock + threadIdx.x;
    if (k >= quarter) return;
    UniMul<F> m;
#pragma unroll
    for (int i = 0; i < L; i++) {
#pragma unroll
        for (int j = 0; j < L; j++) m.t[i][j] = g0.t[i * L + j];
    }
    const Fe<F> u0 = fri_ml_fold4_stage1<F, COSET>(m, ntt_pow2t<F>(pw_lo, pw_hi, (uint64_t)k << shift), fe_load<F>(in, k), fe_load<F>(in, k + 2 * quarter), c);
    const Fe<F> u1 = fri_ml_fold4_stage1<F, COSET>(m, ntt_pow2t<F>(pw_lo, pw_hi, (uint64_t)(k + quarter) << shift), fe_load<F>(in, k + quarter),
                                                   fe_load<F>(in, k + 3 * quarter), c);
    const Fe<F> s = fe_add<F>(u0, u1);
    Fe<F> t = fe_mul_u_pre<F>(ntt_pow2t<F>(pw_lo, pw_hi, (uint64_t)k << (shift + 1)), fe_sub<F>(u0, u1));
    if constexpr (COSET) t = fe_sub<F>(t, Multiplier<F>(c.c2).times(s));
    else t = fe_sub<F>(t, s);
    fe_store<F>(out, k, fe_add<F>(fe_halve<F>(s), Multiplier<F>(g1).times(t)));
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

// The round pass of the opening at SEVERAL points (include/zkmle.h "... opened at several points"): the weights are a table W_l of their
// own, the gamma-combination of the points' eq tables, folded by the same challenge as T_l -- the pass does not know how many points
// there are.  Lane i < q (FOLD):
//     T_l[2i + X] = T_{l-1}[4i + 2X] + r (T_{l-1}[4i + 2X + 1] - T_{l-1}[4i + 2X]),   W_l[2i + X] the same from W_{l-1}
//     s_0 += W_l[2i] T_l[2i],   s_1 += W_l[2i+1] T_l[2i+1],   s_inf += (W_l[2i+1] - W_l[2i]) (T_l[2i+1] - T_l[2i])
// g_l at the nodes 0, 1 and infinity (the X^2 coefficient), as sumcheck_kernels.cuh; the host forms g_l(2) = 2 g_l(1) - g_l(0) + 2 s_inf.
// Eight contiguous reads and four writes per lane.  T is folded and stored before W is loaded, so at most four loaded elements are live at
// a time beside the three lazy sums.  !FOLD: tin and win have 2 q entries each and are only read; tout, wout and r are not used.
// partials[X * gridDim.x + block], X < 3.
template <class F, bool FOLD> __global__ void __launch_bounds__(kBlock) fri_ml_round_w_kernel(const void *__restrict__ tin, const void *__restrict__ win,
                                                                                            void *__restrict__ tout, void *__restrict__ wout, size_t q, Fe<F> r,
                                                                                            void *__restrict__ partials) {
    __shared__ Wide<F> sh[3 * kBlock / 64];
    const size_t stride = (size_t)gridDim.x * kBlock;
    Wide<F> sum[3] = {wide_zero<F>(), wide_zero<F>(), wide_zero<F>()};
    const Multiplier<F> mr(r);
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < q; i += stride) {
        Fe<F> t0, t1, w0, w1;
        if (FOLD) {
            {
                const Fe<F> a0 = fe_load<F>(tin, 4 * i), a1 = fe_load<F>(tin, 4 * i + 1), b0 = fe_load<F>(tin, 4 * i + 2), b1 = fe_load<F>(tin, 4 * i + 3);
                t0 = fe_add<F>(a0, mr.times(fe_sub<F>(a1, a0)));
                t1 = fe_add<F>(b0, mr.times(fe_sub<F>(b1, b0)));
                fe_store<F>(tout, 2 * i, t0);
                fe_store<F>(tout, 2 * i + 1, t1);
            }
            {
                const Fe<F> a0 = fe_load<F>(win, 4 * i), a1 = fe_load<F>(win, 4 * i + 1), b0 = fe_load<F>(win, 4 * i + 2), b1 = fe_load<F>(win, 4 * i + 3);
                w0 = fe_add<F>(a0, mr.times(fe_sub<F>(a1, a0)));
                w1 = fe_add<F>(b0, mr.times(fe_sub<F>(b1, b0)));
                fe_store<F>(wout, 2 * i, w0);
                fe_store<F>(wout, 2 * i + 1, w1);
            }
        } else {
            t0 = fe_load<F>(tin, 2 * i);
            t1 = fe_load<F>(tin, 2 * i + 1);
            w0 = fe_load<F>(win, 2 * i);
            w1 = fe_load<F>(win, 2 * i + 1);
        }
        wide_add_fe<F>(sum[0], fe_mul<F>(w0, t0));
        wide_add_fe<F>(sum[1], fe_mul<F>(w1, t1));
        wide_add_fe<F>(sum[2], fe_mul<F>(fe_sub<F>(w1, w0), fe_sub<F>(t1, t0)));
    }
    Fe<F> tot;
    if (block_reduce_wide<F, 3>(sum, sh, tot)) fe_store<F>(partials, (size_t)threadIdx.x * gridDim.x + blockIdx.x, tot);
}

// The first step's fold of k codewords opened together, the combination fused in: lane i < part = N / SIDES forms, for each side s,
//     u_s = sum_j c_j f_j[i + s part]
// by lincomb_at (mle_kernels.cuh: raw products into 64-bit columns, a normalisation per kRawCarryEvery of them, ONE reduction per side, the
// coefficients read from the argument block where they are used), one side after the other so that one accumulator is live at a time, and
// then applies fri_ml_fold_kernel's fold (SIDES = 2: u_0, u_1) or fri_ml_fold4_kernel's (SIDES = 4: u_0, u_2 and u_1, u_3, then the pair)
// to the canonical u_s.  The k N entries are read once and N / SIDES written; the combined layer never exists in memory.  Layer 0 only:
// w^-i is the table's entry i.
// Every fold here is s / 2 + g (w (a - b) - c s) with g as a Multiplier in registers (8 argument words), the form of fri_ml_fold4_kernel's
// second stage, and NOT the 81 rows of a FriUni: beside the combination's pointers and coefficients the rows do not fit the scalar
// registers (106 with 50 spilled into lanes and a private segment, profiles/fri_ml_batch).  Each result is the canonical residue of the
// value the rows give, so the table is byte for byte the one the single-table kernels leave on zk_mle_linear_combination's output.
// g0 = r0 / (2 c); SIDES = 4: g1 = r1 / (2 c^2) and c.c2 = c^2, not read otherwise.
constexpr int kFriMlBatchMax = 16;                           // ZK_FRI_ML_BATCH_MAX
constexpr int kFriMlBatchBlocks = 768;                       // three workgroups a compute unit
template <class F> struct FriMlBatchArgs {
    const void *t[kFriMlBatchMax];                           // the k codewords (one may appear more than once)
    Fe<F> c[kFriMlBatchMax];                                 // lincomb_coeff of the k coefficients
    int k;
};
// one fold: s / 2 + g (w (a - b) - c s), s = a + b
template <class F, bool COSET> __device__ __forceinline__ Fe<F> fri_ml_fold_by(const Multiplier<F> &g, const Ufe<F> &w, const Fe<F> &a, const Fe<F> &b, const Fe<F> &c) {
    const Fe<F> s = fe_add<F>(a, b);
    Fe<F> t = fe_mul_u_pre<F>(w, fe_sub<F>(a, b));
    if constexpr (COSET) t = fe_sub<F>(t, Multiplier<F>(c).times(s));
    else t = fe_sub<F>(t, s);
    return fe_add<F>(fe_halve<F>(s), g.times(t));
}
// the pass's body, generic over the argument block (FriMlBatchArgs, or FriMlBatchArgsCap of another capacity: lincomb_at reads t, c and k)
template <class F, int SIDES, bool COSET, class Args>
__device__ __forceinline__ void fri_ml_fold_batch_body(const Args &a, void *__restrict__ out, size_t part, const void *__restrict__ pw_lo, const void *__restrict__ pw_hi,
                                                       const FriMlShift2<F, COSET> &c, const Fe<F> &g0, const Fe<F> &g1) {
    static_assert(SIDES == 2 || SIDES == 4, "a fold by 2 or by 4");
    const size_t stride = (size_t)gridDim.x * kFriBlock;
    Fe<F> c1 = g0, c2 = g0;                                  // the shifts; not read without a coset
    if constexpr (COSET) {
        c1 = c.c;
        c2 = c.c2;
    }
    for (size_t i = (size_t)blockIdx.x * kFriBlock + threadIdx.x; i < part; i += stride) {
        const Multiplier<F> m0(g0);
        if constexpr (SIDES == 2) {
            const Fe<F> u0 = lincomb_at<F>(a, i), u1 = lincomb_at<F>(a, i + part);
            fe_store<F>(out, i, fri_ml_fold_by<F, COSET>(m0, ntt_pow2t<F>(pw_lo, pw_hi, (uint64_t)i), u0, u1, c1));
        } else {                                              // each pair is folded as soon as it is there: two sides and one fold live
            const Fe<F> u0 = lincomb_at<F>(a, i), u2 = lincomb_at<F>(a, i + 2 * part);
            const Fe<F> v0 = fri_ml_fold_by<F, COSET>(m0, ntt_pow2t<F>(pw_lo, pw_hi, (uint64_t)i), u0, u2, c1);
            const Fe<F> u1 = lincomb_at<F>(a, i + part), u3 = lincomb_at<F>(a, i + 3 * part);
            const Fe<F> v1 = fri_ml_fold_by<F, COSET>(m0, ntt_pow2t<F>(pw_lo, pw_hi, (uint64_t)(i + part)), u1, u3, c1);
            fe_store<F>(out, i, fri_ml_fold_by<F, COSET>(Multiplier<F>(g1), ntt_pow2t<F>(pw_lo, pw_hi, (uint64_t)i << 1), v0, v1, c2));
        }
    }
}
template <class F, int SIDES, bool COSET> __global__ void __launch_bounds__(kFriBlock) fri_ml_fold_batch_kernel(FriMlBatchArgs<F> a, void *__restrict__ out, size_t part,
                                                                                                          const void *__restrict__ pw_lo,
                                                                                                          const void *__restrict__ pw_hi,
                                                                                                          FriMlShift2<F, COSET> c, Fe<F> g0, Fe<F> g1) {
    fri_ml_fold_batch_body<F, SIDES, COSET>(a, out, part, pw_lo, pw_hi, c, g0, g1);
}

// The same pass for 17 .. 32 codewords ("FRI commitments opened together, wide": ZK_FRI_ML_WIDE_MAX).  The argument block has a capacity
// parameter; the 16-slot block above stays the type it was, so k <= 16 launches the instantiation it always did, through either door.  The
// 32-slot block is 32 pointers, 32 coefficients and k: 256 + 1024 + 4 = 1284 bytes of kernel arguments (static_assert below), read where
// they are used like the narrow one's.  lincomb_at takes one reduction for up to kRawTermsMax = 70 (BLS12-381 Fr) terms, so 32 need no
// intermediate one; its static_assert checks the block's slots.
constexpr int kFriMlWideMax = 32;                            // ZK_FRI_ML_WIDE_MAX
template <class F, int CAP> struct FriMlBatchArgsCap {
    const void *t[CAP];
    Fe<F> c[CAP];
    int k;
};
using FriMlWideArgs381 = FriMlBatchArgsCap<Fr381, kFriMlWideMax>;
static_assert(sizeof(FriMlWideArgs381::t) + sizeof(FriMlWideArgs381::c) + sizeof(int) == 1284, "the wide block: 32 pointers, 32 coefficients, k");
template <class F, int CAP, int SIDES, bool COSET>
__global__ void __launch_bounds__(kFriBlock) fri_ml_fold_batch_wide_kernel(FriMlBatchArgsCap<F, CAP> a, void *__restrict__ out, size_t part, const void *__restrict__ pw_lo,
                                                                           const void *__restrict__ pw_hi, FriMlShift2<F, COSET> c, Fe<F> g0, Fe<F> g1) {
    fri_ml_fold_batch_body<F, SIDES, COSET>(a, out, part, pw_lo, pw_hi, c, g0, g1);
}

}  // namespace zk
