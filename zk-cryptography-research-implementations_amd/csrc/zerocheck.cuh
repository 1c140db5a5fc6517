// zerocheck.cuh -- the round pass of the zerocheck of a product (include/zkmle.h "Zerocheck of a product of committed tables"): the sumcheck
// of  sum_x E[x] (A[x] B[x] - C[x]) = 0  with E = eq(., tau), in the idiom of fri_ml.cuh's fri_ml_round_w_kernel.
//
//   round   one pass per round over the four tables A_{l-1}, B_{l-1}, C_{l-1}, E_{l-1} of 4 q entries each (FOLD), lane i < q:
//             X_l[2i + k] = X_{l-1}[4i + 2k] + r (X_{l-1}[4i + 2k + 1] - X_{l-1}[4i + 2k])   the MLE fold of the LAST variable, X = A, B, C, E
//           and with X0 = X_l[2i], X1 = X_l[2i + 1], X2 = 2 X1 - X0 (the pair's line at the node 2; additions only):
//             s_0   += E0 (A0 B0 - C0)                     g_l(0)
//             s_1   += E1 (A1 B1 - C1)                     g_l(1)
//             s_2   += E2 (A2 B2 - C2)                     g_l(2)
//             s_inf += (E1 - E0) (A1 - A0) (B1 - B0)       the X^3 coefficient: C is linear in X and has no share in it
//           The host forms g_l(3) = 3 g_l(2) - 3 g_l(1) + g_l(0) + 6 s_inf (the third difference of a cubic is six times its leading
//           coefficient).  Sixteen contiguous reads and eight writes of 32 bytes per lane, sixteen products.
//           One table is folded and stored before the next is loaded, and what a table contributes is folded into the running products at
//           once (A and B leave four products, C turns three of them into differences, E multiplies them into the sums), so at most four
//           loaded elements are live beside four running values and the four lazy sums.
//           Round 0 (FOLD = false) reads two contiguous entries of each table and writes nothing: A, B, C are then the commitments' own
//           coefficient tables.  The sums are mle_kernels.cuh's Wide (a carry chain per term, one reduction per workgroup); the
//           workgroups' sums are added by finish_sums_kernel, a second launch of one block.
#pragma once
#include "mle_kernels.cuh"

namespace zk {

// the four tables of a pass, in the order A, B, C, E: read, and (FOLD) written
struct ZerocheckTables {
    const void *in[4];
    void *out[4];
};

// the pair (X_l[2i], X_l[2i + 1]) of table `in`: folded from four entries by r and stored (FOLD), or read as it is
template <class F, bool FOLD> __device__ __forceinline__ void zerocheck_pair(const void *__restrict__ in, void *__restrict__ out, size_t i, const Multiplier<F> &mr,
                                                                           Fe<F> &x0, Fe<F> &x1) {
    if constexpr (FOLD) {
        const Fe<F> a0 = fe_load<F>(in, 4 * i), a1 = fe_load<F>(in, 4 * i + 1), b0 = fe_load<F>(in, 4 * i + 2), b1 = fe_load<F>(in, 4 * i + 3);
        x0 = fe_add<F>(a0, mr.times(fe_sub<F>(a1, a0)));
        x1 = fe_add<F>(b0, mr.times(fe_sub<F>(b1, b0)));
        fe_store<F>(out, 2 * i, x0);
        fe_store<F>(out, 2 * i + 1, x1);
    } else {
        x0 = fe_load<F>(in, 2 * i);
        x1 = fe_load<F>(in, 2 * i + 1);
    }
}

// q = the number of pairs a launch covers; partials[X * gridDim.x + block] = the block's share of sum X, X < 4 (s_0, s_1, s_2, s_inf).
// FOLD: every t.in has 4 q entries, every t.out 2 q.  !FOLD: every t.in has 2 q entries; t.out and r are not used.
template <class F, bool FOLD> __global__ void __launch_bounds__(kBlock) zerocheck_mul_round_kernel(ZerocheckTables t, size_t q, Fe<F> r, void *__restrict__ partials) {
    __shared__ Wide<F> sh[4 * kBlock / 64];
    const size_t stride = (size_t)gridDim.x * kBlock;
    Wide<F> sum[4] = {wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>()};
    const Multiplier<F> mr(r);
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < q; i += stride) {
        Fe<F> p0, p1, p2, pinf;                               // A B at the nodes 0, 1, 2 and its X^2 coefficient; then less C
        {
            Fe<F> a0, a1, b0, b1;
            zerocheck_pair<F, FOLD>(t.in[0], t.out[0], i, mr, a0, a1);
            zerocheck_pair<F, FOLD>(t.in[1], t.out[1], i, mr, b0, b1);
            const Fe<F> da = fe_sub<F>(a1, a0), db = fe_sub<F>(b1, b0);
            p0 = fe_mul<F>(a0, b0);
            p1 = fe_mul<F>(a1, b1);
            p2 = fe_mul<F>(fe_add<F>(a1, da), fe_add<F>(b1, db));
            pinf = fe_mul<F>(da, db);
        }
        {
            Fe<F> c0, c1;
            zerocheck_pair<F, FOLD>(t.in[2], t.out[2], i, mr, c0, c1);
            p0 = fe_sub<F>(p0, c0);
            p1 = fe_sub<F>(p1, c1);
            p2 = fe_sub<F>(p2, fe_add<F>(c1, fe_sub<F>(c1, c0)));
        }
        Fe<F> e0, e1;
        zerocheck_pair<F, FOLD>(t.in[3], t.out[3], i, mr, e0, e1);
        const Fe<F> de = fe_sub<F>(e1, e0);
        wide_add_fe<F>(sum[0], fe_mul<F>(e0, p0));
        wide_add_fe<F>(sum[1], fe_mul<F>(e1, p1));
        wide_add_fe<F>(sum[2], fe_mul<F>(fe_add<F>(e1, de), p2));
        wide_add_fe<F>(sum[3], fe_mul<F>(de, pinf));
    }
    Fe<F> tot;
    if (block_reduce_wide<F, 4>(sum, sh, tot)) fe_store<F>(partials, (size_t)threadIdx.x * gridDim.x + blockIdx.x, tot);
}

}  // namespace zk
