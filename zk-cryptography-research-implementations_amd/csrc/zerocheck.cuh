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
//
// The Plonk gate (include/zkmle.h "Zerocheck of a Plonk gate over committed tables") is the same pass over nine tables, in the order
// A, B, C, qM, qL, qR, qO, qC, E:  sum_x E (qM A B + qL A + qR B + qO C + qC), a quartic in X:
//   round   lane i < q folds the nine tables as above (36 reads and 18 writes of 32 bytes, 18 products) and, with Y_k the pair's line at the
//           node k (Y_{k+1} = Y_k + (Y1 - Y0): additions only), accumulates at k = 0, 1, 2, 3
//             s_k   += E_k ((qM_k B_k + qL_k) A_k + qR_k B_k + qO_k C_k + qC_k)
//             s_inf += (E1 - E0) (qM1 - qM0) (A1 - A0) (B1 - B0)      the X^4 coefficient: only qM A B has a share in it
//           The host forms g(4) = 4 g(3) - 6 g(2) + 4 g(1) - g(0) + 24 s_inf (the fourth difference of a quartic is 24 times its leading
//           coefficient).  23 products for the message.  The tables come in the order B, qR, qM, qL, A, qO, C, qC, E and each one's share
//           goes into the running values u_k, v_k and the infinity term at once: B's four node values die with qM, v_k = qR_k B_k with A.
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

// the nine tables of a gate pass, in the order A, B, C, qM, qL, qR, qO, qC, E
struct ZerocheckGateTables {
    const void *in[9];
    void *out[9];
};

// y[k] = the line through (0, x0), (1, x1) at the node k < 4
template <class F> __device__ __forceinline__ void zerocheck_nodes(const Fe<F> &x0, const Fe<F> &x1, Fe<F> (&y)[4]) {
    const Fe<F> dx = fe_sub<F>(x1, x0);
    y[0] = x0;
    y[1] = x1;
    y[2] = fe_add<F>(x1, dx);
    y[3] = fe_add<F>(y[2], dx);
}

// partials[X * gridDim.x + block] = the block's share of sum X, X < 5 (s_0, s_1, s_2, s_3, s_inf); q, FOLD and the tables' lengths as in
// zerocheck_mul_round_kernel
template <class F, bool FOLD> __global__ void __launch_bounds__(kBlock) zerocheck_gate_round_kernel(ZerocheckGateTables t, size_t q, Fe<F> r, void *__restrict__ partials) {
    enum { A, B, C, QM, QL, QR, QO, QC, E };
    __shared__ Wide<F> sh[5 * kBlock / 64];
    const size_t stride = (size_t)gridDim.x * kBlock;
    Wide<F> sum[5] = {wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>()};
    const Multiplier<F> mr(r);
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < q; i += stride) {
        Fe<F> u[4], v[4], uinf, x0, x1, y[4];                 // u_k: the bracket that A multiplies, then the gate at the node k; v_k = qR_k B_k
        {
            Fe<F> b[4];
            zerocheck_pair<F, FOLD>(t.in[B], t.out[B], i, mr, x0, x1);
            zerocheck_nodes<F>(x0, x1, b);
            const Fe<F> db = fe_sub<F>(x1, x0);
            zerocheck_pair<F, FOLD>(t.in[QR], t.out[QR], i, mr, x0, x1);
            zerocheck_nodes<F>(x0, x1, y);
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = fe_mul<F>(y[k], b[k]);
            zerocheck_pair<F, FOLD>(t.in[QM], t.out[QM], i, mr, x0, x1);
            zerocheck_nodes<F>(x0, x1, y);
#pragma unroll
            for (int k = 0; k < 4; k++) u[k] = fe_mul<F>(y[k], b[k]);
            uinf = fe_mul<F>(fe_sub<F>(x1, x0), db);
        }
        zerocheck_pair<F, FOLD>(t.in[QL], t.out[QL], i, mr, x0, x1);
        zerocheck_nodes<F>(x0, x1, y);
#pragma unroll
        for (int k = 0; k < 4; k++) u[k] = fe_add<F>(u[k], y[k]);
        zerocheck_pair<F, FOLD>(t.in[A], t.out[A], i, mr, x0, x1);
        zerocheck_nodes<F>(x0, x1, y);
#pragma unroll
        for (int k = 0; k < 4; k++) u[k] = fe_add<F>(fe_mul<F>(u[k], y[k]), v[k]);
        uinf = fe_mul<F>(uinf, fe_sub<F>(x1, x0));
        {
            Fe<F> c[4];
            zerocheck_pair<F, FOLD>(t.in[QO], t.out[QO], i, mr, x0, x1);
            zerocheck_nodes<F>(x0, x1, y);
            zerocheck_pair<F, FOLD>(t.in[C], t.out[C], i, mr, x0, x1);
            zerocheck_nodes<F>(x0, x1, c);
#pragma unroll
            for (int k = 0; k < 4; k++) u[k] = fe_add<F>(u[k], fe_mul<F>(y[k], c[k]));
        }
        zerocheck_pair<F, FOLD>(t.in[QC], t.out[QC], i, mr, x0, x1);
        zerocheck_nodes<F>(x0, x1, y);
#pragma unroll
        for (int k = 0; k < 4; k++) u[k] = fe_add<F>(u[k], y[k]);
        zerocheck_pair<F, FOLD>(t.in[E], t.out[E], i, mr, x0, x1);
        zerocheck_nodes<F>(x0, x1, y);
#pragma unroll
        for (int k = 0; k < 4; k++) wide_add_fe<F>(sum[k], fe_mul<F>(y[k], u[k]));
        wide_add_fe<F>(sum[4], fe_mul<F>(fe_sub<F>(x1, x0), uinf));
    }
    Fe<F> tot;
    if (block_reduce_wide<F, 5>(sum, sh, tot)) fe_store<F>(partials, (size_t)threadIdx.x * gridDim.x + blockIdx.x, tot);
}

}  // namespace zk
