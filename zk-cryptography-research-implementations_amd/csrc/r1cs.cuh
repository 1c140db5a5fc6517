// r1cs.cuh -- the two sparse kernels of an R1CS instance (include/zkmle.h "R1CS instance: sparse matrices times a table"): the products
// A z, B z, C z of three sparse matrices with a table, and the weighted transpose M[y] = sum_x E[x] (A + rho B + rho^2 C)[x, y].
//
//   form     One compressed form serves both: `off` (item boundaries), `idx` (the gathered operand's index per entry) and `val` (the entry's
//            value).  The products read the CSR form of the three matrices laid end to end -- item g = k 2^s + row, k = 0, 1, 2 for A, B, C,
//            so the three products are ONE sparse product of 3 2^s rows -- and the transpose reads the CSC forms, item k 2^d + column.
//   values   An entry's value v is kept as the 32-bit limbs of the integer v R_u mod p, R_u = 2^(29 L) the radix of ufield.cuh's scan (the host
//            converts once, at creation): u_from_limbs32 of it is the fully reduced multiplier that raw_mul_add wants, at no product per entry.
//            The gathered operand is a stored element x R_std, so the raw sum, divided by R_u in raw_mont_reduce, is sum v x R_std: a stored
//            element again.
//   sums     r1cs_dot: raw integer products in mle_kernels.cuh's RawAcc, normalised every kRawCarryEvery, reduced every kR1csChunk<F> terms
//            (the largest multiple of kRawCarryEvery within kRawTermsMax<F>: 68 of 70, 168 of 169) and the reduced parts added in the field.
//            Every value and every operand is a canonical residue, so kRawTermsMax's bound holds whatever they are.
//   bins     Items are binned by length at creation (r1cs_host.h): up to ZK_R1CS_ROW_SPLIT entries one item to a lane, four entries in flight;
//            above it one item to a workgroup, lane t taking the entries t, t + 256, .., the lanes' reduced sums added through LDS.  Field
//            addition is exact, so the value does not depend on the bin.  A transpose item is a column of all three matrices: its length is
//            the three columns' together, and the lane (or every lane of the workgroup) adds s_A + rho s_B + rho^2 s_C before anything is
//            stored, so M is written once and no table per matrix exists.
//   grids    Both kernels of a bin walk their item list with a grid-stride loop that carries nothing from one item to the next; the cap is
//            r1cs_block_cap() (ZK_R1CS_BLOCKS, read at every call so that a test can put a lane on its second item).
#pragma once
#include "mle_kernels.cuh"

namespace zk {

struct R1csSparse {
    const uint32_t *off;         // item i's entries are off[i] .. off[i + 1] - 1
    const uint32_t *idx;         // per entry: the index of the operand it multiplies
    const void *val;             // per entry: v R_u mod p in 32-bit limbs
};

// terms of one reduction: whole carry groups, within the bound
template <class F> constexpr int kR1csChunk = kRawTermsMax<F> / kRawCarryEvery * kRawCarryEvery;
static_assert(kR1csChunk<Fr381> == 68 && kR1csChunk<Bn254Fr> == 168, "68 of 70 and 168 of 169 terms");

template <class F> __device__ __forceinline__ void r1cs_raw_zero(RawAcc<F> &ra) {
#pragma unroll
    for (int c = 0; c < 2 * UParams<F>::L; c++) ra.c[c] = 0;
}
// the normalised columns as a stored element
template <class F> __device__ __forceinline__ Fe<F> r1cs_raw_finish(RawAcc<F> &ra) { return u_to_limbs32<F>(u_reduce_once<F>(raw_mont_reduce<F>(ra))); }

// sum over the entries t = b, b + step, .. < e of val[t] x[idx[t]]
template <class F> __device__ __forceinline__ Fe<F> r1cs_dot(const R1csSparse &m, size_t b, size_t e, size_t step, const void *__restrict__ x) {
    constexpr int kChunk = kR1csChunk<F>;
    static_assert(kChunk <= kRawTermsMax<F> && kChunk % kRawCarryEvery == 0, "terms of one reduction");
    Fe<F> tot = fe_zero<F>();
    RawAcc<F> ra;
    r1cs_raw_zero<F>(ra);
    int n = 0;                                               // terms in ra: a multiple of kRawCarryEvery below kChunk between two trips
    size_t t = b;
    for (; t + (kRawCarryEvery - 1) * step < e; t += kRawCarryEvery * step) {
        Fe<F> v[kRawCarryEvery], w[kRawCarryEvery];
#pragma unroll
        for (int i = 0; i < kRawCarryEvery; i++) {
            v[i] = fe_load<F>(m.val, t + i * step);
            w[i] = fe_load<F>(x, m.idx[t + i * step]);
        }
#pragma unroll
        for (int i = 0; i < kRawCarryEvery; i++) raw_mul_add<F>(ra, u_from_limbs32<F>(w[i]), u_from_limbs32<F>(v[i]));
        raw_normalize<F>(ra);
        n += kRawCarryEvery;
        if (n == kChunk) {
            tot = fe_add<F>(tot, r1cs_raw_finish<F>(ra));
            r1cs_raw_zero<F>(ra);
            n = 0;
        }
    }
    if (t < e) {                                             // at most kRawCarryEvery - 1 more: n stays below kChunk
        for (; t < e; t += step, n++) raw_mul_add<F>(ra, u_from_limbs32<F>(fe_load<F>(x, m.idx[t])), u_from_limbs32<F>(fe_load<F>(m.val, t)));
        raw_normalize<F>(ra);
    }
    if (n) tot = fe_add<F>(tot, r1cs_raw_finish<F>(ra));
    return tot;
}

// the workgroup's sum of v over its kBlock lanes, valid in lane 0; sh is free again on return
template <class F> __device__ __forceinline__ Fe<F> r1cs_block_sum(Fe<F> v, Fe<F> *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
#pragma unroll 1
    for (unsigned h = kBlock / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) sh[threadIdx.x] = fe_add<F>(sh[threadIdx.x], sh[threadIdx.x + h]);
        __syncthreads();
    }
    v = sh[0];
    __syncthreads();
    return v;
}

// ---- the products ---------------------------------------------------------------------------------------------------------------------
struct R1csOut3 {
    void *t[3];                  // A z, B z, C z: 2^log_rows elements each
};
template <class F> __device__ __forceinline__ void r1cs_store_row(const R1csOut3 &o, uint32_t g, unsigned log_rows, const Fe<F> &v) {
    const uint32_t k = g >> log_rows, row = g & ((1u << log_rows) - 1u);
    fe_store<F>(k == 0 ? o.t[0] : (k == 1 ? o.t[1] : o.t[2]), row, v);
}
// items[0 .. nitems): the rows g = k 2^log_rows + row of up to ZK_R1CS_ROW_SPLIT entries, one to a lane; z: 2^d elements
template <class F> __global__ void __launch_bounds__(kBlock) r1cs_matvec_lane_kernel(R1csSparse m, const uint32_t *__restrict__ items, size_t nitems, unsigned log_rows,
                                                                                      const void *__restrict__ z, R1csOut3 out) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < nitems; i += stride) {
        const uint32_t g = items[i];
        r1cs_store_row<F>(out, g, log_rows, r1cs_dot<F>(m, m.off[g], m.off[g + 1], 1, z));
    }
}
// the rows above ZK_R1CS_ROW_SPLIT entries, one to a workgroup
template <class F> __global__ void __launch_bounds__(kBlock) r1cs_matvec_block_kernel(R1csSparse m, const uint32_t *__restrict__ items, size_t nitems, unsigned log_rows,
                                                                                       const void *__restrict__ z, R1csOut3 out) {
    __shared__ Fe<F> sh[kBlock];
    for (size_t i = blockIdx.x; i < nitems; i += gridDim.x) {
        const uint32_t g = items[i];
        const Fe<F> v = r1cs_block_sum<F>(r1cs_dot<F>(m, (size_t)m.off[g] + threadIdx.x, m.off[g + 1], kBlock, z), sh);
        if (threadIdx.x == 0) r1cs_store_row<F>(out, g, log_rows, v);
    }
}

// ---- the weighted transpose -------------------------------------------------------------------------------------------------------------
// column y's share of lane `first` with `step` lanes to the column: s_A + rho s_B + rho^2 s_C over the CSC items y, ncols + y, 2 ncols + y
template <class F> __device__ __forceinline__ Fe<F> r1cs_bind_column(const R1csSparse &m, size_t y, size_t ncols, size_t first, size_t step, const void *__restrict__ E,
                                                                     const Multiplier<F> &rho, const Multiplier<F> &rho2) {
    Fe<F> v = r1cs_dot<F>(m, (size_t)m.off[y] + first, m.off[y + 1], step, E);
    v = fe_add<F>(v, rho.times(r1cs_dot<F>(m, (size_t)m.off[ncols + y] + first, m.off[ncols + y + 1], step, E)));
    return fe_add<F>(v, rho2.times(r1cs_dot<F>(m, (size_t)m.off[2 * ncols + y] + first, m.off[2 * ncols + y + 1], step, E)));
}
// items[0 .. nitems): the columns y of up to ZK_R1CS_ROW_SPLIT entries in the three matrices together, one to a lane; E: 2^s elements;
// M[y] is written for the listed columns only (the lists cover every column the caller asked for)
template <class F> __global__ void __launch_bounds__(kBlock) r1cs_bind_lane_kernel(R1csSparse m, const uint32_t *__restrict__ items, size_t nitems, size_t ncols,
                                                                                    const void *__restrict__ E, Fe<F> rho, Fe<F> rho2, void *__restrict__ M) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    const Multiplier<F> mr(rho), mr2(rho2);
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < nitems; i += stride) {
        const uint32_t y = items[i];
        fe_store<F>(M, y, r1cs_bind_column<F>(m, y, ncols, 0, 1, E, mr, mr2));
    }
}
template <class F> __global__ void __launch_bounds__(kBlock) r1cs_bind_block_kernel(R1csSparse m, const uint32_t *__restrict__ items, size_t nitems, size_t ncols,
                                                                                     const void *__restrict__ E, Fe<F> rho, Fe<F> rho2, void *__restrict__ M) {
    __shared__ Fe<F> sh[kBlock];
    const Multiplier<F> mr(rho), mr2(rho2);
    for (size_t i = blockIdx.x; i < nitems; i += gridDim.x) {
        const uint32_t y = items[i];
        const Fe<F> v = r1cs_block_sum<F>(r1cs_bind_column<F>(m, y, ncols, threadIdx.x, kBlock, E, mr, mr2), sh);
        if (threadIdx.x == 0) fe_store<F>(M, y, v);
    }
}

// the grid cap of the four kernels, in workgroups: ZK_R1CS_BLOCKS (1 .. kMaxBlocks), read at every call
inline int r1cs_block_cap() {
    const char *e = getenv("ZK_R1CS_BLOCKS");
    const int k = e ? atoi(e) : kMaxBlocks;
    return k < 1 ? 1 : (k > kMaxBlocks ? kMaxBlocks : k);
}

}  // namespace zk
