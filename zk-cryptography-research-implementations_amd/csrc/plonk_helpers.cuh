// plonk_helpers.cuh -- the four helper tables of the Plonk proof with lookup rows on column commitments (include/zkmle.h "Plonk with lookups on
// column commitments") in ONE pass over A, B, C, SA, SB, SC, qK, T0, T1, T2, M, in the single-denominator form:
//
//     H_j[x] = N_j[x] inv0(Did_j[x] Dsig_j[x]),   j < 3          N_j = Dsig_j - Did_j = gamma (S_j[x] - id_j[x]),   id_j[x] = j n + x
//                                                                Did_j = beta + W_j[x] + gamma id_j[x],   Dsig_j = beta + W_j[x] + gamma S_j[x]
//     HL[x]  = (qK[x] Dt[x] - M[x] Dw[x]) inv0(Dw[x] Dt[x])      Dw = beta + A + gamma B + gamma^2 C,   Dt = beta + T0 + gamma T1 + gamma^2 T2
//
// with inv0(0) = 0.  ONE inverse per entry, of the product of its two denominators, where wiring_fractions_kernel and lookup_fractions_kernel take
// two: 1 / Did - 1 / Dsig = (Dsig - Did) / (Did Dsig) and qK / Dw - M / Dt = (qK Dt - M Dw) / (Dw Dt).
//
//   the two definitions   Where no denominator is zero the entries are, as field elements, exactly those of the two existing kernels.  Where a
//       PRODUCT of two denominators is zero the entry here is 0; the existing kernels give inv0 per denominator.  The two differ only when
//       exactly ONE of the pair is zero: there the old entry is -1 / Dsig (or 1 / Did, -M / Dt, qK / Dw) and the new one 0.  The verifier's relation
//       for that entry is H Did Dsig - N = 0 (H Dw Dt - qK Dt + M Dw = 0): with exactly one denominator zero the product is zero, so the relation
//       asks N = Dsig - Did = 0, which is false as the other denominator is not zero (for the lookup: qK Dt - M Dw = 0, false unless the one
//       multiplier that remains is zero, and then both definitions give 0) -- the relation cannot hold for either definition, the proof is
//       rejected either way, and what the helper holds there is of no consequence.  With BOTH zero the relation reads H 0 - 0 = 0, and 0
//       satisfies it; that is also what both old kernels give (0 - 0).
//
//   layout   the tile layout of wiring_fractions_kernel: a lane takes the kPlonkHelpersBatch rows base + 256 t of its block's tile of
//       256 kPlonkHelpersBatch, so every access of a wave is contiguous.  A row has four products P_0 .. P_3 (P_j = Did_j Dsig_j, P_3 = Dw Dt);
//       the running prefix product of the lane's 4 T of them is kept IN THE FOUR OUTPUT TABLES on the way forward (the prefix up to P_j of row i
//       in H_j[i]: pcs_quotient_kernel's MEM idiom, so that a lane's batch is not bounded by registers), the whole product is inverted once
//       (pcs_inverse), and on the way back each row's denominators are formed again from the inputs, column 3 first: its prefix is H_2[i], H_1[i],
//       H_0[i] and, for column 0, H_3[i - 256] -- each read before the lane overwrites it with the entry itself.  A zero product enters the
//       chain as 1 and its own output is selected to 0: no other entry sees it.  gamma id comes from the index: one product per lane for gamma
//       base, then additions of gamma 256 from row to row and of gamma n from wire to wire.
//       The rows are a rolled loop (unroll 1) and the four columns are unrolled by pcs_static_for: unrolled rows over small local arrays went to
//       scratch memory.
//
//   budget (by count)   per row, forward: gamma S_j 3, gamma B, gamma^2 C, gamma T1, gamma^2 T2 4, the four products 4, the chain 4: 15.  Back:
//       the same 11 to form the products again, qK Dt and M Dw 2, and per column the prefix's share, the chain's step and the numerator 12: 25.
//       The inversion: about 383 products a lane over 4 T = 64 products' worth of rows: 24 a row at T = 16.  About 64 a row, against about 228 for
//       the three wiring_fractions_kernel launches (56 each) with lookup_denominators_kernel and lookup_fractions_kernel (about 60).  34 accesses
//       of 32 bytes a row: 11 reads and 4 writes forward, 11 + 4 reads and 4 writes back.
#pragma once
#include "wiring.cuh"

namespace zk {

constexpr int kPlonkHelpersBatch = 16;                       // rows per lane: 64 products an inversion
constexpr int kPlonkHelpersIn = 11, kPlonkHelpersOut = 4;

// A, B, C, SA, SB, SC, qK, T0, T1, T2, M; then H0, H1, H2, HL: no output is an input's memory
enum { PH_A, PH_B, PH_C, PH_SA, PH_SB, PH_SC, PH_QK, PH_T0, PH_T1, PH_T2, PH_M };
struct PlonkHelpersTables {
    const void *in[kPlonkHelpersIn];
    void *out[kPlonkHelpersOut];
};

template <class F> struct PlonkHelpersConsts {
    Fe<F> beta, gamma, gamma2, gn, g256;                     // gn = gamma n (from one wire's ids to the next one's), g256 = gamma 256
};

// column J of row i: the product of its two denominators, and with NUM its numerator.  J < 3: wire J, gid = gamma (J n + i); J = 3: the lookup
template <class F, int J, bool NUM>
__device__ __forceinline__ void plonk_helpers_terms(const PlonkHelpersTables &tb, size_t i, const Fe<F> &beta, const Multiplier<F> &mg, const Multiplier<F> &mg2,
                                                    const Fe<F> &gid, Fe<F> &num, Fe<F> &prod) {
    if constexpr (J < 3) {
        Fe<F> did, dsig;
        wiring_denominators<F>(tb.in[PH_A + J], tb.in[PH_SA + J], i, beta, mg, gid, did, dsig);
        if (NUM) num = fe_sub<F>(dsig, did);
        prod = fe_mul_u<F>(did, dsig);
    } else {
        const Fe<F> dw = fe_add<F>(fe_add<F>(beta, fe_load<F>(tb.in[PH_A], i)), fe_add<F>(mg.times(fe_load<F>(tb.in[PH_B], i)), mg2.times(fe_load<F>(tb.in[PH_C], i))));
        const Fe<F> dt = fe_add<F>(fe_add<F>(beta, fe_load<F>(tb.in[PH_T0], i)), fe_add<F>(mg.times(fe_load<F>(tb.in[PH_T1], i)), mg2.times(fe_load<F>(tb.in[PH_T2], i))));
        if (NUM) num = fe_sub<F>(fe_mul_u<F>(fe_load<F>(tb.in[PH_QK], i), dt), fe_mul_u<F>(fe_load<F>(tb.in[PH_M], i), dw));
        prod = fe_mul_u<F>(dw, dt);
    }
}

// H0, H1, H2, HL at the rows x < n of the tables of n entries
template <class F> __global__ void __launch_bounds__(kPcsBlock) plonk_lookup_helpers_kernel(PlonkHelpersTables tb, size_t n, PlonkHelpersConsts<F> c) {
    constexpr int T = kPlonkHelpersBatch;
    const size_t base = (size_t)blockIdx.x * (T * kPcsBlock) + threadIdx.x;
    if (base >= n) return;
    const Multiplier<F> mg(c.gamma), mg2(c.gamma2);
    const Fe<F> one = fe_one<F>(), zero = fe_zero<F>();
    Fe<F> gid0 = mg.times(fe_from_u64<F>((uint64_t)base));   // gamma x of the row at hand
    Fe<F> acc = one;
    int rows = 0;
#pragma unroll 1
    for (int t = 0; t < T; t++) {
        const size_t i = base + (size_t)t * kPcsBlock;
        if (i >= n) break;
        Fe<F> gid = gid0;
        pcs_static_for(std::make_integer_sequence<int, kPlonkHelpersOut>{}, [&](auto jc) {
            constexpr int J = decltype(jc)::value;
            Fe<F> num, prod;
            plonk_helpers_terms<F, J, false>(tb, i, c.beta, mg, mg2, gid, num, prod);
            acc = fe_mul_u<F>(acc, wiring_select<F>(fe_is_zero<F>(prod), one, prod));
            fe_store<F>(tb.out[J], i, acc);
            if (J < 2) gid = fe_add<F>(gid, c.gn);
        });
        gid0 = fe_add<F>(gid0, c.g256);
        rows = t + 1;
    }
    Fe<F> inv = pcs_inverse<F>(acc);                         // 1 / the product of the lane's non-zero products
#pragma unroll 1
    for (int t = rows - 1; t >= 0; t--) {
        const size_t i = base + (size_t)t * kPcsBlock;
        gid0 = fe_sub<F>(gid0, c.g256);
        Fe<F> gid = fe_add<F>(gid0, fe_dbl<F>(c.gn));        // wire 2's
        pcs_static_for(std::make_integer_sequence<int, kPlonkHelpersOut>{}, [&](auto jc) {
            constexpr int J = kPlonkHelpersOut - 1 - decltype(jc)::value;
            Fe<F> num, prod;
            plonk_helpers_terms<F, J, true>(tb, i, c.beta, mg, mg2, gid, num, prod);
            const bool z = fe_is_zero<F>(prod);
            Fe<F> pinv = inv;                                // the lane's first product: nothing stands before it
            if (J > 0 || t > 0) {
                pinv = fe_mul_u<F>(inv, J > 0 ? fe_load<F>(tb.out[J > 0 ? J - 1 : 0], i) : fe_load<F>(tb.out[kPlonkHelpersOut - 1], i - (J > 0 ? 0 : kPcsBlock)));
                inv = fe_mul_u<F>(inv, wiring_select<F>(z, one, prod));
            }
            fe_store<F>(tb.out[J], i, wiring_select<F>(z, zero, fe_mul_u<F>(num, pinv)));
            if (J > 0 && J < 3) gid = fe_sub<F>(gid, c.gn);
        });
    }
}

}  // namespace zk
