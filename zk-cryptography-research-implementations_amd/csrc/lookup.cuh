// lookup.cuh -- the kernels of the lookup argument over FRI commitments (include/zkmle.h "Lookup: rows of a committed table"): the
// multiplicity count, the helper table of logarithmic derivatives and the round pass of its sumcheck.
//
//   multiplicities  M[y] = the number of witness rows x with qK[x] = 1 and (A, B, C)[x] = (T0, T1, T2)[y], credited to the smallest y of a
//               repeated row.  A hash table of `cap` = 2 n 32-bit slots (a power of two; all ones = empty) holds table-row indices: open
//               addressing, linear probing, the key the three elements as stored (the inputs are reduced, so equal elements are equal limbs).
//               The hash is murmur3's over all 3 N limbs with its final avalanche: nothing rests on how Montgomery form spreads small integers.
//                 insert   a lane per table row y: an empty slot is claimed by atomicCAS; a slot whose row equals the lane's own in all three
//                          columns and all limbs is lowered by atomicMin (only when y is below what the lane saw there: the slot only ever
//                          falls); any other slot is passed.  A slot never becomes empty again and the triple it stands for never changes,
//                          so every distinct triple ends in exactly one slot, whatever the arrival order, and that slot ends at the
//                          smallest index of the triple.
//                 count    (a later launch) a lane per witness row with qK = 1 probes the same way: at the slot of its triple it adds one to
//                          counts[slot's index], at an empty slot one to the miss counter.  A wave whose lanes all found one target adds
//                          once (the contended case of a table that is one row).
//                 finish   counts -> field elements in stored form.
//               Every probe loop is bounded by cap; a loop that runs out (it cannot: at most n of the 2 n slots are ever taken) sets the error
//               word and ends.
//   denominators  Dw = beta + A + gamma B + gamma^2 C and Dt = beta + T0 + gamma T1 + gamma^2 T2 into two columns of pool memory: a lane per
//               entry, 6 reads, 2 writes, 4 products.  With them the fractions kernel below reads four tables and is wiring_fractions_kernel
//               with two more products; reading the eight tables itself it would form the gamma products twice (forward and back: 8 products,
//               14 reads and a write an entry against 4, 12 reads and 3 writes) and hold two multipliers beside the sixteen prefix products.
//   fractions   H[x] = qK[x] inv0(Dw[x]) - M[x] inv0(Dt[x]), inv0(0) = 0: wiring_fractions_kernel's layout and Montgomery trick (a tile of
//               kPcsBlock x kLookupBatch entries, one pcs_inverse per lane, the denominators read again on the way back, a zero denominator
//               entered as 1 and selected to 0).  Per entry: 2 products for the prefix chain, 4 on the way back, 2 for qK and M, and a
//               sixteenth of a lane's inversion.
//   round       one pass per round over the ten tables A, B, C, qK, T0, T1, T2, M, H, E, in the idiom of wiring_round_kernel: lane i < q
//               folds each table's four entries to the pair (X[2i], X[2i+1]) and stores it (FOLD), or reads the pair (round 0).  Dw, Dt, H, qK,
//               M, E are lines in X per pair (Y_{k+1} = Y_k + (Y1 - Y0): additions only); gamma B, gamma^2 C, gamma T1, gamma^2 T2 at the
//               pair's two entries are the only products before the relation.  It accumulates
//                   s_k   += E_k (Dt_k (H_k Dw_k - qK_k) + M_k Dw_k)                    k = 0, 1, 2, 3
//                   s_inf += (E1 - E0)(H1 - H0)(Dw1 - Dw0)(Dt1 - Dt0)                   the X^4 coefficient: only E H Dw Dt has a share in it
//                   s_ev  += H[2i],    s_od += H[2i+1]
//               and the host adds mu times the line through s_ev, s_od (wiring_message).  Products per lane: 2 per table folded (20), the
//               gamma products 8, the infinity term 3, four per node (16): 47 in the fold form, 27 in round 0's.  40 reads and 20 writes of
//               32 bytes in the fold form; 20 reads in round 0's.  The seven sums are Wide (one plain addition a term, up to 2^32 terms: no
//               raw-product accumulator and so no kRawTermsMax bound applies).  The folded tables are one block (a base and a stride); beta,
//               gamma and gamma^2 wait in LDS as the wiring's uniform elements do: twenty pointers, the fold's multiplier and the modulus
//               leave the scalar registers no room for three more elements and two more multipliers.
#pragma once
#include "wiring.cuh"

namespace zk {

constexpr int kLookupBatch = 8;                              // entries per lane of the fractions kernel: 16 denominators an inversion
constexpr uint32_t kLookupEmpty = 0xFFFFFFFFu, kLookupNone = 0xFFFFFFFEu;   // an empty slot; a lane that looks nothing up

struct LookupStatus {                                        // one block of device memory, zero before the first launch
    unsigned long long misses;
    uint32_t error;
    uint32_t pad;
};

__device__ __forceinline__ uint32_t lookup_rotl(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }
template <class F> __device__ __forceinline__ uint32_t lookup_mix(uint32_t h, const Fe<F> &a) {
#pragma unroll
    for (int k = 0; k < F::N; k++) {
        uint32_t w = a.l[k] * 0xCC9E2D51u;
        w = lookup_rotl(w, 15) * 0x1B873593u;
        h = lookup_rotl(h ^ w, 13) * 5u + 0xE6546B64u;
    }
    return h;
}
// murmur3 (x86_32) over the 3 N limbs of the triple
template <class F> __device__ __forceinline__ uint32_t lookup_hash(const Fe<F> &a, const Fe<F> &b, const Fe<F> &c) {
    uint32_t h = lookup_mix<F>(lookup_mix<F>(lookup_mix<F>(0x5EEDu, a), b), c) ^ (uint32_t)(12 * F::N);
    h = (h ^ (h >> 16)) * 0x85EBCA6Bu;
    h = (h ^ (h >> 13)) * 0xC2B2AE35u;
    return h ^ (h >> 16);
}
template <class F> __device__ __forceinline__ bool lookup_same(const Fe<F> &a, const Fe<F> &b) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < F::N; k++) v |= a.l[k] ^ b.l[k];
    return v == 0;
}
// row y of the table equals (a, b, c)
template <class F> __device__ __forceinline__ bool lookup_row_is(const void *__restrict__ T0, const void *__restrict__ T1, const void *__restrict__ T2, size_t y,
                                                                const Fe<F> &a, const Fe<F> &b, const Fe<F> &c) {
    return lookup_same<F>(fe_load<F>(T0, y), a) && lookup_same<F>(fe_load<F>(T1, y), b) && lookup_same<F>(fe_load<F>(T2, y), c);
}

// slots: cap words, all ones.  cap is a power of two, cap >= 2 n, n <= 2^31
template <class F> __global__ void __launch_bounds__(kBlock) lookup_insert_kernel(const void *__restrict__ T0, const void *__restrict__ T1, const void *__restrict__ T2, size_t n,
                                                                                 uint32_t *__restrict__ slots, size_t cap, LookupStatus *__restrict__ st) {
    const size_t y = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (y >= n) return;
    const Fe<F> a = fe_load<F>(T0, y), b = fe_load<F>(T1, y), c = fe_load<F>(T2, y);
    const size_t mask = cap - 1;
    size_t s = lookup_hash<F>(a, b, c) & mask;
    for (size_t probe = 0; probe < cap; probe++, s = (s + 1) & mask) {
        uint32_t cur = __hip_atomic_load(&slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kLookupEmpty) {
            cur = atomicCAS(&slots[s], kLookupEmpty, (uint32_t)y);
            if (cur == kLookupEmpty) return;                 // claimed
        }
        if (cur < n && lookup_row_is<F>(T0, T1, T2, cur, a, b, c)) {
            if ((uint32_t)y < cur) atomicMin(&slots[s], (uint32_t)y);
            return;
        }
    }
    atomicOr(&st->error, 1u);
}

// counts: n words, zero.  one = the field's one as stored.  After lookup_insert_kernel has ended
template <class F> __global__ void __launch_bounds__(kBlock) lookup_count_kernel(const void *__restrict__ A, const void *__restrict__ B, const void *__restrict__ C,
                                                                                const void *__restrict__ QK, const void *__restrict__ T0, const void *__restrict__ T1,
                                                                                const void *__restrict__ T2, size_t n, const uint32_t *__restrict__ slots, size_t cap,
                                                                                uint32_t *__restrict__ counts, LookupStatus *__restrict__ st) {
    const size_t x = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (x >= n) return;
    uint32_t target = kLookupNone;
    bool lost = false;
    if (lookup_same<F>(fe_load<F>(QK, x), fe_one<F>())) {
        const Fe<F> a = fe_load<F>(A, x), b = fe_load<F>(B, x), c = fe_load<F>(C, x);
        const size_t mask = cap - 1;
        size_t s = lookup_hash<F>(a, b, c) & mask;
        lost = true;
        for (size_t probe = 0; probe < cap; probe++, s = (s + 1) & mask) {
            const uint32_t cur = slots[s];
            if (cur == kLookupEmpty || (cur < n && lookup_row_is<F>(T0, T1, T2, cur, a, b, c))) {
                target = cur;
                lost = false;
                break;
            }
        }
    }
    if (lost) atomicOr(&st->error, 2u);
    // the wave's lanes that are here (the last wave of the grid may be short)
    const unsigned long long here = __ballot(1);
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)target);
    if (__ballot(target == first) == here) {                 // one target for the whole wave: one addition
        if (first != kLookupNone && (unsigned)__lane_id() == (unsigned)__ffsll((long long)here) - 1u) {
            const uint32_t k = (uint32_t)__popcll(here);
            if (first == kLookupEmpty) atomicAdd(&st->misses, (unsigned long long)k);
            else atomicAdd(&counts[first], k);
        }
        return;
    }
    if (target == kLookupEmpty) atomicAdd(&st->misses, 1ull);
    else if (target != kLookupNone) atomicAdd(&counts[target], 1u);
}

template <class F> __global__ void __launch_bounds__(kBlock) lookup_finish_kernel(const uint32_t *__restrict__ counts, size_t n, void *__restrict__ M) {
    const size_t y = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (y < n) fe_store<F>(M, y, fe_from_u64<F>((uint64_t)counts[y]));
}

// DW[x] = beta + X0[x] + gamma X1[x] + gamma^2 X2[x] for the wires and DT the same for the table's columns; DW, DT are no input's memory
template <class F> __global__ void __launch_bounds__(kBlock) lookup_denominators_kernel(const void *__restrict__ A, const void *__restrict__ B, const void *__restrict__ C,
                                                                                       const void *__restrict__ T0, const void *__restrict__ T1, const void *__restrict__ T2,
                                                                                       void *__restrict__ DW, void *__restrict__ DT, size_t n, Fe<F> beta, Fe<F> gamma,
                                                                                       Fe<F> gamma2) {
    const size_t x = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (x >= n) return;
    const Multiplier<F> mg(gamma), mg2(gamma2);
    fe_store<F>(DW, x, fe_add<F>(fe_add<F>(beta, fe_load<F>(A, x)), fe_add<F>(mg.times(fe_load<F>(B, x)), mg2.times(fe_load<F>(C, x)))));
    fe_store<F>(DT, x, fe_add<F>(fe_add<F>(beta, fe_load<F>(T0, x)), fe_add<F>(mg.times(fe_load<F>(T1, x)), mg2.times(fe_load<F>(T2, x)))));
}

// H[x] = qK[x] inv0(DW[x]) - M[x] inv0(DT[x]) for x < n.  H is no input's memory.
template <class F> __global__ void __launch_bounds__(kPcsBlock) lookup_fractions_kernel(const void *__restrict__ DW, const void *__restrict__ DT, const void *__restrict__ QK,
                                                                                       const void *__restrict__ M, void *__restrict__ H, size_t n) {
    constexpr int T = kLookupBatch;
    const size_t base = (size_t)blockIdx.x * (T * kPcsBlock) + threadIdx.x;
    if (base >= n) return;
    const Fe<F> one = fe_one<F>(), zero = fe_zero<F>();
    Fe<F> pre[2 * T];
    Fe<F> acc = one;
    pcs_static_for(std::make_integer_sequence<int, T>{}, [&](auto tc) {
        constexpr int t = decltype(tc)::value;
        const size_t i = base + (size_t)t * kPcsBlock;
        if (i < n) {
            Fe<F> dw = fe_load<F>(DW, i), dt = fe_load<F>(DT, i);
            dw = wiring_select<F>(fe_is_zero<F>(dw), one, dw);
            dt = wiring_select<F>(fe_is_zero<F>(dt), one, dt);
            acc = t == 0 ? dw : fe_mul_u<F>(acc, dw);
            pre[2 * t] = acc;
            acc = fe_mul_u<F>(acc, dt);
            pre[2 * t + 1] = acc;
        }
    });
    Fe<F> inv = pcs_inverse<F>(acc);                         // 1 / the product of the lane's non-zero denominators
    pcs_static_for(std::make_integer_sequence<int, T>{}, [&](auto tc) {
        constexpr int t = T - 1 - decltype(tc)::value;
        const size_t i = base + (size_t)t * kPcsBlock;
        if (i < n) {
            const Fe<F> dw = fe_load<F>(DW, i), dt = fe_load<F>(DT, i);
            const bool zw = fe_is_zero<F>(dw), zt = fe_is_zero<F>(dt);
            const Fe<F> idt = fe_mul_u<F>(inv, pre[2 * t]);
            inv = fe_mul_u<F>(inv, wiring_select<F>(zt, one, dt));
            Fe<F> idw = inv;
            if (t > 0) {
                idw = fe_mul_u<F>(inv, pre[t > 0 ? 2 * t - 1 : 0]);
                inv = fe_mul_u<F>(inv, wiring_select<F>(zw, one, dw));
            }
            fe_store<F>(H, i, fe_sub<F>(fe_mul_u<F>(fe_load<F>(QK, i), wiring_select<F>(zw, zero, idw)), fe_mul_u<F>(fe_load<F>(M, i), wiring_select<F>(zt, zero, idt))));
        }
    });
}

// the ten tables of a pass, in the order A, B, C, qK, T0, T1, T2, M, H, E.  The folded tables are one block: table j at out0 + j ostride bytes
enum { LOOKUP_A, LOOKUP_B, LOOKUP_C, LOOKUP_QK, LOOKUP_T0, LOOKUP_T1, LOOKUP_T2, LOOKUP_M, LOOKUP_H, LOOKUP_E, LOOKUP_TABLES };
typedef WiringTables LookupTables;
template <class F> struct LookupConsts {
    Fe<F> beta, gamma, gamma2;
};
enum { LOOKUP_BETA, LOOKUP_GAMMA, LOOKUP_GAMMA2, LOOKUP_UNIFORM };

// the line beta + X + gamma Y + gamma^2 Z at the pair: its value at the even entry and its step
template <class F, bool FOLD, int X>
__device__ __forceinline__ void lookup_denominator_line(const LookupTables &t, size_t i, const Multiplier<F> &mr, const WiringUniform<F> &cs, Fe<F> &d0, Fe<F> &dd) {
    Fe<F> x0, x1, d1;
    zerocheck_pair<F, FOLD>(t.in[X], t.out(X), i, mr, x0, x1);
    {
        const Fe<F> beta = cs[LOOKUP_BETA];
        d0 = fe_add<F>(beta, x0);
        d1 = fe_add<F>(beta, x1);
    }
    zerocheck_pair<F, FOLD>(t.in[X + 1], t.out(X + 1), i, mr, x0, x1);
    {
        const Multiplier<F> mg(cs[LOOKUP_GAMMA]);
        d0 = fe_add<F>(d0, mg.times(x0));
        d1 = fe_add<F>(d1, mg.times(x1));
    }
    zerocheck_pair<F, FOLD>(t.in[X + 2], t.out(X + 2), i, mr, x0, x1);
    {
        const Multiplier<F> mg2(cs[LOOKUP_GAMMA2]);
        d0 = fe_add<F>(d0, mg2.times(x0));
        d1 = fe_add<F>(d1, mg2.times(x1));
    }
    dd = fe_sub<F>(d1, d0);
}

// partials[X * gridDim.x + block] = the block's share of sum X, X < 7 (s_0, s_1, s_2, s_3, s_inf, s_ev, s_od); q, FOLD and the tables'
// lengths as in zerocheck_mul_round_kernel.  Two waves a SIMD, as the wiring's pass.
template <class F, bool FOLD> __global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) lookup_round_kernel(LookupTables t, size_t q, Fe<F> r, LookupConsts<F> c, void *__restrict__ partials) {
    __shared__ Wide<F> sh[7 * kBlock / 64];
    __shared__ WiringWord4 csh[2 * LOOKUP_UNIFORM];
    if (threadIdx.x == 0) {
        const auto put = [&](int k, const Fe<F> &e) {
            csh[2 * k] = WiringWord4{e.l[0], e.l[1], e.l[2], e.l[3]};
            csh[2 * k + 1] = WiringWord4{e.l[4], e.l[5], e.l[6], e.l[7]};
        };
        put(LOOKUP_BETA, c.beta);
        put(LOOKUP_GAMMA, c.gamma);
        put(LOOKUP_GAMMA2, c.gamma2);
    }
    __syncthreads();
    const WiringUniform<F> cs{(const volatile __attribute__((address_space(3))) WiringWord4 *)csh};
    const size_t stride = (size_t)gridDim.x * kBlock, first = (size_t)blockIdx.x * kBlock + threadIdx.x;
    Wide<F> sum[7] = {wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>()};
    const Multiplier<F> mr(r);
    for (size_t i = first; i < q; i += stride) {
        Fe<F> e, de, x1;
        zerocheck_pair<F, FOLD>(t.in[LOOKUP_E], t.out(LOOKUP_E), i, mr, e, x1);
        de = fe_sub<F>(x1, e);
        Fe<F> dw, ddw, dt, ddt;
        lookup_denominator_line<F, FOLD, LOOKUP_A>(t, i, mr, cs, dw, ddw);
        __builtin_amdgcn_sched_barrier(0);                    // a line at a time: left alone the scheduler requests the next line's tables ahead
        lookup_denominator_line<F, FOLD, LOOKUP_T0>(t, i, mr, cs, dt, ddt);
        __builtin_amdgcn_sched_barrier(0);
        Fe<F> h, dh;
        zerocheck_pair<F, FOLD>(t.in[LOOKUP_H], t.out(LOOKUP_H), i, mr, h, x1);
        wide_add_fe<F>(sum[5], h);
        wide_add_fe<F>(sum[6], x1);
        dh = fe_sub<F>(x1, h);
        wide_add_fe<F>(sum[4], fe_mul<F>(de, fe_mul<F>(dh, fe_mul<F>(ddw, ddt))));
        Fe<F> k, dk, m, dm;
        zerocheck_pair<F, FOLD>(t.in[LOOKUP_QK], t.out(LOOKUP_QK), i, mr, k, x1);
        dk = fe_sub<F>(x1, k);
        zerocheck_pair<F, FOLD>(t.in[LOOKUP_M], t.out(LOOKUP_M), i, mr, m, x1);
        dm = fe_sub<F>(x1, m);
        const auto node = [&](Wide<F> &sk, bool last) {
            wide_add_fe<F>(sk, fe_mul<F>(e, fe_add<F>(fe_mul<F>(dt, fe_sub<F>(fe_mul<F>(h, dw), k)), fe_mul<F>(m, dw))));
            if (last) return;
            e = fe_add<F>(e, de);
            dw = fe_add<F>(dw, ddw);
            dt = fe_add<F>(dt, ddt);
            h = fe_add<F>(h, dh);
            k = fe_add<F>(k, dk);
            m = fe_add<F>(m, dm);
        };
        node(sum[0], false);
        node(sum[1], false);
        node(sum[2], false);
        node(sum[3], true);
        __builtin_amdgcn_sched_barrier(0);
    }
    Fe<F> tot;
    if (block_reduce_wide<F, 7>(sum, sh, tot)) fe_store<F>(partials, (size_t)threadIdx.x * gridDim.x + blockIdx.x, tot);
}

}  // namespace zk
