// plonk_lookup.cuh -- the round pass of the Plonk proof with lookup rows (include/zkmle.h "Plonk with lookups: gate, wiring, public inputs and
// lookup rows in one sumcheck"): plonk.cuh's pass with a fifth phase.  ONE pass per round over the twenty-one tables A, B, C, qM, qL, qR, qO, qC,
// SA, SB, SC, qK, T0, T1, T2, M, H0, H1, H2, HL, E, in the idiom of plonk_round_kernel: grid-stride over the q pairs, zerocheck_pair, seven Wide
// lazy sums, block_reduce_wide<F, 7>, then finish_sums_kernel; the host's wiring_message is unchanged.
//
//   round   plonk_round_kernel's sums (plonk.cuh), and with Dw = beta + A + gamma B + gamma^2 C, Dt = beta + T0 + gamma T1 + gamma^2 T2 as lines
//           at the pair and Y_k the pair's line at the node k,
//               s_k   += alpha^4 E_k (Dt_k (HL_k Dw_k - qK_k) + M_k Dw_k)                  k = 0 .. 3
//               s_inf += alpha^4 (E1 - E0)(HL1 - HL0)(Dw1 - Dw0)(Dt1 - Dt0)
//               s_ev  += mu HL[2i],    s_od += mu HL[2i+1]
//           The host multiplies the line through (s_ev, s_od) by mu (wiring_message), so HL enters the message as mu^2 HL beside
//           mu (H0 + H1 + H2): seven sums, not nine, for two products by the uniform mu.  (Nine sums were not tried: seven fit, see below.)
//   schedule  the gate, then wires 0, 1, 2 (plonk.cuh's own phases on this pass's argument block), then the lookup: the line alpha^2 E that wire
//           2 ran on is multiplied by alpha^2 (two products); A, B, C for Dw are NOT folded again, they are read back through plonk_pair_again
//           as the wires read them; T0, T1, T2, HL, qK and M fold and store.  lookup_round_kernel's arithmetic: the denominators' lines with
//           gamma and gamma^2 as multipliers from LDS, the factored node, the infinity term.  Between the phases only the line of E, gamma id
//           and the seven sums are live; a sched_barrier stands between them.
//   budget  (by count, not measured)  products per lane in the fold form: 2 per table folded (42), the gate's 25 and the wires' 55 of plonk.cuh,
//           and the lookup's 31: alpha^2 on the line of E 2, gamma B, gamma^2 C, gamma T1, gamma^2 T2 at two entries 8, mu HL 2, the infinity
//           term 3, four per node 16.  42 + 25 + 55 + 31 = 153 (plonk_round_kernel 110 + lookup_round_kernel 47 = 157 for the pair); 111 in
//           round 0's form.
//           Accesses of 32 bytes per lane: 84 reads and 42 writes reach HBM in the fold form (42 reads in round 0's) -- the pair of passes has
//           100 and 50 -- and 12 reads of the pairs of A, B, C that the lane itself touched earlier in the iteration (6 by the wires, 6 by Dw).
//   registers  as plonk.cuh: the folded tables are one block (a base and a stride), table j's input pointer is read from the argument segment
//           where it is used (one 8-byte scalar load at 8 j, j < 21: `in` is the first member of the first argument, static_assert below),
//           and ten uniform elements wait in LDS behind an LDS-typed pointer: plonk.cuh's seven, gamma^2, alpha^2 and mu.
//           amdgpu_waves_per_eu(2, 2) holds the allocator to 256 registers; profiles/plonk_lookup/kernel_resource_usage.txt has the compiler's
//           report for the four instantiations.
#pragma once
#include "plonk.cuh"

namespace zk {

constexpr int kPlonkLookupTables = 21;

struct PlonkLookupTables {
    const void *in[kPlonkLookupTables];
    void *out0;
    size_t ostride;
    __device__ __forceinline__ void *out(int j) const { return (char *)out0 + (size_t)j * ostride; }
};
static_assert(__builtin_offsetof(PlonkLookupTables, in) == 0 && sizeof(PlonkLookupTables) == 8 * kPlonkLookupTables + 16,
              "plonk_in reads in[j], 8 bytes at 8 j, at the start of the argument segment");

// the places of the twenty-one; the first eleven are plonk.cuh's
enum { PLOOK_QK = 11, PLOOK_T0 = 12, PLOOK_T1, PLOOK_T2, PLOOK_M = 15, PLOOK_H = 16, PLOOK_HL = 19, PLOOK_E = 20 };

// the pass's uniform values: PlonkConsts' with gamma^2, alpha^2 and mu
template <class F> struct PlonkLookupConsts {
    Fe<F> beta, gamma, alpha, alpha3, gid0, gstep, gwire, gnext, gamma2, alpha2, mu;
};
// the uniform elements that wait in LDS: plonk.cuh's seven at their places, then three more
template <class F> struct PlonkLookupUniform : PlonkUniform<F> {
    enum { GAMMA2 = PlonkUniform<F>::COUNT, ALPHA2, MU, COUNT_ALL };
};

// one term of the line beta + X + gamma Y + gamma^2 Z at the pair: (d0, d1) += cs[which] (x0, x1), which = GAMMA or GAMMA2 (lookup_denominator_line's
// arithmetic, a term at a time: two of the three pairs are read back here and not folded)
template <class F, class U> __device__ __forceinline__ void plonk_lookup_line_add(const U &cs, int which, const Fe<F> &x0, const Fe<F> &x1, Fe<F> &d0, Fe<F> &d1) {
    const Multiplier<F> m(cs[which]);
    d0 = fe_add<F>(d0, m.times(x0));
    d1 = fe_add<F>(d1, m.times(x1));
}

// the lookup's share of the seven sums on the line (e, de) = alpha^4 E at the pair
template <class F, bool FOLD>
__device__ __forceinline__ void plonk_lookup_phase(const PlonkLookupTables &t, size_t i, const Multiplier<F> &mr, const PlonkLookupUniform<F> &cs, Fe<F> e, const Fe<F> &de,
                                                   Wide<F> &s0, Wide<F> &s1, Wide<F> &s2, Wide<F> &s3, Wide<F> &sinf, Wide<F> &sev, Wide<F> &sod) {
    using U = PlonkLookupUniform<F>;
    using T = PlonkLookupTables;
    Fe<F> x0, x1, dw, ddw, dt, ddt;
    {                                                         // Dw from the pairs of A, B, C the gate left
        Fe<F> d1;
        plonk_pair_again<F, FOLD, PLONK_A, T>(t, i, x0, x1);
        {
            const Fe<F> beta = cs[U::BETA];
            dw = fe_add<F>(beta, x0);
            d1 = fe_add<F>(beta, x1);
        }
        plonk_pair_again<F, FOLD, PLONK_B, T>(t, i, x0, x1);
        plonk_lookup_line_add<F>(cs, U::GAMMA, x0, x1, dw, d1);
        plonk_pair_again<F, FOLD, PLONK_C, T>(t, i, x0, x1);
        plonk_lookup_line_add<F>(cs, U::GAMMA2, x0, x1, dw, d1);
        ddw = fe_sub<F>(d1, dw);
    }
    __builtin_amdgcn_sched_barrier(0);                        // a line at a time, as lookup_round_kernel
    {                                                         // Dt: T0, T1, T2 fold and store
        Fe<F> d1;
        zerocheck_pair<F, FOLD>(plonk_in(PLOOK_T0), t.out(PLOOK_T0), i, mr, x0, x1);
        {
            const Fe<F> beta = cs[U::BETA];
            dt = fe_add<F>(beta, x0);
            d1 = fe_add<F>(beta, x1);
        }
        zerocheck_pair<F, FOLD>(plonk_in(PLOOK_T1), t.out(PLOOK_T1), i, mr, x0, x1);
        plonk_lookup_line_add<F>(cs, U::GAMMA, x0, x1, dt, d1);
        zerocheck_pair<F, FOLD>(plonk_in(PLOOK_T2), t.out(PLOOK_T2), i, mr, x0, x1);
        plonk_lookup_line_add<F>(cs, U::GAMMA2, x0, x1, dt, d1);
        ddt = fe_sub<F>(d1, dt);
    }
    __builtin_amdgcn_sched_barrier(0);
    Fe<F> h, dh;
    zerocheck_pair<F, FOLD>(plonk_in(PLOOK_HL), t.out(PLOOK_HL), i, mr, h, x1);
    {
        const Multiplier<F> mm(cs[U::MU]);                    // mu HL: the host's mu makes it mu^2 HL
        wide_add_fe<F>(sev, mm.times(h));
        wide_add_fe<F>(sod, mm.times(x1));
    }
    dh = fe_sub<F>(x1, h);
    wide_add_fe<F>(sinf, fe_mul<F>(de, fe_mul<F>(dh, fe_mul<F>(ddw, ddt))));
    Fe<F> k, dk, m, dm;
    zerocheck_pair<F, FOLD>(plonk_in(PLOOK_QK), t.out(PLOOK_QK), i, mr, k, x1);
    dk = fe_sub<F>(x1, k);
    zerocheck_pair<F, FOLD>(plonk_in(PLOOK_M), t.out(PLOOK_M), i, mr, m, x1);
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
    node(s0, false);
    node(s1, false);
    node(s2, false);
    node(s3, true);
}

// partials[X * gridDim.x + block] = the block's share of sum X, X < 7 (s_0, s_1, s_2, s_3, s_inf, s_ev, s_od); q, FOLD and the tables' lengths as
// in zerocheck_mul_round_kernel.  Two waves a SIMD, as plonk_round_kernel.
template <class F, bool FOLD> __global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) plonk_lookup_round_kernel(PlonkLookupTables t, size_t q, Fe<F> r, PlonkLookupConsts<F> c, void *__restrict__ partials) {
    using U = PlonkLookupUniform<F>;
    using T = PlonkLookupTables;
    __shared__ Wide<F> sh[7 * kBlock / 64];
    __shared__ WiringWord4 csh[2 * U::COUNT_ALL];
    __shared__ WiringWord4 gsh[2 * kBlock];                   // a lane's gamma id waits here through the lookup's phase: 8 KiB
    if (threadIdx.x == 0) {
        const auto put = [&](int k, const Fe<F> &e) {
            csh[2 * k] = WiringWord4{e.l[0], e.l[1], e.l[2], e.l[3]};
            csh[2 * k + 1] = WiringWord4{e.l[4], e.l[5], e.l[6], e.l[7]};
        };
        put(U::BETA, c.beta);
        put(U::GAMMA, c.gamma);
        put(U::ALPHA, c.alpha);
        put(U::ALPHA3, c.alpha3);
        put(U::GSTEP, c.gstep);
        put(U::GWIRE, c.gwire);
        put(U::GNEXT, c.gnext);
        put(U::GAMMA2, c.gamma2);
        put(U::ALPHA2, c.alpha2);
        put(U::MU, c.mu);
    }
    __syncthreads();
    const U cs{{(const volatile __attribute__((address_space(3))) WiringWord4 *)csh}};
    const size_t stride = (size_t)gridDim.x * kBlock, first = (size_t)blockIdx.x * kBlock + threadIdx.x;
    Wide<F> sum[7] = {wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>()};
    const Multiplier<F> mr(r);
    volatile __attribute__((address_space(3))) WiringWord4 *const gs = (volatile __attribute__((address_space(3))) WiringWord4 *)gsh + 2 * threadIdx.x;
    // gamma id_0 at the lane's first pair: gamma (c_l + 2^l 2 first)
    Fe<F> gid = fe_add<F>(c.gid0, fe_mul<F>(fe_dbl<F>(c.gstep), fe_from_u64<F>((uint64_t)first)));
    for (size_t i = first; i < q; i += stride) {
        Fe<F> e0, de;
        plonk_gate<F, FOLD, T, PLOOK_E>(t, i, mr, cs, e0, de, sum[0], sum[1], sum[2], sum[3], sum[4]);
        __builtin_amdgcn_sched_barrier(0);                    // a phase at a time, as plonk_round_kernel
        plonk_wire<F, FOLD, 0, T, PLOOK_H>(t, i, mr, cs, gid, e0, de, sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6]);
        __builtin_amdgcn_sched_barrier(0);
        gid = fe_add<F>(gid, cs[U::GWIRE]);
        {
            const Multiplier<F> ma(cs[U::ALPHA]);
            e0 = ma.times(e0);
            de = ma.times(de);
        }
        plonk_wire<F, FOLD, 1, T, PLOOK_H>(t, i, mr, cs, gid, e0, de, sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6]);
        __builtin_amdgcn_sched_barrier(0);
        gid = fe_add<F>(gid, cs[U::GWIRE]);
        {
            const Multiplier<F> ma(cs[U::ALPHA]);
            e0 = ma.times(e0);
            de = ma.times(de);
        }
        plonk_wire<F, FOLD, 2, T, PLOOK_H>(t, i, mr, cs, gid, e0, de, sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6]);
        __builtin_amdgcn_sched_barrier(0);
        gid = fe_add<F>(gid, cs[U::GNEXT]);
        // the lookup needs no id: gamma id leaves the registers for the phase (the lane's own 32 bytes of LDS; with it live the fold form of
        // BLS12-381 Fr spilled two registers)
        gs[0] = WiringWord4{gid.l[0], gid.l[1], gid.l[2], gid.l[3]};
        gs[1] = WiringWord4{gid.l[4], gid.l[5], gid.l[6], gid.l[7]};
        {
            const Multiplier<F> ma2(cs[U::ALPHA2]);           // alpha^2 E -> alpha^4 E
            e0 = ma2.times(e0);
            de = ma2.times(de);
        }
        plonk_lookup_phase<F, FOLD>(t, i, mr, cs, e0, de, sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6]);
        __builtin_amdgcn_sched_barrier(0);
        {
            const WiringWord4 a = gs[0], b = gs[1];
            gid.l[0] = a.x; gid.l[1] = a.y; gid.l[2] = a.z; gid.l[3] = a.w;
            gid.l[4] = b.x; gid.l[5] = b.y; gid.l[6] = b.z; gid.l[7] = b.w;
        }
    }
    Fe<F> tot;
    if (block_reduce_wide<F, 7>(sum, sh, tot)) fe_store<F>(partials, (size_t)threadIdx.x * gridDim.x + blockIdx.x, tot);
}

}  // namespace zk
