// plonk.cuh -- the round pass of the Plonk proof (include/zkmle.h "Plonk: gate, wiring and public inputs in one sumcheck"): the gate's zerocheck
// (zerocheck.cuh) and the wiring's sumcheck (wiring.cuh) in ONE pass per round over the fifteen tables A, B, C, qM, qL, qR, qO, qC, SA, SB, SC, H0,
// H1, H2, E, in the idiom of wiring_round_kernel: grid-stride over the q pairs, zerocheck_pair, seven Wide lazy sums, block_reduce_wide<F, 7>, then
// finish_sums_kernel; the host's wiring_message is unchanged.  The public inputs are in no table and in no kernel: they are the claimed sum.
//
//   round   lane i < q folds each table's four entries to the pair (X[2i], X[2i+1]) and stores it (FOLD), or reads the pair (round 0), and
//           accumulates, with Y_k the pair's line at the node k,
//               s_k   += E_k [ sum_j alpha^j (H_j,k Did_j,k Dsig_j,k - N_j,k) + alpha^3 ((qM_k B_k + qL_k) A_k + qR_k B_k + qO_k C_k + qC_k) ]      k = 0 .. 3
//               s_inf += (E1 - E0) [ sum_j alpha^j (H_j1 - H_j0)(Did_j1 - Did_j0)(Dsig_j1 - Dsig_j0) + alpha^3 (qM1 - qM0)(A1 - A0)(B1 - B0) ]
//               s_ev  += H_0[2i] + H_1[2i] + H_2[2i],    s_od += H_0[2i+1] + H_1[2i+1] + H_2[2i+1]
//           (Did, Dsig, N as in wiring.cuh; only qM A B has a share in the gate's X^4 coefficient).
//   schedule  the gate first, in zerocheck_gate_round_kernel's order B, qR, qM, qL, A, qO, C, qC: its running values u_k, v_k and the infinity
//           term die into the five zerocheck sums as soon as E is there, scaled by the line alpha^3 E (alpha^3 comes from the host: two products).
//           Then the three wires as in wiring_round_kernel, each multiplied by its line alpha^j E at once, so that only the line of E and gamma id
//           live from one phase to the next.  A, B, C were folded and stored by the gate; a wire does NOT form its pair again and does not keep it
//           across the gate either (six more live elements cost the pass its registers): it reads the pair back, two entries that the same lane
//           stored (FOLD) or read (round 0) a phase earlier, through a pointer the compiler is told nothing about (no __restrict__, and laundered,
//           so that it neither forwards the stored value -- which would keep it live -- nor reorders the read before the store).
//   budget  products per lane: 2 per table folded (30), the gate's 16 node products, 2 for its infinity term, 2 for alpha^3 E and 5 into the
//           sums (25), the wires' 55 of wiring.cuh:  110 in the fold form, 80 in round 0's.  Accesses of 32 bytes per lane: 60 reads and 30 writes
//           in the fold form, 30 reads in round 0's -- every table entry comes from HBM once a round -- and 6 reads of the pair of A, B, C that the
//           lane itself touched a phase earlier: 96 (36) instructions, of which 6 are served by the cache.
//   registers  the folded tables are one block (a base and a stride) and seven uniform elements wait in LDS behind an LDS-typed pointer, as in
//           wiring.cuh; amdgpu_waves_per_eu(2, 2) holds the allocator to 256 registers.
#pragma once
#include "wiring.cuh"

namespace zk {

constexpr int kPlonkTables = 15;

// the fifteen tables of a pass, in the order A, B, C, qM, qL, qR, qO, qC, SA, SB, SC, H0, H1, H2, E.  The folded tables are one block: table j at
// out0 + j ostride bytes
struct PlonkTables {
    const void *in[kPlonkTables];
    void *out0;
    size_t ostride;
    __device__ __forceinline__ void *out(int j) const { return (char *)out0 + (size_t)j * ostride; }
};
// The fifteen input pointers do not stay in scalar registers through the loop (thirty of 102, beside the fold's multiplier, the modulus and the
// block of the folded tables: the fold form spilled two): table j's is read from the kernel's argument segment where it is used -- PlonkTables is
// the kernel's first argument and `in` its first member -- through a laundered pointer, so that the reads are not gathered in front of the loop again.
static_assert(__builtin_offsetof(PlonkTables, in) == 0, "plonk_in reads in[j] at the start of the argument segment");
typedef const void __attribute__((address_space(1))) *PlonkGlobal;   // global by its type: what comes out of a laundering would be a flat access
__device__ __forceinline__ const void *plonk_in(int j) {
    const PlonkGlobal __attribute__((address_space(4))) *ka = (const PlonkGlobal __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    return (const void *)ka[j];
}
// the pass's uniform values: WiringConsts' and alpha^3
template <class F> struct PlonkConsts {
    Fe<F> beta, gamma, alpha, alpha3, gid0, gstep, gwire, gnext;
};

// the uniform elements that wait in LDS (wiring.cuh's WiringUniform with alpha^3)
template <class F> struct PlonkUniform {
    static_assert(F::N == 8, "two 16-byte reads an element");
    enum { BETA, GAMMA, ALPHA, ALPHA3, GSTEP, GWIRE, GNEXT, COUNT };
    const volatile __attribute__((address_space(3))) WiringWord4 *w;
    __device__ __forceinline__ Fe<F> operator[](int k) const {
        const WiringWord4 a = w[2 * k], b = w[2 * k + 1];
        Fe<F> o;
        o.l[0] = a.x; o.l[1] = a.y; o.l[2] = a.z; o.l[3] = a.w;
        o.l[4] = b.x; o.l[5] = b.y; o.l[6] = b.z; o.l[7] = b.w;
        return o;
    }
};

enum { PLONK_A, PLONK_B, PLONK_C, PLONK_QM, PLONK_QL, PLONK_QR, PLONK_QO, PLONK_QC, PLONK_S, PLONK_H = 11, PLONK_E = 14 };

// the gate's share of the five zerocheck sums; (e0, de) = the line of E at the pair, which the wires go on with.  T, E_AT: the pass's argument
// block and E's place in it (plonk_lookup.cuh has a longer block; the gate's eight tables stand first in both)
template <class F, bool FOLD, class T = PlonkTables, int E_AT = PLONK_E>
__device__ __forceinline__ void plonk_gate(const T &t, size_t i, const Multiplier<F> &mr, const PlonkUniform<F> &cs, Fe<F> &e0, Fe<F> &de, Wide<F> &s0,
                                           Wide<F> &s1, Wide<F> &s2, Wide<F> &s3, Wide<F> &sinf) {
    Fe<F> u[4], v[4], uinf, x0, x1, y[4];                     // zerocheck_gate_round_kernel's running values
    {
        Fe<F> b[4];
        zerocheck_pair<F, FOLD>(plonk_in(PLONK_B), t.out(PLONK_B), i, mr, x0, x1);
        zerocheck_nodes<F>(x0, x1, b);
        const Fe<F> db = fe_sub<F>(x1, x0);
        zerocheck_pair<F, FOLD>(plonk_in(PLONK_QR), t.out(PLONK_QR), i, mr, x0, x1);
        zerocheck_nodes<F>(x0, x1, y);
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = fe_mul<F>(y[k], b[k]);
        zerocheck_pair<F, FOLD>(plonk_in(PLONK_QM), t.out(PLONK_QM), i, mr, x0, x1);
        zerocheck_nodes<F>(x0, x1, y);
#pragma unroll
        for (int k = 0; k < 4; k++) u[k] = fe_mul<F>(y[k], b[k]);
        uinf = fe_mul<F>(fe_sub<F>(x1, x0), db);
    }
    zerocheck_pair<F, FOLD>(plonk_in(PLONK_QL), t.out(PLONK_QL), i, mr, x0, x1);
    zerocheck_nodes<F>(x0, x1, y);
#pragma unroll
    for (int k = 0; k < 4; k++) u[k] = fe_add<F>(u[k], y[k]);
    zerocheck_pair<F, FOLD>(plonk_in(PLONK_A), t.out(PLONK_A), i, mr, x0, x1);
    zerocheck_nodes<F>(x0, x1, y);
#pragma unroll
    for (int k = 0; k < 4; k++) u[k] = fe_add<F>(fe_mul<F>(u[k], y[k]), v[k]);
    uinf = fe_mul<F>(uinf, fe_sub<F>(x1, x0));
    {
        Fe<F> c[4];
        zerocheck_pair<F, FOLD>(plonk_in(PLONK_QO), t.out(PLONK_QO), i, mr, x0, x1);
        zerocheck_nodes<F>(x0, x1, y);
        zerocheck_pair<F, FOLD>(plonk_in(PLONK_C), t.out(PLONK_C), i, mr, x0, x1);
        zerocheck_nodes<F>(x0, x1, c);
#pragma unroll
        for (int k = 0; k < 4; k++) u[k] = fe_add<F>(u[k], fe_mul<F>(y[k], c[k]));
    }
    zerocheck_pair<F, FOLD>(plonk_in(PLONK_QC), t.out(PLONK_QC), i, mr, x0, x1);
    zerocheck_nodes<F>(x0, x1, y);
#pragma unroll
    for (int k = 0; k < 4; k++) u[k] = fe_add<F>(u[k], y[k]);
    zerocheck_pair<F, FOLD>(plonk_in(E_AT), t.out(E_AT), i, mr, e0, x1);
    de = fe_sub<F>(x1, e0);
    {
        const Multiplier<F> ma3(cs[PlonkUniform<F>::ALPHA3]);
        x0 = ma3.times(e0);                                   // the line alpha^3 E
        x1 = ma3.times(de);
    }
    wide_add_fe<F>(sinf, fe_mul<F>(x1, uinf));
    wide_add_fe<F>(s0, fe_mul<F>(x0, u[0]));
    x0 = fe_add<F>(x0, x1);
    wide_add_fe<F>(s1, fe_mul<F>(x0, u[1]));
    x0 = fe_add<F>(x0, x1);
    wide_add_fe<F>(s2, fe_mul<F>(x0, u[2]));
    x0 = fe_add<F>(x0, x1);
    wide_add_fe<F>(s3, fe_mul<F>(x0, u[3]));
}

// the pair of wire J a second time: what the gate stored (FOLD) or read (round 0).  The pointer is laundered: the compiler must take the read for
// one that may alias the gate's store and may not replace it by the stored value
template <class F, bool FOLD, int J, class T = PlonkTables> __device__ __forceinline__ void plonk_pair_again(const T &t, size_t i, Fe<F> &x0, Fe<F> &x1) {
    const void *p;
    if constexpr (FOLD) {
        PlonkGlobal g = (PlonkGlobal)t.out(J);
        asm volatile("" : "+s"(g));
        p = (const void *)g;
    } else {
        p = plonk_in(J);
    }
    x0 = fe_load<F>(p, 2 * i);
    x1 = fe_load<F>(p, 2 * i + 1);
}

// wire J's share of the seven sums: wiring.cuh's wiring_wire on the tables of this pass, W_J read back.  T, H_AT: the pass's argument block and
// H0's place in it
template <class F, bool FOLD, int J, class T = PlonkTables, int H_AT = PLONK_H>
__device__ __forceinline__ void plonk_wire(const T &t, size_t i, const Multiplier<F> &mr, const PlonkUniform<F> &cs, const Fe<F> &gid, Fe<F> e, const Fe<F> &de,
                                           Wide<F> &s0, Wide<F> &s1, Wide<F> &s2, Wide<F> &s3, Wide<F> &sinf, Wide<F> &sev, Wide<F> &sod) {
    Fe<F> x0, x1;
    const Fe<F> gid1 = fe_add<F>(gid, cs[PlonkUniform<F>::GSTEP]);
    plonk_pair_again<F, FOLD, J>(t, i, x0, x1);
    Fe<F> did, ddid;
    {
        const Fe<F> beta = cs[PlonkUniform<F>::BETA];
        did = fe_add<F>(fe_add<F>(beta, x0), gid);
        ddid = fe_sub<F>(fe_add<F>(fe_add<F>(beta, x1), gid1), did);
    }
    zerocheck_pair<F, FOLD>(plonk_in(PLONK_S + J), t.out(PLONK_S + J), i, mr, x0, x1);
    Fe<F> nn, dn;
    {
        const Multiplier<F> mg(cs[PlonkUniform<F>::GAMMA]);
        nn = fe_sub<F>(mg.times(x0), gid);
        dn = fe_sub<F>(fe_sub<F>(mg.times(x1), gid1), nn);
    }
    zerocheck_pair<F, FOLD>(plonk_in(H_AT + J), t.out(H_AT + J), i, mr, x0, x1);
    wide_add_fe<F>(sev, x0);
    wide_add_fe<F>(sod, x1);
    const Fe<F> dh = fe_sub<F>(x1, x0);
    wide_add_fe<F>(sinf, fe_mul<F>(de, fe_mul<F>(dh, fe_mul<F>(ddid, fe_add<F>(ddid, dn)))));
    const auto node = [&](Wide<F> &sk, bool last) {
        wide_add_fe<F>(sk, fe_mul<F>(e, fe_sub<F>(fe_mul<F>(x0, fe_mul<F>(did, fe_add<F>(did, nn))), nn)));
        if (last) return;
        did = fe_add<F>(did, ddid);
        nn = fe_add<F>(nn, dn);
        x0 = fe_add<F>(x0, dh);
        e = fe_add<F>(e, de);
    };
    node(s0, false);
    node(s1, false);
    node(s2, false);
    node(s3, true);
}

// partials[X * gridDim.x + block] = the block's share of sum X, X < 7 (s_0, s_1, s_2, s_3, s_inf, s_ev, s_od); q, FOLD and the tables' lengths as
// in zerocheck_mul_round_kernel.  Two waves a SIMD are asked for, as for wiring_round_kernel.
template <class F, bool FOLD> __global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) plonk_round_kernel(PlonkTables t, size_t q, Fe<F> r, PlonkConsts<F> c, void *__restrict__ partials) {
    using U = PlonkUniform<F>;
    __shared__ Wide<F> sh[7 * kBlock / 64];
    __shared__ WiringWord4 csh[2 * U::COUNT];
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
    }
    __syncthreads();
    const U cs{(const volatile __attribute__((address_space(3))) WiringWord4 *)csh};
    const size_t stride = (size_t)gridDim.x * kBlock, first = (size_t)blockIdx.x * kBlock + threadIdx.x;
    Wide<F> sum[7] = {wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>()};
    const Multiplier<F> mr(r);
    // gamma id_0 at the lane's first pair: gamma (c_l + 2^l 2 first)
    Fe<F> gid = fe_add<F>(c.gid0, fe_mul<F>(fe_dbl<F>(c.gstep), fe_from_u64<F>((uint64_t)first)));
    for (size_t i = first; i < q; i += stride) {
        Fe<F> e0, de;
        plonk_gate<F, FOLD>(t, i, mr, cs, e0, de, sum[0], sum[1], sum[2], sum[3], sum[4]);
        __builtin_amdgcn_sched_barrier(0);                    // a phase at a time: left alone the scheduler requests the next phase's tables ahead
        plonk_wire<F, FOLD, 0>(t, i, mr, cs, gid, e0, de, sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6]);
        __builtin_amdgcn_sched_barrier(0);
        gid = fe_add<F>(gid, cs[U::GWIRE]);
        {
            const Multiplier<F> ma(cs[U::ALPHA]);
            e0 = ma.times(e0);
            de = ma.times(de);
        }
        plonk_wire<F, FOLD, 1>(t, i, mr, cs, gid, e0, de, sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6]);
        __builtin_amdgcn_sched_barrier(0);
        gid = fe_add<F>(gid, cs[U::GWIRE]);
        {
            const Multiplier<F> ma(cs[U::ALPHA]);
            e0 = ma.times(e0);
            de = ma.times(de);
        }
        plonk_wire<F, FOLD, 2>(t, i, mr, cs, gid, e0, de, sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6]);
        __builtin_amdgcn_sched_barrier(0);
        gid = fe_add<F>(gid, cs[U::GNEXT]);
    }
    Fe<F> tot;
    if (block_reduce_wide<F, 7>(sum, sh, tot)) fe_store<F>(partials, (size_t)threadIdx.x * gridDim.x + blockIdx.x, tot);
}

}  // namespace zk
