// wiring.cuh -- the two kernels of the permutation check over FRI commitments (include/zkmle.h "Wiring: a permutation check over committed
// tables"): the logarithmic-derivative helper tables and the round pass of its sumcheck.
//
//   fractions   H[x] = inv0(beta + W[x] + gamma (first + x)) - inv0(beta + W[x] + gamma S[x]),  inv0(0) = 0, one wire per launch.
//               The 2 n inverses by Montgomery's trick per lane, in the tile layout of fri_pcs.cuh's quotient kernel: a lane takes the
//               kWiringBatch entries base + 256 t of its block's tile of 256 kWiringBatch (every access of a wave is contiguous), keeps the
//               prefix products of its 2 kWiringBatch denominators in registers, inverts the full product once by Fermat (pcs_inverse) and
//               walks back, forming each denominator again from W and S (two reads and one product are cheaper than sixteen more live
//               elements).  A zero denominator enters the chain as 1 and its own output is selected to 0: a compare and a select per
//               denominator, and no other entry of the batch sees it.  gamma (first + x) comes from the index: one product per lane,
//               then additions of gamma 256.  Per entry: 2 products for gamma S (forward and back), 2 for the prefix chain, 4 on the way
//               back, and a sixteenth of a lane's inversion (255 squarings and the multiplications of p - 2).
//   round       one pass per round over the ten tables A, B, C, SA, SB, SC, H0, H1, H2, E, in the idiom of zerocheck_gate_round_kernel:
//               lane i < q folds each table's four entries to the pair (X[2i], X[2i+1]) and stores it (FOLD), or reads the pair (round 0).
//               With Y_k the pair's line at the node k (additions only), and for the wire j
//                   Did_j = beta + W_j + gamma id_j,   Dsig_j = beta + W_j + gamma S_j,   N_j = gamma (S_j - id_j) = Dsig_j - Did_j,
//               all three lines in X (gamma id_j at the pair's two entries differs by gamma 2^l, from wire to wire by gamma 2^d: no table, no product), it
//               accumulates
//                   s_k   += E_k sum_j alpha^j (H_j,k Did_j,k Dsig_j,k - N_j,k)                       k = 0, 1, 2, 3
//                   s_inf += (E1 - E0) sum_j alpha^j (H_j1 - H_j0)(Did_j1 - Did_j0)(Dsig_j1 - Dsig_j0)   the X^4 coefficient
//                   s_ev  += H_0[2i] + H_1[2i] + H_2[2i],    s_od += H_0[2i+1] + H_1[2i+1] + H_2[2i+1]
//               and the host adds mu times the line through s_ev, s_od to the node values: the linear term costs no product.
//               A wire at a time, straight into the sums: E is loaded first, and each wire's term is multiplied by the line alpha^j E at
//               once (alpha scales the line of E between the wires: two products), so that nothing but that line lives from one wire to
//               the next -- running values for the three wires together cost five more live elements and the pass a wave.
//               Products per lane: 2 per table folded (20), gamma S 2 per wire (6), H Did Dsig 10 per wire with the infinity term (30),
//               E's five per wire (15), alpha 2 for each of the wires B and C (4):  75 in the fold form, 55 in round 0's.  40 reads and
//               20 writes of 32 bytes in the fold form; 20 reads in round 0's.  The folded tables are one block (a base and a stride), and
//               five of the uniform elements wait in LDS: twenty pointers and the uniform values do not fit the scalar registers together.
#pragma once
#include "fri_pcs.cuh"
#include "zerocheck.cuh"

namespace zk {

constexpr int kWiringBatch = 8;                              // entries per lane of the fractions kernel: 16 denominators an inversion

template <class F> __device__ __forceinline__ Fe<F> wiring_select(bool c, const Fe<F> &a, const Fe<F> &b) {
    Fe<F> o;
#pragma unroll
    for (int k = 0; k < F::N; k++) o.l[k] = c ? a.l[k] : b.l[k];
    return o;
}

// the two denominators of entry i; gid = gamma id(i)
template <class F> __device__ __forceinline__ void wiring_denominators(const void *__restrict__ W, const void *__restrict__ S, size_t i, const Fe<F> &beta,
                                                                     const Multiplier<F> &mg, const Fe<F> &gid, Fe<F> &did, Fe<F> &dsig) {
    const Fe<F> bw = fe_add<F>(beta, fe_load<F>(W, i));
    did = fe_add<F>(bw, gid);
    dsig = fe_add<F>(bw, mg.times(fe_load<F>(S, i)));
}

// H[x] for x < n.  gfirst = gamma first, g256 = gamma 256 (the distance of a lane's entries).  H is no input's memory.
template <class F> __global__ void __launch_bounds__(kPcsBlock) wiring_fractions_kernel(const void *__restrict__ W, const void *__restrict__ S, void *__restrict__ H, size_t n,
                                                                                       Fe<F> beta, Fe<F> gamma, Fe<F> gfirst, Fe<F> g256) {
    constexpr int T = kWiringBatch;
    const size_t base = (size_t)blockIdx.x * (T * kPcsBlock) + threadIdx.x;
    if (base >= n) return;
    const Multiplier<F> mg(gamma);
    const Fe<F> one = fe_one<F>(), zero = fe_zero<F>();
    Fe<F> gid = fe_add<F>(gfirst, mg.times(fe_from_u64<F>((uint64_t)base)));
    Fe<F> pre[2 * T];
    Fe<F> acc = one;
    pcs_static_for(std::make_integer_sequence<int, T>{}, [&](auto tc) {
        constexpr int t = decltype(tc)::value;
        const size_t i = base + (size_t)t * kPcsBlock;
        if (i < n) {
            Fe<F> did, dsig;
            wiring_denominators<F>(W, S, i, beta, mg, gid, did, dsig);
            did = wiring_select<F>(fe_is_zero<F>(did), one, did);
            dsig = wiring_select<F>(fe_is_zero<F>(dsig), one, dsig);
            acc = t == 0 ? did : fe_mul_u<F>(acc, did);
            pre[2 * t] = acc;
            acc = fe_mul_u<F>(acc, dsig);
            pre[2 * t + 1] = acc;
        }
        gid = fe_add<F>(gid, g256);
    });
    Fe<F> inv = pcs_inverse<F>(acc);                         // 1 / the product of the lane's non-zero denominators
    pcs_static_for(std::make_integer_sequence<int, T>{}, [&](auto tc) {
        constexpr int t = T - 1 - decltype(tc)::value;
        const size_t i = base + (size_t)t * kPcsBlock;
        gid = fe_sub<F>(gid, g256);
        if (i < n) {
            Fe<F> did, dsig;
            wiring_denominators<F>(W, S, i, beta, mg, gid, did, dsig);
            const bool zd = fe_is_zero<F>(did), zs = fe_is_zero<F>(dsig);
            const Fe<F> isig = fe_mul_u<F>(inv, pre[2 * t]);
            inv = fe_mul_u<F>(inv, wiring_select<F>(zs, one, dsig));
            Fe<F> idid = inv;
            if (t > 0) {
                idid = fe_mul_u<F>(inv, pre[t > 0 ? 2 * t - 1 : 0]);
                inv = fe_mul_u<F>(inv, wiring_select<F>(zd, one, did));
            }
            fe_store<F>(H, i, fe_sub<F>(wiring_select<F>(zd, zero, idid), wiring_select<F>(zs, zero, isig)));
        }
    });
}

// the ten tables of a pass, in the order A, B, C, SA, SB, SC, H0, H1, H2, E.  The folded tables are one block: table j at out0 + j ostride
// bytes
struct WiringTables {
    const void *in[10];
    void *out0;
    size_t ostride;
    __device__ __forceinline__ void *out(int j) const { return (char *)out0 + (size_t)j * ostride; }
};
// the pass's uniform values.  With the tables the sums are taken over at step 2^l and offset c_l:  gid0 = gamma c_l, the first pair's gamma id
// of wire A; gstep = gamma 2^l; gwire = gamma 2^d (from one wire's ids to the next one's); gnext = gamma (2^(l+1) gridDim.x kBlock - 2 2^d):
// from wire C's ids at a lane's pair to wire A's at its next pair
template <class F> struct WiringConsts {
    Fe<F> beta, gamma, alpha, gid0, gstep, gwire, gnext;
};

// The pass's uniform elements that the scalar registers have no room for (beta, gamma, alpha, gstep, gwire, gnext beside twenty pointers, the
// fold's multiplier and the modulus) wait in LDS and are read where they are used: a volatile read, so that the compiler does not gather them in
// front of the loop again.
typedef uint32_t WiringWord4 __attribute__((ext_vector_type(4)));
template <class F> struct WiringUniform {
    static_assert(F::N == 8, "two 16-byte reads an element");
    enum { BETA, GAMMA, ALPHA, GSTEP, GWIRE, GNEXT, COUNT };
    const volatile __attribute__((address_space(3))) WiringWord4 *w;   // LDS by its type: a volatile read through a generic pointer stays a flat load
    __device__ __forceinline__ Fe<F> operator[](int k) const {
        const WiringWord4 a = w[2 * k], b = w[2 * k + 1];
        Fe<F> o;
        o.l[0] = a.x; o.l[1] = a.y; o.l[2] = a.z; o.l[3] = a.w;
        o.l[4] = b.x; o.l[5] = b.y; o.l[6] = b.z; o.l[7] = b.w;
        return o;
    }
};

// wire J's share of the seven sums.  gid = gamma id_J at the pair's even entry; (e, de) = the line alpha^J E at the pair.  Three lines in X:
// Did, N = Dsig - Did = gamma S - gamma id, and H; Dsig_k = Did_k + N_k.  E multiplies every wire's term on its own, so nothing but the line
// of E lives from one wire to the next.
template <class F, bool FOLD, int J>
__device__ __forceinline__ void wiring_wire(const WiringTables &t, size_t i, const Multiplier<F> &mr, const WiringUniform<F> &cs, const Fe<F> &gid,
                                            Fe<F> e, const Fe<F> &de, Wide<F> &s0, Wide<F> &s1, Wide<F> &s2, Wide<F> &s3, Wide<F> &sinf, Wide<F> &sev, Wide<F> &sod) {
    Fe<F> x0, x1;
    const Fe<F> gid1 = fe_add<F>(gid, cs[WiringUniform<F>::GSTEP]);
    zerocheck_pair<F, FOLD>(t.in[J], t.out(J), i, mr, x0, x1);
    Fe<F> did, ddid;
    {
        const Fe<F> beta = cs[WiringUniform<F>::BETA];
        did = fe_add<F>(fe_add<F>(beta, x0), gid);
        ddid = fe_sub<F>(fe_add<F>(fe_add<F>(beta, x1), gid1), did);
    }
    zerocheck_pair<F, FOLD>(t.in[3 + J], t.out(3 + J), i, mr, x0, x1);
    Fe<F> nn, dn;
    {
        const Multiplier<F> mg(cs[WiringUniform<F>::GAMMA]);
        nn = fe_sub<F>(mg.times(x0), gid);
        dn = fe_sub<F>(fe_sub<F>(mg.times(x1), gid1), nn);
    }
    zerocheck_pair<F, FOLD>(t.in[6 + J], t.out(6 + J), i, mr, x0, x1);
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

// partials[X * gridDim.x + block] = the block's share of sum X, X < 7 (s_0, s_1, s_2, s_3, s_inf, s_ev, s_od); q, FOLD and the tables'
// lengths as in zerocheck_mul_round_kernel
// Two waves a SIMD are asked for: left to one, the allocator spreads the pass over 260 to 470 registers (it runs the nodes' products side by
// side) and spills scalars; held to 256 it fits with neither scratch nor spills.
template <class F, bool FOLD> __global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) wiring_round_kernel(WiringTables t, size_t q, Fe<F> r, WiringConsts<F> c, void *__restrict__ partials) {
    __shared__ Wide<F> sh[7 * kBlock / 64];
    __shared__ WiringWord4 csh[2 * WiringUniform<F>::COUNT];
    if (threadIdx.x == 0) {
        const auto put = [&](int k, const Fe<F> &e) {
            csh[2 * k] = WiringWord4{e.l[0], e.l[1], e.l[2], e.l[3]};
            csh[2 * k + 1] = WiringWord4{e.l[4], e.l[5], e.l[6], e.l[7]};
        };
        put(WiringUniform<F>::BETA, c.beta);
        put(WiringUniform<F>::GAMMA, c.gamma);
        put(WiringUniform<F>::ALPHA, c.alpha);
        put(WiringUniform<F>::GSTEP, c.gstep);
        put(WiringUniform<F>::GWIRE, c.gwire);
        put(WiringUniform<F>::GNEXT, c.gnext);
    }
    __syncthreads();
    const WiringUniform<F> cs{(const volatile __attribute__((address_space(3))) WiringWord4 *)csh};
    const size_t stride = (size_t)gridDim.x * kBlock, first = (size_t)blockIdx.x * kBlock + threadIdx.x;
    Wide<F> sum[7] = {wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>(), wide_zero<F>()};
    const Multiplier<F> mr(r);
    // gamma id_0 at the lane's first pair: gamma (c_l + 2^l 2 first)
    Fe<F> gid = fe_add<F>(c.gid0, fe_mul<F>(fe_dbl<F>(c.gstep), fe_from_u64<F>((uint64_t)first)));
    for (size_t i = first; i < q; i += stride) {
        Fe<F> e0, e1;
        zerocheck_pair<F, FOLD>(t.in[9], t.out(9), i, mr, e0, e1);
        Fe<F> de = fe_sub<F>(e1, e0);
        wiring_wire<F, FOLD, 0>(t, i, mr, cs, gid, e0, de, sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6]);
        __builtin_amdgcn_sched_barrier(0);                    // a wire at a time: left alone the scheduler requests the next wire's tables ahead
        gid = fe_add<F>(gid, cs[WiringUniform<F>::GWIRE]);
        {
            const Multiplier<F> ma(cs[WiringUniform<F>::ALPHA]);
            e0 = ma.times(e0);
            de = ma.times(de);
        }
        wiring_wire<F, FOLD, 1>(t, i, mr, cs, gid, e0, de, sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6]);
        __builtin_amdgcn_sched_barrier(0);
        gid = fe_add<F>(gid, cs[WiringUniform<F>::GWIRE]);
        {
            const Multiplier<F> ma(cs[WiringUniform<F>::ALPHA]);
            e0 = ma.times(e0);
            de = ma.times(de);
        }
        wiring_wire<F, FOLD, 2>(t, i, mr, cs, gid, e0, de, sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6]);
        __builtin_amdgcn_sched_barrier(0);
        gid = fe_add<F>(gid, cs[WiringUniform<F>::GNEXT]);
    }
    Fe<F> tot;
    if (block_reduce_wide<F, 7>(sum, sh, tot)) fe_store<F>(partials, (size_t)threadIdx.x * gridDim.x + blockIdx.x, tot);
}

}  // namespace zk
