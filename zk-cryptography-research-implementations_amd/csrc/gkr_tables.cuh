// gkr_tables.cuh -- what the table kernels of the sparse GKR prover (zkmle_gkr_sparse.hip phase1_tables_kernel / phase2_tables_kernel) do per
// gate: where a gate's weight and the entry at its other index come from, the chain of products between them, and the two terms a gate
// contributes.  Everything is __host__ __device__: the kernels and tools/gkr_tables_selftest.hip (a host program that replays one gate and
// reports every intermediate's value before its reduction; tests/test_gkr_tables_cpu.py, tests/_gkr_tables_model.py) compile the same code.
#pragma once
#include <string.h>

#include "ufield.cuh"

namespace zk {

// an element of a table in memory: the 16-byte vector loads of fields.cuh on the device, a plain copy on the host
template <class F> ZK_HD Fe<F> table_entry(const void *base, size_t idx) {
#if defined(__HIP_DEVICE_COMPILE__)
    return fe_load<F>(base, idx);
#else
    Fe<F> r;
    memcpy(r.l, reinterpret_cast<const char *>(base) + idx * (4 * F::N), 4 * F::N);
    return r;
#endif
}

// Where a gate's weight w_g = alpha eq(rb, out_g) + beta eq(rc, out_g) comes from.  Small layers: the table w (gate order), indexed through the
// group's order list.  Layers of > kEqSmallBits output bits: straight from the HALF tables of the two eq tables (entry o = hi[o >> lbits] *
// lo[o & mask], eq_table.cuh; the constants ride on the high halves), indexed by the gate's output index stored in grouped order -- four
// 64 KB tables that live in L2 and two products per gate, instead of building two 2^out_bits tables, adding them up gate by gate into w
// (three passes over 128 MB at 2^22) and gathering w from HBM.
struct GateWeights {
    const void *w;                       // non-null: the table of weights in gate order
    const void *ah, *al, *bh, *bl;       // else: half tables of alpha eq(rb, .) and (bh non-null) beta eq(rc, .)
    unsigned lbits;
    const void *uah, *ual, *ubh, *ubl;   // the same half tables in the products' internal form (below); uah non-null: the kernels use these
};
// the table gathered at a gate's other index: an array (W in phase 1), or the half tables of an eq table (eq(rb*, .) in phase 2)
struct OtherTable {
    const void *tab;                     // non-null: the table itself
    const void *hi, *lo;                 // else its half tables
    unsigned lbits;
    const void *uhi, *ulo;               // the half tables in the internal form (with GateWeights::uah)
};
// ---- half tables in the products' internal form (r3) ------------------------------------------------------------------------------
// The table kernels are VALU-bound, and more than half of their VALU work was not multiply-adds but what surrounds a product on stored
// operands: 32-bit -> 29-bit limbs of one operand, digit extraction of the other, conditional subtraction and 29-bit -> 32-bit limbs of
// the result -- ~190 instructions around 162 multiply-adds, four products per gate.  The half tables are 2^11 entries each and are
// built once per layer, so they are converted once: L limbs of 29 bits per entry (ufield.cuh), and the Montgomery factors are chosen so that
// a gate's chain of products needs no conversion until its result is stored.  With R = 2^(32 N) (the stored form) and U = 2^(29 L):
//   weights:  ah' = limbs29(ah R), al' = al U  ->  umul2(ah', al', bh', bl') = (ah al + bh bl) R = the weight in the stored form;
//   other:    hi' = hi U, lo' = lo U            ->  umul(hi', lo') = hi lo U;   umul(w R, h U) = w h R, the stored form of the product;
//   or a stored table entry x R                 ->  umul_std(w R, x R) = w x R  (digits of x: the one conversion left).
// Nothing between the converted half tables and the stored result is reduced.  A scan's value is below (sum of its products) / U + p, so for
// canonical stored inputs (tests/_gkr_tables_model.py chain_bounds computes these from p, U and R, and replays the scan limb by limb):
//   the weight (one or two products of operands below p)   < p (1 + 2 p / U):       1.029 p, 1 + 2^-24 p, 1.012 p, 1.012 p  (fields 0 .. 3)
//   the product of the other table's halves                < p (1 + p / U):         1.015 p, 1 + 2^-25 p, 1.006 p, 1.006 p
//   the result through the halves,  umul(w, h)             < p (1 + 1.05 p / U):    1.015 p, 1 + 2^-25 p, 1.006 p, 1.006 p
//   the result through a stored entry,  umul_std(w, x)     < p (1 + 1.03 p / R):    1.466 p, 1.102 p,     1.192 p, 1.192 p
// all below 2 p: one conditional subtraction gives the canonical limbs the old chain gave.
template <class F> constexpr int u_stride_words() { return (UParams<F>::L + 3) / 4 * 4; }          // 16-byte aligned entries
template <class F> ZK_HD Ufe<F> ufe_load(const void *tab, uint32_t idx) {
    const uint32_t *p = reinterpret_cast<const uint32_t *>(tab) + (size_t)idx * u_stride_words<F>();
    Ufe<F> r;
#pragma unroll
    for (int j = 0; j < UParams<F>::L; j++) r.l[j] = p[j];
    return r;
}
// a half-table entry as 29-bit limbs, before its reduction: the stored integer itself (mont = 0: exact) or times U / R (mont = 1: below 2 p)
template <class F> ZK_HD Ufe<F> half_to_u_raw(const Fe<F> &x, int mont) { return mont ? u_from_std<F>(x) : u_from_limbs32<F>(x); }
// ... and as the tables hold it: fully reduced
template <class F> ZK_HD Ufe<F> half_to_u(const Fe<F> &x, int mont) { return mont ? u_reduce_once<F>(half_to_u_raw<F>(x, 1)) : u_from_limbs32<F>(x); }
template <class F> ZK_HD Ufe<F> gate_weight_u(const GateWeights &g, uint32_t idx) {        // the weight, stored form, as 29-bit limbs, not reduced
    const uint32_t h = idx >> g.lbits, l = idx & ((1u << g.lbits) - 1u);
    if (g.ubh) return umul2<F>(ufe_load<F>(g.uah, h), ufe_load<F>(g.ual, l), ufe_load<F>(g.ubh, h), ufe_load<F>(g.ubl, l));
    return umul<F>(ufe_load<F>(g.uah, h), ufe_load<F>(g.ual, l));
}
template <class F> ZK_HD Ufe<F> other_halves_u(const OtherTable &t, uint32_t idx) {       // the entry times U from the internal-form halves, not reduced
    return umul<F>(ufe_load<F>(t.uhi, idx >> t.lbits), ufe_load<F>(t.ulo, idx & ((1u << t.lbits) - 1u)));
}
template <class F> ZK_HD Ufe<F> other_times_u(const OtherTable &t, uint32_t idx, const Ufe<F> &wu) {   // w x entry, stored form, not reduced
    if (t.tab) return umul_std<F>(wu, table_entry<F>(t.tab, idx));
    return umul<F>(wu, other_halves_u<F>(t, idx));
}
template <class F> ZK_HD Fe<F> other_entry(const OtherTable &t, uint32_t idx) {
    if (t.tab) return table_entry<F>(t.tab, idx);
    return fe_mul<F>(table_entry<F>(t.hi, idx >> t.lbits), table_entry<F>(t.lo, idx & ((1u << t.lbits) - 1u)));
}
template <class F> ZK_HD Fe<F> gate_weight(const GateWeights &g, uint32_t idx) {
    if (g.w) return table_entry<F>(g.w, idx);
    const uint32_t h = idx >> g.lbits, l = idx & ((1u << g.lbits) - 1u);
    if (g.bh) return fe_mul2_u<F>(table_entry<F>(g.ah, h), table_entry<F>(g.al, l), table_entry<F>(g.bh, h), table_entry<F>(g.bl, l));   // one reduction for both products
    return fe_mul<F>(table_entry<F>(g.ah, h), table_entry<F>(g.al, l));
}
struct Phase1Op {            // per gate: w and t = w W[right]; add gate: H1 += w, H0 += t; mul gate: H1 += t
    static constexpr bool kNeedsWeight = true;
    template <class F> static ZK_HD void terms(const Fe<F> &wg, const Fe<F> &t, uint32_t op, Fe<F> &x, Fe<F> &y) {
        if (op == 0) { x = wg; y = t; } else { x = t; y = fe_zero<F>(); }
    }
};
struct Phase2Op {            // per gate: t = w eqL[left]; add gate: A += t; mul gate: M += t
    static constexpr bool kNeedsWeight = false;
    template <class F> static ZK_HD void terms(const Fe<F> &, const Fe<F> &t, uint32_t op, Fe<F> &x, Fe<F> &y) {
        if (op == 0) { x = t; y = fe_zero<F>(); } else { x = fe_zero<F>(); y = t; }
    }
};
// one gate's two terms: oi indexes the weights (GateWeights), ti the other table, pi is the operation.  UH: half tables in the internal
// form, no conversions inside the chain and ONE conditional subtraction per stored value at its end
template <class F, class Op, bool UH>
ZK_HD void gate_terms(const GateWeights &gw, const OtherTable &tab, uint32_t oi, uint32_t ti, uint32_t pi, Fe<F> &x, Fe<F> &y) {
    if constexpr (UH) {
        const Ufe<F> wu = gate_weight_u<F>(gw, oi);
        const Fe<F> t = u_to_limbs32<F>(u_reduce_once<F>(other_times_u<F>(tab, ti, wu)));
        const Fe<F> wg = Op::kNeedsWeight ? u_to_limbs32<F>(u_reduce_once<F>(wu)) : fe_zero<F>();
        Op::template terms<F>(wg, t, pi, x, y);
    } else {
        const Fe<F> e = other_entry<F>(tab, ti);
        const Fe<F> wg = gate_weight<F>(gw, oi);
        Op::template terms<F>(wg, fe_mul<F>(wg, e), pi, x, y);
    }
}

}  // namespace zk
