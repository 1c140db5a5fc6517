// gkr_tables_selftest.hip -- one gate of the sparse GKR prover's table kernels (csrc/gkr_tables.cuh: the conversion of half tables to the
// products' internal form, gate_weight_u, other_times_u, the one conditional subtraction per stored value, the two terms of Phase1Op and
// Phase2Op) compiled for the host, for all four fields.  tests/test_gkr_tables_cpu.py feeds it the operands of
// tests/golden/gkr_table_witnesses.json and random ones and compares every answer, and whether each intermediate reached p before its
// reduction, with the limb-exact Python model tests/_gkr_tables_model.py; the GPU path of the same functions is tests/test_gpu_gkr_tables.py.
//
// Standard input, one gate a line; an element is its 64-bit limbs in the stored (Montgomery) form, hexadecimal, least significant first (four,
// six for field 1):
//   G <field> <phase 1|2> <op 0|1> <nw> <no> <elements>
//     nw = 2: ah al bh bl, nw = 1: ah al  (weights from half tables, internal form);  nw = 0: w  (the weight itself, stored form)
//     no = 1: hi lo  (the other table's halves: internal form with nw > 0, stored form with nw = 0);  no = 0: x  (the other table's entry)
//   -> G <x> <y> <al> <bl> <hi> <lo> <weight> <other> <final>
//     x, y: the gate's two stored terms (phase 1: to H1, H0; phase 2: to A, M);  then for the converted low halves al and bl, the converted hi and
//     lo, the weight, the product of the other table's halves and the final product: 0, 1 or 2 = the value before its reduction is below p, at
//     least p, at least 2 p;  - = the form has no such intermediate.
// field: 0 = BLS12-381 Fr, 1 = BLS12-381 Fq, 2 = BN254 Fq, 3 = BN254 Fr.  Exit status 2 on a line it cannot read.
#include "../zk-cryptography-research-implementations_amd/csrc/gkr_tables.cuh"
#include <stdio.h>
using namespace zk;

template <class F> bool read_fe(Fe<F> &x) {
    for (int k = 0; k < F::N / 2; k++) {
        unsigned long long w;
        if (scanf("%llx", &w) != 1) return false;
        x.l[2 * k] = (uint32_t)w;
        x.l[2 * k + 1] = (uint32_t)(w >> 32);
    }
    return true;
}
template <class F> void print_fe(const Fe<F> &x) {
    for (int k = 0; k < F::N / 2; k++) printf(" %08x%08x", x.l[2 * k + 1], x.l[2 * k]);
}
// 0, 1, 2: a normalized value (limbs below 2^29) is below p, at least p, at least 2 p
template <class F> int level(const Ufe<F> &v) {
    constexpr int L = UParams<F>::L;
    int lv = 0;
    for (int mult = 1; mult <= 2; mult++) {
        int64_t c = 0;
        for (int j = 0; j < L; j++) c = ((int64_t)v.l[j] - (int64_t)mult * UParams<F>::p(j) + c) >> UB;     // the borrow out of limb j
        if (c >= 0) lv = mult;
    }
    return lv;
}
template <class F> struct Entry {            // a one-entry table in the internal form, aligned as the device tables are
    alignas(16) uint32_t w[u_stride_words<F>()];
    void set(const Ufe<F> &u) {
        for (int j = 0; j < u_stride_words<F>(); j++) w[j] = j < UParams<F>::L ? u.l[j] : 0u;
    }
};
template <class F> bool one_gate() {
    int phase, op, nw, no;
    if (scanf("%d %d %d %d", &phase, &op, &nw, &no) != 4) return false;
    if ((phase != 1 && phase != 2) || (op != 0 && op != 1) || nw < 0 || nw > 2 || no < 0 || no > 1 || (phase == 1 && no)) return false;
    alignas(16) Fe<F> wt[4], ot[2];              // ah al bh bl | w;   hi lo | x
    for (int i = 0; i < (nw ? 2 * nw : 1); i++)
        if (!read_fe<F>(wt[i])) return false;
    for (int i = 0; i < (no ? 2 : 1); i++)
        if (!read_fe<F>(ot[i])) return false;
    char flag[7] = {'-', '-', '-', '-', '-', '-', '-'};
    GateWeights gw{};
    OtherTable tab{};
    Entry<F> uw[4], uo[2];
    if (nw) {
        gw.ah = &wt[0]; gw.al = &wt[1];
        if (nw == 2) { gw.bh = &wt[2]; gw.bl = &wt[3]; }
        for (int i = 0; i < 2 * nw; i++) {
            uw[i].set(half_to_u<F>(wt[i], i & 1));                   // high halves as they are stored, low halves times U / R
            if (i & 1) flag[i / 2] = (char)('0' + level<F>(half_to_u_raw<F>(wt[i], 1)));
        }
        gw.uah = uw[0].w; gw.ual = uw[1].w;
        if (nw == 2) { gw.ubh = uw[2].w; gw.ubl = uw[3].w; }
    } else {
        gw.w = &wt[0];
    }
    if (no) {
        tab.hi = &ot[0]; tab.lo = &ot[1];
        if (nw) {
            for (int i = 0; i < 2; i++) {
                uo[i].set(half_to_u<F>(ot[i], 1));
                flag[2 + i] = (char)('0' + level<F>(half_to_u_raw<F>(ot[i], 1)));
            }
            tab.uhi = uo[0].w; tab.ulo = uo[1].w;
        }
    } else {
        tab.tab = &ot[0];
    }
    Fe<F> x, y;
    if (nw) {
        const Ufe<F> wu = gate_weight_u<F>(gw, 0);
        flag[4] = (char)('0' + level<F>(wu));
        if (no) flag[5] = (char)('0' + level<F>(other_halves_u<F>(tab, 0)));
        flag[6] = (char)('0' + level<F>(other_times_u<F>(tab, 0, wu)));
        if (phase == 1) gate_terms<F, Phase1Op, true>(gw, tab, 0, 0, (uint32_t)op, x, y);
        else gate_terms<F, Phase2Op, true>(gw, tab, 0, 0, (uint32_t)op, x, y);
    } else {
        if (phase == 1) gate_terms<F, Phase1Op, false>(gw, tab, 0, 0, (uint32_t)op, x, y);
        else gate_terms<F, Phase2Op, false>(gw, tab, 0, 0, (uint32_t)op, x, y);
    }
    printf("G");
    print_fe<F>(x);
    print_fe<F>(y);
    for (int i = 0; i < 7; i++) printf(" %c", flag[i]);
    printf("\n");
    return true;
}

int main() {
    char c;
    int field;
    while (scanf(" %c %d", &c, &field) == 2) {
        bool ok = false;
        if (c == 'G' && field == 0) ok = one_gate<Fr381>();
        if (c == 'G' && field == 1) ok = one_gate<Fq381>();
        if (c == 'G' && field == 2) ok = one_gate<Bn254Fq>();
        if (c == 'G' && field == 3) ok = one_gate<Bn254Fr>();
        if (!ok) {
            fprintf(stderr, "bad case line\n");
            return 2;
        }
    }
    return 0;
}
