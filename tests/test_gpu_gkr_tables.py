"""GPU: the sparse GKR prover's table kernels (csrc/zkmle_gkr_sparse.hip phase1_tables_kernel / phase2_tables_kernel, csrc/gkr_tables.cuh) on
tables the test chooses, through zk_gkr_sparse_phase_tables -- the prover's own set-up and launch functions.  Inside a proof the half tables are
eq tables of Fiat-Shamir challenges, so the chain of unreduced 29-bit-limb products only ever sees uniform values and, below 2^13 outputs, is
not run at all; here it runs on all four fields at operands built to reach p before each reduction (tests/golden/gkr_table_witnesses.json,
replayed on the host by tests/test_gkr_tables_cpu.py), on structured tables, and at the geometry of grouped_pair_sums.

Everything is compared byte for byte with the plain reference of tests/_gkr_tables_model.py (field sums per group over Python integers), the
inputs are read back unchanged, and every case runs twice with identical output.

A planted witness proves nothing by sitting alone in its group: the group's sum starts as fe_add(0, term), and that addition's own conditional
subtraction finishes any term below 2 p, reduced or not.  Each witness therefore also sits beside a companion gate whose terms are the stored
integer p - 1 (see test_witness_planted_at_an_add_and_a_mul_gate).  With that, a library built without the final u_reduce_once fails every
witness case whose final flag is set, and one built without the weight's fails every phase-1 case whose weight flag is set.

Forms (weights / other table), the four the prover reaches:  hh = half tables in the internal form / internal halves (phase 2);  ht = internal
half tables / a table (W in phase 1, the eq table in phase 2);  th = a weight table / stored halves (phase 2);  tt = both tables."""
import random

import numpy as np
import pytest

import __graft_entry__ as G

import _gkr_tables_model as T

pytestmark = pytest.mark.gpu
FIELDS = (0, 1, 2, 3)
OUT_BITS, LBITS, OTHER_LBITS = 8, 4, 4
WITNESSES = {f: T.load_witnesses(f)[0] for f in FIELDS}        # replayed by the model while pytest collects (load_witnesses)


def package():
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    return zk


def to_limbs(field, values):
    nb = T.STD_BITS[field] // 8
    return np.frombuffer(b"".join(int(v).to_bytes(nb, "little") for v in values), np.uint64).reshape(-1, nb // 8).copy()


def to_ints(field, arr):
    n = T.STD_BITS[field] // 64
    return [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(arr, np.uint64).reshape(-1, n)]


class Case:
    """one call of the hook: gates (rows of left, right, out, op), stored-integer tables, and the reference's answer"""

    def __init__(self, field, phase, gates, in_bits, halves=None, w=None, other=None, other_halves=None, u=0, out_bits=OUT_BITS, lbits=LBITS,
                 other_lbits=OTHER_LBITS):
        self.field, self.phase, self.gates, self.in_bits, self.out_bits = field, phase, [tuple(g) for g in gates], in_bits, out_bits
        self.halves, self.w, self.other, self.other_halves, self.u = halves, w, other, other_halves, u
        self.lbits, self.other_lbits = lbits, other_lbits

    def want(self):
        return T.phase_tables(self.field, self.phase, self.gates, self.in_bits, halves=self.halves, lbits=self.lbits, w=self.w, other=self.other,
                              other_halves=self.other_halves, other_lbits=self.other_lbits, u=self.u)

    def run(self, zk, tag):
        f = self.field
        up = lambda t: zk.MultilinearPolynomial(f, to_limbs(f, t))
        inputs = {}
        kw = {"lbits": self.lbits, "other_lbits": self.other_lbits}
        if self.halves is not None:
            inputs["halves"] = [up(t) for t in self.halves]
            kw["halves"] = inputs["halves"]
        elif self.gates:
            inputs["w"] = [zk.MultilinearPolynomial.vector(f, to_limbs(f, self.w))]
            kw["w"] = inputs["w"][0]
        if self.other is not None:
            inputs["other"] = [up(self.other)]
            kw["other"] = inputs["other"][0]
        else:
            inputs["other_halves"] = [up(t) for t in self.other_halves]
            kw["other_halves"] = inputs["other_halves"]
        if self.phase == 2:
            kw["u"] = to_limbs(f, [self.u])[0]
        rows = np.array(self.gates, np.uint64).reshape(-1, 4)
        wx, wy = self.want()
        first = None
        for rep in range(2):
            x, y = zk.gkr.sparse_phase_tables(f, self.phase, rows, self.out_bits, self.in_bits, **kw)
            got = (to_ints(f, x.evaluated_values), to_ints(f, y.evaluated_values))
            if rep == 0:
                first = got
                bad = [i for i in range(1 << self.in_bits) if (got[0][i], got[1][i]) != (wx[i], wy[i])]
                assert not bad, (tag, "groups", bad[:8])
            else:
                assert got == first, (tag, "second run differs")
        src = {"halves": self.halves, "w": [self.w], "other": [self.other], "other_halves": self.other_halves}
        for name, tabs in inputs.items():                                         # the inputs are unchanged
            for t, orig in zip(tabs, src[name]):
                assert to_ints(f, t.evaluated_values) == list(orig), (tag, name)
        assert np.array_equal(rows, np.array(self.gates, np.uint64).reshape(-1, 4))


def random_gates(rng, n, in_bits, out_bits=OUT_BITS):
    return [(rng.randrange(1 << in_bits), rng.randrange(1 << in_bits), rng.randrange(1 << out_bits), rng.randrange(2)) for _ in range(n)]


def random_table(rng, p, n):
    return [rng.randrange(p) for _ in range(n)]


# ---- witnesses ---------------------------------------------------------------------------------------------------------------------------------
WITNESS_CASES = [(f, w["name"], ph) for f in FIELDS for w in WITNESSES[f] for ph in T.witness_phases(w)]


@pytest.mark.parametrize("field,name,phase", WITNESS_CASES, ids=["f%d-%s-phase%d" % c for c in WITNESS_CASES])
def test_witness_planted_at_an_add_and_a_mul_gate(field, name, phase):
    """512 groups (workgroups of 224, 224 and 64), 2^8 outputs from 16-entry half tables, about 2000 random gates over random tables; the witness
    owns one output index and one index of the other table -- the half-table rows behind them hold its operands -- and sits at an add gate and
    at a mul gate: in phase 1 the add gate sends u_reduce_once(weight) to H1 and the product to H0, the mul gate the product to H1.  Before the
    GPU runs, the model replays the two planted gates from the tables and must report the fixture's flags."""
    w = next(x for x in WITNESSES[field] if x["name"] == name)
    p, in_bits = T.MODULUS[field], 9
    rng = random.Random("%d %s %d" % (field, name, phase))
    nh = len(w["halves"])
    halves = [random_table(rng, p, 1 << (OUT_BITS - LBITS if i % 2 == 0 else LBITS)) for i in range(nh)]
    o, t = rng.randrange(1 << OUT_BITS), rng.randrange(1 << in_bits)
    row = lambda i: (o >> LBITS) if i % 2 == 0 else (o & ((1 << LBITS) - 1))          # ah, bh by the high bits of the output index, al, bl by the low
    thi, tlo = t >> OTHER_LBITS, t & ((1 << OTHER_LBITS) - 1)
    for i, v in enumerate(w["halves"]):
        halves[i][row(i)] = v
    other = other_halves = None
    if "other" in w:
        other = random_table(rng, p, 1 << in_bits)
        other[t] = w["other"]
    else:
        other_halves = [random_table(rng, p, 1 << (in_bits - OTHER_LBITS)), random_table(rng, p, 1 << OTHER_LBITS)]
        other_halves[0][thi], other_halves[1][tlo] = w["other_halves"]
    # A lone gate cannot show a missing reduction: the group's sum starts as fe_add(0, term), whose own conditional subtraction finishes a
    # term below 2 p.  So the witness also sits in 32 groups of two gates, beside a companion gate whose weight and product are both the
    # stored integer p - 1: (p - 1) + (p + s) leaves fe_add at or above p unless the term was reduced.  The order inside a group is the
    # device sort's (atomics): half of the pairs put the companion first in the gate list, half the witness.
    mask_l, mask_o = (1 << LBITS) - 1, (1 << OTHER_LBITS) - 1
    oc = next(v for v in iter(lambda: rng.randrange(1 << OUT_BITS), None) if v >> LBITS != o >> LBITS and v & mask_l != o & mask_l)
    tc = next(v for v in iter(lambda: rng.randrange(1 << in_bits), None) if v >> OTHER_LBITS != thi and v & mask_o != tlo)
    rl, inv = (lambda v: T.real(field, v)), (lambda v: pow(v, -1, p))
    rest = rl(halves[2][oc >> LBITS]) * rl(halves[3][oc & mask_l]) if nh == 4 else 0
    halves[1][oc & mask_l] = T.stored(field, (rl(p - 1) - rest) * inv(rl(halves[0][oc >> LBITS])) % p)
    if other is not None:
        other[tc] = T.stored(field, 1)
        centry = {"other": other[tc]}
    else:
        other_halves[1][tc & mask_o] = T.stored(field, inv(rl(other_halves[0][tc >> OTHER_LBITS])))
        centry = {"other_halves": (other_halves[0][tc >> OTHER_LBITS], other_halves[1][tc & mask_o])}
    cx, cy, _ = T.gate(field, phase, 0, halves=tuple(halves[i][(oc >> LBITS) if i % 2 == 0 else (oc & mask_l)] for i in range(nh)), **centry)
    assert cx == p - 1 and (phase == 2 or cy == p - 1)
    pair_keys = rng.sample(range(1 << in_bits), 32)
    gates = [g for g in random_gates(rng, 2400, in_bits) if g[phase - 1] not in pair_keys][:2000]
    for j, key in enumerate(pair_keys):
        op = 1 if phase == 1 and j >= 16 else 0                    # phase 1: both gate types reach H1; phase 2: A is the table read back as it is
        pair = [(oc, tc), (o, t)] if j % 2 == 0 else [(o, t), (oc, tc)]
        gates += [(key, ti, oi, op) if phase == 1 else (ti, key, oi, op) for oi, ti in pair]
    for op, g in enumerate(rng.sample(range(2000), 2)):
        key = next(v for v in iter(lambda: rng.randrange(1 << in_bits), None) if v not in pair_keys)
        gates[g] = (key, t, o, op) if phase == 1 else (t, key, o, op)
        entry = {"other": other[t]} if other is not None else {"other_halves": (other_halves[0][thi], other_halves[1][tlo])}
        planted = tuple(halves[i][row(i)] for i in range(nh))
        tr = T.gate(field, phase, op, halves=planted, **entry)[2]
        assert tr.flags(field) == w["flags"] and all(tr.level(field, s) == 1 for s in w["targets"]), (field, name, tr.flags(field))
    u = rng.choice((0, 1, p - 1, rng.randrange(p)))
    Case(field, phase, gates, in_bits, halves=halves, other=other, other_halves=other_halves, u=u).run(package(), (field, name, phase))


# ---- structured tables -------------------------------------------------------------------------------------------------------------------------
KINDS = ("stored_pm1", "real_pm1", "zero", "one", "mix")
STRUCTURED = [(f, k) for f in (0, 3) for k in KINDS] + [(f, k) for f in (1, 2) for k in ("stored_pm1", "mix")]


def kind_table(field, kind, n, rng):
    p = T.MODULUS[field]
    if kind == "mix":
        return [rng.choice((0, p - 1, rng.randrange(p))) for _ in range(n)]
    return [{"stored_pm1": p - 1, "real_pm1": T.stored(field, p - 1), "zero": 0, "one": T.stored(field, 1)}[kind]] * n


@pytest.mark.parametrize("field,kind", STRUCTURED)
def test_structured_tables_every_form_both_phases(field, kind):
    """half tables, the weight table and the other table all of one kind; u rotates through 0, 1, p - 1 and a uniform draw"""
    zk = package()
    p, in_bits, ng = T.MODULUS[field], 9, 1500
    rng = random.Random("%d %s" % (field, kind))
    us = [0, T.stored(field, 1), T.stored(field, p - 1), rng.randrange(p)]
    k = 0
    for form, phases in (("hh", (2,)), ("ht", (1, 2)), ("th", (2,)), ("tt", (1, 2))):
        for phase in phases:
            for nw in ((4, 2) if form[0] == "h" else (0,)):
                gates = random_gates(rng, ng, in_bits)
                halves = [kind_table(field, kind, 1 << (OUT_BITS - LBITS if i % 2 == 0 else LBITS), rng) for i in range(nw)] if nw else None
                w = kind_table(field, kind, ng, rng) if not nw else None
                other = kind_table(field, kind, 1 << in_bits, rng) if form[1] == "t" else None
                oh = [kind_table(field, kind, 1 << (in_bits - OTHER_LBITS), rng), kind_table(field, kind, 1 << OTHER_LBITS, rng)] if form[1] == "h" else None
                Case(field, phase, gates, in_bits, halves=halves, w=w, other=other, other_halves=oh, u=us[k % 4]).run(zk, (field, kind, form, phase, nw))
                k += 1


# ---- the geometry of grouped_pair_sums -------------------------------------------------------------------------------------------------------
GROUPS = 224                     # kPhaseGroups: the groups a workgroup owns; a pass stages 256 gates


def spread(rng, lo, hi, n):
    counts = {}
    for _ in range(n):
        g = rng.randrange(lo, hi)
        counts[g] = counts.get(g, 0) + 1
    return counts


def geometry_scenarios(rng, nb):
    """name -> {group: number of gates}"""
    nwg = (nb + GROUPS - 1) // GROUPS
    span = lambda k: (k * GROUPS, min((k + 1) * GROUPS, nb))
    out = {}
    for rot in range(3 if nwg < 3 else 1):                      # a workgroup with no gates, with exactly 256 (one full pass), with 257
        counts = {}
        for k in range(nwg):
            counts.update(spread(rng, *span(k), (0, 256, 257)[(k + rot) % 3]))
        out["per_workgroup_0_256_257_rot%d" % rot] = counts
    for k in sorted({0, nwg - 1}):                              # a run over slots 255 and 256 of its workgroup's gate range: two passes
        lo, hi = span(k)
        out["straddle_wg%d" % k] = {lo: 255, lo + 1: 2} if hi - lo >= 2 else {}
    if nb > GROUPS + 1:
        out["runs_256_and_513_in_wg1"] = {**spread(rng, 0, GROUPS, 100), GROUPS: 256, GROUPS + 1: 513}
    out["all_under_last_group"] = {nb - 1: 600}
    if nb > GROUPS - 1:
        out["all_under_group_223"] = {GROUPS - 1: 600}
    if nb > GROUPS:
        out["all_under_group_224"] = {GROUPS: 600}
    out["all_add"] = spread(rng, 0, nb, 900)
    out["all_mul"] = spread(rng, 0, nb, 900)
    return {k: v for k, v in out.items() if v}


@pytest.mark.parametrize("in_bits", [1, 7, 8, 9, 10])
@pytest.mark.parametrize("internal", [False, True], ids=["tables", "internal"])
def test_geometry_of_the_grouped_sums(internal, in_bits):
    zk = package()
    field = 0
    p, nb = T.MODULUS[field], 1 << in_bits
    rng = random.Random(7000 + in_bits + (100 if internal else 0))
    other_lbits = max(1, in_bits // 2)
    for name, counts in geometry_scenarios(rng, nb).items():
        for phase in (1, 2):
            gates = []
            for grp, n in counts.items():
                for _ in range(n):
                    oth, o = rng.randrange(nb), rng.randrange(1 << OUT_BITS)
                    op = 0 if name == "all_add" else 1 if name == "all_mul" else rng.randrange(2)
                    gates.append((grp, oth, o, op) if phase == 1 else (oth, grp, o, op))
            rng.shuffle(gates)
            assert len(gates) <= 1 << 13
            halves = [random_table(rng, p, 1 << (OUT_BITS - LBITS)), random_table(rng, p, 1 << LBITS)] * 2 if internal else None
            w = None if internal else random_table(rng, p, len(gates))
            use_halves = internal and phase == 2 and in_bits > 1
            other = None if use_halves else random_table(rng, p, nb)
            oh = [random_table(rng, p, nb >> other_lbits), random_table(rng, p, 1 << other_lbits)] if use_halves else None
            Case(field, phase, gates, in_bits, halves=halves, w=w, other=other, other_halves=oh, u=rng.randrange(p),
                 other_lbits=other_lbits).run(zk, (name, phase, in_bits, internal))


@pytest.mark.parametrize("in_bits", [1, 9])
def test_no_gates_gives_zero_tables(in_bits):
    zk = package()
    field = 0
    rng = random.Random(in_bits)
    for phase in (1, 2):
        c = Case(field, phase, [], in_bits, w=[], other=random_table(rng, T.MODULUS[field], 1 << in_bits), u=5)
        assert c.want() == ([0] * (1 << in_bits), [0] * (1 << in_bits))
        c.run(zk, ("no gates", phase, in_bits))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_unreachable_forms_and_misfit_tables_are_refused_with_nothing_written():
    import ctypes as C
    zk = package()
    from zkmle_amd import _lib as L
    field, in_bits = 0, 5
    rng = random.Random(11)
    p = T.MODULUS[field]
    tab = lambda n, f=field: zk.MultilinearPolynomial(f, to_limbs(f, random_table(rng, T.MODULUS[f], n)))
    gates = np.array(random_gates(rng, 40, in_bits), np.uint64)
    hi, lo, other, ohi, olo = tab(16), tab(16), tab(32), tab(4), tab(8)
    w = zk.MultilinearPolynomial.vector(field, to_limbs(field, random_table(rng, p, 40)))
    u = to_limbs(field, [7])[0]
    good = dict(field=field, phase=2, out_bits=OUT_BITS, in_bits=in_bits, ah=hi, al=lo, bh=hi, bl=lo, lbits=4, w=None, other=None, ohi=ohi, olo=olo,
                other_lbits=3, u=u)

    def call(**over):
        a = {**good, **over}
        x, y = C.c_void_p(), C.c_void_p()
        h = lambda t: t._h if t is not None else None
        rc = zk.lib().zk_gkr_sparse_phase_tables(a["field"], a["phase"], gates.ctypes.data, len(gates), a["out_bits"], a["in_bits"], h(a["ah"]), h(a["al"]),
                                                 h(a["bh"]), h(a["bl"]), a["lbits"], h(a["w"]), h(a["other"]), h(a["ohi"]), h(a["olo"]), a["other_lbits"],
                                                 L.p64(a["u"]) if a["u"] is not None else None, C.byref(x), C.byref(y))
        if rc == 0:
            for t in (x, y):
                L.check(zk.lib().zk_table_free(t))
        else:
            assert x.value is None and y.value is None
        return rc

    assert call() == 0 and call(bh=None, bl=None) == 0 and call(ohi=None, olo=None, other=other) == 0
    assert call(ah=None, al=None, bh=None, bl=None, w=w) == 0 and call(ah=None, al=None, bh=None, bl=None, w=w, ohi=None, olo=None, other=other) == 0
    bad = [dict(phase=0), dict(phase=3), dict(phase=1),                              # phase 1 has no halves of the other table
           dict(w=w), dict(ah=None, al=None, bh=None, bl=None),                       # half tables and a weight table; neither
           dict(bl=None), dict(bh=None), dict(al=None), dict(ah=None),
           dict(other=other),                                                       # the other table and its halves
           dict(ohi=None), dict(olo=None), dict(ohi=None, olo=None),
           dict(lbits=0), dict(lbits=OUT_BITS), dict(lbits=5), dict(other_lbits=0), dict(other_lbits=in_bits), dict(other_lbits=2),
           dict(ah=tab(8)), dict(al=tab(32)), dict(bh=tab(32)), dict(bl=tab(8)), dict(ohi=tab(8)), dict(olo=tab(4)),
           dict(ohi=None, olo=None, other=tab(16)), dict(ah=None, al=None, bh=None, bl=None, w=tab(32)),
           dict(ah=tab(16, 3)), dict(bl=tab(16, 3)), dict(olo=tab(8, 3)), dict(ohi=None, olo=None, other=tab(32, 3)), dict(field=3), dict(field=4),
           dict(u=None), dict(out_bits=0), dict(in_bits=0), dict(out_bits=31)]
    for over in bad:
        assert call(**over) == L.ZK_E_ARG, over
