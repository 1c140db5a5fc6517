"""Integer models of what the sparse GKR prover's table kernels compute per gate (csrc/gkr_tables.cuh, csrc/zkmle_gkr_sparse.hip
phase1_tables_kernel / phase2_tables_kernel).  Helper of tests/test_gkr_tables_cpu.py, tests/test_gpu_gkr_tables.py and
tests/golden/make_gkr_table_witnesses.py.

Two models.  The PLAIN REFERENCE (phase_tables) is the definition: field sums per group over real values, as Python integers.  The SHADOW
MODEL (gate) replays one gate's chain of 29-bit-limb Montgomery products the way the kernel runs it: every scan limb by limb (u_row of
csrc/ufield.cuh: it asserts that no 64-bit column reaches 2^64 and records the largest), every intermediate as the exact integer it has
BEFORE any reduction, every operand of a product checked to have limbs below 2^29 (a normalized value below U = 2^(29 L)), and
u_reduce_once as the ONE conditional subtraction it is -- so a value at or above 2 p would come out wrong here as it would on the GPU.

All table entries are STORED integers (x R mod p, R = 2^(32 N): what the limbs of a table hold).  With U = 2^(29 L), a scan of products
sum a_i b_i leaves (sum a_i b_i + m p) / U with m = -(sum a_i b_i) / p mod U: congruent to (sum a_i b_i) / U and below (sum a_i b_i) / U + p.
The chain (weights from half tables, internal form):
    al' = reduce(umul_std(U mod p, al))                      the low halves times U / R;  the high halves are used as the stored integers
    wu  = umul2(ah, al', bh, bl')  or  umul(ah, al')           the weight in the stored form, not reduced
    fin = umul_std(wu, x)                                     other table entry x, or
    fin = umul(wu, umul(hi', lo')),  hi' lo' = reduce(umul_std(U mod p, hi lo))
    t = limbs32(reduce(fin));  phase 1 also wg = limbs32(reduce(wu))
and with a weight table w: t = w x / R mod p on canonical values, x the entry or hi lo / R mod p.
Phase 1 sends (wg, t) to (H1, H0) at an add gate and (t, 0) at a mul gate; phase 2 sends t to A at an add gate and to M at a mul gate."""
from _foldk_shadow_model import MODULUS, ULIMBS, STD_BITS, stored, real               # noqa: F401

UB = 29
MASK = (1 << UB) - 1
STAGES = ("al", "bl", "hi", "lo", "weight", "other", "final")           # the flag columns of tools/gkr_tables_selftest.hip, in its order
REDUCTIONS = ("conversion", "weight", "final")                          # the three places where the chain calls u_reduce_once


def radix(field):
    return 1 << (UB * ULIMBS[field])


def std_radix(field):
    return 1 << STD_BITS[field]


def shift(field):
    return UB * ULIMBS[field] - STD_BITS[field]


def limbs29(field, v):
    """a product operand: normalized limbs below 2^29, that is a value below U"""
    assert 0 <= v < radix(field), "a product operand with a limb at or above 2^29"
    return [(v >> (UB * j)) & MASK for j in range(ULIMBS[field])]


class Trace:
    """before[stage] = the stage's value before its reduction; max_column = the largest value any 64-bit column held"""

    def __init__(self):
        self.before, self.max_column = {}, 0

    def level(self, field, stage):
        v = self.before.get(stage)
        return None if v is None else min(v // MODULUS[field], 2)

    def flags(self, field):
        return ["-" if self.level(field, s) is None else str(self.level(field, s)) for s in STAGES]


def scan(field, rows, tr):
    """rows[i] = [(a, d), ...]: row i adds a * d for every pair (a: a value below U, d: a 29-bit digit), then takes one Montgomery step.
    -> the value of the normalized columns (u_normalize_columns: asserted below U, its final carry is zero)"""
    p, L = MODULUS[field], ULIMBS[field]
    inv = (-pow(p, -1, 1 << UB)) % (1 << UB)
    pl = [(p >> (UB * j)) & MASK for j in range(L)]
    T = [0] * L
    for row in rows:
        for a, d in row:
            assert 0 <= d <= MASK
            al = limbs29(field, a)
            for j in range(L):
                T[j] += al[j] * d
        m = ((T[0] & 0xFFFFFFFF) * inv) & MASK
        for j in range(L):
            T[j] += m * pl[j]
        tr.max_column = max(tr.max_column, max(T))
        assert max(T) < 1 << 64, "a column overflows 64 bits"
        assert T[0] & MASK == 0
        carry = T[0] >> UB
        T = T[1:] + [0]
        T[0] += carry
        assert T[0] < 1 << 64
    v = sum(t << (UB * j) for j, t in enumerate(T))
    assert v < radix(field), "u_normalize_columns drops a carry"
    return v


def digits(field, v):
    return [(v >> (UB * i)) & MASK for i in range(ULIMBS[field])]


def umul(field, a, b, tr):
    return scan(field, [[(a, d)] for d in digits(field, limbs_value(field, b))], tr)


def limbs_value(field, v):
    limbs29(field, v)
    return v


def umul2(field, a1, b1, a2, b2, tr):
    d1, d2 = digits(field, limbs_value(field, b1)), digits(field, limbs_value(field, b2))
    return scan(field, [[(a1, d1[i]), (a2, d2[i])] for i in range(ULIMBS[field])], tr)


def umul_std(field, a, x, tr):
    """x: a stored element below R; the digits of x << SH are scanned"""
    assert 0 <= x < std_radix(field)
    return scan(field, [[(a, d)] for d in digits(field, x << shift(field))], tr)


def reduce_once(field, v):
    return v - MODULUS[field] if v >= MODULUS[field] else v


def to_limbs32(field, v):
    return v % std_radix(field)                        # u_to_limbs32 keeps the low 32 N bits


def convert(field, x, tr, stage, skip):
    """a low half (or a half of the other table) into the internal form: x U / R, reduced"""
    raw = umul_std(field, radix(field) % MODULUS[field], x, tr)
    tr.before[stage] = raw
    return raw if "conversion" in skip else reduce_once(field, raw)


def gate(field, phase, op, halves=None, w=None, other=None, other_halves=None, skip=()):
    """One gate.  halves = (ah, al) or (ah, al, bh, bl): stored half-table entries, internal-form chain;  else w: the weight, stored.
    other: the other table's entry, or other_halves = (hi, lo).  skip: names of REDUCTIONS to leave out.
    -> (x, y, Trace): the two stored terms as the kernel's LDS slots hold them"""
    p, R = MODULUS[field], std_radix(field)
    tr = Trace()
    assert phase in (1, 2) and op in (0, 1) and (halves is None) != (w is None) and (other is None) != (other_halves is None)
    assert phase == 2 or other_halves is None
    if halves is not None:
        assert len(halves) in (2, 4) and all(0 <= v < p for v in halves)
        al = convert(field, halves[1], tr, "al", skip)
        if len(halves) == 4:
            bl = convert(field, halves[3], tr, "bl", skip)
            wu = umul2(field, halves[0], al, halves[2], bl, tr)
        else:
            wu = umul(field, halves[0], al, tr)
        tr.before["weight"] = wu
        if other is not None:
            assert 0 <= other < p
            fin = umul_std(field, wu, other, tr)
        else:
            assert all(0 <= v < p for v in other_halves)
            hi, lo = convert(field, other_halves[0], tr, "hi", skip), convert(field, other_halves[1], tr, "lo", skip)
            oth = umul(field, hi, lo, tr)
            tr.before["other"] = oth
            fin = umul(field, wu, oth, tr)
        tr.before["final"] = fin
        t = to_limbs32(field, fin if "final" in skip else reduce_once(field, fin))
        wg = to_limbs32(field, wu if "weight" in skip else reduce_once(field, wu)) if phase == 1 else 0
    else:
        rinv = pow(R, -1, p)
        assert 0 <= w < p
        e = other if other is not None else other_halves[0] * other_halves[1] * rinv % p
        wg, t = w, w * e * rinv % p
    if phase == 1:
        return (wg, t, tr) if op == 0 else (t, 0, tr)
    return (t, 0, tr) if op == 0 else (0, t, tr)


def selftest_line(field, phase, op, halves=None, w=None, other=None, other_halves=None):
    n = STD_BITS[field] // 64
    hexs = lambda v: " ".join("%016x" % ((v >> (64 * k)) & (2 ** 64 - 1)) for k in range(n))
    ws = list(halves) if halves is not None else [w]
    os_ = list(other_halves) if other_halves is not None else [other]
    return "G %d %d %d %d %d %s" % (field, phase, op, len(ws) // 2, 1 if other_halves is not None else 0, " ".join(hexs(v) for v in ws + os_))


def parse_selftest_row(field, row):
    """-> (x, y, flags) of a line of tools/gkr_tables_selftest.hip"""
    n = STD_BITS[field] // 64
    val = lambda ws: sum(int(w, 16) << (64 * k) for k, w in enumerate(ws))
    assert row[0] == "G" and len(row) == 1 + 2 * n + len(STAGES)
    return val(row[1:1 + n]), val(row[1 + n:1 + 2 * n]), row[1 + 2 * n:]


def chain_bounds(field):
    """what the chain's values stay below for canonical stored inputs, as exact fractions of p (numerator, p):
    a scan's value is below (its products) / U + p"""
    p, U, R = MODULUS[field], radix(field), std_radix(field)
    q = (p - 1) * (p - 1)
    conv = p + (U % p) * (p - 1) // R + 1                       # umul_std(U mod p, x)
    weight = p + 2 * q // U + 1                                 # two products of operands below p
    oth = p + q // U + 1
    fin_halves = p + weight * oth // U + 1
    fin_table = p + weight * (p - 1) // R + 1                   # the digits of x << SH: wu x 2^SH / U = wu x / R
    return {"conversion": conv, "weight": weight, "other": oth, "final_halves": fin_halves, "final_table": fin_table}


# ---- the plain reference ---------------------------------------------------------------------------------------------------------------------
def gate_weights_real(field, gates, halves=None, lbits=0, w=None):
    """the real weight of every gate (gates: rows of (left, right, out, op))"""
    p = MODULUS[field]
    if w is not None:
        return [real(field, v) for v in w]
    tabs = [[real(field, v) for v in t] for t in halves]
    mask = (1 << lbits) - 1
    out = []
    for g in gates:
        o = g[2]
        v = tabs[0][o >> lbits] * tabs[1][o & mask]
        if len(tabs) == 4:
            v += tabs[2][o >> lbits] * tabs[3][o & mask]
        out.append(v % p)
    return out


def phase_tables(field, phase, gates, in_bits, halves=None, lbits=0, w=None, other=None, other_halves=None, other_lbits=0, u=0):
    """(H1, H0) or (C, A) as lists of 2^in_bits STORED integers; u is a stored element"""
    p = MODULUS[field]
    wr = gate_weights_real(field, gates, halves, lbits, w)
    if other is not None:
        orl = [real(field, v) for v in other]
    else:
        hi, lo = [[real(field, v) for v in t] for t in other_halves]
        orl = [hi[i >> other_lbits] * lo[i & ((1 << other_lbits) - 1)] % p for i in range(1 << in_bits)]
    X, Y = [0] * (1 << in_bits), [0] * (1 << in_bits)
    for (left, right, _, op), wg in zip(gates, wr):
        if phase == 1:
            t = wg * orl[right]
            if op == 0:
                X[left] += wg
                Y[left] += t
            else:
                X[left] += t
        else:
            t = wg * orl[left]
            if op == 0:
                X[right] += t                                   # A
            else:
                Y[right] += t                                   # M
    if phase == 2:
        ur = real(field, u)
        X, Y = [a + ur * m for a, m in zip(X, Y)], X            # C = A + u M, A
    return [stored(field, v % p) for v in X], [stored(field, v % p) for v in Y]


# ---- the committed witnesses -----------------------------------------------------------------------------------------------------------------
def witness_kwargs(w):
    kw = {"halves": tuple(w["halves"])}
    if "other" in w:
        kw["other"] = w["other"]
    else:
        kw["other_halves"] = tuple(w["other_halves"])
    return kw


def witness_phases(w):
    return (2,) if "other_halves" in w else (1, 2)             # the other table's halves exist in phase 2 only


def load_witnesses(field):
    """tests/golden/gkr_table_witnesses.json for one field, as integers.  Every witness is replayed by the shadow model HERE, so a module
    that loads them while pytest collects it fails to collect if a witness does not do what the file says: the recorded flags are the
    model's, and every stage the witness was built for is at or above p (and below 2 p) before its reduction."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gkr_table_witnesses.json")) as f:
        d = json.load(f)["fields"][str(field)]
    out = []
    for rec in d["witnesses"]:
        w = {"name": rec["name"], "targets": list(rec["targets"]), "flags": list(rec["flags"]), "halves": [int(v, 16) for v in rec["halves"]]}
        if "other" in rec:
            w["other"] = int(rec["other"], 16)
        else:
            w["other_halves"] = [int(v, 16) for v in rec["other_halves"]]
        for phase in witness_phases(w):
            for op in (0, 1):
                tr = gate(field, phase, op, **witness_kwargs(w))[2]
                assert tr.flags(field) == w["flags"], (field, w["name"], tr.flags(field))
                assert all(tr.level(field, s) == 1 for s in w["targets"]), (field, w["name"])
                assert [tr.before[s] - MODULUS[field] for s in w["targets"]] == [int(s, 16) for s in rec["s"]], (field, w["name"])
        out.append(w)
    return out, d["triple"]
