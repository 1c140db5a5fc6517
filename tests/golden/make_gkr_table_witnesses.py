"""Generator of tests/golden/gkr_table_witnesses.json: operands of ONE gate of the sparse GKR prover's table kernels (csrc/gkr_tables.cuh) at
which a chosen intermediate of the unreduced chain of 29-bit-limb products is at or above p before its reduction, for the four fields.
Uniform operands reach p about once in 2^(29 L) / p products (never, in practice, on BLS12-381 Fq), so no random test takes the chain's
conditional subtractions there.

    python tests/golden/make_gkr_table_witnesses.py        (CPU only, a few seconds; seeded: the file does not depend on the machine)

Construction (tests/_gkr_tables_model.py has the chain; U = 2^(29 L), R = 2^(32 N), all operands canonical stored elements).  A scan of
a b leaves (a b + m p) / U: congruent to a b / U and below a b / U + p.  So with b = s U / a mod p the value is s or p + s, and it is p + s
whenever a b / U exceeds s -- which the model then confirms; the same with two products (solve for the last operand) and with
umul_std (R in place of U).  A converted half v' = v U / R mod p is any canonical value: v = v' R / U mod p.
  al              the conversion of a low half, umul_std(U mod p, al) = p + s
  weight1 / 2     the weight from one product / from two (umul2) = p + s
  other           the product of the other table's converted halves = p + s
  final_table     umul_std(weight, entry) = p + s, the weight from random halves
  final_halves    umul(weight, product of the halves) = p + s
  weight+final    weight = p + s1 and then the entry solved for final = p + s2
  other+final     the halves' product = p + s2 and then the weight's residue solved for final = p + s3
  triple          weight = p + s1, other = p + s2 and final at or above p: (p + s1)(p + s2) / U mod p has to fall below about p^2 / U, one pair
                  (s1, s2) in U / p; searched over s1, s2 <= TRIPLE_SPAN on the 9-limb fields, not attempted on BLS12-381 Fq (one in 2^25)
  pm1             all four half-table entries and the other entry the stored integer p - 1: the largest weight umul2 is given
  largest_final   the weight of weight2's largest witness, the entry solved for the largest final value found
Each stage has s = 1 and a LARGE s: the inequality allows s < a b / U <= a (p - 1) / U =: smax for the chosen first operand a, and a hit
at s needs b(s) >= s U / a, which a random residue passes with probability 1 - s / smax; so the largest hit of DRAWS seeded draws from the top
1 / 32 of [0, smax] is recorded (within a few per cent of the bound; the exact maximum is out of reach of a search)."""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _gkr_tables_model as T                                                          # noqa: E402

SEED, DRAWS, TRIPLE_SPAN = 20261020, 600, 400
NAMES = {0: "bls12_381_fr", 1: "bls12_381_fq", 2: "bn254_fq", 3: "bn254_fr"}
ABOUT = ("Stored-form (Montgomery) operands of one gate of the sparse GKR table kernels (csrc/gkr_tables.cuh) whose named intermediates are "
         "at or above p before their reduction; built by tests/golden/make_gkr_table_witnesses.py from closed forms, see its docstring. "
         "halves = ah al [bh bl], other = the other table's entry or other_halves = hi lo; flags = below p / at least p / at least 2 p (0 / 1 / 2) "
         "for al bl hi lo weight other final as tests/_gkr_tables_model.py and tools/gkr_tables_selftest.hip report them; targets = the stages the "
         "witness was built for; s = their values above p. Elements and s are hexadecimal integers.")


class Field:
    def __init__(self, field):
        self.f, self.p, self.U, self.R = field, T.MODULUS[field], T.radix(field), T.std_radix(field)
        self.rng = random.Random(SEED + field)

    def inv(self, v):
        return pow(v, -1, self.p)

    def rand(self):
        return self.rng.randrange(1, self.p)

    def conv(self, v):                      # a stored half -> its canonical internal form
        return v * self.U * self.inv(self.R) % self.p

    def unconv(self, v):
        return v * self.R * self.inv(self.U) % self.p

    def run(self, w):
        phase = 2 if "other_halves" in w else 1
        return T.gate(self.f, phase, 0, halves=tuple(w["halves"]), other=w.get("other"), other_halves=w.get("other_halves"))[2]

    def hit(self, w, targets):
        tr = self.run(w)
        return all(tr.level(self.f, s) == 1 for s in targets) and all(tr.level(self.f, s) in (None, 0, 1) for s in T.STAGES)


def al_stage(F, s, fixed):
    return {"halves": [fixed["ah"], s * F.R * F.inv(F.U % F.p) % F.p], "other": fixed["x"]}, (F.U % F.p) * (F.p - 1) // F.R


def weight1_stage(F, s, fixed):
    return {"halves": [fixed["ah"], F.unconv(s * F.U * F.inv(fixed["ah"]) % F.p)], "other": fixed["x"]}, fixed["ah"] * (F.p - 1) // F.U


def weight2_stage(F, s, fixed):
    ah, al, bh = fixed["ah"], fixed["al"], fixed["bh"]
    ubl = (s * F.U - ah * F.conv(al)) * F.inv(bh) % F.p
    return {"halves": [ah, al, bh, F.unconv(ubl)], "other": fixed["x"]}, (ah * F.conv(al) + bh * (F.p - 1)) // F.U


def other_stage(F, s, fixed):
    uhi = F.conv(fixed["hi"])
    return ({"halves": [fixed["ah"], fixed["al"], fixed["bh"], fixed["bl"]], "other_halves": [fixed["hi"], F.unconv(s * F.U * F.inv(uhi) % F.p)]},
            uhi * (F.p - 1) // F.U)


def weight_before(F, halves):
    return T.gate(F.f, 1, 0, halves=tuple(halves), other=0)[2].before["weight"]


def final_table_stage(F, s, fixed, halves=None):
    halves = halves or [fixed["ah"], fixed["al"], fixed["bh"], fixed["bl"]]
    wu = weight_before(F, halves)
    return {"halves": halves, "other": s * F.R * F.inv(wu) % F.p}, wu * (F.p - 1) // F.R


def final_halves_stage(F, s, fixed):
    halves = [fixed["ah"], fixed["al"], fixed["bh"], fixed["bl"]]
    wu, uhi = weight_before(F, halves), F.conv(fixed["hi"])
    ulo = s * F.U * F.inv(wu) * F.U * F.inv(uhi) % F.p
    return {"halves": halves, "other_halves": [fixed["hi"], F.unconv(ulo)]}, wu * (F.p - 1) // F.U


STAGE_BUILDERS = (("al", al_stage, ["al"]), ("weight1", weight1_stage, ["weight"]), ("weight2", weight2_stage, ["weight"]),
                  ("other", other_stage, ["other"]), ("final_table", final_table_stage, ["final"]), ("final_halves", final_halves_stage, ["final"]))


def record(F, name, w, targets):
    tr = F.run(w)
    assert all(tr.level(F.f, s) == 1 for s in targets), (F.f, name)
    out = {"name": name, "targets": targets, "s": ["%x" % (tr.before[s] - F.p) for s in targets], "halves": ["%x" % v for v in w["halves"]]}
    if "other" in w:
        out["other"] = "%x" % w["other"]
    else:
        out["other_halves"] = ["%x" % v for v in w["other_halves"]]
    out["flags"] = tr.flags(F.f)
    return out


def one_field(field):
    F = Field(field)
    fixed = {k: F.rand() for k in ("ah", "al", "bh", "bl", "hi", "x")}
    wit, largest = [], {}
    for name, build, targets in STAGE_BUILDERS:
        s = 1
        while not F.hit(build(F, s, fixed)[0], targets):        # s = 1, or the smallest s that the fixed operands allow
            s += 1
            assert s < 64, (field, name)
        wit.append(record(F, "%s_s%d" % (name, s), build(F, s, fixed)[0], targets))
        smax = build(F, 1, fixed)[1]
        best = None
        for _ in range(DRAWS):
            s = smax - F.rng.randrange(smax // 32)
            if (best is None or s > best) and F.hit(build(F, s, fixed)[0], targets):
                best = s
        assert best is not None, (field, name)
        largest[name] = build(F, best, fixed)[0]
        wit.append(record(F, name + "_large", largest[name], targets))
    # weight and final: weight2's witnesses, then the entry solved for the final value
    for tag, s1, s2 in (("s1", 1, 1), ("mixed", 12345, 2)):
        halves = None
        while halves is None or not F.hit(w, ["weight", "final"]):
            halves = weight2_stage(F, s1, fixed)[0]["halves"]
            w = final_table_stage(F, s2, fixed, halves)[0]
            s1 += 1
        wit.append(record(F, "weight+final_" + tag, w, ["weight", "final"]))
    # other and final: the halves' product at p + s2, then a one-product weight whose residue makes the final value p + s3
    for tag, s2, s3 in (("s1", 1, 1), ("mixed", 2, 12345)):
        while True:
            oh = other_stage(F, s2, fixed)[0]["other_halves"]
            oth = T.gate(field, 2, 0, halves=(fixed["ah"], fixed["al"]), other_halves=tuple(oh))[2].before["other"]
            ual = s3 * F.U * F.inv(oth) * F.U * F.inv(fixed["ah"]) % F.p
            w = {"halves": [fixed["ah"], F.unconv(ual)], "other_halves": oh}
            if F.hit(w, ["other", "final"]):
                break
            s2 += 1
        wit.append(record(F, "other+final_" + tag, w, ["other", "final"]))
    # all three at once: a search over (s1, s2), one pair in about U / p
    triple = "not attempted: one pair (s1, s2) in about 2^25"
    if T.ULIMBS[field] == 9:
        triple = "none within %d x %d" % (TRIPLE_SPAN, TRIPLE_SPAN)
        found, inv_u = None, F.inv(F.U)
        for s2 in range(1, TRIPLE_SPAN + 1):
            oh = other_stage(F, s2, fixed)[0]["other_halves"]
            for s1 in range(1, TRIPLE_SPAN + 1):
                s3 = (F.p + s1) * (F.p + s2) * inv_u % F.p
                if s3 * F.U < (F.p + s1) * (F.p + s2):                       # final = p + s3 needs s3 below (p + s1)(p + s2) / U
                    w = {"halves": weight2_stage(F, s1, fixed)[0]["halves"], "other_halves": oh}
                    if F.hit(w, ["weight", "other", "final"]):
                        found = (s1, s2, w)
                        break
            if found:
                break
        if found:
            triple = "found at s1 = %d, s2 = %d" % found[:2]
            wit.append(record(F, "triple", found[2], ["weight", "other", "final"]))
    w = {"halves": [F.p - 1] * 4, "other": F.p - 1}
    wit.append(record(F, "pm1_table", w, []))
    w = {"halves": [F.p - 1] * 4, "other_halves": [F.p - 1] * 2}
    wit.append(record(F, "pm1_halves", w, []))
    # the largest final value: the largest weight witness, the table form (its bound is the widest), the entry for a large s
    halves = largest["weight2"]["halves"]
    smax, best = final_table_stage(F, 1, fixed, halves)[1], None
    for _ in range(DRAWS):
        s = smax - F.rng.randrange(smax // 32)
        if (best is None or s > best) and F.hit(final_table_stage(F, s, fixed, halves)[0], ["weight", "final"]):
            best = s
    assert best is not None
    wit.append(record(F, "largest_final", final_table_stage(F, best, fixed, halves)[0], ["weight", "final"]))
    return {"name": NAMES[field], "triple": triple, "witnesses": wit}


def main():
    out = {"about": ABOUT, "command": "python tests/golden/make_gkr_table_witnesses.py", "seed": SEED, "draws": DRAWS, "triple_span": TRIPLE_SPAN,
           "fields": {str(f): one_field(f) for f in range(4)}}
    with open(os.path.join(HERE, "gkr_table_witnesses.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for f, d in out["fields"].items():
        print(f, d["name"], len(d["witnesses"]), "witnesses; triple:", d["triple"])


if __name__ == "__main__":
    main()
