"""CPU: one gate of the sparse GKR prover's table kernels (csrc/gkr_tables.cuh) compiled for the host (tools/gkr_tables_selftest.hip)
against the limb-exact shadow model of tests/_gkr_tables_model.py, for the four fields, and what the model says about the committed
witnesses of tests/golden/gkr_table_witnesses.json (tests/golden/make_gkr_table_witnesses.py).

The chain runs up to three 29-bit-limb Montgomery products per gate without reducing in between and takes ONE conditional subtraction per
stored value.  Uniform operands leave a product at or above p about once in 2^(29 L) / p tries -- never on BLS12-381 Fq, 2^25.3 -- so the
witnesses are built to put each intermediate at p + s.  Checked here:
  - the host program equals the model, in the stored outputs and in every "at least p / at least 2 p" flag, on every witness and on random gates;
  - every witness puts the stages it was built for at or above p: a condition checked while pytest collects this module (load_witnesses);
  - the witnesses discriminate: with the reduction of the weight (phase 1, add gate) or of the final product left out, the model's stored
    outputs differ on the witnesses of that stage.  The third u_reduce_once, in the conversion of the half tables, is NOT observable in the
    stored outputs: an unreduced al' = al U / R + p is a congruent operand below 2 p, the weight stays far below 2 p and the final subtraction
    still yields the canonical value.  What the conversion's witnesses show is that the reduction runs (the host program's flag) and that
    without it the outputs are the same, every intermediate still below 2 p;
  - no intermediate reaches 2 p, every intermediate stays below the bound csrc/gkr_tables.cuh states (chain_bounds), no 64-bit column
    reaches 2^64 (the model asserts it inside every scan), for every witness and for tables of stored p - 1;
  - on BLS12-381 Fq, 10^4 random gates never bring a product of the internal-form chain (weight, halves' product, final) to p."""
import os
import random
import subprocess

import pytest

import _gkr_tables_model as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (0, 1, 2, 3)
RANDOM_GATES = 300
WITNESSES = {f: T.load_witnesses(f) for f in FIELDS}            # replayed by the model while pytest collects: see load_witnesses


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gkr_tables") / "gkr_tables_selftest")
    src = os.path.join(ROOT, "tools", "gkr_tables_selftest.hip")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O2", "-std=c++17", src, "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = [r.split() for r in out.stdout.splitlines()]
        assert len(rows) == len(lines)
        return rows

    return run


def random_gate(rng, field):
    p = T.MODULUS[field]
    phase, op, nw = rng.choice((1, 2)), rng.choice((0, 1)), rng.choice((0, 1, 2))
    kw = {"halves": tuple(rng.randrange(p) for _ in range(2 * nw))} if nw else {"w": rng.randrange(p)}
    if phase == 2 and rng.random() < 0.5:
        kw["other_halves"] = (rng.randrange(p), rng.randrange(p))
    else:
        kw["other"] = rng.randrange(p)
    return phase, op, kw


def check_against_model(selftest, field, cases):
    """cases: (phase, op, kwargs of T.gate) -> the flags of each"""
    rows = selftest([T.selftest_line(field, ph, op, **kw) for ph, op, kw in cases])
    flags = []
    for (ph, op, kw), row in zip(cases, rows):
        x, y, fl = T.parse_selftest_row(field, row)
        mx, my, tr = T.gate(field, ph, op, **kw)
        assert (x, y) == (mx, my) and fl == tr.flags(field), (field, ph, op, kw, fl, tr.flags(field))
        flags.append(fl)
    return flags


def witness_cases(field):
    return [(w, ph, op) for w in WITNESSES[field][0] for ph in T.witness_phases(w) for op in (0, 1)]


@pytest.mark.parametrize("field", FIELDS)
def test_host_program_equals_the_shadow_model_on_witnesses_and_random_gates(selftest, field):
    rng = random.Random(0x6A7E + field)
    cases = [(ph, op, T.witness_kwargs(w)) for w, ph, op in witness_cases(field)]
    nwit = len(cases)
    cases += [random_gate(rng, field) for _ in range(RANDOM_GATES)]
    p = T.MODULUS[field]
    for v in (0, 1, p - 1, T.stored(field, 1), T.stored(field, p - 1)):                       # every operand the same edge value, every form
        cases += [(2, op, {"halves": (v,) * n, "other_halves": (v, v)}) for op in (0, 1) for n in (2, 4)]
        cases += [(ph, 0, {"halves": (v,) * 4, "other": v}) for ph in (1, 2)]
        cases += [(2, 1, {"w": v, "other_halves": (v, v)}), (1, 0, {"w": v, "other": v})]
    flags = check_against_model(selftest, field, cases)
    for (w, ph, op), fl in zip(witness_cases(field), flags[:nwit]):
        assert fl == w["flags"], (field, w["name"])
        assert all(fl[T.STAGES.index(s)] == "1" for s in w["targets"]), (field, w["name"])      # the host program ran the subtraction there


@pytest.mark.parametrize("field", FIELDS)
def test_every_stage_has_a_witness_at_or_above_p(field):
    """al (conversion), the one-product weight, the umul2 weight, the halves' product, umul_std with a table entry and the final product
    through the halves: each alone at s = 1 (or the least s the fixed operands allow) and at a large s; the pairs; the triple on the 9-limb fields"""
    wit, triple = WITNESSES[field]
    names = {w["name"].rsplit("_", 1)[0] for w in wit}
    assert {"al", "weight1", "weight2", "other", "final_table", "final_halves", "weight+final", "other+final", "pm1"} <= names
    for stage in ("al", "weight1", "weight2", "other", "final_table", "final_halves"):
        assert sum(w["name"].startswith(stage + "_") for w in wit) == 2, (field, stage)
    by = {w["name"]: w for w in wit}
    assert len(by["weight1_large"]["halves"]) == 2 and len(by["weight2_large"]["halves"]) == 4
    assert by["weight+final_s1"]["targets"] == ["weight", "final"] and by["other+final_s1"]["targets"] == ["other", "final"]
    if T.ULIMBS[field] == 9:
        assert triple.startswith("found") and by["triple"]["targets"] == ["weight", "other", "final"]
    else:
        assert triple.startswith("not attempted") and "triple" not in by
    assert by["largest_final"]["targets"] == ["weight", "final"]
    p = T.MODULUS[field]
    assert by["pm1_table"]["halves"] == [p - 1] * 4 and by["pm1_halves"]["other_halves"] == [p - 1] * 2


@pytest.mark.parametrize("field", FIELDS)
def test_witnesses_discriminate_a_missing_reduction(field):
    p = T.MODULUS[field]
    seen = {"weight": 0, "final": 0, "conversion": 0}
    for w, ph, op in witness_cases(field):
        kw = T.witness_kwargs(w)
        x, y, tr = T.gate(field, ph, op, **kw)
        assert x < p and y < p
        if "final" in w["targets"]:
            bx, by_, _ = T.gate(field, ph, op, skip=("final",), **kw)
            assert (bx, by_) != (x, y), (field, w["name"], ph, op)
            seen["final"] += 1
        if "weight" in w["targets"] and ph == 1 and op == 0:                               # the add gate of phase 1 sends u_reduce_once(wu) to H1
            bx, by_, _ = T.gate(field, ph, op, skip=("weight",), **kw)
            assert bx == x + p and by_ == y, (field, w["name"])
            seen["weight"] += 1
        if "al" in w["targets"]:
            bx, by_, btr = T.gate(field, ph, op, skip=("conversion",), **kw)
            assert tr.before["al"] >= p and (bx, by_) == (x, y), (field, w["name"])         # not observable: see the module's docstring
            assert btr.before["weight"] % p == tr.before["weight"] % p                      # a congruent operand, p larger
            assert all(btr.level(field, s) in (None, 0, 1) for s in T.STAGES)
            seen["conversion"] += 1
    assert seen["final"] >= 8 and seen["weight"] >= 4 and seen["conversion"] >= 4, seen


@pytest.mark.parametrize("field", FIELDS)
def test_no_intermediate_reaches_2p_and_the_stated_bounds_hold(field):
    p = T.MODULUS[field]
    b = T.chain_bounds(field)
    cases = [(ph, op, T.witness_kwargs(w)) for w, ph, op in witness_cases(field)]
    for v in (p - 1, T.stored(field, p - 1)):
        cases += [(2, 0, {"halves": (v,) * n, "other_halves": (v, v)}) for n in (2, 4)] + [(1, 0, {"halves": (v,) * n, "other": v}) for n in (2, 4)]
    worst = {}
    for ph, op, kw in cases:
        tr = T.gate(field, ph, op, **kw)[2]                                               # asserts every column below 2^64 and every operand's limbs
        assert tr.max_column < 1 << 64
        for s in T.STAGES:
            assert tr.level(field, s) in (None, 0, 1), (field, kw, s)
        for s in ("al", "bl", "hi", "lo"):
            assert tr.before.get(s, 0) < b["conversion"]
        assert tr.before["weight"] < b["weight"] and tr.before.get("other", 0) < b["other"]
        assert tr.before["final"] < (b["final_table"] if "other" in kw else b["final_halves"])
        worst["column"] = max(worst.get("column", 0), tr.max_column)
    assert max(b.values()) < 2 * p
    # umul2's own bound, "a live column collects at most L * 3 * 2^58": the model's largest column is within it
    assert worst["column"] < T.ULIMBS[field] * 3 << 58 < 1 << 64


def test_random_gates_never_reach_p_on_bls12_381_fq(selftest):
    """why the witnesses are needed: 10^4 uniform gates, weights and the other table from halves (three products a gate), and not one product of
    the chain at or above p -- 2^(29 L) / p = 2^25.3.  (The CONVERSION's value, umul_std(U mod p, x) < 1.075 p, and a final umul_std reach p
    in about one gate in 14 and one in 10: those run on random tables too.)"""
    field, rng = 1, random.Random(0xF9)
    p = T.MODULUS[field]
    lines = [T.selftest_line(field, 2, i & 1, halves=tuple(rng.randrange(p) for _ in range(4)), other_halves=(rng.randrange(p), rng.randrange(p)))
             for i in range(10000)]
    rows = selftest(lines)
    conv = 0
    for row in rows:
        fl = T.parse_selftest_row(field, row)[2]
        assert fl[4:] == ["0", "0", "0"], fl
        conv += fl[:4].count("1")
    assert conv > 0
