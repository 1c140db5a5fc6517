"""CPU: the arithmetic of the FRI fold's last step compiled for the host (tools/fri_fold_selftest.hip: fe_halve and uni_muladd of
csrc/fri.cuh, unimul_from and fe_from_u_below_2p of csrc/ufield.cuh) against Python integers, over both scalar fields:

  fe_from_u_below_2p(uni_muladd(unimul_from(gamma), s, t)) = s + gamma t mod p   and   fe_halve(x) = x / 2 mod p

on seeded random operands, on the grid {0, 1, 2, p - 2, p - 1, (p - 1) / 2, (p + 1) / 2}^3 (as values and as stored limbs), and on the
committed witnesses of tests/golden/fri_fold_witnesses.json, whose value before the reduction is >= 2 p: uniform operands take the second
subtraction of fe_from_u_below_2p about once in 2^28, so without them that branch is never run.  The same for ufold, a + r (b - a), the
fold of the GKR round kernels (csrc/sumcheck_kernels.cuh), with the witnesses of tests/golden/gkr_ufold_witnesses.json."""
import os
import random
import subprocess

import pytest

import _fri_witness as W
import _ntt_model as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (0, 3)
RANDOM_CASES = 500


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fri_fold") / "fri_fold_selftest")
    src = os.path.join(ROOT, "tools", "fri_fold_selftest.hip")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O2", "-std=c++17", src, "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = [r.split() for r in out.stdout.splitlines()]
        assert len(rows) == len(lines)
        return rows

    return run


def edge_values(p):
    return (0, 1, 2, p - 2, p - 1, (p - 1) // 2, (p + 1) // 2)


def muladd(selftest, field, cases):
    """cases: stored-form (gamma, s, t) -> [(canonical stored result, before >= p, before >= 2 p)], each result checked against Python"""
    p = NM.MODULUS[field]
    rows = selftest(["M %d %s %s %s" % (field, W.int_to_limbs(g), W.int_to_limbs(s), W.int_to_limbs(t)) for g, s, t in cases])
    out = []
    for (g, s, t), row in zip(cases, rows):
        assert row[0] == "M"
        got, ge_p, ge_2p = W.limbs_to_int(row[1:5]), int(row[5]), int(row[6])
        want = (W.real(field, s) + W.real(field, g) * W.real(field, t)) % p
        assert got < p and W.real(field, got) == want, (field, hex(g), hex(s), hex(t), hex(got))
        assert ge_p >= ge_2p
        out.append((got, ge_p, ge_2p))
    return out


@pytest.mark.parametrize("field", FIELDS)
def test_muladd_equals_python_integers_on_random_and_edge_operands(selftest, field):
    p = NM.MODULUS[field]
    rng = random.Random(0xF01D + field)
    cases = [tuple(rng.randrange(p) for _ in range(3)) for _ in range(RANDOM_CASES)]
    edges = edge_values(p)
    cases += [(g, s, t) for g in edges for s in edges for t in edges]                                       # the stored limbs themselves
    cases += [tuple(W.stored(field, v) for v in (g, s, t)) for g in edges for s in edges for t in edges]    # the values
    res = muladd(selftest, field, cases)
    assert any(ge_p for _, ge_p, _ in res) and not all(ge_p for _, ge_p, _ in res)      # both sides of the FIRST subtraction are run


@pytest.mark.parametrize("field", FIELDS)
def test_every_committed_witness_needs_the_second_subtraction(selftest, field):
    gamma, s, ts = W.load(field)
    p = NM.MODULUS[field]
    assert len(set(ts)) >= 3 and s == p - 1 and gamma < p and all(t < p for t in ts)
    for _, ge_p, ge_2p in muladd(selftest, field, [(gamma, s, t) for t in ts]):
        assert ge_p == 1 and ge_2p == 1


@pytest.mark.parametrize("field", FIELDS)
def test_halve_equals_python_integers(selftest, field):
    p = NM.MODULUS[field]
    rng = random.Random(0xA1F + field)
    xs = [rng.randrange(p) for _ in range(RANDOM_CASES)] + list(edge_values(p)) + [W.stored(field, v) for v in edge_values(p)] + [3, p - 3]
    rows = selftest(["H %d %s" % (field, W.int_to_limbs(x)) for x in xs])
    inv2 = pow(2, -1, p)
    for x, row in zip(xs, rows):
        got = W.limbs_to_int(row[1:5])
        assert row[0] == "H" and got == x * inv2 % p, (field, hex(x), hex(got))
        assert W.real(field, got) == W.real(field, x) * inv2 % p


def ufold(selftest, field, cases):
    """cases: stored-form (r, a, b) -> [(canonical stored result, before >= p, before >= 2 p)], each result checked against Python"""
    p = NM.MODULUS[field]
    rows = selftest(["U %d %s %s %s" % (field, W.int_to_limbs(r), W.int_to_limbs(a), W.int_to_limbs(b)) for r, a, b in cases])
    out = []
    for (r, a, b), row in zip(cases, rows):
        assert row[0] == "U"
        got, ge_p, ge_2p = W.limbs_to_int(row[1:5]), int(row[5]), int(row[6])
        want = (W.real(field, a) + W.real(field, r) * (W.real(field, b) - W.real(field, a))) % p
        assert got < p and W.real(field, got) == want, (field, hex(r), hex(a), hex(b), hex(got))
        assert ge_p >= ge_2p
        out.append((got, ge_p, ge_2p))
    return out


@pytest.mark.parametrize("field", FIELDS)
def test_ufold_equals_python_integers_on_random_and_edge_operands(selftest, field):
    p = NM.MODULUS[field]
    rng = random.Random(0xF01E + field)
    cases = [tuple(rng.randrange(p) for _ in range(3)) for _ in range(RANDOM_CASES)]
    edges = edge_values(p)
    cases += [(r, a, b) for r in edges for a in edges for b in edges]
    cases += [tuple(W.stored(field, v) for v in (r, a, b)) for r in edges for a in edges for b in edges]
    res = ufold(selftest, field, cases)
    assert any(ge_p for _, ge_p, _ in res) and not all(ge_p for _, ge_p, _ in res)


@pytest.mark.parametrize("field", FIELDS)
def test_every_committed_ufold_witness_needs_the_second_subtraction(selftest, field):
    r, a, bs = W.load(field, "gkr_ufold_witnesses.json")
    p = NM.MODULUS[field]
    assert len(set(bs)) >= 3 and a == p - 1 and r < p and all(b < p for b in bs)
    for _, ge_p, ge_2p in ufold(selftest, field, [(r, a, b) for b in bs]):
        assert ge_p == 1 and ge_2p == 1
