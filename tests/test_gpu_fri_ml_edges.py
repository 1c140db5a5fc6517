"""GPU: the multilinear FRI folds (csrc/fri_ml.cuh: fri_ml_fold_kernel, fri_ml_fold4_kernel, fri_ml_fold_batch_kernel,
fri_ml_fold_batch_wide_kernel) at operands that uniform tables do not reach.  Everything compares byte for byte with Python integers: the
model's fold (tests/_fri_ml_model.py), twice for a fold by 4, which tests/test_fri_ml_edges_cpu.py ties to the four-point formula at every
length.  The tables are those of tests/_fri_ml_edges.py; no tolerance anywhere, and every lane of every result is compared.

  witnesses    lanes whose last step needs the SECOND subtraction of fe_from_u_below_2p (ufield.cuh), which uniform tables take about
               once in 2^28 outputs: the committed (gamma, s, t) of tests/golden/fri_fold_witnesses.json planted so that the lane's
               halved sum is s and its operand w^-k (a - b) - c (a + b) is t.  zk_fri_ml_fold at 2^10 (two workgroups), 2^13 (the last
               one-level power table) and 2^14 (the first two-level one), lanes 0, 255, 256 and the last; zk_fri_ml_fold4 at 2^11, 2^13
               and 2^14 with the witnesses in pair 0, in pair 1 and in both pairs of an output lane, r1 random, 0 and p - 1.  A fold
               without that subtraction leaves s + gamma t + p in exactly those lanes
  structured   the nine tables of tests/test_gpu_fri_edges.py, t = 0 in every lane, stored s = t = p - 1 in every lane, and for the fold
               by 4 a first fold with u0 = u1 and with u0 + u1 = p in every output lane; the cosets none, an explicit 1 (the COSET = true
               instantiation, the bytes of none), p - 1, 1 / 2, w_N, w_2N and, by 4, w_4; r in {0, 1, p - 1, 2 c, p - 2 c} (gamma = 0, 1,
               p - 1) and r1 in the same set of c^2.  Up to 2^9 (by 4: 2^10) every table meets every coset, and with each such pair every
               r, or every r0 and every r1; at 2^13 and 2^14 every table is folded once without and once with a coset, challenge and
               coset rotating with the table
  other tail   zk_fri_ml_fold_batch (k = 2, 16) and zk_fri_ml_fold_batch_wide (k = 17, 32) end in fe_halve(s) + Multiplier(g).times(t)
               instead of the rows of a FriUni.  Given one table k times with coefficients that sum to 1 they fold the table itself, so the
               same witness tables (2^11) and structured tables (2^9) go through them, by 2 and by 4: the header's claim that this tail
               leaves the canonical residue of what the rows give, in the lanes where the rows' value is at or above 2 p"""
import random

import numpy as np
import pytest

import _fri_ml_edges as E
import _fri_ml_model as ML
import _ntt_model as NM
from test_gpu_fri import table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)
from test_gpu_fri_edges import stored_ints

pytestmark = pytest.mark.gpu
FIELDS = (0, 3)
BATCH_KS = (2, 16, 17, 32)                                  # <= 16: zk_fri_ml_fold_batch, above: zk_fri_ml_fold_batch_wide


def elem(zk, field, v):
    return None if v is None else zk.from_ints(field, [v])[0]


def model_fold(field, values, r, coset, r1=None):
    """the model's fold by r, or by (r, r1) its two folds; coset None: 1"""
    p, c = NM.MODULUS[field], 1 if coset is None else coset
    out = ML.fold(field, values, r, c)
    return out if r1 is None else ML.fold(field, out, r1, c * c % p)


def unit_coefficients(field, k, seed):
    """k coefficients that sum to 1: (lambda, 1 - lambda) at k = 2"""
    p = NM.MODULUS[field]
    some = NM.random_ints(field, k - 1, seed)
    return some + [(1 - sum(some)) % p]


def library_fold(zk, field, values, r, coset, r1=None, k=None, seed=0):
    """-> the limbs of zk_fri_ml_fold / zk_fri_ml_fold4 (r1 given) of the canonical `values`, or with k of zk_fri_ml_fold_batch[_wide] on
    k times the same table with coefficients that sum to 1"""
    cw, e0, e1, cs = table_of(zk, field, values), elem(zk, field, r), elem(zk, field, r1), elem(zk, field, coset)
    if k is None:
        got = zk.fri.ml_fold(cw, e0, cs) if r1 is None else zk.fri.ml_fold4(cw, e0, e1, cs)
    else:
        batch = zk.fri.ml_fold_batch if k <= 16 else zk.fri.ml_fold_batch_wide
        got = batch([cw] * k, zk.from_ints(field, unit_coefficients(field, k, 4400 + seed + k)), e0, e1, cs)
    return got.evaluated_values


def fold_mismatches(zk, field, values, r, coset, r1=None, k=None):
    """the library's fold against the model's, element for element -> (the library's limbs, the indices that differ)"""
    have = library_fold(zk, field, values, r, coset, r1, k, seed=len(values))
    want = to_mont(zk, field, model_fold(field, values, r, coset, r1))
    assert have.shape == want.shape
    return have, np.nonzero((have != want).any(axis=1))[0]


def fold_and_compare(zk, field, values, r, coset, what, r1=None, k=None, planted=None):
    """on failure: the first failing indices and their number, as fold_and_compare of tests/test_gpu_fri_edges.py"""
    _, bad = fold_mismatches(zk, field, values, r, coset, r1, k)
    assert bad.size == 0, (what, bad[:8].tolist(), bad.size) + (() if planted is None else ("planted lanes", planted))


def witness_fold_and_compare(zk, field, values, r, coset, what, ts, lanes, planted, r1=None, k=None):
    """a fold of a witness table.  The lanes `lanes` (of `planted`, the output lanes that read a witness) leave s + gamma t: they are looked
    at first, as stored integers, so that a failure names the branch: canonical limbs, and s + gamma t mod p.  Then the whole table"""
    p = NM.MODULUS[field]
    have, bad = fold_mismatches(zk, field, values, r, coset, r1, k)
    at = stored_ints(have[lanes])
    where = (what, "differ from the model", bad[:8].tolist(), bad.size, "planted lanes", planted)
    assert all(v < p for v in at), ("not canonical: the second subtraction of fe_from_u_below_2p", lanes, [hex(v) for v in at]) + where
    assert at == [E.witness_output(field, ts[k]) for k in lanes], (lanes,) + where
    assert bad.size == 0, where


def random_coset(field, seed):
    return random.Random(seed).randrange(2, NM.MODULUS[field])


# ---- the second subtraction ------------------------------------------------------------------------------------------------------------
def fold_witness_table(field, logn, coset):
    """-> (canonical values, r, lanes, {lane: t})"""
    values = NM.random_ints(field, 1 << logn, 9300 + 10 * logn + field)
    lanes = E.fold_lanes(1 << (logn - 1))
    return values, E.plant_fold(field, values, lanes, 1 if coset is None else coset), lanes, E.fold_ts(field, lanes)


def fold4_witness_table(field, logn, coset):
    """-> (canonical values, r0, first-fold lanes, output lanes, output lanes with both pairs planted, {first-fold lane: t})"""
    q = 1 << (logn - 2)
    values = NM.random_ints(field, 1 << logn, 9400 + 10 * logn + field)
    lanes = E.fold4_lanes(q)
    both = [k for k in lanes if k < q and k + q in lanes]
    return values, E.plant_fold4(field, values, lanes, 1 if coset is None else coset), lanes, sorted({k % q for k in lanes}), both, E.fold4_ts(field, q, lanes)


@pytest.mark.parametrize("logn,coset", [(10, "none"), (10, "random"), (10, "explicit 1"), (13, "none"), (13, "random"), (14, "none"), (14, "random")])
@pytest.mark.parametrize("field", FIELDS)
def test_fold_lanes_that_need_the_second_subtraction(zk, field, logn, coset):
    c = {"none": None, "explicit 1": 1, "random": random_coset(field, 79 * logn + field)}[coset]
    values, r, lanes, ts = fold_witness_table(field, logn, c)
    assert lanes == [0, 255, 256, (1 << (logn - 1)) - 1]
    witness_fold_and_compare(zk, field, values, r, c, (field, logn, coset), ts, lanes, lanes)


@pytest.mark.parametrize("with_coset", (False, True))
@pytest.mark.parametrize("logn", (11, 13, 14))
@pytest.mark.parametrize("field", FIELDS)
def test_fold4_lanes_whose_first_stage_needs_the_second_subtraction(zk, field, logn, with_coset):
    """The second stage reduces again, and it returns the right bytes from most u's that are too large by p: a build whose first stage
    lacked the second subtraction differed from the model only in the lanes with both pairs planted, at r1 = p - 1 and without a coset.
    So those lanes and that challenge are what this test must keep."""
    p, q = NM.MODULUS[field], 1 << (logn - 2)
    c = random_coset(field, 83 * logn + field) if with_coset else None
    values, r0, lanes, outs, both, ts = fold4_witness_table(field, logn, c)
    assert lanes == [0, 255, 256, q - 1, q, q + 255, 2 * q - 1] and both == [0, 255, q - 1]      # pair 0 alone: 256; pair 1 is never alone
    # r1 = 0 leaves (u0 + u1) / 2, and both pairs of the lanes in `both` carry the same t: the output is u0 = u1 itself
    witness_fold_and_compare(zk, field, values, r0, c, (field, logn, with_coset, "r1 = 0"), ts, both, outs, r1=0)
    for r1 in (p - 1, random.Random(logn + field).randrange(2, p - 1)):
        fold_and_compare(zk, field, values, r0, c, (field, logn, with_coset, "r1", r1), r1=r1, planted=outs)


@pytest.mark.parametrize("with_coset", (False, True))
@pytest.mark.parametrize("field", FIELDS)
def test_fold4_with_the_witnesses_in_pair_1_alone(zk, field, with_coset):
    """the lanes above never have pair 1 planted without pair 0; here only the second half of the first fold's lanes is planted"""
    logn, p = 11, NM.MODULUS[field]
    q = 1 << (logn - 2)
    c = random_coset(field, 89 + field) if with_coset else None
    values = NM.random_ints(field, 1 << logn, 9500 + field)
    lanes = [q, q + 255, q + 256, 2 * q - 1]
    r0 = E.plant_fold4(field, values, lanes, 1 if c is None else c)
    for r1 in (0, random.Random(field).randrange(2, p - 1)):
        fold_and_compare(zk, field, values, r0, c, (field, with_coset, "r1", r1), r1=r1, planted=[k - q for k in lanes])


# ---- structured tables -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", E.coset_names())
@pytest.mark.parametrize("logn", (1, 2, 8, 9))
@pytest.mark.parametrize("field", FIELDS)
def test_structured_tables_fold_as_the_model_with_every_challenge(zk, field, logn, cname):
    c = E.coset_of(field, logn, cname)
    for tname in E.table_names():
        values = E.structured_table(field, logn, tname, c or 1)
        for r in E.challenges_of(field, c or 1):
            fold_and_compare(zk, field, values, r, c, (field, logn, tname, cname, r))


@pytest.mark.parametrize("cname", E.coset_names(by4=True))
@pytest.mark.parametrize("logn", (2, 3, 9, 10))
@pytest.mark.parametrize("field", FIELDS)
def test_structured_tables_fold_by_4_as_the_model_with_every_challenge(zk, field, logn, cname):
    """with each table every r0 and every r1 once: five folds, the r1's turned by the table's number"""
    p = NM.MODULUS[field]
    c = E.coset_of(field, logn, cname)
    r0s, r1s = E.challenges_of(field, c or 1), E.challenges_of(field, (c or 1) ** 2 % p)
    for j, tname in enumerate(E.table_names(by4=True)):
        for i, r0 in enumerate(r0s):
            values = E.structured_table(field, logn, tname, c or 1, r0)
            fold_and_compare(zk, field, values, r0, c, (field, logn, tname, cname, r0, "r1 number", (i + j) % 5), r1=r1s[(i + j) % 5])


def rotation(field, logn, j, with_coset, by4):
    """-> (coset name, coset, r0, r1) for table number j: the cosets in turn, the five challenges in turn with a step after each round"""
    p = NM.MODULUS[field]
    named = E.coset_names(by4)[1:]                           # without "none"
    cname = named[j % len(named)] if with_coset else "none"
    c = E.coset_of(field, logn, cname)
    r0 = E.challenges_of(field, c or 1)[(j + j // 5) % 5]
    return cname, c, r0, E.challenges_of(field, (c or 1) ** 2 % p)[(2 * j + 1) % 5] if by4 else None


@pytest.mark.parametrize("by4", (False, True), ids=("fold2", "fold4"))
@pytest.mark.parametrize("with_coset", (False, True))
@pytest.mark.parametrize("logn", (13, 14))
@pytest.mark.parametrize("field", FIELDS)
def test_structured_tables_fold_as_the_model_at_the_power_table_boundary(zk, field, logn, with_coset, by4):
    """2^13: the last one-level power table (N / 2 = 4096); 2^14: the first two-level one.  Eleven or thirteen tables against five
    challenges and six or seven cosets: the rotation meets every challenge at least twice and every coset at least once"""
    for j, tname in enumerate(E.table_names(by4)):
        cname, c, r0, r1 = rotation(field, logn, j, with_coset, by4)
        fold_and_compare(zk, field, E.structured_table(field, logn, tname, c or 1, r0), r0, c, (field, logn, tname, cname, r0, r1), r1=r1)


# ---- the other tail: the batch kernels on the same operands ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", BATCH_KS)
@pytest.mark.parametrize("with_coset", (False, True), ids=("plain", "coset"))
@pytest.mark.parametrize("field", FIELDS)
def test_batch_folds_of_the_witness_tables(zk, field, with_coset, k):
    logn, p = 11, NM.MODULUS[field]
    c = random_coset(field, 97 + field) if with_coset else None
    values, r, lanes, ts = fold_witness_table(field, logn, c)
    witness_fold_and_compare(zk, field, values, r, c, (field, with_coset, k, "by 2"), ts, lanes, lanes, k=k)
    values, r0, lanes, outs, both, ts = fold4_witness_table(field, logn, c)
    witness_fold_and_compare(zk, field, values, r0, c, (field, with_coset, k, "by 4, r1 = 0"), ts, both, outs, r1=0, k=k)
    fold_and_compare(zk, field, values, r0, c, (field, with_coset, k, "by 4"), r1=random.Random(k + field).randrange(2, p - 1), k=k, planted=outs)


@pytest.mark.parametrize("by4", (False, True), ids=("fold2", "fold4"))
@pytest.mark.parametrize("with_coset", (False, True), ids=("plain", "coset"))
@pytest.mark.parametrize("field", FIELDS)
def test_batch_folds_of_the_structured_tables(zk, field, with_coset, by4):
    """every table through the narrow and the wide kernel (k = 2 or 16, and 17 or 32), challenge, coset and k rotating with the table"""
    logn = 9
    for j, tname in enumerate(E.table_names(by4)):
        cname, c, r0, r1 = rotation(field, logn, j, with_coset, by4)
        values = E.structured_table(field, logn, tname, c or 1, r0)
        for k in (BATCH_KS[j % 2], BATCH_KS[2 + (j // 2) % 2]):
            fold_and_compare(zk, field, values, r0, c, (field, tname, cname, r0, r1, k), r1=r1, k=k)
