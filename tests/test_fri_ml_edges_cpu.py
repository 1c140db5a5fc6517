"""CPU: the tables of tests/_fri_ml_edges.py do what tests/test_gpu_fri_ml_edges.py relies on, in Python integers alone.

  unfold        inverts the model's fold (tests/_fri_ml_model.py): the lane sees the chosen S and T and leaves S + (r / 2c) T
  planted       as STORED integers a planted lane's halved sum and operand are exactly a committed (s, t) of
                tests/golden/fri_fold_witnesses.json, gamma = r / 2c is the file's, and the model's output there is s + gamma t mod p: the
                triples tests/test_fri_arith_cpu.py shows to need the second subtraction of fe_from_u_below_2p.  For a fold and for both
                pairs of a fold by 4
  structured    each table has the property it is named for in the operands the kernel sees: the parity of the stored sum, t = 0, stored
                s = t = p - 1, and after the first fold u0 = u1 and u0 + u1 = p
  two models    the four-point formula (tests/_fri_ml_arity_model.py) equals two folds of the model on every planted and structured table
                at 2^2 .. 2^10, so either is a reference for a fold by 4 at every length"""
import random

import pytest

import _fri_ml_arity_model as AM
import _fri_ml_edges as E
import _fri_ml_model as ML
import _fri_witness as W
import _ntt_model as NM

FIELDS = (0, 3)


def shift(field, seed, with_coset):
    return random.Random(seed).randrange(2, NM.MODULUS[field]) if with_coset else 1


@pytest.mark.parametrize("with_coset", (False, True))
@pytest.mark.parametrize("field", FIELDS)
def test_unfold_inverts_the_models_fold(field, with_coset):
    p = NM.MODULUS[field]
    rng = random.Random(31 + field + with_coset)
    for logn in (1, 2, 5, 10):
        n = 1 << logn
        h, c = n // 2, shift(field, logn + field, with_coset)
        w = NM.root_of_unity(field, logn)
        values, r = NM.random_ints(field, n, 60 + logn + field), rng.randrange(p)
        chosen = {}
        for k in E.fold_lanes(h):
            S, T = rng.choice((0, 1, p - 1, rng.randrange(p))), rng.choice((0, 1, p - 1, rng.randrange(p)))
            a, b = values[k], values[k + h] = E.unfold(field, n, k, c, S, T)
            assert 0 <= a < p and 0 <= b < p
            assert (a + b) % p == 2 * S % p and (pow(w, -k, p) * (a - b) - c * (a + b)) % p == T
            chosen[k] = (S, T)
        out = ML.fold(field, values, r, c)
        for k, (S, T) in chosen.items():
            assert out[k] == (S + r * pow(2 * c, -1, p) * T) % p, (logn, k)
        Ss, Ts = NM.random_ints(field, h, 61 + logn), NM.random_ints(field, h, 62 + logn)      # the whole table at once: the same pairs
        whole = E.unfold_all(field, n, c, Ss, Ts)
        assert all((whole[k], whole[k + h]) == E.unfold(field, n, k, c, Ss[k], Ts[k]) for k in range(h))
        assert ML.fold(field, E.fold_target(field, n, c, r, Ss, 63), r, c) == Ss and ML.fold(field, E.fold_target(field, n, c, 0, Ss, 64), 0, c) == Ss


def assert_lane_is_a_witness(field, n, c, values, k, t, r, out):
    p = NM.MODULUS[field]
    gamma, s, ts = W.load(field)
    assert t in ts and W.stored(field, r * pow(2 * c, -1, p)) == gamma
    assert E.stored_operands(field, n, k, c, values[k], values[k + n // 2]) == (s, t), k
    assert W.stored(field, out[k]) == (s + W.real(field, gamma) * t) % p == E.witness_output(field, t), k


@pytest.mark.parametrize("with_coset", (False, True))
@pytest.mark.parametrize("field", FIELDS)
def test_planted_lanes_of_a_fold_carry_the_committed_operands(field, with_coset):
    logn = 10
    n, c = 1 << logn, shift(field, 7 + field, with_coset)
    values = NM.random_ints(field, n, 70 + field)
    before = list(values)
    lanes = E.fold_lanes(n // 2)
    assert lanes == [0, 255, 256, 511]
    r = E.plant_fold(field, values, lanes, c)
    ts = E.fold_ts(field, lanes)
    assert len(set(ts.values())) >= 3                                                     # the file's t's in turn
    out = ML.fold(field, values, r, c)
    for k in lanes:
        assert_lane_is_a_witness(field, n, c, values, k, ts[k], r, out)
    touched = set(lanes) | {k + n // 2 for k in lanes}
    assert all(values[i] == before[i] for i in range(n) if i not in touched)


@pytest.mark.parametrize("with_coset", (False, True))
@pytest.mark.parametrize("field", FIELDS)
def test_planted_lanes_of_a_fold_by_4_carry_the_committed_operands_in_both_pairs(field, with_coset):
    p, logn = NM.MODULUS[field], 11
    n, c = 1 << logn, shift(field, 9 + field, with_coset)
    q = n // 4
    values = NM.random_ints(field, n, 80 + field)
    lanes = E.fold4_lanes(q)
    assert lanes == [0, 255, 256, 511, 512, 767, 1023]
    r0 = E.plant_fold4(field, values, lanes, c)
    ts = E.fold4_ts(field, q, lanes)
    first = ML.fold(field, values, r0, c)
    for k in lanes:                                          # pair 0 (k < q) reads k and k + 2q, pair 1 k and k + 2q of the lane k >= q
        assert_lane_is_a_witness(field, n, c, values, k, ts[k], r0, first)
    both = [k for k in range(q) if k in lanes and k + q in lanes]
    assert both == [0, 255, 511] and 256 in lanes and 256 + q not in lanes
    for r1 in (0, 1, p - 1, random.Random(field).randrange(p)):
        out = AM.fold4_formula(field, values, r0, r1, c)
        assert out == ML.fold(field, first, r1, c * c % p)
        if r1 == 0:                                          # the same t in both pairs: u0 = u1, and r1 = 0 leaves their mean
            assert all(ts[k] == ts[k + q] and W.stored(field, out[k]) == E.witness_output(field, ts[k]) for k in both)


def stored_first_fold(field, logn, values, r0, c):
    return [W.stored(field, v) for v in ML.fold(field, values, r0, c)]


@pytest.mark.parametrize("cname", E.coset_names(by4=True))
@pytest.mark.parametrize("logn", (2, 3, 9))
@pytest.mark.parametrize("field", FIELDS)
def test_structured_tables_have_the_property_they_are_named_for(field, logn, cname):
    p, n = NM.MODULUS[field], 1 << logn
    h, q = n // 2, n // 4
    c = E.coset_of(field, logn, cname) or 1
    if cname == "w_4":
        assert c * c % p == p - 1
    assert len(E.table_names()) == 11 and len(E.table_names(by4=True)) == 13
    for name in E.table_names():
        values = E.structured_table(field, logn, name, c)
        assert len(values) == n and all(0 <= v < p for v in values), name
        ops = [E.stored_operands(field, n, k, c, values[k], values[k + h]) for k in range(h)]
        sums = [(W.stored(field, values[k]) + W.stored(field, values[k + h])) % p for k in range(h)]      # what fe_halve tests
        if name == "halved sum odd":
            assert all(v % 2 == 1 for v in sums)
        elif name == "halved sum even":
            assert all(v % 2 == 0 for v in sums)
        elif name == "t == 0":
            assert all(t == 0 for _, t in ops) and len({s for s, _ in ops}) == h
        elif name == "stored s == t == p - 1":
            assert all(o == (p - 1, p - 1) for o in ops)
        elif name == "a == b":
            assert all(values[k] == values[k + h] for k in range(h))
        elif name == "a + b == p":
            assert all(v == 0 for v in sums)
    for r0 in E.challenges_of(field, c):
        for name in E.FOLD4_ONLY:
            u = stored_first_fold(field, logn, E.structured_table(field, logn, name, c, r0), r0, c)
            if name == "u0 == u1":
                assert all(u[k] == u[k + q] != 0 for k in range(q)), (name, r0)
            else:
                assert all(u[k] + u[k + q] == p for k in range(q)), (name, r0)


@pytest.mark.parametrize("logn", range(2, 11))
@pytest.mark.parametrize("field", FIELDS)
def test_the_four_point_formula_equals_two_folds_of_the_model(field, logn):
    p, n = NM.MODULUS[field], 1 << logn
    cosets = E.coset_names(by4=True)
    tables = [(name, None) for name in E.table_names(by4=True)] + [("planted", False), ("planted", True)]
    for j, (name, with_coset) in enumerate(tables):
        if name == "planted":
            c = shift(field, logn, with_coset)
            values = NM.random_ints(field, n, 90 + logn + field)
            r0 = E.plant_fold4(field, values, E.fold4_lanes(n // 4), c)
        else:
            c = E.coset_of(field, logn, cosets[(j + logn) % len(cosets)]) or 1
            r0 = E.challenges_of(field, c)[(j + j // 5) % 5]
            values = E.structured_table(field, logn, name, c, r0)
        c2 = c * c % p
        for r1 in (E.challenges_of(field, c2)[(2 * j + 1) % 5], random.Random(j + logn).randrange(p)):
            assert AM.fold4_formula(field, values, r0, r1, c) == ML.fold(field, ML.fold(field, values, r0, c), r1, c2), (name, c, r0, r1)
