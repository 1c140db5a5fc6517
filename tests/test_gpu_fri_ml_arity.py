"""GPU: the multilinear opening of a FRI commitment folded by 4 (csrc/fri_ml.cuh fri_ml_fold4_kernel, csrc/zkmle_fri_ml.hip; include/zkmle.h
"FRI commitment opened with a fold arity"), over BLS12-381 Fr and BN254 Fr.  Everything compares byte for byte; no tolerance anywhere.

  fold4      zk_fri_ml_fold4 = two zk_fri_ml_fold calls, both fields, with and without a coset, at the lengths 4 and 8 (one and two lanes),
             2^10 (one workgroup of 256 lanes), 2^11 (two: a table is a power of two, so "one more than a workgroup" is two) and 2^15 (the
             power tables' second level: a product instead of a table read); challenges random and r0, r1 in {0, 1, p - 1}; tables random,
             all p - 1 and all 0; at 4 and 8 also the model's four-point formula.  The operands uniform tables never reach (the second
             subtraction in either pair of the first stage, u0 = u1, u0 + u1 = p, c^2 = p - 1), against two folds of the model up to
             2^14: tests/test_gpu_fri_ml_edges.py
  open       zk_fri_ml_open_points_arity(log_arity = 2) equals the model of tests/_fri_ml_arity_model.py in every output and passes the host
             verifier: d in {3, 4, 6, 10} with f chosen for R = 2, 3, 4, 5, 6, 8 and 9, b in {1, 2}, with and without a coset, P in {1, 2, 8}
  arity 1    through the new entry point: zk_fri_ml_open_points' bytes at d = 6
  statuses   the argument errors come before the device is touched and write nothing"""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import _fri_ml_arity_model as AM
import _fri_ml_cases as FC
import _ntt_model as NM
from oracle import pymodel as M
from test_gpu_fri import hasher_for, table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
FIELDS = (0, 3)
Q = 8


def elem(zk, field, v):
    return zk.from_ints(field, [v])[0]


# ---- the fold ---------------------------------------------------------------------------------------------------------------------------
def check_fold4(zk, field, table, pairs, coset):
    p = NM.MODULUS[field]
    cw = table_of(zk, field, table)
    cs = None if coset == 1 else elem(zk, field, coset)
    cs2 = None if coset == 1 else elem(zk, field, coset * coset % p)
    before = cw.evaluated_values
    for r0, r1 in pairs:
        e0, e1 = elem(zk, field, r0), elem(zk, field, r1)
        got = zk.fri.ml_fold4(cw, e0, e1, cs)
        want = zk.fri.ml_fold(zk.fri.ml_fold(cw, e0, cs), e1, cs2)
        assert len(got) == len(table) // 4
        assert np.array_equal(got.evaluated_values, want.evaluated_values), (len(table), coset != 1, r0, r1)
        if len(table) <= 8:
            assert np.array_equal(got.evaluated_values, to_mont(zk, field, AM.fold4_formula(field, table, r0, r1, coset)))
    assert np.array_equal(cw.evaluated_values, before)        # only read


@pytest.mark.parametrize("with_coset", (False, True))
@pytest.mark.parametrize("loglen", (2, 3, 10, 11, 15))
@pytest.mark.parametrize("field", FIELDS)
def test_fold4_equals_two_folds(zk, field, loglen, with_coset):
    p, n = NM.MODULUS[field], 1 << loglen
    rng = random.Random(131 * loglen + field + with_coset)
    coset = rng.randrange(2, p) if with_coset else 1
    edge = [(r0, r1) for r0 in (0, 1, p - 1) for r1 in (0, 1, p - 1)]
    rand = [(rng.randrange(2, p - 1), rng.randrange(2, p - 1))]
    check_fold4(zk, field, NM.random_ints(field, n, 5100 + loglen + field), rand + (edge if loglen <= 11 else edge[::4]), coset)
    check_fold4(zk, field, [p - 1] * n, rand + [(p - 1, p - 1), (1, 0)], coset)
    check_fold4(zk, field, [0] * n, rand + [(p - 1, 1)], coset)


# ---- the opening ------------------------------------------------------------------------------------------------------------------------
gpu_commitment = FC.gpu_commitment
points_for = functools.partial(FC.points_for, bit_at_1=True)


@functools.lru_cache(maxsize=None)
def model_commitment(zk, field, d, b, with_coset):
    return FC.commitment(field, d, b, FC.coset_of(field, d, b, with_coset, 67), 9700 + 17 * d + b + field, hasher_for(zk, 2 << (d + b)))


def open_raw(zk, gc, pm, f, nq, a, transcript=None):
    """zk_fri_ml_open_points_arity itself (the Python wrapper routes log_arity = 1 to zk_fri_ml_open_points) -> (status, opening)"""
    from zkmle_amd import _lib as L
    op = zk.fri.FriMlPointsOpening(gc.field, pm.shape[0], gc.d, gc.log_blowup, f, nq, gc.coset, a)
    rc = zk.lib().zk_fri_ml_open_points_arity(gc._h, L.p64(pm), pm.shape[0], f, nq, a, None if transcript is None else transcript._h, L.p64(op.ys),
                                              L.p64(op.gamma), L.p64(op.round_polys), L.p8(op.roots), L.p64(op.final_table), L.p64(op.challenges),
                                              L.p64(op.query_indices), L.p64(op.query_values), L.p8(op.query_paths))
    return rc, op


def assert_same_opening(zk, got, fl):
    for name, arr in (("ys", got.ys), ("gamma", got.gamma), ("polys", got.round_polys), ("roots", got.roots), ("final", got.final_table),
                      ("challenges", got.challenges), ("indices", got.query_indices), ("values", got.query_values), ("paths", got.query_paths)):
        assert arr.shape == fl[name].shape and np.array_equal(arr, fl[name]), name


# (field, d, b, f, P, coset): R = 2, 3, 2, 4, 3, 5, 6, 8, 9; every P and b with and without a coset on both fields
CASES = [(0, 3, 1, 1, 1, False), (3, 3, 2, 0, 2, True), (3, 4, 1, 2, 8, False), (0, 4, 2, 0, 2, True), (0, 6, 2, 3, 8, True), (3, 6, 1, 1, 1, True),
         (0, 6, 1, 0, 2, False), (3, 10, 2, 2, 2, False), (0, 10, 1, 1, 1, True), (3, 10, 1, 2, 8, True)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_opening_equals_the_model(zk, case):
    field, d, b, f, P, with_coset = case
    p = NM.MODULUS[field]
    cm = model_commitment(zk, field, d, b, with_coset)
    hasher = hasher_for(zk, 2 << (d + b))
    pts = points_for(field, d, P, d * 1000 + b * 100 + f * 10 + P + field)
    op = AM.open_points(cm, pts, f, Q, hasher=hasher)
    assert AM.verify(op, hasher=hasher)
    fl = AM.flat(zk, op)
    pm = to_mont(zk, field, [v for z in pts for v in z]).reshape(P, d, 4)
    with gpu_commitment(zk, cm) as gc:
        assert gc.root == cm["root"]
        codeword_before = gc.codeword().evaluated_values
        got = zk.fri.open_multilinear_points(gc, pm, f, Q, log_arity=2)
        assert got.log_arity == 2
        assert_same_opening(zk, got, fl)
        assert zk.fri.verify_multilinear_points(gc.root, pm, got)
        assert np.array_equal(gc.codeword().evaluated_values, codeword_before)
        st = zk.fri.ml_last_stats()
        assert st["rounds"] == d - f and st["queries"] == Q
        again = zk.fri.open_multilinear_points(gc, pm, f, Q, log_arity=2)   # the commitment's tables were only read
        assert_same_opening(zk, again, fl)
    bad = zk.fri.FriMlPointsOpening(field, P, d, b, f, Q, got.coset, 2)
    for name in ("ys", "round_polys", "roots", "final_table", "query_values", "query_paths"):
        setattr(bad, name, getattr(got, name).copy())
    bad.ys[P - 1] = to_mont(zk, field, [(op["ys"][P - 1] + 1) % p])[0]
    assert not zk.fri.verify_multilinear_points(cm["root"], pm, bad)


def test_opening_on_a_callers_transcript(zk):
    field, d, b, f, P = 0, 5, 1, 0, 2
    cm = model_commitment(zk, field, d, b, True)
    pts = points_for(field, d, P, 79)
    mt = M.Transcript()
    mt.append(b"before the opening")
    op = AM.open_points(cm, pts, f, Q, mt, hasher=hasher_for(zk, 2 << (d + b)))
    t, v, want = zk.Transcript(), zk.Transcript(), zk.Transcript()
    t.append(b"before the opening")
    v.append(b"before the opening")
    want.append(bytes(mt.buf))
    pm = to_mont(zk, field, [x for z in pts for x in z]).reshape(P, d, 4)
    with gpu_commitment(zk, cm) as gc:
        got = zk.fri.open_multilinear_points(gc, pm, f, Q, transcript=t, log_arity=2)
    assert_same_opening(zk, got, AM.flat(zk, op))
    assert zk.fri.verify_multilinear_points(cm["root"], pm, got, transcript=v)
    assert np.array_equal(t.export_state(), want.export_state()) and np.array_equal(v.export_state(), want.export_state())


@pytest.mark.parametrize("field", FIELDS)
def test_arity_one_through_the_new_entry_point_is_the_several_point_opening(zk, field):
    d, b, f, P = 6, 2, 1, 2
    cm = model_commitment(zk, field, d, b, True)
    pm = to_mont(zk, field, [v for z in points_for(field, d, P, 5 + field) for v in z]).reshape(P, d, 4)
    with gpu_commitment(zk, cm) as gc:
        old = zk.fri.open_multilinear_points(gc, pm, f, Q)
        rc, new = open_raw(zk, gc, pm, f, Q, 1)
        assert rc == 0
        for name in ("ys", "gamma", "round_polys", "roots", "final_table", "challenges", "query_indices", "query_values", "query_paths"):
            a, c = getattr(old, name), getattr(new, name)
            assert a.shape == c.shape and np.array_equal(a, c), name
        assert zk.fri.verify_multilinear_points(gc.root, pm, new, log_arity=1)
        rc, two = open_raw(zk, gc, pm, f, Q, 2)
        assert rc == 0 and not np.array_equal(two.round_polys[0], old.round_polys[0])   # the arity is in the transcript: another gamma


def test_argument_errors_return_the_documented_status_and_write_nothing(zk):
    from zkmle_amd import _lib as L
    field, d, b = 3, 4, 1
    p = NM.MODULUS[field]
    cm = model_commitment(zk, field, d, b, False)
    pm = to_mont(zk, field, NM.random_ints(field, 2 * d, 5)).reshape(2, d, 4)
    fill = np.uint64(0xA5A5A5A5A5A5A5A5)
    with gpu_commitment(zk, cm) as gc:
        def call(points, P, f, nq, a):
            from zkmle_amd import _lib as L
            op = zk.fri.FriMlPointsOpening(field, 2, d, b, 0, 8, None, 2)
            words = (op.ys, op.gamma, op.round_polys, op.final_table, op.challenges, op.query_indices, op.query_values)
            for arr in words:
                arr[...] = fill
            op.roots[...] = 0xA5
            op.query_paths[...] = 0xA5
            rc = zk.lib().zk_fri_ml_open_points_arity(gc._h, L.p64(points), P, f, nq, a, None, L.p64(op.ys), L.p64(op.gamma), L.p64(op.round_polys),
                                                      L.p8(op.roots), L.p64(op.final_table), L.p64(op.challenges), L.p64(op.query_indices),
                                                      L.p64(op.query_values), L.p8(op.query_paths))
            return rc, all((arr == fill).all() for arr in words) and (op.roots == 0xA5).all() and (op.query_paths == 0xA5).all()

        for P, f, nq, a in ((2, 0, 8, 0), (2, 0, 8, 3), (2, 3, 8, 2), (0, 0, 8, 2), (9, 0, 8, 2), (2, 4, 8, 2), (2, 0, 0, 2), (2, 0, 4097, 2)):
            assert call(pm, P, f, nq, a) == (L.ZK_E_ARG, True), (P, f, nq, a)
        assert open_raw(zk, gc, pm, 3, 8, 1)[0] == 0         # R = 1 is an arity-1 opening
        unreduced = pm.copy()
        unreduced[1, 2] = np.frombuffer((int.from_bytes(pm[1, 2].tobytes(), "little") + p).to_bytes(32, "little"), np.uint64)
        assert call(unreduced, 2, 0, 8, 2) == (L.ZK_E_ARG, True)
        with pytest.raises(L.ZkError) as e:
            zk.fri.open_multilinear_points(gc, pm, 3, 8, log_arity=2)
        assert e.value.code == L.ZK_E_ARG
    # the fold
    T = zk.MultilinearPolynomial.random(field, 2, 1)
    one = elem(zk, field, 1)
    with pytest.raises(L.ZkError) as e:
        zk.fri.ml_fold4(T, one, one)
    assert e.value.code == L.ZK_E_ARG
    with pytest.raises(L.ZkError) as e:
        zk.fri.ml_fold4(zk.MultilinearPolynomial.random(field, 8, 1), one, one, np.zeros(4, np.uint64))
    assert e.value.code == L.ZK_E_ARG
