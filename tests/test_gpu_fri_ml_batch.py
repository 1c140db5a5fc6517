"""GPU: several FRI commitments opened as multilinear polynomials with one proof (csrc/fri_ml.cuh fri_ml_fold_batch_kernel, csrc/zkmle_fri_ml.hip
zk_fri_ml_fold_batch and zk_fri_ml_open_batch; include/zkmle.h "FRI commitments opened together"), over BLS12-381 Fr and BN254 Fr.  Everything
is byte for byte; no tolerance anywhere.

  fold      zk_fri_ml_fold_batch equals zk_fri_ml_fold4 (r1 = None: zk_fri_ml_fold) of zk_mle_linear_combination of the codewords: both fields,
            with and without a coset, every length 2^2 .. 2^15 (fold by 2: from 2^1), k in {1, 2, 4, 5, 16} (one group of the lazy sum's four
            products, one past it, the maximum); 2^20 with k = 3 (the grid-stride loop runs more than once); and the operands random tables
            never reach: every entry and coefficient p - 1 at k = 16, all zeros, one table passed twice, r0 and r1 in {0, 1, p - 1}.
            Against the model's integers, in the lanes where the single-table kernels need their second subtraction and on structured
            tables, at k = 2 and 16: tests/test_gpu_fri_ml_edges.py
  opening   equals the model of tests/_fri_ml_batch_model.py in every output on the cases of tests/test_fri_ml_batch_cpu.py (k in {1, 2, 5}, the
            three schedules) and passes zk_fri_ml_verify_batch; a caller's transcript ends in the verifier's state
  k = 1     the claims are those of zk_fri_ml_open_points_arity on the same commitment.  The round polynomials, later roots and final table
            are NOT compared with that opening: gamma and every r_l are hashes of a transcript that holds the 16-byte tag here and does not
            there, and nothing a caller absorbs in front can make the two agree.  They are compared with the model only.
  refusals  mixed d, mixed coset, mixed log_group, k = 0, k = 17, grouped commitments with log_arity = 1: ZK_E_ARG, nothing written"""
import ctypes as C
import random

import numpy as np
import pytest

import _fri_ml_batch_model as BM
import _fri_ml_cases as FC
import _ntt_model as NM
from oracle import pymodel as M
from test_fri_ml_batch_cpu import CASES, KS, SCHEDULES, case_id, commitment, hasher, points_for, sched_id
from test_gpu_fri import table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
Q = 8
FIELDS = (0, 3)
FOLD_KS = (1, 2, 4, 5, 16)


def elem(zk, field, v):
    return zk.from_ints(field, [v])[0]


def reference_fold(zk, tables, coeffs, r0, r1, cs):
    comb = zk.MultilinearPolynomial.linear_combination(tables, coeffs)
    return zk.fri.ml_fold(comb, r0, cs) if r1 is None else zk.fri.ml_fold4(comb, r0, r1, cs)


def check_fold(zk, tables, coeffs, r0, r1, cs, what):
    got = zk.fri.ml_fold_batch(tables, coeffs, r0, r1, cs)
    want = reference_fold(zk, tables, coeffs, r0, r1, cs)
    assert len(got) == len(want) == len(tables[0]) // (2 if r1 is None else 4), what
    assert np.array_equal(got.evaluated_values, want.evaluated_values), what


@pytest.mark.parametrize("by4", (False, True), ids=("fold2", "fold4"))
@pytest.mark.parametrize("with_coset", (False, True), ids=("plain", "coset"))
@pytest.mark.parametrize("field", FIELDS)
def test_fold_batch_equals_the_fold_of_the_combination(zk, field, with_coset, by4):
    p = NM.MODULUS[field]
    rng = random.Random(733 * field + 2 * with_coset + by4)
    cs = elem(zk, field, rng.randrange(2, p)) if with_coset else None
    for loglen in range(2 if by4 else 1, 16):
        tables = [zk.MultilinearPolynomial.random(field, 1 << loglen, 5000 + 31 * loglen + j) for j in range(max(FOLD_KS))]
        for k in FOLD_KS:
            coeffs = zk.from_ints(field, [rng.randrange(p) for _ in range(k)])
            r0, r1 = elem(zk, field, rng.randrange(p)), elem(zk, field, rng.randrange(p)) if by4 else None
            check_fold(zk, tables[:k], coeffs, r0, r1, cs, (loglen, k))


@pytest.mark.parametrize("by4", (False, True), ids=("fold2", "fold4"))
@pytest.mark.parametrize("field", FIELDS)
def test_fold_batch_at_a_length_the_grid_covers_more_than_once(zk, field, by4):
    p = NM.MODULUS[field]
    rng = random.Random(97 + field + by4)
    tables = [zk.MultilinearPolynomial.random(field, 1 << 20, 6100 + j) for j in range(3)]
    coeffs = zk.from_ints(field, [rng.randrange(p) for _ in range(3)])
    check_fold(zk, tables, coeffs, elem(zk, field, rng.randrange(p)), elem(zk, field, rng.randrange(p)) if by4 else None,
               elem(zk, field, rng.randrange(2, p)), "2^20")


@pytest.mark.parametrize("with_coset", (False, True), ids=("plain", "coset"))
@pytest.mark.parametrize("field", FIELDS)
def test_fold_batch_at_operands_random_tables_never_reach(zk, field, with_coset):
    p, n = NM.MODULUS[field], 1 << 9
    rng = random.Random(389 + field + with_coset)
    cs = elem(zk, field, rng.randrange(2, p)) if with_coset else None
    top = table_of(zk, field, [p - 1] * n)
    zeros = table_of(zk, field, [0] * n)
    rnd = zk.MultilinearPolynomial.random(field, n, 77)
    edge = [elem(zk, field, v) for v in (0, 1, p - 1)]
    some = elem(zk, field, rng.randrange(p))
    for r1 in (None, some):
        # the lazy sum's bound: 16 products of (p - 1)(p - 1) before the one reduction
        check_fold(zk, [top] * 16, zk.from_ints(field, [p - 1] * 16), some, r1, cs, "all p - 1")
        check_fold(zk, [top] * 16, zk.from_ints(field, [p - 1] * 16), edge[2], None if r1 is None else edge[2], cs, "all p - 1, r = p - 1")
        check_fold(zk, [zeros] * 5, zk.from_ints(field, [rng.randrange(p) for _ in range(5)]), some, r1, cs, "zeros")
        check_fold(zk, [rnd, zeros, rnd], zk.from_ints(field, [0, 5, 0]), some, r1, cs, "zero coefficients")
        # the same table twice: c_0 f + c_1 f, and f - f
        check_fold(zk, [rnd, rnd], zk.from_ints(field, [rng.randrange(p), rng.randrange(p)]), some, r1, cs, "twice")
        check_fold(zk, [rnd, rnd], zk.from_ints(field, [1, p - 1]), some, r1, cs, "f - f")
    tabs = [rnd, zk.MultilinearPolynomial.random(field, n, 78), top]
    coeffs = zk.from_ints(field, [rng.randrange(p) for _ in range(3)])
    for r0 in edge:
        check_fold(zk, tabs, coeffs, r0, None, cs, "r0 edge")
        for r1 in edge:
            check_fold(zk, tabs, coeffs, r0, r1, cs, "r0, r1 edge")


# ---- the opening --------------------------------------------------------------------------------------------------------------------------
gpu_commitment = FC.gpu_commitment


def assert_same_opening(got, fl):
    for name, arr in (("ys", got.ys), ("gamma", got.gamma), ("polys", got.round_polys), ("roots", got.roots), ("final", got.final_table),
                      ("challenges", got.challenges), ("indices", got.query_indices), ("values", got.query_values), ("paths", got.query_paths)):
        assert arr.shape == fl[name].shape and np.array_equal(arr, fl[name]), name


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_opening_equals_the_model(zk, case, sched):
    field, d, b, f, P, with_coset = case
    a, grouped = sched
    p = NM.MODULUS[field]
    pts = points_for(field, d, P)
    pm = to_mont(zk, field, [v for z in pts for v in z]).reshape(P, d, 4)
    cms = [commitment(field, d, b, with_coset, grouped, j) for j in range(max(KS))]
    gcs = [gpu_commitment(zk, cm) for cm in cms]
    try:
        for k in KS:
            op = BM.open_batch(cms[:k], pts, f, Q, a, hasher=hasher())
            fl = BM.flat(zk, op)
            got = zk.fri.open_multilinear_batch(gcs[:k], pm, f, Q, log_arity=a)
            assert got.k == k and got.log_arity == a and got.grouped == grouped
            assert_same_opening(got, fl)
            roots = [gc.root for gc in gcs[:k]]
            assert roots == op["own_roots"] and zk.fri.verify_multilinear_batch(roots, pm, got)
            st = zk.fri.ml_last_stats()
            assert st["rounds"] == d - f and st["queries"] == Q
            if k > 1:
                assert not zk.fri.verify_multilinear_batch(roots[1:] + roots[:1], pm, got)
            bad = zk.fri.FriMlBatchOpening(field, k, P, d, b, f, Q, got.coset, a, grouped)
            for name in ("ys", "round_polys", "roots", "final_table", "query_values", "query_paths"):
                setattr(bad, name, getattr(got, name).copy())
            bad.ys[k - 1, P - 1] = to_mont(zk, field, [(op["ys"][k - 1][P - 1] + 1) % p])[0]
            assert not zk.fri.verify_multilinear_batch(roots, pm, bad)
        # k = 1: the claims of the single-table opening of the same commitment (the rest is bound to another transcript: see the module's text)
        single = zk.fri.open_multilinear_points(gcs[0], pm, f, Q, log_arity=a)
        one = zk.fri.open_multilinear_batch(gcs[:1], pm, f, Q, log_arity=a)
        assert np.array_equal(one.ys[0], single.ys) and np.array_equal(one.roots[0], single.roots[0])
        assert one.roots.shape == single.roots.shape and one.query_paths.shape == single.query_paths.shape
        assert zk.fri.verify_multilinear_points(gcs[0].root, pm, single)   # the commitments were only read
    finally:
        for gc in gcs:
            gc.free()


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_opening_on_a_callers_transcript(zk, sched):
    field, d, b, f, P, k = 0, 6, 1, 1, 2, 3
    a, grouped = sched
    cms = [commitment(field, d, b, True, grouped, j) for j in range(k)]
    pts = points_for(field, d, P)
    mt = M.Transcript()
    mt.append(b"before the opening")
    op = BM.open_batch(cms, pts, f, Q, a, mt, hasher=hasher())
    t, v, want = zk.Transcript(), zk.Transcript(), zk.Transcript()
    t.append(b"before the opening")
    v.append(b"before the opening")
    want.append(bytes(mt.buf))
    pm = to_mont(zk, field, [x for z in pts for x in z]).reshape(P, d, 4)
    gcs = [gpu_commitment(zk, cm) for cm in cms]
    try:
        got = zk.fri.open_multilinear_batch(gcs, pm, f, Q, log_arity=a, transcript=t)
    finally:
        for gc in gcs:
            gc.free()
    assert_same_opening(got, BM.flat(zk, op))
    assert zk.fri.verify_multilinear_batch(op["own_roots"], pm, got, transcript=v)
    assert np.array_equal(t.export_state(), want.export_state()) and np.array_equal(v.export_state(), want.export_state())
    assert not zk.fri.verify_multilinear_batch(op["own_roots"], pm, got)   # bound to the prior content


def test_refusals_write_nothing(zk):
    from zkmle_amd import _lib as L
    lib = zk.lib()
    field, nq = 3, 8
    p = NM.MODULUS[field]
    mk = lambda d, b, coset, lg, seed: zk.fri.commit(zk.MultilinearPolynomial.random(field, 1 << d, seed), b, coset, log_group=lg)
    c1, c2 = elem(zk, field, 5), elem(zk, field, 7)
    base, same, other_d, other_b = mk(4, 1, None, 0, 1), mk(4, 1, None, 0, 2), mk(5, 1, None, 0, 3), mk(4, 2, None, 0, 4)
    cos1, cos2, grp, grp2 = mk(4, 1, c1, 0, 5), mk(4, 1, c2, 0, 6), mk(4, 1, None, 2, 7), mk(4, 1, None, 2, 8)
    every = (base, same, other_d, other_b, cos1, cos2, grp, grp2)
    pm = to_mont(zk, field, NM.random_ints(field, 2 * 5, 5)).reshape(-1, 4)
    FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
    w = lambda n: np.full(n, FILL, np.uint64)
    by = lambda n: np.full(n, 0xA5, np.uint8)
    ys, gamma, polys, roots, fin, chal, idx, vals, paths = w(17 * 8), w(4), w(4 * 3 * 5), by(32 * 24), w(4 << 5), w(4 * 5), w(nq), w(4 * nq * 80), by(32 * nq * 600)
    outs = (ys, gamma, polys, roots, fin, chal, idx, vals, paths)

    def raw(cms, k=None, a=1, f=0):
        hs = (C.c_void_p * 17)(*[c._h for c in cms])
        return lib.zk_fri_ml_open_batch(hs, len(cms) if k is None else k, L.p64(pm), 2, f, nq, a, None, L.p64(ys), L.p64(gamma), L.p64(polys), L.p8(roots),
                                        L.p64(fin), L.p64(chal), L.p64(idx), L.p64(vals), L.p8(paths))

    try:
        for cms, kw in (([base, other_d], {}), ([other_d, base], {}), ([base, other_b], {}), ([base, cos1], {}), ([cos1, base], {}), ([cos1, cos2], {}),
                        ([base, grp], {}), ([grp, base], dict(a=2)), ([base, same], dict(k=0)), ([base] * 17, {}), ([grp, grp2], dict(a=1)),
                        ([base, same], dict(a=0)), ([base, same], dict(a=3)), ([base, same], dict(f=4)), ([base, same], dict(a=2, f=3))):
            assert raw(cms, **kw) == L.ZK_E_ARG, (len(cms), kw)
            assert all((o == (FILL if o.dtype == np.uint64 else 0xA5)).all() for o in outs), kw
        pts = pm[:8].reshape(2, 4, 4)
        with pytest.raises(ValueError):
            zk.fri.open_multilinear_batch([grp, grp2], pts, 0, nq)
        # what was refused in one company is still good for an opening in another
        for cms, a in (([base, same], 1), ([base, same, base], 2), ([cos1, cos1], 1), ([grp, grp2], 2)):
            got = zk.fri.open_multilinear_batch(cms, pts, 0, nq, log_arity=a)
            assert zk.fri.verify_multilinear_batch([c.root for c in cms], pts, got)
    finally:
        for c in every:
            c.free()
