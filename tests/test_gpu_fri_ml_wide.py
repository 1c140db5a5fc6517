"""GPU: up to 32 FRI commitments opened as multilinear polynomials with one proof (csrc/fri_ml.cuh fri_ml_fold_batch_wide_kernel,
csrc/zkmle_fri_ml.hip zk_fri_ml_fold_batch_wide and zk_fri_ml_open_batch_wide_pow; include/zkmle.h "FRI commitments opened together, wide"),
over BLS12-381 Fr and BN254 Fr.  Everything is byte for byte; no tolerance anywhere.

  fold      zk_fri_ml_fold_batch_wide at k = 17, 20 and 32 equals zk_fri_ml_fold4 (r1 = None: zk_fri_ml_fold) of zk_mle_linear_combination of
            the codewords: both fields, with and without a coset, every codeword length 2^2 .. 2^12, fold by 2 and by 4; at k = 1, 9 and 16 it
            equals zk_fri_ml_fold_batch; every entry and coefficient p - 1 at k = 32 (the one reduction's bound), and zeros; once at length
            2^20 with k = 17 built from three distinct tables repeated: the second trip of the kernel's grid-stride loop at 768 blocks.
            Against the model's integers, in the lanes where the single-table kernels need their second subtraction and on structured
            tables, at k = 17 and 32: tests/test_gpu_fri_ml_edges.py
  opening   zk_fri_ml_open_batch_wide_pow at k = 17, 20 and 32, d = 4 .. 8, the three schedules, equals the model of
            tests/_fri_ml_wide_model.py in every output and passes zk_fri_ml_verify_batch_wide_pow; once with 8 bits of proof of work; at k = 9
            it equals zk_fri_ml_open_batch_pow byte for byte
  refusals  k = 33, k = 0, mixed shapes: ZK_E_ARG, nothing written; the narrow opener still refuses k = 17"""
import ctypes as C
import random

import numpy as np
import pytest

import _fri_ml_cases as FC
import _fri_ml_wide_model as WB
import _ntt_model as NM
from test_fri_ml_wide_cpu import SCHEDULES, coset_of, hasher, sched_id
from test_gpu_fri import table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
Q = 6
FIELDS = (0, 3)
WIDE_KS, NARROW_KS = (17, 20, 32), (1, 9, 16)


def elem(zk, field, v):
    return zk.from_ints(field, [v])[0]


def reference_fold(zk, tables, coeffs, r0, r1, cs):
    comb = zk.MultilinearPolynomial.linear_combination(tables, coeffs)
    return zk.fri.ml_fold(comb, r0, cs) if r1 is None else zk.fri.ml_fold4(comb, r0, r1, cs)


def check_fold(zk, tables, coeffs, r0, r1, cs, what):
    got = zk.fri.ml_fold_batch_wide(tables, coeffs, r0, r1, cs)
    want = reference_fold(zk, tables, coeffs, r0, r1, cs)
    assert len(got) == len(want) == len(tables[0]) // (2 if r1 is None else 4), what
    assert np.array_equal(got.evaluated_values, want.evaluated_values), what
    return got


@pytest.mark.parametrize("by4", (False, True), ids=("fold2", "fold4"))
@pytest.mark.parametrize("with_coset", (False, True), ids=("plain", "coset"))
@pytest.mark.parametrize("field", FIELDS)
def test_the_wide_fold_equals_the_fold_of_the_combination(zk, field, with_coset, by4):
    p = NM.MODULUS[field]
    rng = random.Random(739 * field + 2 * with_coset + by4)
    cs = elem(zk, field, rng.randrange(2, p)) if with_coset else None
    for loglen in range(2, 13):
        tables = [zk.MultilinearPolynomial.random(field, 1 << loglen, 7000 + 37 * loglen + j) for j in range(32)]
        for k in WIDE_KS + NARROW_KS:
            coeffs = zk.from_ints(field, [rng.randrange(p) for _ in range(k)])
            r0, r1 = elem(zk, field, rng.randrange(p)), elem(zk, field, rng.randrange(p)) if by4 else None
            got = check_fold(zk, tables[:k], coeffs, r0, r1, cs, (loglen, k))
            if k <= 16:                                       # the narrow hook: the same kernel instantiation
                narrow = zk.fri.ml_fold_batch(tables[:k], coeffs, r0, r1, cs)
                assert np.array_equal(got.evaluated_values, narrow.evaluated_values), (loglen, k)


@pytest.mark.parametrize("field", FIELDS)
def test_the_wide_fold_at_operands_random_tables_never_reach(zk, field):
    p, n = NM.MODULUS[field], 1 << 9
    rng = random.Random(397 + field)
    top, zeros, rnd = table_of(zk, field, [p - 1] * n), table_of(zk, field, [0] * n), zk.MultilinearPolynomial.random(field, n, 79)
    some = elem(zk, field, rng.randrange(p))
    for cs in (None, elem(zk, field, rng.randrange(2, p))):
        for r1 in (None, some):
            # the lazy sum's bound: 32 products of (p - 1)(p - 1) before the one reduction
            check_fold(zk, [top] * 32, zk.from_ints(field, [p - 1] * 32), some, r1, cs, "all p - 1")
            check_fold(zk, [top] * 32, zk.from_ints(field, [p - 1] * 32), elem(zk, field, p - 1), None if r1 is None else elem(zk, field, p - 1), cs, "all p - 1, r = p - 1")
            check_fold(zk, [zeros] * 17, zk.from_ints(field, [rng.randrange(p) for _ in range(17)]), some, r1, cs, "zeros")
            check_fold(zk, [rnd] * 16 + [top] + [rnd] * 3, zk.from_ints(field, [1, p - 1] * 8 + [0] + [rng.randrange(p) for _ in range(3)]), some, r1, cs, "f - f, a zero coefficient")


@pytest.mark.parametrize("by4", (False, True), ids=("fold2", "fold4"))
def test_the_wide_fold_on_the_second_trip_of_its_loop(zk, by4):
    """2^20 entries: 2^19 or 2^18 lanes against 768 blocks of 256"""
    field = 0
    p = NM.MODULUS[field]
    rng = random.Random(101 + by4)
    three = [zk.MultilinearPolynomial.random(field, 1 << 20, 7900 + j) for j in range(3)]
    tables = [three[j % 3] for j in range(17)]
    coeffs = zk.from_ints(field, [rng.randrange(p) for _ in range(17)])
    check_fold(zk, tables, coeffs, elem(zk, field, rng.randrange(p)), elem(zk, field, rng.randrange(p)) if by4 else None, elem(zk, field, rng.randrange(2, p)), "2^20")


# ---- the opening --------------------------------------------------------------------------------------------------------------------------
def assert_same_opening(got, fl):
    for name, arr in (("ys", got.ys), ("gamma", got.gamma), ("polys", got.round_polys), ("roots", got.roots), ("final", got.final_table),
                      ("challenges", got.challenges), ("indices", got.query_indices), ("values", got.query_values), ("paths", got.query_paths)):
        assert arr.shape == fl[name].shape and np.array_equal(arr, fl[name]), name


# d = 4 .. 8 under the three schedules; the field, the blow-up, the coset and log_final rotate
def grid():
    out = []
    for d in range(4, 9):
        for s, sched in enumerate(SCHEDULES):
            n = d + s
            out.append(pytest.param(FIELDS[n % 2], d, 1 + n % 2, (0, 1, d - 2)[n % 3], n % 4 < 2, sched, id="f%d-d%d-%s" % (FIELDS[n % 2], d, sched_id(sched))))
    return out


def open_case(zk, field, d, b, f, with_coset, sched, ks, g_bits=0):
    a, grouped = sched
    p = NM.MODULUS[field]
    pts = FC.points_for(field, d, 1, 107 * d + field)
    pm = to_mont(zk, field, pts[0]).reshape(1, d, 4)
    coset = coset_of(field, d, b, with_coset)
    cms = [FC.commitment(field, d, b, coset, 9500 + 19 * d + field + 101 * j, hasher(), grouped) for j in range(max(ks))]
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    try:
        for k in ks:
            tr = WB.pow_transcript(d, f, g_bits) if g_bits else None
            op = WB.open_batch(cms[:k], pts, f, Q, a, tr, hasher())
            fl = WB.flat(zk, op)
            got = zk.fri.open_multilinear_batch_wide(gcs[:k], pm, f, Q, log_arity=a, grinding_bits=g_bits)
            assert got.k == k and got.log_arity == a and got.grouped == grouped and got.pow_nonce == (tr.nonce if g_bits else 0)
            assert_same_opening(got, fl)
            roots = [gc.root for gc in gcs[:k]]
            assert roots == op["own_roots"] and zk.fri.verify_multilinear_batch_wide(roots, pm, got)
            assert not zk.fri.verify_multilinear_batch_wide(roots[1:] + roots[:1], pm, got)
            got.ys[k - 1, 0] = to_mont(zk, field, [(op["ys"][k - 1][0] + 1) % p])[0]
            assert not zk.fri.verify_multilinear_batch_wide(roots, pm, got)
            if k <= 16:
                narrow = zk.fri.open_multilinear_batch(gcs[:k], pm, f, Q, log_arity=a, grinding_bits=g_bits)
                assert_same_opening(narrow, fl)
    finally:
        for gc in gcs:
            gc.free()


@pytest.mark.parametrize("field,d,b,f,with_coset,sched", grid())
def test_the_wide_opening_equals_the_model(zk, field, d, b, f, with_coset, sched):
    open_case(zk, field, d, b, f, with_coset, sched, WIDE_KS + ((9,) if d == 4 else ()))


def test_the_wide_opening_with_proof_of_work(zk):
    open_case(zk, 3, 6, 2, 1, True, (2, True), (20,), g_bits=8)


def test_refusals_write_nothing(zk):
    from zkmle_amd import _lib as L
    lib = zk.lib()
    nq = 4
    mk = lambda field, d, b, coset, lg, seed: zk.fri.commit(zk.MultilinearPolynomial.random(field, 1 << d, seed), b, coset, log_group=lg)
    base = [mk(3, 4, 1, None, 0, 1 + j) for j in range(3)]
    others = {"d": mk(3, 5, 1, None, 0, 31), "blow-up": mk(3, 4, 2, None, 0, 32), "field": mk(0, 4, 1, None, 0, 33), "coset": mk(3, 4, 1, elem(zk, 3, 5), 0, 34),
              "grouping": mk(3, 4, 1, None, 2, 35)}
    FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
    w = lambda n: np.full(n, FILL, np.uint64)
    by = lambda n: np.full(n, 0xA5, np.uint8)
    ys, gamma, polys, roots, fin, chal, idx, vals, paths = w(4 * 33), w(4), w(12 * 4), by(32 * 40), w(4 << 4), w(4 * 4), w(nq), w(4 * nq * 80), by(32 * nq * 400)
    outs = (ys, gamma, polys, roots, fin, chal, idx, vals, paths)
    nonce = C.c_uint64(0xA5)
    pts = zk.from_ints(3, [3, 4, 5, 6]).reshape(1, 4, 4)
    t = zk.Transcript()
    t.append(b"untouched")
    before = t.export_state().copy()

    def raw(cms, k=None, wide=True):
        arr = (C.c_void_p * 33)(*[c._h for c in cms])
        fn = lib.zk_fri_ml_open_batch_wide_pow if wide else lib.zk_fri_ml_open_batch_pow
        return fn(arr, len(cms) if k is None else k, L.p64(pts), 1, 0, nq, 1, t._h, L.p64(ys), L.p64(gamma), L.p64(polys), L.p8(roots), L.p64(fin), L.p64(chal), L.p64(idx),
                  L.p64(vals), L.p8(paths), 0, C.byref(nonce))

    def refused(what, *a, **kw):
        assert raw(*a, **kw) == L.ZK_E_ARG, what
        assert all((o == (FILL if o.dtype == np.uint64 else 0xA5)).all() for o in outs) and nonce.value == 0xA5, what
        assert np.array_equal(t.export_state(), before), what

    try:
        twenty = [base[j % 3] for j in range(20)]
        refused("k = 33", [base[j % 3] for j in range(33)])
        refused("k = 0", twenty, k=0)
        refused("k = 17 by the narrow opener", twenty[:17], wide=False)
        for kind, other in others.items():
            for place in (0, 7, 19):
                cms = list(twenty)
                cms[place] = other
                refused((kind, place), cms)
        with pytest.raises(zk.ZkError):
            zk.fri.open_multilinear_batch_wide([base[j % 3] for j in range(33)], pts, 0, nq)
        # what was refused in one company is still good in another: the same commitment may stand in several places
        got = zk.fri.open_multilinear_batch_wide(twenty, pts, 0, nq)
        assert zk.fri.verify_multilinear_batch_wide([c.root for c in twenty], pts, got)
    finally:
        for c in base + list(others.values()):
            c.free()
