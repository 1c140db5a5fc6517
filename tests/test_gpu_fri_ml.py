"""GPU: the multilinear opening of a FRI commitment (csrc/fri_ml.cuh, csrc/zkmle_fri_ml.hip) over BLS12-381 Fr and BN254 Fr.  Everything
compares byte for byte with the library's own independent paths and with the Python model (tests/_fri_ml_model.py); no tolerance anywhere.

  fold       zk_fri_ml_fold = zk_uni_low_degree_extend(zk_mle_fold(T, last, r), b, c^2) for every codeword length 8 .. 2^15 (ntt_pow2t's
             switch from a table read to a product at 2^13 included), both fields, with and without a coset, r = 0, 1, p - 1 and random;
             r = 0 and r = 1 give the extensions of the even and the odd entries; lengths 2 .. 64 (2 and 4 have no table of two variables
             behind them) against the model's integers, whose layers tests/test_fri_ml_cpu.py ties to the same extension.  The
             operands uniform tables never reach (the second subtraction of the fold's last step, structured tables, cosets that are
             roots of unity), against the model's integers up to 2^14: tests/test_gpu_fri_ml_edges.py
  open       every output equals the model's at d = 1 .. 10, b = 1, 2, f = 0, 1, d - 1, Q = 8, and at d = 14, b = 2, f = 3 (several
             workgroups per reduction); y = zk_mle_evaluate; root_0 = the commitment's root; the host verifier accepts; the commitment's
             tables are unchanged
  sumcheck   prove_succinct / verify_succinct round-trip at d = 1, 5, 12; a tampered claimed sum is rejected

The issue asked for the succinct sumcheck's rounds to equal those of zk_sumcheck_basic_prove_on "started from a transcript that absorbed the
same root".  zk_sumcheck_basic_prove_on also absorbs the table's bytes (prover.rs:38-39) before the claimed sum, so its challenges cannot be
the succinct prover's, whose point is not to absorb the table.  What is compared instead, byte for byte, is the basic sumcheck of the model
on the transcript  root || claimed sum || rounds  -- the same round computation, with Python integers."""
import functools
import random

import numpy as np
import pytest

import _fri_ml_model as ML
import _fri_pcs_model as PM
import _ntt_model as NM
from oracle import pymodel as M
from test_gpu_fri import hasher_for, table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
FIELDS = (0, 3)


def elem(zk, field, v):
    return zk.from_ints(field, [v])[0]


def coset_of(field, d, b, with_coset):
    return random.Random(59 * d + b + field).randrange(2, NM.MODULUS[field]) if with_coset else 1


# ---- the fold --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_coset", (False, True))
@pytest.mark.parametrize("loglen", range(3, 16))
@pytest.mark.parametrize("field", FIELDS)
def test_fold_is_the_extension_of_the_mle_fold(zk, field, loglen, with_coset):
    p = NM.MODULUS[field]
    b = 1 if loglen % 2 else 2
    d = loglen - b
    c = coset_of(field, d, b, with_coset)
    cs, cs2 = (elem(zk, field, c), elem(zk, field, c * c % p)) if with_coset else (None, None)
    T = zk.MultilinearPolynomial.random(field, 1 << d, 900 + loglen + field)
    vals = T.evaluated_values
    cw = zk.ntt.low_degree_extend(T, b, cs)
    assert len(cw) == 1 << loglen
    for r in (0, 1, p - 1, random.Random(loglen * 7 + field).randrange(2, p - 1)):
        rm = elem(zk, field, r)
        got = zk.fri.ml_fold(cw, rm, cs).evaluated_values
        want = zk.ntt.low_degree_extend(zk.MultilinearPolynomial.partial_evaluate(T, d - 1, rm), b, cs2).evaluated_values
        assert got.shape == want.shape and np.array_equal(got, want), (loglen, r)
        if r in (0, 1):                                      # f_even and f_odd themselves
            half = zk.MultilinearPolynomial.vector(field, np.ascontiguousarray(vals[r::2]))
            assert np.array_equal(got, zk.ntt.low_degree_extend(half, b, cs2).evaluated_values), (loglen, r)


@pytest.mark.parametrize("field", FIELDS)
def test_fold_equals_the_models_integers(zk, field):
    """arbitrary tables (no codeword of low degree), lengths 2 .. 64: the formula itself, independent of the library's transform"""
    p = NM.MODULUS[field]
    for loglen in range(1, 7):
        table = NM.random_ints(field, 1 << loglen, 40 + loglen + field)
        for c in (1, coset_of(field, loglen, 3, True)):
            for r in (0, 1, p - 1, random.Random(loglen + field).randrange(2, p - 1)):
                got = zk.fri.ml_fold(table_of(zk, field, table), elem(zk, field, r), None if c == 1 else elem(zk, field, c)).evaluated_values
                assert np.array_equal(got, to_mont(zk, field, ML.fold(field, table, r, c))), (loglen, c == 1, r)


# ---- the opening -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_commitment(zk, field, d, b, with_coset):
    coset = coset_of(field, d, b, with_coset)
    return PM.commit(field, NM.random_ints(field, 1 << d, 8100 + 17 * d + b + field), b, coset, hasher_for(zk, 2 << (d + b)))


def gpu_commitment(zk, cm):
    cs = None if cm["coset"] == 1 else elem(zk, cm["field"], cm["coset"])
    return zk.fri.commit(table_of(zk, cm["field"], cm["coeffs"]), cm["b"], cs)


def assert_same_opening(zk, got, op):
    fl = ML.flat(zk, op)
    for name, arr in (("y", got.y), ("polys", got.round_polys), ("roots", got.roots), ("final", got.final_table), ("challenges", got.challenges),
                      ("indices", got.query_indices), ("values", got.query_values), ("paths", got.query_paths)):
        assert arr.shape == fl[name].shape and np.array_equal(arr, fl[name]), name


def check_opening(zk, field, d, b, f, with_coset, Q=8):
    p = NM.MODULUS[field]
    cm = model_commitment(zk, field, d, b, with_coset)
    rng = random.Random(d * 100 + b * 10 + f + field)
    z = [rng.randrange(p) for _ in range(d)]
    if d >= 3:
        z[1], z[d - 1] = rng.choice((0, 1)), p - 1
    op = ML.open_at(cm, z, f, Q, hasher=hasher_for(zk, 2 << (d + b)))
    zm = to_mont(zk, field, z)
    with gpu_commitment(zk, cm) as gc:
        assert gc.root == cm["root"]
        coeffs_before, codeword_before = table_of(zk, field, cm["coeffs"]).evaluated_values, gc.codeword().evaluated_values
        got = zk.fri.open_multilinear(gc, zm, f, Q)
        assert_same_opening(zk, got, op)
        assert np.array_equal(got.y, table_of(zk, field, cm["coeffs"]).evaluate(zm))
        assert got.roots[0].tobytes() == gc.root
        assert zk.fri.verify_multilinear(gc.root, zm, got)
        assert np.array_equal(gc.codeword().evaluated_values, codeword_before)
        again = zk.fri.open_multilinear(gc, zm, f, Q)        # the coefficient table was only read: the same proof comes out again
        assert_same_opening(zk, again, op)
        assert np.array_equal(coeffs_before, to_mont(zk, field, cm["coeffs"]))
        st = zk.fri.ml_last_stats()
        assert st["rounds"] == d - f and st["queries"] == Q
    bad = to_mont(zk, field, [(op["y"] + 1) % p])[0]
    got.y = bad
    assert not zk.fri.verify_multilinear(cm["root"], zm, got)


@pytest.mark.parametrize("b", (1, 2))
@pytest.mark.parametrize("d", range(1, 11))
def test_opening_equals_the_model(zk, d, b):
    """field and coset alternate with the shape, so that both fields meet every path: f = 0 (R = d), f = 1, f = d - 1 (R = 1)"""
    for f in sorted({0, min(1, d - 1), d - 1}):
        for field in FIELDS:
            check_opening(zk, field, d, b, f, with_coset=(d + b + f + field) % 2 == 1)


def test_opening_with_several_workgroups_per_reduction(zk):
    check_opening(zk, 3, 14, 2, 3, with_coset=True)


def test_opening_on_a_callers_transcript(zk):
    field, d, b, f, Q = 0, 5, 1, 1, 8
    cm = model_commitment(zk, field, d, b, True)
    z = NM.random_ints(field, d, 77)
    mt = M.Transcript()
    mt.append(b"before the opening")
    op = ML.open_at(cm, z, f, Q, mt, hasher=hasher_for(zk, 2 << (d + b)))
    t, v, want = zk.Transcript(), zk.Transcript(), zk.Transcript()
    t.append(b"before the opening")
    v.append(b"before the opening")
    want.append(bytes(mt.buf))
    with gpu_commitment(zk, cm) as gc:
        got = zk.fri.open_multilinear(gc, to_mont(zk, field, z), f, Q, transcript=t)
    assert_same_opening(zk, got, op)
    assert zk.fri.verify_multilinear(cm["root"], to_mont(zk, field, z), got, transcript=v)
    assert np.array_equal(t.export_state(), want.export_state()) and np.array_equal(v.export_state(), want.export_state())


def test_prover_codes_that_need_a_commitment(zk):
    from zkmle_amd import _lib as L
    field, d, b = 3, 4, 1
    p = NM.MODULUS[field]
    cm = model_commitment(zk, field, d, b, False)
    z = to_mont(zk, field, NM.random_ints(field, d, 5))
    with gpu_commitment(zk, cm) as gc:
        for f, Q in ((4, 8), (7, 8), (0, 0), (0, 4097)):
            with pytest.raises(L.ZkError) as e:
                zk.fri.open_multilinear(gc, z, f, Q)
            assert e.value.code == L.ZK_E_ARG, (f, Q)
        unreduced = z.copy()
        unreduced[2] = np.frombuffer((int.from_bytes(z[2].tobytes(), "little") + p).to_bytes(32, "little"), np.uint64)
        with pytest.raises(L.ZkError) as e:
            zk.fri.open_multilinear(gc, unreduced, 0, 8)
        assert e.value.code == L.ZK_E_ARG


# ---- the succinct basic sumcheck ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,d,b,f", [(0, 1, 1, 0), (3, 5, 2, 1), (0, 12, 1, 4)])
def test_succinct_sumcheck_round_trip(zk, field, d, b, f):
    p, Q = NM.MODULUS[field], 8
    cm = model_commitment(zk, field, d, b, d == 5)
    model = ML.sumcheck_prove(cm, f, Q, hasher=hasher_for(zk, 2 << (d + b)))
    with gpu_commitment(zk, cm) as gc:
        proof, challenges = zk.sumcheck.prove_succinct(gc, f, Q)
        codeword_after = gc.codeword().evaluated_values
    assert np.array_equal(codeword_after, to_mont(zk, field, cm["codeword"]))
    assert proof.root == cm["root"]
    assert np.array_equal(proof.initial_claimed_sum, to_mont(zk, field, [model["claimed_sum"]])[0])
    assert np.array_equal(proof.round_univariate_polynomials.reshape(-1, 4), to_mont(zk, field, [e for pair in model["rounds"] for e in pair]))
    assert np.array_equal(challenges, to_mont(zk, field, model["challenges"]))
    assert_same_opening(zk, proof.opening, model["opening"])
    assert zk.sumcheck.verify_succinct(proof)
    assert zk.sumcheck.verify_succinct(proof, root=cm["root"])
    assert not zk.sumcheck.verify_succinct(proof, root=bytes(32))
    proof.initial_claimed_sum = to_mont(zk, field, [(model["claimed_sum"] + 1) % p])[0]
    assert not zk.sumcheck.verify_succinct(proof)
