"""GPU: the Spartan prover (csrc/zkmle_r1cs.hip zk_r1cs_prove; include/zkmle.h "R1CS satisfiability: Spartan over a FRI commitment") over
BLS12-381 Fr and BN254 Fr, every output byte for byte against the prover of tests/_r1cs_model.py.

  prove     s = 9, d = 10 for the three schedules (log_arity 1; 2; 2 on grouped leaves) and s = 12, d = 13 once per field, with l = 0 and l = 5
            public values, with and without bytes a caller's transcript absorbed before, once with 8 bits of proof of work: tau, the round
            polynomials, the challenges, va vb vc, rho and the whole opening equal the model's; zk.r1cs.verify accepts and ends in the
            prover's transcript state; another public value is rejected
  false     the proof of an instance one row of which the witness violates is made (ZK_OK) and rejected
  refusals  a witness commitment of another size or field, l = 2^(d-1), grouped leaves at log_arity 1: ZK_E_ARG, and the transcript has not moved"""
import numpy as np
import pytest

import _fri_ml_cases as FC
import _grind_model as GR
import _ntt_model as NM
import _r1cs_model as RM
from oracle import pymodel as M
from test_gpu_fri import to_mont, zk  # noqa: F401  (zk: the module's fixture)
from test_gpu_fri_ml_weighted import assert_same_opening

pytestmark = pytest.mark.gpu
FIELDS = (0, 3)
SCHEDULES = [(1, False), (2, False), (2, True)]
sched_id = lambda s: "a%d%s" % (s[0], "g" if s[1] else "")
Q = 5


def instance(zk, field, s, d, mats):
    return zk.R1CS(field, s, d, *(([e[0] for e in m], [e[1] for e in m], zk.from_ints(field, [e[2] for e in m])) for m in mats))


def prove_both(zk, field, s, d, npub, sched, f, bits=0, prior=b"", violate=None):
    a, grouped = sched
    hasher = FC.hasher(zk, grouped)
    mats, w, public = RM.satisfied_instance(field, s, d, npub, 17000 + 31 * s + npub + field, violate)
    cm = (FC.GM if grouped else FC.PM).commit(field, w, 1, FC.coset_of(field, d, 1, npub == 0, 73), hasher)
    mt, lt, vt = M.Transcript(), zk.Transcript(), zk.Transcript()
    if prior:
        for t in (mt, lt, vt):
            t.append(prior)
    pr = RM.prove(field, s, d, mats, cm, public, f, Q, a, mt, hasher, (lambda t: GR.grind(t, bits)) if bits else None)
    inst = instance(zk, field, s, d, mats)
    pub = zk.from_ints(field, public)
    with FC.gpu_commitment(zk, cm) as gcm:
        got = zk.r1cs.prove(inst, gcm, pub, f, Q, log_arity=a, transcript=lt, grinding_bits=bits)
    return got, pr, (inst, cm, pub, public, mats), (mt.sample(), lt.sample_random_challenge(), vt)


def assert_same_proof(zk, got, pr):
    fl = RM.flat(zk, pr)
    for name, a in (("tau", got.tau), ("polys", got.round_polys), ("challenges", got.challenges), ("vs", got.vs), ("rho", got.rho)):
        assert a.shape == fl[name].shape and np.array_equal(a, fl[name]), name
    assert_same_opening(zk, got.opening, pr["opening"])


@pytest.mark.parametrize("npub", (0, 5))
@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
@pytest.mark.parametrize("field", FIELDS)
def test_proof_equals_the_model(zk, field, sched, npub):
    bits = 8 if (sched, npub) == (SCHEDULES[2], 5) else 0
    prior = b"absorbed before the proof" if npub else b""
    got, pr, (inst, cm, pub, public, mats), (mend, lend, vt) = prove_both(zk, field, 9, 10, npub, sched, (0, 3, 1)[SCHEDULES.index(sched)], bits, prior)
    assert RM.is_satisfied(field, 9, 10, mats, cm["coeffs"], public)
    assert_same_proof(zk, got, pr)
    assert mend == lend
    assert zk.r1cs.verify(inst, cm["root"], pub, got, vt) and vt.sample_random_challenge() == mend
    if npub:
        other = pub.copy()
        other[2] = zk.from_ints(field, [7])[0]
        assert not zk.r1cs.verify(inst, cm["root"], other, got)
    st = zk.r1cs.last_stats()
    assert st["ms_total"] > 0 and st["ms_rounds"] > 0 and st["ms_opening"] > 0


@pytest.mark.parametrize("field", FIELDS)
def test_proof_at_s_12_d_13(zk, field):
    got, pr, (inst, cm, pub, _, _), (mend, lend, _) = prove_both(zk, field, 12, 13, 5 * (field == 3), SCHEDULES[1 + (field == 0)], 2)
    assert_same_proof(zk, got, pr)
    assert mend == lend and zk.r1cs.verify(inst, cm["root"], pub, got)


@pytest.mark.parametrize("field", FIELDS)
def test_a_violated_row_is_proved_and_rejected(zk, field):
    got, pr, (inst, cm, pub, public, mats), _ = prove_both(zk, field, 9, 10, 5, SCHEDULES[1], 1, violate=77)
    assert not RM.is_satisfied(field, 9, 10, mats, cm["coeffs"], public)
    assert_same_proof(zk, got, pr)
    assert not zk.r1cs.verify(inst, cm["root"], pub, got)


def test_refusals_before_the_transcript_moves(zk):
    field, s, d = 0, 4, 5
    mats, w, public = RM.satisfied_instance(field, s, d, 2, 17100)
    inst = instance(zk, field, s, d, mats)
    fresh = zk.Transcript().sample_random_challenge()
    small = FC.PM.commit(field, w[:8], 1, 1, FC.hasher(zk))
    right = FC.PM.commit(field, w, 1, 1, FC.hasher(zk))
    other = FC.PM.commit(3, [v % NM.MODULUS[3] for v in w], 1, 1, FC.hasher(zk))
    grouped = FC.GM.commit(field, w, 1, 1, FC.hasher(zk, True))
    with FC.gpu_commitment(zk, small) as gs, FC.gpu_commitment(zk, right) as gr, FC.gpu_commitment(zk, other) as go, FC.gpu_commitment(zk, grouped) as gg:
        for cmh, pub, f in ((gs, public, 1), (go, public, 1), (gr, [1] * 16, 1), (gr, public, 4)):
            t = zk.Transcript()
            with pytest.raises(zk.ZkError) as e:
                zk.r1cs.prove(inst, cmh, zk.from_ints(field, pub), f, Q, transcript=t)
            assert e.value.code == -7 and t.sample_random_challenge() == fresh
        with pytest.raises(ValueError):
            zk.r1cs.prove(inst, gg, zk.from_ints(field, public), 1, Q, log_arity=1)
        assert zk.r1cs.verify(inst, right["root"], zk.from_ints(field, public), zk.r1cs.prove(inst, gr, zk.from_ints(field, public), 1, Q))
