"""CPU: the host verifier of the Spartan proof (include/zkmle.h "R1CS satisfiability: Spartan over a FRI commitment") on the proofs of the integer
model tests/_r1cs_model.py: a satisfied instance at s = 4, d = 5, l = 2, log_final = 1, both fields, log_arity 1 and 2 (and 2 on grouped leaves).

  accepts      zk_r1cs_verify accepts the model's proof, as the model's verifier does; a caller's transcript ends in the model's state
  rejects      ok = 0 with status ZK_OK after one changed bit in each proof component (round polynomials, va vb vc, c, the opening's round
               polynomials, roots, final table, values, paths), one changed public value, one changed matrix value (a second handle), one
               carried opening challenge (the verifier computes w_final from the carried ones, so it is consistent with the change), and for
               the proof of an instance that one row does not satisfy
  public terms zk_r1cs_public_terms equals the model's c_pub and w_final, for every number of opening challenges
  sizes        zk_r1cs_sizes equals the lengths of the model's proof
  statuses     a NULL, l out of range, a bad arity: ZK_E_ARG, and a caller's transcript is as it was
  fixture      tests/golden/r1cs_proof.bin, what tools/r1cs_selftest.hip reads (a stand-alone host program for a sanitizer build; its header has
               the commands), is the model's proof and verifies

The prover runs in tests/test_gpu_r1cs_prove.py."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import __graft_entry__ as G
import _fri_ml_cases as FC
import _ntt_model as NM
import _r1cs_model as RM
from oracle import pymodel as M

zk = G.import_package()
P64, P8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
FIELDS = (0, 3)
SCHEDULES = [(1, False), (2, False), (2, True)]
sched_id = lambda s: "a%d%s" % (s[0], "g" if s[1] else "")
S, D, NPUB, B, F, Q = 4, 5, 2, 1, 1, 4
hasher = functools.partial(FC.hasher, zk, True)


def instance(field, mats):
    return zk.R1CS(field, S, D, *(([e[0] for e in m], [e[1] for e in m], zk.from_ints(field, [e[2] for e in m])) for m in mats))


@functools.lru_cache(maxsize=None)
def case(field, sched, violate=None, prior=b""):
    a, grouped = sched
    mats, w, public = RM.satisfied_instance(field, S, D, NPUB, 7100 + field, violate)
    cm = (FC.GM if grouped else FC.PM).commit(field, w, B, FC.coset_of(field, D - 1, B, field == 3, 71), hasher())
    tr = M.Transcript()
    if prior:
        tr.append(prior)
    pr = RM.prove(field, S, D, mats, cm, public, F, Q, a, tr, hasher())
    return mats, public, cm, pr, tr.sample()


def lib_verify(field, mats, public, cm, pr, prior=b"", over=None, inst=None):
    """zk_r1cs_verify on the model's proof with some flat parts replaced -> (status, ok, the transcript's next sample)"""
    fl = RM.flat(zk, pr)
    op = dict(fl.pop("opening"))
    fl = {"polys": fl["polys"], "vs": fl["vs"], "public": zk.from_ints(field, public), "open_polys": op.pop("polys"), **op}   # the opening's challenges, not the rounds'
    fl.update(over or {})
    arr8 = lambda b: np.frombuffer(bytes(b), np.uint8).copy()
    root, roots, paths = arr8(fl["root"]), arr8(fl["roots"]), arr8(fl["paths"])
    keep = {n: np.ascontiguousarray(fl[n], np.uint64) for n in ("public", "polys", "vs", "c", "open_polys", "final", "challenges", "values")}
    p64 = lambda n: keep[n].ctypes.data_as(P64)
    o = pr["opening"]
    coset = None if o["coset"] == 1 else zk.from_ints(field, [o["coset"]])
    t = zk.Transcript()
    if prior:
        t.append(prior)
    ok = C.c_int(-1)
    inst = inst or instance(field, mats)
    rc = zk.lib().zk_r1cs_verify(inst._h, root.ctypes.data_as(P8), p64("public"), len(public), o["b"], o["f"], o["Q"], fl.get("a", o["a"]), 2 if o["grouped"] else 0,
                                 None if coset is None else coset.ctypes.data_as(P64), t._h, p64("polys"), p64("vs"), p64("c"), p64("open_polys"),
                                 roots.ctypes.data_as(P8), p64("final"), p64("challenges"), p64("values"), paths.ctypes.data_as(P8), 0, 0, C.byref(ok))
    return rc, ok.value, t.sample_random_challenge()


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
@pytest.mark.parametrize("field", FIELDS)
def test_the_models_proof_is_accepted(field, sched):
    for prior in (b"", b"absorbed before the proof"):
        mats, public, cm, pr, end = case(field, sched, None, prior)
        assert RM.is_satisfied(field, S, D, mats, cm["coeffs"], public)
        tr = M.Transcript()
        if prior:
            tr.append(prior)
        assert RM.verify(pr, mats, cm["root"], public, tr, hasher()) and tr.sample() == end
        assert lib_verify(field, mats, public, cm, pr, prior) == (0, 1, end)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
@pytest.mark.parametrize("field", FIELDS)
def test_single_changes_are_rejected(field, sched):
    p = NM.MODULUS[field]
    mats, public, cm, pr, _ = case(field, sched)
    rng = random.Random(7200 + field)
    inst = instance(field, mats)
    fl = RM.flat(zk, pr)
    parts = {"polys": fl["polys"], "vs": fl["vs"], "c": fl["opening"]["c"], "open_polys": fl["opening"]["polys"], "final": fl["opening"]["final"],
             "values": fl["opening"]["values"]}
    for name, arr in parts.items():
        flatarr = np.ascontiguousarray(arr, np.uint64).copy().reshape(-1)
        for at in {0, flatarr.size - 4, rng.randrange(flatarr.size)}:
            bad = flatarr.copy()
            bad[at] ^= np.uint64(1 << rng.randrange(64))
            assert lib_verify(field, mats, public, cm, pr, over={name: bad}, inst=inst)[:2] == (0, 0), (name, at)
    for name in ("roots", "paths", "root"):
        raw = bytearray(fl["opening"][name])
        at = rng.randrange(len(raw))
        raw[at] ^= 1 << rng.randrange(8)
        assert lib_verify(field, mats, public, cm, pr, over={name: bytes(raw)}, inst=inst)[:2] == (0, 0), (name, at)
    # one public value
    other = [public[0], (public[1] + 1) % p]
    assert lib_verify(field, mats, other, cm, pr, inst=inst)[:2] == (0, 0) and not RM.verify(pr, mats, cm["root"], other, None, hasher())
    # one matrix value, through a second handle
    r, c, v = mats[1][3]
    changed = [mats[0], mats[1][:3] + [(r, c, (v + 1) % p)] + mats[1][4:], mats[2]]
    assert lib_verify(field, changed, public, cm, pr)[:2] == (0, 0) and not RM.verify(pr, changed, cm["root"], public, None, hasher())
    # one carried opening challenge: the verifier folds its weights by the carried challenges, so w_final agrees with the change
    for l in range(len(pr["opening"]["challenges"])):
        ch = list(pr["opening"]["challenges"])
        ch[l] = (ch[l] + 1) % p
        assert lib_verify(field, mats, public, cm, pr, over={"challenges": zk.from_ints(field, ch)}, inst=inst)[:2] == (0, 0), l
        assert not RM.verify(dict(pr, opening=dict(pr["opening"], challenges=ch)), mats, cm["root"], public, None, hasher())
    assert lib_verify(field, mats, public, cm, pr, inst=inst)[:2] == (0, 1)


@pytest.mark.parametrize("field", FIELDS)
def test_an_instance_unsatisfied_in_one_row_is_rejected(field):
    mats, public, cm, pr, _ = case(field, SCHEDULES[0], violate=5)
    z = list(cm["coeffs"]) + RM.xvec(field, D, public)
    a, b, c = RM.matvec(field, S, mats, z)
    assert sum(1 for x, y, v in zip(a, b, c) if x * y % NM.MODULUS[field] != v) == 1
    assert lib_verify(field, mats, public, cm, pr)[:2] == (0, 0) and not RM.verify(pr, mats, cm["root"], public, None, hasher())


@pytest.mark.parametrize("field", FIELDS)
def test_public_terms_equal_the_model(field):
    p = NM.MODULUS[field]
    mats, public, cm, pr, _ = case(field, SCHEDULES[0])
    inst = instance(field, mats)
    rng = random.Random(7300 + field)
    for R in range(D):
        rx, rho, rs = [rng.randrange(p) for _ in range(S)], rng.choice((0, p - 1, rng.randrange(p))), [rng.randrange(p) for _ in range(R)]
        for pub in (public, [], [p - 1] * 5):
            c_pub, wf = zk.r1cs.public_terms(inst, zk.from_ints(field, pub), zk.from_ints(field, rx), zk.from_ints(field, [rho])[0], zk.from_ints(field, rs))
            want_c, want_w = RM.public_terms(field, S, D, mats, pub, rx, rho, rs)
            assert zk.to_ints(field, c_pub.reshape(1, -1)) == [want_c] and zk.to_ints(field, wf) == want_w, (R, len(pub))


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_sizes_equal_the_proofs_lengths(sched):
    _, _, _, pr, _ = case(0, sched)
    fl = RM.flat(zk, pr)
    op = fl["opening"]
    got = zk.r1cs.sizes(S, D, B, F, Q, sched[0], sched[1])
    assert got == (fl["polys"].size // 4, len(pr["opening"]["roots"]), op["final"].shape[0], op["values"].shape[0] * op["values"].shape[1], len(op["paths"]),
                   op["polys"].size // 4)
    assert got[0] == 4 * S


def test_statuses_leave_the_transcript_alone():
    mats, public, cm, pr, _ = case(0, SCHEDULES[0])
    fresh = zk.Transcript().sample_random_challenge()
    rc, _, after = lib_verify(0, mats, public, cm, pr, over={"a": 3})
    assert rc == -7 and after == fresh
    L = zk.lib()
    inst = instance(0, mats)
    assert L.zk_r1cs_verify(inst._h, *([None] * 2), 0, B, F, Q, 1, 0, None, None, *([None] * 9), 0, 0, None) == -7
    assert L.zk_r1cs_verify(None, *([None] * 2), 0, B, F, Q, 1, 0, None, None, *([None] * 9), 0, 0, None) == -7
    assert L.zk_r1cs_prove(None, None, None, 0, F, Q, 1, 0, None, *([None] * 14)) == -7
    out = [C.c_size_t(0) for _ in range(6)]
    assert L.zk_r1cs_sizes(0, D, B, F, Q, 1, 0, *[C.byref(o) for o in out]) == -7
    assert L.zk_r1cs_sizes(S, D, B, D - 1, Q, 1, 0, *[C.byref(o) for o in out]) == -7        # log_final is counted on the witness: d - 1 variables


def test_the_selftest_fixture_is_the_models_proof():
    """tests/golden/r1cs_proof.bin, what tools/r1cs_selftest.hip reads, is the model's proof with its instance, and verifies"""
    import importlib.util
    import os
    path = os.path.join(G.ROOT, "tests", "golden", "make_r1cs_fixture.py")
    spec = importlib.util.spec_from_file_location("make_r1cs_fixture", path)
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    with open(mk.OUT, "rb") as fh:
        stored = fh.read()
    assert stored == mk.fixture_bytes(zk) and len(stored) < 16 << 10
    mats, public, cm, pr = mk.model_case(zk)
    assert RM.verify(pr, mats, cm["root"], public, None, mk.hasher(zk))
    assert lib_verify(mk.FIELD, mats, public, cm, pr)[:2] == (0, 1)
