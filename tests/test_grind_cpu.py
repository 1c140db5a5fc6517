"""CPU: the host side of the proof-of-work step of the FRI transcripts (include/zkmle.h "Proof-of-work grinding").  Everything compares against
the model of tests/_grind_model.py, which is oracle/pymodel.py's Transcript and Keccak and nothing of the library's:

  search      zk_host_transcript_grind returns the model's nonce and leaves the model's state, for every fill 0 .. 135 of the sponge's open block
              at the moment the nonce is appended, on a fresh transcript and on one that has absorbed more than one block, with bits in
              {1, 7, 8, 9} and start in {0, 1, one above the first hit}; and at bits = 12 on the fills around the block's end
  check       zk_transcript_grind_check ends in the prover's state and gives 0 for w - 1, w + 1, one bit more, and another g in the tag
  statuses    the header's, all before any device call
  verifiers   zk_fri_verify_pow and zk_fri_ml_verify_batch_pow at g = 0 agree with the verifiers they extend on model proofs; at g > 0 they accept
              the extended models' proofs and reject a wrong nonce, the right nonce under another g, and answers to indices drawn without the step

The pure-Python Keccak costs about a millisecond a permutation, so the seeds of the search cases (SEEDS, found with the host search) are those
whose first two hits are small; the bits = 12 cases keep a first hit of two bytes.  The GPU search runs in tests/test_gpu_grind.py."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import __graft_entry__ as G
import _fri_ml_batch_model as BM
import _fri_ml_grouped_model as GM
import _fri_model as FM
import _fri_pcs_model as PM
import _grind_model as GR
import _ntt_model as NM
from oracle import pymodel as M

zk = G.import_package()
from zkmle_amd import _lib as L   # noqa: E402

P64, P8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
p64 = lambda a: a.ctypes.data_as(P64) if a is not None else None
p8 = lambda a: a.ctypes.data_as(P8) if a is not None else None
NEW_NAMES = ("zk_transcript_grind", "zk_host_transcript_grind", "zk_transcript_grind_check", "zk_transcript_grind_last_stats", "zk_fri_prove_pow",
             "zk_fri_verify_pow", "zk_fri_ml_open_batch_pow", "zk_fri_ml_verify_batch_pow")
RATE = 136
BITS_OF = (1, 7, 8, 9)                                       # of fill f: BITS_OF[f % 4]
# SEEDS[kind][fill]: the content seed of the case (kind 0: fresh, 1: more than one block absorbed); see the module's text
SEEDS = (
    (0, 8, 59, 628, 0, 111, 61, 1156, 0, 23, 323, 767, 0, 288, 284, 1193, 0, 175, 724, 1039, 0, 40, 467, 749, 0, 158, 9, 403, 0, 128, 755, 714, 0,
     33, 25, 1, 0, 13, 486, 543, 0, 63, 171, 1508, 0, 21, 273, 947, 0, 175, 192, 357, 0, 257, 65, 1860, 0, 30, 157, 231, 0, 30, 18, 1039, 0, 98,
     132, 36, 0, 33, 145, 513, 0, 69, 65, 306, 0, 34, 280, 421, 0, 71, 83, 29, 0, 25, 103, 572, 0, 84, 763, 349, 0, 32, 1630, 3727, 0, 62, 775, 575,
     0, 90, 667, 420, 0, 104, 271, 1020, 0, 193, 258, 297, 0, 58, 70, 718, 0, 150, 71, 431, 0, 75, 523, 2614, 0, 91, 211, 1799, 0, 22, 129, 657, 0,
     125, 17, 1052),
    (0, 30, 244, 93, 0, 37, 91, 101, 0, 1, 6, 1061, 0, 15, 4, 1343, 0, 16, 457, 302, 0, 54, 416, 306, 0, 94, 642, 145, 0, 115, 5, 3210, 0, 16, 284,
     857, 0, 19, 144, 2422, 0, 15, 413, 1588, 0, 96, 69, 1010, 0, 323, 65, 639, 0, 10, 13, 7240, 0, 29, 269, 550, 0, 3, 274, 3538, 0, 13, 217, 688,
     0, 27, 53, 1561, 0, 22, 11, 547, 0, 16, 411, 706, 0, 214, 282, 120, 0, 154, 779, 79, 0, 44, 17, 936, 0, 21, 1102, 601, 0, 77, 261, 1447, 0, 62,
     442, 721, 0, 125, 81, 569, 0, 48, 21, 1021, 0, 100, 234, 151, 0, 194, 216, 6, 0, 18, 2, 544, 0, 38, 693, 408, 0, 223, 7, 2775, 0, 24, 178, 803),
)
# (fill, seed) at bits = 12, fresh: first hits of two bytes, from 256 up to 767
SEEDS12 = ((0, 0), (64, 4), (127, 29), (128, 0), (129, 4), (135, 10))


def prior(kind, fill, seed):
    """what the transcript holds before the step, sized so that the open block holds `fill` bytes once the 8-byte tag is in"""
    n = (fill - 8) % RATE + (2 * RATE if kind else 0)
    return random.Random(1000 * seed + fill + 7 * kind).randbytes(n)


def lib_transcript(data):
    t = zk.Transcript()
    t.append(data)
    return t


def model_transcript(data):
    t = M.Transcript()
    t.append(data)
    return t


def same_state(t, mt):
    """the library transcript `t` is in the state of the model transcript `mt`"""
    return np.array_equal(t.export_state(), lib_transcript(bytes(mt.buf)).export_state())


def test_new_exports_are_present():
    lib = zk.lib()
    header = open(G.ROOT + "/include/zkmle.h").read()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in header, name
    assert "Proof-of-work grinding" in header and "#define ZK_FRI_GRIND_MAX_BITS 32" in header and "zk_grind_stats;" in header
    import inspect
    for fn in (zk.fri.prove, zk.fri.open_multilinear_batch, zk.fri.FriProof.__init__, zk.fri.FriMlBatchOpening.__init__):
        assert inspect.signature(fn).parameters["grinding_bits"].default == 0
    for name in ("grind", "grind_host", "check_grind"):
        assert callable(getattr(zk.Transcript, name)), name
    assert callable(zk.fri.grind_last_stats)
    pr = zk.fri.FriProof(0, 3, 1, 0, 2)
    assert (pr.grinding_bits, pr.pow_nonce) == (0, 0)


def test_the_seed_tables_cover_every_fill():
    assert len(SEEDS) == 2 and all(len(row) == RATE for row in SEEDS)
    assert {f for f, _ in SEEDS12} >= {0, 127, 128, 129, 135}
    for kind in (0, 1):
        for fill in range(RATE):
            t = lib_transcript(prior(kind, fill, SEEDS[kind][fill]) + GR.tag(9))
            assert int(t.export_state()[25]) == fill


@pytest.mark.parametrize("kind", (0, 1), ids=("fresh", "blocks"))
@pytest.mark.parametrize("part", range(8))
def test_the_host_search_returns_the_models_nonce(kind, part):
    for fill in range(part, RATE, 8):
        bits, data = BITS_OF[fill % 4], prior(kind, fill, SEEDS[kind][fill])
        first = None
        for start in (0, 1, None):                           # None: one above the first hit
            start = first + 1 if start is None else start
            mt, t = model_transcript(data), lib_transcript(data)
            want = GR.grind(mt, bits, start)
            assert t.grind_host(bits, start) == want, (kind, fill, bits, start)
            assert same_state(t, mt), (kind, fill, bits, start)
            assert want >= start and (first is None or want >= first)
            first = want if first is None else first


@pytest.mark.parametrize("fill,seed", SEEDS12)
def test_the_host_search_at_twelve_bits(fill, seed):
    data = prior(0, fill, seed)
    mt, t = model_transcript(data), lib_transcript(data)
    want = GR.grind(mt, 12)
    assert 256 <= want < 768
    assert t.grind_host(12) == want and same_state(t, mt)
    # the checker: the prover's state, and the model's verdicts around the nonce
    for w, bits in ((want, 12), (want - 1, 12), (want + 1, 12), (want, 13), (want, 11), (want, 8)):
        vm, v = model_transcript(data), lib_transcript(data)
        verdict = GR.check(vm, bits, w)
        assert v.check_grind(bits, w) == verdict, (w, bits)
        assert same_state(v, vm)
        if (w, bits) == (want, 12):
            assert verdict and np.array_equal(v.export_state(), t.export_state())
        elif w == want - 1:
            assert not verdict                              # the search returns the smallest


def next_bit_is_one(data, bits, w):
    """digest bit `bits` (the one after the zero bits) of the step's challenge"""
    mt = model_transcript(data + GR.tag(bits) + GR.be64(w))
    d = M.keccak256(mt.buf)
    return (d[bits // 8] >> (7 - bits % 8)) & 1 == 1


def test_the_check_rejects_neighbours_one_more_bit_and_another_tag():
    seen = {"plus": 0, "minus": 0, "bit": 0, "tag": 0}
    for kind in (0, 1):
        for fill in (0, 5, 64, 119, 120, 127, 128, 129, 131, 135):
            bits = 8
            data = prior(kind, fill, SEEDS[kind][fill] + 50000)
            t = lib_transcript(data)
            w = t.grind_host(bits)
            assert lib_transcript(data).check_grind(bits, w)
            if w > 0:
                assert not lib_transcript(data).check_grind(bits, w - 1)
                seen["minus"] += 1
            if not GR.check(model_transcript(data), bits, w + 1):
                assert not lib_transcript(data).check_grind(bits, w + 1)
                seen["plus"] += 1
            if next_bit_is_one(data, bits, w):               # the challenge has exactly `bits` zero bits: one bit more is asked of another digest
                mt, v = model_transcript(data), lib_transcript(data)
                verdict = GR.check(mt, bits + 1, w)
                assert v.check_grind(bits + 1, w) == verdict and same_state(v, mt)
                seen["bit"] += not verdict
            for other in (bits - 1, bits - 4, 1):            # fewer bits demanded, but the tag is another: the digest is another
                if not GR.check(model_transcript(data), other, w):
                    assert not lib_transcript(data).check_grind(other, w)
                    seen["tag"] += 1
    assert seen["minus"] >= 10 and seen["plus"] >= 15 and seen["bit"] >= 4 and seen["tag"] >= 10, seen


def test_a_search_that_runs_out_leaves_the_transcript_as_it_was():
    data = prior(0, 40, 4242)
    t = lib_transcript(data)
    w = t.grind_host(12)
    assert w > 4
    t2 = lib_transcript(data)
    nonce = C.c_uint64(77)
    assert zk.lib().zk_host_transcript_grind(t2._h, 12, 0, w, C.byref(nonce)) == L.ZK_E_RANGE     # candidates 0 .. w - 1
    assert nonce.value == 77 and np.array_equal(t2.export_state(), lib_transcript(data).export_state())
    assert zk.lib().zk_host_transcript_grind(t2._h, 12, 0, w + 1, C.byref(nonce)) == 0 and nonce.value == w
    assert np.array_equal(t2.export_state(), t.export_state())
    with pytest.raises(L.ZkError):
        lib_transcript(data).grind_host(12, 0, w)
    # 2^64 - 1 is no candidate
    assert zk.lib().zk_host_transcript_grind(lib_transcript(data)._h, 1, 2**64 - 1, 0, C.byref(nonce)) == L.ZK_E_RANGE


def test_statuses_without_a_device():
    lib = zk.lib()
    t = zk.Transcript()
    before = t.export_state().copy()
    nonce, ok = C.c_uint64(5), C.c_int(-1)
    for bits in (0, 33, 64, 2**32 - 1):
        assert lib.zk_transcript_grind(t._h, bits, 0, 0, C.byref(nonce)) == L.ZK_E_ARG
        assert lib.zk_host_transcript_grind(t._h, bits, 0, 0, C.byref(nonce)) == L.ZK_E_ARG
        assert lib.zk_transcript_grind_check(t._h, bits, 0, C.byref(ok)) == L.ZK_E_ARG
    for lb in (1, 7, 31, 64):
        assert lib.zk_transcript_grind(t._h, 8, 0, lb, C.byref(nonce)) == L.ZK_E_ARG
    assert lib.zk_transcript_grind(None, 8, 0, 0, C.byref(nonce)) == L.ZK_E_ARG and lib.zk_transcript_grind(t._h, 8, 0, 0, None) == L.ZK_E_ARG
    assert lib.zk_host_transcript_grind(None, 8, 0, 0, C.byref(nonce)) == L.ZK_E_ARG and lib.zk_host_transcript_grind(t._h, 8, 0, 0, None) == L.ZK_E_ARG
    assert lib.zk_transcript_grind_check(None, 8, 0, C.byref(ok)) == L.ZK_E_ARG and lib.zk_transcript_grind_check(t._h, 8, 0, None) == L.ZK_E_ARG
    assert lib.zk_transcript_grind_last_stats(None) == L.ZK_E_ARG
    import torch
    if not torch.cuda.is_available():
        for lb in (0, 8, 30):
            assert lib.zk_transcript_grind(t._h, 8, 0, lb, C.byref(nonce)) == L.ZK_E_NO_DEVICE
    assert (nonce.value, ok.value) == (5, -1) and np.array_equal(t.export_state(), before)

    # the _pow verifiers and provers: grinding_bits above 32 is ZK_E_ARG whatever else holds
    roots, fin, vals, paths = np.zeros(64 * 32, np.uint8), np.zeros(4 << 10, np.uint64), np.zeros(1 << 16, np.uint64), np.zeros(1 << 20, np.uint8)
    own, pts, ys, polys = np.zeros(17 * 32, np.uint8), np.zeros(8 * 64 * 4, np.uint64), np.zeros(16 * 8 * 4, np.uint64), np.zeros(64 * 12, np.uint64)
    for field in (0, 3):
        ver = lambda g: lib.zk_fri_verify_pow(field, 3, 1, 0, 4, None, None, p8(roots), p64(fin), p64(vals), p8(paths), g, 0, C.byref(ok))
        verb = lambda g: lib.zk_fri_ml_verify_batch_pow(field, p8(own), 2, 3, 1, 0, 4, 1, 0, None, p64(pts), 2, p64(ys), None, p64(polys), p8(roots), p64(fin),
                                                        p64(vals), p8(paths), g, 0, C.byref(ok))
        for v in (ver, verb):
            assert v(33) == L.ZK_E_ARG and v(2**32 - 1) == L.ZK_E_ARG and ok.value == -1
            for g in (0, 1, 32):
                assert v(g) == 0 and ok.value == 0                  # zeros are no proof
                ok.value = -1
    h = C.c_void_p()
    L.check(lib.zk_table_wrap(0, C.c_void_p(0x1000), 8, C.byref(h)))
    w = lambda n, ty=np.uint64: np.full(n, 7, ty)
    rt, fn, be, qi, vl, pa = w(64 * 32, np.uint8), w(64), w(64), w(8), w(1 << 10), w(1 << 14, np.uint8)
    prove = lambda g, n: lib.zk_fri_prove_pow(h, 1, 0, 4, None, None, p8(rt), p64(fn), p64(be), p64(qi), p64(vl), p8(pa), g, n)
    assert prove(33, C.byref(nonce)) == L.ZK_E_ARG and prove(8, None) == L.ZK_E_ARG and prove(2**31, C.byref(nonce)) == L.ZK_E_ARG
    if not torch.cuda.is_available():
        assert prove(8, C.byref(nonce)) == L.ZK_E_NO_DEVICE and prove(0, None) == L.ZK_E_NO_DEVICE
    nul = (C.c_void_p * 17)()
    opn = lambda cms, k, g, n: lib.zk_fri_ml_open_batch_pow(cms, k, p64(pts), 2, 0, 4, 1, None, p64(w(16 * 8 * 4)), None, p64(w(64 * 12)), p8(rt), p64(fn), None, None,
                                                            p64(vl), p8(pa), g, n)
    assert opn(nul, 2, 33, C.byref(nonce)) == L.ZK_E_ARG and opn(nul, 2, 8, None) == L.ZK_E_ARG and opn(nul, 2, 0, None) == L.ZK_E_ARG
    assert nonce.value == 5 and all((a == 7).all() for a in (rt, fn, be, qi, vl, pa))
    lib.zk_table_free(h)


# ---- the verifiers ------------------------------------------------------------------------------------------------------------------------
def fri_inputs(field, d, b, with_coset, seed=0):
    coeffs = NM.random_ints(field, 1 << d, 900 + 17 * d + field + seed)
    coset = random.Random(d * 8 + b + seed).randrange(2, NM.MODULUS[field]) if with_coset else 1
    return coeffs, coset


def fri_verify_pow(pr, fl, g, nonce, tr=None):
    ok = C.c_int(-1)
    cm = zk.from_ints(pr["field"], [pr["coset"]])[0]
    rc = zk.lib().zk_fri_verify_pow(pr["field"], pr["d"], pr["b"], pr["f"], pr["Q"], p64(cm), None if tr is None else tr._h, p8(fl["roots"]), p64(fl["final"]),
                                    p64(fl["values"]), p8(fl["paths"]), g, nonce, C.byref(ok))
    return rc, ok.value


def fri_verify_old(pr, fl):
    ok = C.c_int(-1)
    cm = zk.from_ints(pr["field"], [pr["coset"]])[0]
    rc = zk.lib().zk_fri_verify(pr["field"], pr["d"], pr["b"], pr["f"], pr["Q"], p64(cm), None, p8(fl["roots"]), p64(fl["final"]), p64(fl["values"]),
                                p8(fl["paths"]), C.byref(ok))
    return rc, ok.value


# (field, d, b, f, Q, coset given): cases of tests/test_fri_cpu.py GRID
FRI_CASES = [(0, 3, 2, 0, 5, True), (0, 4, 1, 3, 6, False), (3, 4, 3, 0, 6, True), (3, 5, 1, 1, 3, True)]
FRI_G = 7


@pytest.mark.parametrize("case", FRI_CASES)
def test_fri_verify_pow(case):
    field, d, b, f, Q, with_coset = case
    coeffs, coset = fri_inputs(field, d, b, with_coset)
    R = d - f
    plain = FM.prove(field, coeffs, b, f, Q, coset)
    pf = FM.flat(zk, plain)
    # g = 0: the verifier it extends, on a proof and on a damaged one
    assert fri_verify_pow(plain, pf, 0, 0) == fri_verify_old(plain, pf) == (0, 1)
    assert fri_verify_pow(plain, pf, 0, 12345) == (0, 1)        # no step, no nonce
    bad = dict(pf, final=pf["final"].copy())
    bad["final"][0, 0] ^= np.uint64(1)
    assert fri_verify_pow(plain, bad, 0, 0) == fri_verify_old(plain, bad) == (0, 0)
    # g > 0: the model with the step in front of its first index (its sample number R)
    mt = GR.PowTranscript(FRI_G, R)
    pr = FM.prove(field, coeffs, b, f, Q, coset, mt)
    w = mt.nonce
    vt = GR.PowTranscript(FRI_G, R, w)
    assert FM.verify(pr, vt) and vt.pow_ok and vt.buf == mt.buf
    fl = FM.flat(zk, pr)
    t = zk.Transcript()
    assert fri_verify_pow(pr, fl, FRI_G, w, t) == (0, 1)
    assert same_state(t, mt)
    assert pr["indices"] != plain["indices"]
    assert fri_verify_pow(pr, fl, FRI_G, w + 1) == (0, 0) and fri_verify_pow(pr, fl, FRI_G, w ^ (1 << 40)) == (0, 0)
    for g in (FRI_G - 1, FRI_G + 1, 0):                         # the right nonce under another g
        assert fri_verify_pow(pr, fl, g, w) == (0, 0), g
    assert fri_verify_old(pr, fl) == (0, 0)
    # answers to indices drawn without the step: the transcripts agree up to the step, so w is a nonce of the plain proof's transcript as well
    assert fri_verify_pow(plain, pf, FRI_G, w) == (0, 0)
    # the Python wrapper reads g and the nonce from the proof object
    proof = zk.FriProof(field, d, b, f, Q, coset=zk.from_ints(field, [coset])[0], grinding_bits=FRI_G)
    proof.roots, proof.final_coeffs, proof.query_values, proof.query_paths = fl["roots"], fl["final"], fl["values"], fl["paths"]
    proof.pow_nonce = w + 1
    assert not zk.fri.verify(proof)
    proof.pow_nonce = w
    assert zk.fri.verify(proof)
    proof.grinding_bits = 0
    assert not zk.fri.verify(proof)


@functools.lru_cache(maxsize=None)
def hasher():
    return GM.check_host_keccak(zk)


SCHEDULES = [(1, False), (2, False), (2, True)]              # (log_arity, grouped)
sched_id = lambda s: "a%d%s" % (s[0], "g" if s[1] else "")
BATCH_G, BATCH_Q = 5, 8


def batch_verify(op, fl, g, nonce, tr=None, old=False):
    ok = C.c_int(-1)
    cm = zk.from_ints(op["field"], [op["coset"]])[0]
    head = (op["field"], p8(fl["own_roots"]), op["k"], op["d"], op["b"], op["f"], op["Q"], op["a"], 2 if op["grouped"] else 0, p64(cm), p64(fl["points"]),
            len(op["points"]), p64(fl["ys"]), None if tr is None else tr._h, p64(fl["polys"]), p8(fl["roots"]), p64(fl["final"]), p64(fl["values"]), p8(fl["paths"]))
    if old:
        rc = zk.lib().zk_fri_ml_verify_batch(*head, C.byref(ok))
    else:
        rc = zk.lib().zk_fri_ml_verify_batch_pow(*head, g, nonce, C.byref(ok))
    return rc, ok.value


@pytest.mark.parametrize("k", (1, 3))
@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_fri_ml_verify_batch_pow(sched, k):
    a, grouped = sched
    field, d, b, f, P = (0, 4, 2, 0, 2) if k == 1 else (3, 4, 1, 1, 2)
    R = d - f
    p = NM.MODULUS[field]
    coset = random.Random(43 * d + b + field).randrange(2, p)
    cms = []
    for j in range(k):
        coeffs = NM.random_ints(field, 1 << d, 8100 + 13 * d + field + 101 * j)
        cms.append(GM.commit(field, coeffs, b, coset, hasher()) if grouped else PM.commit(field, coeffs, b, coset, hasher()))
    rng = random.Random(103 * d + 7 * P + field)
    pts = [[rng.randrange(p) for _ in range(d)] for _ in range(P)]
    plain = BM.open_batch(cms, pts, f, BATCH_Q, a, hasher=hasher())
    pf = BM.flat(zk, plain)
    assert batch_verify(plain, pf, 0, 0) == batch_verify(plain, pf, 0, 0, old=True) == (0, 1)
    bad = dict(pf, ys=pf["ys"].copy())
    bad["ys"][0, 0, 0] ^= np.uint64(1)
    assert batch_verify(plain, bad, 0, 0) == batch_verify(plain, bad, 0, 0, old=True) == (0, 0)
    # g > 0: the batch model with the step in front of its first index (its sample number 1 + R: gamma, then the R round challenges)
    mt = GR.PowTranscript(BATCH_G, 1 + R)
    op = BM.open_batch(cms, pts, f, BATCH_Q, a, mt, hasher=hasher())
    w = mt.nonce
    vt = GR.PowTranscript(BATCH_G, 1 + R, w)
    assert BM.verify(op, vt, hasher()) and vt.pow_ok and vt.buf == mt.buf
    fl = BM.flat(zk, op)
    t = zk.Transcript()
    assert batch_verify(op, fl, BATCH_G, w, t) == (0, 1)
    assert same_state(t, mt)
    assert op["indices"] != plain["indices"] and op["polys"] == plain["polys"] and op["roots"] == plain["roots"]
    assert batch_verify(op, fl, BATCH_G, w + 1) == (0, 0) and batch_verify(op, fl, BATCH_G, w ^ (1 << 63)) == (0, 0)
    for g in (BATCH_G - 1, BATCH_G + 1, 0):
        assert batch_verify(op, fl, g, w) == (0, 0), g
    assert batch_verify(op, fl, 0, 0, old=True) == (0, 0)
    assert batch_verify(plain, pf, BATCH_G, w) == (0, 0)        # indices drawn without the step, under a nonce that passes it
    # the Python wrapper
    o = zk.fri.FriMlBatchOpening(field, k, P, d, b, f, BATCH_Q, coset=zk.from_ints(field, [coset])[0], log_arity=a, grouped=grouped, grinding_bits=BATCH_G)
    o.ys, o.round_polys, o.roots, o.final_table, o.query_values, o.query_paths = fl["ys"], fl["polys"], fl["roots"], fl["final"], fl["values"], fl["paths"]
    o.pow_nonce = w
    assert zk.fri.verify_multilinear_batch(op["own_roots"], fl["points"], o)
    o.pow_nonce = w + 1
    assert not zk.fri.verify_multilinear_batch(op["own_roots"], fl["points"], o)
