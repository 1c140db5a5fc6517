"""CPU: the host verifier of the opening against a weight table (include/zkmle.h "FRI commitment opened against a weight table") on the
openings of the integer model tests/_fri_ml_weighted_model.py, d = 4, both fields, the three schedules (log_arity 1; 2; 2 on grouped leaves).

  accepts     zk_fri_ml_verify_weighted and zk.fri.verify_weighted accept the model's openings, as the model's own verifier does; with 8 bits of
              proof of work too; a caller's transcript ends in the model's state
  rejects     ok = 0 with status ZK_OK after one flipped bit in c, the round polynomials, a later root, the final table, w_final, the query
              values and the paths; with another root in the verifier's hands; with the nonce off by one; with a false claim c that the prover
              made round 0 sum to; and -- the case the comparison of the challenges exists for -- with one carried challenge changed and a
              w_final folded by the changed challenges, which is consistent with everything the verifier is handed
  sizes       zk_fri_ml_sizes_weighted equals the model's counts and the lengths of the model's opening
  statuses    a NULL, an arity out of range, grouped leaves at log_arity 1: ZK_E_ARG

The prover runs in tests/test_gpu_fri_ml_weighted.py."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import __graft_entry__ as G
import _fri_ml_cases as FC
import _fri_ml_weighted_model as WM
import _grind_model as GR
import _ntt_model as NM
from oracle import pymodel as M

zk = G.import_package()
P64, P8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
FIELDS = (0, 3)
SCHEDULES = [(1, False), (2, False), (2, True)]
sched_id = lambda s: "a%d%s" % (s[0], "g" if s[1] else "")
D, B, F, Q = 4, 1, 1, 5
hasher = functools.partial(FC.hasher, zk, True)


@functools.lru_cache(maxsize=None)
def opening(field, sched, bits=0, false_c=None, prior=b""):
    a, grouped = sched
    cm = FC.commitment(field, D, B, FC.coset_of(field, D, B, field == 3, 53), 6100 + field, hasher(), grouped)
    W0 = NM.random_ints(field, 1 << D, 6200 + field)
    tr = M.Transcript()
    if prior:
        tr.append(prior)
    op = WM.open_weighted(cm, W0, F, Q, a, tr, hasher(), (lambda t: GR.grind(t, bits)) if bits else None, false_c)
    op["W0"], op["bits"], op["end"] = W0, bits, tr.sample()
    return op


def lib_verify(op, prior=b"", **over):
    """zk_fri_ml_verify_weighted on the model's opening with some of its flat parts replaced -> (status, ok, the transcript's next sample)"""
    fl = WM.flat(zk, op)
    fl.update(over)
    field = op["field"]
    arr8 = lambda b: np.frombuffer(bytes(b), np.uint8).copy()
    root, roots, paths = arr8(fl["root"]), arr8(fl["roots"]), arr8(fl["paths"])
    coset = None if op["coset"] == 1 else zk.from_ints(field, [op["coset"]])
    t = zk.Transcript()
    if prior:
        t.append(prior)
    ok = C.c_int(-1)
    p64 = lambda x: np.ascontiguousarray(x, np.uint64).ctypes.data_as(P64)
    keep = [np.ascontiguousarray(fl[n], np.uint64) for n in ("c", "challenges", "w_final", "polys", "final", "values")]
    rc = zk.lib().zk_fri_ml_verify_weighted(field, root.ctypes.data_as(P8), op["d"], op["b"], op["f"], op["Q"], op["a"], 2 if op["grouped"] else 0,
                                            None if coset is None else p64(coset), keep[0].ctypes.data_as(P64), keep[1].ctypes.data_as(P64),
                                            keep[2].ctypes.data_as(P64), t._h, keep[3].ctypes.data_as(P64), roots.ctypes.data_as(P8),
                                            keep[4].ctypes.data_as(P64), keep[5].ctypes.data_as(P64), paths.ctypes.data_as(P8), op["bits"],
                                            fl.get("nonce", op["nonce"]), C.byref(ok))
    return rc, ok.value, t.sample_random_challenge()


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
@pytest.mark.parametrize("field", FIELDS)
def test_the_models_opening_is_accepted(field, sched):
    for bits, prior in ((0, b""), (8, b""), (0, b"bound before the opening")):
        op = opening(field, sched, bits, None, prior)
        p = NM.MODULUS[field]
        assert op["c"] == sum(t * w for t, w in zip(FC.commitment(field, D, B, op["coset"], 6100 + field, hasher(), sched[1])["coeffs"], op["W0"])) % p
        assert op["w_final"] == WM.fold_weights(field, op["W0"], op["challenges"])
        tr = M.Transcript()
        if prior:
            tr.append(prior)
        assert WM.verify_weighted(op, tr, hasher(), (lambda t, w: GR.check(t, bits, w)) if bits else None)
        rc, ok, end = lib_verify(op, prior)
        assert (rc, ok) == (0, 1) and end == op["end"] == tr.sample(), (bits, prior)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
@pytest.mark.parametrize("field", FIELDS)
def test_one_changed_bit_anywhere_is_rejected(field, sched):
    op = opening(field, sched, 8)
    rng = random.Random(6300 + field)
    base = WM.flat(zk, op)
    for name in ("c", "polys", "final", "w_final", "values"):
        arr = np.ascontiguousarray(base[name], np.uint64).copy().reshape(-1)
        for at in {0, arr.size - 4, rng.randrange(arr.size)}:
            bad = arr.copy()
            bad[at] ^= np.uint64(1 << rng.randrange(64))
            assert lib_verify(op, **{name: bad})[:2] == (0, 0), (name, at)
    for name in ("roots", "paths", "root"):
        raw = bytearray(base[name])
        for at in {len(raw) - 1, rng.randrange(len(raw))} | ({40} if name == "roots" and len(raw) > 40 else set()):
            bad = bytearray(raw)
            bad[at] ^= 1 << rng.randrange(8)
            assert lib_verify(op, **{name: bytes(bad)})[:2] == (0, 0), (name, at)
    assert lib_verify(op, nonce=op["nonce"] + 1)[:2] == (0, 0)
    assert lib_verify(op)[:2] == (0, 1)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
@pytest.mark.parametrize("field", FIELDS)
def test_a_changed_challenge_with_a_consistent_w_final_is_rejected(field, sched):
    p = NM.MODULUS[field]
    op = opening(field, sched)
    for l in range(D - F):
        ch = list(op["challenges"])
        ch[l] = (ch[l] + 1) % p
        wf = WM.fold_weights(field, op["W0"], ch)             # what a verifier computes from the proof's own copy of the challenges
        assert wf != op["w_final"]
        assert lib_verify(op, challenges=zk.from_ints(field, ch), w_final=zk.from_ints(field, wf))[:2] == (0, 0), l
        assert not WM.verify_weighted(dict(op, challenges=ch, w_final=wf), None, hasher())
    # and a false claim, with round 0 shifted to sum to it, fails the chain's end
    bad = opening(field, sched, 0, (op["c"] + 1) % p)
    assert bad["c"] != op["c"] and lib_verify(bad)[:2] == (0, 0) and not WM.verify_weighted(bad, None, hasher())


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_sizes_equal_the_model(sched):
    a, grouped = sched
    out = [C.c_size_t(0) for _ in range(5)]
    assert zk.lib().zk_fri_ml_sizes_weighted(D, B, F, Q, a, 2 if grouped else 0, *[C.byref(o) for o in out]) == 0
    got = tuple(int(o.value) for o in out)
    assert got == WM.sizes(D, B, F, Q, a, grouped) == zk.fri.ml_sizes_weighted(D, B, F, Q, a, grouped)
    op = opening(0, sched)
    fl = WM.flat(zk, op)
    assert got == (len(op["roots"]), len(op["final"]), fl["values"].shape[0] * fl["values"].shape[1], len(fl["paths"]), 3 * len(op["polys"]))


def test_statuses():
    L = zk.lib()
    out = [C.c_size_t(0) for _ in range(5)]
    refs = [C.byref(o) for o in out]
    assert L.zk_fri_ml_sizes_weighted(D, B, F, Q, 3, 0, *refs) == -7
    assert L.zk_fri_ml_sizes_weighted(D, B, F, Q, 1, 2, *refs) == -7          # grouped leaves need log_arity 2
    assert L.zk_fri_ml_sizes_weighted(D, B, D - 1, Q, 2, 0, *refs) == -7      # one round cannot fold by 4
    args = [None] * 14
    assert L.zk_fri_ml_open_weighted(None, None, F, Q, 1, 0, *args[:10]) == -7
    op = opening(0, SCHEDULES[0])
    assert lib_verify(dict(op, a=3))[0] == -7
    assert lib_verify(dict(op, grouped=True))[0] == -7
