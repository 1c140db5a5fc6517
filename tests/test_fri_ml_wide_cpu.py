"""CPU: the host side of the WIDE opening of several FRI commitments (include/zkmle.h "FRI commitments opened together, wide").  Everything
compares byte for byte against tests/_fri_ml_wide_model.py, the batch model run without its cap of 16:

  wide        zk_fri_ml_verify_batch_wide_pow accepts the model's openings at k = 17, 20 and 32 for d = 3 .. 5 under the three schedules, with
              and without the proof-of-work step; a nonce off by one is rejected
  narrow      at k = 1, 9 and 16 it accepts exactly what zk_fri_ml_verify_batch_pow accepts, rejects what that rejects, and ends in the same
              transcript state
  cap         k = 0 and k = 33 are ZK_E_ARG from every wide function; the narrow functions still refuse k = 17
  tampered    one flipped bit in a claim, a round value, a later root, a commitment's root, a layer-0 value, a layer-0 path or T_R at k = 20
  sizes       zk_fri_ml_sizes_batch_wide equals the model and, for k <= 16, the narrow function
  header      the block's text and the exports

Commitments cannot exist without a device: the fold kernel and the prover run in tests/test_gpu_fri_ml_wide.py."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import __graft_entry__ as G
import _fri_ml_cases as FC
import _fri_ml_wide_model as WB
from oracle import pymodel as M

zk = G.import_package()
P64, P8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
p64 = lambda a: a.ctypes.data_as(P64) if a is not None else None
p8 = lambda a: a.ctypes.data_as(P8) if a is not None else None
NEW_NAMES = ("zk_fri_ml_fold_batch_wide", "zk_fri_ml_sizes_batch_wide", "zk_fri_ml_open_batch_wide_pow", "zk_fri_ml_verify_batch_wide_pow")
SCHEDULES = [(1, False), (2, False), (2, True)]              # (log_arity, grouped)
# (field, d, b, f, coset): d = 3 .. 5 on both fields, R = 2 .. 5
CASES = [(0, 3, 1, 1, False), (3, 4, 2, 0, True), (0, 5, 1, 2, True), (3, 5, 1, 0, False)]
WIDE_KS, NARROW_KS = (17, 20, 32), (1, 9, 16)
Q, BITS = 4, 5
ARG = -7                                                     # ZK_E_ARG (checked against the package's in test_the_caps)
case_id = lambda c: "-".join(str(int(v)) for v in c)
sched_id = lambda s: "a%d%s" % (s[0], "g" if s[1] else "")

hasher = functools.partial(FC.hasher, zk, True)
tampered = FC.tampered
coset_of = functools.partial(FC.coset_of, mul=59)


@functools.lru_cache(maxsize=None)
def commitment(field, d, b, with_coset, grouped, j):
    return FC.commitment(field, d, b, coset_of(field, d, b, with_coset), 9300 + 17 * d + field + 101 * j, hasher(), grouped)


@functools.lru_cache(maxsize=None)
def opening(case, sched, k, bits=0, prefix=b""):
    """-> (the model's opening of k commitments at one point on a transcript that holds `prefix`, the nonce)"""
    field, d, b, f, with_coset = case
    cms = [commitment(field, d, b, with_coset, sched[1], j) for j in range(k)]
    tr = WB.pow_transcript(d, f, bits, prefix=prefix) if bits else M.Transcript()
    if prefix and not bits:
        tr.append(prefix)
    op = WB.open_batch(cms, FC.points_for(field, d, 1, 31 * d + field + k), f, Q, sched[0], tr, hasher())
    return op, (tr.nonce if bits else 0)


def lib_verify(op, fl=None, tr=None, g=0, nonce=0, wide=True, **over):
    """zk_fri_ml_verify_batch_wide_pow (or the narrow one) on the model's opening `op` (flat arrays `fl`) -> (status, ok)"""
    fl = WB.flat(zk, op) if fl is None else fl
    s = {n: op[n] for n in ("d", "b", "f", "Q", "k", "a")}
    s.update({n: v for n, v in over.items() if n in s})
    cm = zk.from_ints(op["field"], [op["coset"]])[0]
    ok = C.c_int(-1)
    fn = zk.lib().zk_fri_ml_verify_batch_wide_pow if wide else zk.lib().zk_fri_ml_verify_batch_pow
    rc = fn(op["field"], p8(fl["own_roots"]), s["k"], s["d"], s["b"], s["f"], s["Q"], s["a"], 2 if op["grouped"] else 0, p64(cm), p64(fl["points"]), len(op["points"]),
            p64(fl["ys"]), None if tr is None else tr._h, p64(fl["polys"]), p8(fl["roots"]), p64(fl["final"]), p64(fl["values"]), p8(fl["paths"]), g, nonce, C.byref(ok))
    return rc, ok.value


def test_new_exports_and_the_header():
    lib = zk.lib()
    header = open(G.ROOT + "/include/zkmle.h").read()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in header, name
    assert "FRI commitments opened together, wide" in header and "#define ZK_FRI_ML_WIDE_MAX 32" in header and "#define ZK_FRI_ML_BATCH_MAX 16" in header
    for name in ("open_multilinear_batch_wide", "verify_multilinear_batch_wide", "ml_fold_batch_wide", "ml_sizes_wide", "FriMlWideOpening"):
        assert hasattr(zk.fri, name), name


@pytest.mark.parametrize("k", WIDE_KS)
@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_wide_verifier_accepts_the_models_openings(case, sched, k):
    field, d, b, f, with_coset = case
    op, _ = opening(case, sched, k)
    assert WB.verify(op, hasher=hasher())
    fl = WB.flat(zk, op)
    assert lib_verify(op, fl) == (0, 1)
    assert lib_verify(op, fl, wide=False)[0] == ARG          # the narrow verifier keeps its cap
    assert lib_verify(op, fl, k=k - 1) == (0, 0)
    assert WB.sizes(k, d, b, f, Q, *sched) == (fl["roots"].shape[0], fl["final"].shape[0], fl["values"].size // 4, fl["paths"].size, fl["polys"].size // 4)
    assert zk.fri.ml_sizes_wide(d, b, f, Q, sched[0], sched[1], k=k) == WB.sizes(k, d, b, f, Q, *sched)
    # the Python wrapper
    cs = zk.from_ints(field, [op["coset"]])[0]
    o = zk.fri.FriMlWideOpening(field, k, 1, d, b, f, Q, coset=cs, log_arity=sched[0], grouped=sched[1])
    assert o.roots.shape == fl["roots"].shape and o.query_values.shape == fl["values"].shape and o.query_paths.shape == fl["paths"].shape
    o.ys, o.round_polys, o.roots, o.final_table, o.query_values, o.query_paths = fl["ys"], fl["polys"], fl["roots"], fl["final"], fl["values"], fl["paths"]
    assert zk.fri.verify_multilinear_batch_wide(op["own_roots"], fl["points"], o)
    assert not zk.fri.verify_multilinear_batch_wide(op["own_roots"][::-1], fl["points"], o)


@pytest.mark.parametrize("k", WIDE_KS)
@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_the_wide_verifier_with_the_proof_of_work_step(sched, k):
    for case in (CASES[1], CASES[2]):
        op, nonce = opening(case, sched, k, BITS)
        vt = WB.pow_transcript(case[1], case[3], BITS, nonce)
        assert WB.verify(op, vt, hasher()) and vt.pow_ok
        fl = WB.flat(zk, op)
        assert lib_verify(op, fl, g=BITS, nonce=nonce) == (0, 1)
        assert lib_verify(op, fl, g=BITS, nonce=nonce + 1) == (0, 0) and lib_verify(op, fl, g=BITS - 1, nonce=nonce) == (0, 0)
        assert lib_verify(op, fl) == (0, 0)                   # without the step the indices are others
        assert lib_verify(op, fl, g=33, nonce=nonce)[0] == ARG


@pytest.mark.parametrize("k", NARROW_KS)
@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_up_to_sixteen_the_wide_verifier_is_the_narrow_one(sched, k):
    prior = b"a caller's own"
    for case, bits in ((CASES[1], 0), (CASES[2], BITS)):
        op, nonce = opening(case, sched, k, bits, prior)
        base = WB.flat(zk, op)
        rng = random.Random(k + case[1])
        variants = [base, tampered(base, "ys", (k - 1, 0, 1), rng), tampered(base, "values", (1, 0, 2), rng), tampered(base, "roots", (k - 1, 5), rng),
                    tampered(base, "final", (0, 3), rng), tampered(base, "paths", (7,), rng)]
        for n, fl in enumerate(variants):
            tw, tn = zk.Transcript(), zk.Transcript()
            for t in (tw, tn):
                t.append(prior)
            want = (0, 1 if n == 0 else 0)
            assert lib_verify(op, fl, tw, g=bits, nonce=nonce) == want and lib_verify(op, fl, tn, g=bits, nonce=nonce, wide=False) == want, n
            assert np.array_equal(tw.export_state(), tn.export_state())
        assert lib_verify(op, base, g=bits, nonce=nonce) == lib_verify(op, base, g=bits, nonce=nonce, wide=False) == (0, 0)   # bound to the prior content


def test_the_caps():
    from zkmle_amd import _lib as L
    lib = zk.lib()
    assert L.ZK_E_ARG == ARG
    op, _ = opening(CASES[1], SCHEDULES[0], 17)
    fl = FC.padded(WB.flat(zk, op), room=1 << 16)
    for k in (0, 33, 1 << 31):
        assert lib_verify(op, fl, k=k)[0] == L.ZK_E_ARG and lib_verify(op, fl, k=k, wide=False)[0] == L.ZK_E_ARG
    assert lib_verify(op, fl, k=17, wide=False)[0] == L.ZK_E_ARG and lib_verify(op, fl, k=32)[0] == 0

    def sizes(fn, k):
        out = [C.c_size_t(0) for _ in range(5)]
        return fn(k, 6, 1, 0, 8, 1, 0, *[C.byref(o) for o in out]), tuple(int(o.value) for o in out)

    for k in range(1, 33):
        rc, got = sizes(lib.zk_fri_ml_sizes_batch_wide, k)
        assert rc == 0 and got == WB.sizes(k, 6, 1, 0, 8)
        assert sizes(lib.zk_fri_ml_sizes_batch, k) == ((0, got) if k <= 16 else (L.ZK_E_ARG, (0,) * 5))
    assert sizes(lib.zk_fri_ml_sizes_batch_wide, 0)[0] == L.ZK_E_ARG and sizes(lib.zk_fri_ml_sizes_batch_wide, 33)[0] == L.ZK_E_ARG
    with pytest.raises(zk.ZkError):
        zk.fri.ml_sizes(6, 1, 0, 8, k=17)
    # the hook and the prover, as far as they go without a device: the argument errors first, and nothing written
    h = C.c_void_p()
    L.check(lib.zk_table_wrap(0, C.c_void_p(0x1000), 4, C.byref(h)))
    one, out = zk.from_ints(0, [1] * 33), C.c_void_p()
    fold = lambda fn, k: fn((C.c_void_p * 33)(*([h] * 33)), k, p64(one), p64(one[0]), None, None, C.byref(out))
    assert fold(lib.zk_fri_ml_fold_batch_wide, 0) == L.ZK_E_ARG and fold(lib.zk_fri_ml_fold_batch_wide, 33) == L.ZK_E_ARG
    assert fold(lib.zk_fri_ml_fold_batch, 17) == L.ZK_E_ARG
    import torch
    if not torch.cuda.is_available():
        assert fold(lib.zk_fri_ml_fold_batch_wide, 17) == L.ZK_E_NO_DEVICE and fold(lib.zk_fri_ml_fold_batch_wide, 32) == L.ZK_E_NO_DEVICE
    assert not out.value
    w = lambda n: np.full(n, 7, np.uint64)
    pts, ys, gamma, pl, rt, fn_, vl, pa = w(64 * 4), w(33 * 4), w(4), w(64 * 12), np.full(96 * 32, 7, np.uint8), w(4 << 10), w(1 << 12), np.full(1 << 12, 7, np.uint8)
    nul = (C.c_void_p * 33)()
    nonce = C.c_uint64(7)
    opn = lambda k: lib.zk_fri_ml_open_batch_wide_pow(nul, k, p64(pts), 1, 0, 4, 1, None, p64(ys), p64(gamma), p64(pl), p8(rt), p64(fn_), None, None, p64(vl), p8(pa), 0,
                                                      C.byref(nonce))
    assert opn(0) == L.ZK_E_ARG and opn(33) == L.ZK_E_ARG and opn(20) == L.ZK_E_ARG
    assert all((a == 7).all() for a in (ys, gamma, pl, rt, fn_, vl, pa)) and nonce.value == 7
    lib.zk_table_free(h)


def spots_of(kind, op, base, rng):
    k, f, R = op["k"], op["f"], op["d"] - op["f"]
    L_ = op["d"] + op["b"]
    sides = WB.steps(L_, R, op["a"])[0][1]
    n = L_ - 2 if op["grouped"] else L_
    d0 = (1 if op["grouped"] else sides) * n
    per_q = base["paths"].size // Q
    if kind == "claim":
        return [("ys", (j, 0, rng.randrange(4))) for j in range(k)]
    if kind == "round":
        return [("polys", (l, i, rng.randrange(4))) for l in range(R) for i in range(3)]
    if kind == "later_root":
        return [("roots", (s, rng.randrange(32))) for s in range(k, len(op["roots"]))]
    if kind == "own_root":
        return [(name, (j, rng.randrange(32))) for j in range(k) for name in ("roots", "own_roots")]
    if kind == "layer0_value":
        return [("values", (1, j * sides + s, rng.randrange(4))) for j in range(k) for s in range(sides)]
    if kind == "layer0_path":
        return [("paths", (2 * per_q + 32 * (j * d0 + at) + rng.randrange(32),)) for j in range(k) for at in (0, d0 - 1)]
    assert kind == "final"
    return [("final", (j, rng.randrange(4))) for j in range(1 << f)]


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
@pytest.mark.parametrize("kind", ("claim", "round", "later_root", "own_root", "layer0_value", "layer0_path", "final"))
def test_a_tampered_opening_of_twenty_is_rejected(kind, sched):
    seen = 0
    for case in (CASES[1], CASES[2]):
        op, _ = opening(case, sched, 20)
        base = WB.flat(zk, op)
        rng = random.Random(411 + case[1] + len(kind))
        spots = spots_of(kind, op, base, rng)
        seen += len(spots)
        for name, at in spots:
            assert lib_verify(op, tampered(base, name, at, rng)) == (0, 0), (case, name, at)
    assert seen or kind == "later_root"
