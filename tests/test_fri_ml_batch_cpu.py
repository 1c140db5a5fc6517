"""CPU: the host side of the multilinear opening of several FRI commitments with one proof (include/zkmle.h "FRI commitments opened
together").  Everything compares byte for byte against the big-integer model of tests/_fri_ml_batch_model.py:

  opening     zk_fri_ml_verify_batch accepts the model's openings on both fields, on the cases of tests/test_fri_ml_grouped_cpu.py with d in
              {3, 4, 6} (R = 2 .. 6), with k in {1, 2, 5} under each of the three schedules (log_arity 1; 2; 2 with grouped leaves), and rejects
              one change of each class: a claim, a round value, a later root, one commitment's root, one commitment's layer-0 value, one
              commitment's path, T_R, k, the order of two commitments, and an opening of the single-table protocol offered as k = 1
  sizes       zk_fri_ml_sizes_batch equals the model's sizes, and the single-table sizes plus (k - 1) times step 0's share
  statuses    every ZK_E_ARG of the header comes before any device call and writes nothing
  transcript  a caller's transcript ends in the model's state on ZK_OK

Commitments cannot exist without a device: the fold kernel and the prover run in tests/test_gpu_fri_ml_batch.py."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import __graft_entry__ as G
import _fri_ml_arity_model as AM
import _fri_ml_batch_model as BM
import _fri_ml_cases as FC
import _fri_ml_grouped_model as GM
import _fri_ml_model as ML
import _fri_ml_points_model as PT
import _ntt_model as NM

zk = G.import_package()
P64, P8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
p64 = lambda a: a.ctypes.data_as(P64) if a is not None else None
p8 = lambda a: a.ctypes.data_as(P8) if a is not None else None
NEW_NAMES = ("zk_fri_ml_fold_batch", "zk_fri_ml_sizes_batch", "zk_fri_ml_open_batch", "zk_fri_ml_verify_batch")
# (field, d, b, f, P, coset): the cases of tests/test_fri_ml_grouped_cpu.py CASES with d in {3, 4, 6}: R = 2, 3, 2, 4, 3, 5, 6
CASES = [(0, 3, 1, 1, 1, False), (3, 3, 2, 0, 2, True), (3, 4, 1, 2, 8, False), (0, 4, 2, 0, 2, True), (0, 6, 2, 3, 8, True), (3, 6, 1, 1, 1, True),
         (0, 6, 1, 0, 2, False)]
SCHEDULES = [(1, False), (2, False), (2, True)]              # (log_arity, grouped)
KS = (1, 2, 5)
Q = 8
case_id = lambda c: "-".join(str(int(v)) for v in c)
sched_id = lambda s: "a%d%s" % (s[0], "g" if s[1] else "")


hasher = functools.partial(FC.hasher, zk, True)
tampered = FC.tampered
padded = functools.partial(FC.padded, room=8192)
coset_of = functools.partial(FC.coset_of, mul=43)


@functools.lru_cache(maxsize=None)
def commitment(field, d, b, with_coset, grouped, j):
    return FC.commitment(field, d, b, coset_of(field, d, b, with_coset), 8100 + 13 * d + field + 101 * j, hasher(), grouped)


def points_for(field, d, P):
    return FC.points_for(field, d, P, 103 * d + 7 * P + field)


@functools.lru_cache(maxsize=None)
def opening(case, sched, k):
    field, d, b, f, P, with_coset = case
    a, grouped = sched
    cms = [commitment(field, d, b, with_coset, grouped, j) for j in range(k)]
    return BM.open_batch(cms, points_for(field, d, P), f, Q, a, hasher=hasher())


def lib_verify(op, fl=None, tr=None, **over):
    """zk_fri_ml_verify_batch on the model's opening `op` (flat arrays `fl`) -> (status, ok)"""
    fl = BM.flat(zk, op) if fl is None else fl
    s = {n: op[n] for n in ("d", "b", "f", "Q", "k", "a")}
    s["lg"] = 2 if op["grouped"] else 0
    s.update({n: v for n, v in over.items() if n in s})
    coset = over.get("coset", op["coset"])
    cm = None if coset is None else zk.from_ints(op["field"], [coset])[0]
    ok = C.c_int(-1)
    rc = zk.lib().zk_fri_ml_verify_batch(op["field"], p8(fl["own_roots"]), s["k"], s["d"], s["b"], s["f"], s["Q"], s["a"], s["lg"], p64(cm), p64(fl["points"]),
                                         len(op["points"]), p64(fl["ys"]), None if tr is None else tr._h, p64(fl["polys"]), p8(fl["roots"]),
                                         p64(fl["final"]), p64(fl["values"]), p8(fl["paths"]), C.byref(ok))
    return rc, ok.value


def test_new_exports_are_present():
    lib = zk.lib()
    header = open(G.ROOT + "/include/zkmle.h").read()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in header, name
    assert "FRI commitments opened together" in header and "#define ZK_FRI_ML_BATCH_MAX 16" in header
    import inspect
    assert "k" in inspect.signature(zk.fri.ml_sizes).parameters
    for name in ("open_multilinear_batch", "verify_multilinear_batch", "ml_fold_batch", "FriMlBatchOpening"):
        assert hasattr(zk.fri, name), name


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_model_openings_pass_the_model_verifier_and_the_library_verifier(case, sched, k):
    field, d, b, f, P, with_coset = case
    a, grouped = sched
    op = opening(case, sched, k)
    for j in range(k):
        assert op["ys"][j] == [ML.mle_evaluate(field, commitment(field, d, b, with_coset, grouped, j)["coeffs"], z) for z in op["points"]]
    assert BM.verify(op, hasher=hasher())
    fl = BM.flat(zk, op)
    assert lib_verify(op, fl) == (0, 1)
    if not with_coset:
        assert lib_verify(op, fl, coset=None) == (0, 1)
    assert BM.sizes(k, d, b, f, Q, a, grouped) == (fl["roots"].shape[0], fl["final"].shape[0], fl["values"].size // 4, fl["paths"].size, fl["polys"].size // 4)
    # the Python wrapper
    cs = zk.from_ints(field, [op["coset"]])[0]
    o = zk.fri.FriMlBatchOpening(field, k, P, d, b, f, Q, coset=cs, log_arity=a, grouped=grouped)
    assert o.roots.shape == fl["roots"].shape and o.query_values.shape == fl["values"].shape and o.query_paths.shape == fl["paths"].shape
    assert o.ys.shape == fl["ys"].shape
    o.ys, o.round_polys, o.roots, o.final_table, o.query_values, o.query_paths = fl["ys"], fl["polys"], fl["roots"], fl["final"], fl["values"], fl["paths"]
    assert zk.fri.verify_multilinear_batch(op["own_roots"], fl["points"], o)
    assert not zk.fri.verify_multilinear_batch([r[::-1] for r in op["own_roots"]], fl["points"], o)


# R = 4 (steps alone), R = 5 (a final fold-2 step behind fold-4 steps), R = 2 (at arity 2 step 0 is the only step)
TAMPER = [(CASES[3], 2), (CASES[5], 5), (CASES[2], 2)]


def step0_share(op):
    """(values, digests) of one commitment's part of step 0, and the path length"""
    L = op["d"] + op["b"]
    _, sides = BM.steps(L, op["d"] - op["f"], op["a"])[0]
    n = L - 2 if op["grouped"] else L
    return sides, (1 if op["grouped"] else sides) * n, n


def spots_of(kind, op, base, rng):
    k, f, R = op["k"], op["f"], op["d"] - op["f"]
    v0, d0, n = step0_share(op)
    per_q = base["paths"].size // Q
    if kind == "claim":                                       # every y_{j,p}
        return [("ys", (j, q, rng.randrange(4))) for j in range(k) for q in range(len(op["points"]))]
    if kind == "round":
        return [("polys", (l, i, rng.randrange(4))) for l in range(R) for i in range(3)]
    if kind == "later_root":                                  # in the proof's list, behind the k commitments'
        return [("roots", (s, rng.randrange(32))) for s in range(k, len(op["roots"]))]
    if kind == "own_root":                                    # commitment j's root: the proof's copy, and the verifier's
        return [(name, (j, rng.randrange(32))) for j in range(k) for name in ("roots", "own_roots")]
    if kind == "layer0_value":                                # every side of every commitment's step-0 values, at query 1
        return [("values", (1, j * v0 + s, rng.randrange(4))) for j in range(k) for s in range(v0)]
    if kind == "layer0_path":                                 # the first and the last digest of every commitment's first and last path, at query 2
        out = []
        for j in range(k):
            for start in (0, d0 - n):
                off = 2 * per_q + 32 * (j * d0 + start)
                out += [("paths", (off + rng.randrange(32),)), ("paths", (off + 32 * (n - 1) + rng.randrange(32),))]
        return out
    assert kind == "final"
    return [("final", (j, rng.randrange(4))) for j in range(1 << f)]


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
@pytest.mark.parametrize("kind", ("claim", "round", "later_root", "own_root", "layer0_value", "layer0_path", "final"))
def test_a_tampered_opening_is_rejected(kind, sched):
    seen = 0
    for case, k in TAMPER:
        op = opening(case, sched, k)
        base = BM.flat(zk, op)
        rng = random.Random(917 + case[1] + case[0] + len(kind) + k)
        spots = spots_of(kind, op, base, rng)
        seen += len(spots)
        for name, at in spots:
            assert lib_verify(op, tampered(base, name, at, rng)) == (0, 0), (case, k, name, at)
    assert seen
    if kind == "layer0_value":                                # the same residue, not reduced: x + p < 2^256
        p = NM.MODULUS[op["field"]]
        for at in ((3, 0), (0, base["values"].shape[1] - 1), (2, step0_share(op)[0])):
            fl = {n: v.copy() for n, v in base.items()}
            fl["values"][at] = np.frombuffer((int.from_bytes(fl["values"][at].tobytes(), "little") + p).to_bytes(32, "little"), np.uint64)
            assert lib_verify(op, fl) == (0, 0), at


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_another_k_or_another_order_is_rejected(sched):
    for case, k in ((CASES[3], 2), (CASES[5], 5)):
        op = opening(case, sched, k)
        base = BM.flat(zk, op)
        big = padded(base)
        assert lib_verify(op, big) == (0, 1)
        assert lib_verify(op, big, k=k - 1) == (0, 0) and lib_verify(op, big, k=k + 1) == (0, 0)
        # the verifier holds the roots in another order
        sw = {n: v.copy() for n, v in base.items()}
        sw["own_roots"][[0, 1]] = sw["own_roots"][[1, 0]]
        assert lib_verify(op, sw) == (0, 0)
        sw["roots"][[0, 1]] = sw["roots"][[1, 0]]             # ... and the proof's copy with them
        assert lib_verify(op, sw) == (0, 0)
        # ... and the claims and the step-0 answers too: every path now leads to its root, but gamma and alpha^j belong to the other order
        v0, d0, _ = step0_share(op)
        sw["ys"][[0, 1]] = sw["ys"][[1, 0]]
        vals = sw["values"].copy()
        vals[:, :v0], vals[:, v0:2 * v0] = sw["values"][:, v0:2 * v0], sw["values"][:, :v0]
        sw["values"] = vals
        pq = sw["paths"].reshape(Q, -1).copy()
        pq[:, :32 * d0], pq[:, 32 * d0:64 * d0] = sw["paths"].reshape(Q, -1)[:, 32 * d0:64 * d0], sw["paths"].reshape(Q, -1)[:, :32 * d0]
        sw["paths"] = pq.reshape(-1)
        assert lib_verify(op, sw) == (0, 0)
        # the model's own verifier agrees
        other = dict(op, own_roots=op["own_roots"][1::-1] + op["own_roots"][2:])
        assert not BM.verify(other, hasher=hasher())


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[5]], ids=case_id)
def test_a_single_table_opening_is_no_batch_of_one_and_the_reverse(case):
    """at k = 1 the layouts are those of the single-table protocol of the same schedule; the transcripts are not"""
    field, d, b, f, P, with_coset = case
    pts = points_for(field, d, P)
    cs = zk.from_ints(field, [coset_of(field, d, b, with_coset)])[0]
    for sched, single_model in zip(SCHEDULES, (PT, AM, GM)):
        a, grouped = sched
        cm = commitment(field, d, b, with_coset, grouped, 0)
        single = single_model.open_points(cm, pts, f, Q, hasher=hasher())
        assert single_model.verify(single, hasher=hasher())
        sf = single_model.flat(zk, single)
        batch = opening(case, sched, 1)
        bf = BM.flat(zk, batch)
        assert single["ys"] == batch["ys"][0] and sf["roots"].shape == bf["roots"].shape and sf["paths"].shape == bf["paths"].shape
        assert sf["values"].size == bf["values"].size
        # the single-table opening offered as k = 1
        as_batch = dict(bf, ys=sf["ys"].reshape(1, P, 4), polys=sf["polys"], roots=sf["roots"], final=sf["final"], values=sf["values"], paths=sf["paths"])
        assert lib_verify(batch, as_batch) == (0, 0)
        # the batch of one offered to the single-table verifier
        o = zk.fri.FriMlPointsOpening(field, P, d, b, f, Q, coset=cs, log_arity=a, grouped=grouped)
        o.ys, o.round_polys, o.roots, o.final_table, o.query_values, o.query_paths = sf["ys"], sf["polys"], sf["roots"], sf["final"], sf["values"], sf["paths"]
        assert zk.fri.verify_multilinear_points(cm["root"], sf["points"], o)
        o.ys, o.round_polys, o.roots, o.final_table = bf["ys"][0], bf["polys"], bf["roots"], bf["final"]
        o.query_values, o.query_paths = bf["values"].reshape(o.query_values.shape), bf["paths"]
        assert not zk.fri.verify_multilinear_points(cm["root"], bf["points"], o)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_a_callers_transcript_ends_in_the_models_state(sched):
    from oracle import pymodel as M
    a, grouped = sched
    prior = b"what the caller had absorbed before"
    cms = [commitment(3, 4, 1, True, grouped, j) for j in range(3)]
    mt = M.Transcript()
    mt.append(prior)
    op = BM.open_batch(cms, points_for(3, 4, 2), 1, Q, a, mt, hasher=hasher())
    vt = M.Transcript()
    vt.append(prior)
    assert BM.verify(op, vt, hasher()) and vt.buf == mt.buf
    t = zk.Transcript()
    t.append(prior)
    assert lib_verify(op, tr=t) == (0, 1)
    want = zk.Transcript()
    want.append(bytes(mt.buf))
    assert np.array_equal(t.export_state(), want.export_state())
    assert lib_verify(op) == (0, 0)                           # the opening is bound to the prior content


def test_sizes():
    from zkmle_amd import _lib as L
    lib = zk.lib()

    def sizes(k, d, b, f, q, a, lg):
        out = [C.c_size_t(0) for _ in range(5)]
        rc = lib.zk_fri_ml_sizes_batch(k, d, b, f, q, a, lg, *[C.byref(o) for o in out])
        return rc, tuple(int(o.value) for o in out)

    for d in (3, 4, 6, 10, 24):
        for b in (1, 2):
            for f in range(0, d):
                for q in (1, 8, 64):
                    for a, grouped in SCHEDULES:
                        L_, R = d + b, d - f
                        if a == 2 and R < 2:
                            assert sizes(2, d, b, f, q, a, 2 * grouped)[0] == L.ZK_E_ARG
                            continue
                        single = zk.fri.ml_sizes(d, b, f, q, log_arity=a, grouped=grouped)
                        sides0 = 2 if a == 1 else 4
                        path0 = (L_ - 2) if grouped else sides0 * L_
                        for k in (1, 2, 5, 16):
                            want = (k + single[0] - 1, single[1], single[2] + (k - 1) * q * sides0, single[3] + (k - 1) * q * 32 * path0, single[4])
                            assert sizes(k, d, b, f, q, a, 2 * grouped) == (0, want), (k, d, b, f, q, a, grouped)
                            assert BM.sizes(k, d, b, f, q, a, grouped) == want
                            assert zk.fri.ml_sizes(d, b, f, q, log_arity=a, grouped=grouped, k=k) == want
    # k = 4 at (24, 2, 6): the paths of one proof against four
    for a, grouped in SCHEDULES:
        one, four = zk.fri.ml_sizes(24, 2, 6, 64, a, grouped)[3], zk.fri.ml_sizes(24, 2, 6, 64, a, grouped, k=4)[3]
        assert one < four < 4 * one
    for k, a, lg in ((0, 1, 0), (17, 1, 0), (2, 0, 0), (2, 3, 0), (2, 1, 2), (2, 2, 1), (2, 2, 3), (1 << 31, 2, 2)):
        assert sizes(k, 6, 1, 0, 8, a, lg)[0] == L.ZK_E_ARG, (k, a, lg)
    assert sizes(2, 4, 1, 4, 8, 1, 0)[0] == L.ZK_E_ARG and sizes(2, 4, 0, 0, 8, 1, 0)[0] == L.ZK_E_ARG and sizes(2, 4, 1, 0, 0, 1, 0)[0] == L.ZK_E_ARG
    assert sizes(2, 40, 1, 0, 8, 1, 0)[0] == L.ZK_E_RANGE
    assert lib.zk_fri_ml_sizes_batch(2, 4, 1, 0, 8, 2, 2, None, None, None, None, None) == 0
    with pytest.raises(ValueError):
        zk.fri.ml_sizes(4, 1, 0, 8, log_arity=1, grouped=True, k=2)


def test_statuses_without_a_device():
    from zkmle_amd import _lib as L
    lib = zk.lib()
    roots, fin, vals, paths = np.zeros(64 * 32, np.uint8), np.zeros(4 << 10, np.uint64), np.zeros(1 << 16, np.uint64), np.zeros(1 << 20, np.uint8)
    own, pts, ys, polys = np.zeros(17 * 32, np.uint8), np.zeros(8 * 64 * 4, np.uint64), np.zeros(16 * 8 * 4, np.uint64), np.zeros(64 * 12, np.uint64)
    ok = C.c_int(-1)
    for field in (0, 1, 2, 3):
        ver = lambda d, b, f, q, k=2, a=1, lg=0, P=2, okp=C.byref(ok), o=own: lib.zk_fri_ml_verify_batch(
            field, p8(o), k, d, b, f, q, a, lg, None, p64(pts), P, p64(ys), None, p64(polys), p8(roots), p64(fin), p64(vals), p8(paths), okp)
        for kw in (dict(k=0), dict(k=17), dict(a=0), dict(a=3), dict(lg=1), dict(lg=3), dict(lg=2), dict(P=0), dict(P=9), dict(okp=None), dict(o=None)):
            assert ver(3, 1, 0, 4, **kw) == L.ZK_E_ARG, kw
        assert ver(3, 1, 2, 4, a=2) == L.ZK_E_ARG and ver(3, 1, 2, 4, a=2, lg=2) == L.ZK_E_ARG   # R = 1
        for d, b, f, q in ((3, 0, 0, 4), (3, 9, 0, 4), (3, 1, 0, 0), (3, 1, 0, 4097), (3, 1, 3, 4), (0, 1, 0, 4), (40, 1, 40, 4)):
            assert ver(d, b, f, q) == L.ZK_E_ARG, (d, b, f, q)
        if field in (1, 2):
            assert ver(3, 1, 0, 4) == L.ZK_E_RANGE
        else:
            assert ver(NM.two_adicity(field), 1, 0, 4) == L.ZK_E_RANGE and ver(40, 1, 0, 4) == L.ZK_E_RANGE
            assert ok.value == -1
            for a, lg in ((1, 0), (2, 0), (2, 2)):
                assert ver(3, 1, 0, 4, a=a, lg=lg) == 0 and ok.value == 0               # zeros are no proof
                ok.value = -1
    # the prover and the fold, as far as they go without a device: every argument error first, and nothing written
    h = {}
    for field, n in ((0, 1), (0, 2), (0, 4), (0, 8), (0, 6), (1, 8), (3, 4)):
        h[field, n] = C.c_void_p()
        L.check(lib.zk_table_wrap(field, C.c_void_p(0x1000), n, C.byref(h[field, n])))
    out = C.c_void_p()
    one = zk.from_ints(0, [1] * 17)
    zero = np.zeros(4, np.uint64)

    def fold(tabs, k=None, coeffs=one, r0=one[0], r1=one[0], coset=None, o=C.byref(out)):
        hs = None if tabs is None else (C.c_void_p * max(len(tabs), 1))(*tabs)
        return lib.zk_fri_ml_fold_batch(hs, len(tabs) if k is None else k, p64(coeffs), p64(r0), p64(r1), p64(coset), o)

    t4, t8 = h[0, 4], h[0, 8]
    assert fold(None, k=2) == L.ZK_E_ARG and fold([t4, t4], k=0) == L.ZK_E_ARG and fold([t4] * 17) == L.ZK_E_ARG
    assert fold([t4, None]) == L.ZK_E_ARG and fold([None, t4]) == L.ZK_E_ARG
    assert fold([t4, h[3, 4]]) == L.ZK_E_ARG and fold([t4, t8]) == L.ZK_E_LEN_MISMATCH and fold([t8, t4, t8]) == L.ZK_E_LEN_MISMATCH
    assert fold([t4, t4], coeffs=None) == L.ZK_E_ARG and fold([t4, t4], r0=None) == L.ZK_E_ARG and fold([t4, t4], o=None) == L.ZK_E_ARG
    assert fold([t4, t4], coset=zero) == L.ZK_E_ARG
    assert fold([h[0, 1]]) == L.ZK_E_ARG and fold([h[0, 2], h[0, 2]]) == L.ZK_E_ARG and fold([h[0, 1]], r1=None) == L.ZK_E_ARG   # too short for the fold
    assert fold([h[0, 6], h[0, 6]]) == L.ZK_E_NOT_POW2 and fold([h[1, 8]]) == L.ZK_E_RANGE
    import torch
    if not torch.cuda.is_available():
        assert fold([t4, t4]) == L.ZK_E_NO_DEVICE and fold([h[0, 2], h[0, 2]], r1=None) == L.ZK_E_NO_DEVICE and fold([t4] * 16) == L.ZK_E_NO_DEVICE
    assert not out.value
    w = lambda n: np.full(n, 7, np.uint64)
    ysb, gamma, pl, rt, fn, vl, pa = w(16 * 8 * 4), w(4), w(64 * 12), np.full(64 * 32, 7, np.uint8), w(4 << 10), w(1 << 12), np.full(1 << 12, 7, np.uint8)
    opn = lambda cms, k, o_ys=ysb: lib.zk_fri_ml_open_batch(cms, k, p64(pts), 2, 0, 4, 1, None, p64(o_ys), p64(gamma), p64(pl), p8(rt), p64(fn), None, None, p64(vl), p8(pa))
    nul = (C.c_void_p * 17)()
    assert opn(None, 2) == L.ZK_E_ARG and opn(nul, 0) == L.ZK_E_ARG and opn(nul, 17) == L.ZK_E_ARG and opn(nul, 2) == L.ZK_E_ARG
    assert opn(nul, 2, None) == L.ZK_E_ARG
    assert all((a == 7).all() for a in (ysb, gamma, pl, rt, fn, vl, pa))
    for t in h.values():
        lib.zk_table_free(t)
