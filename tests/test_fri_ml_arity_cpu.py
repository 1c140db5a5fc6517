"""CPU: the host side of the multilinear opening folded by 4 (include/zkmle.h "FRI commitment opened with a fold arity").  The Python model
of tests/_fri_ml_arity_model.py is checked against itself (two model folds equal the four-point formula; its openings pass its verifier) and
the library's HOST verifier zk_fri_ml_verify_points_arity accepts the model's log_arity = 2 openings over both fields at R = 2 (one fold by 4
straight to the final table), R = 3 (a fold by 4, then a fold by 2), R = 4 and R = 5, b in {1, 2}, with and without a coset, P in {1, 2, 8},
Q = 8; it rejects a flipped round element, root, final-table entry, opened value at each side, path digest, and an unreduced element.  With
log_arity = 1 the new entry points are the several-point protocol's: its model's openings are accepted and a caller's transcript ends in the
same state.  zk_fri_ml_sizes_arity equals the header's formulas, and the argument statuses are the documented ones.

A zk_fri_commitment cannot exist without a device: the fold kernel and the prover run in tests/test_gpu_fri_ml_arity.py."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import __graft_entry__ as G
import _fri_ml_arity_model as AM
import _fri_ml_cases as FC
import _fri_ml_model as ML
import _fri_ml_points_model as PT
import _ntt_model as NM
from oracle import pymodel as M

zk = G.import_package()
P64, P8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
p64 = lambda a: a.ctypes.data_as(P64) if a is not None else None
p8 = lambda a: a.ctypes.data_as(P8) if a is not None else None
NEW_NAMES = ("zk_fri_ml_fold4", "zk_fri_ml_sizes_arity", "zk_fri_ml_open_points_arity", "zk_fri_ml_verify_points_arity")
SHAPES = [(3, 1, 1), (4, 2, 1), (4, 1, 0), (6, 2, 1)]        # (d, b, f): R = 2, 3, 4, 5
Q = 8


hasher = functools.partial(FC.hasher, zk)
padded = FC.padded


@functools.lru_cache(maxsize=None)
def commitment(field, d, b, with_coset):
    return FC.commitment(field, d, b, FC.coset_of(field, d, b, with_coset, 43), 7300 + 13 * d + field, hasher())


def points_for(field, d, P):
    return FC.points_for(field, d, P, 101 * d + 7 * P + field)


@functools.lru_cache(maxsize=None)
def opening(field, d, b, f, with_coset, P):
    return AM.open_points(commitment(field, d, b, with_coset), points_for(field, d, P), f, Q, hasher=hasher())


def lib_verify(op, fl=None, tr=None, a=2, flat=AM.flat, **over):
    """zk_fri_ml_verify_points_arity on the model's opening `op` (flat arrays `fl`) -> (status, ok)"""
    fl = flat(zk, op) if fl is None else fl
    s = {n: op[n] for n in ("d", "b", "f", "Q")}
    s.update({n: v for n, v in over.items() if n in s})
    coset = over.get("coset", op["coset"])
    cm = None if coset is None else zk.from_ints(op["field"], [coset])[0]
    ok = C.c_int(-1)
    rc = zk.lib().zk_fri_ml_verify_points_arity(op["field"], p8(fl["root"]), s["d"], s["b"], s["f"], s["Q"], a, p64(cm), p64(fl["points"]), len(op["points"]),
                                                p64(fl["ys"]), None if tr is None else tr._h, p64(fl["polys"]), p8(fl["roots"]), p64(fl["final"]),
                                                p64(fl["values"]), p8(fl["paths"]), C.byref(ok))
    return rc, ok.value


def test_new_exports_are_present():
    lib = zk.lib()
    header = open(G.ROOT + "/include/zkmle.h").read()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in header, name
    assert "FRI commitment opened with a fold arity" in header
    assert callable(zk.fri.ml_fold4)
    assert zk.fri.FriMlPointsOpening(0, 2, 5, 1, 0, 4, log_arity=2).log_arity == 2


@pytest.mark.parametrize("field", (0, 3))
def test_two_model_folds_equal_the_four_point_formula(field):
    p = NM.MODULUS[field]
    rng = random.Random(19 + field)
    for loglen in (2, 3, 5):
        table = NM.random_ints(field, 1 << loglen, 8100 + loglen + field)
        for coset in (1, rng.randrange(2, p)):
            edge = [(r0, r1) for r0 in (0, 1, p - 1) for r1 in (0, 1, p - 1)]
            for r0, r1 in edge + [(rng.randrange(p), rng.randrange(p))]:
                twice = ML.fold(field, ML.fold(field, table, r0, coset), r1, coset * coset % p)
                assert AM.fold4_formula(field, table, r0, r1, coset) == twice, (loglen, coset, r0, r1)


@pytest.mark.parametrize("with_coset", (False, True))
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("field", (0, 3))
def test_model_openings_pass_the_model_verifier_and_the_library_verifier(field, shape, with_coset):
    d, b, f = shape
    for P in (1, 2, 8):
        op = opening(field, d, b, f, with_coset, P)
        assert op["ys"] == [ML.mle_evaluate(field, commitment(field, d, b, with_coset)["coeffs"], z) for z in op["points"]]
        assert len(op["roots"]) == (d - f + 1) // 2
        assert AM.verify(op, hasher=hasher()), P
        fl = AM.flat(zk, op)
        assert lib_verify(op, fl) == (0, 1), (field, shape, with_coset, P)
        if not with_coset:
            assert lib_verify(op, fl, coset=None) == (0, 1)
        assert AM.sizes(d, b, f, Q) == (fl["roots"].shape[0], fl["final"].shape[0], fl["values"].size // 4, fl["paths"].size, fl["polys"].size // 4)
        assert lib_verify(op, padded(fl), a=1) == (0, 0)       # the same bytes are no arity-1 proof
    # the Python wrapper on the last opening
    cs = zk.from_ints(field, [op["coset"]])[0]
    o = zk.fri.FriMlPointsOpening(field, 8, d, b, f, Q, coset=cs, log_arity=2)
    assert o.roots.shape == fl["roots"].shape and o.query_values.shape == fl["values"].shape and o.query_paths.shape == fl["paths"].shape
    o.ys, o.round_polys, o.roots, o.final_table, o.query_values, o.query_paths = fl["ys"], fl["polys"], fl["roots"], fl["final"], fl["values"], fl["paths"]
    assert zk.fri.verify_multilinear_points(op["root"], fl["points"], o)
    assert zk.fri.verify_multilinear_points(op["root"], fl["points"], o, log_arity=2)
    assert not zk.fri.verify_multilinear_points(op["root"][::-1], fl["points"], o)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("field", (0, 3))
def test_every_tampered_class_is_rejected(field, shape):
    """one flipped bit of a round element, a root, a final-table entry, an opened value at each side of each step, a path digest of each path;
    and an element of each class that is not reduced"""
    d, b, f = shape
    L, R = d + b, d - f
    op = opening(field, d, b, f, True, 2)
    base = AM.flat(zk, op)
    assert lib_verify(op, base) == (0, 1)
    rng = random.Random(913 + d + field)
    st = AM.steps(L, R)
    spots = [("polys", (l, k, rng.randrange(4))) for l in range(R) for k in range(3)]
    spots += [("roots", (s, rng.randrange(32))) for s in range(len(op["roots"]))]
    spots += [("final", (j, rng.randrange(4))) for j in range(1 << f)]
    spots += [("ys", (k, rng.randrange(4))) for k in range(2)]
    voff = poff = 0
    per_query = base["paths"].size // Q
    for l, sides in st:                                       # query 1 for the values, query 2 for the paths: every side of every step
        for s in range(sides):
            spots.append(("values", (1, voff + s, rng.randrange(4))))
            spots.append(("paths", (2 * per_query + poff + rng.randrange(32),)))                    # the first digest of the path
            spots.append(("paths", (2 * per_query + poff + 32 * (L - l - 1) + rng.randrange(32),)))   # and the last
            poff += 32 * (L - l)
        voff += sides
    assert poff == per_query and voff == base["values"].shape[1]
    for name, at in spots:
        fl = {n: v.copy() for n, v in base.items()}
        bits = 8 if fl[name].dtype == np.uint8 else 64
        fl[name][at] ^= fl[name].dtype.type(1 << rng.randrange(bits))
        assert lib_verify(op, fl) == (0, 0), (name, at)
    p = NM.MODULUS[field]
    for name, at in (("ys", (1,)), ("points", (0, 1)), ("polys", (R - 1, 2)), ("final", (0,)), ("values", (3, 0)), ("values", (0, voff - 1))):
        fl = {n: v.copy() for n, v in base.items()}           # the same residue, not reduced: x + p < 2^256
        fl[name][at] = np.frombuffer((int.from_bytes(fl[name][at].tobytes(), "little") + p).to_bytes(32, "little"), np.uint64)
        assert lib_verify(op, fl) == (0, 0), (name, at)


def test_a_verifier_with_other_parameters_rejects():
    op = opening(0, 4, 2, 1, True, 2)
    fl = AM.flat(zk, op)
    big = {n: np.concatenate([v.reshape(-1), np.zeros(4 * v.size + 4096, v.dtype)]) for n, v in fl.items()}   # room for any shape below
    assert lib_verify(op, big) == (0, 1)
    for over in ({"Q": 7}, {"f": 0}, {"f": 2}, {"coset": 1}, {"coset": None}, {"b": 1}, {"d": 5}):
        assert lib_verify(op, big, **over) == (0, 0), over


def test_a_callers_transcript_ends_in_the_models_state():
    prior = b"what the caller had absorbed before"
    cm = commitment(3, 4, 1, True)
    mt = M.Transcript()
    mt.append(prior)
    op = AM.open_points(cm, points_for(3, 4, 2), 1, Q, mt, hasher=hasher())
    vt = M.Transcript()
    vt.append(prior)
    assert AM.verify(op, vt, hasher()) and vt.buf == mt.buf
    t = zk.Transcript()
    t.append(prior)
    assert lib_verify(op, tr=t) == (0, 1)
    want = zk.Transcript()
    want.append(bytes(mt.buf))
    assert np.array_equal(t.export_state(), want.export_state())
    assert lib_verify(op) == (0, 0)                           # the opening is bound to the prior content


@pytest.mark.parametrize("field", (0, 3))
def test_arity_one_is_the_several_point_protocol(field):
    """a proof of tests/_fri_ml_points_model.py is accepted through the new entry point, and the transcript's next challenge is the one
    after zk_fri_ml_verify_points"""
    for d, b, f, P in ((1, 1, 0, 1), (4, 2, 1, 2), (5, 1, 0, 8)):
        cm = commitment(field, d, b, d % 2 == 0)
        op = PT.open_points(cm, points_for(field, d, P), f, Q, hasher=hasher())
        fl = PT.flat(zk, op)
        t_new, t_old = zk.Transcript(), zk.Transcript()
        assert lib_verify(op, fl, tr=t_new, a=1, flat=PT.flat) == (0, 1), (d, b, f, P)
        ok = C.c_int(-1)
        cs = zk.from_ints(field, [op["coset"]])[0]
        assert zk.lib().zk_fri_ml_verify_points(field, p8(fl["root"]), d, b, f, Q, p64(cs), p64(fl["points"]), P, p64(fl["ys"]), t_old._h, p64(fl["polys"]),
                                                p8(fl["roots"]), p64(fl["final"]), p64(fl["values"]), p8(fl["paths"]), C.byref(ok)) == 0 and ok.value == 1
        assert np.array_equal(t_new.export_state(), t_old.export_state())
        assert np.array_equal(t_new.random_challenge_as_field_element(field), t_old.random_challenge_as_field_element(field))
        if d - f >= 2:
            assert lib_verify(op, padded(fl), a=2) == (0, 0)   # and no arity-2 proof


def test_sizes_and_statuses():
    from zkmle_amd import _lib as L
    lib = zk.lib()

    def sizes(d, b, f, q, a):
        out = [C.c_size_t(0) for _ in range(5)]
        rc = lib.zk_fri_ml_sizes_arity(d, b, f, q, a, *[C.byref(o) for o in out])
        return rc, tuple(int(o.value) for o in out)

    for d in range(2, 12):
        for b in (1, 2, 3):
            for f in range(0, d - 1):
                for q in (1, 8, 64):
                    assert sizes(d, b, f, q, 2) == (0, AM.sizes(d, b, f, q)), (d, b, f, q)
                    assert sizes(d, b, f, q, 1) == (0, ML.sizes(d, b, f, q))
                    assert zk.fri.ml_sizes(d, b, f, q, log_arity=2) == AM.sizes(d, b, f, q) and zk.fri.ml_sizes(d, b, f, q) == ML.sizes(d, b, f, q)
    # R = 2: one root, four values and four paths of L digests a query; R = 3: two roots, 4 + 2 values
    assert AM.sizes(5, 2, 3, 8) == (1, 8, 32, 32 * 8 * 4 * 7, 6) and AM.sizes(5, 2, 2, 8) == (2, 4, 48, 32 * 8 * (4 * 7 + 2 * 5), 9)
    assert sizes(4, 1, 0, 8, 0)[0] == L.ZK_E_ARG and sizes(4, 1, 0, 8, 3)[0] == L.ZK_E_ARG and sizes(4, 1, 3, 8, 2)[0] == L.ZK_E_ARG
    assert sizes(4, 1, 3, 8, 1)[0] == 0 and sizes(4, 1, 4, 8, 2)[0] == L.ZK_E_ARG and sizes(40, 1, 0, 8, 2)[0] == L.ZK_E_RANGE
    assert lib.zk_fri_ml_sizes_arity(4, 1, 0, 8, 2, None, None, None, None, None) == 0
    with pytest.raises(L.ZkError) as e:
        zk.fri.ml_sizes(4, 1, 3, 8, log_arity=2)
    assert e.value.code == L.ZK_E_ARG

    roots, fin, vals, paths = np.zeros(64 * 32, np.uint8), np.zeros(4 << 10, np.uint64), np.zeros(1 << 16, np.uint64), np.zeros(1 << 20, np.uint8)
    root, pts, ys, polys = np.zeros(32, np.uint8), np.zeros(8 * 64 * 4, np.uint64), np.zeros(8 * 4, np.uint64), np.zeros(64 * 12, np.uint64)
    ok = C.c_int(-1)
    for field in (0, 1, 2, 3):
        ver = lambda d, b, f, q, a, P=2, okp=C.byref(ok): lib.zk_fri_ml_verify_points_arity(
            field, p8(root), d, b, f, q, a, None, p64(pts), P, p64(ys), None, p64(polys), p8(roots), p64(fin), p64(vals), p8(paths), okp)
        for a in (0, 3, 1 << 31):
            assert ver(3, 1, 0, 4, a) == L.ZK_E_ARG, a
        assert ver(3, 1, 2, 4, 2) == L.ZK_E_ARG                                             # R = 1
        assert ver(3, 1, 0, 4, 2, okp=None) == L.ZK_E_ARG and ver(3, 1, 0, 4, 2, P=0) == L.ZK_E_ARG and ver(3, 1, 0, 4, 2, P=9) == L.ZK_E_ARG
        for d, b, f, q in ((3, 0, 0, 4), (3, 9, 0, 4), (3, 1, 0, 0), (3, 1, 0, 4097), (3, 1, 3, 4), (0, 1, 0, 4), (40, 1, 40, 4), (40, 1, 39, 4)):
            assert ver(d, b, f, q, 2) == L.ZK_E_ARG, (d, b, f, q)
        if field in (1, 2):
            assert ver(3, 1, 0, 4, 2) == L.ZK_E_RANGE and ver(3, 1, 2, 4, 1) == L.ZK_E_RANGE
        else:
            assert ver(NM.two_adicity(field), 1, 0, 4, 2) == L.ZK_E_RANGE and ver(40, 1, 0, 4, 2) == L.ZK_E_RANGE
            assert ver(3, 1, 0, 4, 2) == 0 and ok.value == 0                                # zeros are no proof
            assert ver(3, 1, 2, 4, 1) == 0 and ok.value == 0
    # the device entries, as far as they go without a table or a commitment
    one = zk.from_ints(0, [1])[0]
    out = C.c_void_p()
    assert lib.zk_fri_ml_open_points_arity(None, p64(pts), 2, 0, 4, 2, None, p64(ys), None, p64(polys), p8(roots), p64(fin), None, None, p64(vals),
                                           p8(paths)) == L.ZK_E_ARG
    assert lib.zk_fri_ml_fold4(None, p64(one), p64(one), None, C.byref(out)) == L.ZK_E_ARG
    h = {}
    for n in (1, 2, 4, 6, 8):
        h[n] = C.c_void_p()
        L.check(lib.zk_table_wrap(0, C.c_void_p(0x1000), n, C.byref(h[n])))
    other = C.c_void_p()
    L.check(lib.zk_table_wrap(1, C.c_void_p(0x1000), 8, C.byref(other)))
    f4 = lambda t, r0=one, r1=one, cs=None, o=C.byref(out): lib.zk_fri_ml_fold4(t, p64(r0), p64(r1), p64(cs), o)
    assert f4(h[1]) == L.ZK_E_ARG and f4(h[2]) == L.ZK_E_ARG and f4(h[8], r1=None) == L.ZK_E_ARG and f4(h[8], o=None) == L.ZK_E_ARG
    assert f4(h[8], cs=np.zeros(4, np.uint64)) == L.ZK_E_ARG and f4(h[6]) == L.ZK_E_NOT_POW2 and f4(other) == L.ZK_E_RANGE
    import torch
    if not torch.cuda.is_available():
        assert f4(h[4]) == L.ZK_E_NO_DEVICE and f4(h[8]) == L.ZK_E_NO_DEVICE
    assert not out.value
    for t in list(h.values()) + [other]:
        lib.zk_table_free(t)
