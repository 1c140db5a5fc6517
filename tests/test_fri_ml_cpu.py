"""CPU: the host side of the multilinear opening of a FRI commitment (include/zkmle.h "FRI commitment opened as a multilinear polynomial").
The Python model of tests/_fri_ml_model.py is checked against itself (its openings pass its verifier, a false y does not) and against the
identity the protocol rests on: every layer f_l of the Lagrange-form fold is the Reed-Solomon extension of the MLE fold T_l.  The library's
HOST verifier zk_fri_ml_verify accepts the model's openings over both fields, the shapes (d, b, f) = (1,1,0), (4,2,1), (6,1,0), (5,2,4), with
and without a coset, at random points and at points with entries in {0, 1, p - 1}; it rejects a single-bit change in every byte class, every
parameter that differs from the prover's and every element that is not reduced, and leaves a caller's transcript in the model's state.  The
same for zk_sumcheck_basic_verify_succinct on a model proof.  Counts and precondition codes are the header's, all before the device check.

A zk_fri_commitment cannot exist without a device: the prover runs in tests/test_gpu_fri_ml.py.  The new fold kernel adds no arithmetic
helper of its own (its products are fe_mul_u_pre, Multiplier and uni_muladd, which tools/fri_fold_selftest.hip and tools/ufield_selftest.hip
cover), so there is no new host-compiled self-test.

Trees are hashed with the library's host Keccak (tests/_merkle_model.py check_host_keccak: checked against the pure-Python one first)."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import __graft_entry__ as G
import _fri_ml_model as ML
import _fri_model as FM
import _fri_pcs_model as PM
import _merkle_model as MM
import _ntt_model as NM
from oracle import pymodel as M

zk = G.import_package()
P64, P8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
p64 = lambda a: a.ctypes.data_as(P64) if a is not None else None
p8 = lambda a: a.ctypes.data_as(P8) if a is not None else None
NEW_NAMES = ("zk_fri_ml_fold", "zk_fri_ml_sizes", "zk_fri_ml_open", "zk_fri_ml_verify", "zk_fri_ml_last_stats", "zk_sumcheck_basic_prove_succinct",
             "zk_sumcheck_basic_verify_succinct")
SHAPES = [(1, 1, 0), (4, 2, 1), (6, 1, 0), (5, 2, 4)]        # (d, b, f)


@functools.lru_cache(maxsize=None)
def hasher():
    return MM.check_host_keccak(zk)


@functools.lru_cache(maxsize=None)
def commitment(field, d, b, with_coset, seed=0):
    """a model commitment of one shape; built once per module"""
    coset = random.Random(37 * d + b + field).randrange(2, NM.MODULUS[field]) if with_coset else 1
    return PM.commit(field, NM.random_ints(field, 1 << d, 5200 + 13 * d + field + seed), b, coset, hasher())


def points(field, d):
    """a random point, and points whose entries lie in {0, 1, p - 1}: nothing is refused for lying in a domain"""
    p, rng = NM.MODULUS[field], random.Random(91 * d + field)
    edge = [[rng.choice((0, 1, p - 1)) for _ in range(d)] for _ in range(2)]
    return [[rng.randrange(p) for _ in range(d)], [0] * d, [1] * d, [p - 1] * d] + edge


def lib_verify(op, fl=None, tr=None, **over):
    """zk_fri_ml_verify on the model's opening `op` (flat arrays `fl`), parameters overridable -> (status, ok)"""
    fl = ML.flat(zk, op) if fl is None else fl
    a = {n: op[n] for n in ("d", "b", "f", "Q")}
    a.update({n: v for n, v in over.items() if n in a})
    coset = over.get("coset", op["coset"])
    cm = None if coset is None else zk.from_ints(op["field"], [coset])[0]
    ok = C.c_int(-1)
    rc = zk.lib().zk_fri_ml_verify(op["field"], p8(fl["root"]), a["d"], a["b"], a["f"], a["Q"], p64(cm), p64(fl["z"]), p64(fl["y"]),
                                   None if tr is None else tr._h, p64(fl["polys"]), p8(fl["roots"]), p64(fl["final"]), p64(fl["values"]),
                                   p8(fl["paths"]), C.byref(ok))
    return rc, ok.value


def test_new_exports_are_present():
    lib = zk.lib()
    header = open(G.ROOT + "/include/zkmle.h").read()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in header, name
    assert "zk_fri_ml_stats;" in header
    for name in ("open_multilinear", "verify_multilinear", "ml_fold", "FriMlOpening", "ml_sizes", "ml_last_stats"):
        assert callable(getattr(zk.fri, name)), name
    assert callable(zk.sumcheck.prove_succinct) and callable(zk.sumcheck.verify_succinct)


def test_sizes_agree_with_the_model():
    from zkmle_amd import _lib as L
    lib = zk.lib()
    out = [C.c_size_t(0) for _ in range(5)]
    for d, b, f, Q in [(1, 1, 0, 1), (3, 1, 0, 4), (5, 2, 2, 7), (11, 2, 6, 40), (22, 2, 6, 64), (24, 8, 23, 4096), (31, 1, 0, 1)]:
        assert lib.zk_fri_ml_sizes(d, b, f, Q, *[C.byref(o) for o in out]) == 0
        assert tuple(o.value for o in out) == ML.sizes(d, b, f, Q) == zk.fri.ml_sizes(d, b, f, Q)
    assert lib.zk_fri_ml_sizes(5, 2, 2, 7, *[None] * 5) == 0
    for bad in [(5, 0, 2, 7), (5, 9, 2, 7), (5, 2, 5, 7), (5, 2, 2, 0), (5, 2, 2, 4097), (0, 2, 0, 7)]:
        assert lib.zk_fri_ml_sizes(*bad, *[C.byref(o) for o in out]) == L.ZK_E_ARG, bad
    assert lib.zk_fri_ml_sizes(31, 2, 0, 1, *[C.byref(o) for o in out]) == L.ZK_E_RANGE
    assert lib.zk_fri_ml_sizes(31, 2, 0, 0, *[C.byref(o) for o in out]) == L.ZK_E_ARG        # ZK_E_ARG comes first


@pytest.mark.parametrize("with_coset", (False, True))
@pytest.mark.parametrize("field", (0, 3))
def test_every_model_layer_is_the_extension_of_the_folded_table(field, with_coset):
    """the identity the protocol rests on: f_l = low_degree_extend(T_l, b, c_l) for every l, the uncommitted layer R included"""
    p = NM.MODULUS[field]
    for d, b, f in ((4, 2, 1), (5, 1, 0)):
        cm = commitment(field, d, b, with_coset)
        op = ML.open_at(cm, points(field, d)[0], f, 2, hasher=hasher())
        c = cm["coset"]
        assert len(op["layers"]) == len(op["tables"]) == d - f + 1
        for l, (layer, table) in enumerate(zip(op["layers"], op["tables"])):
            assert layer == FM.extend(field, table, b, c), (d, b, f, l)
            c = c * c % p
        assert op["final"] == op["tables"][-1] and len(op["final"]) == 1 << f


@pytest.mark.parametrize("with_coset", (False, True))
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("field", (0, 3))
def test_model_openings_pass_the_model_verifier_and_the_library_verifier(field, shape, with_coset):
    d, b, f = shape
    cm = commitment(field, d, b, with_coset)
    for z in points(field, d):
        op = ML.open_at(cm, z, f, 3, hasher=hasher())
        assert op["y"] == ML.mle_evaluate(field, cm["coeffs"], z)
        assert ML.verify(op, hasher=hasher()), z
        fl = ML.flat(zk, op)
        assert lib_verify(op, fl) == (0, 1), (field, shape, with_coset, z)
        if not with_coset:
            assert lib_verify(op, fl, coset=None) == (0, 1)
        assert ML.sizes(d, b, f, 3) == (fl["roots"].shape[0], fl["final"].shape[0], fl["values"].size // 4, fl["paths"].size, fl["polys"].size // 4)
    # the Python wrapper on the last opening
    cs = zk.from_ints(field, [cm["coset"]])[0]
    o = zk.fri.FriMlOpening(field, d, b, f, 3, coset=cs)
    o.y, o.round_polys, o.roots, o.final_table, o.query_values, o.query_paths = fl["y"], fl["polys"], fl["roots"], fl["final"], fl["values"], fl["paths"]
    assert zk.fri.verify_multilinear(cm["root"], fl["z"], o)
    assert not zk.fri.verify_multilinear(cm["root"][::-1], fl["z"], o)


def test_a_false_y_is_rejected_by_the_model_and_by_the_library():
    """a round 0 shifted so that it sums to the false claim passes its own check; the next one -- round 1's sum, or with R = 1 the final
    A_R MLE(T_R)(..) = claim -- is what fails, since everything after round 0 is the honest run"""
    for field, d, b, f in ((0, 6, 1, 0), (3, 5, 2, 2)):
        cm = commitment(field, d, b, field == 3, seed=3)
        z = points(field, d)[0]
        honest = ML.open_at(cm, z, f, 8, hasher=hasher())
        assert ML.verify(honest, hasher=hasher()) and lib_verify(honest) == (0, 1)
        op = ML.open_at(cm, z, f, 8, false_y=honest["y"] + 1, hasher=hasher())
        assert op["y"] != honest["y"] and (op["polys"][0][0] + op["polys"][0][1] - op["y"]) % NM.MODULUS[field] == 0
        assert not ML.verify(op, hasher=hasher())
        assert lib_verify(op) == (0, 0)


def small_opening(tr=None):
    cm = commitment(0, 3, 1, True, seed=9)
    return ML.open_at(cm, points(0, 3)[0], 0, 4, tr, hasher=hasher())


def test_every_single_bit_change_is_rejected():
    """every byte class: the round polynomials, the roots, the final table, the values, the paths, y, z and the verifier's root"""
    op = small_opening()
    d, L, R, Q = 3, 4, 3, 4
    base = ML.flat(zk, op)
    assert lib_verify(op, base) == (0, 1)
    rng = random.Random(7411)
    spots = [("polys", (l, k, rng.randrange(4))) for l in range(R) for k in range(3)]
    spots += [("roots", (l, rng.randrange(32))) for l in range(R)]
    spots += [("final", (0, rng.randrange(4)))]
    spots += [("y", (w,)) for w in range(4)]
    spots += [("z", (i, rng.randrange(4))) for i in range(d)]
    spots += [("root", (rng.randrange(32),)) for _ in range(3)]
    for q in (0, 3):
        for l in range(R):
            spots += [("values", (q, l, s, rng.randrange(4))) for s in range(2)]
    per_query = base["paths"].size // Q
    off = 0
    for l in range(R):                                                               # query 1: first and last digest of both paths of every layer
        for side in range(2):
            spots.append(("paths", (per_query + off + rng.randrange(32),)))
            spots.append(("paths", (per_query + off + 32 * (L - l - 1) + rng.randrange(32),)))
            off += 32 * (L - l)
    assert off == per_query
    for name, at in spots:
        fl = {n: v.copy() for n, v in base.items()}
        bits = 8 if fl[name].dtype == np.uint8 else 64
        fl[name][at] ^= fl[name].dtype.type(1 << rng.randrange(bits))
        assert lib_verify(op, fl) == (0, 0), (name, at)
    p = NM.MODULUS[0]
    for name, at in (("y", ()), ("z", (1,)), ("polys", (1, 2)), ("polys", (0, 0)), ("final", (0,)), ("values", (2, 1, 0))):
        fl = {n: v.copy() for n, v in base.items()}                                  # the same residue, not reduced: x + p < 2^256
        fl[name][at] = np.frombuffer((int.from_bytes(fl[name][at].tobytes(), "little") + p).to_bytes(32, "little"), np.uint64)
        assert lib_verify(op, fl) == (0, 0), name


def test_a_verifier_with_other_parameters_rejects():
    op = small_opening()
    fl = ML.flat(zk, op)
    big = {n: np.concatenate([v.reshape(-1), np.zeros(4 * v.size + 4096, v.dtype)]) for n, v in fl.items()}   # room for any shape below
    assert lib_verify(op, big) == (0, 1)
    for over in ({"Q": 3}, {"Q": 5}, {"f": 1}, {"coset": 1}, {"coset": None}, {"coset": op["coset"] + 1}, {"b": 2}, {"d": 4}, {"d": 2}):
        assert lib_verify(op, big, **over) == (0, 0), over
    other = ML.open_at(commitment(0, 3, 1, True, seed=9), points(0, 3)[1], 0, 4, hasher=hasher())
    assert lib_verify(op, dict(big, z=ML.flat(zk, other)["z"])) == (0, 0)               # another point


def test_a_callers_transcript_ends_in_the_models_state():
    prior = b"what the caller had absorbed before"
    mt = M.Transcript()
    mt.append(prior)
    op = small_opening(mt)
    vt = M.Transcript()
    vt.append(prior)
    assert ML.verify(op, vt, hasher()) and vt.buf == mt.buf
    t = zk.Transcript()
    t.append(prior)
    assert lib_verify(op, tr=t) == (0, 1)
    want = zk.Transcript()
    want.append(bytes(mt.buf))
    assert np.array_equal(t.export_state(), want.export_state())
    assert lib_verify(op) == (0, 0)                                   # the opening is bound to the prior content


# ---- the succinct basic sumcheck --------------------------------------------------------------------------------------------------------
def lib_verify_sumcheck(pr, root, tr=None, claimed=None):
    op = pr["opening"]
    fl = ML.flat(zk, op)
    field = op["field"]
    cs = zk.from_ints(field, [pr["claimed_sum"] if claimed is None else claimed])[0]
    rp = zk.from_ints(field, [e for pair in pr["rounds"] for e in pair])
    cm = zk.from_ints(field, [op["coset"]])[0]
    rbuf = np.frombuffer(root, np.uint8).copy()
    ok = C.c_int(-1)
    rc = zk.lib().zk_sumcheck_basic_verify_succinct(field, p8(rbuf), op["d"], op["b"], op["f"], op["Q"], p64(cm), None if tr is None else tr._h, p64(cs),
                                                    p64(rp), p64(fl["y"]), p64(fl["polys"]), p8(fl["roots"]), p64(fl["final"]), p64(fl["values"]),
                                                    p8(fl["paths"]), C.byref(ok))
    return rc, ok.value


@pytest.mark.parametrize("field,d,b,f", [(0, 1, 1, 0), (0, 4, 2, 1), (3, 5, 1, 0), (3, 5, 2, 4)])
def test_the_succinct_sumcheck_verifier_accepts_the_models_proofs(field, d, b, f):
    p = NM.MODULUS[field]
    cm = commitment(field, d, b, d % 2 == 1, seed=5)
    pr = ML.sumcheck_prove(cm, f, 3, hasher=hasher())
    assert pr["claimed_sum"] == sum(cm["coeffs"]) % p and pr["opening"]["z"] == pr["challenges"]
    assert ML.sumcheck_verify(pr, cm["root"], hasher=hasher())
    assert lib_verify_sumcheck(pr, cm["root"]) == (0, 1)
    assert lib_verify_sumcheck(pr, cm["root"], claimed=(pr["claimed_sum"] + 1) % p) == (0, 0)      # a tampered claimed sum
    bad_root = bytes([cm["root"][0] ^ 1]) + cm["root"][1:]
    assert not ML.sumcheck_verify(pr, bad_root, hasher=hasher()) and lib_verify_sumcheck(pr, bad_root) == (0, 0)
    e0, e1 = pr["rounds"][0]
    shifted = dict(pr, rounds=[((e0 + 1) % p, (e1 - 1) % p)] + pr["rounds"][1:])                    # still sums to the claim
    assert not ML.sumcheck_verify(shifted, cm["root"], hasher=hasher()) and lib_verify_sumcheck(shifted, cm["root"]) == (0, 0)


def test_the_succinct_sumcheck_verifier_leaves_a_callers_transcript_in_the_models_state():
    prior = b"a caller's earlier statements"
    cm = commitment(0, 4, 1, True, seed=6)
    mt = M.Transcript()
    mt.append(prior)
    pr = ML.sumcheck_prove(cm, 1, 3, mt, hasher=hasher())
    vt = M.Transcript()
    vt.append(prior)
    assert ML.sumcheck_verify(pr, cm["root"], vt, hasher()) and vt.buf == mt.buf
    t = zk.Transcript()
    t.append(prior)
    assert lib_verify_sumcheck(pr, cm["root"], tr=t) == (0, 1)
    want = zk.Transcript()
    want.append(bytes(mt.buf))
    assert np.array_equal(t.export_state(), want.export_state())
    assert lib_verify_sumcheck(pr, cm["root"]) == (0, 0)


def wrapped(field, length):
    """a table handle over memory nobody reads: the precondition codes are returned before anything is launched"""
    from zkmle_amd import _lib as L
    h = C.c_void_p()
    L.check(zk.lib().zk_table_wrap(field, C.c_void_p(0x1000), length, C.byref(h)))
    return h


def test_precondition_codes_come_before_the_device_check():
    import torch
    from zkmle_amd import _lib as L
    lib = zk.lib()
    have_gpu = torch.cuda.is_available()
    roots, fin, vals, paths = np.zeros(64 * 32, np.uint8), np.zeros(4 << 10, np.uint64), np.zeros(1 << 16, np.uint64), np.zeros(1 << 20, np.uint8)
    root, z, y, polys = np.zeros(32, np.uint8), np.zeros(64 * 4, np.uint64), np.zeros(4, np.uint64), np.zeros(64 * 12, np.uint64)
    cs, rp = np.zeros(4, np.uint64), np.zeros(64 * 8, np.uint64)
    for field in (0, 1, 2, 3):
        nl = zk.limbs(field)
        zero, one = np.zeros(nl, np.uint64), zk.from_ints(field, [1])[0]
        out = C.c_void_p()
        # the fold: zk_fri_fold's order
        fold = lambda t, r, coset, o=C.byref(out): lib.zk_fri_ml_fold(t, p64(r), p64(coset), o)
        t1, t6, t8 = (wrapped(field, n) for n in (1, 6, 8))
        assert fold(None, one, None) == L.ZK_E_ARG and fold(t8, None, None) == L.ZK_E_ARG and fold(t8, one, None, None) == L.ZK_E_ARG
        assert fold(t1, one, None) == L.ZK_E_ARG and fold(t8, one, zero) == L.ZK_E_ARG and fold(t6, one, zero) == L.ZK_E_ARG
        assert fold(t6, one, None) == L.ZK_E_NOT_POW2
        if field in (1, 2):
            assert fold(t8, one, None) == L.ZK_E_RANGE
        else:
            big = wrapped(field, 1 << (NM.two_adicity(field) + 1))
            assert fold(big, one, None) == L.ZK_E_RANGE
            lib.zk_table_free(big)
            if not have_gpu:
                assert fold(t8, one, None) == L.ZK_E_NO_DEVICE and fold(t8, one, one) == L.ZK_E_NO_DEVICE
        for h in (t1, t6, t8):
            lib.zk_table_free(h)
        # the verifiers: host code, the same order without a device check
        ok = C.c_int(-1)
        ver = lambda d, b, f, Q, coset, okp=C.byref(ok), r=root, zz=z: lib.zk_fri_ml_verify(
            field, p8(r), d, b, f, Q, p64(coset), p64(zz), p64(y), None, p64(polys), p8(roots), p64(fin), p64(vals), p8(paths), okp)
        sver = lambda d, b, f, Q, coset, okp=C.byref(ok), r=root, c=cs: lib.zk_sumcheck_basic_verify_succinct(
            field, p8(r), d, b, f, Q, p64(coset), None, p64(c), p64(rp), p64(y), p64(polys), p8(roots), p64(fin), p64(vals), p8(paths), okp)
        for v in (ver, sver):
            assert v(3, 1, 0, 4, None, None) == L.ZK_E_ARG and v(3, 1, 0, 4, None, r=None) == L.ZK_E_ARG
            for d, b, f, Q in ((3, 0, 0, 4), (3, 9, 0, 4), (3, 1, 0, 0), (3, 1, 0, 4097), (3, 1, 3, 4), (0, 1, 0, 4), (40, 1, 40, 4), (40, 0, 0, 4)):
                assert v(d, b, f, Q, None) == L.ZK_E_ARG, (d, b, f, Q)
            assert v(3, 1, 0, 4, zero) == L.ZK_E_ARG
            if field in (1, 2):
                assert v(3, 1, 0, 4, None) == L.ZK_E_RANGE
            else:
                assert v(NM.two_adicity(field), 1, 0, 4, None) == L.ZK_E_RANGE and v(40, 1, 0, 4, None) == L.ZK_E_RANGE
                assert v(3, 1, 0, 4, None) == 0 and ok.value == 0                      # zeros are no proof
                assert v(3, 1, 0, 4, one) == 0 and ok.value == 0
        assert ver(3, 1, 0, 4, None, zz=None) == L.ZK_E_ARG and sver(3, 1, 0, 4, None, c=None) == L.ZK_E_ARG
        assert lib.zk_fri_ml_verify(-1, p8(root), 3, 1, 0, 4, None, p64(z), p64(y), None, p64(polys), p8(roots), p64(fin), p64(vals), p8(paths),
                                    C.byref(ok)) == L.ZK_E_ARG
        # the provers' entry points, as far as they go without a commitment
        op = lambda cm, zz, yy=y: lib.zk_fri_ml_open(cm, p64(zz), 0, 4, None, p64(yy), p64(polys), p8(roots), p64(fin), None, None, p64(vals), p8(paths))
        assert op(None, z) == L.ZK_E_ARG
        assert lib.zk_sumcheck_basic_prove_succinct(None, 0, 4, None, p64(cs), p64(rp), p64(z), p64(y), p64(polys), p8(roots), p64(fin), None, None,
                                                    p64(vals), p8(paths)) == L.ZK_E_ARG
    assert lib.zk_fri_ml_last_stats(None) == L.ZK_E_ARG
