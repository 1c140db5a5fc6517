"""CPU: the host side of the Merkle tree with grouped leaves and of the multilinear opening over such trees (include/zkmle.h "Merkle commitment
with grouped leaves", "FRI commitment opened with grouped leaves").  Everything compares byte for byte against the big-integer model of
tests/_fri_ml_grouped_model.py:

  leaf and path   zk_merkle_verify_grouped accepts the model's leaves and paths on both fields for log_group 1 and 2 at depths 0, 1 and 5 and
                  rejects a changed element in each slot, two slots swapped, a changed digest, a wrong index and an element >= p
  opening         zk_fri_ml_verify_points_grouped accepts the model's openings on the cases of tests/test_gpu_fri_ml_arity.py (R = 2 .. 9: the
                  fold-4 step and the final fold-2 step with its pair leaf), and rejects one change of each class; an ungrouped fold-by-4
                  opening of the same table is no grouped one, and the reverse
  sizes           zk_fri_ml_sizes_grouped equals the header's formula; 144 digests a query at (24, 2, 6); below arity 1's whenever R >= 2
  statuses        the argument errors come before any device call and write nothing

A commitment cannot exist without a device: the kernels and the prover run in tests/test_gpu_merkle_grouped.py and test_gpu_fri_ml_grouped.py."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import __graft_entry__ as G
import _fri_ml_arity_model as AM
import _fri_ml_cases as FC
import _fri_ml_grouped_model as GM
import _fri_ml_model as ML
import _fri_pcs_model as PM
import _merkle_model as MM
import _ntt_model as NM

zk = G.import_package()
P64, P8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
p64 = lambda a: a.ctypes.data_as(P64) if a is not None else None
p8 = lambda a: a.ctypes.data_as(P8) if a is not None else None
NEW_NAMES = ("zk_merkle_build_grouped", "zk_mle_merkle_root_grouped", "zk_merkle_verify_grouped", "zk_fri_commit_grouped",
             "zk_fri_commitment_log_group", "zk_fri_ml_sizes_grouped", "zk_fri_ml_open_points_grouped", "zk_fri_ml_verify_points_grouped")
# (field, d, b, f, P, coset) of tests/test_gpu_fri_ml_arity.py CASES (a GPU module: not imported here): R = 2, 3, 2, 4, 3, 5, 6, 8, 9
CASES = [(0, 3, 1, 1, 1, False), (3, 3, 2, 0, 2, True), (3, 4, 1, 2, 8, False), (0, 4, 2, 0, 2, True), (0, 6, 2, 3, 8, True), (3, 6, 1, 1, 1, True),
         (0, 6, 1, 0, 2, False), (3, 10, 2, 2, 2, False), (0, 10, 1, 1, 1, True), (3, 10, 1, 2, 8, True)]
Q = 8
case_id = lambda c: "-".join(str(int(v)) for v in c)


hasher = functools.partial(FC.hasher, zk, True)
padded, tampered = FC.padded, FC.tampered


def test_new_exports_are_present():
    lib = zk.lib()
    header = open(G.ROOT + "/include/zkmle.h").read()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in header, name
    assert "FRI commitment opened with grouped leaves" in header and "Merkle commitment with grouped leaves" in header
    import inspect
    assert "log_group" in inspect.signature(zk.fri.commit).parameters and "log_group" in inspect.signature(zk.merkle_root).parameters
    assert "log_group" in inspect.signature(zk.MerkleTree.build).parameters and "log_group" in inspect.signature(zk.MerkleTree.verify).parameters
    assert zk.fri.FriMlPointsOpening(0, 2, 5, 1, 0, 4, log_arity=2, grouped=True).grouped


# ---- leaf and path ------------------------------------------------------------------------------------------------------------------------
def c_verify(field, root, depth, index, lg, elements, path):
    ok = C.c_int(-1)
    rbuf = np.frombuffer(bytes(root), np.uint8).copy()
    pbuf = np.frombuffer(b"".join(path), np.uint8).copy() if path else None
    el = np.ascontiguousarray(elements, np.uint64)
    rc = zk.lib().zk_merkle_verify_grouped(field, p8(rbuf), depth, index, lg, p64(el), p8(pbuf), C.byref(ok))
    return rc, ok.value


@pytest.mark.parametrize("lg", (1, 2))
@pytest.mark.parametrize("field", (0, 3))
def test_merkle_verify_grouped_agrees_with_the_model(field, lg):
    p, G_ = NM.MODULUS[field], 1 << lg
    rng = random.Random(77 * field + lg)
    for depth in (0, 1, 5):
        part = 1 << depth
        ints = MM.random_ints(field, part << lg, 4100 + 10 * depth + field + lg)
        levels = GM.levels_of(ints, lg)
        root = levels[-1][0]
        assert len(levels) == depth + 1 and len(levels[0]) == part
        if depth == 0:
            assert root == levels[0][0]
        for j in sorted({0, part - 1, part // 2, rng.randrange(part)}):
            group = [ints[j + s * part] for s in range(G_)]
            path = MM.path_of(levels, j)
            assert GM.verify_leaf(root, j, group, path)
            el = zk.from_ints(field, group)
            assert c_verify(field, root, depth, j, lg, el, path) == (0, 1), (depth, j)
            assert zk.MerkleTree.verify(field, root, j, el, np.frombuffer(b"".join(path), np.uint8), log_group=lg)
            for s in range(G_):                               # a changed element in each slot; the same residue, not reduced
                bad = el.copy()
                bad[s, rng.randrange(4)] ^= np.uint64(1 << rng.randrange(64))
                assert c_verify(field, root, depth, j, lg, bad, path) == (0, 0), (depth, j, s)
                unred = el.copy()
                v = int.from_bytes(el[s].tobytes(), "little") + p
                if v < 1 << 256:
                    unred[s] = np.frombuffer(v.to_bytes(32, "little"), np.uint64)
                    assert c_verify(field, root, depth, j, lg, unred, path) == (0, 0), (depth, j, s)
            for a, b in ((0, 1), (0, G_ - 1)):                 # two slots swapped
                if group[a] != group[b]:
                    sw = el.copy()
                    sw[[a, b]] = sw[[b, a]]
                    assert c_verify(field, root, depth, j, lg, sw, path) == (0, 0)
            for l in range(depth):                            # a changed digest, and the neighbour's index
                bp = list(path)
                bp[l] = bytes([bp[l][0] ^ 1]) + bp[l][1:]
                assert c_verify(field, root, depth, j, lg, el, bp) == (0, 0)
            if depth:
                assert c_verify(field, root, depth, j ^ 1, lg, el, path) == (0, 0)
                assert c_verify(field, root, depth, j ^ (part >> 1), lg, el, path) == (0, 0)
        # a pair leaf has a node's length but a leaf's tag: the node over the same 64 bytes is another digest
        if lg == 1:
            two = GM.leaf_bytes(ints, 1)[0]
            assert levels[0][0] == hasher()(b"\x00" + two) != hasher()(b"\x01" + two)


def test_merkle_grouped_statuses():
    from zkmle_amd import _lib as L
    lib = zk.lib()
    root, el, path = np.zeros(32, np.uint8), np.zeros(24, np.uint64), np.zeros(64, np.uint8)
    ok = C.c_int(-1)
    ver = lambda field, depth, index, lg, r=root, e=el, okp=C.byref(ok): lib.zk_merkle_verify_grouped(field, p8(r), depth, index, lg, p64(e), p8(path), okp)
    assert ver(0, 1, 0, 3) == L.ZK_E_ARG and ver(1, 1, 0, 2) == L.ZK_E_ARG and ver(4, 1, 0, 2) == L.ZK_E_ARG
    assert ver(0, 1, 0, 2, r=None) == L.ZK_E_ARG and ver(0, 1, 0, 2, e=None) == L.ZK_E_ARG and ver(0, 1, 0, 2, okp=None) == L.ZK_E_ARG
    assert ver(0, 1, 2, 2) == L.ZK_E_RANGE and ver(0, 64, 0, 2) == L.ZK_E_RANGE
    assert ok.value == -1
    assert ver(0, 1, 1, 2) == 0 and ok.value == 0 and ver(2, 2, 3, 1) == 0 and ok.value == 0   # zeros are no path; the other 32-byte field
    # the device entries, as far as they go without a device: every argument error first, and nothing written
    h = {}
    for field, n in ((0, 1), (0, 2), (0, 4), (0, 6), (1, 8), (3, 2)):
        h[field, n] = C.c_void_p()
        L.check(lib.zk_table_wrap(field, C.c_void_p(0x1000), n, C.byref(h[field, n])))
    out = C.c_void_p()
    r = np.full(32, 0xA5, np.uint8)
    build = lambda t, lg, o=C.byref(out): lib.zk_merkle_build_grouped(t, lg, o)
    rootf = lambda t, lg, rr=r: lib.zk_mle_merkle_root_grouped(t, lg, p8(rr))
    for fn in (build, rootf):
        assert fn(h[0, 4], 3) == L.ZK_E_ARG                  # log_group = 3
        assert fn(h[1, 8], 2) == L.ZK_E_ARG and fn(h[1, 8], 1) == L.ZK_E_ARG   # a 48-byte field
        assert fn(h[0, 2], 2) == L.ZK_E_ARG and fn(h[0, 1], 1) == L.ZK_E_ARG and fn(h[3, 2], 2) == L.ZK_E_ARG   # len < 2^log_group
        assert fn(None, 2) == L.ZK_E_ARG
        assert fn(h[0, 6], 2) == L.ZK_E_NOT_POW2
    assert build(h[0, 4], 2, None) == L.ZK_E_ARG and rootf(h[0, 4], 2, None) == L.ZK_E_ARG
    import torch
    if not torch.cuda.is_available():
        assert build(h[0, 4], 2) == L.ZK_E_NO_DEVICE and rootf(h[0, 4], 1) == L.ZK_E_NO_DEVICE and build(h[0, 4], 0) == L.ZK_E_NO_DEVICE
    assert not out.value and (r == 0xA5).all()
    # the commitment: log_group outside {0, 2}, a null table, a null commitment
    cm = C.c_void_p()
    one = zk.from_ints(0, [1])[0]
    for lg in (1, 3, 1 << 31):
        assert lib.zk_fri_commit_grouped(h[0, 4], 1, None, lg, C.byref(cm)) == L.ZK_E_ARG, lg
    assert lib.zk_fri_commit_grouped(None, 1, None, 2, C.byref(cm)) == L.ZK_E_ARG and lib.zk_fri_commit_grouped(h[0, 4], 1, None, 2, None) == L.ZK_E_ARG
    assert lib.zk_fri_commit_grouped(h[0, 1], 1, None, 2, C.byref(cm)) == L.ZK_E_ARG and lib.zk_fri_commit_grouped(h[0, 4], 0, None, 2, C.byref(cm)) == L.ZK_E_ARG
    assert lib.zk_fri_commit_grouped(h[0, 6], 1, None, 2, C.byref(cm)) == L.ZK_E_NOT_POW2 and lib.zk_fri_commit_grouped(h[1, 8], 1, None, 2, C.byref(cm)) == L.ZK_E_RANGE
    assert lib.zk_fri_commit_grouped(h[0, 4], 1, p64(np.zeros(4, np.uint64)), 2, C.byref(cm)) == L.ZK_E_ARG
    if not torch.cuda.is_available():
        assert lib.zk_fri_commit_grouped(h[0, 4], 1, p64(one), 2, C.byref(cm)) == L.ZK_E_NO_DEVICE
    assert not cm.value and lib.zk_fri_commitment_log_group(None) == 0
    pts, ys, polys = np.zeros(8 * 64 * 4, np.uint64), np.full(8 * 4, 7, np.uint64), np.full(64 * 12, 7, np.uint64)
    roots, fin, vals, paths = np.full(64 * 32, 7, np.uint8), np.full(4 << 10, 7, np.uint64), np.full(1 << 12, 7, np.uint64), np.full(1 << 12, 7, np.uint8)
    assert lib.zk_fri_ml_open_points_grouped(None, p64(pts), 2, 0, 4, None, p64(ys), None, p64(polys), p8(roots), p64(fin), None, None, p64(vals),
                                             p8(paths)) == L.ZK_E_ARG
    assert all((a == 7).all() for a in (ys, polys, roots, fin, vals, paths))
    for t in h.values():
        lib.zk_table_free(t)


# ---- the opening --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coeffs_of(field, d, b, with_coset):
    coset = random.Random(43 * d + b + field).randrange(2, NM.MODULUS[field]) if with_coset else 1
    return tuple(NM.random_ints(field, 1 << d, 7300 + 13 * d + field)), coset


@functools.lru_cache(maxsize=None)
def commitment(field, d, b, with_coset):
    coeffs, coset = coeffs_of(field, d, b, with_coset)
    return GM.commit(field, list(coeffs), b, coset, hasher())


def points_for(field, d, P):
    return FC.points_for(field, d, P, 101 * d + 7 * P + field)


@functools.lru_cache(maxsize=None)
def opening(case):
    field, d, b, f, P, with_coset = case
    return GM.open_points(commitment(field, d, b, with_coset), points_for(field, d, P), f, Q, hasher=hasher())


def lib_verify(op, fl=None, tr=None, **over):
    """zk_fri_ml_verify_points_grouped on the model's opening `op` (flat arrays `fl`) -> (status, ok)"""
    fl = GM.flat(zk, op) if fl is None else fl
    s = {n: op[n] for n in ("d", "b", "f", "Q")}
    s.update({n: v for n, v in over.items() if n in s})
    coset = over.get("coset", op["coset"])
    cm = None if coset is None else zk.from_ints(op["field"], [coset])[0]
    ok = C.c_int(-1)
    rc = zk.lib().zk_fri_ml_verify_points_grouped(op["field"], p8(fl["root"]), s["d"], s["b"], s["f"], s["Q"], p64(cm), p64(fl["points"]), len(op["points"]),
                                                  p64(fl["ys"]), None if tr is None else tr._h, p64(fl["polys"]), p8(fl["roots"]), p64(fl["final"]),
                                                  p64(fl["values"]), p8(fl["paths"]), C.byref(ok))
    return rc, ok.value


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_model_openings_pass_the_model_verifier_and_the_library_verifier(case):
    field, d, b, f, P, with_coset = case
    op = opening(case)
    assert op["ys"] == [ML.mle_evaluate(field, commitment(field, d, b, with_coset)["coeffs"], z) for z in op["points"]]
    assert GM.verify(op, hasher=hasher())
    fl = GM.flat(zk, op)
    assert lib_verify(op, fl) == (0, 1)
    if not with_coset:
        assert lib_verify(op, fl, coset=None) == (0, 1)
    assert GM.sizes(d, b, f, Q) == (fl["roots"].shape[0], fl["final"].shape[0], fl["values"].size // 4, fl["paths"].size, fl["polys"].size // 4)
    # the Python wrapper
    cs = zk.from_ints(field, [op["coset"]])[0]
    o = zk.fri.FriMlPointsOpening(field, P, d, b, f, Q, coset=cs, log_arity=2, grouped=True)
    assert o.roots.shape == fl["roots"].shape and o.query_values.shape == fl["values"].shape and o.query_paths.shape == fl["paths"].shape
    o.ys, o.round_polys, o.roots, o.final_table, o.query_values, o.query_paths = fl["ys"], fl["polys"], fl["roots"], fl["final"], fl["values"], fl["paths"]
    assert zk.fri.verify_multilinear_points(op["root"], fl["points"], o)
    assert not zk.fri.verify_multilinear_points(op["root"][::-1], fl["points"], o)


TAMPER_CASES = [CASES[3], CASES[5], CASES[8]]                # R = 4, 5 and 9: fold-4 steps alone, and with the final fold-2 step


def spots_of(kind, op, base, rng):
    d, b, f = op["d"], op["b"], op["f"]
    L, R = d + b, d - f
    if kind == "value":                                       # every side of every step's group, at query 1
        return [("values", (1, k, rng.randrange(4))) for k in range(base["values"].shape[1])]
    if kind == "path":                                        # the first and the last digest of every step's path, at query 2
        out, poff, per_query = [], 0, base["paths"].size // Q
        for l, sides in GM.steps(L, R):
            n = L - l - (sides.bit_length() - 1)
            out += [("paths", (2 * per_query + poff + rng.randrange(32),)), ("paths", (2 * per_query + poff + 32 * (n - 1) + rng.randrange(32),))]
            poff += 32 * n
        assert poff == per_query
        return out
    if kind == "root":
        return [("roots", (s, rng.randrange(32))) for s in range(len(op["roots"]))]
    if kind == "round":
        return [("polys", (l, k, rng.randrange(4))) for l in range(R) for k in range(3)]
    if kind == "final":
        return [("final", (j, rng.randrange(4))) for j in range(1 << f)]
    return [("ys", (k, rng.randrange(4))) for k in range(len(op["ys"]))]


@pytest.mark.parametrize("kind", ("value", "path", "root", "round", "final", "y"))
def test_a_tampered_opening_is_rejected(kind):
    for case in TAMPER_CASES:
        op = opening(case)
        base = GM.flat(zk, op)
        rng = random.Random(913 + case[1] + case[0] + len(kind))
        spots = spots_of(kind, op, base, rng)
        assert spots
        for name, at in spots:
            assert lib_verify(op, tampered(base, name, at, rng)) == (0, 0), (case, name, at)
    if kind == "value":                                       # the same residue, not reduced: x + p < 2^256
        p = NM.MODULUS[op["field"]]
        for at in ((3, 0), (0, base["values"].shape[1] - 1)):
            fl = {n: v.copy() for n, v in base.items()}
            fl["values"][at] = np.frombuffer((int.from_bytes(fl["values"][at].tobytes(), "little") + p).to_bytes(32, "little"), np.uint64)
            assert lib_verify(op, fl) == (0, 0), at


@pytest.mark.parametrize("case", [CASES[1], CASES[5], CASES[7]], ids=case_id)
def test_the_ungrouped_opening_is_no_grouped_one_and_the_reverse(case):
    """the same table, points and parameters under the fold-by-4 protocol of tests/_fri_ml_arity_model.py and under this one"""
    field, d, b, f, P, with_coset = case
    coeffs, coset = coeffs_of(field, d, b, with_coset)
    pts = points_for(field, d, P)
    plain = AM.open_points(PM.commit(field, list(coeffs), b, coset, hasher()), pts, f, Q, hasher=hasher())
    grouped = opening(case)
    assert AM.verify(plain, hasher=hasher()) and plain["ys"] == grouped["ys"] and plain["root"] != grouped["root"]
    cs = zk.from_ints(field, [coset])[0]
    for op, flat_, is_grouped in ((plain, AM.flat(zk, plain), False), (grouped, GM.flat(zk, grouped), True)):
        big = padded(flat_)
        for as_grouped in (False, True):
            o = zk.fri.FriMlPointsOpening(field, P, d, b, f, Q, coset=cs, log_arity=2, grouped=as_grouped)
            o.ys, o.round_polys, o.roots, o.final_table, o.query_values, o.query_paths = (
                flat_["ys"], flat_["polys"], flat_["roots"], flat_["final"], big["values"], big["paths"])
            assert zk.fri.verify_multilinear_points(op["root"], flat_["points"], o) == (as_grouped == is_grouped), (is_grouped, as_grouped)
    assert lib_verify(plain, padded(AM.flat(zk, plain))) == (0, 0)


def test_a_callers_transcript_ends_in_the_models_state():
    from oracle import pymodel as M
    prior = b"what the caller had absorbed before"
    cm = commitment(3, 4, 1, True)
    mt = M.Transcript()
    mt.append(prior)
    op = GM.open_points(cm, points_for(3, 4, 2), 1, Q, mt, hasher=hasher())
    vt = M.Transcript()
    vt.append(prior)
    assert GM.verify(op, vt, hasher()) and vt.buf == mt.buf
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

    def sizes(d, b, f, q):
        out = [C.c_size_t(0) for _ in range(5)]
        rc = lib.zk_fri_ml_sizes_grouped(d, b, f, q, *[C.byref(o) for o in out])
        return rc, tuple(int(o.value) for o in out)

    for d in (3, 4, 6, 10, 24):
        for b in (1, 2, 3):
            for f in range(0, d - 1):
                for q in (1, 8, 64):
                    L_, R = d + b, d - f
                    want = ((R + 1) // 2, 1 << f, q * (4 * (R // 2) + 2 * (R % 2)),
                            32 * q * (sum(L_ - l - 2 for l in range(0, R - 1, 2)) + (L_ - (R - 1) - 1 if R % 2 else 0)), 3 * R)
                    assert sizes(d, b, f, q) == (0, want) and GM.sizes(d, b, f, q) == want, (d, b, f, q)
                    assert zk.fri.ml_sizes(d, b, f, q, log_arity=2, grouped=True) == want
                    assert want[3] < ML.sizes(d, b, f, q)[3] and want[3] < AM.sizes(d, b, f, q)[3]   # smaller than arity 1's, R >= 2
    assert sizes(24, 2, 6, 1)[1][3] == 144 * 32 and ML.sizes(24, 2, 6, 1)[3] == 630 * 32 and AM.sizes(24, 2, 6, 1)[3] == 648 * 32
    assert sizes(4, 1, 3, 8)[0] == L.ZK_E_ARG and sizes(4, 1, 4, 8)[0] == L.ZK_E_ARG and sizes(40, 1, 0, 8)[0] == L.ZK_E_RANGE   # R = 1, R = 0
    assert sizes(4, 0, 0, 8)[0] == L.ZK_E_ARG and sizes(4, 1, 0, 0)[0] == L.ZK_E_ARG
    assert lib.zk_fri_ml_sizes_grouped(4, 1, 0, 8, None, None, None, None, None) == 0
    with pytest.raises(ValueError):
        zk.fri.ml_sizes(4, 1, 0, 8, log_arity=1, grouped=True)


def test_verifier_statuses():
    from zkmle_amd import _lib as L
    lib = zk.lib()
    roots, fin, vals, paths = np.zeros(64 * 32, np.uint8), np.zeros(4 << 10, np.uint64), np.zeros(1 << 16, np.uint64), np.zeros(1 << 20, np.uint8)
    root, pts, ys, polys = np.zeros(32, np.uint8), np.zeros(8 * 64 * 4, np.uint64), np.zeros(8 * 4, np.uint64), np.zeros(64 * 12, np.uint64)
    ok = C.c_int(-1)
    for field in (0, 1, 2, 3):
        ver = lambda d, b, f, q, P=2, okp=C.byref(ok): lib.zk_fri_ml_verify_points_grouped(
            field, p8(root), d, b, f, q, None, p64(pts), P, p64(ys), None, p64(polys), p8(roots), p64(fin), p64(vals), p8(paths), okp)
        assert ver(3, 1, 2, 4) == L.ZK_E_ARG                                                # R = 1
        assert ver(3, 1, 0, 4, okp=None) == L.ZK_E_ARG and ver(3, 1, 0, 4, P=0) == L.ZK_E_ARG and ver(3, 1, 0, 4, P=9) == L.ZK_E_ARG
        for d, b, f, q in ((3, 0, 0, 4), (3, 9, 0, 4), (3, 1, 0, 0), (3, 1, 0, 4097), (3, 1, 3, 4), (0, 1, 0, 4), (40, 1, 40, 4), (40, 1, 39, 4)):
            assert ver(d, b, f, q) == L.ZK_E_ARG, (d, b, f, q)
        if field in (1, 2):
            assert ver(3, 1, 0, 4) == L.ZK_E_RANGE
        else:
            assert ver(NM.two_adicity(field), 1, 0, 4) == L.ZK_E_RANGE and ver(40, 1, 0, 4) == L.ZK_E_RANGE
            assert ver(3, 1, 0, 4) == 0 and ok.value == 0                                   # zeros are no proof
