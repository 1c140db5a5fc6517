"""CPU: the host side of the FRI low-degree proof (include/zkmle.h "FRI low-degree proof").  The Python model of tests/_fri_model.py is
checked against itself (a fold of the extension is the extension of the folded coefficients; its proofs pass its verifier); the library's
HOST verifier zk_fri_verify accepts the model's proofs over a grid of shapes, rejects every single-bit change and every parameter that
differs from the prover's, and leaves a caller's transcript in the model's state; the counts and the precondition codes are the header's,
all before the device check."""
import ctypes as C
import random

import numpy as np
import pytest

import __graft_entry__ as G
import _fri_model as FM
import _ntt_model as NM
from oracle import pymodel as M

zk = G.import_package()
P64, P8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
p64 = lambda a: a.ctypes.data_as(P64) if a is not None else None
p8 = lambda a: a.ctypes.data_as(P8) if a is not None else None
NEW_NAMES = ("zk_fri_fold", "zk_fri_proof_sizes", "zk_fri_prove", "zk_fri_prove_codeword", "zk_fri_verify", "zk_fri_last_stats")
# (field, d, b, f, Q, coset given): f = 0, f = d - 1, b = 1 and the NULL coset are among them
GRID = [(0, 1, 1, 0, 3, False), (0, 2, 1, 1, 4, True), (0, 3, 2, 0, 5, True), (0, 4, 1, 3, 6, False), (0, 5, 2, 2, 7, True),
        (0, 6, 3, 1, 4, False), (3, 1, 2, 0, 2, True), (3, 3, 1, 2, 5, False), (3, 4, 3, 0, 6, True), (3, 5, 1, 1, 3, True)]


def test_new_exports_are_present():
    lib = zk.lib()
    header = open(G.ROOT + "/include/zkmle.h").read()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in header, name
    assert "zk_fri_stats;" in header
    for name in ("fold", "prove", "prove_codeword", "verify", "sizes", "last_stats", "FriProof"):
        assert callable(getattr(zk.fri, name)), name
    assert zk.FriProof is zk.fri.FriProof


def model_proof(field, d, b, f, Q, with_coset, seed=0, tr=None):
    p = NM.MODULUS[field]
    coeffs = NM.random_ints(field, 1 << d, 900 + 17 * d + field + seed)
    coset = random.Random(d * 8 + b + seed).randrange(2, p) if with_coset else 1
    return FM.prove(field, coeffs, b, f, Q, coset, tr)


def lib_verify(pr, fl=None, tr=None, **over):
    """zk_fri_verify on the model's proof `pr` (flat arrays `fl`), parameters overridable -> (status, ok)"""
    fl = FM.flat(zk, pr) if fl is None else fl
    a = {k: pr[k] for k in ("d", "b", "f", "Q")}
    a.update({k: v for k, v in over.items() if k in a})
    coset = over.get("coset", pr["coset"])
    cm = None if coset is None else zk.from_ints(pr["field"], [coset])[0]
    ok = C.c_int(-1)
    rc = zk.lib().zk_fri_verify(pr["field"], a["d"], a["b"], a["f"], a["Q"], p64(cm), None if tr is None else tr._h, p8(fl["roots"]),
                                p64(fl["final"]), p64(fl["values"]), p8(fl["paths"]), C.byref(ok))
    return rc, ok.value


@pytest.mark.parametrize("field", [0, 3])
def test_model_fold_of_the_extension_is_the_extension_of_the_folded_coefficients(field):
    p = NM.MODULUS[field]
    for d in range(1, 9):
        for b in (1, 2):
            a = NM.random_ints(field, 1 << d, 40 * field + d)
            rng = random.Random(100 * d + b + field)
            beta, c = rng.randrange(p), rng.randrange(2, p)
            for coset in (1, c):
                folded = [(a[2 * i] + beta * a[2 * i + 1]) % p for i in range(1 << (d - 1))]
                assert FM.fold(field, FM.extend(field, a, b, coset), beta, coset) == FM.extend(field, folded, b, coset * coset % p), (d, b, coset != 1)


@pytest.mark.parametrize("case", GRID)
def test_model_proof_passes_the_model_verifier_and_the_library_verifier(case):
    pr = model_proof(*case)
    assert FM.verify(pr)
    assert len(pr["roots"]) == pr["d"] - pr["f"] and len(pr["final"]) == 1 << pr["f"]
    fl = FM.flat(zk, pr)
    assert lib_verify(pr, fl) == (0, 1), case
    if not case[5]:                                                  # NULL and the element 1 are the same coset
        assert lib_verify(pr, fl, coset=None) == (0, 1)
    assert zk.fri.sizes(*case[1:5]) == FM.sizes(*case[1:5]) == (fl["roots"].shape[0], fl["final"].shape[0], fl["values"].size // 4, fl["paths"].size)
    proof = zk.FriProof(case[0], *case[1:5], coset=zk.from_ints(case[0], [pr["coset"]])[0])
    proof.roots, proof.final_coeffs, proof.query_values, proof.query_paths = fl["roots"], fl["final"], fl["values"], fl["paths"]
    assert zk.fri.verify(proof) and proof.sizes == FM.sizes(*case[1:5])


def test_every_single_bit_change_is_rejected():
    pr = model_proof(0, 4, 2, 1, 6, True)
    L, R = 6, 3
    base = FM.flat(zk, pr)
    assert lib_verify(pr, base) == (0, 1)
    rng = random.Random(4216)
    per_query = base["paths"].size // 6
    spots = []
    for l in range(R):
        spots.append(("roots", (l, rng.randrange(32))))
    for j in range(2):
        spots.append(("final", (j, rng.randrange(4))))
    for q in (0, 5):
        for l in range(R):
            spots.append(("values", (q, l, 0, rng.randrange(4))))                     # a low value
            spots.append(("values", (q, l, 1, rng.randrange(4))))                     # a high value
    off = 0
    for l in range(R):                                                              # query 2: first and last digest of both paths of every layer
        for side in range(2):
            spots.append(("paths", (2 * per_query + off + rng.randrange(32),)))
            spots.append(("paths", (2 * per_query + off + 32 * (L - l - 1) + rng.randrange(32),)))
            off += 32 * (L - l)
    assert off == per_query
    for name, at in spots:
        fl = {k: v.copy() for k, v in base.items()}
        bits = 8 if fl[name].dtype == np.uint8 else 64
        fl[name][at] ^= fl[name].dtype.type(1 << rng.randrange(bits))
        assert lib_verify(pr, fl) == (0, 0), (name, at)
    fl = {k: v.copy() for k, v in base.items()}                                     # the same residue, not reduced: x + p < 2^256
    fl["final"][0] = np.frombuffer((int.from_bytes(fl["final"][0].tobytes(), "little") + NM.MODULUS[0]).to_bytes(32, "little"), np.uint64)
    assert lib_verify(pr, fl) == (0, 0)


def test_a_verifier_with_other_parameters_rejects():
    pr = model_proof(0, 4, 2, 1, 6, True)
    fl = FM.flat(zk, pr)
    big = {k: np.concatenate([v.reshape(-1), np.zeros(4 * v.size + 4096, v.dtype)]) for k, v in fl.items()}   # room for any shape below
    assert lib_verify(pr, big) == (0, 1)
    for over in ({"Q": 5}, {"Q": 7}, {"f": 0}, {"f": 2}, {"coset": 1}, {"coset": None}, {"coset": pr["coset"] + 1}, {"b": 1}, {"d": 5}):
        assert lib_verify(pr, big, **over) == (0, 0), over


def test_a_callers_transcript_ends_in_the_models_state():
    prior = b"what the caller had absorbed before"
    for case in (GRID[2], GRID[8]):
        mt = M.Transcript()
        mt.append(prior)
        pr = model_proof(*case, tr=mt)
        vt = M.Transcript()
        vt.append(prior)
        assert FM.verify(pr, vt) and vt.buf == mt.buf
        t = zk.Transcript()
        t.append(prior)
        assert lib_verify(pr, tr=t) == (0, 1)
        want = zk.Transcript()
        want.append(bytes(mt.buf))
        assert np.array_equal(t.export_state(), want.export_state())
        assert lib_verify(pr) == (0, 0)                               # the proof is bound to the prior content


def test_proof_sizes():
    from zkmle_amd import _lib as L
    lib = zk.lib()
    out = [C.c_size_t(0) for _ in range(4)]
    for d, b, f, Q in [(1, 1, 0, 1), (5, 2, 2, 7), (11, 2, 6, 40), (22, 2, 6, 64), (24, 8, 23, 4096), (31, 1, 0, 1)]:
        assert lib.zk_fri_proof_sizes(d, b, f, Q, *[C.byref(o) for o in out]) == 0
        assert tuple(o.value for o in out) == FM.sizes(d, b, f, Q)
    assert lib.zk_fri_proof_sizes(5, 2, 2, 7, None, None, None, None) == 0
    for bad in [(5, 0, 2, 7), (5, 9, 2, 7), (5, 2, 5, 7), (5, 2, 2, 0), (5, 2, 2, 4097), (0, 2, 0, 7)]:
        assert lib.zk_fri_proof_sizes(*bad, *[C.byref(o) for o in out]) == L.ZK_E_ARG, bad
    assert lib.zk_fri_proof_sizes(31, 2, 0, 1, *[C.byref(o) for o in out]) == L.ZK_E_RANGE
    assert lib.zk_fri_proof_sizes(40, 9, 0, 1, *[C.byref(o) for o in out]) == L.ZK_E_ARG       # ZK_E_ARG comes first


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
    for field in (0, 1, 2, 3):
        nl = zk.limbs(field)
        zero, one = np.zeros(nl, np.uint64), zk.from_ints(field, [1])[0]
        for fn in (lib.zk_fri_prove, lib.zk_fri_prove_codeword):
            is_cw = fn is lib.zk_fri_prove_codeword
            call = lambda t, b, f, Q, coset, r=roots: fn(t, b, f, Q, p64(coset), None, p8(r), p64(fin), None, None, p64(vals), p8(paths))
            t8, t6, t64 = wrapped(field, 8), wrapped(field, 6), wrapped(field, 64)
            assert call(None, 1, 0, 4, None) == L.ZK_E_ARG
            assert call(t8, 1, 0, 4, None, None) == L.ZK_E_ARG                         # no room for the roots
            for b, Q in ((0, 4), (9, 4), (1, 0), (1, 4097)):
                assert call(t8, b, 0, Q, None) == L.ZK_E_ARG and call(t6, b, 0, Q, None) == L.ZK_E_ARG
            assert call(t8, 1, 0, 4, zero) == L.ZK_E_ARG and call(t6, 1, 0, 4, zero) == L.ZK_E_ARG
            assert call(t6, 1, 0, 4, None) == L.ZK_E_NOT_POW2 and call(t6, 1, 0, 4, one) == L.ZK_E_NOT_POW2
            assert call(t8, 1, 3, 4, None) == L.ZK_E_ARG                               # f >= d, whatever the field
            if is_cw:
                assert call(t8, 3, 0, 4, None) == L.ZK_E_ARG and call(t8, 4, 0, 4, None) == L.ZK_E_ARG   # no longer than the blow-up
            if field in (1, 2):
                assert call(t8, 1, 0, 4, None) == L.ZK_E_RANGE and call(t64, 2, 1, 4, one) == L.ZK_E_RANGE
            else:
                s = NM.two_adicity(field)
                big = wrapped(field, 1 << (s + 1 if is_cw else s - 1))              # d + b = s + 1
                assert call(big, 2, 0, 4, None) == L.ZK_E_RANGE and call(big, 2, 0, 4, one) == L.ZK_E_RANGE
                lib.zk_table_free(big)
                if not have_gpu:
                    assert call(t8, 1, 0, 4, None) == L.ZK_E_NO_DEVICE and call(t64, 2, 1, 4, one) == L.ZK_E_NO_DEVICE
            for h in (t8, t6, t64):
                lib.zk_table_free(h)
        # the fold
        out = C.c_void_p()
        t1, t2, t6, t8 = (wrapped(field, n) for n in (1, 2, 6, 8))
        fold = lambda t, beta, coset, o=C.byref(out): lib.zk_fri_fold(t, p64(beta), p64(coset), o)
        assert fold(None, one, None) == L.ZK_E_ARG and fold(t8, None, None) == L.ZK_E_ARG and fold(t8, one, None, None) == L.ZK_E_ARG
        assert fold(t1, one, None) == L.ZK_E_ARG and fold(t8, one, zero) == L.ZK_E_ARG and fold(t6, one, zero) == L.ZK_E_ARG
        assert fold(t6, one, None) == L.ZK_E_NOT_POW2
        if field in (1, 2):
            assert fold(t8, one, None) == L.ZK_E_RANGE and fold(t2, one, one) == L.ZK_E_RANGE
        elif not have_gpu:
            assert fold(t8, one, None) == L.ZK_E_NO_DEVICE and fold(t2, one, one) == L.ZK_E_NO_DEVICE
        # the verifier: host code, the same order without a device check
        ok = C.c_int(-1)
        ver = lambda d, b, f, Q, coset, okp=C.byref(ok): lib.zk_fri_verify(field, d, b, f, Q, p64(coset), None, p8(roots), p64(fin), p64(vals), p8(paths), okp)
        assert ver(3, 1, 0, 4, None, None) == L.ZK_E_ARG
        for d, b, f, Q in ((3, 0, 0, 4), (3, 9, 0, 4), (3, 1, 0, 0), (3, 1, 0, 4097), (3, 1, 3, 4), (0, 1, 0, 4), (40, 1, 40, 4)):
            assert ver(d, b, f, Q, None) == L.ZK_E_ARG, (d, b, f, Q)
        assert ver(3, 1, 0, 4, zero) == L.ZK_E_ARG
        if field in (1, 2):
            assert ver(3, 1, 0, 4, None) == L.ZK_E_RANGE and ver(1, 1, 0, 1, one) == L.ZK_E_RANGE
        else:
            s = NM.two_adicity(field)
            assert ver(s, 1, 0, 4, None) == L.ZK_E_RANGE and ver(40, 1, 0, 4, None) == L.ZK_E_RANGE
            assert ver(3, 1, 0, 4, None) == 0 and ok.value == 0                        # zeros are no proof
    assert lib.zk_fri_verify(7, 3, 1, 0, 4, None, None, p8(roots), p64(fin), p64(vals), p8(paths), C.byref(C.c_int())) == L.ZK_E_ARG
    assert lib.zk_fri_last_stats(None) == L.ZK_E_ARG
