"""Host side of the batched multilinear-KZG opening (include/zkmle.h zk_kzg_batch_verify; extension: no reference counterpart): a proof
built by the big-int model (oracle/pymodel.py: gamma from the transcript model, open_and_prove of sum_j gamma^j f_j) is accepted, tampered
ones are rejected, the caller's transcript ends where the model's does, and the argument codes of the verifier and of the prover / the
k-table combination come before any device or transcript use.  Runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import pairing_model as M
from oracle import pymodel as PM

zkp = G.import_package()
from zkmle_amd import _lib as L   # noqa: E402

RQ = 1 << 384
R = PM.R


def lib():
    lb = L.lib()
    if not getattr(lb, "_kzg_batch_declared", False):
        u64p, vp, sz = L.u64p, L.vp, C.c_size_t
        lb.zk_kzg_setup_g2.argtypes = [u64p, sz, u64p]
        lb.zk_kzg_batch_verify.argtypes = [u64p, sz, u64p, sz, u64p, u64p, sz, u64p, sz, vp, C.POINTER(C.c_int)]
        lb.zk_kzg_batch_open.argtypes = [C.POINTER(vp), sz, u64p, vp, vp, u64p, sz, sz, vp, u64p, u64p, u64p]
        lb.zk_transcript_new.argtypes = [C.POINTER(vp)]
        lb.zk_transcript_free.argtypes = [vp]
        lb.zk_transcript_append.argtypes = [vp, L.u8p, sz]
        lb.zk_transcript_sample.argtypes = [vp, L.u8p]
        lb._kzg_batch_declared = True
    return lb


def fq_limbs(v):
    v = v * RQ % M.P
    return [(v >> (64 * i)) & ((1 << 64) - 1) for i in range(6)]


def g1_arr(p):
    return np.array(([0] * 12) if p is None else fq_limbs(p[0]) + fq_limbs(p[1]), np.uint64)


def fr_arr(k):
    v = k % R * (1 << 256) % R
    return np.array([(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)], np.uint64)


def model_gamma(t, commitments, point, evals):
    """the transcript schedule of zk_kzg_batch_open: x || y of every commitment (48-byte big-endian, infinity = 96 zero bytes), the
    point and the evaluations (32-byte big-endian), then gamma = the next sample mod r"""
    for c in commitments:
        t.append(bytes(96) if c is None else PM.be32(c[0], 48) + PM.be32(c[1], 48))
    for x in list(point) + list(evals):
        t.append(PM.be32(x))
    return t.challenge(R)


def model_batch_proof(n, k, seed):
    rng = np.random.default_rng(seed)
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % R
    taus = [rnd() for _ in range(n)]
    polys = [[rnd() for _ in range(1 << n)] for _ in range(k)]
    point = [rnd() for _ in range(n)]
    pts = PM.kzg_setup_g1(taus)
    commitments = [PM.kzg_commit(f, pts) for f in polys]
    evals = [PM.evaluate(f, point, R) for f in polys]
    t = PM.Transcript()
    gamma = model_gamma(t, commitments, point, evals)
    g = [sum(pow(gamma, j, R) * f[i] for j, f in enumerate(polys)) % R for i in range(1 << n)]
    v, proofs = PM.kzg_open(g, pts, point)
    assert v == sum(pow(gamma, j, R) * e for j, e in enumerate(evals)) % R
    g2p = np.zeros((n, 24), np.uint64)
    L.check(lib().zk_kzg_setup_g2(L.p64(np.stack([fr_arr(x) for x in taus])), n, L.p64(g2p)))
    return dict(commitments=commitments, point=point, evals=evals, proofs=proofs, g2=g2p, model=t)


class Transcript:
    def __init__(self):
        self.h = C.c_void_p()
        L.check(lib().zk_transcript_new(C.byref(self.h)))

    def append(self, data):
        buf = np.frombuffer(bytes(data), np.uint8).copy()
        L.check(lib().zk_transcript_append(self.h, L.p8(buf), len(buf)))

    def sample(self):
        out = np.zeros(32, np.uint8)
        L.check(lib().zk_transcript_sample(self.h, L.p8(out)))
        return out.tobytes()

    def __del__(self):
        lib().zk_transcript_free(self.h)


def batch_verify(commitments, point, evals, proofs, g2, ng2=None, t=None, k=None):
    ok = C.c_int(-1)
    cs = np.stack([g1_arr(c) for c in commitments]) if commitments else np.zeros((1, 12), np.uint64)
    pt = np.stack([fr_arr(x) for x in point]) if point else np.zeros((1, 4), np.uint64)
    ev = np.stack([fr_arr(x) for x in evals]) if evals else np.zeros((1, 4), np.uint64)
    prs = np.stack([g1_arr(p) for p in proofs]) if proofs else np.zeros((1, 12), np.uint64)
    rc = lib().zk_kzg_batch_verify(L.p64(cs), len(commitments) if k is None else k, L.p64(pt), len(point), L.p64(ev), L.p64(prs),
                                   len(proofs), L.p64(g2), g2.shape[0] if ng2 is None else ng2, t.h if t is not None else None,
                                   C.byref(ok))
    return rc if rc != 0 else ok.value


@pytest.mark.parametrize("n,k", [(1, 1), (1, 3), (2, 2), (3, 1), (3, 3), (2, 1), (1, 2), (2, 3), (3, 2)])
def test_batch_verify_accepts_the_model_proof_and_rejects_tampering(n, k):
    d = model_batch_proof(n, k, 100 * n + k)
    args = (d["commitments"], d["point"], d["evals"], d["proofs"], d["g2"])
    assert batch_verify(*args) == 1
    bad = list(d["evals"])
    bad[-1] = (bad[-1] + 1) % R                                           # a changed evaluation
    assert batch_verify(d["commitments"], d["point"], bad, d["proofs"], d["g2"]) == 0
    cs = list(d["commitments"])
    cs[-1] = PM.g1_add(cs[-1], PM.G1)                                     # a changed commitment
    assert batch_verify(cs, d["point"], d["evals"], d["proofs"], d["g2"]) == 0
    if k >= 2:                                                            # two commitments swapped
        cs = list(d["commitments"])
        cs[0], cs[1] = cs[1], cs[0]
        assert batch_verify(cs, d["point"], d["evals"], d["proofs"], d["g2"]) == 0
    prs = list(d["proofs"])
    prs[0] = PM.g1_add(prs[0], PM.G1)                                     # a changed proof point
    assert batch_verify(d["commitments"], d["point"], d["evals"], prs, d["g2"]) == 0
    pt = list(d["point"])
    pt[-1] = (pt[-1] + 1) % R                                             # a changed opening point
    assert batch_verify(d["commitments"], pt, d["evals"], d["proofs"], d["g2"]) == 0
    t = Transcript()
    t.append(b"\x00")                                                     # a transcript that absorbed one extra byte first: another
    assert batch_verify(*args, t=t) == (1 if k == 1 else 0)               # gamma (at k = 1, g = f_0 whatever gamma is)


@pytest.mark.parametrize("n,k", [(2, 3), (3, 2)])
def test_batch_verify_leaves_the_callers_transcript_where_the_model_is(n, k):
    d = model_batch_proof(n, k, 7 * n + k)
    prefix = b"earlier proof bytes"
    t = Transcript()
    t.append(prefix)
    model = PM.Transcript()
    model.append(prefix)
    model_gamma(model, d["commitments"], d["point"], d["evals"])
    # the same proof is valid only for the transcript it was made on: rebuild it on the prefixed one
    gamma_ok = batch_verify(d["commitments"], d["point"], d["evals"], d["proofs"], d["g2"], t=t)
    assert gamma_ok == 0                                                  # gamma differs from the fresh transcript's
    assert t.sample() == model.sample()                                   # ... and the transcript has moved as the model's did
    fresh = Transcript()
    assert batch_verify(d["commitments"], d["point"], d["evals"], d["proofs"], d["g2"], t=fresh) == 1
    assert fresh.sample() == d["model"].sample()


def test_batch_verify_with_a_commitment_at_infinity():
    """a zero polynomial commits to the point at infinity, which the transcript absorbs as 96 zero bytes"""
    n, k = 2, 2
    rng = np.random.default_rng(5)
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % R
    taus, point = [rnd() for _ in range(n)], [rnd() for _ in range(n)]
    polys = [[0] * (1 << n), [rnd() for _ in range(1 << n)]]
    pts = PM.kzg_setup_g1(taus)
    commitments = [PM.kzg_commit(f, pts) for f in polys]
    assert commitments[0] is None
    evals = [PM.evaluate(f, point, R) for f in polys]
    gamma = model_gamma(PM.Transcript(), commitments, point, evals)
    g = [sum(pow(gamma, j, R) * f[i] for j, f in enumerate(polys)) % R for i in range(1 << n)]
    _, proofs = PM.kzg_open(g, pts, point)
    g2p = np.zeros((n, 24), np.uint64)
    L.check(lib().zk_kzg_setup_g2(L.p64(np.stack([fr_arr(x) for x in taus])), n, L.p64(g2p)))
    assert batch_verify(commitments, point, evals, proofs, g2p) == 1


def test_batch_verify_length_and_argument_codes():
    d = model_batch_proof(2, 2, 77)
    args = (d["commitments"], d["point"], d["evals"], d["proofs"], d["g2"])
    assert batch_verify(*args, k=0) == L.ZK_E_ARG                         # k = 0
    assert batch_verify(d["commitments"], d["point"], d["evals"], d["proofs"][:1], d["g2"], ng2=1) == L.ZK_E_KZG_LEN   # nopen != nproofs
    assert batch_verify(*args, ng2=3) == L.ZK_E_KZG_LEN                   # ng2 > nproofs
    # a refused call leaves the transcript untouched
    t = Transcript()
    assert batch_verify(*args, ng2=3, t=t) == L.ZK_E_KZG_LEN
    assert t.sample() == PM.Transcript().sample()


def wrapped(field, length, addr):
    """a non-owning handle over a made-up device address: the argument checks never dereference it"""
    h = C.c_void_p()
    L.check(L.lib().zk_table_wrap(field, C.c_void_p(addr), length, C.byref(h)))
    return h


def test_combination_and_batch_open_codes_come_before_the_device():
    lb = lib()
    a, b, c = wrapped(0, 8, 0x10000), wrapped(0, 8, 0x20000), wrapped(0, 4, 0x30000)
    q, out = wrapped(1, 8, 0x40000), wrapped(0, 8, 0x50000)
    coeffs = np.zeros((65, 6), np.uint64)

    def comb(tabs, outh, k=None):
        arr = (L.vp * max(len(tabs), 1))(*[t.value for t in tabs])
        return lb.zk_mle_linear_combination(arr, len(tabs) if k is None else k, L.p64(coeffs), outh, None)

    assert comb([a, b], out, k=0) == L.ZK_E_ARG                           # k = 0
    assert comb([a] * 65, out) == L.ZK_E_ARG                              # k > 64
    assert comb([a, q], out) == L.ZK_E_ARG                                # mixed fields
    assert comb([a, c], out) == L.ZK_E_NVARS                              # unequal lengths
    assert comb([a, b], a) == L.ZK_E_ARG                                  # out aliases an input
    assert comb([a, b], wrapped(0, 8, 0x20000 + 32)) == L.ZK_E_ARG        # ... or overlaps one
    assert comb([a, b], c) == L.ZK_E_ARG                                  # out too short

    key = None
    cs, pt, ev, gm, pr = (np.zeros((4, 12), np.uint64), np.zeros((3, 4), np.uint64), np.zeros((4, 4), np.uint64),
                          np.zeros(4, np.uint64), np.zeros((3, 12), np.uint64))
    bases = C.c_void_p(0x1234)                                            # never dereferenced before the table checks fail

    def bopen(tabs, nopen=3, n_g2=3, k=None):
        arr = (L.vp * max(len(tabs), 1))(*[t.value for t in tabs])
        return lb.zk_kzg_batch_open(arr, len(tabs) if k is None else k, L.p64(cs), bases, key, L.p64(pt), nopen, n_g2, None,
                                    L.p64(ev), L.p64(gm), L.p64(pr))

    assert bopen([a, b], k=0) == L.ZK_E_ARG
    assert bopen([a] * 65) == L.ZK_E_ARG
    assert bopen([a, c]) == L.ZK_E_NVARS
    assert bopen([q, q]) == L.ZK_E_ARG                                    # BLS12-381 Fr only
    assert bopen([a, b], nopen=3, n_g2=2) == L.ZK_E_KZG_LEN               # nopen != n_g2, as zk_kzg_open
