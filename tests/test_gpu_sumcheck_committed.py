"""GPU: the provers bound to a table's Merkle root instead of its bytes (include/zkmle.h: zk_sumcheck_basic_prove_committed,
zk_sumcheck_basic_verify_committed, zk_gkr_sparse_prove_committed).  They differ from the modelled provers in the transcript's first append
alone, so the model is oracle/pymodel.py's own prover run on a Transcript subclass that replaces its first append by the Merkle root of
those bytes cut into leaves (tests/_merkle_model.py)."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as G
import _merkle_model as MM
from _committed_worker import proof_digest
from oracle import pymodel as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def zk():
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    return zk


def model_basic_prove(zk, field, ints, prior=b""):
    """-> (root, claimed, rounds, challenges, the transcript's end state).  32-byte fields: pymodel.sumcheck_basic_prove itself on the
    committed transcript; Fq381: the same lines with the 48-byte encoding (pymodel's be32 defaults to 32 bytes)."""
    esz, p = MM.ELEMENT_BYTES[field], MM.MODULUS[field]
    cls = MM.committed_transcript_class(esz, zk, prior)
    made = []

    class Recording(cls):
        def __init__(self):
            super().__init__()
            made.append(self)

    if esz == 32:
        with MM.patched_transcript(Recording):
            claimed, rounds, chal = M.sumcheck_basic_prove(ints, p)
    else:
        t = Recording()
        claimed = sum(ints) % p                                           # prover.rs:28
        t.append(b"".join(M.be32(v, esz) for v in ints))                  # :38-39 -> the root
        t.append(M.be32(claimed, esz))                                    # :40-41
        cur, rounds, chal = list(ints), [], []
        while len(cur) > 1:                                               # :46
            h = len(cur) // 2
            uni = [sum(cur[:h]) % p, sum(cur[h:]) % p]                    # :74-89
            rounds.append(uni)
            t.append(M.be32(uni[0], esz) + M.be32(uni[1], esz))           # :52-55
            r = t.challenge(p)                                            # :58
            chal.append(r)
            cur = M.partial_evaluate(cur, 0, r, p)                        # :61
    return cls.last_root, claimed, rounds, chal, bytes(made[0].buf)


def check_against_model(zk, field, ints, proof, challenges):
    root, claimed, rounds, chal, _ = model_basic_prove(zk, field, ints)
    assert proof.root == root
    assert zk.to_ints(field, proof.initial_claimed_sum) == [claimed]
    assert [zk.to_ints(field, r) for r in proof.round_univariate_polynomials] == rounds
    assert zk.to_ints(field, challenges) == chal


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_committed_proof_equals_the_committed_model(zk, field):
    for logn in range(13):
        ints = MM.random_ints(field, 1 << logn, 7000 + 16 * field + logn)
        mont = zk.from_ints(field, ints)
        prover = zk.Prover.init(field, mont)
        proof = prover.prove_committed()
        check_against_model(zk, field, ints, proof, prover.challenges)
        assert proof.root == zk.merkle_root(prover.initial_polynomial)
        if logn:                                                          # the root is really what was bound
            plain = zk.Prover.init(field, mont)
            plain.prove()
            assert not np.array_equal(plain.challenges, prover.challenges)
        V = zk.Verifier.init()
        assert V.verify_committed(proof) is True
        assert V.verify_committed(proof, root=proof.root) is True
        if logn >= 2:                                                     # (one round alone passes under any challenge)
            assert V.verify(proof) is False                               # the uncommitted verifier replays another transcript
        if logn:
            bad = zk.sumcheck.SumcheckProof(proof.initial_polynomial, proof.initial_claimed_sum, proof.round_univariate_polynomials.copy(), root=proof.root)
            bad.round_univariate_polynomials[logn // 2, 1, 0] ^= np.uint64(1)          # a changed message
            assert V.verify_committed(bad) is False
        wrong = bytearray(proof.root)
        wrong[7] ^= 0x10
        assert V.verify_committed(proof, root=bytes(wrong)) is False      # a wrong root
        other = mont.copy()                                               # a table with one changed entry
        other[(1 << logn) // 3, 0] ^= np.uint64(2)
        moved = zk.sumcheck.SumcheckProof(zk.MultilinearPolynomial(field, other), proof.initial_claimed_sum, proof.round_univariate_polynomials, root=proof.root)
        assert V.verify_committed(moved) is False
        moved.root = None                                                 # ... also when no root comes with the proof
        assert V.verify_committed(moved, root=None) is False


def test_caller_transcript_with_prior_appends_ends_in_the_model_state(zk):
    field, logn = 3, 9
    prior = [b"domain separator", bytes(range(200))]
    ints = MM.random_ints(field, 1 << logn, 31)
    prover = zk.Prover.init(field, zk.from_ints(field, ints))
    for b in prior:
        prover.transcript.append(b)
    proof = prover.prove_committed()
    root, claimed, rounds, chal, buf = model_basic_prove(zk, field, ints, prior=b"".join(prior))
    assert proof.root == root and zk.to_ints(field, prover.challenges) == chal
    assert [zk.to_ints(field, r) for r in proof.round_univariate_polynomials] == rounds
    after = M.Transcript()
    after.buf += buf
    assert prover.transcript.sample_random_challenge() == after.sample()   # the same sponge: the same next digest
    # NULL transcript = a fresh one
    from zkmle_amd import _lib as L
    Lm = zk.limbs(field)
    cs, rp, ch, rt = np.zeros(Lm, np.uint64), np.zeros((logn, 2, Lm), np.uint64), np.zeros((logn, Lm), np.uint64), np.zeros(32, np.uint8)
    zk.sumcheck._decl()
    L.check(zk.lib().zk_sumcheck_basic_prove_committed(prover.initial_polynomial._h, None, L.p8(rt), L.p64(cs), L.p64(rp), L.p64(ch)))
    assert zk.to_ints(field, ch) == model_basic_prove(zk, field, ints)[3] and rt.tobytes() == root


def run_worker(field, logn, seed, env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_committed_worker.py"), str(field), str(logn), str(seed)], capture_output=True,
                       text=True, env=e, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_2p20_equals_the_model_and_the_device_transcript_gives_the_same_bytes(zk):
    field, logn, seed = 0, 20, 0xC0117
    poly = zk.MultilinearPolynomial.random(field, 1 << logn, seed)
    prover = zk.Prover.init(field, poly)
    proof = prover.prove_committed()
    check_against_model(zk, field, poly.to_ints(), proof, prover.challenges)
    assert zk.Verifier.init().verify_committed(proof) is True
    mine = proof_digest(proof, prover.challenges)
    for env in ({"ZK_HOST_TRANSCRIPT": "0"}, {"ZK_FOLD_SPLIT2": "0"}):
        out = run_worker(field, logn, seed, env)
        assert out["digest"] == mine and out["verified"] is True, env


@pytest.mark.parametrize("logn", [22, 24])
def test_large_committed_proofs_replay_on_the_host(zk, logn):
    field, n = 0, 1 << logn
    p = MM.MODULUS[field]
    poly = zk.MultilinearPolynomial.random(field, n, 0xBEEF + logn)
    prover = zk.Prover.init(field, poly)
    proof = prover.prove_committed()
    assert proof.root == zk.merkle_root(poly)
    cs = zk.to_ints(field, proof.initial_claimed_sum)[0]
    msgs = [zk.to_ints(field, r) for r in proof.round_univariate_polynomials]
    t = M.Transcript()                                                     # the host replay: root, claimed sum, then round by round
    t.append(proof.root)
    t.append(M.be32(cs))
    chal, claim = [], cs
    for e0, e1 in msgs:
        assert (e0 + e1) % p == claim
        t.append(M.be32(e0) + M.be32(e1))
        r = t.challenge(p)
        chal.append(r)
        claim = (e0 + r * (e1 - e0)) % p
    assert zk.to_ints(field, prover.challenges) == chal
    assert zk.to_ints(field, poly.half_sums()) == msgs[0]
    assert zk.to_ints(field, poly.evaluate(prover.challenges)) == [claim]
    assert zk.Verifier.init().verify_committed(proof) is True
    st = zk.sumcheck.last_stats()
    print(f"2^{logn}: committed verify's binding {st['ms_absorb']:.2f} ms")


# ---- sparse GKR with the output layer bound by its root ------------------------------------------------------------------------
WIDE_SHAPES = [(3, 5, 4, 3), (2, 6, 3, 5, 2), (1, 4, 2), (2, 2, 2), (4, 1, 3), (1, 1, 1), (3, 3), (5, 2), (2, 5), (1, 6, 1), (6, 1, 4),
               (2, 3, 4, 5, 1), (4, 4, 4, 4), (3, 1)]                      # the first 14 shapes of tests/test_gpu_gkr_sparse.py


@pytest.mark.parametrize("shape", WIDE_SHAPES)
def test_sparse_gkr_committed_equals_the_committed_wide_model(zk, shape):
    *out_bits, in_last = shape
    widths = list(out_bits) + [in_last]
    for f in (0, 2):
        p = MM.MODULUS[f]
        rng = random.Random(hash(shape) % 1000 + f)
        spec = []
        for l in range(len(out_bits)):
            n_out, n_in = 1 << widths[l], 1 << widths[l + 1]
            seen = set()
            for _ in range(rng.randrange(n_out // 2 + 1, 2 * n_out + 2)):
                seen.add((rng.randrange(n_in), rng.randrange(n_in), rng.randrange(n_out), rng.choice([0, 1])))
            spec.append(sorted(seen, key=lambda g: (g[2], g[0], g[1], g[3])))
        xs = [rng.choice([0, 1, p - 1, rng.randrange(p)]) for _ in range(1 << in_last)]
        cls = MM.committed_transcript_class(32, zk)
        with MM.patched_transcript(cls):
            want = M.gkr_prove_wide(spec, out_bits, xs, p)
        plain_want = M.gkr_prove_wide(spec, out_bits, xs, p)
        rows = [np.array(layer, np.uint64).reshape(-1, 4) for layer in spec]
        x = zk.from_ints(f, xs)
        proof = zk.gkr.sparse_prove(f, rows, out_bits, x, commit_output=True)
        assert proof.output_root == cls.last_root
        assert zk.to_ints(f, proof.circuit_output) == want["circuit_output"]
        assert zk.to_ints(f, proof.output_challenges) == want["output_challenges"]
        assert zk.to_ints(f, proof.layer_claims) == want["layer_claims"]
        assert [zk.to_ints(f, c) for c in proof.coeffs] == want["coeffs"]
        assert zk.to_ints(f, proof.challenges) == want["challenges"]
        assert zk.to_ints(f, proof.wb_evals) == want["wb"] and zk.to_ints(f, proof.wc_evals) == want["wc"]
        assert zk.to_ints(f, proof.claimed_sum.reshape(1, -1)) == [want["claimed_sum"]]
        assert zk.gkr.sparse_verify(f, rows, out_bits, proof, x, commit_output=True) is True
        tampered = zk.gkr.SparseProof(**{**proof.__dict__, "circuit_output": proof.circuit_output.copy()})
        tampered.circuit_output[len(tampered.circuit_output) // 2, 0] ^= np.uint64(1)   # one output wire changed
        assert zk.gkr.sparse_verify(f, rows, out_bits, tampered, x, commit_output=True) is False
        tampered.output_root = None
        assert zk.gkr.sparse_verify(f, rows, out_bits, tampered, x, commit_output=True) is False
        # the uncommitted prover keeps its bytes
        plain = zk.gkr.sparse_prove(f, rows, out_bits, x)
        assert plain.output_root is None
        assert zk.to_ints(f, plain.output_challenges) == plain_want["output_challenges"]
        assert [zk.to_ints(f, c) for c in plain.coeffs] == plain_want["coeffs"] and zk.to_ints(f, plain.challenges) == plain_want["challenges"]
        assert zk.gkr.sparse_verify(f, rows, out_bits, plain, x) is True
