"""GPU: the FRI low-degree prover (csrc/fri.cuh, csrc/zkmle_fri.hip) over BLS12-381 Fr and BN254 Fr.

Sizes the model reaches (tests/_fri_model.py, Python integers): one fold equals the model element for element for every 2^1 .. 2^14, and a
whole proof -- roots, final coefficients, betas, indices, values, paths -- equals the model's byte for byte for d = 1 .. 11 with N up to
2^13, which crosses the 4096-entry boundary of the power tables (N / 2 > 4096) and the one-workgroup finish of the tree (512 nodes).

Sizes it does not reach (N = 2^20 and 2^24, BLS12-381 Fr): the proof is tied to calls that existed before the prover did.  The host
verifier accepts it; every root_l equals zk_mle_merkle_root of zk_uni_low_degree_extend(a_l, b, c_l), where a_l is the coefficient table
folded l times as a[0::2] + beta a[1::2] by zk_mle_linear_combination with the betas the prover returned; the final coefficients equal
a_R; every opened value equals the entry of that independently built layer."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import __graft_entry__ as G
import _fri_model as FM
import _merkle_model as MM
import _ntt_model as NM
from oracle import pymodel as M

pytestmark = pytest.mark.gpu
FIELDS = (0, 3)
# (d, b, f, Q): N = 2^(d + b) reaches 2^13 twice; f = 0, f = d - 1 and b = 1 are among them
SHAPES = [(1, 1, 0, 3), (2, 2, 1, 4), (3, 1, 0, 5), (4, 3, 2, 6), (5, 2, 0, 8), (6, 1, 5, 4), (7, 2, 3, 9), (8, 3, 1, 5), (9, 2, 4, 6),
          (10, 2, 0, 7), (10, 3, 2, 5), (11, 2, 6, 40), (11, 1, 10, 3)]


@pytest.fixture(scope="module")
def zk():
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    return zk


def to_mont(zk, field, ints):
    nl = zk.limbs(field)
    canon = np.frombuffer(b"".join(int(v).to_bytes(8 * nl, "little") for v in ints), np.uint64).reshape(-1, nl).copy()
    out = np.zeros_like(canon)
    from zkmle_amd import _lib as L
    L.check(zk.lib().zk_vec_from_canonical(field, L.p64(canon), canon.shape[0], L.p64(out)))
    return out


def table_of(zk, field, ints):
    return zk.MultilinearPolynomial.vector(field, to_mont(zk, field, ints))


def hasher_for(zk, n):
    return MM.check_host_keccak(zk) if n > MM.PURE_PYTHON_MAX else M.keccak256


def assert_same_proof(zk, got, pr):
    """the library's FriProof against the model's dict, every array byte for byte"""
    fl = FM.flat(zk, pr)
    for name, arr in (("roots", got.roots), ("final", got.final_coeffs), ("betas", got.betas), ("indices", got.query_indices),
                      ("values", got.query_values), ("paths", got.query_paths)):
        assert arr.shape == fl[name].shape and np.array_equal(arr, fl[name]), name


def case_inputs(zk, field, d, b, with_coset, seed=0):
    p = NM.MODULUS[field]
    coeffs = NM.random_ints(field, 1 << d, 7000 + 31 * d + b + field + seed)
    coset = random.Random(d * 16 + b + seed).randrange(2, p) if with_coset else 1
    return coeffs, coset, (zk.from_ints(field, [coset])[0] if with_coset else None)


@pytest.mark.parametrize("logn", range(1, 15))
@pytest.mark.parametrize("field", FIELDS)
def test_fold_equals_the_model(zk, field, logn):
    p, n = NM.MODULUS[field], 1 << logn
    v = NM.random_ints(field, n, 300 * field + logn)
    rng = random.Random(11 * logn + field)
    beta, c = rng.randrange(p), rng.randrange(2, p)
    cw = table_of(zk, field, v)
    for coset, cm in ((1, None), (c, zk.from_ints(field, [c])[0])):
        got = zk.fri.fold(cw, zk.from_ints(field, [beta])[0], cm)
        assert len(got) == n // 2
        want = to_mont(zk, field, FM.fold(field, v, beta, coset))
        bad = np.nonzero((got.evaluated_values != want).any(axis=1))[0]
        assert bad.size == 0, (field, logn, coset != 1, bad[:8], bad.size)
    for special in (0, 1, p - 1):                                    # beta = 0 keeps the halved sum alone
        got = zk.fri.fold(cw, zk.from_ints(field, [special])[0], None)
        assert np.array_equal(got.evaluated_values, to_mont(zk, field, FM.fold(field, v, special, 1))), (field, logn, special)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("field", FIELDS)
def test_proof_equals_the_model_byte_for_byte(zk, field, shape):
    d, b, f, Q = shape
    with_coset = (d + field) % 3 != 0
    coeffs, coset, cm = case_inputs(zk, field, d, b, with_coset)
    pr = FM.prove(field, coeffs, b, f, Q, coset, hasher=hasher_for(zk, 1 << (d + b)))
    poly = table_of(zk, field, coeffs)
    got = zk.fri.prove(poly, b, f, Q, cm)
    assert_same_proof(zk, got, pr)
    assert zk.fri.verify(got)
    st = zk.fri.last_stats()
    assert st["layers"] == d - f and st["queries"] == Q and st["ms_total"] > 0
    # the same bytes from the codeword the caller already holds
    again = zk.fri.prove_codeword(zk.low_degree_extend(poly, b, cm), b, f, Q, cm)
    assert_same_proof(zk, again, pr)
    assert zk.fri.last_stats()["ms_extend"] == 0
    # the first committed layer is the tree everybody else builds
    assert got.roots[0].tobytes() == zk.merkle_root(zk.low_degree_extend(poly, b, cm))


@pytest.mark.parametrize("field", FIELDS)
def test_a_callers_transcript_ends_in_the_models_state(zk, field):
    prior = b"absorbed before the proof"
    d, b, f, Q = 9, 2, 3, 5
    coeffs, coset, cm = case_inputs(zk, field, d, b, True, seed=5)
    mt = M.Transcript()
    mt.append(prior)
    pr = FM.prove(field, coeffs, b, f, Q, coset, mt, hasher_for(zk, 1 << (d + b)))
    t = zk.Transcript()
    t.append(prior)
    got = zk.fri.prove(table_of(zk, field, coeffs), b, f, Q, cm, transcript=t)
    assert_same_proof(zk, got, pr)
    want = zk.Transcript()
    want.append(bytes(mt.buf))
    assert np.array_equal(t.export_state(), want.export_state())
    tv = zk.Transcript()
    tv.append(prior)
    assert zk.fri.verify(got, tv) and np.array_equal(tv.export_state(), want.export_state())
    assert not zk.fri.verify(got)


def test_a_table_that_is_no_codeword_gets_a_proof_that_is_rejected(zk):
    field, b, Q = 0, 2, 40
    junk = zk.MultilinearPolynomial.random(field, 1 << 12, 0xF41)          # seeded: SplitMix64 stream 0xF41
    got = zk.fri.prove_codeword(junk, b, 3, Q)                              # ZK_OK: not of low degree is not an error
    assert not zk.fri.verify(got)
    # An honest codeword with ONE entry changed.  SEED = 1 was picked with the model (SEED = 0 misses): with it the changed entry E is one of the two
    # entries of layer 0 that some query opens (asserted below), so the verifier sees the change itself.
    SEED, d, f = 1, 6, 2
    p, N = NM.MODULUS[field], 1 << (d + b)
    coeffs = NM.random_ints(field, 1 << d, 5150 + SEED)
    E = random.Random(SEED).randrange(N)
    cw = FM.extend(field, coeffs, b)
    honest = zk.fri.prove_codeword(table_of(zk, field, cw), b, f, Q)
    assert zk.fri.verify(honest)
    cw[E] = (cw[E] + 1) % p
    got = zk.fri.prove_codeword(table_of(zk, field, cw), b, f, Q)
    assert_same_proof(zk, got, FM.prove_codeword(field, cw, b, f, Q))
    assert any(int(i) % (N // 2) == E % (N // 2) for i in got.query_indices), "no query opens the changed entry: pick another SEED"
    assert not zk.fri.verify(got)


def test_two_threads_on_two_streams_give_the_serial_proofs(zk):
    import torch
    lib = zk.lib()
    jobs = []
    for k in range(2):
        poly = zk.MultilinearPolynomial.random(0, 1 << (14 + 2 * k), 0xF2A + k)
        cm = zk.from_ints(0, [91 + k])[0]
        jobs.append((poly, cm, zk.fri.prove(poly, 2, 4 + k, 24, cm)))
    streams = [torch.cuda.Stream() for _ in jobs]
    errors = []

    def work(job, stream):
        poly, cm, want = job
        try:
            lib.zk_set_stream(C.c_void_p(stream.cuda_stream))
            for _ in range(3):
                got = zk.fri.prove(poly, 2, want.log_final, 24, cm)
                for name in ("roots", "final_coeffs", "betas", "query_indices", "query_values", "query_paths"):
                    assert np.array_equal(getattr(got, name), getattr(want, name)), name
                assert zk.fri.verify(got)
        except Exception as e:      # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(j, st)) for j, st in zip(jobs, streams)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_release_cached_memory_between_proofs(zk):
    from zkmle_amd import _lib as L
    poly = zk.MultilinearPolynomial.random(0, 1 << 15, 0xCAC)
    first = zk.fri.prove(poly, 2, 5, 16)
    L.check(zk.lib().zk_release_cached_memory())
    second = zk.fri.prove(poly, 2, 5, 16)
    for name in ("roots", "final_coeffs", "betas", "query_indices", "query_values", "query_paths"):
        assert np.array_equal(getattr(first, name), getattr(second, name)), name
    assert zk.fri.verify(second)


@pytest.mark.parametrize("d", (18, 22))
def test_large_proofs_are_tied_to_the_calls_that_existed_before(zk, d):
    field, b, f, Q = 0, 2, 6, 64
    p, R, N = NM.MODULUS[field], d - f, 1 << (d + b)
    c = random.Random(d).randrange(2, p)
    poly = zk.MultilinearPolynomial.random(field, 1 << d, 0xB16 + d)
    proof = zk.fri.prove(poly, b, f, Q, zk.from_ints(field, [c])[0])
    assert zk.fri.verify(proof)                                                            # route 1
    betas = zk.to_ints(field, proof.betas)
    a = poly
    for l in range(R + 1):
        if l == R:
            assert np.array_equal(proof.final_coeffs, a.evaluated_values), "final coefficients"     # route 3
            break
        layer = zk.low_degree_extend(a, b, zk.from_ints(field, [pow(c, 1 << l, p)])[0])
        assert proof.roots[l].tobytes() == zk.merkle_root(layer), l                          # route 2
        host = layer.evaluated_values
        half = (N >> l) // 2
        for q in range(Q):                                                                 # route 4
            j = int(proof.query_indices[q]) % half
            assert np.array_equal(proof.query_values[q, l, 0], host[j]) and np.array_equal(proof.query_values[q, l, 1], host[j + half]), (l, q)
        del host, layer
        coeffs = a.evaluated_values
        even, odd = (zk.MultilinearPolynomial.vector(field, np.ascontiguousarray(coeffs[k::2])) for k in range(2))
        a = zk.MultilinearPolynomial.linear_combination([even, odd], zk.from_ints(field, [1, betas[l]]))
