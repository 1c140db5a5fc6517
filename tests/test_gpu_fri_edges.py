"""GPU: the FRI fold and prover (csrc/fri.cuh, csrc/zkmle_fri.hip) at operands that uniform tables do not reach.

Everything compares byte for byte with the Python models (tests/_fri_model.py, _ntt_model.py, _merkle_model.py); no tolerance anywhere.

  witness fold   lanes whose last step needs the SECOND subtraction of fe_from_u_below_2p (ufield.cuh): uniform tables take it about once
                 in 2^28 outputs.  The committed operands (gamma, s, t) of tests/golden/fri_fold_witnesses.json are planted in lane k as
                 a = s + t w^k / 2, b = s - t w^k / 2 (stored form), beta = 2 c gamma, so that the kernel's halved sum is s and its
                 twisted difference t.  A kernel without that subtraction returns s + gamma t + p in exactly those lanes.
  structured     tables of 0, of p - 1, equal pairs, pairs that sum to p, deltas, alternating 1 and p - 1, halved sums all odd / all even
                 (the parity the kernel sees: of the stored limbs), with gamma = p - 1, 1 and 0 and the cosets p - 1, 1 / 2, w_N, w_2N.
                 Up to 2^9 every table meets every beta and every coset; at 2^13 and 2^14, where one model fold takes a quarter of a
                 second, every table is folded once without and once with a coset, beta and coset rotating with the table.
  proof edges    zero / constant / x^(n - 1) / all p - 1 polynomials, the cosets p - 1, w_2N and an explicit 1, b = 8, Q = 4096 (a 1-bit
                 index space at N = 4), R = 1, and a proof after each refused call."""
import ctypes as C
import random

import numpy as np
import pytest

import _fri_model as FM
import _fri_witness as W
import _merkle_model as MM
import _ntt_model as NM
from oracle import pymodel as M
from test_gpu_fri import assert_same_proof, hasher_for, table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
FIELDS = (0, 3)


def to_ints(zk, field, limbs):
    return zk.to_ints(field, np.ascontiguousarray(limbs))


def stored_ints(limbs):
    """the rows of a (len, 4) u64 table as the integers of their limbs: the stored form itself"""
    return [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(limbs)]


def fold_and_compare(zk, field, values, beta, coset, what):
    """zk.fri.fold of the canonical values against FM.fold, element for element -> the library's limbs"""
    got = zk.fri.fold(table_of(zk, field, values), zk.from_ints(field, [beta])[0], None if coset is None else zk.from_ints(field, [coset])[0])
    want = to_mont(zk, field, FM.fold(field, values, beta, 1 if coset is None else coset))
    have = got.evaluated_values
    bad = np.nonzero((have != want).any(axis=1))[0]
    assert have.shape == want.shape and bad.size == 0, (what, bad[:8].tolist(), bad.size)
    return have


# ---- the second subtraction ------------------------------------------------------------------------------------------------------------
def witness_table(field, logn, coset, seed):
    """-> (canonical values, beta, lanes): lane k of `lanes` folds to s + gamma t with the committed stored operands"""
    p, n = NM.MODULUS[field], 1 << logn
    h = n // 2
    gamma, s, ts = W.load(field)
    w, inv2 = NM.root_of_unity(field, logn), pow(2, -1, p)
    values = NM.random_ints(field, n, seed)
    lanes = sorted({0, 255, 256, h - 1})
    for j, k in enumerate(lanes):
        half_delta = ts[j % len(ts)] * pow(w, k, p) * inv2 % p          # the kernel multiplies a - b by w^-k: stored (a - b) w^-k = t
        values[k] = W.real(field, (s + half_delta) % p)
        values[k + h] = W.real(field, (s - half_delta) % p)
    return values, 2 * coset * W.real(field, gamma) % p, lanes


@pytest.mark.parametrize("with_coset", (False, True))
@pytest.mark.parametrize("logn", (10, 13, 14))
@pytest.mark.parametrize("field", FIELDS)
def test_fold_lanes_that_need_the_second_subtraction(zk, field, logn, with_coset):
    p = NM.MODULUS[field]
    c = random.Random(77 * logn + field).randrange(2, p) if with_coset else 1
    values, beta, lanes = witness_table(field, logn, c, 9100 + 10 * logn + field)
    got = zk.fri.fold(table_of(zk, field, values), zk.from_ints(field, [beta])[0], zk.from_ints(field, [c])[0] if with_coset else None)
    have = got.evaluated_values
    # the planted lanes first, so that a failure names the branch: canonical limbs, and the stored integers s + gamma t mod p
    gamma, s, ts = W.load(field)
    at = stored_ints(have[lanes])
    assert all(v < p for v in at), ("not canonical: the second subtraction of fe_from_u_below_2p", lanes, [hex(v) for v in at])
    assert at == [(s + W.real(field, gamma) * ts[j % len(ts)]) % p for j in range(len(lanes))], lanes
    want = to_mont(zk, field, FM.fold(field, values, beta, c))
    bad = np.nonzero((have != want).any(axis=1))[0]
    assert bad.size == 0, (field, logn, with_coset, bad[:8].tolist(), bad.size, "planted lanes", lanes)


# ---- structured tables -----------------------------------------------------------------------------------------------------------------
def structured_tables(field, logn):
    """-> [(name, canonical values)]"""
    p, n = NM.MODULUS[field], 1 << logn
    h = n // 2
    rnd = NM.random_ints(field, h, 8800 + logn + field)
    rng = random.Random(8900 + logn + field)
    low, high = [0] * n, [0] * n
    low[h // 3], high[h + (2 * h) // 3] = 1, 1
    out = [("all 0", [0] * n), ("all p - 1", [p - 1] * n), ("a == b", rnd + rnd), ("a + b == p", rnd + [(p - v) % p for v in rnd]),
           ("delta in the low half", low), ("delta in the high half", high), ("alternating 1, p - 1", [1, p - 1] * h if n > 2 else [1, p - 1])]
    for name, parity in (("halved sum odd", 1), ("halved sum even", 0)):                  # the parity of the STORED sum: what fe_halve tests
        a = [rng.randrange(p) for _ in range(h)]
        sums = [(rng.randrange(p - 1) // 2) * 2 + parity for _ in range(h)]               # < p, of the wanted parity
        out.append((name, [W.real(field, v) for v in a] + [W.real(field, (t - v) % p) for v, t in zip(a, sums)]))
    return out


def cosets_of(field, logn):
    p = NM.MODULUS[field]
    return [("p - 1", p - 1), ("1 / 2", pow(2, -1, p)), ("w_N", NM.root_of_unity(field, logn)), ("w_2N", NM.root_of_unity(field, logn + 1))]


def betas_of(field, c):
    """gamma = beta / (2 c) = p - 1, 1, 0"""
    p = NM.MODULUS[field]
    return [("gamma = p - 1", (p - 2 * c) % p), ("gamma = 1", 2 * c % p), ("beta = 0", 0)]


@pytest.mark.parametrize("logn", (1, 2, 8, 9))
@pytest.mark.parametrize("field", FIELDS)
def test_structured_tables_fold_as_the_model_every_combination(zk, field, logn):
    for tname, values in structured_tables(field, logn):
        for cname, c in [("none", None)] + cosets_of(field, logn):
            for bname, beta in betas_of(field, 1 if c is None else c):
                fold_and_compare(zk, field, values, beta, c, (field, logn, tname, cname, bname))


@pytest.mark.parametrize("with_coset", (False, True))
@pytest.mark.parametrize("logn", (13, 14))
@pytest.mark.parametrize("field", FIELDS)
def test_structured_tables_fold_as_the_model_at_the_power_table_boundary(zk, field, logn, with_coset):
    """2^13: the last one-level power table (N / 2 = 4096); 2^14: the first two-level one.  Nine tables, three betas, four cosets: the
    rotation below meets every beta three times and every coset at least twice."""
    cosets = cosets_of(field, logn)
    for j, (tname, values) in enumerate(structured_tables(field, logn)):
        cname, c = cosets[j % 4] if with_coset else ("none", None)
        bname, beta = betas_of(field, 1 if c is None else c)[(j + j // 3) % 3]
        fold_and_compare(zk, field, values, beta, c, (field, logn, tname, cname, bname))


# ---- proof edges -----------------------------------------------------------------------------------------------------------------------
def prove_and_compare(zk, field, coeffs, b, f, Q, coset=1, pass_coset=None, tr=None):
    """zk.fri.prove against FM.prove byte for byte, accepted by zk.fri.verify -> (proof, model's proof).  `pass_coset`: None passes a NULL
    coset to the library, True the element `coset`; default: NULL exactly when coset == 1.  `tr`: the MODEL's transcript."""
    d = len(coeffs).bit_length() - 1
    give = coset != 1 if pass_coset is None else pass_coset
    cm = zk.from_ints(field, [coset])[0] if give else None
    pr = FM.prove(field, coeffs, b, f, Q, coset, tr, hasher_for(zk, 1 << (d + b)))
    got = zk.fri.prove(table_of(zk, field, coeffs), b, f, Q, cm)
    assert_same_proof(zk, got, pr)
    assert zk.fri.verify(got)
    return got, pr


def edge_polynomials(field, d):
    p, n = NM.MODULUS[field], 1 << d
    return {"zero": [0] * n, "constant": [p - 2] + [0] * (n - 1), "x^(n - 1)": [0] * (n - 1) + [1], "all p - 1": [p - 1] * n}


@pytest.mark.parametrize("shape", [(6, 2, 2), (10, 3, 0)])
@pytest.mark.parametrize("poly", ("zero", "constant", "x^(n - 1)", "all p - 1"))
@pytest.mark.parametrize("field", FIELDS)
def test_proofs_of_structured_polynomials(zk, field, poly, shape):
    d, b, f = shape
    p = NM.MODULUS[field]
    coset = random.Random(d + field).randrange(2, p) if (d + field) % 2 else 1
    got, pr = prove_and_compare(zk, field, edge_polynomials(field, d)[poly], b, f, 6, coset)
    if poly in ("zero", "constant"):                           # every layer is one value: every opened pair cancels in the fold
        want = 0 if poly == "zero" else p - 2
        assert set(to_ints(zk, field, got.query_values.reshape(-1, 4))) == {want}
        assert to_ints(zk, field, got.final_coeffs) == [want] + [0] * ((1 << f) - 1)


@pytest.mark.parametrize("field", FIELDS)
def test_proofs_on_cosets_that_are_roots_of_unity(zk, field):
    d, b, f, Q = 7, 2, 3, 6
    p = NM.MODULUS[field]
    coeffs = NM.random_ints(field, 1 << d, 4700 + field)
    for c in (p - 1, NM.root_of_unity(field, d + b + 1)):
        prove_and_compare(zk, field, coeffs, b, f, Q, c)
    none, pr = prove_and_compare(zk, field, coeffs, b, f, Q, 1)
    one, _ = prove_and_compare(zk, field, coeffs, b, f, Q, 1, pass_coset=True)
    for name in ("roots", "final_coeffs", "betas", "query_indices", "query_values", "query_paths"):
        assert np.array_equal(getattr(one, name), getattr(none, name)), name


@pytest.mark.parametrize("d", (1, 5))
@pytest.mark.parametrize("field", FIELDS)
def test_proofs_at_the_largest_blowup(zk, field, d):
    p = NM.MODULUS[field]
    prove_and_compare(zk, field, NM.random_ints(field, 1 << d, 4800 + d + field), 8, 0, 5, random.Random(d).randrange(2, p))


class HostKeccakTranscript(M.Transcript):
    """oracle/pymodel.py's transcript with its hash swapped for the library's HOST zk_keccak256.  The model's transcript hashes everything
    absorbed so far for every sample: 4096 samples in pure Python take minutes.  As for the large trees (tests/_merkle_model.py), the host
    hash is checked against the pure-Python one first, here also on inputs of several blocks."""

    def __init__(self, zk):
        super().__init__()
        self.hash = MM.check_host_keccak(zk)
        for n in (0, 135, 136, 137, 1000):
            data = bytes((11 * i + n) & 0xFF for i in range(n))
            assert self.hash(data) == M.keccak256(data), n

    def sample(self):
        d = self.hash(bytes(self.buf))
        self.buf += d
        return d


@pytest.mark.parametrize("d", (1, 3))
@pytest.mark.parametrize("field", FIELDS)
def test_proofs_with_the_most_queries(zk, field, d):
    Q = 4096
    got, pr = prove_and_compare(zk, field, NM.random_ints(field, 1 << d, 4900 + d + field), 1, 0, Q, 1 if d == 1 else 3,
                                tr=HostKeccakTranscript(zk))
    half = (1 << (d + 1)) // 2
    assert set(int(i) for i in got.query_indices) == set(range(half))          # 4096 draws from 2 or 8 indices: every one is drawn
    per = got.query_paths.size // Q
    paths = got.query_paths.reshape(Q, per)
    first = {}
    for q, i in enumerate(int(i) for i in got.query_indices):                 # the same index: the same answer, byte for byte
        k = first.setdefault(i, q)
        assert np.array_equal(got.query_values[q], got.query_values[k]) and np.array_equal(paths[q], paths[k]), (q, k)


@pytest.mark.parametrize("field", FIELDS)
def test_proof_of_one_fold(zk, field):
    d, b = 11, 2
    got, _ = prove_and_compare(zk, field, NM.random_ints(field, 1 << d, 5000 + field), b, d - 1, 7, 5)
    assert got.roots.shape[0] == 1 and got.final_coeffs.shape[0] == 1 << (d - 1)


@pytest.mark.parametrize("refused", ("ZK_E_ARG", "ZK_E_NOT_POW2", "ZK_E_RANGE"))
def test_a_refused_call_leaves_the_next_proof_unchanged(zk, refused):
    """the rejections of tests/test_fri_cpu.py test_precondition_codes_come_before_the_device_check that a machine with a device still
    reaches: the proof after one is the proof before it, and the model's"""
    from zkmle_amd import _lib as L
    field, d, b, f, Q, c = 0, 6, 2, 1, 9, 11
    coeffs = NM.random_ints(field, 1 << d, 5100)
    before, _ = prove_and_compare(zk, field, coeffs, b, f, Q, c)
    poly, cm = table_of(zk, field, coeffs), zk.from_ints(field, [c])[0]
    with pytest.raises(L.ZkError) as e:
        if refused == "ZK_E_ARG":
            zk.fri.prove(poly, b, f, Q, np.zeros(4, np.uint64))                                    # a zero coset
        elif refused == "ZK_E_NOT_POW2":
            zk.fri.prove(zk.MultilinearPolynomial.vector(field, to_mont(zk, field, coeffs[:48])), b, f, Q, cm)
        else:
            zk.fri.prove(zk.MultilinearPolynomial.vector(1, zk.from_ints(1, list(range(1, 9)))), 1, 0, Q)   # an Fq field has no domain
    assert e.value.code == getattr(L, refused)
    after, _ = prove_and_compare(zk, field, coeffs, b, f, Q, c)
    for name in ("roots", "final_coeffs", "betas", "query_indices", "query_values", "query_paths"):
        assert np.array_equal(getattr(after, name), getattr(before, name)), name
