"""GPU: the k-table linear combination (zk_mle_linear_combination) against Python integers, and the batched multilinear-KZG opening
(zk_kzg_batch_open: k polynomials at one point, one proof; extension: no reference counterpart) against the oracle's naive open_and_prove
of sum_j gamma^j f_j, with gamma from the transcript model, and against the single openings it replaces."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import oracle as O
from oracle import pymodel as PM

pytestmark = pytest.mark.gpu
R = PM.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def zk():
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    return zk


def host_random(zk, field, n, seed):
    t = np.zeros((n, zk.limbs(field)), np.uint64)
    assert zk.lib().zk_host_fill_random(field, seed, 0, n, t.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
    return t


def comb_rc(zk, tables, coeffs, out):
    from zkmle_amd import _lib as L
    arr = (L.vp * len(tables))(*[t._h.value for t in tables])
    c = np.ascontiguousarray(coeffs, np.uint64)
    return zk.lib().zk_mle_linear_combination(arr, len(tables), L.p64(c), out._h, None)


# ---- zk_mle_linear_combination --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [0, 3])
@pytest.mark.parametrize("length", [1, 2, 3, 1000])
@pytest.mark.parametrize("k", [1, 2, 7, 64])
def test_linear_combination_vs_python_ints(zk, field, length, k):
    p = zk.mle.MODULI[field]
    MP = zk.MultilinearPolynomial
    rows = [host_random(zk, field, length, 9000 + 97 * j + length) for j in range(k)]
    tabs = [MP.vector(field, r) for r in rows]
    ints = [zk.to_ints(field, r) for r in rows]
    rng = np.random.default_rng(k * 1000 + length + field)
    cf = [0, 1, p - 1] + [int.from_bytes(rng.bytes(40), "little") % p for _ in range(k)]
    cf = cf[:k] if k > 1 else [p - 1]
    got = MP.linear_combination(tabs, zk.from_ints(field, cf)).to_ints()
    want = [sum(c * col[i] for c, col in zip(cf, ints)) % p for i in range(length)]
    assert got == want
    if k >= 2:                                                    # the same table passed more than once
        got = MP.linear_combination([tabs[0]] * k, zk.from_ints(field, cf)).to_ints()
        assert got == [sum(cf) * ints[0][i] % p for i in range(length)]


@pytest.mark.parametrize("field", [0, 3])
def test_linear_combination_reduction_bounds_all_p_minus_1(zk, field):
    """k = 64 tables of p - 1 with coefficients p - 1: the largest value the one-reduction-per-output accumulation sees"""
    p = zk.mle.MODULI[field]
    MP = zk.MultilinearPolynomial
    n = 1000
    t = MP.vector(field, zk.from_ints(field, [p - 1] * n))
    got = MP.linear_combination([t] * 64, zk.from_ints(field, [p - 1] * 64)).to_ints()
    assert got == [64 % p] * n
    distinct = [MP.vector(field, zk.from_ints(field, [p - 1] * n)) for _ in range(64)]
    got = MP.linear_combination(distinct, zk.from_ints(field, [p - 1] * 63 + [1])).to_ints()
    assert got == [(63 - 1) % p] * n


@pytest.mark.parametrize("field", [0, 3])
def test_linear_combination_2p20_vs_the_elementwise_chain(zk, field):
    """2^20 entries, k = 7: equal to scalar_mul + add_polynomials (evaluation_form.rs:49, :145) chained, and to Python ints on a sample"""
    p = zk.mle.MODULI[field]
    MP = zk.MultilinearPolynomial
    n, k = 1 << 20, 7
    tabs = [MP.random(field, n, 0xC0FFEE + j) for j in range(k)]
    cf = [0, 1, p - 1, 5, 2 ** 200 % p, p - 2, 123456789]
    cm = zk.from_ints(field, cf)
    got = MP.linear_combination(tabs, cm)
    acc = tabs[0].scalar_mul(cm[0])
    for j in range(1, k):
        acc = MP.add_polynomials(acc, tabs[j].scalar_mul(cm[j]))
    gv = got.evaluated_values
    assert np.array_equal(gv, acc.evaluated_values)
    idx = np.random.default_rng(20).choice(n, 512, replace=False)
    cols = [zk.to_ints(field, t.evaluated_values[idx]) for t in tabs]
    want = [sum(c * col[s] for c, col in zip(cf, cols)) % p for s in range(len(idx))]
    assert zk.to_ints(field, gv[idx]) == want


def test_linear_combination_codes(zk):
    from zkmle_amd import _lib as L
    MP = zk.MultilinearPolynomial
    a, b = MP.random(0, 64, 1), MP.random(0, 64, 2)
    out = MP.alloc(0, 64)
    c = zk.from_ints(0, list(range(65)))
    assert comb_rc(zk, [a, MP.random(0, 32, 3)], c, out) == L.ZK_E_NVARS
    assert comb_rc(zk, [a] * 65, c, out) == L.ZK_E_ARG
    assert comb_rc(zk, [a, b], c, a) == L.ZK_E_ARG                  # out aliases an input
    assert comb_rc(zk, [a, MP.random(3, 64, 4)], c, out) == L.ZK_E_ARG
    with pytest.raises(zk.ReferencePanic):
        MP.linear_combination([a, MP.random(0, 32, 3)], c[:2])


# ---- zk_kzg_batch_open ----------------------------------------------------------------------------------------------------------
def model_gamma(commitments, opening_ints, eval_ints, prefix=b""):
    t = PM.Transcript()
    t.append(prefix)
    for c in commitments:
        xy = O.g1_affine_ints(c)
        t.append(bytes(96) if xy is None else PM.be32(xy[0], 48) + PM.be32(xy[1], 48))
    for x in list(opening_ints) + list(eval_ints):
        t.append(PM.be32(x))
    return t.challenge(R), t


def setup_for(zk, n, seed):
    rng = np.random.default_rng(seed)
    taus = zk.from_ints(0, [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)])
    return zk.TrustedSetup.initialize_setup(taus)


@pytest.mark.parametrize("n", [0, 1, 2, 5, 10])
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_batch_open_vs_oracle(zk, n, k):
    MP, KZG = zk.MultilinearPolynomial, zk.MultilinearKZG
    if n == 0:                                                     # one point, no proofs: as zk_kzg_open at nopen = 0
        setup = zk.TrustedSetup(zk.G1Bases(O.g1_generator()[None, :]), 0)
    else:
        setup = setup_for(zk, n, 500 + n)
    pts = setup.g1_powers_of_tau.points()
    vals = [host_random(zk, 0, 1 << n, 7000 + 31 * n + j) for j in range(k)]
    polys = [MP(0, v) for v in vals]
    commitments = np.stack([KZG.commit_to_polynomial(f, setup) for f in polys])
    for j in range(k):
        assert np.array_equal(commitments[j], O.kzg_commit(vals[j], pts))
    opening = host_random(zk, 0, n, 8100 + n) if n else np.zeros((0, 4), np.uint64)
    proof = KZG.batch_open_and_prove(polys, setup, opening, commitments)
    for j in range(k):
        assert np.array_equal(proof.evaluations[j], O.evaluate(O.FR381, vals[j], opening) if n else vals[j][0])
    gamma, _ = model_gamma(commitments, O.to_ints(O.FR381, opening) if n else [], O.to_ints(O.FR381, proof.evaluations))
    assert O.to_ints(O.FR381, proof.gamma) == [gamma]
    cols = [O.to_ints(O.FR381, v) for v in vals]
    g = O.from_ints(O.FR381, [sum(pow(gamma, j, R) * cols[j][i] for j in range(k)) % R for i in range(1 << n)])
    if n == 0:
        assert proof.proofs.shape[0] == 0
        return
    ev, want = O.kzg_open(g, pts, opening)
    assert np.array_equal(proof.proofs, want)
    assert KZG.batch_verify(setup, commitments, opening, proof) is True
    if k == 1:                                                     # g = f_0: the single opening's proof
        single = KZG.open_and_prove(polys[0], setup, opening)
        assert np.array_equal(single.proofs, proof.proofs) and np.array_equal(single.evaluation, proof.evaluations[0])


def test_batch_open_on_the_callers_transcript(zk):
    """the prover absorbs into the caller's transcript; a verifier replaying it from the same state accepts and ends in the same state"""
    MP, KZG = zk.MultilinearPolynomial, zk.MultilinearKZG
    n, k = 6, 3
    setup = setup_for(zk, n, 66)
    polys = [MP.random(0, 1 << n, 660 + j) for j in range(k)]
    commitments = np.stack([KZG.commit_to_polynomial(f, setup) for f in polys])
    opening = host_random(zk, 0, n, 661)
    tp, tv = zk.Transcript(), zk.Transcript()
    for t in (tp, tv):
        t.append(b"a sumcheck came first")
    proof = KZG.batch_open_and_prove(polys, setup, opening, commitments, transcript=tp)
    gamma, model = model_gamma(commitments, O.to_ints(O.FR381, opening), O.to_ints(O.FR381, proof.evaluations),
                               prefix=b"a sumcheck came first")
    assert O.to_ints(O.FR381, proof.gamma) == [gamma]
    assert KZG.batch_verify(setup, commitments, opening, proof) is False          # a fresh transcript samples another gamma
    assert KZG.batch_verify(setup, commitments, opening, proof, transcript=tv) is True
    assert tp.sample_random_challenge() == tv.sample_random_challenge() == model.sample()


def level_points(zk, polys, setup, opening):
    return [zk.MultilinearKZG.open_and_prove(f, setup, opening) for f in polys]


def test_batch_open_2p20_vs_single_openings(zk):
    """2^20, k = 4: every batched proof point is sum_j gamma^j (the same level's point of zk_kzg_open of f_j); the same with the
    opening key's levels precomputed; batch_verify accepts and rejects a tampered evaluation"""
    MP, KZG = zk.MultilinearPolynomial, zk.MultilinearKZG
    n, k = 20, 4
    setup = setup_for(zk, n, 2020)
    polys = [MP.random(0, 1 << n, 0x2020 + j) for j in range(k)]
    commitments = np.stack([KZG.commit_to_polynomial(f, setup) for f in polys])
    opening = host_random(zk, 0, n, 2021)
    proof = KZG.batch_open_and_prove(polys, setup, opening, commitments)
    singles = level_points(zk, polys, setup, opening)
    powers = [O.from_ints(O.FR381, [pow(O.to_ints(O.FR381, proof.gamma)[0], j, R)])[0] for j in range(k)]
    for i in range(n):
        acc = np.zeros(12, np.uint64)
        for j in range(k):
            acc = O.g1_add(acc, O.g1_mul_fr(singles[j].proofs[i], powers[j]))
        assert O.g1_affine_ints(acc) == O.g1_affine_ints(proof.proofs[i]), i
    for j in range(k):
        assert np.array_equal(singles[j].evaluation, proof.evaluations[j])
    assert KZG.batch_verify(setup, commitments, opening, proof) is True
    bad = proof.evaluations.copy()
    bad[2] = O.from_ints(O.FR381, [O.to_ints(O.FR381, bad[2])[0] + 1])[0]
    assert KZG.batch_verify(setup, commitments, opening, zk.MultilinearKZGBatchProof(bad, proof.gamma, proof.proofs)) is False
    setup.precompute_for_opens(min_points=1 << 16)
    pre = KZG.batch_open_and_prove(polys, setup, opening, commitments)
    assert np.array_equal(pre.proofs, proof.proofs) and np.array_equal(pre.gamma, proof.gamma)


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as G
zk = G.import_package()
from zkmle_amd import _lib
_lib.check(zk.lib().zk_init(0))
MP, KZG = zk.MultilinearPolynomial, zk.MultilinearKZG
n, k = 14, 3
taus = zk.from_ints(0, [3 + 7 * i for i in range(n)])
setup = zk.TrustedSetup.initialize_setup(taus)
polys = [MP.random(0, 1 << n, 1400 + j) for j in range(k)]
cs = np.stack([KZG.commit_to_polynomial(f, setup) for f in polys])
opening = zk.from_ints(0, [11 + 13 * i for i in range(n)])
pr = KZG.batch_open_and_prove(polys, setup, opening, cs)
print(json.dumps({"proofs": pr.proofs.tolist(), "gamma": pr.gamma.tolist(), "ok": KZG.batch_verify(setup, cs, opening, pr)}))
"""


def test_batch_open_same_proof_on_every_path(zk):
    """the same proof on a non-blocking user stream (zk_set_stream), and with the level MSMs on the caller's thread
    (ZK_KZG_OPEN_THREADS=1, read once per process: a child process) against the default three threads"""
    import torch
    MP, KZG = zk.MultilinearPolynomial, zk.MultilinearKZG
    n, k = 14, 3
    setup = zk.TrustedSetup.initialize_setup(zk.from_ints(0, [3 + 7 * i for i in range(n)]))
    polys = [MP.random(0, 1 << n, 1400 + j) for j in range(k)]
    cs = np.stack([KZG.commit_to_polynomial(f, setup) for f in polys])
    opening = zk.from_ints(0, [11 + 13 * i for i in range(n)])
    base = KZG.batch_open_and_prove(polys, setup, opening, cs)
    assert KZG.batch_verify(setup, cs, opening, base) is True
    st = torch.cuda.Stream()
    L = zk.lib()
    L.zk_set_stream.argtypes = [C.c_void_p]
    assert L.zk_set_stream(C.c_void_p(st.cuda_stream)) == 0
    try:
        on_stream = KZG.batch_open_and_prove(polys, setup, opening, cs)
    finally:
        assert L.zk_set_stream(None) == 0
    assert np.array_equal(on_stream.proofs, base.proofs) and np.array_equal(on_stream.evaluations, base.evaluations)
    env = dict(os.environ, ZK_KZG_OPEN_THREADS="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    v = json.loads(r.stdout.strip().splitlines()[-1])
    assert v["ok"] is True
    assert np.array_equal(np.array(v["proofs"], np.uint64), base.proofs) and np.array_equal(np.array(v["gamma"], np.uint64), base.gamma)
