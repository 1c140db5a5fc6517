"""GPU parity: basic sumcheck and GKR sumcheck provers (proof bytes identical to the oracle's),
mirroring sumcheck_protocol/src/basic_sumcheck/protocol.rs and gkr_sumcheck/sumcheck_gkr_protocol.rs tests."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import oracle as O

pytestmark = pytest.mark.gpu
FID = {"bn254_fq": 2, "bls12_381_fr": 0}


@pytest.fixture(scope="module")
def zk():
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    return zk


def rand_table(zk, field, n, seed):
    t = np.zeros((n, zk.limbs(field)), np.uint64)
    assert zk.lib().zk_host_fill_random(field, seed, 0, n, t.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
    return t


def test_prover_init_claimed_sums(zk, ref_kats):
    for k in ref_kats["basic_sumcheck_claimed_sum"]:          # prover.rs:99-107, protocol.rs:10-26
        f = FID[k["field"]]
        prover = zk.Prover.init(f, zk.from_ints(f, k["table"]))
        assert zk.to_ints(f, prover.initial_claimed_sum) == [k["expect"]]
        assert prover.is_initialized is True
        assert prover.initial_polynomial.to_ints() == k["table"]
    with pytest.raises(zk.ReferencePanic, match="Can't prove without init"):
        zk.Prover().prove()


def test_basic_sumcheck_reference_roundtrips(zk, ref_kats):
    for k in ref_kats["basic_sumcheck_roundtrip"]:            # protocol.rs:28-116
        f = FID[k["field"]]
        if "table" in k:
            table = zk.from_ints(f, k["table"])
        else:                                                 # vec![Fr::from(3); 1 << 20]  protocol.rs:42-44 (full size here)
            table = np.tile(zk.from_ints(f, [k["table_constant"]]), (1 << k["log_len"], 1))
        prover = zk.Prover.init(f, table)
        proof = prover.prove()
        assert zk.Verifier.init().verify(proof) is True, k["src"]
        if len(table) <= (1 << 12):
            cs, rp, ch = O.sumcheck_basic_prove(f, table)
            assert np.array_equal(proof.initial_claimed_sum, cs)
            assert np.array_equal(proof.round_univariate_polynomials, rp)
            assert np.array_equal(prover.challenges, ch)
        bad = zk.sumcheck.SumcheckProof(proof.initial_polynomial, proof.initial_claimed_sum,
                                        proof.round_univariate_polynomials.copy())
        bad.round_univariate_polynomials[0, 0, 0] ^= np.uint64(1)
        assert zk.Verifier.init().verify(bad) is False


def test_basic_sumcheck_derived_vectors(zk, derived_kats):
    for d in derived_kats["basic_sumcheck"]:
        f = FID[d["field"]]
        prover = zk.Prover.init(f, zk.from_ints(f, d["table"]))
        proof = prover.prove()
        assert zk.to_ints(f, proof.initial_claimed_sum) == [int(d["claimed"], 16)]
        for got, exp in zip(proof.round_univariate_polynomials, d["rounds"]):
            assert zk.to_ints(f, got) == [int(x, 16) for x in exp]
        assert zk.to_ints(f, prover.challenges)[: len(d["challenges"])] == [int(x, 16) for x in d["challenges"]]


@pytest.mark.parametrize("field", [0, 1, 2, 3])
@pytest.mark.parametrize("logn", [0, 1, 2, 3, 7, 11, 12, 13, 14, 15, 16])    # 12..15: one pass of 1..4 rounds before the tail (basic_multi.cuh)
def test_basic_sumcheck_random_vs_oracle(zk, field, logn):
    table = rand_table(zk, field, 1 << logn, 1000 + logn)
    prover = zk.Prover.init(field, table)
    proof = prover.prove()
    cs, rp, ch = O.sumcheck_basic_prove(field, table)
    assert np.array_equal(proof.initial_claimed_sum, cs)
    assert np.array_equal(proof.round_univariate_polynomials.reshape(rp.shape), rp)
    assert np.array_equal(prover.challenges.reshape(ch.shape), ch)
    assert zk.Verifier.init().verify(proof) is True


@pytest.mark.parametrize("field,logn", [(0, 3), (0, 13), (2, 16)])
def test_prover_transcript_field_ends_where_the_reference_leaves_it(zk, field, logn):
    """`Prover { transcript, .. }` is a public field the reference's prove() appends to (prover.rs:10, :38-58): after prove() it has absorbed
    the table, the claimed sum and every round message, and has sampled every challenge.  Replayed here append by append on a second
    transcript (fiat_shamir_transcript.rs:22-43): both must give the same next sample -- and so must a prover whose transcript had already
    absorbed something (zk_sumcheck_basic_prove_on runs on the caller's sponge)."""
    table = rand_table(zk, field, 1 << logn, 4000 + logn)
    for prefix in (b"", b"state the caller left"):
        prover = zk.Prover.init(field, table)
        replay = zk.Transcript()
        if prefix:
            prover.transcript.append(prefix)
            replay.append(prefix)
        proof = prover.prove()
        replay.append(prover.initial_polynomial.convert_to_bytes())                       # :38-39
        replay.append(O.fe_to_bytes_be(field, proof.initial_claimed_sum))                 # :40-41
        for k in range(logn):
            replay.append(O.fe_to_bytes_be(field, proof.round_univariate_polynomials[k, 0]) +
                          O.fe_to_bytes_be(field, proof.round_univariate_polynomials[k, 1]))   # :51-55
            assert np.array_equal(replay.random_challenge_as_field_element(field), prover.challenges[k])   # :58
        assert prover.transcript.sample_random_challenge() == replay.sample_random_challenge()
        if not prefix:
            cs, rp, _ = O.sumcheck_basic_prove(field, table)
            assert np.array_equal(proof.initial_claimed_sum, cs) and np.array_equal(proof.round_univariate_polynomials.reshape(rp.shape), rp)


def test_basic_sumcheck_config2_2p20_random(zk):
    """BASELINE config 2 size (20 variables, random table): proof equals the oracle's"""
    field, logn = 0, 20
    table = rand_table(zk, field, 1 << logn, 0x5EED0002)
    prover = zk.Prover.init(field, table)
    proof = prover.prove()
    cs, rp, ch = O.sumcheck_basic_prove(field, table)
    assert np.array_equal(proof.initial_claimed_sum, cs)
    assert np.array_equal(proof.round_univariate_polynomials, rp)
    assert zk.Verifier.init().verify(proof) is True


def mk_sum(zk, f, products):
    MP = zk.MultilinearPolynomial
    return zk.SumPolynomial([zk.ProductPolynomial([MP(f, t) for t in prod]) for prod in products])


def test_composed_polynomial_reference_kats(zk, ref_kats):
    MP = zk.MultilinearPolynomial
    k = ref_kats["product_poly"]
    f = FID[k["field"]]
    pp = zk.ProductPolynomial([MP.from_ints(f, t) for t in k["polys"]])
    assert zk.to_ints(f, pp.evaluate(zk.from_ints(f, k["evaluate"]["values"]))) == [k["evaluate"]["expect"]]
    pe = k["partial_evaluate"]
    assert [p.to_ints() for p in pp.partial_evaluate(pe["var"], zk.from_ints(f, [pe["value"]])[0])] == pe["expect"]
    assert pp.multiply_polynomials_element_wise().to_ints() == k["multiply_element_wise"]
    assert pp.degree() == k["degree"]
    with pytest.raises(zk.ReferencePanic, match="different number of variables"):
        zk.ProductPolynomial([MP.from_ints(f, t) for t in k["new_panics"]["polys"]])
    s = ref_kats["sum_poly"]
    sp = zk.SumPolynomial([zk.ProductPolynomial([MP.from_ints(f, t) for t in prod]) for prod in s["products"]])
    assert zk.to_ints(f, sp.evaluate(zk.from_ints(f, s["evaluate"]["values"]))) == [s["evaluate"]["expect"]]
    assert sp.add_polynomials_element_wise().to_ints() == s["add_element_wise"]
    assert sp.degree() == s["degree"] and sp.number_of_variables() == s["number_of_variables"]
    pe = s["partial_evaluate"]
    folded = sp.partial_evaluate(pe["var"], zk.from_ints(f, [pe["value"]])[0])
    assert [[p.to_ints() for p in pp_.polynomials] for pp_ in folded.product_polynomials] == pe["expect"]
    with pytest.raises(zk.ReferencePanic, match="different number of variables"):   # sum_polynomial.rs:101-113
        zk.SumPolynomial([zk.ProductPolynomial([MP.from_ints(f, [0, 2])]), zk.ProductPolynomial([MP.from_ints(f, [0, 0, 0, 3])])])
    with pytest.raises(zk.ReferencePanic):
        zk.SumPolynomial([pp]).add_polynomials_element_wise()


def test_gkr_round_univariate_and_roundtrip(zk, ref_kats, derived_kats):
    for k in ref_kats["gkr_round_univariate"]:               # sumcheck_gkr_protocol.rs:163-186
        f = FID[k["field"]]
        sp = mk_sum(zk, f, [[zk.from_ints(f, t) for t in prod] for prod in k["products"]])
        assert zk.to_ints(f, zk.sumcheck.generate_round_univariate(sp)) == k["expect"]
    for k in ref_kats["gkr_sumcheck_roundtrip"]:             # :188-212
        f = FID[k["field"]]
        sp = mk_sum(zk, f, [[zk.from_ints(f, t) for t in prod] for prod in k["products"]])
        result = zk.sumcheck.prove(sp, zk.from_ints(f, [k["claimed_sum"]])[0], zk.Transcript.new())
        verified = zk.sumcheck.verify(result, zk.Transcript.new(), f)
        assert verified.is_proof_valid is True
        assert np.array_equal(verified.random_challenges, result.random_challenges)
        assert np.array_equal(sp.evaluate(result.random_challenges), verified.last_claimed_sum)
    d = derived_kats["gkr_sumcheck"]
    f = FID[d["field"]]
    sp = mk_sum(zk, f, [[zk.from_ints(f, t) for t in prod] for prod in d["products"]])
    result = zk.sumcheck.prove(sp, zk.from_ints(f, [d["claimed"]])[0], zk.Transcript.new())
    assert [zk.to_ints(f, r) for r in result.round_univariate_polynomials] == [[int(x, 16) for x in r] for r in d["coeffs"]]
    assert zk.to_ints(f, result.random_challenges) == [int(x, 16) for x in d["challenges"]]
    bad = zk.sumcheck.verify(zk.sumcheck.SumcheckProverProof(zk.from_ints(f, [13])[0], result.round_univariate_polynomials,
                                                            result.random_challenges), zk.Transcript.new(), f)
    assert bad.is_proof_valid is False


@pytest.mark.parametrize("field", [0, 2])
@pytest.mark.parametrize("shape", [(2, 2, 1), (2, 2, 2), (2, 2, 5), (2, 2, 11), (3, 2, 6), (2, 3, 6), (1, 2, 4), (4, 3, 3), (2, 1, 4),
                                   (3, 2, 13), (2, 3, 12), (8, 2, 12)])   # > 2^11 entries: producer + finish kernels before the tail
def test_gkr_sumcheck_random_vs_oracle(zk, field, shape):
    nprod, nfac, logn = shape
    n = 1 << logn
    tabs = np.stack([np.stack([rand_table(zk, field, n, 50 * p + f + logn) for f in range(nfac)]) for p in range(nprod)])
    sp = mk_sum(zk, field, tabs)
    if nprod < 2 or nfac < 2:      # add_polynomials_element_wise asserts "> 1" (sum_polynomial.rs:58-61, product_polynomial.rs:59-62)
        with pytest.raises(O.OraclePanic):
            O.gkr_round_univariate(field, tabs)
        with pytest.raises(zk.ReferencePanic):
            zk.sumcheck.generate_round_univariate(sp)
        with pytest.raises(zk.ReferencePanic):
            zk.sumcheck.prove(sp, rand_table(zk, field, 1, 5)[0], zk.Transcript())
        return
    assert np.array_equal(zk.sumcheck.generate_round_univariate(sp), O.gkr_round_univariate(field, tabs))
    if nprod >= 2 and nfac >= 2:
        red = O.sumpoly_reduce(field, tabs)
        assert np.array_equal(sp.add_polynomials_element_wise().evaluated_values, red)
        claimed = O.vec_sum(field, red)
    else:
        claimed = rand_table(zk, field, 1, 5)[0]
    if nprod >= 2 and nfac >= 2:
        t_gpu, t_cpu = zk.Transcript(), O.Transcript()
        t_gpu.append(b"prefix")
        t_cpu.append(b"prefix")
        result = zk.sumcheck.prove(sp, claimed, t_gpu)
        co, ch = O.sumcheck_gkr_prove(field, tabs, claimed, t_cpu)
        assert np.array_equal(result.round_univariate_polynomials, co)
        assert np.array_equal(result.random_challenges, ch)
        assert t_gpu.sample_random_challenge() == t_cpu.sample_random_challenge()   # transcripts stay in lock-step
        # inputs untouched (the reference clones, :33)
        assert np.array_equal(sp.product_polynomials[0].polynomials[0].evaluated_values, tabs[0, 0])
        tv = zk.Transcript()
        tv.append(b"prefix")
        v = zk.sumcheck.verify(result, tv, field)
        assert v.is_proof_valid and np.array_equal(v.last_claimed_sum, sp.evaluate(ch))


def test_gkr_sumcheck_large_2p20(zk):
    """4 tables of 2^20 (f(b,c) of a layer with 2^10 wires): proof equals the oracle's"""
    field, n = 2, 1 << 20
    MP = zk.MultilinearPolynomial
    tabs = np.stack([np.stack([MP.random(field, n, 70 + 2 * p + f).evaluated_values for f in range(2)]) for p in range(2)])
    sp = mk_sum(zk, field, tabs)
    claimed = O.vec_sum(field, O.sumpoly_reduce(field, tabs))
    result = zk.sumcheck.prove(sp, claimed, zk.Transcript())
    co, ch = O.sumcheck_gkr_prove(field, tabs, claimed, O.Transcript())
    assert np.array_equal(result.round_univariate_polynomials, co) and np.array_equal(result.random_challenges, ch)


@pytest.mark.gpu
@pytest.mark.parametrize("field", [0, 1, 3])
def test_device_transcript_any_sponge_fill(zk, field):
    """The rounds run against a sponge that lives on the device (csrc/dev_transcript.cuh).  Whatever the host absorbed
    before -- any length mod 4 (byte-granular path) and mod 136 (block boundary inside the message, inside the digest,
    exactly at the end) -- proof, challenges and the sponge handed back must equal the oracle's."""
    n = 1 << 3
    tabs = np.stack([np.stack([rand_table(zk, field, n, 900 + 2 * p + f) for f in range(2)]) for p in range(2)])
    sp = mk_sum(zk, field, tabs)
    claimed = O.vec_sum(field, O.sumpoly_reduce(field, tabs))
    for plen in [0, 1, 2, 3, 4, 5, 7, 8, 39, 40, 41, 63, 100, 103, 104, 105, 131, 132, 133, 134, 135, 136, 137, 271, 272, 273]:
        prefix = bytes((7 * i + plen) & 0xFF for i in range(plen))
        t_gpu, t_cpu = zk.Transcript(), O.Transcript()
        t_gpu.append(prefix)
        t_cpu.append(prefix)
        result = zk.sumcheck.prove(sp, claimed, t_gpu)
        co, ch = O.sumcheck_gkr_prove(field, tabs, claimed, t_cpu)
        assert np.array_equal(result.round_univariate_polynomials, co), plen
        assert np.array_equal(result.random_challenges, ch), plen
        t_gpu.append(b"\x01\x02\x03")                     # the host sponge continues from the device state
        t_cpu.append(b"\x01\x02\x03")
        assert t_gpu.sample_random_challenge() == t_cpu.sample_random_challenge(), plen
    st = zk.sumcheck.last_stats()
    assert st["rounds"] == 3 and st["ms_rounds"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("field,logn", [(1, 13), (3, 12)])
def test_sumcheck_provers_other_fields_beyond_the_tail(zk, field, logn):
    """12-limb (BLS12-381 Fq) and BN254 Fr tables larger than the tail kernel's 2^11 entries: the two-launch rounds
    (fold_round_evals / fold_half_sums + sumcheck_finish_kernel) and the hand-over to the tail, against the oracle"""
    n = 1 << logn
    tabs = np.stack([np.stack([rand_table(zk, field, n, 700 + 2 * p + f) for f in range(2)]) for p in range(2)])
    sp = mk_sum(zk, field, tabs)
    claimed = O.vec_sum(field, O.sumpoly_reduce(field, tabs))
    t_gpu, t_cpu = zk.Transcript(), O.Transcript()
    result = zk.sumcheck.prove(sp, claimed, t_gpu)
    co, ch = O.sumcheck_gkr_prove(field, tabs, claimed, t_cpu)
    assert np.array_equal(result.round_univariate_polynomials, co) and np.array_equal(result.random_challenges, ch)
    assert t_gpu.sample_random_challenge() == t_cpu.sample_random_challenge()
    table = tabs[0, 0]
    proof = zk.Prover.init(field, zk.MultilinearPolynomial(field, table)).prove()
    cs, rp, _ = O.sumcheck_basic_prove(field, table)
    assert np.array_equal(proof.initial_claimed_sum, cs) and np.array_equal(proof.round_univariate_polynomials, rp)


@pytest.mark.gpu
def test_two_host_threads_prove_concurrently(zk):
    """Distinct handles may be driven from different threads (include/zkmle.h): reduction partials, staging buffers and the
    per-call statistics are per thread, the caching pool is locked.  Two threads prove different statements at the same
    time, each on its own stream (ctypes drops the GIL inside the library); every proof must still equal the oracle's."""
    import threading
    field = 0
    jobs = []
    for k in range(2):
        n = 1 << (12 + k)
        tabs = np.stack([np.stack([rand_table(zk, field, n, 1300 + 10 * k + 2 * p + f) for f in range(2)]) for p in range(2)])
        claimed = O.vec_sum(field, O.sumpoly_reduce(field, tabs))
        co, ch = O.sumcheck_gkr_prove(field, tabs, claimed, O.Transcript())
        cs, rp, _ = O.sumcheck_basic_prove(field, tabs[0, 0])
        jobs.append((tabs, claimed, co, ch, cs, rp))
    errors = []
    import ctypes as C
    import torch
    lib = zk.lib()
    lib.zk_set_stream.argtypes = [C.c_void_p]
    lib.zk_get_stream.restype = C.c_void_p
    streams = [torch.cuda.Stream() for _ in jobs]           # each thread drives its own HIP stream (zk_set_stream)

    def work(job, stream):
        tabs, claimed, co, ch, cs, rp = job
        try:
            lib.zk_set_stream(C.c_void_p(stream.cuda_stream))
            assert (lib.zk_get_stream() or 0) == stream.cuda_stream
            for _ in range(5):
                sp = mk_sum(zk, field, tabs)
                res = zk.sumcheck.prove(sp, claimed, zk.Transcript())
                assert np.array_equal(res.round_univariate_polynomials, co) and np.array_equal(res.random_challenges, ch)
                proof = zk.Prover.init(field, zk.MultilinearPolynomial(field, tabs[0, 0])).prove()
                assert np.array_equal(proof.initial_claimed_sum, cs) and np.array_equal(proof.round_univariate_polynomials, rp)
        except Exception as e:      # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(j, st)) for j, st in zip(jobs, streams)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


@pytest.mark.gpu
def test_full_size_provers_size_independent_properties(zk):
    """BASELINE config 5 sizes, checked by the verifier's side of the protocol (the byte-for-byte comparison of these sizes with the
    oracle lives in tests/test_gpu_full_size_parity.py): a 2^24 basic sumcheck proof passes the verifier's round
    equations (p_k(0) + p_k(1) = previous claim, verifier.rs:47-64) recomputed here on the host with the oracle's field
    arithmetic, its last claim equals the table's evaluation at the challenges (:67-70, GPU evaluate cross-checked by a
    second, unfused fold chain), and a tampered round is rejected.  Same for a GKR sumcheck on 4 tables of 2^22."""
    field = 0
    p = O.modulus(field)
    poly = zk.MultilinearPolynomial.random(field, 1 << 24, 0x5EED0005)
    prover = zk.Prover.init(field, poly)
    proof = prover.prove()
    rp = [zk.to_ints(field, r) for r in proof.round_univariate_polynomials]
    claim = zk.to_ints(field, proof.initial_claimed_sum)[0]
    ch = zk.to_ints(field, prover.challenges)
    assert len(rp) == 24
    for (e0, e1), r in zip(rp, ch):
        assert (e0 + e1) % p == claim
        claim = (e0 + r * (e1 - e0)) % p
    assert zk.to_ints(field, poly.evaluate(prover.challenges))[0] == claim
    cur = poly                                                     # the same evaluation through 24 separate fold launches
    for r in prover.challenges:
        cur = zk.MultilinearPolynomial.partial_evaluate(cur, 0, r)
    assert zk.to_ints(field, cur.evaluated_values)[0] == claim
    assert zk.Verifier.init().verify(proof) is True
    bad = proof.round_univariate_polynomials.copy()
    bad[7, 0, 0] ^= np.uint64(1)
    assert zk.Verifier.init().verify(zk.sumcheck.SumcheckProof(proof.initial_polynomial, proof.initial_claimed_sum, bad)) is False
    del poly, proof, prover, cur
    n = 1 << 22
    tabs = [[zk.MultilinearPolynomial.random(field, n, 0x5EED0400 + 2 * q + f) for f in range(2)] for q in range(2)]
    sp = zk.SumPolynomial([zk.ProductPolynomial(t) for t in tabs])
    claimed = sp.add_polynomials_element_wise().sum()
    res = zk.sumcheck.prove(sp, claimed, zk.Transcript())
    v = zk.sumcheck.verify(res, zk.Transcript(), field)
    assert v.is_proof_valid and np.array_equal(v.last_claimed_sum, sp.evaluate(res.random_challenges))
    co = res.round_univariate_polynomials.copy()
    co[3, 1, 0] ^= np.uint64(1)
    bad = zk.sumcheck.SumcheckProverProof(res.claimed_sum, co, res.random_challenges)
    assert not zk.sumcheck.verify(bad, zk.Transcript(), field).is_proof_valid


@pytest.mark.gpu
@pytest.mark.parametrize("field,logn,consts", [(0, 1, (1, 1)), (0, 3, (0, 1)), (0, 7, (1, 1)), (0, 11, (0, 1)), (0, 12, (1, 0)), (0, 14, (0, 1)),
                                               (0, 17, (0, 1)), (0, 18, (1, 1)), (2, 13, (0, 1)), (1, 9, (0, 1)), (1, 13, (1, 0)), (3, 16, (0, 1))])
def test_gkr_rounds_with_constant_factors_vs_oracle(zk, field, logn, consts):
    """zk_sumcheck_gkr_rounds_cf: a product whose second factor is a constant never materialises that table (the sparse GKR prover's
    W H1 + H0 * 1 and C W + A * u).  Coefficients, challenges, final values and the sponge must equal the oracle's proof of the
    same SumPolynomial with the constant tables written out -- every kernel that takes the shortcut: tail (<= 2^11 entries, all
    three lane splits), split rounds, large fused rounds, 4- and 6-limb fields."""
    n = 1 << logn
    MP = zk.MultilinearPolynomial
    cvals = rand_table(zk, field, 2, 4000 + logn)
    cvals[1] = O.from_ints(field, [1])[0]
    full = np.stack([np.stack([MP.random(field, n, 3000 + 10 * logn + 2 * p + f).evaluated_values for f in range(2)]) for p in range(2)])
    for p in range(2):
        if consts[p]:
            full[p, 1] = cvals[p]
    tables = [(MP(field, full[p, 0]), None if consts[p] else MP(field, full[p, 1])) for p in range(2)]
    claimed = O.vec_sum(field, O.sumpoly_reduce(field, full))
    t_gpu, t_cpu = zk.Transcript(), O.Transcript()
    t_gpu.append(b"phase")
    t_cpu.append(b"phase")
    t_gpu.append(O.fe_to_bytes_be(field, claimed))                 # sumcheck_gkr_protocol.rs:35 (the rounds entry leaves it to the caller)
    co, ch, fin = zk.sumcheck.gkr_rounds_const_factors(field, tables, cvals, t_gpu)
    want_co, want_ch = O.sumcheck_gkr_prove(field, full, claimed, t_cpu)
    assert np.array_equal(co, want_co) and np.array_equal(ch, want_ch)
    assert t_gpu.sample_random_challenge() == t_cpu.sample_random_challenge()
    want_fin = np.stack([O.evaluate(field, full[p, f], want_ch) for p in range(2) for f in range(2)])
    assert np.array_equal(fin, want_fin)
