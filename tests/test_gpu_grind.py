"""GPU: the nonce search of the proof-of-work step (csrc/grind.cuh fri_grind_kernel, csrc/zkmle_grind.hip; include/zkmle.h "Proof-of-work
grinding") and the provers that take the step.  Everything is byte for byte.

  search    zk_transcript_grind equals zk_host_transcript_grind -- the GPU against the host's one-core search, whose definition
            tests/test_grind_cpu.py ties to the model -- in nonce and in the state the transcript is left in: every fill 0 .. 135 of the sponge's
            open block at 10 bits; bits in {1, 2, 8, 9, 15, 16, 17, 20} at the fills 0, 127 (the pad's two bytes meet in the last byte), 128 (the
            nonce ends the block), 129 and 135 (it straddles two); 256 candidates a launch with the hit dozens of launches in; 2 bits with the
            default batch, where a launch holds hits by the hundred thousand and the smallest must win; starts just below 2^32 and above 2^40
            (the nonce's high word, and the carry into it inside one launch); two searches in a row on one transcript
  fri       fri.prove(.., grinding_bits=g) at d = 6, b = 2, f = 1, Q = 8 on both fields: g = 0 gives zk_fri_prove's bytes; g = 9 equals the model
            of tests/_fri_model.py with the step of tests/_grind_model.py in every output and in the nonce, passes zk_fri_verify_pow, and draws
            other indices than g = 0
  batch     fri.open_multilinear_batch(.., grinding_bits=9) at d = 6, k in {1, 3}, P = 2 under the three schedules: byte for byte the model of
            tests/_fri_ml_batch_model.py with the step, through the verifier; g = 0 gives zk_fri_ml_open_batch's bytes

The transcripts are seeded.  The seeds below were chosen with the host search (and, for the proofs, the models) so that every nonce stays
below 2^(bits + 4) and the one-core side of a case costs a fraction of a second: no search here goes above 20 bits, where the search's own
cap of 2^(bits + 6) candidates bounds even a kernel that never finds anything to 2^26 hashes."""
import ctypes as C
import random

import numpy as np
import pytest

import _fri_ml_batch_model as BM
import _fri_ml_grouped_model as GM
import _fri_model as FM
import _fri_pcs_model as PM
import _grind_model as GR
import _merkle_model as MM
import _ntt_model as NM
from test_gpu_fri import table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
RATE = 136
EDGE_FILLS = (0, 127, 128, 129, 135)
EDGE_BITS = (1, 2, 8, 9, 15, 16, 17, 20)
# EDGE_SEEDS[bits][i]: the content seed at fill EDGE_FILLS[i]; nonces below min(2^(bits + 4), 2^18)
EDGE_SEEDS = {1: (0, 0, 0, 0, 0), 2: (0, 0, 0, 0, 0), 8: (0, 0, 0, 0, 0), 9: (0, 0, 0, 0, 0), 15: (0, 0, 0, 0, 0), 16: (0, 0, 0, 1, 0), 17: (0, 0, 0, 0, 0),
              20: (0, 2, 4, 4, 6)}
LAUNCHES_SEED = 0                                            # fill 40, 16 bits: the nonce lies in [2^13, 2^17), 32 launches of 256 and more
CARRY_SEED = 0                                               # fill 131, 12 bits from 2^32 - 3: the nonce is above 2^32
FRI_SEEDS = {0: 12, 3: 7}                                    # field -> the coefficients' seed: the model's nonce at 9 bits is below 40
# (log_arity, grouped, k) -> the points' seed: the model's nonce at 9 bits is below 20
BATCH_SEEDS = {(1, False, 1): 1, (1, False, 3): 26, (2, False, 1): 20, (2, False, 3): 42, (2, True, 1): 23, (2, True, 3): 240}
SCHEDULES = [(1, False), (2, False), (2, True)]              # (log_arity, grouped)
sched_id = lambda s: "a%d%s" % (s[0], "g" if s[1] else "")


def prior(fill, seed, blocks=0):
    """what the transcript holds before the step, sized so that the open block holds `fill` bytes once the 8-byte tag is in"""
    n = (fill - 8) % RATE + blocks * RATE
    return random.Random(7919 * seed + fill).randbytes(n)


def transcript(zk, data):
    t = zk.Transcript()
    t.append(data)
    return t


def gpu_equals_host(zk, data, bits, start=0, log_batch=0, bound=None):
    """one search on each side of the same transcript -> the nonce"""
    h, g = transcript(zk, data), transcript(zk, data)
    want = h.grind_host(bits, start)
    assert want - start < (bound if bound is not None else min(1 << (bits + 4), 1 << 18)), "the case's seed no longer keeps the nonce small"
    got = g.grind(bits, start, log_batch)
    assert got == want, (bits, start, log_batch, got, want)
    assert np.array_equal(g.export_state(), h.export_state())
    st = zk.fri.grind_last_stats()
    assert st["candidates"] == want - start + 1 and st["launches"] >= 1 and st["ms"] > 0
    return got


@pytest.mark.parametrize("part", range(4))
def test_every_fill_at_ten_bits(zk, part):
    for fill in range(part, RATE, 4):
        data = prior(fill, fill, blocks=fill % 3)
        assert int(transcript(zk, data + GR.tag(10)).export_state()[25]) == fill
        gpu_equals_host(zk, data, 10)


@pytest.mark.parametrize("bits", EDGE_BITS)
def test_the_fills_around_the_blocks_end(zk, bits):
    for fill, seed in zip(EDGE_FILLS, EDGE_SEEDS[bits]):
        gpu_equals_host(zk, prior(fill, seed), bits)


def test_a_hit_many_launches_in(zk):
    w = gpu_equals_host(zk, prior(40, LAUNCHES_SEED), 16, log_batch=8)
    assert w >= 1 << 13
    assert zk.fri.grind_last_stats()["launches"] == w // 256 + 1
    # the same nonce from one launch
    assert gpu_equals_host(zk, prior(40, LAUNCHES_SEED), 16, log_batch=20) == w
    assert zk.fri.grind_last_stats()["launches"] == 1


@pytest.mark.parametrize("fill", (40, 128, 131))
def test_the_smallest_of_very_many_hits_wins(zk, fill):
    for seed in range(4):
        gpu_equals_host(zk, prior(fill, seed), 2)


def test_the_nonces_high_word(zk):
    w = gpu_equals_host(zk, prior(131, CARRY_SEED), 12, start=(1 << 32) - 3)
    assert w >= 1 << 32                                      # the launch that started below 2^32 found it above
    for fill in (40, 128, 133):
        w = gpu_equals_host(zk, prior(fill, 3), 12, start=(1 << 40) + 1)
        assert w > 1 << 40
        gpu_equals_host(zk, prior(fill, 3), 12, start=(1 << 40) + 1, log_batch=8)
    # a start of which nothing is left: 2^64 - 1 is no candidate, on either side
    from zkmle_amd import _lib as L
    n = C.c_uint64(5)
    for fn, last in ((zk.lib().zk_transcript_grind, 0), (zk.lib().zk_host_transcript_grind, 0)):
        t = transcript(zk, b"end")
        before = t.export_state().copy()
        assert fn(t._h, 1, 2**64 - 1, last, C.byref(n)) == L.ZK_E_RANGE and n.value == 5 and np.array_equal(t.export_state(), before)


def test_two_searches_in_a_row(zk):
    data = prior(77, 1)
    h, g = transcript(zk, data), transcript(zk, data)
    for bits in (12, 10, 12):
        want = h.grind_host(bits)
        assert g.grind(bits) == want
        assert np.array_equal(g.export_state(), h.export_state())
    # ... and the verifier's steps end there too
    v = transcript(zk, data)
    for bits in (12, 10, 12):
        t = transcript(zk, b"")
        t.import_state(v.export_state())
        w = t.grind_host(bits)
        assert v.check_grind(bits, w)
    assert np.array_equal(v.export_state(), g.export_state())


# ---- the provers --------------------------------------------------------------------------------------------------------------------------
FRI_SHAPE = (6, 2, 1, 8)                                     # d, b, f, Q
G_BITS = 9


def fri_inputs(field, seed):
    d, b, f, Q = FRI_SHAPE
    coeffs = NM.random_ints(field, 1 << d, 31000 + 17 * field + seed)
    coset = random.Random(500 + field + seed).randrange(2, NM.MODULUS[field])
    return coeffs, coset


def fri_proof_arrays(pr):
    return (("roots", pr.roots), ("final", pr.final_coeffs), ("betas", pr.betas), ("indices", pr.query_indices), ("values", pr.query_values),
            ("paths", pr.query_paths))


@pytest.mark.parametrize("field", (0, 3))
def test_fri_prove_with_grinding(zk, field):
    d, b, f, Q = FRI_SHAPE
    R = d - f
    coeffs, coset = fri_inputs(field, FRI_SEEDS[field])
    cm = zk.from_ints(field, [coset])[0]
    poly = table_of(zk, field, coeffs)
    # g = 0: the bytes of zk_fri_prove
    old = zk.fri._run(zk.lib().zk_fri_prove, poly, d, b, f, Q, cm, None)
    plain = zk.fri.prove(poly, b, f, Q, cm, grinding_bits=0)
    assert (plain.grinding_bits, plain.pow_nonce) == (0, 0)
    for (name, x), (_, y) in zip(fri_proof_arrays(plain), fri_proof_arrays(old)):
        assert np.array_equal(x, y), name
    assert zk.fri.verify(plain)
    # g = 9: the model with the step in front of its first index
    hasher = MM.check_host_keccak(zk)
    mt = GR.PowTranscript(G_BITS, R)
    pr = FM.prove(field, coeffs, b, f, Q, coset, mt, hasher)
    assert mt.nonce < 40, "the case's seed no longer keeps the model's search short"
    got = zk.fri.prove(poly, b, f, Q, cm, grinding_bits=G_BITS)
    assert (got.grinding_bits, got.pow_nonce) == (G_BITS, mt.nonce)
    fl = FM.flat(zk, pr)
    for name, arr in fri_proof_arrays(got):
        assert arr.shape == fl[name].shape and np.array_equal(arr, fl[name]), name
    assert not np.array_equal(got.query_indices, plain.query_indices)
    assert np.array_equal(got.roots, plain.roots) and np.array_equal(got.final_coeffs, plain.final_coeffs)
    ok = C.c_int(-1)
    from zkmle_amd import _lib as L
    args = (field, d, b, f, Q, L.p64(cm), None, L.p8(got.roots), L.p64(got.final_coeffs), L.p64(got.query_values), L.p8(got.query_paths))
    assert zk.lib().zk_fri_verify_pow(*args, G_BITS, got.pow_nonce, C.byref(ok)) == 0 and ok.value == 1
    assert zk.lib().zk_fri_verify_pow(*args, G_BITS, got.pow_nonce + 1, C.byref(ok)) == 0 and ok.value == 0
    assert zk.lib().zk_fri_verify_pow(*args, 0, 0, C.byref(ok)) == 0 and ok.value == 0
    assert zk.fri.verify(got)
    st = zk.fri.grind_last_stats()
    assert st["candidates"] == mt.nonce + 1 and st["launches"] == 1
    # a caller's transcript ends where the verifier's does
    t, v = transcript(zk, b"before"), transcript(zk, b"before")
    mine = zk.fri.prove(poly, b, f, Q, cm, transcript=t, grinding_bits=G_BITS)
    assert zk.fri.verify(mine, transcript=v) and np.array_equal(t.export_state(), v.export_state())


BATCH_SHAPE = (6, 1, 1, 8, 2)                                # d, b, f, Q, P: R = 5, so arity 2 ends in a fold by 2


def batch_inputs(zk, sched, k, seed):
    d, b, f, Q, P = BATCH_SHAPE
    a, grouped = sched
    field = 0 if k == 1 else 3
    p = NM.MODULUS[field]
    coset = random.Random(61 + field).randrange(2, p)
    hasher = GM.check_host_keccak(zk)
    cms = []
    for j in range(k):
        coeffs = NM.random_ints(field, 1 << d, 41000 + 101 * j + field)
        cms.append(GM.commit(field, coeffs, b, coset, hasher) if grouped else PM.commit(field, coeffs, b, coset, hasher))
    rng = random.Random(977 * seed + 13 * k + a + 2 * grouped)
    pts = [[rng.randrange(p) for _ in range(d)] for _ in range(P)]
    return field, cms, pts, hasher


def opening_arrays(op):
    return (("ys", op.ys), ("gamma", op.gamma), ("polys", op.round_polys), ("roots", op.roots), ("final", op.final_table),
            ("challenges", op.challenges), ("indices", op.query_indices), ("values", op.query_values), ("paths", op.query_paths))


@pytest.mark.parametrize("k", (1, 3))
@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_open_multilinear_batch_with_grinding(zk, sched, k):
    d, b, f, Q, P = BATCH_SHAPE
    a, grouped = sched
    R = d - f
    field, cms, pts, hasher = batch_inputs(zk, sched, k, BATCH_SEEDS[a, grouped, k])
    pm = to_mont(zk, field, [v for z in pts for v in z]).reshape(P, d, 4)
    gcs = [zk.fri.commit(table_of(zk, field, cm["coeffs"]), b, zk.from_ints(field, [cm["coset"]])[0], log_group=cm.get("log_group", 0)) for cm in cms]
    try:
        roots = [gc.root for gc in gcs]
        # g = 0: the bytes of zk_fri_ml_open_batch
        old = zk.fri.FriMlBatchOpening(field, k, P, d, b, f, Q, gcs[0].coset, a, grouped)
        from zkmle_amd import _lib as L
        L.check(zk.lib().zk_fri_ml_open_batch(zk.fri._handles(gcs), k, L.p64(pm), P, f, Q, a, None, L.p64(old.ys), L.p64(old.gamma), L.p64(old.round_polys),
                                              L.p8(old.roots), L.p64(old.final_table), L.p64(old.challenges), L.p64(old.query_indices),
                                              L.p64(old.query_values), L.p8(old.query_paths)))
        plain = zk.fri.open_multilinear_batch(gcs, pm, f, Q, log_arity=a, grinding_bits=0)
        assert (plain.grinding_bits, plain.pow_nonce) == (0, 0)
        for (name, x), (_, y) in zip(opening_arrays(plain), opening_arrays(old)):
            assert np.array_equal(x, y), name
        assert zk.fri.verify_multilinear_batch(roots, pm, plain)
        # g = 9: the batch model with the step in front of its first index (gamma and the R round challenges come before)
        mt = GR.PowTranscript(G_BITS, 1 + R)
        op = BM.open_batch(cms, pts, f, Q, a, mt, hasher=hasher)
        assert mt.nonce < 20, "the case's seed no longer keeps the model's search short"
        got = zk.fri.open_multilinear_batch(gcs, pm, f, Q, log_arity=a, grinding_bits=G_BITS)
        assert (got.grinding_bits, got.pow_nonce) == (G_BITS, mt.nonce)
        fl = BM.flat(zk, op)
        for name, arr in opening_arrays(got):
            assert arr.shape == fl[name].shape and np.array_equal(arr, fl[name]), name
        assert not np.array_equal(got.query_indices, plain.query_indices)
        assert zk.fri.verify_multilinear_batch(roots, pm, got)
        got.pow_nonce += 1
        assert not zk.fri.verify_multilinear_batch(roots, pm, got)
        got.pow_nonce -= 1
        got.grinding_bits = G_BITS + 1
        assert not zk.fri.verify_multilinear_batch(roots, pm, got)
        got.grinding_bits = 0
        assert not zk.fri.verify_multilinear_batch(roots, pm, got)
    finally:
        for gc in gcs:
            gc.free()
