"""GPU: the multilinear opening of a FRI commitment at several points (csrc/fri_ml.cuh fri_ml_round_w_kernel, csrc/zkmle_fri_ml.hip) and the
succinct sparse GKR proof that ends in it (csrc/zkmle_gkr_sparse.hip), over BLS12-381 Fr and BN254 Fr.  Everything compares byte for byte
with the Python model (tests/_fri_ml_points_model.py) or with the library's own independent paths; no tolerance anywhere.

  round      zk_fri_ml_round = the model's integers for both fields and both forms (r = NULL: nothing folded; r given: T and W folded first),
             table lengths 2^1 .. 2^15 (one lane, under a wave, one workgroup of 256 lanes, two -- a table is a power of two, so "just over
             one" is two -- and up to 64 workgroups per reduction),
             r = 0, 1, p - 1 and random, W all zero and W with entries p - 1
  stride     the second trip of the grid-stride loops of both round passes, fri_ml_round_w_kernel and the one-point opening's
             fri_ml_round_kernel: one child process (tests/_fri_ml_worker.py) with ZK_REDUCE_BLOCKS=64
  open       every output equals the model's at d = 1 .. 10, b = 1, 2, P = 1, 2, 3, both fields, with and without a coset (f among 0, 1,
             d - 1); once at d = 15 and once with P = 8; ys = zk_mle_evaluate at each point; a caller's transcript; argument errors
  gkr        sparse_prove_succinct / sparse_verify_succinct on both fields: the reference shape at depth 3 and a random wide circuit with
             in_bits between 6 and 10; the challenges equal the replay of the schedule (root first); input_evals = evaluate(inputs, rb / rc);
             one flipped bit of the root, of input_evals or of a layer coefficient is rejected, and so is a proof for other inputs shown with
             the first root; gkr.sparse_verify on an ordinary proof is unchanged"""
import copy
import functools
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import _fri_ml_cases as FC
import _fri_ml_points_model as PT
import _ntt_model as NM
from oracle import pymodel as M
from test_gpu_fri import hasher_for, table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (0, 3)


def elem(zk, field, v):
    return zk.from_ints(field, [v])[0]


# ---- the round pass --------------------------------------------------------------------------------------------------------------------
def check_round(zk, field, T, W, rs):
    p = NM.MODULUS[field]
    tt, wt = table_of(zk, field, T), table_of(zk, field, W)
    assert np.array_equal(zk.fri.ml_round(tt, wt), to_mont(zk, field, PT.round_g3(T, W, p))), "round 0's form"
    if len(T) < 4:
        return
    for r in rs:
        to, wo, g3 = zk.fri.ml_round(tt, wt, elem(zk, field, r))
        T1, W1 = PT.ML.mle_fold_last(field, T, r), PT.ML.mle_fold_last(field, W, r)
        assert np.array_equal(to.evaluated_values, to_mont(zk, field, T1)) and np.array_equal(wo.evaluated_values, to_mont(zk, field, W1)), r
        assert np.array_equal(g3, to_mont(zk, field, PT.round_g3(T1, W1, p))), r
    assert np.array_equal(tt.evaluated_values, to_mont(zk, field, T)) and np.array_equal(wt.evaluated_values, to_mont(zk, field, W))   # only read


@pytest.mark.parametrize("loglen", range(1, 16))
@pytest.mark.parametrize("field", FIELDS)
def test_round_pass_equals_the_models_integers(zk, field, loglen):
    """FOLD = false covers q = len / 2 lanes, FOLD = true q = len / 4: 1 lane .. 2^14 (64 workgroups)"""
    p, n = NM.MODULUS[field], 1 << loglen
    rng = random.Random(31 * loglen + field)
    T, W = NM.random_ints(field, n, 1200 + loglen + field), NM.random_ints(field, n, 2200 + loglen + field)
    rs = (0, 1, p - 1, rng.randrange(2, p - 1)) if loglen <= 12 else (p - 1, rng.randrange(2, p - 1))
    check_round(zk, field, T, W, rs)


@pytest.mark.parametrize("field", FIELDS)
def test_round_pass_at_operands_random_tables_never_reach(zk, field):
    p = NM.MODULUS[field]
    rng = random.Random(77 + field)
    for loglen in (2, 6, 10, 11):                            # lanes with / without r: 1 / 2, 16 / 32, 256 / 512, 512 / 1024 (one, two, four workgroups)
        n = 1 << loglen
        T = NM.random_ints(field, n, 3200 + loglen + field)
        edge = [rng.choice((0, p - 1, p - 1, rng.randrange(p))) for _ in range(n)]
        for W in ([0] * n, [p - 1] * n, edge):
            check_round(zk, field, T, W, (p - 1, rng.randrange(2, p - 1)))
        check_round(zk, field, [p - 1] * n, [p - 1] * n, (p - 1, 1))


def test_the_second_trip_of_the_grid_stride_loops():
    e = dict(os.environ, ZK_REDUCE_BLOCKS="64")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_fri_ml_worker.py")], capture_output=True, text=True, env=e, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["blocks"] == 64, out
    assert out["trips"] == {"round_w round0": 2, "round_w fold": 2, "round round0": 4, "round fold": 2}, out
    assert out["mismatches"] == [] and out["checked"] == 15, out


# ---- the opening -----------------------------------------------------------------------------------------------------------------------
coset_of = functools.partial(FC.coset_of, mul=61)
gpu_commitment = FC.gpu_commitment


@functools.lru_cache(maxsize=None)
def model_commitment(zk, field, d, b, with_coset):
    return FC.commitment(field, d, b, coset_of(field, d, b, with_coset), 9100 + 17 * d + b + field, hasher_for(zk, 2 << (d + b)))


def assert_same_opening(zk, got, op):
    fl = PT.flat(zk, op)
    for name, arr in (("ys", got.ys), ("gamma", got.gamma), ("polys", got.round_polys), ("roots", got.roots), ("final", got.final_table),
                      ("challenges", got.challenges), ("indices", got.query_indices), ("values", got.query_values), ("paths", got.query_paths)):
        assert arr.shape == fl[name].shape and np.array_equal(arr, fl[name]), name


def points_for(field, d, P, seed):
    p, rng = NM.MODULUS[field], random.Random(seed)
    pts = [[rng.randrange(p) for _ in range(d)] for _ in range(P)]
    if d >= 3:
        pts[0][1], pts[0][d - 1] = rng.choice((0, 1)), p - 1
    if P == 3:
        pts[2] = list(pts[1])                                # equal points are allowed
    return pts


def check_opening(zk, field, d, b, f, P, with_coset, Q=8):
    p = NM.MODULUS[field]
    cm = model_commitment(zk, field, d, b, with_coset)
    pts = points_for(field, d, P, d * 1000 + b * 100 + f * 10 + P + field)
    op = PT.open_points(cm, pts, f, Q, hasher=hasher_for(zk, 2 << (d + b)))
    pm = to_mont(zk, field, [v for z in pts for v in z]).reshape(P, d, 4)
    with gpu_commitment(zk, cm) as gc:
        assert gc.root == cm["root"]
        codeword_before = gc.codeword().evaluated_values
        got = zk.fri.open_multilinear_points(gc, pm, f, Q)
        assert_same_opening(zk, got, op)
        T = table_of(zk, field, cm["coeffs"])
        for k in range(P):
            assert np.array_equal(got.ys[k], T.evaluate(pm[k])), k
        assert got.roots[0].tobytes() == gc.root
        assert zk.fri.verify_multilinear_points(gc.root, pm, got)
        assert np.array_equal(gc.codeword().evaluated_values, codeword_before)
        again = zk.fri.open_multilinear_points(gc, pm, f, Q)   # the commitment's tables were only read: the same proof comes out again
        assert_same_opening(zk, again, op)
        st = zk.fri.ml_last_stats()
        assert st["rounds"] == d - f and st["queries"] == Q
    for k in range(P):
        bad = copy.copy(got)
        bad.ys = got.ys.copy()
        bad.ys[k] = to_mont(zk, field, [(op["ys"][k] + 1) % p])[0]
        assert not zk.fri.verify_multilinear_points(cm["root"], pm, bad), k


@pytest.mark.parametrize("b", (1, 2))
@pytest.mark.parametrize("d", range(1, 11))
def test_opening_equals_the_model(zk, d, b):
    """both fields and P = 1, 2, 3 at every (d, b); f and the coset alternate so that every P and field meets f = 0, 1 and d - 1, with and
    without a coset, over the range of d"""
    fs = sorted({0, min(1, d - 1), d - 1})
    for field in FIELDS:
        for P in (1, 2, 3):
            f = fs[(d + P + field) % len(fs)]
            check_opening(zk, field, d, b, f, P, with_coset=(d + b + P + (field & 1)) % 2 == 1)


def test_opening_at_d_15(zk):
    """several workgroups per reduction in every early round; the combination pass over 2^15 entries"""
    check_opening(zk, 3, 15, 1, 4, 2, with_coset=True, Q=4)


def test_opening_at_eight_points(zk):
    check_opening(zk, 0, 7, 2, 1, 8, with_coset=True)
    check_opening(zk, 3, 4, 1, 0, 8, with_coset=False)


def test_opening_on_a_callers_transcript(zk):
    field, d, b, f, Q, P = 0, 5, 1, 1, 8, 2
    cm = model_commitment(zk, field, d, b, True)
    pts = points_for(field, d, P, 78)
    mt = M.Transcript()
    mt.append(b"before the opening")
    op = PT.open_points(cm, pts, f, Q, mt, hasher=hasher_for(zk, 2 << (d + b)))
    t, v, want = zk.Transcript(), zk.Transcript(), zk.Transcript()
    t.append(b"before the opening")
    v.append(b"before the opening")
    want.append(bytes(mt.buf))
    pm = to_mont(zk, field, [x for z in pts for x in z]).reshape(P, d, 4)
    with gpu_commitment(zk, cm) as gc:
        got = zk.fri.open_multilinear_points(gc, pm, f, Q, transcript=t)
    assert_same_opening(zk, got, op)
    assert zk.fri.verify_multilinear_points(cm["root"], pm, got, transcript=v)
    assert np.array_equal(t.export_state(), want.export_state()) and np.array_equal(v.export_state(), want.export_state())


def test_argument_errors_return_the_documented_status_and_write_nothing(zk):
    import ctypes as C
    from zkmle_amd import _lib as L
    field, d, b = 3, 4, 1
    p = NM.MODULUS[field]
    cm = model_commitment(zk, field, d, b, False)
    pm = to_mont(zk, field, NM.random_ints(field, 2 * d, 5)).reshape(2, d, 4)
    lib = zk.lib()
    with gpu_commitment(zk, cm) as gc:
        def call(points, P, f, Q):
            op = zk.fri.FriMlPointsOpening(field, 2, d, b, 0, 8)
            for a in (op.ys, op.gamma, op.round_polys, op.final_table, op.challenges, op.query_indices, op.query_values):
                a[...] = np.uint64(0xA5A5A5A5A5A5A5A5)
            op.roots[...] = 0xA5
            op.query_paths[...] = 0xA5
            rc = lib.zk_fri_ml_open_points(gc._h, L.p64(points), P, f, Q, None, L.p64(op.ys), L.p64(op.gamma), L.p64(op.round_polys), L.p8(op.roots),
                                           L.p64(op.final_table), L.p64(op.challenges), L.p64(op.query_indices), L.p64(op.query_values), L.p8(op.query_paths))
            untouched = all((a == np.uint64(0xA5A5A5A5A5A5A5A5)).all() for a in (op.ys, op.gamma, op.round_polys, op.final_table, op.challenges,
                                                                                   op.query_indices, op.query_values))
            return rc, untouched and (op.roots == 0xA5).all() and (op.query_paths == 0xA5).all()

        for P, f, Q in ((0, 0, 8), (9, 0, 8), (2, 4, 8), (2, 7, 8), (2, 0, 0), (2, 0, 4097)):
            assert call(pm, P, f, Q) == (L.ZK_E_ARG, True), (P, f, Q)
        unreduced = pm.copy()
        unreduced[1, 2] = np.frombuffer((int.from_bytes(pm[1, 2].tobytes(), "little") + p).to_bytes(32, "little"), np.uint64)
        assert call(unreduced, 2, 0, 8) == (L.ZK_E_ARG, True)
        assert call(unreduced, 1, 0, 8)[0] == 0              # the unreduced entry lies in the second point: one point opens
        with pytest.raises(L.ZkError) as e:
            zk.fri.open_multilinear_points(gc, pm[:, :3], 0, 8)
        assert e.value.code == L.ZK_E_ARG
    # the round pass
    T = zk.MultilinearPolynomial.random(field, 8, 1)
    short = zk.MultilinearPolynomial.random(field, 2, 2)
    g3 = np.full((3, 4), 7, np.uint64)
    to, wo = C.c_void_p(), C.c_void_p()
    one = elem(zk, field, 1)
    assert lib.zk_fri_ml_round(T._h, short._h, None, None, None, L.p64(g3)) == L.ZK_E_LEN_MISMATCH
    assert lib.zk_fri_ml_round(short._h, short._h, L.p64(one), C.byref(to), C.byref(wo), L.p64(g3)) == L.ZK_E_ARG
    assert (g3 == 7).all() and not to.value and not wo.value


# ---- the succinct sparse GKR -----------------------------------------------------------------------------------------------------------
def reference_shape_circuit(depth, seed):
    """the reference's shape: layer i has 2^i outputs over 2^(i+1) inputs, out_bits = [1, 1, 2, ..]"""
    rng = random.Random(seed)
    rows = []
    for i in range(depth):
        n_out, n_in = 1 << i, 1 << (i + 1)
        seen = set()
        for o in range(n_out):
            for _ in range(rng.choice([1, 1, 2])):
                seen.add((rng.randrange(n_in), rng.randrange(n_in), o, rng.randrange(2)))
        rows.append(np.array(sorted(seen), np.uint64))
    return rows, [1] + list(range(1, depth)), depth


def wide_circuit(bits, seed):
    """tests/test_gpu_gkr_sparse.py test_wide_circuits_verify's construction: one gate per output, random wiring"""
    rng = np.random.default_rng(seed)
    *out_bits, in_last = bits
    widths = list(out_bits) + [in_last]
    rows = []
    for l in range(len(out_bits)):
        n_out, n_in = 1 << widths[l], 1 << widths[l + 1]
        g = np.zeros((n_out, 4), np.uint64)
        g[:, 0] = rng.integers(0, n_in, n_out)
        g[:, 1] = rng.integers(0, n_in, n_out)
        g[:, 2] = np.arange(n_out)
        g[:, 3] = rng.integers(0, 2, n_out)
        rows.append(g)
    return rows, list(out_bits), in_last


def copy_proof(zk, proof, **over):
    return zk.gkr.SparseProof(**{**proof.__dict__, **over})


@pytest.mark.parametrize("shape", ("reference", "wide"))
@pytest.mark.parametrize("field", FIELDS)
def test_succinct_sparse_gkr(zk, field, shape):
    p = NM.MODULUS[field]
    rows, out_bits, k = reference_shape_circuit(3, 11 + field) if shape == "reference" else wide_circuit((3, 7, 9, 6, 8), 23 + field)
    b, f, Q = 2, min(2, k - 1), 8
    x = zk.MultilinearPolynomial.random(field, 1 << k, 0x600 + field)
    inputs = x.evaluated_values
    with zk.fri.commit(x, b, elem(zk, field, 0x5EED)) as cm:
        proof = zk.gkr.sparse_prove_succinct(field, rows, out_bits, cm, f, Q)
        root = cm.root
    assert proof.input_root == root
    assert zk.gkr.sparse_verify_succinct(field, rows, out_bits, proof) is True
    # the challenges are the replay's: the root first, then gkr_protocol.rs' appends unchanged
    nl, off, per_layer = len(rows), 0, []
    for r in proof.rounds:
        per_layer.append([zk.to_ints(field, proof.coeffs[j]) for j in range(off, off + r)])
        off += r
    replay = PT.gkr_succinct_replay(p, root, zk.to_ints(field, proof.circuit_output), out_bits[0], zk.to_ints(field, proof.layer_claims), per_layer,
                                    zk.to_ints(field, proof.wb_evals) if nl > 1 else [], zk.to_ints(field, proof.wc_evals) if nl > 1 else [])
    assert zk.to_ints(field, proof.output_challenges) == replay["output_challenges"]
    assert zk.to_ints(field, proof.challenges) == [c for layer in replay["challenges"] for c in layer]
    # ... and differ from the unbound proof's, whose transcript starts with the output layer
    plain = zk.gkr.sparse_prove(field, rows, out_bits, inputs)
    assert np.array_equal(plain.circuit_output, proof.circuit_output) and not np.array_equal(plain.output_challenges, proof.output_challenges)
    # the opened values are the inputs' extension at the last layer's rb and rc, which are the opening's points
    rb, rc = proof.challenges[off - 2 * k:off - k], proof.challenges[off - k:off]
    assert np.array_equal(proof.input_evals[0], x.evaluate(rb)) and np.array_equal(proof.input_evals[1], x.evaluate(rc))
    assert zk.fri.verify_multilinear_points(root, np.stack([rb, rc]), proof.opening)
    # one bit of the root, of input_evals, of a layer coefficient
    assert not zk.gkr.sparse_verify_succinct(field, rows, out_bits, copy_proof(zk, proof, input_root=bytes([root[0] ^ 1]) + root[1:]))
    assert not zk.gkr.sparse_verify_succinct(field, rows, out_bits, copy_proof(zk, proof, input_root=root[:31] + bytes([root[31] ^ 0x80])))
    for which in (0, 1):
        ev = proof.input_evals.copy()
        ev[which, 0] ^= np.uint64(1)
        assert not zk.gkr.sparse_verify_succinct(field, rows, out_bits, copy_proof(zk, proof, input_evals=ev)), which
    for j in (0, off - 1):
        co = proof.coeffs.copy()
        co[j, 1, 0] ^= np.uint64(1)
        assert not zk.gkr.sparse_verify_succinct(field, rows, out_bits, copy_proof(zk, proof, coeffs=co)), j
    # a proof for a commitment to other inputs, shown with the first root
    other_x = zk.MultilinearPolynomial.random(field, 1 << k, 0x700 + field)
    with zk.fri.commit(other_x, b, elem(zk, field, 0x5EED)) as cm2:
        other = zk.gkr.sparse_prove_succinct(field, rows, out_bits, cm2, f, Q)
    assert other.input_root != root and zk.gkr.sparse_verify_succinct(field, rows, out_bits, other)
    assert not zk.gkr.sparse_verify_succinct(field, rows, out_bits, copy_proof(zk, other, input_root=root))
    # the unbound verifier is what it was
    assert zk.gkr.sparse_verify(field, rows, out_bits, plain, inputs) is True
    assert zk.gkr.sparse_verify(field, rows, out_bits, proof, inputs) is False


def test_succinct_sparse_gkr_needs_a_commitment_of_the_input_width(zk):
    from zkmle_amd import _lib as L
    field = 3
    rows, out_bits, k = wide_circuit((2, 4, 6), 5)
    x = zk.MultilinearPolynomial.random(field, 1 << (k + 1), 9)
    with zk.fri.commit(x, 1) as cm:
        circuit = zk.gkr.SparseCircuit(rows, out_bits, 1 << k)
        with pytest.raises(L.ZkError) as e:
            zk.gkr.sparse_prove_succinct(field, None, None, cm, 0, 4, circuit=circuit)
        assert e.value.code == L.ZK_E_LEN_MISMATCH
