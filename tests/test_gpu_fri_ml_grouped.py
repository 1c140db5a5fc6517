"""GPU: the commitment with grouped leaves and its multilinear opening (csrc/zkmle_fri_pcs.hip zk_fri_commit_grouped, csrc/zkmle_fri_ml.hip
zk_fri_ml_open_points_grouped; include/zkmle.h "FRI commitment opened with grouped leaves"), over BLS12-381 Fr and BN254 Fr.  Everything
compares byte for byte with the model of tests/_fri_ml_grouped_model.py; no tolerance anywhere.

  commit     the grouped root equals the model's; log_group = 0 gives zk_fri_commit's root; coefficients and codeword are zk_fri_commit's
  open       the opening equals the model in every output and passes the host verifier, on the cases of tests/test_gpu_fri_ml_arity.py
             (R = 2 .. 9: fold-4 steps, and the final fold-2 step with its pair leaf); through a caller's transcript, which ends in the
             verifier's state; the codeword and the commitment's tree are unchanged after an opening
  refusals   each of the six openers that walk a tree of 2 N - 1 digests returns ZK_E_ARG on a grouped commitment and writes nothing;
             zk_fri_ml_open_points_grouped returns ZK_E_ARG on an ungrouped one"""
import ctypes as C
import functools

import numpy as np
import pytest

import _fri_ml_cases as FC
import _fri_ml_grouped_model as GM
import _ntt_model as NM
from oracle import pymodel as M
from test_gpu_fri import table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)
from test_gpu_fri_ml_arity import CASES, assert_same_opening, elem, points_for

pytestmark = pytest.mark.gpu
Q = 8
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)


def hasher_for(zk, n):
    return GM.check_host_keccak(zk) if n > 1 << 10 else M.keccak256


gpu_commitment = FC.gpu_commitment


@functools.lru_cache(maxsize=None)
def model_commitment(zk, field, d, b, with_coset):
    return FC.commitment(field, d, b, FC.coset_of(field, d, b, with_coset, 67), 9700 + 17 * d + b + field, hasher_for(zk, 2 << (d + b)), True)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_opening_equals_the_model(zk, case):
    field, d, b, f, P, with_coset = case
    p = NM.MODULUS[field]
    cm = model_commitment(zk, field, d, b, with_coset)
    hasher = hasher_for(zk, 2 << (d + b))
    pts = points_for(field, d, P, d * 1000 + b * 100 + f * 10 + P + field)
    op = GM.open_points(cm, pts, f, Q, hasher=hasher)
    assert GM.verify(op, hasher=hasher)
    fl = GM.flat(zk, op)
    pm = to_mont(zk, field, [v for z in pts for v in z]).reshape(P, d, 4)
    with gpu_commitment(zk, cm) as gc:
        assert gc.log_group == 2 and gc.root == cm["root"]
        assert np.array_equal(gc.codeword().evaluated_values, to_mont(zk, field, cm["codeword"]))
        codeword_before = gc.codeword().evaluated_values
        got = zk.fri.open_multilinear_points(gc, pm, f, Q, log_arity=2)
        assert got.log_arity == 2 and got.grouped
        assert_same_opening(zk, got, fl)
        assert zk.fri.verify_multilinear_points(gc.root, pm, got)
        assert np.array_equal(gc.codeword().evaluated_values, codeword_before)
        st = zk.fri.ml_last_stats()
        assert st["rounds"] == d - f and st["queries"] == Q
        again = zk.fri.open_multilinear_points(gc, pm, f, Q, log_arity=2)   # the commitment's tables and tree were only read: root_0 and
        assert_same_opening(zk, again, fl)                                   # layer 0's paths come out of the tree again
    bad = zk.fri.FriMlPointsOpening(field, P, d, b, f, Q, got.coset, 2, grouped=True)
    for name in ("ys", "round_polys", "roots", "final_table", "query_values", "query_paths"):
        setattr(bad, name, getattr(got, name).copy())
    bad.ys[P - 1] = to_mont(zk, field, [(op["ys"][P - 1] + 1) % p])[0]
    assert not zk.fri.verify_multilinear_points(cm["root"], pm, bad)


@pytest.mark.parametrize("field", (0, 3))
def test_commit_roots(zk, field):
    d, b = 5, 2
    cm = model_commitment(zk, field, d, b, True)
    cs = elem(zk, field, cm["coset"])
    coeffs = table_of(zk, field, cm["coeffs"])
    with zk.fri.commit(coeffs, b, cs) as plain, zk.fri.commit(coeffs, b, cs, log_group=0) as zero, zk.fri.commit(coeffs, b, cs, log_group=2) as grouped:
        assert (plain.log_group, zero.log_group, grouped.log_group) == (0, 0, 2)
        assert zero.root == plain.root != grouped.root == cm["root"]
        cw = plain.codeword()
        assert np.array_equal(grouped.codeword().evaluated_values, cw.evaluated_values)
        assert grouped.root == zk.merkle_root(cw, log_group=2) and plain.root == zk.merkle_root(cw)
        # the commitment's tree: layer 0's paths of an opening are those of a tree built from the codeword
        tree = zk.MerkleTree.build(cw, log_group=2)
        pm = to_mont(zk, field, [v for z in points_for(field, d, 1, 3) for v in z]).reshape(1, d, 4)
        op = zk.fri.open_multilinear_points(grouped, pm, 1, Q, log_arity=2)
        L0 = d + b - 2
        per = op.query_paths.size // Q
        want = tree.open(op.query_indices % np.uint64(1 << L0))
        for q in range(Q):
            assert np.array_equal(op.query_paths[q * per:q * per + 32 * L0].reshape(L0, 32), want[q]), q
        # the quotient does not read the tree and works on a grouped commitment
        z, y, g = elem(zk, field, 12345), elem(zk, field, 7), elem(zk, field, 9)
        assert np.array_equal(zk.fri.quotient([grouped], z, y[None], g).evaluated_values, zk.fri.quotient([plain], z, y[None], g).evaluated_values)


def test_opening_on_a_callers_transcript(zk):
    field, d, b, f, P = 0, 5, 1, 0, 2
    cm = model_commitment(zk, field, d, b, True)
    pts = points_for(field, d, P, 79)
    mt = M.Transcript()
    mt.append(b"before the opening")
    op = GM.open_points(cm, pts, f, Q, mt, hasher=hasher_for(zk, 2 << (d + b)))
    t, v, want = zk.Transcript(), zk.Transcript(), zk.Transcript()
    t.append(b"before the opening")
    v.append(b"before the opening")
    want.append(bytes(mt.buf))
    pm = to_mont(zk, field, [x for z in pts for x in z]).reshape(P, d, 4)
    with gpu_commitment(zk, cm) as gc:
        got = zk.fri.open_multilinear_points(gc, pm, f, Q, transcript=t, log_arity=2)
    assert_same_opening(zk, got, GM.flat(zk, op))
    assert zk.fri.verify_multilinear_points(cm["root"], pm, got, transcript=v)
    assert np.array_equal(t.export_state(), want.export_state()) and np.array_equal(v.export_state(), want.export_state())


def filled(n, dtype=np.uint64):
    return np.full(n, FILL if dtype == np.uint64 else 0xA5, dtype)


def untouched(arrs):
    return all((a == (FILL if a.dtype == np.uint64 else 0xA5)).all() for a in arrs)


def test_the_ungrouped_openers_refuse_a_grouped_commitment(zk):
    from zkmle_amd import _lib as L
    lib = zk.lib()
    field, d, b, f, nq = 3, 4, 1, 0, 8
    cm = model_commitment(zk, field, d, b, False)
    pm = to_mont(zk, field, NM.random_ints(field, 2 * d, 5)).reshape(2, d, 4)
    z = elem(zk, field, 0xABCDEF)
    with gpu_commitment(zk, cm) as gc, gpu_commitment(zk, cm, log_group=0) as plain:
        w = lambda n: filled(n)
        by = lambda n: filled(n, np.uint8)
        # zk_fri_ml_open, zk_fri_ml_open_points, zk_fri_ml_open_points_arity at both arities
        ys, gamma, polys, roots, fin, chal, idx, vals, paths = w(8), w(4), w(4 * 3 * d), by(32 * d), w(4 << d), w(4 * d), w(nq), w(4 * nq * 4 * d), by(32 * nq * 4 * d * (d + b))
        outs = (ys, gamma, polys, roots, fin, chal, idx, vals, paths)
        tail = (L.p64(polys), L.p8(roots), L.p64(fin), L.p64(chal), L.p64(idx), L.p64(vals), L.p8(paths))
        assert lib.zk_fri_ml_open(gc._h, L.p64(pm[0]), f, nq, None, L.p64(ys), *tail) == L.ZK_E_ARG and untouched(outs)
        assert lib.zk_fri_ml_open_points(gc._h, L.p64(pm), 2, f, nq, None, L.p64(ys), L.p64(gamma), *tail) == L.ZK_E_ARG and untouched(outs)
        for a in (1, 2):
            assert lib.zk_fri_ml_open_points_arity(gc._h, L.p64(pm), 2, f, nq, a, None, L.p64(ys), L.p64(gamma), *tail) == L.ZK_E_ARG and untouched(outs)
        # the grouped opener on an ungrouped commitment, and on a grouped one with R = 1
        assert lib.zk_fri_ml_open_points_grouped(plain._h, L.p64(pm), 2, f, nq, None, L.p64(ys), L.p64(gamma), *tail) == L.ZK_E_ARG and untouched(outs)
        assert lib.zk_fri_ml_open_points_grouped(gc._h, L.p64(pm), 2, d - 1, nq, None, L.p64(ys), L.p64(gamma), *tail) == L.ZK_E_ARG and untouched(outs)
        with pytest.raises(ValueError):
            zk.fri.open_multilinear_points(gc, pm, f, nq)     # log_arity = 1 on a grouped commitment
        # zk_fri_pcs_open
        hs = (C.c_void_p * 1)(gc._h)
        betas, ov, opaths = w(4 * d), w(4 * nq * 2), by(32 * nq * 2 * (d + b))
        assert lib.zk_fri_pcs_open(hs, 1, L.p64(z), f, nq, None, L.p64(ys), L.p8(roots), L.p64(fin), L.p64(betas), L.p64(idx), L.p64(vals), L.p8(paths),
                                   L.p64(ov), L.p8(opaths)) == L.ZK_E_ARG and untouched(outs + (betas, ov, opaths))
        # zk_sumcheck_basic_prove_succinct
        cs, rp, ch, y = w(4), w(4 * 2 * d), w(4 * d), w(4)
        assert lib.zk_sumcheck_basic_prove_succinct(gc._h, f, nq, None, L.p64(cs), L.p64(rp), L.p64(ch), L.p64(y), *tail) == L.ZK_E_ARG
        assert untouched(outs + (cs, rp, ch, y))
        # zk_gkr_sparse_prove_succinct: one layer of 8 gates over the 16 committed inputs
        gates = [np.array([(2 * k, 2 * k + 1, k, k % 2) for k in range(8)], np.uint64)]   # (left, right, out, op)
        with pytest.raises(L.ZkError) as e:
            zk.gkr.sparse_prove_succinct(field, gates, [3], gc, f, nq)
        assert e.value.code == L.ZK_E_ARG
        assert zk.gkr.sparse_prove_succinct(field, gates, [3], plain, f, nq).input_root == plain.root
        # the commitment is as it was
        got = zk.fri.open_multilinear_points(gc, pm, f, nq, log_arity=2)
        assert zk.fri.verify_multilinear_points(gc.root, pm, got)
