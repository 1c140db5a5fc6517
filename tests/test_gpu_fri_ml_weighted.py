"""GPU: the opening of a FRI commitment against a caller's weight table (csrc/zkmle_fri_ml.hip Weighted; include/zkmle.h "FRI commitment opened
against a weight table") over BLS12-381 Fr and BN254 Fr, every output byte for byte against tests/_fri_ml_weighted_model.py.

  open      d = 10 for the three schedules (log_arity 1; 2; 2 on grouped leaves) with 0 and 8 bits of proof of work, with and without a coset
            and a caller's transcript among them: c, the round polynomials, roots, final table, challenges, nonce, indices, values and paths
            equal the model's; the host verifier accepts with the model's w_final and rejects with another; the caller's weight table is
            unchanged
  eq        with W_0 = eq(., z) the claim is zk_mle_evaluate(T, z)
  operands  a weight table of all p - 1 on a table of all p - 1; a weight table of all zero
  capped    d = 13 in a child process with ZK_REDUCE_BLOCKS=64 (tests/_fri_ml_weighted_worker.py)
  refusals  a weight table of another length or field, grouped leaves at log_arity 1, a missing output: a status, nothing proved"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _fri_ml_cases as FC
import _fri_ml_model as ML
import _fri_ml_weighted_model as WM
import _grind_model as GR
import _ntt_model as NM
from oracle import pymodel as M
from test_gpu_fri import table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (0, 3)
SCHEDULES = [(1, False), (2, False), (2, True)]
sched_id = lambda s: "a%d%s" % (s[0], "g" if s[1] else "")
Q = 6


def assert_same_opening(zk, got, op):
    fl = WM.flat(zk, op)
    for name, a, b in (("c", got.c, fl["c"]), ("polys", got.round_polys, fl["polys"]), ("final", got.final_table, fl["final"]),
                       ("challenges", got.challenges, fl["challenges"]), ("values", got.query_values, fl["values"])):
        assert a.shape == b.shape and np.array_equal(a, b), name
    assert got.roots.tobytes() == fl["roots"] and got.query_paths.tobytes() == fl["paths"] and list(got.query_indices) == fl["indices"]
    assert got.pow_nonce == op["nonce"]


def open_both(zk, field, d, b, f, sched, W0, bits=0, with_coset=False, prior=b"", seed=0, coeffs=None):
    """(the library's opening, the model's, the two transcripts' next samples, the device weight table)"""
    a, grouped = sched
    hasher = FC.hasher(zk, grouped)
    coset = FC.coset_of(field, d, b, with_coset, 67)
    cm = (FC.GM if grouped else FC.PM).commit(field, coeffs, b, coset, hasher) if coeffs is not None else FC.commitment(field, d, b, coset, 16000 + seed + field, hasher, grouped)
    mt, lt = M.Transcript(), zk.Transcript()
    if prior:
        mt.append(prior)
        lt.append(prior)
    op = WM.open_weighted(cm, W0, f, Q, a, mt, hasher, (lambda t: GR.grind(t, bits)) if bits else None)
    wt = table_of(zk, field, W0)
    with FC.gpu_commitment(zk, cm) as gcm:
        got = zk.fri.open_weighted(gcm, wt, f, Q, log_arity=a, transcript=lt, grinding_bits=bits)
    assert np.array_equal(wt.evaluated_values, to_mont(zk, field, W0))
    return got, op, cm, (mt.sample(), lt.sample_random_challenge())


@pytest.mark.parametrize("bits", (0, 8))
@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
@pytest.mark.parametrize("field", FIELDS)
def test_opening_equals_the_model(zk, field, sched, bits):
    d, b = 10, 1 + (field == 3)
    f = (0, 3, 1)[SCHEDULES.index(sched)]
    with_coset, prior = (field == 0) == (bits == 0), b"the caller bound W_0 here" if bits else b""
    W0 = NM.random_ints(field, 1 << d, 16100 + field + bits)
    got, op, cm, ends = open_both(zk, field, d, b, f, sched, W0, bits, with_coset, prior, seed=bits)
    assert_same_opening(zk, got, op)
    assert ends[0] == ends[1]
    vt = zk.Transcript()
    if prior:
        vt.append(prior)
    assert zk.fri.verify_weighted(cm["root"], to_mont(zk, field, op["w_final"]), got, vt) and vt.sample_random_challenge() == ends[0]
    other = list(op["w_final"])
    other[-1] = (other[-1] + 1) % NM.MODULUS[field]
    assert not zk.fri.verify_weighted(cm["root"], to_mont(zk, field, other), got)


@pytest.mark.parametrize("field", FIELDS)
def test_with_an_eq_table_the_claim_is_the_evaluation(zk, field):
    p, d = NM.MODULUS[field], 10
    z = FC.points_for(field, d, 1, 16200 + field)[0]
    W0 = ML.eq_table(z, p)
    got, op, cm, _ = open_both(zk, field, d, 1, 2, SCHEDULES[1], W0, seed=3)
    assert_same_opening(zk, got, op)
    y = table_of(zk, field, cm["coeffs"]).evaluate(zk.from_ints(field, z))
    assert np.array_equal(got.c, y) and op["c"] == ML.mle_evaluate(field, cm["coeffs"], z)


@pytest.mark.parametrize("field", FIELDS)
def test_weights_at_the_edge_operands(zk, field):
    p, d = NM.MODULUS[field], 10
    for W0, coeffs in (([p - 1] * (1 << d), [p - 1] * (1 << d)), ([0] * (1 << d), None), ([p - 1] * (1 << d), None)):
        got, op, cm, _ = open_both(zk, field, d, 1, 1, SCHEDULES[0], W0, seed=5, coeffs=coeffs)
        assert_same_opening(zk, got, op)
        assert zk.fri.verify_weighted(cm["root"], to_mont(zk, field, op["w_final"]), got)


def test_the_round_pass_under_a_capped_grid():
    e = dict(os.environ, ZK_REDUCE_BLOCKS="64")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_fri_ml_weighted_worker.py")], capture_output=True, text=True, env=e, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out == {"blocks": 64, "checked": 18, "mismatches": []}, out


def test_refusals(zk):
    field, d = 0, 6
    cm = FC.commitment(field, d, 1, 1, 16300, FC.hasher(zk))
    grouped = FC.commitment(field, d, 1, 1, 16300, FC.hasher(zk, True), True)
    W = table_of(zk, field, [1] * (1 << d))
    with FC.gpu_commitment(zk, cm) as gcm, FC.gpu_commitment(zk, grouped) as ggm:
        for args, code in (((gcm, table_of(zk, field, [1] * (1 << (d - 1))), 1, Q), -2), ((gcm, table_of(zk, 3, [1] * (1 << d)), 1, Q), -7),
                           ((gcm, W, d, Q), -7), ((gcm, W, d - 1, Q, 2), -7), ((gcm, W, 1, 0), -7)):
            with pytest.raises(zk.ZkError) as e:
                zk.fri.open_weighted(*args)
            assert e.value.code == code, args[2:]
        with pytest.raises(ValueError):
            zk.fri.open_weighted(ggm, W, 1, Q, log_arity=1)
        op, L = zk.fri.FriMlWeightedOpening(field, d, 1, 1, Q, None, 2, True), zk._lib
        outs = (L.p64(op.c), L.p64(op.round_polys), L.p8(op.roots), L.p64(op.final_table), L.p64(op.challenges), L.p64(op.query_indices), L.p64(op.query_values),
                L.p8(op.query_paths), None)
        assert zk.lib().zk_fri_ml_open_weighted(ggm._h, W._h, 1, Q, 1, 0, None, *outs) == -7       # grouped leaves at log_arity 1
        assert zk.lib().zk_fri_ml_open_weighted(ggm._h, W._h, 1, Q, 2, 8, None, *outs) == -7       # proof of work without room for the nonce
