"""GPU: the zerocheck of a Plonk gate over eight FRI commitments (csrc/zerocheck.cuh zerocheck_gate_round_kernel, csrc/zkmle_zerocheck.hip;
include/zkmle.h "Zerocheck of a Plonk gate over committed tables"), over BLS12-381 Fr and BN254 Fr.  Everything is byte for byte; no tolerance
anywhere.

  round     zk_zerocheck_gate_round equals the model of tests/_zerocheck_gate_model.py for every table length 2^1 .. 2^15 (one lane, under a
            wave, one workgroup, two, up to 64 workgroups a reduction), in both forms and both fields, r among 0, 1, p - 1 and random; the
            folded tables equal mle_fold_last, the inputs are unchanged; and at 2^10 entries at the operands random tables never reach: all
            nine tables all p - 1, E all zero, all selectors zero (every sum is 0), entries drawn from {0, p - 1, random}, a satisfied circuit
            (g(0) = g(1) = 0 in round 0's form; g(0) + g(1) = the previous quartic at r after a fold)
  stride    the second trip of the grid-stride loop: one child process (tests/_zerocheck_worker.py gate) with ZK_REDUCE_BLOCKS=64 runs round
            0's form at 2^16 entries and the fold form at 2^17, on random tables and on tables all p - 1 with r = p - 1, against the same
            model; the child reports the cap it ran with
  tie       with qM = 1, qO = p - 1, qL = qR = qC = 0 the pass is zk_zerocheck_mul_round's on (A, B, C, E): g5[0 .. 3] = its g4, g5[4] the
            cubic extrapolated
  prove     on a satisfied circuit every output equals the model's: d = 1 .. 8 with both blow-ups, the three schedules, with and without a
            coset, log_final among 0, 1, d - 1 and both fields spread over them; once at d = 12; once with 8 bits of proof of work.
            ys = zk_mle_evaluate of each table at the reversed challenges; verify_gate accepts; a second proof is identical; a false
            statement is proved and not verified; a caller's transcript ends in the verifier's state
  refusals  a commitment of another d, field, blow-up, coset or grouping in any of the eight places, grouped ones at log_arity = 1,
            grinding_bits = 33: ZK_E_ARG, nothing written, the transcript as it was"""
import ctypes as C
import random

import numpy as np
import pytest

import _fri_ml_cases as FC
import _fri_ml_grouped_model as GM
import _fri_ml_model as ML
import _fri_pcs_model as PM
import _ntt_model as NM
import _zerocheck_gate_model as ZG
from oracle import pymodel as M
from test_gpu_fri import table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)
from test_gpu_zerocheck import run_stride_worker

pytestmark = pytest.mark.gpu
FIELDS = (0, 3)
Q = 6
SCHEDULES = [(1, False), (2, False), (2, True)]
sched_id = lambda s: "a%d%s" % (s[0], "g" if s[1] else "")


def elem(zk, field, v):
    return zk.from_ints(field, [v])[0]


def check_round(zk, field, tabs, r, what):
    """both the hook's outputs against the model on the nine integer tables `tabs` = (A, B, C, qM, qL, qR, qO, qC, E); r = None: round 0's form"""
    p = NM.MODULUS[field]
    dev = [table_of(zk, field, t) for t in tabs]
    before = [t.evaluated_values.copy() for t in dev]
    if r is None:
        g5 = zk.zerocheck.gate_round(dev)
        want = tabs
    else:
        folded, g5 = zk.zerocheck.gate_round(dev, r=elem(zk, field, r))
        want = [ML.mle_fold_last(field, t, r) for t in tabs]
        assert len(folded) == 9
        for got, w in zip(folded, want):
            assert len(got) == len(w) and np.array_equal(got.evaluated_values, to_mont(zk, field, w)), what
    g = ZG.round_g5(want, p)
    assert g5.shape == (5, 4) and np.array_equal(g5, to_mont(zk, field, g)), what
    for t, b in zip(dev, before):
        assert np.array_equal(t.evaluated_values, b), what
    return g


@pytest.mark.parametrize("fold", (False, True), ids=("round0", "fold"))
@pytest.mark.parametrize("field", FIELDS)
def test_round_equals_the_model_at_every_length(zk, field, fold):
    p = NM.MODULUS[field]
    rng = random.Random(6100 + field + 2 * fold)
    for loglen in range(2 if fold else 1, 16):
        n = 1 << loglen
        tabs = [NM.random_ints(field, n, 6200 + 11 * loglen + j + field) for j in range(9)]
        r = (0, 1, p - 1, rng.randrange(p))[loglen % 4] if fold else None
        check_round(zk, field, tabs, r, (loglen, r))


@pytest.mark.parametrize("fold", (False, True), ids=("round0", "fold"))
@pytest.mark.parametrize("field", FIELDS)
def test_round_at_operands_random_tables_never_reach(zk, field, fold):
    p = NM.MODULUS[field]
    rng = random.Random(6300 + field + 2 * fold)
    rs = (0, 1, p - 1, rng.randrange(p)) if fold else (None,)
    n = 1 << 10                                               # four workgroups of a fold pass, eight of round 0's
    rnd = [NM.random_ints(field, n, 6400 + j + field) for j in range(9)]
    circ = ZG.circuit(field, n, 6500 + field)
    prev = ZG.round_g5(circ + [rnd[8]], p)
    assert prev[0] == 0 and prev[1] == 0
    for r in rs:
        check_round(zk, field, [[p - 1] * n] * 9, r, "all p - 1")
        check_round(zk, field, rnd[:8] + [[0] * n], r, "E zero")
        g = check_round(zk, field, rnd[:3] + [[0] * n] * 5 + [rnd[8]], r, "selectors zero")
        assert g == [0] * 5
        mixed = [[rng.choice((0, p - 1, rng.randrange(p))) for _ in range(n)] for _ in range(9)]
        check_round(zk, field, mixed, r, "0, p - 1, random")
        g = check_round(zk, field, circ + [rnd[8]], r, "a satisfied circuit")
        if r is None:
            assert g[0] == 0 and g[1] == 0                   # the gate vanishes on the cube
        else:
            assert (g[0] + g[1]) % p == ZG.interpolate5(prev, r, p)


@pytest.mark.parametrize("fold", (False, True), ids=("round0", "fold"))
@pytest.mark.parametrize("field", FIELDS)
def test_the_gate_with_the_products_selectors_is_the_mul_round(zk, field, fold):
    """qM = 1, qO = p - 1, qL = qR = qC = 0: the gate is A B - C, and the message a cubic"""
    p = NM.MODULUS[field]
    rng = random.Random(6600 + field + 2 * fold)
    for loglen in (1, 2, 7, 10, 13):
        if fold and loglen < 2:
            continue
        n = 1 << loglen
        A, B, Cc, E = (NM.random_ints(field, n, 6700 + 5 * loglen + j + field) for j in range(4))
        nine = [A, B, Cc, [1] * n, [0] * n, [0] * n, [p - 1] * n, [0] * n, E]
        r = elem(zk, field, rng.randrange(p)) if fold else None
        dev = [table_of(zk, field, t) for t in nine]
        got5 = zk.zerocheck.gate_round(dev, r=r)
        got4 = zk.zerocheck.mul_round(dev[0], dev[1], dev[2], dev[8], r=r)
        g5, g4 = (got5[-1], got4[-1]) if fold else (got5, got4)
        assert np.array_equal(g5[:4], g4), loglen
        g = [int(v) for v in zk.to_ints(field, g5)]
        assert (g[3] * 4 - g[2] * 6 + g[1] * 4 - g[0]) % p == g[4], loglen   # the fourth difference of a cubic is 0: s_inf = 0
        if fold:
            for j, k in ((0, 0), (1, 1), (2, 2), (3, 8)):
                assert np.array_equal(got4[j].evaluated_values, got5[0][k].evaluated_values), (loglen, j)


def test_the_second_trip_of_the_grid_stride_loop():
    run_stride_worker("gate")


# ---- the prover ---------------------------------------------------------------------------------------------------------------------------
def hasher(zk):
    return FC.hasher(zk, True)


def model_commitments(zk, field, d, b, coset, grouped, seed, false_at=None):
    return [(GM if grouped else PM).commit(field, t, b, coset, hasher(zk)) for t in ZG.circuit(field, 1 << d, seed, false_at)]


def assert_same_proof(zk, got, pr):
    fl = ZG.flat(zk, pr)
    op = got.opening
    for name, arr in (("tau", got.tau), ("polys", got.round_polys), ("challenges", got.challenges), ("ys", got.ys), ("gamma", op.gamma),
                      ("open_polys", op.round_polys), ("roots", op.roots), ("final", op.final_table), ("open_challenges", op.challenges),
                      ("indices", op.query_indices), ("values", op.query_values), ("paths", op.query_paths)):
        assert arr.shape == fl[name].shape and np.array_equal(arr, fl[name]), name
    assert op.pow_nonce == pr["nonce"]
    assert np.array_equal(got.point[0], fl["points"][0])


def prove_case(zk, field, d, b, f, with_coset, sched, g_bits=0, seed=0):
    a, grouped = sched
    coset = FC.coset_of(field, d, b, with_coset, 61)
    cms = model_commitments(zk, field, d, b, coset, grouped, 7100 + 23 * d + field + seed)
    pr = ZG.prove(cms, f, Q, a, ZG.pow_transcript(d, f, g_bits) if g_bits else None, hasher(zk))
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    try:
        got = zk.zerocheck.prove_gate(gcs[:3], gcs[3:], f, Q, log_arity=a, grinding_bits=g_bits)
        assert isinstance(got, zk.zerocheck.ZerocheckGateProof) and isinstance(got.opening, zk.fri.FriMlBatchOpening) and got.round_polys.shape == (d, 5, 4)
        assert_same_proof(zk, got, pr)
        roots = [gc.root for gc in gcs]
        assert roots == pr["roots"] and zk.zerocheck.verify_gate(roots, got)
        assert not zk.zerocheck.verify_gate([roots[1], roots[0]] + roots[2:], got)
        st = zk.zerocheck.last_stats()
        assert st["rounds"] == d and st["ms_total"] > 0
        # the claims are the tables' values at the reversed challenges, by the call that existed before
        for j, cm in enumerate(cms):
            y = table_of(zk, field, cm["coeffs"]).evaluate(np.ascontiguousarray(got.challenges[::-1]))
            assert np.array_equal(y, got.ys[j]), j
        # the commitments were only read: a second proof from them is identical
        again = zk.zerocheck.prove_gate(gcs[:3], gcs[3:], f, Q, log_arity=a, grinding_bits=g_bits)
        assert_same_proof(zk, again, pr)
    finally:
        for gc in gcs:
            gc.free()


# d = 1 .. 8 under every schedule it allows; blow-up, coset, log_final in (0, 1, d - 1) and the field rotate so that each d meets both
# blow-ups and each schedule every log_final (tests/test_gpu_zerocheck.py's grid; the model commits eight tables a case, so d stops lower)
def grid():
    out = []
    for d in range(1, 9):
        for s, sched in enumerate(SCHEDULES):
            k = d + s
            f = (0, 1, d - 1)[k % 3] % d
            if sched[0] == 2 and d - f < 2:
                f = 0
                if d < 2:
                    continue
            out.append(pytest.param(FIELDS[k % 2], d, 1 + (d + s // 2) % 2, f, k % 4 < 2, sched, id="f%d-d%d-%s" % (FIELDS[k % 2], d, sched_id(sched))))
    return out


@pytest.mark.parametrize("field,d,b,f,with_coset,sched", grid())
def test_prove_equals_the_model(zk, field, d, b, f, with_coset, sched):
    prove_case(zk, field, d, b, f, with_coset, sched)


def test_prove_at_d_12(zk):
    prove_case(zk, 0, 12, 1, 1, True, (2, True))


def test_prove_with_proof_of_work(zk):
    prove_case(zk, 3, 6, 2, 1, True, (2, True), g_bits=8)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_a_false_statement_is_proved_and_not_verified(zk, sched):
    field, d, b, f = 3, 5, 1, 1
    a, grouped = sched
    cms = model_commitments(zk, field, d, b, 1, grouped, 7300, false_at=19)
    pr = ZG.prove(cms, f, Q, a, hasher=hasher(zk))
    assert ZG.verify(pr, hasher=hasher(zk)) == (False, 0)
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    try:
        got = zk.zerocheck.prove_gate(gcs[:3], gcs[3:], f, Q, log_arity=a)
        assert_same_proof(zk, got, pr)
        assert not zk.zerocheck.verify_gate([gc.root for gc in gcs], got)
    finally:
        for gc in gcs:
            gc.free()


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_prove_on_a_callers_transcript(zk, sched):
    field, d, b, f = 0, 6, 1, 1
    a, grouped = sched
    cms = model_commitments(zk, field, d, b, FC.coset_of(field, d, b, True, 61), grouped, 7400)
    mt = M.Transcript()
    mt.append(b"before the zerocheck")
    pr = ZG.prove(cms, f, Q, a, mt, hasher(zk))
    t, v, want = zk.Transcript(), zk.Transcript(), zk.Transcript()
    t.append(b"before the zerocheck")
    v.append(b"before the zerocheck")
    want.append(bytes(mt.buf))
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    try:
        got = zk.zerocheck.prove_gate(gcs[:3], gcs[3:], f, Q, log_arity=a, transcript=t)
    finally:
        for gc in gcs:
            gc.free()
    assert_same_proof(zk, got, pr)
    assert zk.zerocheck.verify_gate(pr["roots"], got, transcript=v)
    assert np.array_equal(t.export_state(), want.export_state()) and np.array_equal(v.export_state(), want.export_state())
    assert not zk.zerocheck.verify_gate(pr["roots"], got)     # bound to the prior content


def test_refusals_write_nothing(zk):
    from zkmle_amd import _lib as L
    lib = zk.lib()
    nq = 8
    mk = lambda field, d, b, coset, lg, seed: zk.fri.commit(zk.MultilinearPolynomial.random(field, 1 << d, seed), b, coset, log_group=lg)
    base = [mk(3, 4, 1, None, 0, 1 + j) for j in range(8)]
    others = {"d": mk(3, 5, 1, None, 0, 11), "blow-up": mk(3, 4, 2, None, 0, 12), "field": mk(0, 4, 1, None, 0, 13), "coset": mk(3, 4, 1, elem(zk, 3, 5), 0, 14),
              "grouping": mk(3, 4, 1, None, 2, 15)}
    grp = [mk(3, 4, 1, None, 2, 21 + j) for j in range(8)]
    every = base + list(others.values()) + grp
    FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
    w = lambda n: np.full(n, FILL, np.uint64)
    by = lambda n: np.full(n, 0xA5, np.uint8)
    tau, polys, chal, ys, gamma, opolys, roots, fin, ochal, idx, vals, paths = (w(4 * 5), w(20 * 5), w(4 * 5), w(32), w(4), w(12 * 5), by(32 * 32), w(4 << 5),
                                                                                  w(4 * 5), w(nq), w(4 * nq * 160), by(32 * nq * 1200))
    outs = (tau, polys, chal, ys, gamma, opolys, roots, fin, ochal, idx, vals, paths)
    nonce = C.c_uint64(0xA5)
    t = zk.Transcript()
    t.append(b"untouched")
    before = t.export_state().copy()

    def raw(cms, a=1, f=0, g=0):
        arr = (C.c_void_p * 8)(*[c._h for c in cms])
        return lib.zk_zerocheck_gate_prove(arr, f, nq, a, g, t._h, L.p64(tau), L.p64(polys), L.p64(chal), L.p64(ys), L.p64(gamma), L.p64(opolys),
                                           L.p8(roots), L.p64(fin), L.p64(ochal), L.p64(idx), L.p64(vals), L.p8(paths), C.byref(nonce))

    def refused(cms, what, **kw):
        assert raw(cms, **kw) == L.ZK_E_ARG, what
        assert all((o == (FILL if o.dtype == np.uint64 else 0xA5)).all() for o in outs) and nonce.value == 0xA5, what
        assert np.array_equal(t.export_state(), before), what

    try:
        for kind, other in others.items():
            for place in range(8):
                cms = list(base)
                cms[place] = other
                refused(cms, (kind, place), a=2 if kind == "grouping" and place == 0 else 1)
        refused(grp, "grouped at log_arity 1", a=1)
        refused(base, "grinding_bits 33", g=33)
        for kw in (dict(a=0), dict(a=3), dict(f=4), dict(a=2, f=3)):
            refused(base, kw, **kw)
        with pytest.raises(ValueError):
            zk.zerocheck.prove_gate(grp[:3], grp[3:], 0, nq)
        with pytest.raises(ValueError):
            zk.zerocheck.prove_gate(base[:2], base[2:], 0, nq)
        # what was refused in one company is still good for a proof in another (of a false statement: the tables are random)
        for cms, a in ((base, 1), ([base[0]] * 2 + base[2:], 2), (grp, 2)):
            got = zk.zerocheck.prove_gate(cms[:3], cms[3:], 0, nq, log_arity=a)
            assert not zk.zerocheck.verify_gate([c.root for c in cms], got)
    finally:
        for c in every:
            c.free()
