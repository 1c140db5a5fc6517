"""GPU: the zerocheck of a product over three FRI commitments (csrc/zerocheck.cuh zerocheck_mul_round_kernel, csrc/zkmle_zerocheck.hip; include/zkmle.h
"Zerocheck of a product of committed tables"), over BLS12-381 Fr and BN254 Fr.  Everything is byte for byte; no tolerance anywhere.

  round     zk_zerocheck_mul_round equals the model of tests/_zerocheck_model.py for every table length 2^1 .. 2^15 (one lane, under a wave, one
            workgroup, two, up to 64 workgroups a reduction), in both forms and both fields, r among 0, 1, p - 1 and random; the folded
            tables equal mle_fold_last, the inputs are unchanged; and at the operands random tables never reach: all four tables all p - 1,
            E all zero, C = A o B exactly (g(0) + g(1) = 0 then, at every length), entries drawn from {0, p - 1, random}
  stride    the second trip of the grid-stride loop: one child process (tests/_zerocheck_worker.py mul) with ZK_REDUCE_BLOCKS=64 runs round
            0's form at 2^16 entries and the fold form at 2^17, on random tables and on tables all p - 1 with r = p - 1, against the same
            model; the child reports the cap it ran with
  finish    finish_sums_kernel above 256 partials a sum: round 0's form at 2^18 entries under the default cap (512 workgroups), random
            tables and all p - 1
  prove     with C = A o B in Python integers every output equals the model's: d = 1 .. 10 with both blow-ups, the three schedules, with and
            without a coset, log_final among 0, 1, d - 1 and both fields spread over them; once at d = 15; once with 8 bits of proof of work.
            ys = zk_mle_evaluate of each table at the reversed challenges; verify_mul accepts; a false statement is proved and not verified;
            a caller's transcript ends in the verifier's state
  refusals  commitments of different d, field, blow-up or grouping, and grouped ones at log_arity = 1: ZK_E_ARG, nothing written"""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import _fri_ml_cases as FC
import _fri_ml_grouped_model as GM
import _fri_ml_model as ML
import _fri_pcs_model as PM
import _ntt_model as NM
import _zerocheck_model as ZM
from oracle import pymodel as M
from test_gpu_fri import table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (0, 3)
Q = 6
SCHEDULES = [(1, False), (2, False), (2, True)]
sched_id = lambda s: "a%d%s" % (s[0], "g" if s[1] else "")


def elem(zk, field, v):
    return zk.from_ints(field, [v])[0]


def check_round(zk, field, tabs, r, what):
    """both the hook's outputs against the model on the integer tables `tabs` = (A, B, C, E); r = None: round 0's form"""
    p = NM.MODULUS[field]
    dev = [table_of(zk, field, t) for t in tabs]
    before = [t.evaluated_values.copy() for t in dev]
    if r is None:
        g4 = zk.zerocheck.mul_round(*dev)
        want = tabs
    else:
        *folded, g4 = zk.zerocheck.mul_round(*dev, r=elem(zk, field, r))
        want = [ML.mle_fold_last(field, t, r) for t in tabs]
        for got, w in zip(folded, want):
            assert len(got) == len(w) and np.array_equal(got.evaluated_values, to_mont(zk, field, w)), what
    g = ZM.round_g4(*want, p)
    assert np.array_equal(g4, to_mont(zk, field, g)), what
    for t, b in zip(dev, before):
        assert np.array_equal(t.evaluated_values, b), what
    return g


@pytest.mark.parametrize("fold", (False, True), ids=("round0", "fold"))
@pytest.mark.parametrize("field", FIELDS)
def test_round_equals_the_model_at_every_length(zk, field, fold):
    p = NM.MODULUS[field]
    rng = random.Random(4100 + field + 2 * fold)
    for loglen in range(2 if fold else 1, 16):
        n = 1 << loglen
        tabs = [NM.random_ints(field, n, 4200 + 7 * loglen + j + field) for j in range(4)]
        r = (0, 1, p - 1, rng.randrange(p))[loglen % 4] if fold else None
        check_round(zk, field, tabs, r, (loglen, r))


@pytest.mark.parametrize("fold", (False, True), ids=("round0", "fold"))
@pytest.mark.parametrize("field", FIELDS)
def test_round_at_operands_random_tables_never_reach(zk, field, fold):
    p = NM.MODULUS[field]
    rng = random.Random(4300 + field + 2 * fold)
    rs = (0, 1, p - 1, rng.randrange(p)) if fold else (None,)
    n = 1 << 10                                               # four workgroups of a fold pass, eight of round 0's
    rnd = [NM.random_ints(field, n, 4400 + j + field) for j in range(4)]
    for r in rs:
        check_round(zk, field, [[p - 1] * n] * 4, r, "all p - 1")
        check_round(zk, field, rnd[:3] + [[0] * n], r, "E zero")
        check_round(zk, field, [[0] * n, rnd[1], [p - 1] * n, rnd[3]], r, "A zero, C all p - 1")
        mixed = [[rng.choice((0, p - 1, rng.randrange(p))) for _ in range(n)] for _ in range(4)]
        check_round(zk, field, mixed, r, "0, p - 1, random")
    # C = A o B exactly: the polynomial vanishes on the cube, so g(0) = g(1) = 0 in round 0's form, and before a fold the sum over the cube is 0
    for loglen in (1, 2, 6, 9, 12):
        m = 1 << loglen
        A, B, E = (NM.random_ints(field, m, 4500 + 3 * loglen + j + field) for j in range(3))
        Cc = [a * b % p for a, b in zip(A, B)]
        g = check_round(zk, field, [A, B, Cc, E], None, ("C = A o B", loglen))
        assert g[0] == 0 and g[1] == 0
        if fold and loglen >= 2:
            for r in rs:
                g = check_round(zk, field, [A, B, Cc, E], r, ("C = A o B folded", loglen, r))
                assert (g[0] + g[1]) % p == ZM.interpolate4(ZM.round_g4(A, B, Cc, E, p), r, p)


def run_stride_worker(kernel):
    """tests/_zerocheck_worker.py for `kernel` ("mul" or "gate") in a fresh process with the reduction grid capped at 64 workgroups"""
    e = dict(os.environ, ZK_REDUCE_BLOCKS="64")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_zerocheck_worker.py"), kernel], capture_output=True, text=True, env=e, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["kernel"] == kernel and out["blocks"] == 64, out
    assert out["trips"] == {"round0": 2, "fold": 2}, out
    assert out["mismatches"] == [] and out["checked"] == 10, out


def test_the_second_trip_of_the_grid_stride_loop():
    run_stride_worker("mul")


# The default cap of the reduction grids (mle_kernels.cuh reduce_block_cap, 1536 workgroups of 256 lanes) and the lanes of the one workgroup
# of finish_sums_kernel, which adds the workgroups' partial sums: past 256 partials a sum, each of its lanes adds a second one.
REDUCE_BLOCK = 256


def reduce_grid_for(work):
    cap = min(max(int(os.environ.get("ZK_REDUCE_BLOCKS", "1536")), 64), 16384)     # this process's cap, as the library reads it
    return max(1, min(-(-work // REDUCE_BLOCK), cap))


@pytest.mark.parametrize("kind", ("random", "all p - 1"))
def test_the_finishing_kernel_above_256_partials(zk, kind):
    """round 0's form at 2^18 entries is 2^17 pairs: 512 workgroups at the default cap, one pair a lane, so what is new here is
    finish_sums_kernel, every lane of which adds two partials of each of the four sums.  The passes of the wiring, Plonk, lookup and
    Plonk-with-lookups provers hand their partials to the same kernel in the same layout (partials[sum * grid + block]) with 7 sums for 4:
    its loop over the sums is the one run here."""
    field, n = 0, 1 << 18
    p = NM.MODULUS[field]
    grid = reduce_grid_for(n // 2)
    assert grid == 512 and -(-grid // REDUCE_BLOCK) == 2
    tabs = [NM.random_ints(field, n, 4600 + j) for j in range(4)] if kind == "random" else [[p - 1] * n] * 4
    check_round(zk, field, tabs, None, kind)


# ---- the prover ---------------------------------------------------------------------------------------------------------------------------
def hasher(zk):
    return FC.hasher(zk, True)


def model_commitments(zk, field, d, b, coset, grouped, seed, false_at=None):
    p = NM.MODULUS[field]
    A, B = NM.random_ints(field, 1 << d, seed), NM.random_ints(field, 1 << d, seed + 1)
    Cc = [x * y % p for x, y in zip(A, B)]
    if false_at is not None:
        Cc[false_at] = (Cc[false_at] + 1) % p
    return [(GM if grouped else PM).commit(field, t, b, coset, hasher(zk)) for t in (A, B, Cc)]


def assert_same_proof(zk, got, pr):
    fl = ZM.flat(zk, pr)
    op = got.opening
    for name, arr in (("tau", got.tau), ("polys", got.round_polys), ("challenges", got.challenges), ("ys", got.ys), ("gamma", op.gamma),
                      ("open_polys", op.round_polys), ("roots", op.roots), ("final", op.final_table), ("open_challenges", op.challenges),
                      ("indices", op.query_indices), ("values", op.query_values), ("paths", op.query_paths)):
        assert arr.shape == fl[name].shape and np.array_equal(arr, fl[name]), name
    assert op.pow_nonce == pr["nonce"]
    assert np.array_equal(got.point[0], fl["points"][0])


def prove_case(zk, field, d, b, f, with_coset, sched, g_bits=0, seed=0):
    a, grouped = sched
    coset = FC.coset_of(field, d, b, with_coset, 53)
    cms = model_commitments(zk, field, d, b, coset, grouped, 5100 + 23 * d + field + seed)
    pr = ZM.prove(cms, f, Q, a, ZM.pow_transcript(d, f, g_bits) if g_bits else None, hasher(zk))
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    try:
        got = zk.zerocheck.prove_mul(*gcs, f, Q, log_arity=a, grinding_bits=g_bits)
        assert_same_proof(zk, got, pr)
        roots = [gc.root for gc in gcs]
        assert roots == pr["roots"] and zk.zerocheck.verify_mul(roots, got)
        assert not zk.zerocheck.verify_mul([roots[2], roots[1], roots[0]], got)
        st = zk.zerocheck.last_stats()
        assert st["rounds"] == d and st["ms_total"] > 0
        # the claims are the tables' values at the reversed challenges, by the call that existed before
        for j, cm in enumerate(cms):
            y = table_of(zk, field, cm["coeffs"]).evaluate(np.ascontiguousarray(got.challenges[::-1]))
            assert np.array_equal(y, got.ys[j]), j
        # the commitments were only read: they open as before
        again = zk.zerocheck.prove_mul(*gcs, f, Q, log_arity=a, grinding_bits=g_bits)
        assert_same_proof(zk, again, pr)
    finally:
        for gc in gcs:
            gc.free()


# d = 1 .. 10 under every schedule it allows; blow-up, coset, log_final in (0, 1, d - 1) and the field rotate so that each d meets both
# blow-ups and each schedule every log_final
def grid():
    out = []
    for d in range(1, 11):
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


def test_prove_at_d_15(zk):
    prove_case(zk, 0, 15, 1, 1, True, (2, True))


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_prove_with_proof_of_work(zk, sched):
    prove_case(zk, 3, 6, 2, 1, True, sched, g_bits=8)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_a_false_statement_is_proved_and_not_verified(zk, sched):
    field, d, b, f = 3, 5, 1, 1
    a, grouped = sched
    cms = model_commitments(zk, field, d, b, 1, grouped, 5300, false_at=19)
    pr = ZM.prove(cms, f, Q, a, hasher=hasher(zk))
    assert ZM.verify(pr, hasher=hasher(zk)) == (False, 0)
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    try:
        got = zk.zerocheck.prove_mul(*gcs, f, Q, log_arity=a)
        assert_same_proof(zk, got, pr)
        assert not zk.zerocheck.verify_mul([gc.root for gc in gcs], got)
    finally:
        for gc in gcs:
            gc.free()


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_prove_on_a_callers_transcript(zk, sched):
    field, d, b, f = 0, 6, 1, 1
    a, grouped = sched
    cms = model_commitments(zk, field, d, b, FC.coset_of(field, d, b, True, 53), grouped, 5400)
    mt = M.Transcript()
    mt.append(b"before the zerocheck")
    pr = ZM.prove(cms, f, Q, a, mt, hasher(zk))
    t, v, want = zk.Transcript(), zk.Transcript(), zk.Transcript()
    t.append(b"before the zerocheck")
    v.append(b"before the zerocheck")
    want.append(bytes(mt.buf))
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    try:
        got = zk.zerocheck.prove_mul(*gcs, f, Q, log_arity=a, transcript=t)
    finally:
        for gc in gcs:
            gc.free()
    assert_same_proof(zk, got, pr)
    assert zk.zerocheck.verify_mul(pr["roots"], got, transcript=v)
    assert np.array_equal(t.export_state(), want.export_state()) and np.array_equal(v.export_state(), want.export_state())
    assert not zk.zerocheck.verify_mul(pr["roots"], got)      # bound to the prior content


def test_refusals_write_nothing(zk):
    from zkmle_amd import _lib as L
    lib = zk.lib()
    nq = 8
    mk = lambda field, d, b, coset, lg, seed: zk.fri.commit(zk.MultilinearPolynomial.random(field, 1 << d, seed), b, coset, log_group=lg)
    base, same, third = mk(3, 4, 1, None, 0, 1), mk(3, 4, 1, None, 0, 2), mk(3, 4, 1, None, 0, 3)
    other_d, other_b, other_f, cos = mk(3, 5, 1, None, 0, 4), mk(3, 4, 2, None, 0, 5), mk(0, 4, 1, None, 0, 6), mk(3, 4, 1, elem(zk, 3, 5), 0, 7)
    grp = [mk(3, 4, 1, None, 2, 8 + j) for j in range(3)]
    every = [base, same, third, other_d, other_b, other_f, cos] + grp
    FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
    w = lambda n: np.full(n, FILL, np.uint64)
    by = lambda n: np.full(n, 0xA5, np.uint8)
    tau, polys, chal, ys, gamma, opolys, roots, fin, ochal, idx, vals, paths = (w(4 * 5), w(16 * 5), w(4 * 5), w(12), w(4), w(12 * 5), by(32 * 24), w(4 << 5),
                                                                                  w(4 * 5), w(nq), w(4 * nq * 80), by(32 * nq * 600))
    outs = (tau, polys, chal, ys, gamma, opolys, roots, fin, ochal, idx, vals, paths)
    nonce = C.c_uint64(0xA5)
    t = zk.Transcript()
    t.append(b"untouched")
    before = t.export_state().copy()

    def raw(cms, a=1, f=0, g=0):
        return lib.zk_zerocheck_mul_prove(*[c._h for c in cms], f, nq, a, g, t._h, L.p64(tau), L.p64(polys), L.p64(chal), L.p64(ys), L.p64(gamma), L.p64(opolys),
                                          L.p8(roots), L.p64(fin), L.p64(ochal), L.p64(idx), L.p64(vals), L.p8(paths), C.byref(nonce))

    try:
        for cms, kw in (([base, same, other_d], {}), ([other_d, base, same], {}), ([base, other_b, same], {}), ([base, same, other_f], {}), ([other_f, base, same], {}),
                        ([base, cos, same], {}), ([base, same, grp[0]], {}), ([grp[0], base, same], dict(a=2)), (grp, dict(a=1)), ([base, same, third], dict(a=0)),
                        ([base, same, third], dict(a=3)), ([base, same, third], dict(f=4)), ([base, same, third], dict(a=2, f=3)), ([base, same, third], dict(g=33))):
            assert raw(cms, **kw) == L.ZK_E_ARG, kw
            assert all((o == (FILL if o.dtype == np.uint64 else 0xA5)).all() for o in outs) and nonce.value == 0xA5, kw
            assert np.array_equal(t.export_state(), before), kw
        with pytest.raises(ValueError):
            zk.zerocheck.prove_mul(*grp, 0, nq)
        # what was refused in one company is still good for a proof in another (of a false statement: the tables are random)
        for cms, a in (([base, same, third], 1), ([base, base, same], 2), (grp, 2)):
            got = zk.zerocheck.prove_mul(*cms, 0, nq, log_arity=a)
            assert not zk.zerocheck.verify_mul([c.root for c in cms], got)
            assert zk.fri.verify_multilinear_batch([c.root for c in cms], got.point, got.opening) is False   # its transcript starts elsewhere
    finally:
        for c in every:
            c.free()
