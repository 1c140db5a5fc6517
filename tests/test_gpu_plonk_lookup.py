"""GPU: the Plonk proof with lookup rows over FRI commitments (csrc/plonk_lookup.cuh, csrc/zkmle_plonk_lookup.hip; include/zkmle.h "Plonk with
lookups: gate, wiring, public inputs and lookup rows in one sumcheck"), over BLS12-381 Fr and BN254 Fr.  Everything is byte for byte against
tests/_plonk_lookup_model.py; no tolerance anywhere.

  round      zk_plonk_lookup_round equals the model (explicit id tables) for every length 2^1 .. 2^13 in both forms and fields, r among 0, 1,
             p - 1 and random, log_step among 0, 1 and 5 with a random id_base; the folded twenty-one equal mle_fold_last (zk_mle_fold's
             result), the inputs are unchanged
  fused      independent of the model: for the same tables and challenges g5 = zk_plonk_round's g5 on the fifteen of the proof without lookups
             + alpha^4 zk_lookup_round's g5 on the lookup's ten called with mu' = mu^2 / alpha^4, node by node
  operands   at 2^10 entries in both forms: all twenty-one tables all p - 1, all zeros, E zero, alpha = 0, mu = 0, a zero denominator in Dw and
             in Dt, qK not boolean, entries from {0, p - 1, random}, and a satisfied circuit with the true helpers (g(0) + g(1) = c)
  stride     the second trip of the grid-stride loop: one child process (tests/_plonk_lookup_worker.py) with ZK_REDUCE_BLOCKS=64 runs the hook
             on BLS12-381 Fr in round 0's form at 2^16 entries and in the fold form at 2^17 against the model
  prove      every output equals the model's: d = 1 .. 8 over both blow-ups, the three schedules, with and without a coset, both fields, l among
             0, 1 and a few, no, some and all rows lookup rows; once at d = 12; once with 8 bits of proof of work.  M and the five helper roots
             equal zk_lookup_multiplicities / zk_wiring_fractions / zk_lookup_fractions + fri.commit on the same inputs; a second proof is
             identical; a false gate row, a false wiring and a lookup miss are each proved with ZK_OK, `misses` as the model counts them, and
             not verified; a caller's transcript ends in the verifier's state
  pair       on the d = 6 XOR circuit of tests/test_gpu_lookup.py the fused proof verifies, and plonk.prove + lookup.prove on the same fifteen
             commitments verify too: the same statements, other bytes
  refusals   a commitment of another d, field, blow-up, coset or grouping in any of the fifteen places, grouped ones at log_arity = 1,
             grinding_bits = 33, npublic > 2^d, no array with npublic > 0, an unreduced public value: ZK_E_ARG, nothing written, the transcript
             as it was"""
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
import _lookup_model as LM
import _ntt_model as NM
import _plonk_lookup_model as KL
import _zerocheck_gate_model as ZG
from oracle import pymodel as M
from test_gpu_fri import table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (0, 3)
Q = 6
T = KL.TABLES
SCHEDULES = [(1, False), (2, False), (2, True)]
sched_id = lambda s: "a%d%s" % (s[0], "g" if s[1] else "")
LOOKUP_TEN = KL.LOOKUP_PLACES + (KL.E_PLACE,)


def elem(zk, field, v):
    return zk.from_ints(field, [v])[0]


def ints_of(zk, field, arr):
    return [int(v) for v in zk.to_ints(field, np.ascontiguousarray(arr))]


# ---- the round pass -----------------------------------------------------------------------------------------------------------------------
def hook_ids(n_summed, log_step, id_base, p):
    d = (n_summed.bit_length() - 1) + log_step
    return [[(j * (1 << d) + id_base + (1 << log_step) * x) % p for x in range(n_summed)] for j in range(3)]


def check_round(zk, field, tabs, ch, r, what, id_base=0, log_step=0, fused=False):
    """both the hook's outputs against the model on the twenty-one integer tables `tabs`; r = None: round 0's form.  fused: also against the
    two hooks of the pair of proofs (needs alpha != 0)"""
    p = NM.MODULUS[field]
    dev = [table_of(zk, field, t) for t in tabs]
    before = [t.evaluated_values.copy() for t in dev]
    els = [elem(zk, field, v) for v in ch]
    kw = dict(id_base=elem(zk, field, id_base), log_step=log_step)
    if r is None:
        g5 = zk.plonk_lookup.round(dev, *els, **kw)
        want = tabs
    else:
        folded, g5 = zk.plonk_lookup.round(dev, *els, r=elem(zk, field, r), **kw)
        want = [ML.mle_fold_last(field, t, r) for t in tabs]
        assert len(folded) == T
        for got, w in zip(folded, want):
            assert len(got) == len(w) and np.array_equal(got.evaluated_values, to_mont(zk, field, w)), what
    g, _ = KL.round_g5(want, hook_ids(len(want[0]), log_step, id_base, p), ch, p)
    assert g5.shape == (5, 4) and np.array_equal(g5, to_mont(zk, field, g)), what
    for t, b in zip(dev, before):
        assert np.array_equal(t.evaluated_values, b), what
    if fused:
        beta, gamma, alpha, mu = ch
        rr = {} if r is None else dict(r=elem(zk, field, r))
        a4 = pow(alpha, 4, p)
        mu2 = mu * mu * pow(a4, -1, p) % p
        gp = zk.plonk.round([dev[j] for j in KL.PLONK_PLACES], *els, **kw, **rr)
        gl = zk.lookup.round([dev[j] for j in LOOKUP_TEN], els[0], els[1], elem(zk, field, mu2), **rr)
        gp, gl = (x if r is None else x[1] for x in (gp, gl))
        both = [(w + a4 * v) % p for w, v in zip(ints_of(zk, field, gp), ints_of(zk, field, gl))]
        assert both == g and ints_of(zk, field, g5) == both, what
    return g


@pytest.mark.parametrize("loglens", ((1, 11), (12, 12), (13, 13)), ids=("2p1-2p11", "2p12", "2p13"))
@pytest.mark.parametrize("fold", (False, True), ids=("round0", "fold"))
@pytest.mark.parametrize("field", FIELDS)
def test_round_equals_the_model_at_every_length(zk, field, fold, loglens):
    p = NM.MODULUS[field]
    rng = random.Random(17200 + field + 2 * fold + loglens[0])
    for loglen in range(max(loglens[0], 2 if fold else 1), loglens[1] + 1):
        n = 1 << loglen
        tabs = [NM.random_ints(field, n, 17300 + 17 * loglen + j + field) for j in range(T)]
        r = (0, 1, p - 1, rng.randrange(p))[loglen % 4] if fold else None
        ch = tuple(rng.randrange(p) for _ in range(4))
        check_round(zk, field, tabs, ch, r, (loglen, r), id_base=rng.randrange(p) if loglen % 3 else 0, log_step=(0, 1, 5)[loglen % 3])


@pytest.mark.parametrize("fold", (False, True), ids=("round0", "fold"))
@pytest.mark.parametrize("field", FIELDS)
def test_round_is_the_sum_of_the_two_passes_it_fuses(zk, field, fold):
    p = NM.MODULUS[field]
    rng = random.Random(17400 + field + 2 * fold)
    for loglen in (1 + fold, 5, 9, 11):
        n = 1 << loglen
        tabs = [NM.random_ints(field, n, 17450 + 17 * loglen + j + field) for j in range(T)]
        ch = tuple(rng.randrange(1, p) for _ in range(4))
        check_round(zk, field, tabs, ch, rng.randrange(p) if fold else None, ("fused", loglen), id_base=rng.randrange(p), log_step=loglen % 3, fused=True)


@pytest.mark.parametrize("fold", (False, True), ids=("round0", "fold"))
@pytest.mark.parametrize("field", FIELDS)
def test_round_at_operands_random_tables_never_reach(zk, field, fold):
    p = NM.MODULUS[field]
    rng = random.Random(17500 + field + 2 * fold)
    r = rng.choice((0, 1, p - 1, rng.randrange(p))) if fold else None
    n, d = 1 << 10, 10                                        # four workgroups of a fold pass, eight of round 0's
    rnd = [NM.random_ints(field, n, 17600 + j + field) for j in range(T)]
    ch = tuple(rng.randrange(1, p) for _ in range(4))
    beta, gamma, alpha, mu = ch
    step = dict(id_base=r, log_step=1) if fold else {}        # the ids that go with the tables after one fold by r: c_1 = r, step 2
    check_round(zk, field, [[p - 1] * n] * T, (p - 1,) * 4, r, "all p - 1", id_base=p - 1, log_step=5)
    check_round(zk, field, [[0] * n] * T, ch, r, "zeros", **step)
    check_round(zk, field, rnd[:20] + [[0] * n], ch, r, "E zero: only mu's terms", **step)
    check_round(zk, field, rnd, (beta, gamma, 0, mu), r, "alpha = 0: only wire A's term and the plain sums", **step)
    check_round(zk, field, rnd, (beta, gamma, alpha, 0), r, "mu = 0", **step)
    # a zero denominator: Dw at every even entry, Dt at every entry divisible by three
    g2 = gamma * gamma % p
    zw = [list(t) for t in rnd]
    for x in range(0, n, 2):
        zw[0][x] = -(beta + gamma * zw[1][x] + g2 * zw[2][x]) % p
    for x in range(0, n, 3):
        zw[12][x] = -(beta + gamma * zw[13][x] + g2 * zw[14][x]) % p
    assert all(LM.denominators(KL.lookup_tables(zw), x, beta, gamma)[0] % p == 0 for x in range(0, n, 2))
    assert all(LM.denominators(KL.lookup_tables(zw), x, beta, gamma)[1] % p == 0 for x in range(0, n, 3))
    check_round(zk, field, zw, ch, r, "zero denominators", fused=True, **step)
    # qK not boolean: the relation is a polynomial identity in qK, whatever the statement means then
    nb = [list(t) for t in rnd]
    nb[11] = [(0, 1, 2, p - 1, rng.randrange(p))[x % 5] for x in range(n)]
    check_round(zk, field, nb, ch, r, "qK not boolean", fused=True, **step)
    mixed = [[rng.choice((0, p - 1, rng.randrange(p))) for _ in range(n)] for _ in range(T)]
    check_round(zk, field, mixed, ch, r, "0, p - 1, random", fused=True, **step)
    # a satisfied circuit with the true helpers: the message sums to the claimed sum
    tabs, pub = KL.circuit(field, d, 17700 + field, 5)
    true = tabs + KL.helper_tables(tabs, beta, gamma, p) + [rnd[20]]
    prev, own = KL.round_g5(true, KL.WM.id_tables(d), ch, p, KL.pi_table(pub, d))
    c = alpha ** 3 * sum(a * b for a, b in zip(KL.pi_table(pub, d), rnd[20])) % p
    assert (own[0] + own[1]) % p == 0 and (prev[0] + prev[1]) % p == c and c != 0
    g = check_round(zk, field, true, ch, r, "a satisfied circuit with the true helpers", **step)
    assert g == prev if r is None else (g[0] + g[1]) % p == KL.interpolate5(prev, r, p)


def test_the_second_trip_of_the_grid_stride_loop():
    e = dict(os.environ, ZK_REDUCE_BLOCKS="64")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_plonk_lookup_worker.py")], capture_output=True, text=True, env=e, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["trips"] == {"round0": 2, "fold": 2}, out
    assert out["mismatches"] == [] and out["checked"] == 2, out


# ---- the prover ---------------------------------------------------------------------------------------------------------------------------
def hasher(zk):
    return FC.hasher(zk, True)


def model_statement(zk, field, d, b, coset, grouped, seed, l, looked="some", **false):
    tabs, pub = KL.circuit(field, d, seed, l, looked, **false)
    assert KL.satisfied(tabs, pub, NM.MODULUS[field]) == (not false.get("false_gate"), not false.get("false_wiring"), false.get("miss") is None)
    return [(GM if grouped else PM).commit(field, t, b, coset, hasher(zk)) for t in tabs], pub


def assert_same_proof(zk, got, pr):
    fl = KL.flat(zk, pr)
    op = got.opening
    for name, arr in (("h_roots", got.h_roots), ("drawn", got.drawn), ("polys", got.round_polys), ("challenges", got.challenges), ("ys", got.ys), ("gamma", op.gamma),
                      ("open_polys", op.round_polys), ("roots", op.roots), ("final", op.final_table), ("open_challenges", op.challenges),
                      ("indices", op.query_indices), ("values", op.query_values), ("paths", op.query_paths)):
        assert arr.shape == fl[name].shape and np.array_equal(arr, fl[name]), name
    assert op.pow_nonce == pr["nonce"]
    assert np.array_equal(got.point[0], fl["points"][0])
    return fl


def gpu_prove(zk, gcs, pub, f, a, **kw):
    return zk.plonk_lookup.prove(gcs[:3], gcs[3:8], gcs[8:11], gcs[11], gcs[12:], pub, f, Q, log_arity=a, **kw)


def check_helpers(zk, field, cms, got, b, coset, grouped):
    """M and the five helper roots from the hooks that existed before, on the committed tables and the challenges the proof drew"""
    n = len(cms[0]["coeffs"])
    beta, gamma = got.drawn[0], got.drawn[1]
    tabs = [table_of(zk, field, cm["coeffs"]) for cm in cms]
    lk = [tabs[j] for j in KL.LOOKUP_PLACES[:7]]
    m, misses = zk.lookup.multiplicities(lk)
    hs = [zk.wiring.fractions(tabs[j], tabs[8 + j], j * n, beta, gamma) for j in range(3)]
    hl = zk.lookup.fractions(lk + [m], beta, gamma)
    cs = None if coset == 1 else elem(zk, field, coset)
    for j, t in enumerate([m] + hs + [hl]):
        c = zk.fri.commit(t, b, cs, log_group=2 if grouped else 0)
        try:
            assert c.root == got.h_roots[j].tobytes(), j
        finally:
            c.free()
    return misses


def prove_case(zk, field, d, b, f, with_coset, sched, l, looked="some", g_bits=0, seed=0):
    a, grouped = sched
    coset = FC.coset_of(field, d, b, with_coset, 73)
    cms, pub = model_statement(zk, field, d, b, coset, grouped, 17800 + 23 * d + field + seed, l, looked)
    pr = KL.prove(cms, pub, f, Q, a, KL.pow_transcript(d, f, g_bits) if g_bits else None, hasher(zk))
    assert KL.verify(pr, tr=KL.pow_transcript(d, f, g_bits, pr["nonce"]) if g_bits else None, hasher=hasher(zk)) == (True, None)
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    pm = to_mont(zk, field, pub) if l else None
    try:
        words = [gc.codeword().evaluated_values.copy() for gc in gcs] if d <= 8 else None
        got = gpu_prove(zk, gcs, pm, f, a, grinding_bits=g_bits)
        assert isinstance(got, zk.plonk_lookup.PlonkLookupProof) and isinstance(got.opening, zk.fri.FriMlWideOpening) and got.round_polys.shape == (d, 5, 4)
        assert_same_proof(zk, got, pr)
        roots = [gc.root for gc in gcs]
        assert roots == pr["roots"] and zk.plonk_lookup.verify(roots, pm, got)
        j = next(i for i in range(1, 15) if roots[i] != roots[0])   # at d = 1 a wiring can make A and B one table
        swapped = list(roots)
        swapped[0], swapped[j] = roots[j], roots[0]
        assert not zk.plonk_lookup.verify(swapped, pm, got)
        st = zk.plonk_lookup.last_stats()
        assert st["rounds"] == d and st["ms_total"] > 0 and st["misses"] == 0
        assert check_helpers(zk, field, cms, got, b, coset, grouped) == 0
        # the claims of the fifteen are the tables' values at the reversed challenges, by the call that existed before
        for j, cm in enumerate(cms):
            y = table_of(zk, field, cm["coeffs"]).evaluate(np.ascontiguousarray(got.challenges[::-1]))
            assert np.array_equal(y, got.ys[j]), j
        # the commitments were only read: their codewords are what they were, and a second proof from their coefficient tables is identical
        if words is not None:
            assert all(np.array_equal(gc.codeword().evaluated_values, c) for gc, c in zip(gcs, words))
        again = gpu_prove(zk, gcs, pm, f, a, grinding_bits=g_bits)
        assert_same_proof(zk, again, pr)
    finally:
        for gc in gcs:
            gc.free()


# d = 1 .. 8 under every schedule it allows; blow-up, coset, log_final in (0, 1, d - 1), the field, the lookup rows and l among 0, 1, a few rotate
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
            looked = ("some", "all", "none")[(d + 2 * s) % 3]
            l = (0, 1, min(3, 1 << d))[(d + s) % 3]
            out.append(pytest.param(FIELDS[k % 2], d, 1 + (d + s // 2) % 2, f, k % 4 < 2, sched, l, looked,
                                    id="f%d-d%d-%s-l%d-%s" % (FIELDS[k % 2], d, sched_id(sched), l, looked)))
    return out


@pytest.mark.parametrize("field,d,b,f,with_coset,sched,l,looked", grid())
def test_prove_equals_the_model(zk, field, d, b, f, with_coset, sched, l, looked):
    prove_case(zk, field, d, b, f, with_coset, sched, l, looked)


def test_prove_at_d_12(zk):
    prove_case(zk, 0, 12, 1, 1, True, (2, True), 1)


def test_prove_with_proof_of_work(zk):
    prove_case(zk, 3, 6, 2, 1, True, (2, True), 3, g_bits=8)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_false_statements_are_proved_and_not_verified(zk, sched):
    field, d, b, f, l = 3, 5, 1, 1, 3
    a, grouped = sched
    for false in (dict(false_gate=True), dict(false_wiring=True), dict(miss=7)):
        cms, pub = model_statement(zk, field, d, b, 1, grouped, 17900, l, **false)
        pr = KL.prove(cms, pub, f, Q, a, hasher=hasher(zk))
        assert KL.verify(pr, hasher=hasher(zk)) == (False, 0) and (pr["misses"] >= 1) == ("miss" in false)
        gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
        try:
            pm = to_mont(zk, field, pub)
            got = gpu_prove(zk, gcs, pm, f, a)                # ZK_OK: the wrapper raises on anything else
            assert_same_proof(zk, got, pr)
            assert zk.plonk_lookup.last_stats()["misses"] == pr["misses"]
            assert not zk.plonk_lookup.verify([gc.root for gc in gcs], pm, got)
        finally:
            for gc in gcs:
                gc.free()


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_prove_on_a_callers_transcript(zk, sched):
    field, d, b, f, l = 0, 6, 1, 1, 3
    a, grouped = sched
    cms, pub = model_statement(zk, field, d, b, FC.coset_of(field, d, b, True, 73), grouped, 18000, l)
    mt = M.Transcript()
    mt.append(b"before the circuit")
    pr = KL.prove(cms, pub, f, Q, a, mt, hasher(zk))
    t, v, want = zk.Transcript(), zk.Transcript(), zk.Transcript()
    t.append(b"before the circuit")
    v.append(b"before the circuit")
    want.append(bytes(mt.buf))
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    pm = to_mont(zk, field, pub)
    try:
        got = gpu_prove(zk, gcs, pm, f, a, transcript=t)
    finally:
        for gc in gcs:
            gc.free()
    assert_same_proof(zk, got, pr)
    assert zk.plonk_lookup.verify(pr["roots"], pm, got, transcript=v)
    assert np.array_equal(t.export_state(), want.export_state()) and np.array_equal(v.export_state(), want.export_state())
    assert not zk.plonk_lookup.verify(pr["roots"], pm, got)   # bound to the prior content


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_the_fused_proof_and_the_pair_of_proofs_state_the_same(zk, sched):
    """the d = 6 circuit of tests/test_gpu_lookup.py: every third row is a lookup into the 3-bit XOR table (its gate selectors are zero, qK = 1);
    the others are additions and multiplications with qK = 0; no cell is wired to another"""
    field, d, b, f = 3, 6, 1, 1
    a, grouped = sched
    p, n, rng = NM.MODULUS[field], 1 << d, random.Random(16500)
    A, B, Cc, qM, qL, qR, qO, qC, qK = ([0] * n for _ in range(9))
    for x in range(n):
        if x % 3 == 0:
            A[x], B[x] = rng.randrange(8), rng.randrange(8)
            Cc[x], qK[x] = A[x] ^ B[x], 1
        else:
            A[x], B[x], mul = rng.randrange(p), rng.randrange(p), rng.randrange(2)
            Cc[x] = A[x] * B[x] % p if mul else (A[x] + B[x]) % p
            qM[x], qL[x], qR[x], qO[x] = mul, 1 - mul, 1 - mul, p - 1
    assert all(ZG.gate(*row) % p == 0 for row in zip(A, B, Cc, qM, qL, qR, qO, qC))
    Tc = zk.plonk_lookup.table_columns(d, [(u, v, u ^ v) for u in range(8) for v in range(8)])
    sig = zk.plonk_lookup.sigma_from_cycles(d, [])
    tabs = [A, B, Cc, qM, qL, qR, qO, qC] + sig + [qK] + Tc
    assert KL.satisfied(tabs, [], p) == (True, True, True) and sum(qK) == 22
    coset = FC.coset_of(field, d, b, True, 61)
    cms = [(GM if grouped else PM).commit(field, t, b, coset, hasher(zk)) for t in tabs]
    pr = KL.prove(cms, [], f, Q, a, hasher=hasher(zk))
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    roots = [cm["root"] for cm in cms]
    try:
        fused = gpu_prove(zk, gcs, None, f, a)
        assert_same_proof(zk, fused, pr)
        assert zk.plonk_lookup.verify(roots, None, fused) and zk.plonk_lookup.last_stats()["misses"] == 0
        t, v = zk.Transcript(), zk.Transcript()
        pp = zk.plonk.prove(gcs[:3], gcs[3:8], gcs[8:11], None, f, Q, log_arity=a, transcript=t)
        pl = zk.lookup.prove(gcs[:3], gcs[11], gcs[12:], f, Q, log_arity=a, transcript=t)
        assert zk.plonk.verify(roots[:11], None, pp, transcript=v) and zk.lookup.verify(roots[:3] + roots[11:], pl, transcript=v)
        assert np.array_equal(t.export_state(), v.export_state())
        # the same statements, other bytes: two points, two openings
        assert not np.array_equal(fused.challenges, pp.challenges) and not np.array_equal(pp.challenges, pl.challenges)
        assert fused.opening.query_paths.size < pp.opening.query_paths.size + pl.opening.query_paths.size
    finally:
        for gc in gcs:
            gc.free()


def test_refusals_write_nothing(zk):
    from zkmle_amd import _lib as L
    lib = zk.lib()
    nq = 8
    mk = lambda field, d, b, coset, lg, seed: zk.fri.commit(zk.MultilinearPolynomial.random(field, 1 << d, seed), b, coset, log_group=lg)
    base = [mk(3, 4, 1, None, 0, 1 + j) for j in range(15)]
    others = {"d": mk(3, 5, 1, None, 0, 31), "blow-up": mk(3, 4, 2, None, 0, 32), "field": mk(0, 4, 1, None, 0, 33), "coset": mk(3, 4, 1, elem(zk, 3, 5), 0, 34),
              "grouping": mk(3, 4, 1, None, 2, 35)}
    grp = [mk(3, 4, 1, None, 2, 41 + j) for j in range(15)]
    every = base + list(others.values()) + grp
    FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
    w = lambda n: np.full(n, FILL, np.uint64)
    by = lambda n: np.full(n, 0xA5, np.uint8)
    hr, drawn, polys, chal, ys, gamma, opolys, roots, fin, ochal, idx, vals, paths = (by(160), w(4 * 9), w(20 * 5), w(4 * 5), w(80), w(4), w(12 * 5), by(32 * 40), w(4 << 5),
                                                                                       w(4 * 5), w(nq), w(4 * nq * 400), by(32 * nq * 3200))
    outs = (hr, drawn, polys, chal, ys, gamma, opolys, roots, fin, ochal, idx, vals, paths)
    nonce = C.c_uint64(0xA5)
    t = zk.Transcript()
    t.append(b"untouched")
    before = t.export_state().copy()
    good_pub = zk.from_ints(3, [5, 6, 7])

    def raw(cms, a=1, f=0, g=0, pub=good_pub, l=None):
        arr = (C.c_void_p * 15)(*[c._h for c in cms])
        l = (0 if pub is None else pub.shape[0]) if l is None else l
        return lib.zk_plonk_lookup_prove(arr, None if pub is None else L.p64(pub), l, f, nq, a, g, t._h, L.p8(hr), L.p64(drawn), L.p64(polys), L.p64(chal), L.p64(ys),
                                         L.p64(gamma), L.p64(opolys), L.p8(roots), L.p64(fin), L.p64(ochal), L.p64(idx), L.p64(vals), L.p8(paths), C.byref(nonce))

    def refused(cms, what, **kw):
        assert raw(cms, **kw) == L.ZK_E_ARG, what
        assert all((o == (FILL if o.dtype == np.uint64 else 0xA5)).all() for o in outs) and nonce.value == 0xA5, what
        assert np.array_equal(t.export_state(), before), what

    try:
        for kind, other in others.items():
            for place in range(15):
                cms = list(base)
                cms[place] = other
                refused(cms, (kind, place), a=2 if kind == "grouping" and place == 0 else 1)
        refused(grp, "grouped at log_arity 1", a=1)
        refused(base, "grinding_bits 33", g=33)
        for kw in (dict(a=0), dict(a=3), dict(f=4), dict(a=2, f=3)):
            refused(base, kw, **kw)
        # the public inputs
        refused(base, "npublic > 2^d", pub=zk.from_ints(3, list(range(17))))
        refused(base, "no array with npublic > 0", pub=None, l=1)
        unreduced = good_pub.copy()
        unreduced[1] = np.uint64(0xFFFFFFFFFFFFFFFF)
        refused(base, "an unreduced public value", pub=unreduced)
        with pytest.raises(ValueError):
            gpu_prove(zk, grp, None, 0, 1)
        with pytest.raises(ValueError):
            zk.plonk_lookup.prove(base[:2], base[2:8], base[8:11], base[11], base[12:], None, 0, nq)
        # what was refused in one company is still good for a proof in another (of a false statement: the tables are random)
        for cms, a, pub in ((base, 1, good_pub), ([base[0]] * 2 + base[2:], 2, None), (grp, 2, zk.from_ints(3, list(range(16))))):
            got = zk.plonk_lookup.prove(cms[:3], cms[3:8], cms[8:11], cms[11], cms[12:], pub, 0, nq, log_arity=a)
            assert not zk.plonk_lookup.verify([c.root for c in cms], pub, got)
    finally:
        for c in every:
            c.free()
