"""GPU: the lookup argument over FRI commitments (csrc/lookup.cuh, csrc/zkmle_lookup.hip; include/zkmle.h "Lookup: rows of a committed
table"), over BLS12-381 Fr and BN254 Fr.  Everything is byte for byte against tests/_lookup_model.py; no tolerance anywhere.

  multiplicities  zk_lookup_multiplicities equals the model (a dict, the smallest index of a repeated row) for every length 2^1 .. 2^14, each
             input run twice with identical output and the inputs unchanged: random instances; a table whose rows are all equal with every
             witness row hitting it (M[0] = n); a repeated row whose copies lie at the first and the last index and in different 2048-entry
             tiles; rows that differ only in T2, or only in the top or the bottom 32-bit limb (as stored) of one column; elements at p - 1 and
             0; qK all 0, all 1, and values other than 0 and 1 (not counted); k rows that are in no table row, with misses == k
  fractions  zk_lookup_fractions equals the model for every length 2^1 .. 2^14 (below, at and above one inversion tile of 2048 entries); zero
             denominators forced into Dw and into Dt at the first and the last slot of a tile, twice within one lane's batch and in every
             slot of one lane's batch: every other entry is exact and the zero's own share follows inv0; tables all p - 1, gamma = 0,
             everything zero; the inputs are unchanged
  round      zk_lookup_round equals the model for every length 2^1 .. 2^13 in both forms and fields, r among 0, 1, p - 1 and random; the
             folded tables equal mle_fold_last, the inputs are unchanged; at 2^10 entries: all ten tables all p - 1, E zero, mu = 0, H zero,
             qK and M zero, gamma = 0, entries from {0, p - 1, random}, and a satisfied instance with the true M and H (g(0) + g(1) = 0 in
             round 0's form, the previous quartic at r after a fold)
  stride     the second trip of the grid-stride loop: one child process (tests/_lookup_worker.py) with ZK_REDUCE_BLOCKS=64 runs round 0's form
             at 2^16 entries and the fold form at 2^17
  prove      every output equals the model's: d = 1 .. 8 over both blow-ups, the three schedules, with and without a coset, log_final among
             0, 1, d - 1, both fields, a range-style table (a short table padded by repetition) and a random table; once at d = 12; once with
             8 bits of proof of work.  ys = zk_mle_evaluate of each table at the reversed challenges; a second proof is identical; a false
             statement is proved with ZK_OK and misses >= 1 and not verified; a caller's transcript ends in the verifier's state
  refusals   a commitment of another d, field, blow-up, coset or grouping in any of the seven places, grouped ones at log_arity = 1,
             grinding_bits = 33: ZK_E_ARG, nothing written, the transcript as it was.  d > 31 cannot be reached with a commitment (the fields'
             two-adicity is 32 and 28, and a table of 2^32 elements is 128 GiB): zk_lookup_prove compares d with 31 before anything else that
             reads it, and tests/test_lookup_cpu.py checks the same bound on zk_lookup_multiplicities with a wrapped table of 2^32 entries
  with 7o    one circuit at d = 6 whose rows are gates or lookups into the 3-bit XOR table: plonk.prove and lookup.prove on one caller's
             transcript, one after the other, both verify on one verifier transcript, which ends where the prover's does"""
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
import _plonk_model as KM
import _zerocheck_gate_model as ZG
from oracle import pymodel as M
from test_gpu_fri import table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (0, 3)
Q = 6
SCHEDULES = [(1, False), (2, False), (2, True)]
sched_id = lambda s: "a%d%s" % (s[0], "g" if s[1] else "")
TILE = 2048                                                   # entries of one inversion tile: 256 lanes of 8


def elem(zk, field, v):
    return zk.from_ints(field, [v])[0]


# ---- the multiplicities -------------------------------------------------------------------------------------------------------------------
def check_multiplicities(zk, field, tabs, what):
    """the hook twice on the seven integer tables against the model -> (M, misses)"""
    p = NM.MODULUS[field]
    dev = [table_of(zk, field, t) for t in tabs]
    before = [t.evaluated_values.copy() for t in dev]
    want, lost = LM.multiplicities(tabs, p)
    want_m = to_mont(zk, field, want)
    for turn in range(2):
        m, misses = zk.lookup.multiplicities(dev)
        assert len(m) == len(tabs[0]) and np.array_equal(m.evaluated_values, want_m), (what, turn)
        assert misses == lost, (what, turn)
    for t, b in zip(dev, before):
        assert np.array_equal(t.evaluated_values, b), what
    return want, lost


def stored_variants(zk, field, rng):
    """six triples as integers: a base row, one that differs from it in T2 only, and four that differ in one 32-bit limb as stored (the top
    or the bottom one of T1, of T0).  The stored words are made here (top word below 2^60, so below p whatever the flipped bit) and turned
    into the integers they stand for"""
    word = lambda: [rng.getrandbits(64), rng.getrandbits(64), rng.getrandbits(64), rng.getrandbits(59)]
    base = [word(), word(), word()]
    rows = [base, [base[0], base[1], word()]]
    for col in (1, 0):
        for limb_word, bit in ((3, 32 + 27), (0, 5)):          # bit 27 of the top 32-bit limb; bit 5 of the bottom one
            row = [list(w) for w in base]
            row[col][limb_word] ^= 1 << bit
            rows.append(row)
    flat = np.array([w for row in rows for w in row], np.uint64)
    ints = zk.to_ints(field, flat)
    assert (to_mont(zk, field, ints) == flat).all()
    return [tuple(int(v) for v in ints[3 * i:3 * i + 3]) for i in range(len(rows))]


def multiplicity_inputs(zk, field, loglen, kind, seed):
    p, rng, n = NM.MODULUS[field], random.Random(seed), 1 << loglen
    if kind == "random":
        return LM.instance(field, loglen, seed)
    if kind == "all equal":
        return LM.instance(field, loglen, seed, rows=[tuple(rng.randrange(p) for _ in range(3))], looked={x: 0 for x in range(n)})
    if kind == "repeated":
        rows = [tuple(rng.randrange(p) for _ in range(3)) for _ in range(n)]
        for y in {0, n - 1, n // 2, min(n - 1, TILE + 5), min(n - 1, 3 * TILE - 1)}:
            rows[y] = rows[n - 1]
        return LM.instance(field, loglen, seed, rows=rows, looked={x: (n - 1 if x % 2 else rng.randrange(n)) for x in range(n)})
    if kind == "near rows":
        rows = stored_variants(zk, field, rng)[:n]
        return LM.instance(field, loglen, seed, rows=rows, looked={x: (x * x + x // 3) % len(rows) for x in range(n) if x % 5})
    if kind == "edges":
        rows = [(0, 0, 0), (p - 1, p - 1, p - 1), (0, p - 1, 0), (p - 1, 0, p - 1), (0, 0, p - 1), (1, 0, 0)][:n]
        return LM.instance(field, loglen, seed, rows=rows, looked={x: rng.randrange(len(rows)) for x in range(n) if x % 7 != 3})
    tabs = LM.instance(field, loglen, seed, looked={x: 0 for x in range(n)})      # every row holds table row 0
    if kind == "qK all 0":
        tabs[3] = [0] * n
    elif kind == "qK not boolean":
        tabs[3] = [(1, 2, p - 1, 0, rng.randrange(2, p))[x % 5] for x in range(n)]
    else:
        assert kind == "qK all 1"
    return tabs


KINDS = ("random", "all equal", "repeated", "near rows", "edges", "qK all 0", "qK all 1", "qK not boolean")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", FIELDS)
def test_multiplicities_equal_the_model_at_every_length(zk, field, kind):
    p = NM.MODULUS[field]
    for loglen in range(1, 15):
        n = 1 << loglen
        tabs = multiplicity_inputs(zk, field, loglen, kind, 13000 + 17 * loglen + field + KINDS.index(kind))
        m, misses = check_multiplicities(zk, field, tabs, (kind, loglen))
        assert misses == 0
        counted = sum(1 for v in tabs[3] if v % p == 1)
        assert sum(m) == counted
        if kind == "all equal":
            assert m == [n] + [0] * (n - 1)
        if kind == "repeated":
            assert m[n - 1] == 0 and m[0] >= n // 2
        if kind == "qK all 0":
            assert m == [0] * n
        if kind == "qK all 1":
            assert counted == n and m[0] == n
        if kind == "qK not boolean":
            assert counted == (n + 4) // 5


@pytest.mark.parametrize("field", FIELDS)
def test_multiplicities_count_the_misses(zk, field):
    p = NM.MODULUS[field]
    rng = random.Random(13500 + field)
    for loglen in range(1, 15):
        n = 1 << loglen
        tabs = LM.instance(field, loglen, 13600 + loglen + field)
        k = min(n, 1 + loglen % 4 + (70 if loglen > 8 else 0))                  # more than a wave's worth of them at the larger lengths
        for x in rng.sample(range(n), k):
            tabs = LM.falsified(tabs, x, p)
        m, misses = check_multiplicities(zk, field, tabs, ("misses", loglen))
        assert misses == k
    # a whole table of misses: every wave adds once
    tabs = LM.instance(field, 10, 13700 + field, looked={})
    tabs[3] = [1] * (1 << 10)
    assert check_multiplicities(zk, field, tabs, "every row a miss") == ([0] * (1 << 10), 1 << 10)


# ---- the helper table ---------------------------------------------------------------------------------------------------------------------
def check_fractions(zk, field, tabs, beta, gamma, what):
    p = NM.MODULUS[field]
    dev = [table_of(zk, field, t) for t in tabs]
    before = [t.evaluated_values.copy() for t in dev]
    H = zk.lookup.fractions(dev, elem(zk, field, beta), elem(zk, field, gamma))
    want = LM.fractions(tabs, beta, gamma, p)
    assert len(H) == len(tabs[0]) and np.array_equal(H.evaluated_values, to_mont(zk, field, want)), what
    for t, b in zip(dev, before):
        assert np.array_equal(t.evaluated_values, b), what
    return want


@pytest.mark.parametrize("field", FIELDS)
def test_fractions_equal_the_model_at_every_length(zk, field):
    p = NM.MODULUS[field]
    rng = random.Random(14100 + field)
    for loglen in range(1, 15):
        n = 1 << loglen
        if loglen % 2:
            tabs = [NM.random_ints(field, n, 14200 + 11 * loglen + j + field) for j in range(8)]
        else:
            tabs = LM.instance(field, loglen, 14300 + loglen + field)
            tabs.append(LM.multiplicities(tabs, p)[0])
        want = check_fractions(zk, field, tabs, rng.randrange(p), rng.randrange(p), loglen)
        assert loglen % 2 or sum(want) % p == 0              # a satisfied instance with the true M: the fractions sum to zero


@pytest.mark.parametrize("field", FIELDS)
def test_fractions_with_zero_denominators(zk, field):
    p = NM.MODULUS[field]
    rng = random.Random(14400 + field)
    n = 2 * TILE
    lane = lambda l: [l + 256 * t for t in range(8)]          # the entries of one lane's batch in the first tile
    places = {"the first slot of a tile": [0], "the last slot of a tile": [TILE - 1], "the first slot of the second tile": [TILE], "the last slot": [n - 1],
              "twice within one lane's batch": [5, 5 + 256 * 3], "every slot of one lane's batch": lane(9), "two lanes' batches": lane(0) + lane(255)}
    for turn, (what, xs) in enumerate(places.items()):
        beta, gamma = rng.randrange(p), rng.randrange(1, p)
        for kind in ("wires", "table", "both"):
            tabs = [NM.random_ints(field, n, 14500 + 10 * turn + j) for j in range(8)]
            for x in xs:
                if kind in ("wires", "both"):
                    tabs[0][x] = (-beta - gamma * tabs[1][x] - gamma * gamma * tabs[2][x]) % p      # Dw = 0
                if kind in ("table", "both"):
                    tabs[4][x] = (-beta - gamma * tabs[5][x] - gamma * gamma * tabs[6][x]) % p      # Dt = 0
            want = check_fractions(zk, field, tabs, beta, gamma, (what, kind))
            for x in xs:                                                 # the zero's own share follows inv0
                dw, dt = (v % p for v in LM.denominators(tabs, x, beta, gamma))
                assert (dw == 0) == (kind != "table") and (dt == 0) == (kind != "wires")
                assert want[x] == (tabs[3][x] * LM.inv0(dw, p) - tabs[7][x] * LM.inv0(dt, p)) % p and (kind != "both" or want[x] == 0)
    beta, gamma = rng.randrange(p), rng.randrange(1, p)
    check_fractions(zk, field, [[p - 1] * n] * 8, p - 1, p - 1, "all p - 1")
    check_fractions(zk, field, [NM.random_ints(field, n, 14600 + j) for j in range(8)], beta, 0, "gamma = 0")
    assert check_fractions(zk, field, [[0] * n] * 8, 0, 0, "everything zero: every denominator is zero") == [0] * n
    ones = [NM.random_ints(field, n, 14700 + j) for j in range(3)] + [[1] * n] + [[0] * n] * 4
    assert check_fractions(zk, field, ones, 0, gamma, "the table's denominators all zero, M zero") == [LM.inv0(LM.denominators(ones, x, 0, gamma)[0], p) for x in range(n)]


# ---- the round pass -----------------------------------------------------------------------------------------------------------------------
def check_round(zk, field, tabs, ch, r, what):
    """both the hook's outputs against the model on the ten integer tables `tabs` = (A, B, C, qK, T0, T1, T2, M, H, E); r = None: round 0's form"""
    p = NM.MODULUS[field]
    dev = [table_of(zk, field, t) for t in tabs]
    before = [t.evaluated_values.copy() for t in dev]
    els = [elem(zk, field, v) for v in ch]
    if r is None:
        g5 = zk.lookup.round(dev, *els)
        want = tabs
    else:
        folded, g5 = zk.lookup.round(dev, *els, r=elem(zk, field, r))
        want = [ML.mle_fold_last(field, t, r) for t in tabs]
        assert len(folded) == 10
        for got, w in zip(folded, want):
            assert len(got) == len(w) and np.array_equal(got.evaluated_values, to_mont(zk, field, w)), what
    g = LM.round_g5(want, ch, p)
    assert g5.shape == (5, 4) and np.array_equal(g5, to_mont(zk, field, g)), what
    for t, b in zip(dev, before):
        assert np.array_equal(t.evaluated_values, b), what
    return g


@pytest.mark.parametrize("loglens", ((1, 11), (12, 13)), ids=("2p1-2p11", "2p12-2p13"))
@pytest.mark.parametrize("fold", (False, True), ids=("round0", "fold"))
@pytest.mark.parametrize("field", FIELDS)
def test_round_equals_the_model_at_every_length(zk, field, fold, loglens):
    p = NM.MODULUS[field]
    rng = random.Random(15000 + field + 2 * fold + loglens[0])
    for loglen in range(max(loglens[0], 2 if fold else 1), loglens[1] + 1):
        n = 1 << loglen
        tabs = [NM.random_ints(field, n, 15100 + 11 * loglen + j + field) for j in range(10)]
        r = (0, 1, p - 1, rng.randrange(p))[loglen % 4] if fold else None
        check_round(zk, field, tabs, tuple(rng.randrange(p) for _ in range(3)), r, (loglen, r))


@pytest.mark.parametrize("fold", (False, True), ids=("round0", "fold"))
@pytest.mark.parametrize("field", FIELDS)
def test_round_at_operands_random_tables_never_reach(zk, field, fold):
    p = NM.MODULUS[field]
    rng = random.Random(15200 + field + 2 * fold)
    rs = (0, 1, p - 1, rng.randrange(p)) if fold else (None,)
    n, d = 1 << 10, 10                                        # four workgroups of a fold pass, eight of round 0's
    rnd = [NM.random_ints(field, n, 15300 + j + field) for j in range(10)]
    ch = tuple(rng.randrange(1, p) for _ in range(3))
    beta, gamma, mu = ch
    zero = [0] * n
    given = LM.instance(field, d, 15400 + field)
    m = LM.multiplicities(given, p)[0]
    true = given + [m, LM.fractions(given + [m], beta, gamma, p), rnd[9]]
    prev = LM.round_g5(true, ch, p)
    assert (prev[0] + prev[1]) % p == 0
    for r in rs:
        check_round(zk, field, [[p - 1] * n] * 10, (p - 1,) * 3, r, "all p - 1")
        check_round(zk, field, rnd[:9] + [zero], ch, r, "E zero: only mu's term")
        check_round(zk, field, rnd, (beta, gamma, 0), r, "mu = 0")
        check_round(zk, field, rnd, (beta, 0, mu), r, "gamma = 0")
        check_round(zk, field, rnd, (0, 0, mu), r, "beta = gamma = 0")
        check_round(zk, field, rnd[:8] + [zero, rnd[9]], ch, r, "H zero")
        g = check_round(zk, field, rnd[:3] + [zero] + rnd[4:7] + [zero, zero, rnd[9]], ch, r, "qK, M and H zero")
        assert g == [0] * 5
        mixed = [[rng.choice((0, p - 1, rng.randrange(p))) for _ in range(n)] for _ in range(10)]
        check_round(zk, field, mixed, ch, r, "0, p - 1, random")
        g = check_round(zk, field, true, ch, r, "a satisfied instance with the true M and H")
        if r is None:
            assert (g[0] + g[1]) % p == 0
        else:
            assert (g[0] + g[1]) % p == LM.interpolate5(prev, r, p)


def test_the_second_trip_of_the_grid_stride_loop():
    e = dict(os.environ, ZK_REDUCE_BLOCKS="64")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_lookup_worker.py")], capture_output=True, text=True, env=e, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["trips"] == {"round0": 2, "fold": 2}, out
    assert out["mismatches"] == [] and out["checked"] == 2, out


# ---- the prover ---------------------------------------------------------------------------------------------------------------------------
def hasher(zk):
    return FC.hasher(zk, True)


def instance_of(kind, field, d, seed):
    """a range-style table (v, v^2, v xor 5 for v < 5, padded by repeating its last row) or a random one"""
    rows = [(v, v * v, v ^ 5) for v in range(min(5, 1 << d))] if kind == "range" else None
    return LM.instance(field, d, seed, rows)


def model_commitments(zk, field, d, b, coset, grouped, seed, kind="random", false=False):
    p = NM.MODULUS[field]
    tabs = instance_of(kind, field, d, seed)
    if false:
        tabs = LM.falsified(tabs, (1 << d) // 2, p)
    assert LM.satisfied(tabs, p) is not false
    return [(GM if grouped else PM).commit(field, t, b, coset, hasher(zk)) for t in tabs]


def assert_same_proof(zk, got, pr):
    fl = LM.flat(zk, pr)
    op = got.opening
    for name, arr in (("h_roots", got.h_roots), ("drawn", got.drawn), ("polys", got.round_polys), ("challenges", got.challenges), ("ys", got.ys), ("gamma", op.gamma),
                      ("open_polys", op.round_polys), ("roots", op.roots), ("final", op.final_table), ("open_challenges", op.challenges),
                      ("indices", op.query_indices), ("values", op.query_values), ("paths", op.query_paths)):
        assert arr.shape == fl[name].shape and np.array_equal(arr, fl[name]), name
    assert op.pow_nonce == pr["nonce"]
    assert np.array_equal(got.point[0], fl["points"][0])


def lookup_prove(zk, gcs, f, a, **kw):
    return zk.lookup.prove(gcs[:3], gcs[3], gcs[4:], f, Q, log_arity=a, **kw)


def prove_case(zk, field, d, b, f, with_coset, sched, kind="random", g_bits=0, seed=0):
    a, grouped = sched
    coset = FC.coset_of(field, d, b, with_coset, 61)
    cms = model_commitments(zk, field, d, b, coset, grouped, 16000 + 23 * d + field + seed, kind)
    pr = LM.prove(cms, f, Q, a, LM.pow_transcript(d, f, g_bits) if g_bits else None, hasher(zk))
    assert LM.verify(pr, tr=LM.pow_transcript(d, f, g_bits, pr["nonce"]) if g_bits else None, hasher=hasher(zk)) == (True, None)
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    try:
        got = lookup_prove(zk, gcs, f, a, grinding_bits=g_bits)
        assert isinstance(got, zk.lookup.LookupProof) and isinstance(got.opening, zk.fri.FriMlBatchOpening) and got.round_polys.shape == (d, 5, 4)
        assert_same_proof(zk, got, pr)
        roots = [gc.root for gc in gcs]
        assert roots == pr["roots"] and zk.lookup.verify(roots, got)
        assert not zk.lookup.verify([roots[1], roots[0]] + roots[2:], got)
        st = zk.lookup.last_stats()
        assert st["rounds"] == d and st["misses"] == 0 and st["ms_total"] > 0
        # the claims of the seven are the tables' values at the reversed challenges, by the call that existed before
        for j, cm in enumerate(cms):
            y = table_of(zk, field, cm["coeffs"]).evaluate(np.ascontiguousarray(got.challenges[::-1]))
            assert np.array_equal(y, got.ys[j]), j
        assert np.array_equal(table_of(zk, field, pr["M"]).evaluate(np.ascontiguousarray(got.challenges[::-1])), got.ys[7])
        # the commitments were only read: a second proof from them is identical
        again = lookup_prove(zk, gcs, f, a, grinding_bits=g_bits)
        assert_same_proof(zk, again, pr)
    finally:
        for gc in gcs:
            gc.free()


# d = 1 .. 8 under every schedule it allows; blow-up, coset, log_final in (0, 1, d - 1), the field and the kind of table rotate so that each d
# meets both blow-ups and each schedule every log_final (tests/test_gpu_wiring.py's grid)
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
            kind = ("random", "range")[(d + s) % 2]
            out.append(pytest.param(FIELDS[k % 2], d, 1 + (d + s // 2) % 2, f, k % 4 < 2, sched, kind, id="f%d-d%d-%s-%s" % (FIELDS[k % 2], d, sched_id(sched), kind)))
    return out


@pytest.mark.parametrize("field,d,b,f,with_coset,sched,kind", grid())
def test_prove_equals_the_model(zk, field, d, b, f, with_coset, sched, kind):
    prove_case(zk, field, d, b, f, with_coset, sched, kind)


def test_prove_at_d_12(zk):
    prove_case(zk, 0, 12, 1, 1, True, (2, True), "range")


def test_prove_with_proof_of_work(zk):
    prove_case(zk, 3, 6, 2, 1, True, (2, True), g_bits=8)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_a_false_statement_is_proved_and_not_verified(zk, sched):
    field, d, b, f = 3, 5, 1, 1
    a, grouped = sched
    cms = model_commitments(zk, field, d, b, 1, grouped, 16300, "range", false=True)
    pr = LM.prove(cms, f, Q, a, hasher=hasher(zk))
    assert pr["misses"] == 1 and LM.verify(pr, hasher=hasher(zk)) == (False, 0)
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    try:
        got = lookup_prove(zk, gcs, f, a)                     # ZK_OK: the prover does not check the statement
        assert zk.lookup.last_stats()["misses"] == 1
        assert_same_proof(zk, got, pr)
        assert not zk.lookup.verify([gc.root for gc in gcs], got)
    finally:
        for gc in gcs:
            gc.free()


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_prove_on_a_callers_transcript(zk, sched):
    field, d, b, f = 0, 6, 1, 1
    a, grouped = sched
    cms = model_commitments(zk, field, d, b, FC.coset_of(field, d, b, True, 61), grouped, 16400)
    mt = M.Transcript()
    mt.append(b"before the lookup")
    pr = LM.prove(cms, f, Q, a, mt, hasher(zk))
    t, v, want = zk.Transcript(), zk.Transcript(), zk.Transcript()
    t.append(b"before the lookup")
    v.append(b"before the lookup")
    want.append(bytes(mt.buf))
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    try:
        got = lookup_prove(zk, gcs, f, a, transcript=t)
    finally:
        for gc in gcs:
            gc.free()
    assert_same_proof(zk, got, pr)
    assert zk.lookup.verify(pr["roots"], got, transcript=v)
    assert np.array_equal(t.export_state(), want.export_state()) and np.array_equal(v.export_state(), want.export_state())
    assert not zk.lookup.verify(pr["roots"], got)             # bound to the prior content


def test_refusals_write_nothing(zk):
    from zkmle_amd import _lib as L
    lib = zk.lib()
    nq = 8
    mk = lambda field, d, b, coset, lg, seed: zk.fri.commit(zk.MultilinearPolynomial.random(field, 1 << d, seed), b, coset, log_group=lg)
    base = [mk(3, 4, 1, None, 0, 1 + j) for j in range(7)]
    others = {"d": mk(3, 5, 1, None, 0, 11), "blow-up": mk(3, 4, 2, None, 0, 12), "field": mk(0, 4, 1, None, 0, 13), "coset": mk(3, 4, 1, elem(zk, 3, 5), 0, 14),
              "grouping": mk(3, 4, 1, None, 2, 15)}
    grp = [mk(3, 4, 1, None, 2, 21 + j) for j in range(7)]
    every = base + list(others.values()) + grp
    FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
    w = lambda n: np.full(n, FILL, np.uint64)
    by = lambda n: np.full(n, 0xA5, np.uint8)
    hr, drawn, polys, chal, ys, gamma, opolys, roots, fin, ochal, idx, vals, paths = (by(64), w(4 * 8), w(20 * 5), w(4 * 5), w(36), w(4), w(12 * 5), by(32 * 32), w(4 << 5),
                                                                                       w(4 * 5), w(nq), w(4 * nq * 180), by(32 * nq * 1400))
    outs = (hr, drawn, polys, chal, ys, gamma, opolys, roots, fin, ochal, idx, vals, paths)
    nonce = C.c_uint64(0xA5)
    t = zk.Transcript()
    t.append(b"untouched")
    before = t.export_state().copy()

    def raw(cms, a=1, f=0, g=0):
        arr = (C.c_void_p * 7)(*[c._h for c in cms])
        return lib.zk_lookup_prove(arr, f, nq, a, g, t._h, L.p8(hr), L.p64(drawn), L.p64(polys), L.p64(chal), L.p64(ys), L.p64(gamma), L.p64(opolys),
                                   L.p8(roots), L.p64(fin), L.p64(ochal), L.p64(idx), L.p64(vals), L.p8(paths), C.byref(nonce))

    def refused(cms, what, **kw):
        assert raw(cms, **kw) == L.ZK_E_ARG, what
        assert all((o == (FILL if o.dtype == np.uint64 else 0xA5)).all() for o in outs) and nonce.value == 0xA5, what
        assert np.array_equal(t.export_state(), before), what

    try:
        for kind, other in others.items():
            for place in range(7):
                cms = list(base)
                cms[place] = other
                refused(cms, (kind, place), a=2 if kind == "grouping" and place == 0 else 1)
        refused(grp, "grouped at log_arity 1", a=1)
        refused(base, "grinding_bits 33", g=33)
        for kw in (dict(a=0), dict(a=3), dict(f=4), dict(a=2, f=3)):
            refused(base, kw, **kw)
        with pytest.raises(ValueError):
            zk.lookup.prove(grp[:3], grp[3], grp[4:], 0, nq)
        with pytest.raises(ValueError):
            zk.lookup.prove(base[:2], base[2], base[3:], 0, nq)
        # what was refused in one company is still good for a proof in another.  The tables are random: no entry of qK is the field's one, so
        # nothing is looked up and nothing missed, but qK is not boolean either and sum_x qK / Dw is not zero: the proof is not verified
        for cms, a in ((base, 1), ([base[0]] * 2 + base[2:], 2), (grp, 2)):
            got = zk.lookup.prove(cms[:3], cms[3], cms[4:], 0, nq, log_arity=a)
            assert zk.lookup.last_stats()["misses"] == 0
            assert not zk.lookup.verify([c.root for c in cms], got)
    finally:
        for c in every:
            c.free()


# ---- together with the Plonk proof --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_a_circuit_with_lookup_rows_is_proved_by_plonk_and_the_lookup_on_one_transcript(zk, sched):
    """every third row is a lookup into the 3-bit XOR table (its gate selectors are zero, qK = 1); the others are additions and
    multiplications with qK = 0; no cell is wired to another"""
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
    T = zk.lookup.table_columns(d, [(u, v, u ^ v) for u in range(8) for v in range(8)])
    assert LM.satisfied([A, B, Cc, qK] + T, p) and sum(qK) == 22
    sig = zk.wiring.identity_sigma(d)
    coset = FC.coset_of(field, d, b, True, 61)
    commit = lambda t: (GM if grouped else PM).commit(field, t, b, coset, hasher(zk))
    plonk_cms = [commit(t) for t in (A, B, Cc, qM, qL, qR, qO, qC) + tuple(sig)]
    look_cms = plonk_cms[:3] + [commit(t) for t in [qK] + T]
    prior = b"one circuit, two proofs"
    mt = M.Transcript()
    mt.append(prior)
    mp = KM.prove(plonk_cms, [], f, Q, a, mt, hasher(zk))
    ml = LM.prove(look_cms, f, Q, a, mt, hasher(zk))
    gp = [FC.gpu_commitment(zk, cm) for cm in plonk_cms]
    gl = gp[:3] + [FC.gpu_commitment(zk, cm) for cm in look_cms[3:]]
    t, v, want = zk.Transcript(), zk.Transcript(), zk.Transcript()
    t.append(prior)
    v.append(prior)
    want.append(bytes(mt.buf))
    try:
        pp = zk.plonk.prove(gp[:3], gp[3:8], gp[8:], None, f, Q, log_arity=a, transcript=t)
        pl = zk.lookup.prove(gl[:3], gl[3], gl[4:], f, Q, log_arity=a, transcript=t)
    finally:
        for gc in gp + gl[3:]:
            gc.free()
    assert_same_proof(zk, pl, ml)
    assert np.array_equal(pp.round_polys, KM.flat(zk, mp)["polys"])
    roots_p, roots_l = [cm["root"] for cm in plonk_cms], [cm["root"] for cm in look_cms]
    assert zk.plonk.verify(roots_p, None, pp, transcript=v) and zk.lookup.verify(roots_l, pl, transcript=v)
    assert np.array_equal(t.export_state(), want.export_state()) and np.array_equal(v.export_state(), want.export_state())
    assert not zk.lookup.verify(roots_l, pl)                  # the lookup's proof is bound to the Plonk proof before it
