"""GPU: the permutation check over FRI commitments (csrc/wiring.cuh, csrc/zkmle_wiring.hip; include/zkmle.h "Wiring: a permutation check over
committed tables"), over BLS12-381 Fr and BN254 Fr.  Everything is byte for byte against tests/_wiring_model.py; no tolerance anywhere.

  fractions  zk_wiring_fractions equals the model for every length 2^1 .. 2^14 (below, at and above one inversion tile of 2048 entries) with
             random beta and gamma and first among 0, n, 2 n; zero denominators forced into W and into S at the first and the last slot of a
             tile, twice within one lane's batch and in every slot of one lane's batch: every other entry is exact and the zero's own entry
             follows inv0; S = id (H is all zero), tables all p - 1, gamma = 0; the inputs are unchanged
  round      zk_wiring_round equals the model (explicit id tables) for every length 2^1 .. 2^15 in both forms and fields, r among 0, 1, p - 1
             and random, log_step among 0, 1 and 5 with a random id_base; the folded tables equal mle_fold_last, the inputs are unchanged; at
             2^10 entries: all ten tables all p - 1, E zero, mu = 0, alpha = 0, H zero with S = id (every sum is 0), entries from {0, p - 1,
             random}, and a satisfied wiring with the true H (g(0) + g(1) = 0 in round 0's form, the previous quartic at r after a fold)
  prove      every output equals the model's: d = 1 .. 8 over both blow-ups, the three schedules, with and without a coset, log_final among
             0, 1, d - 1, both fields, the identity permutation, one 3-cycle across A, B, C and random wirings; once at d = 12; once with 8
             bits of proof of work.  ys = zk_mle_evaluate of each table at the reversed challenges; a second proof is identical; a false
             statement is proved and not verified; a caller's transcript ends in the verifier's state
  refusals   a commitment of another d, field, blow-up, coset or grouping in any of the six places, grouped ones at log_arity = 1,
             grinding_bits = 33: ZK_E_ARG, nothing written, the transcript as it was
  with 7m    a satisfied circuit at d = 6 whose rows are wired (the C of one row is the A of the next): prove_gate and wiring.prove on one
             caller's transcript, one after the other, both verify, and the verifier's transcript ends where the prover's does"""
import ctypes as C
import random

import numpy as np
import pytest

import _fri_ml_cases as FC
import _fri_ml_grouped_model as GM
import _fri_ml_model as ML
import _fri_pcs_model as PM
import _ntt_model as NM
import _wiring_model as WM
import _zerocheck_gate_model as ZG
from oracle import pymodel as M
from test_gpu_fri import table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
FIELDS = (0, 3)
Q = 6
SCHEDULES = [(1, False), (2, False), (2, True)]
sched_id = lambda s: "a%d%s" % (s[0], "g" if s[1] else "")
TILE = 2048                                                   # entries of one inversion tile: 256 lanes of 8


def elem(zk, field, v):
    return zk.from_ints(field, [v])[0]


# ---- the helper tables --------------------------------------------------------------------------------------------------------------------
def check_fractions(zk, field, W, S, first, beta, gamma, what):
    p = NM.MODULUS[field]
    dw, ds = table_of(zk, field, W), table_of(zk, field, S)
    bw, bs = dw.evaluated_values.copy(), ds.evaluated_values.copy()
    H = zk.wiring.fractions(dw, ds, first, elem(zk, field, beta), elem(zk, field, gamma))
    want = WM.fractions(W, S, first, beta, gamma, p)
    assert len(H) == len(W) and np.array_equal(H.evaluated_values, to_mont(zk, field, want)), what
    assert np.array_equal(dw.evaluated_values, bw) and np.array_equal(ds.evaluated_values, bs), what
    return want


@pytest.mark.parametrize("field", FIELDS)
def test_fractions_equal_the_model_at_every_length(zk, field):
    p = NM.MODULUS[field]
    rng = random.Random(8100 + field)
    for loglen in range(1, 15):
        n = 1 << loglen
        first = (0, n, 2 * n)[loglen % 3]
        W = NM.random_ints(field, n, 8200 + 7 * loglen + field)
        S = [rng.randrange(3 * n) for _ in range(n)] if loglen % 2 else NM.random_ints(field, n, 8300 + 7 * loglen + field)
        check_fractions(zk, field, W, S, first, rng.randrange(p), rng.randrange(p), loglen)


@pytest.mark.parametrize("field", FIELDS)
def test_fractions_with_zero_denominators(zk, field):
    p = NM.MODULUS[field]
    rng = random.Random(8400 + field)
    n = 2 * TILE
    lane = lambda l: [l + 256 * t for t in range(8)]          # the entries of one lane's batch in the first tile
    places = {"the first slot of a tile": [0], "the last slot of a tile": [TILE - 1], "the first slot of the second tile": [TILE], "the last slot": [n - 1],
              "twice within one lane's batch": [5, 5 + 256 * 3], "every slot of one lane's batch": lane(9), "two lanes' batches": lane(0) + lane(255)}
    for turn, (what, xs) in enumerate(places.items()):
        first = (0, n, 2 * n)[turn % 3]
        beta, gamma = rng.randrange(p), rng.randrange(1, p)
        ginv = pow(gamma, -1, p)
        for kind in ("id", "sigma", "both"):
            W = NM.random_ints(field, n, 8500 + first + len(xs))
            S = [rng.randrange(3 * n) for _ in range(n)]
            for x in xs:
                if kind in ("id", "both"):
                    W[x] = (-beta - gamma * (first + x)) % p              # beta + W + gamma id = 0
                S[x] = first + x if kind == "both" else (-(beta + W[x]) * ginv) % p if kind == "sigma" else (S[x] if S[x] != first + x else S[x] + 1)
            want = check_fractions(zk, field, W, S, first, beta, gamma, (what, kind, first))
            for x in xs:                                                 # the zero's own entry follows inv0
                did, dsig = (beta + W[x] + gamma * (first + x)) % p, (beta + W[x] + gamma * S[x]) % p
                assert (did == 0) == (kind != "sigma") and (dsig == 0) == (kind != "id")
                assert want[x] == (WM.inv0(did, p) - WM.inv0(dsig, p)) % p and (kind != "both" or want[x] == 0)
    beta, gamma = rng.randrange(p), rng.randrange(1, p)
    W = NM.random_ints(field, n, 8600)
    assert check_fractions(zk, field, W, list(range(n, 2 * n)), n, beta, gamma, "S = id") == [0] * n
    check_fractions(zk, field, [p - 1] * n, [p - 1] * n, 2 * n, p - 1, p - 1, "all p - 1")
    assert check_fractions(zk, field, W, NM.random_ints(field, n, 8601), 0, beta, 0, "gamma = 0") == [0] * n
    check_fractions(zk, field, [0] * n, [0] * n, 0, 0, 0, "everything zero: every denominator is zero")


# ---- the round pass -----------------------------------------------------------------------------------------------------------------------
def hook_ids(n_summed, log_step, id_base, p):
    d = (n_summed.bit_length() - 1) + log_step
    return [[(j * (1 << d) + id_base + (1 << log_step) * x) % p for x in range(n_summed)] for j in range(3)]


def check_round(zk, field, tabs, ch, r, what, id_base=0, log_step=0):
    """both the hook's outputs against the model on the ten integer tables `tabs` = (A, B, C, SA, SB, SC, H0, H1, H2, E); r = None: round 0's form"""
    p = NM.MODULUS[field]
    dev = [table_of(zk, field, t) for t in tabs]
    before = [t.evaluated_values.copy() for t in dev]
    els = [elem(zk, field, v) for v in ch]
    if r is None:
        g5 = zk.wiring.round(dev, *els, id_base=elem(zk, field, id_base), log_step=log_step)
        want = tabs
    else:
        folded, g5 = zk.wiring.round(dev, *els, id_base=elem(zk, field, id_base), log_step=log_step, r=elem(zk, field, r))
        want = [ML.mle_fold_last(field, t, r) for t in tabs]
        assert len(folded) == 10
        for got, w in zip(folded, want):
            assert len(got) == len(w) and np.array_equal(got.evaluated_values, to_mont(zk, field, w)), what
    g = WM.round_g5(want, hook_ids(len(want[0]), log_step, id_base, p), ch, p)
    assert g5.shape == (5, 4) and np.array_equal(g5, to_mont(zk, field, g)), what
    for t, b in zip(dev, before):
        assert np.array_equal(t.evaluated_values, b), what
    return g


@pytest.mark.parametrize("loglens", ((1, 12), (13, 14), (15, 15)), ids=("2p1-2p12", "2p13-2p14", "2p15"))
@pytest.mark.parametrize("fold", (False, True), ids=("round0", "fold"))
@pytest.mark.parametrize("field", FIELDS)
def test_round_equals_the_model_at_every_length(zk, field, fold, loglens):
    p = NM.MODULUS[field]
    rng = random.Random(8700 + field + 2 * fold + loglens[0])
    for loglen in range(max(loglens[0], 2 if fold else 1), loglens[1] + 1):
        n = 1 << loglen
        tabs = [NM.random_ints(field, n, 8800 + 11 * loglen + j + field) for j in range(10)]
        r = (0, 1, p - 1, rng.randrange(p))[loglen % 4] if fold else None
        ch = tuple(rng.randrange(p) for _ in range(4))
        check_round(zk, field, tabs, ch, r, (loglen, r), id_base=rng.randrange(p) if loglen % 3 else 0, log_step=(0, 1, 5)[loglen % 3])


@pytest.mark.parametrize("fold", (False, True), ids=("round0", "fold"))
@pytest.mark.parametrize("field", FIELDS)
def test_round_at_operands_random_tables_never_reach(zk, field, fold):
    p = NM.MODULUS[field]
    rng = random.Random(8900 + field + 2 * fold)
    rs = (0, 1, p - 1, rng.randrange(p)) if fold else (None,)
    n, d = 1 << 10, 10                                        # four workgroups of a fold pass, eight of round 0's
    rnd = [NM.random_ints(field, n, 9000 + j + field) for j in range(10)]
    ch = tuple(rng.randrange(1, p) for _ in range(4))
    beta, gamma, alpha, mu = ch
    ident = WM.id_tables(d)
    ws, ss = WM.wiring(field, d, 9100 + field)
    hs = [WM.fractions(ws[j], ss[j], j * n, beta, gamma, p) for j in range(3)]
    true = ws + ss + hs + [rnd[9]]
    prev = WM.round_g5(true, ident, ch, p)
    assert (prev[0] + prev[1]) % p == 0
    for r in rs:
        step = dict(id_base=r, log_step=1) if fold else {}    # the ids that go with the tables after one fold by r: c_1 = r, step 2
        check_round(zk, field, [[p - 1] * n] * 10, (p - 1,) * 4, r, "all p - 1", id_base=p - 1, log_step=5)
        check_round(zk, field, rnd[:9] + [[0] * n], ch, r, "E zero: only mu's term", **step)
        check_round(zk, field, rnd, (beta, gamma, alpha, 0), r, "mu = 0", **step)
        check_round(zk, field, rnd, (beta, gamma, 0, mu), r, "alpha = 0: only wire A's term", **step)
        g = check_round(zk, field, rnd[:3] + ident + [[0] * n] * 3 + [rnd[9]], ch, r, "H zero and S = id", **step)
        assert g == [0] * 5
        mixed = [[rng.choice((0, p - 1, rng.randrange(p))) for _ in range(n)] for _ in range(10)]
        check_round(zk, field, mixed, ch, r, "0, p - 1, random", **step)
        g = check_round(zk, field, true, ch, r, "a satisfied wiring with the true H", **step)
        if r is None:
            assert (g[0] + g[1]) % p == 0
        else:
            assert (g[0] + g[1]) % p == WM.interpolate5(prev, r, p)


# ---- the prover ---------------------------------------------------------------------------------------------------------------------------
def hasher(zk):
    return FC.hasher(zk, True)


def sigma_of(kind, field, d, seed):
    """-> (wires, sigmas) of one kind of wiring: the identity, one 3-cycle across A, B, C, a random permutation"""
    n = 1 << d
    if kind == "random":
        return WM.wiring(field, d, seed)
    sig = list(range(3 * n))
    if kind == "3-cycle":
        a, b, c = 0 * n + (n - 1), 1 * n + 0, 2 * n + (n // 2)
        sig[a], sig[b], sig[c] = b, c, a
    return WM.wiring(field, d, seed, sigma=sig)


def model_commitments(zk, field, d, b, coset, grouped, seed, kind="random", false=False):
    ws, ss = WM.wiring(field, d, seed, false) if kind == "random" else sigma_of(kind, field, d, seed)
    assert WM.satisfied(ws, ss, NM.MODULUS[field]) is not false
    return [(GM if grouped else PM).commit(field, t, b, coset, hasher(zk)) for t in ws + ss]


def assert_same_proof(zk, got, pr):
    fl = WM.flat(zk, pr)
    op = got.opening
    for name, arr in (("h_roots", got.h_roots), ("drawn", got.drawn), ("polys", got.round_polys), ("challenges", got.challenges), ("ys", got.ys), ("gamma", op.gamma),
                      ("open_polys", op.round_polys), ("roots", op.roots), ("final", op.final_table), ("open_challenges", op.challenges),
                      ("indices", op.query_indices), ("values", op.query_values), ("paths", op.query_paths)):
        assert arr.shape == fl[name].shape and np.array_equal(arr, fl[name]), name
    assert op.pow_nonce == pr["nonce"]
    assert np.array_equal(got.point[0], fl["points"][0])


def prove_case(zk, field, d, b, f, with_coset, sched, kind="random", g_bits=0, seed=0):
    a, grouped = sched
    coset = FC.coset_of(field, d, b, with_coset, 61)
    cms = model_commitments(zk, field, d, b, coset, grouped, 9200 + 23 * d + field + seed, kind)
    pr = WM.prove(cms, f, Q, a, WM.pow_transcript(d, f, g_bits) if g_bits else None, hasher(zk))
    assert WM.verify(pr, tr=WM.pow_transcript(d, f, g_bits, pr["nonce"]) if g_bits else None, hasher=hasher(zk)) == (True, None)
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    try:
        got = zk.wiring.prove(gcs[:3], gcs[3:], f, Q, log_arity=a, grinding_bits=g_bits)
        assert isinstance(got, zk.wiring.WiringProof) and isinstance(got.opening, zk.fri.FriMlBatchOpening) and got.round_polys.shape == (d, 5, 4)
        assert_same_proof(zk, got, pr)
        roots = [gc.root for gc in gcs]
        assert roots == pr["roots"] and zk.wiring.verify(roots, got)
        assert not zk.wiring.verify([roots[1], roots[0]] + roots[2:], got)
        st = zk.wiring.last_stats()
        assert st["rounds"] == d and st["ms_total"] > 0
        # the claims of the six are the tables' values at the reversed challenges, by the call that existed before
        for j, cm in enumerate(cms):
            y = table_of(zk, field, cm["coeffs"]).evaluate(np.ascontiguousarray(got.challenges[::-1]))
            assert np.array_equal(y, got.ys[j]), j
        # the commitments were only read: a second proof from them is identical
        again = zk.wiring.prove(gcs[:3], gcs[3:], f, Q, log_arity=a, grinding_bits=g_bits)
        assert_same_proof(zk, again, pr)
    finally:
        for gc in gcs:
            gc.free()


# d = 1 .. 8 under every schedule it allows; blow-up, coset, log_final in (0, 1, d - 1), the field and the kind of wiring rotate so that each d
# meets both blow-ups and each schedule every log_final (tests/test_gpu_zerocheck_gate.py's grid)
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
            kind = ("random", "identity", "3-cycle")[(d + 2 * s) % 3]
            out.append(pytest.param(FIELDS[k % 2], d, 1 + (d + s // 2) % 2, f, k % 4 < 2, sched, kind, id="f%d-d%d-%s-%s" % (FIELDS[k % 2], d, sched_id(sched), kind)))
    return out


@pytest.mark.parametrize("field,d,b,f,with_coset,sched,kind", grid())
def test_prove_equals_the_model(zk, field, d, b, f, with_coset, sched, kind):
    prove_case(zk, field, d, b, f, with_coset, sched, kind)


def test_prove_at_d_12(zk):
    prove_case(zk, 0, 12, 1, 1, True, (2, True))


def test_prove_with_proof_of_work(zk):
    prove_case(zk, 3, 6, 2, 1, True, (2, True), g_bits=8)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_a_false_statement_is_proved_and_not_verified(zk, sched):
    field, d, b, f = 3, 5, 1, 1
    a, grouped = sched
    cms = model_commitments(zk, field, d, b, 1, grouped, 9300, false=True)
    pr = WM.prove(cms, f, Q, a, hasher=hasher(zk))
    assert WM.verify(pr, hasher=hasher(zk)) == (False, 0)
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    try:
        got = zk.wiring.prove(gcs[:3], gcs[3:], f, Q, log_arity=a)
        assert_same_proof(zk, got, pr)
        assert not zk.wiring.verify([gc.root for gc in gcs], got)
    finally:
        for gc in gcs:
            gc.free()


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_prove_on_a_callers_transcript(zk, sched):
    field, d, b, f = 0, 6, 1, 1
    a, grouped = sched
    cms = model_commitments(zk, field, d, b, FC.coset_of(field, d, b, True, 61), grouped, 9400)
    mt = M.Transcript()
    mt.append(b"before the wiring")
    pr = WM.prove(cms, f, Q, a, mt, hasher(zk))
    t, v, want = zk.Transcript(), zk.Transcript(), zk.Transcript()
    t.append(b"before the wiring")
    v.append(b"before the wiring")
    want.append(bytes(mt.buf))
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    try:
        got = zk.wiring.prove(gcs[:3], gcs[3:], f, Q, log_arity=a, transcript=t)
    finally:
        for gc in gcs:
            gc.free()
    assert_same_proof(zk, got, pr)
    assert zk.wiring.verify(pr["roots"], got, transcript=v)
    assert np.array_equal(t.export_state(), want.export_state()) and np.array_equal(v.export_state(), want.export_state())
    assert not zk.wiring.verify(pr["roots"], got)             # bound to the prior content


def test_refusals_write_nothing(zk):
    from zkmle_amd import _lib as L
    lib = zk.lib()
    nq = 8
    mk = lambda field, d, b, coset, lg, seed: zk.fri.commit(zk.MultilinearPolynomial.random(field, 1 << d, seed), b, coset, log_group=lg)
    base = [mk(3, 4, 1, None, 0, 1 + j) for j in range(6)]
    others = {"d": mk(3, 5, 1, None, 0, 11), "blow-up": mk(3, 4, 2, None, 0, 12), "field": mk(0, 4, 1, None, 0, 13), "coset": mk(3, 4, 1, elem(zk, 3, 5), 0, 14),
              "grouping": mk(3, 4, 1, None, 2, 15)}
    grp = [mk(3, 4, 1, None, 2, 21 + j) for j in range(6)]
    every = base + list(others.values()) + grp
    FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
    w = lambda n: np.full(n, FILL, np.uint64)
    by = lambda n: np.full(n, 0xA5, np.uint8)
    hr, drawn, polys, chal, ys, gamma, opolys, roots, fin, ochal, idx, vals, paths = (by(96), w(4 * 9), w(20 * 5), w(4 * 5), w(36), w(4), w(12 * 5), by(32 * 32), w(4 << 5),
                                                                                       w(4 * 5), w(nq), w(4 * nq * 180), by(32 * nq * 1400))
    outs = (hr, drawn, polys, chal, ys, gamma, opolys, roots, fin, ochal, idx, vals, paths)
    nonce = C.c_uint64(0xA5)
    t = zk.Transcript()
    t.append(b"untouched")
    before = t.export_state().copy()

    def raw(cms, a=1, f=0, g=0):
        arr = (C.c_void_p * 6)(*[c._h for c in cms])
        return lib.zk_wiring_prove(arr, f, nq, a, g, t._h, L.p8(hr), L.p64(drawn), L.p64(polys), L.p64(chal), L.p64(ys), L.p64(gamma), L.p64(opolys),
                                   L.p8(roots), L.p64(fin), L.p64(ochal), L.p64(idx), L.p64(vals), L.p8(paths), C.byref(nonce))

    def refused(cms, what, **kw):
        assert raw(cms, **kw) == L.ZK_E_ARG, what
        assert all((o == (FILL if o.dtype == np.uint64 else 0xA5)).all() for o in outs) and nonce.value == 0xA5, what
        assert np.array_equal(t.export_state(), before), what

    try:
        for kind, other in others.items():
            for place in range(6):
                cms = list(base)
                cms[place] = other
                refused(cms, (kind, place), a=2 if kind == "grouping" and place == 0 else 1)
        refused(grp, "grouped at log_arity 1", a=1)
        refused(base, "grinding_bits 33", g=33)
        for kw in (dict(a=0), dict(a=3), dict(f=4), dict(a=2, f=3)):
            refused(base, kw, **kw)
        with pytest.raises(ValueError):
            zk.wiring.prove(grp[:3], grp[3:], 0, nq)
        with pytest.raises(ValueError):
            zk.wiring.prove(base[:2], base[2:], 0, nq)
        # what was refused in one company is still good for a proof in another (of a false statement: the tables are random)
        for cms, a in ((base, 1), ([base[0]] * 2 + base[2:], 2), (grp, 2)):
            got = zk.wiring.prove(cms[:3], cms[3:], 0, nq, log_arity=a)
            assert not zk.wiring.verify([c.root for c in cms], got)
    finally:
        for c in every:
            c.free()


# ---- together with the gate's zerocheck ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_a_wired_circuit_is_proved_by_the_gate_and_the_wiring_on_one_transcript(zk, sched):
    """row x computes C = A + B or C = A B, and its C is the next row's A: a chain, with the copy constraints C[x] -> A[x + 1] -> C[x]"""
    field, d, b, f = 3, 6, 1, 1
    a, grouped = sched
    p, n, rng = NM.MODULUS[field], 1 << d, random.Random(9500)
    A, B, Cc, qM, qL, qR, qO, qC = ([0] * n for _ in range(8))
    A[0] = rng.randrange(p)
    for x in range(n):
        B[x] = rng.randrange(p)
        if x:
            A[x] = Cc[x - 1]
        mul = rng.randrange(2)
        Cc[x] = A[x] * B[x] % p if mul else (A[x] + B[x]) % p
        qM[x], qL[x], qR[x], qO[x] = mul, 1 - mul, 1 - mul, p - 1
    assert all(ZG.gate(*row) % p == 0 for row in zip(A, B, Cc, qM, qL, qR, qO, qC))
    sig = zk.wiring.sigma_from_cycles(d, [[(2, x), (0, x + 1)] for x in range(n - 1)])
    assert WM.satisfied([A, B, Cc], sig, p) and sig != zk.wiring.identity_sigma(d)
    coset = FC.coset_of(field, d, b, True, 61)
    cms = [(GM if grouped else PM).commit(field, t, b, coset, hasher(zk)) for t in (A, B, Cc, qM, qL, qR, qO, qC) + tuple(sig)]
    prior = b"one circuit, two proofs"
    mt = M.Transcript()
    mt.append(prior)
    mg = ZG.prove(cms[:8], f, Q, a, mt, hasher(zk))
    mw = WM.prove(cms[:3] + cms[8:], f, Q, a, mt, hasher(zk))
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    t, v, want = zk.Transcript(), zk.Transcript(), zk.Transcript()
    t.append(prior)
    v.append(prior)
    want.append(bytes(mt.buf))
    try:
        pg = zk.zerocheck.prove_gate(gcs[:3], gcs[3:8], f, Q, log_arity=a, transcript=t)
        pw = zk.wiring.prove(gcs[:3], gcs[8:], f, Q, log_arity=a, transcript=t)
    finally:
        for gc in gcs:
            gc.free()
    assert_same_proof(zk, pw, mw)
    assert np.array_equal(pg.round_polys, ZG.flat(zk, mg)["polys"])
    roots = [cm["root"] for cm in cms]
    assert zk.zerocheck.verify_gate(roots[:8], pg, transcript=v) and zk.wiring.verify(roots[:3] + roots[8:], pw, transcript=v)
    assert np.array_equal(t.export_state(), want.export_state()) and np.array_equal(v.export_state(), want.export_state())
    assert not zk.wiring.verify(roots[:3] + roots[8:], pw)    # the wiring's proof is bound to the gate's before it
