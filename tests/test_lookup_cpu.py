"""CPU: the host side of the lookup argument over FRI commitments (include/zkmle.h "Lookup: rows of a committed table").  Everything compares
byte for byte against the big-integer model of tests/_lookup_model.py:

  proofs      the model round-trips at d = 1 .. 4 on both fields under the three schedules (log_arity 1; 2; 2 with grouped leaves), with and
              without a coset, on random tables and on a range-style table padded by repetition; zk_lookup_verify and zk.lookup.verify accept
              the model's proofs
  statuses    NULL, a bad field, d + log_blowup over the two-adicity, a zero coset: a status, and a caller's transcript is as it was
  rejected    one flipped bit in each array of the proof (the two helper roots among them) and in a root the verifier holds; two of the seven
              roots swapped (A with B, T0 with T1, A with T0, qK with C); d shown as d + 1 and d - 1; a nonce off by one; a row with qK = 1
              whose triple is not in the table, differing from a table row in the third column only (the first check fails; the same row
              with qK = 0 is accepted); the prover that commits a false M and hides it from the first check (a later one fails, while the
              opening alone still verifies)
  transcript  a caller's transcript ends in the model prover's state on ZK_OK
  sizes       zk_lookup_sizes equals the model's counts
  model       the multiplicities' smallest-index rule, the builder, table_columns
  hooks       the statuses of the three kernels' entry points that need no device, len > 2^31 among them
  fixture     tests/golden/lookup_proof.bin, what tools/lookup_selftest.hip reads, is the model's proof

Commitments cannot exist without a device: the kernels and the prover run in tests/test_gpu_lookup.py."""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest

import __graft_entry__ as G
import _fri_ml_cases as FC
import _fri_ml_grouped_model as GM
import _fri_pcs_model as PM
import _lookup_model as LM
import _ntt_model as NM
from oracle import pymodel as M

zk = G.import_package()
P64, P8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
p64 = lambda a: a.ctypes.data_as(P64) if a is not None else None
p8 = lambda a: a.ctypes.data_as(P8) if a is not None else None
NEW_NAMES = ("zk_lookup_multiplicities", "zk_lookup_hash_slots", "zk_lookup_fractions", "zk_lookup_round", "zk_lookup_sizes", "zk_lookup_prove", "zk_lookup_verify", "zk_lookup_last_stats")
SCHEDULES = [(1, False), (2, False), (2, True)]              # (log_arity, grouped)
# (field, d, b, f, coset): d = 1 .. 4 on both fields, f = 0 and f = d - 1 among them; log_arity 2 runs where R = d - f >= 2
CASES = [(0, 1, 1, 0, False), (3, 1, 2, 0, True), (0, 2, 2, 0, True), (3, 2, 1, 1, False), (3, 2, 1, 0, False), (0, 3, 1, 1, False), (3, 3, 2, 0, True),
         (3, 3, 1, 2, True), (0, 4, 2, 0, True), (3, 4, 1, 2, False), (0, 4, 1, 3, False)]
Q = 4
case_id = lambda c: "-".join(str(int(v)) for v in c)
sched_id = lambda s: "a%d%s" % (s[0], "g" if s[1] else "")
runs = lambda case, sched: sched[0] == 1 or case[1] - case[3] >= 2
GRID = [pytest.param(c, s, id=case_id(c) + "-" + sched_id(s)) for c in CASES for s in SCHEDULES if runs(c, s)]

hasher = functools.partial(FC.hasher, zk, True)
padded = functools.partial(FC.padded, room=16384)
coset_of = functools.partial(FC.coset_of, mul=59)


def tables(field, d, kind="random"):
    """a satisfied instance: a random table, or a range-style one (v, v^2, v xor 5 for v < 3) padded by repeating its last row"""
    rows = [(v, v * v, v ^ 5) for v in range(min(3, 1 << d))] if kind == "range" else None
    return LM.instance(field, d, 5100 + 13 * d + field, rows)


@functools.lru_cache(maxsize=None)
def commitments(field, d, b, with_coset, grouped, kind="random", false=None):
    """false: None, or 'selected' / 'unselected': row 2^d - 1 holds table row 0 with another third column, with qK = 1 / qK = 0"""
    coset = coset_of(field, d, b, with_coset)
    p = NM.MODULUS[field]
    tabs = tables(field, d, kind)
    if false:
        tabs = LM.falsified(tabs, (1 << d) - 1, p, false == "selected")
    assert LM.satisfied(tabs, p) is (false != "selected")
    return tuple((GM if grouped else PM).commit(field, t, b, coset, hasher()) for t in tabs)


@functools.lru_cache(maxsize=None)
def proof(case, sched, kind="random", false=None, cheat=False):
    field, d, b, f, with_coset = case
    return LM.prove(list(commitments(field, d, b, with_coset, sched[1], kind, false)), f, Q, sched[0], hasher=hasher(), cheat=cheat)


def lib_verify(pr, fl=None, tr=None, g=0, nonce=0, **over):
    """zk_lookup_verify on the model's proof `pr` (flat arrays `fl`) -> (status, ok)"""
    op = pr["opening"]
    fl = LM.flat(zk, pr) if fl is None else fl
    s = {n: op[n] for n in ("d", "b", "f", "Q", "a")}
    s["lg"] = 2 if op["grouped"] else 0
    s.update({n: v for n, v in over.items() if n in s})
    coset = over.get("coset", op["coset"])
    cm = None if coset is None else zk.from_ints(op["field"], [coset])[0]
    ok = C.c_int(-1)
    rc = zk.lib().zk_lookup_verify(over.get("field", op["field"]), p8(fl["own_roots"]), s["d"], s["b"], s["f"], s["Q"], s["a"], s["lg"], p64(cm),
                                   None if tr is None else tr._h, p8(fl["h_roots"]), p64(fl["polys"]), p64(fl["ys"]), p64(fl["open_polys"]), p8(fl["roots"]),
                                   p64(fl["final"]), p64(fl["values"]), p8(fl["paths"]), g, nonce, C.byref(ok))
    return rc, ok.value


def wrapper_proof(pr, fl, g=0, nonce=0):
    """zk.lookup.LookupProof holding the model's arrays"""
    op = pr["opening"]
    cs = zk.from_ints(op["field"], [op["coset"]])[0]
    o = zk.lookup.LookupProof(op["field"], op["d"], op["b"], op["f"], op["Q"], coset=cs, log_arity=op["a"], grouped=op["grouped"], grinding_bits=g)
    assert o.round_polys.shape == fl["polys"].shape == (op["d"], 5, 4) and o.drawn.shape == fl["drawn"].shape and o.challenges.shape == fl["challenges"].shape
    assert o.h_roots.shape == fl["h_roots"].shape == (2, 32)
    q = o.opening
    assert isinstance(q, zk.fri.FriMlBatchOpening)
    assert q.roots.shape == fl["roots"].shape and q.query_values.shape == fl["values"].shape and q.query_paths.shape == fl["paths"].shape
    assert q.ys.shape == (9, 1, 4) and q.round_polys.shape == fl["open_polys"].shape
    o.round_polys, o.drawn, o.challenges, o.h_roots = fl["polys"], fl["drawn"], fl["challenges"], fl["h_roots"]
    q.ys, q.round_polys, q.roots, q.final_table, q.query_values, q.query_paths = fl["ys"].reshape(9, 1, 4), fl["open_polys"], fl["roots"], fl["final"], fl["values"], fl["paths"]
    q.pow_nonce = nonce
    return o


def swapped(seq, i, j):
    out = list(seq)
    out[i], out[j] = out[j], out[i]
    return out


def test_new_exports_are_present():
    lib = zk.lib()
    header = open(G.ROOT + "/include/zkmle.h").read()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in header, name
    assert "Lookup: rows of a committed table" in header and "zk_lookup_stats" in header
    for name in ("prove", "verify", "multiplicities", "hash_slots", "fractions", "round", "sizes", "last_stats", "LookupProof", "table_columns"):
        assert hasattr(zk.lookup, name), name
    assert zk.LookupProof is zk.lookup.LookupProof


def test_the_model_of_the_multiplicities_and_the_builder():
    for field in (0, 3):
        p = NM.MODULUS[field]
        # a repeated row is credited at its smallest index; rows nowhere in the table are counted nowhere
        T = [(1, 2, 3), (4, 5, 6), (1, 2, 3), (7, 8, 9)]
        T0, T1, T2 = LM.table_columns(2, T)
        A, B, Cc, qK = [1, 1, 7, 1], [2, 2, 8, 2], [3, 3, 9, 4], [1, 1, 1, 1]
        assert LM.multiplicities([A, B, Cc, qK, T0, T1, T2], p) == ([2, 0, 0, 1], 1)
        assert LM.multiplicities([A, B, Cc, [1, 0, 2, 0], T0, T1, T2], p) == ([1, 0, 0, 0], 0)     # qK = 2 is not a lookup
        assert LM.table_columns(3, T[:2]) == [[1] + [4] * 7, [2] + [5] * 7, [3] + [6] * 7] == zk.lookup.table_columns(3, T[:2])
        for bad in ([], [(1, 2)], [(1, 2, 3)] * 9):
            with pytest.raises(ValueError):
                zk.lookup.table_columns(3, bad)
        tabs = LM.instance(field, 5, 77 + field)
        m, misses = LM.multiplicities(tabs, p)
        assert misses == 0 and sum(m) == sum(tabs[3]) > 0 and LM.satisfied(tabs, p)
        bad = LM.falsified(tabs, 9, p)
        assert LM.multiplicities(bad, p)[1] == 1 and LM.satisfied(LM.falsified(tabs, 9, p, selected=False), p)
        # a satisfied instance: the fractions sum to zero, and with a false row they do not
        beta, gamma = 0x1234567, 0x7654321
        total = lambda t: sum(LM.fractions(t + [LM.multiplicities(t, p)[0]], beta, gamma, p)) % p
        assert total(tabs) == 0 and total(bad) != 0


@pytest.mark.parametrize("case,sched", GRID)
def test_model_proofs_pass_the_model_verifier_and_the_library_verifier(case, sched):
    field, d, b, f, with_coset = case
    a, grouped = sched
    p = NM.MODULUS[field]
    for kind in ("random", "range"):
        pr = proof(case, sched, kind)
        assert pr["misses"] == 0 and LM.verify(pr, hasher=hasher()) == (True, None)
        assert len(pr["polys"]) == d and all(len(g) == 5 for g in pr["polys"])
        assert all((g[0] + g[1]) % p == (0 if l == 0 else LM.interpolate5(pr["polys"][l - 1], pr["challenges"][l - 1], p)) for l, g in enumerate(pr["polys"]))
        assert pr["opening"]["points"] == [pr["challenges"][::-1]]
        fl = LM.flat(zk, pr)
        assert lib_verify(pr, fl) == (0, 1)
        if not with_coset:
            assert lib_verify(pr, fl, coset=None) == (0, 1)
        got = (fl["polys"].size // 4, fl["h_roots"].shape[0], fl["roots"].shape[0], fl["final"].shape[0], fl["values"].size // 4, fl["paths"].size, fl["open_polys"].size // 4)
        assert LM.sizes(d, b, f, Q, a, grouped) == got == zk.lookup.sizes(d, b, f, Q, a, grouped)
        o = wrapper_proof(pr, fl)
        assert zk.lookup.verify(pr["roots"], o)
        assert not zk.lookup.verify(pr["roots"][::-1], o)
        assert np.array_equal(o.point[0], fl["points"][0]) and np.array_equal(o.ys, fl["ys"])


def test_statuses_come_before_the_transcript_is_touched():
    from zkmle_amd import _lib as L
    pr = proof(CASES[6], SCHEDULES[0])
    fl = LM.flat(zk, pr)
    t = zk.Transcript()
    t.append(b"the caller's own")
    before = t.export_state().copy()
    for name in ("own_roots", "h_roots", "polys", "ys", "open_polys", "roots", "final", "values", "paths"):
        class Without(dict):
            def __getitem__(self, key, name=name):
                return None if key == name else dict.__getitem__(self, key)
        assert lib_verify(pr, Without(fl), t)[0] == L.ZK_E_ARG, name
    op = pr["opening"]
    lib = zk.lib()
    assert lib.zk_lookup_verify(op["field"], p8(fl["own_roots"]), 3, 2, 0, Q, 1, 0, None, t._h, p8(fl["h_roots"]), p64(fl["polys"]), p64(fl["ys"]), p64(fl["open_polys"]),
                                p8(fl["roots"]), p64(fl["final"]), p64(fl["values"]), p8(fl["paths"]), 0, 0, None) == L.ZK_E_ARG
    big = padded(fl)
    for over, want in ((dict(field=7), L.ZK_E_ARG), (dict(field=-1), L.ZK_E_ARG), (dict(field=1, coset=None), L.ZK_E_RANGE), (dict(field=2, coset=None), L.ZK_E_RANGE),
                       (dict(coset=0), L.ZK_E_ARG), (dict(d=NM.two_adicity(3) - 1, b=2), L.ZK_E_RANGE), (dict(d=31, b=2), L.ZK_E_RANGE),
                       (dict(d=0), L.ZK_E_ARG), (dict(f=3), L.ZK_E_ARG), (dict(b=0), L.ZK_E_ARG), (dict(Q=0), L.ZK_E_ARG), (dict(a=3), L.ZK_E_ARG),
                       (dict(lg=2), L.ZK_E_ARG), (dict(lg=1), L.ZK_E_ARG), (dict(a=2, f=2), L.ZK_E_ARG)):
        assert lib_verify(pr, big, t, **over) == (want, -1), over
    assert lib_verify(pr, big, t, g=33)[0] == L.ZK_E_ARG
    assert np.array_equal(t.export_state(), before)
    assert lib_verify(pr, fl, t) == (0, 0) and not np.array_equal(t.export_state(), before)   # bound to a fresh transcript; ZK_OK moves it


SPOTS = ("polys", "ys", "own_roots", "h_roots", "roots", "open_polys", "final", "values", "paths")


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
@pytest.mark.parametrize("name", SPOTS)
def test_one_flipped_bit_is_rejected(name, sched):
    for case in (CASES[8], CASES[7] if sched[0] == 1 else CASES[6]):
        pr = proof(case, sched)
        base = LM.flat(zk, pr)
        rng = random.Random(37 * len(name) + case[1] + sched[0])
        flat_size = base[name].size
        spots = {0, flat_size - 1} | {rng.randrange(flat_size) for _ in range(6)}
        if name == "h_roots":
            spots |= {31, 32}                                 # the last byte of M's root and the first of H's
        for at in sorted(spots):
            fl = {n: v.copy() for n, v in base.items()}
            view = fl[name].reshape(-1)
            view[at] ^= view.dtype.type(1 << rng.randrange(8 if view.dtype == np.uint8 else 64))
            assert lib_verify(pr, fl) == (0, 0), (case, name, at)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_swapped_roots_and_another_d_are_rejected(sched):
    case = CASES[8]                                           # d = 4, f = 0
    pr = proof(case, sched)
    base = LM.flat(zk, pr)
    for i, j in ((0, 1), (4, 5), (0, 4), (3, 2)):             # A with B; T0 with T1; A with T0; qK with C
        sw = {n: v.copy() for n, v in base.items()}
        sw["own_roots"][[i, j]] = sw["own_roots"][[j, i]]
        assert lib_verify(pr, sw) == (0, 0), (i, j)
        sw["roots"][[i, j]] = sw["roots"][[j, i]]             # ... and the proof's copy with them
        assert lib_verify(pr, sw) == (0, 0), (i, j)
        sw["ys"][[i, j]] = sw["ys"][[j, i]]                   # ... and the claims: the statement's transcript has the roots in another order
        assert lib_verify(pr, sw) == (0, 0), (i, j)
        assert LM.verify(pr, roots=swapped(pr["roots"], i, j), hasher=hasher())[0] is False
    sw = {n: v.copy() for n, v in base.items()}
    sw["h_roots"][[0, 1]] = sw["h_roots"][[1, 0]]             # the two helper roots
    assert lib_verify(pr, sw) == (0, 0)
    big = padded(base)
    assert lib_verify(pr, big) == (0, 1)
    assert lib_verify(pr, big, d=5) == (0, 0) and lib_verify(pr, big, d=3) == (0, 0)
    assert lib_verify(pr, big, f=1) == (0, 0) and lib_verify(pr, big, Q=Q + 1) == (0, 0) and lib_verify(pr, big, b=1) == (0, 0)


@pytest.mark.parametrize("field", (0, 3))
@pytest.mark.parametrize("d", (1, 2, 3, 4))
def test_a_false_row_fails_the_first_check_and_a_hidden_one_a_later_check(field, d):
    case = (field, d, 1, 0, d % 2 == 0)
    p = NM.MODULUS[field]
    for sched in SCHEDULES:
        if not runs(case, sched):
            continue
        pr = proof(case, sched, "range", "selected")          # the triple differs from table row 0 in the third column only
        assert pr["misses"] == 1 and LM.verify(pr, hasher=hasher()) == (False, 0)
        assert lib_verify(pr) == (0, 0)
        unsel = proof(case, sched, "range", "unselected")     # the same row with qK = 0
        assert unsel["misses"] == 0 and LM.verify(unsel, hasher=hasher()) == (True, None)
        assert lib_verify(unsel) == (0, 1)
        ch = proof(case, sched, "range", "selected", cheat=True)
        assert ch["M"] != pr["M"] and ch["h_roots"][0] != pr["h_roots"][0]
        ok, failed = LM.verify(ch, hasher=hasher())
        assert not ok and 1 <= failed <= d                   # a later round's sum, or the last claim: never the opening, which is honest
        assert lib_verify(ch) == (0, 0)
        # the opening alone is a good one: the claims are the tables' values
        fl = LM.flat(zk, ch)
        ok_open = C.c_int(-1)
        op = ch["opening"]
        vt = M.Transcript()
        LM._statement(vt, ch["roots"], d)
        LM._helpers(vt, ch["h_roots"], d, p)
        for g in ch["polys"]:
            for e in g:
                vt.append(LM.be32(e))
            vt.challenge(p)
        t = zk.Transcript()
        t.append(bytes(vt.buf))
        cs = zk.from_ints(field, [op["coset"]])[0]
        nine = np.concatenate([fl["own_roots"], fl["h_roots"]])
        assert zk.lib().zk_fri_ml_verify_batch(field, p8(nine), 9, d, 1, 0, Q, op["a"], 2 if op["grouped"] else 0, p64(cs), p64(fl["points"]), 1,
                                               p64(fl["ys"]), t._h, p64(fl["open_polys"]), p8(fl["roots"]), p64(fl["final"]), p64(fl["values"]),
                                               p8(fl["paths"]), C.byref(ok_open)) == 0 and ok_open.value == 1


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_the_proof_of_work_nonce(sched):
    field, d, b, f, with_coset = case = CASES[9]              # d = 4, f = 2
    G_BITS = 4
    cms = list(commitments(field, d, b, with_coset, sched[1]))
    mt = LM.pow_transcript(d, f, G_BITS)
    pr = LM.prove(cms, f, Q, sched[0], mt, hasher())
    w = pr["nonce"]
    assert mt.pow_ok and mt.nonce == w
    assert LM.verify(pr, tr=LM.pow_transcript(d, f, G_BITS, w), hasher=hasher()) == (True, None)
    fl = LM.flat(zk, pr)
    assert lib_verify(pr, fl, g=G_BITS, nonce=w) == (0, 1)
    assert lib_verify(pr, fl, g=G_BITS, nonce=w + 1) == (0, 0) and lib_verify(pr, fl, g=G_BITS, nonce=(w - 1) % (1 << 64)) == (0, 0)
    assert lib_verify(pr, fl, g=G_BITS + 1, nonce=w) == (0, 0) and lib_verify(pr, fl) == (0, 0)
    assert LM.verify(pr, tr=LM.pow_transcript(d, f, G_BITS, w + 1), hasher=hasher())[0] is False
    plain = proof(case, sched)
    assert lib_verify(plain, g=G_BITS, nonce=w) == (0, 0)     # indices drawn without the step
    o = wrapper_proof(pr, fl, G_BITS, w)
    assert zk.lookup.verify(pr["roots"], o)
    o.opening.pow_nonce = w + 1
    assert not zk.lookup.verify(pr["roots"], o)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_a_callers_transcript(sched):
    field, d, b, f, with_coset = CASES[6]
    prior = b"what the caller had absorbed before"
    cms = list(commitments(field, d, b, with_coset, sched[1]))
    mt = M.Transcript()
    mt.append(prior)
    pr = LM.prove(cms, f, Q, sched[0], mt, hasher())
    vt = M.Transcript()
    vt.append(prior)
    assert LM.verify(pr, tr=vt, hasher=hasher()) == (True, None) and vt.buf == mt.buf
    t, want = zk.Transcript(), zk.Transcript()
    t.append(prior)
    assert lib_verify(pr, tr=t) == (0, 1)
    want.append(bytes(mt.buf))
    assert np.array_equal(t.export_state(), want.export_state())
    assert lib_verify(pr) == (0, 0)                           # the proof is bound to the prior content
    other = M.Transcript()
    other.append(prior + b"!")
    pr2 = LM.prove(cms, f, Q, sched[0], other, hasher())
    assert pr2["drawn"] != pr["drawn"] and pr["drawn"] != proof(CASES[6], sched)["drawn"]
    assert pr2["h_roots"][0] == pr["h_roots"][0]              # M depends on no challenge
    t2 = zk.Transcript()
    t2.append(prior + b"!")
    assert lib_verify(pr, tr=t2) == (0, 0) and lib_verify(pr2, tr=t2) == (0, 0)   # t2 has moved on: a transcript proves once


def test_sizes():
    from zkmle_amd import _lib as L
    lib = zk.lib()

    def sizes(d, b, f, q, a, lg):
        out = [C.c_size_t(0) for _ in range(7)]
        rc = lib.zk_lookup_sizes(d, b, f, q, a, lg, *[C.byref(o) for o in out])
        return rc, tuple(int(o.value) for o in out)

    for d in (1, 2, 3, 4, 6, 10, 24):
        for b in (1, 2):
            for f in range(0, d):
                for q in (1, 8, 64):
                    for a, grouped in SCHEDULES:
                        if a == 2 and d - f < 2:
                            assert sizes(d, b, f, q, a, 2 * grouped)[0] == L.ZK_E_ARG
                            continue
                        want = (5 * d, 2) + zk.fri.ml_sizes(d, b, f, q, log_arity=a, grouped=grouped, k=9)
                        assert sizes(d, b, f, q, a, 2 * grouped) == (0, want) and LM.sizes(d, b, f, q, a, grouped) == want
                        assert zk.lookup.sizes(d, b, f, q, a, grouped) == want
    for d, b, f, q, a, lg in ((0, 1, 0, 4, 1, 0), (3, 0, 0, 4, 1, 0), (3, 1, 3, 4, 1, 0), (3, 1, 0, 0, 1, 0), (3, 1, 0, 4, 0, 0), (3, 1, 0, 4, 3, 0), (3, 1, 0, 4, 1, 2)):
        assert sizes(d, b, f, q, a, lg)[0] == L.ZK_E_ARG
    assert sizes(40, 1, 0, 8, 1, 0)[0] == L.ZK_E_RANGE
    assert lib.zk_lookup_sizes(4, 1, 0, 8, 2, 2, None, None, None, None, None, None, None) == 0
    with pytest.raises(ValueError):
        zk.lookup.sizes(4, 1, 0, 8, log_arity=1, grouped=True)


def test_prover_and_hook_statuses_without_a_device():
    from zkmle_amd import _lib as L
    lib = zk.lib()
    h = {}
    for field, n in ((0, 1), (0, 2), (0, 4), (0, 8), (0, 6), (1, 8), (3, 4), (0, 1 << 32), (0, 1 << 31)):
        h[field, n] = C.c_void_p()
        L.check(lib.zk_table_wrap(field, C.c_void_p(0x1000), n, C.byref(h[field, n])))
    g5 = np.full(20, 7, np.uint64)
    outs = (C.c_void_p * 10)()
    one = zk.from_ints(0, [1])[0]
    unreduced = np.full(4, 0xFFFFFFFFFFFFFFFF, np.uint64)
    arr = lambda tabs: (C.c_void_p * len(tabs))(*[None if t is None else t.value for t in tabs])

    def rnd(tabs, r=None, o=outs, g=g5, el=None):
        el = [one] * 3 if el is None else el
        return lib.zk_lookup_round(arr(tabs), *[p64(e) for e in el], p64(r), o, p64(g))

    t4, t8 = h[0, 4], h[0, 8]
    assert lib.zk_lookup_round(None, p64(one), p64(one), p64(one), None, outs, p64(g5)) == L.ZK_E_ARG
    for i in range(10):
        tabs = [t4] * 10
        tabs[i] = None
        assert rnd(tabs) == L.ZK_E_ARG
        tabs[i] = h[3, 4]
        assert rnd(tabs) == L.ZK_E_ARG
        if i:
            tabs[i] = t8
            assert rnd(tabs) == L.ZK_E_LEN_MISMATCH
    assert rnd([t4] * 10, g=None) == L.ZK_E_ARG and rnd([t4] * 10, r=one, o=None) == L.ZK_E_ARG and rnd([h[1, 8]] * 10) == L.ZK_E_ARG
    assert rnd([h[0, 6]] * 10) == L.ZK_E_NOT_POW2
    assert rnd([h[0, 1]] * 10) == L.ZK_E_ARG and rnd([h[0, 2]] * 10, r=one) == L.ZK_E_ARG and rnd([t4] * 10, r=unreduced) == L.ZK_E_ARG
    for i in range(3):
        el = [one] * 3
        el[i] = None
        assert rnd([t4] * 10, el=el) == L.ZK_E_ARG
        el[i] = unreduced
        assert rnd([t4] * 10, el=el) == L.ZK_E_ARG
    # the helper table
    H = C.c_void_p()
    fr = lambda tabs, beta=one, gamma=one, out=C.byref(H): lib.zk_lookup_fractions(None if tabs is None else arr(tabs), p64(beta), p64(gamma), out)
    assert fr(None) == L.ZK_E_ARG and fr([t4] * 8, beta=None) == L.ZK_E_ARG and fr([t4] * 8, gamma=None) == L.ZK_E_ARG and fr([t4] * 8, out=None) == L.ZK_E_ARG
    for i in range(8):
        tabs = [t4] * 8
        tabs[i] = None
        assert fr(tabs) == L.ZK_E_ARG
        tabs[i] = h[3, 4]
        assert fr(tabs) == L.ZK_E_ARG
        if i:
            tabs[i] = t8
            assert fr(tabs) == L.ZK_E_LEN_MISMATCH
    assert fr([h[1, 8]] * 8) == L.ZK_E_ARG and fr([h[0, 6]] * 8) == L.ZK_E_NOT_POW2 and fr([h[0, 1]] * 8) == L.ZK_E_ARG
    assert fr([t4] * 8, beta=unreduced) == L.ZK_E_ARG and fr([t4] * 8, gamma=unreduced) == L.ZK_E_ARG
    # the multiplicities
    Mt, misses = C.c_void_p(), C.c_uint64(7)
    mu = lambda tabs, out=C.byref(Mt), lost=C.byref(misses): lib.zk_lookup_multiplicities(None if tabs is None else arr(tabs), out, lost)
    assert mu(None) == L.ZK_E_ARG and mu([t4] * 7, out=None) == L.ZK_E_ARG and mu([t4] * 7, lost=None) == L.ZK_E_ARG
    for i in range(7):
        tabs = [t4] * 7
        tabs[i] = None
        assert mu(tabs) == L.ZK_E_ARG
        tabs[i] = h[3, 4]
        assert mu(tabs) == L.ZK_E_ARG
        if i:
            tabs[i] = t8
            assert mu(tabs) == L.ZK_E_LEN_MISMATCH
    assert mu([h[1, 8]] * 7) == L.ZK_E_ARG and mu([h[0, 6]] * 7) == L.ZK_E_NOT_POW2 and mu([h[0, 1]] * 7) == L.ZK_E_ARG
    assert mu([h[0, 1 << 32]] * 7) == L.ZK_E_ARG              # the counts are 32 bits: d > 31 is refused
    # the hash table's slots (a test hook)
    slots = np.full(16, 7, np.uint32)
    hs = lambda tabs, out=slots: lib.zk_lookup_hash_slots(None if tabs is None else arr(tabs), None if out is None else out.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert hs(None) == L.ZK_E_ARG and hs([t4] * 3, out=None) == L.ZK_E_ARG
    for i in range(3):
        tabs = [t4] * 3
        tabs[i] = None
        assert hs(tabs) == L.ZK_E_ARG
        tabs[i] = h[3, 4]
        assert hs(tabs) == L.ZK_E_ARG
        if i:
            tabs[i] = t8
            assert hs(tabs) == L.ZK_E_LEN_MISMATCH
    assert hs([h[1, 8]] * 3) == L.ZK_E_ARG and hs([h[0, 6]] * 3) == L.ZK_E_NOT_POW2 and hs([h[0, 1]] * 3) == L.ZK_E_ARG
    assert hs([h[0, 1 << 32]] * 3) == L.ZK_E_ARG              # the slots hold 32-bit indices: n > 2^31 is refused
    import torch
    if not torch.cuda.is_available():
        assert rnd([h[0, 2]] * 10) == L.ZK_E_NO_DEVICE and rnd([t4] * 10, r=one) == L.ZK_E_NO_DEVICE and fr([t4] * 8) == L.ZK_E_NO_DEVICE
        assert mu([t4] * 7) == L.ZK_E_NO_DEVICE and mu([h[0, 1 << 31]] * 7) == L.ZK_E_NO_DEVICE
        assert hs([t4] * 3) == L.ZK_E_NO_DEVICE and hs([h[0, 1 << 31]] * 3) == L.ZK_E_NO_DEVICE
    assert (g5 == 7).all() and not any(outs) and not H and not Mt and misses.value == 7 and (slots == 7).all()
    w = lambda n: np.full(n, 7, np.uint64)
    bufs = [w(64) for _ in range(9)]
    r8, hr = np.full(64 * 32, 7, np.uint8), np.full(64, 7, np.uint8)
    prove = lambda cms: lib.zk_lookup_prove(cms, 0, 4, 1, 0, None, p8(hr), p64(bufs[0]), p64(bufs[1]), p64(bufs[2]), p64(bufs[3]), p64(bufs[4]), p64(bufs[5]),
                                            p8(r8), p64(bufs[6]), None, None, p64(bufs[7]), p8(r8), None)
    assert prove(None) == L.ZK_E_ARG and prove((C.c_void_p * 7)()) == L.ZK_E_ARG
    assert all((x == 7).all() for x in bufs) and (r8 == 7).all() and (hr == 7).all()
    assert lib.zk_lookup_last_stats(None) == L.ZK_E_ARG
    for t in h.values():
        lib.zk_table_free(t)


def test_the_selftest_fixture_is_the_models_proof():
    import importlib.util
    path = os.path.join(G.ROOT, "tests", "golden", "make_lookup_fixture.py")
    spec = importlib.util.spec_from_file_location("make_lookup_fixture", path)
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    with open(mk.OUT, "rb") as fh:
        stored = fh.read()
    assert stored == mk.fixture_bytes(zk) and len(stored) < 16 << 10
    pr = mk.model_proof(zk)
    assert pr["misses"] == 0
    assert LM.verify(pr, tr=LM.pow_transcript(mk.D, mk.F, mk.G_BITS, pr["nonce"]), hasher=mk.hasher(zk)) == (True, None)
    assert lib_verify(pr, g=mk.G_BITS, nonce=pr["nonce"]) == (0, 1)
