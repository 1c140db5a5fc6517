"""CPU: the host side of the Plonk proof with lookup rows over FRI commitments (include/zkmle.h "Plonk with lookups: gate, wiring, public inputs
and lookup rows in one sumcheck").  Everything compares byte for byte against the big-integer model of tests/_plonk_lookup_model.py:

  proofs      zk_plonk_lookup_verify and zk.plonk_lookup.verify accept the model's proofs at d = 1 .. 4 on both fields under the three schedules
              (log_arity 1; 2; 2 with grouped leaves), with l among 0, 1, 3 and 2^d public values and with no, some and all rows lookup rows
  rejected    one flipped bit in every array of the proof (each of the five helper roots among them); one public value changed; l off by one;
              two roots swapped; d + 1 and d - 1; a false gate row; a false wiring; a row with qK = 1 that differs from every table row in the
              third column only (accepted with qK = 0); the lookup's cheating prover (a miss credited to row 0); 7n's cheating prover
              (H_j = 0); a nonce off by one; a public value >= p
  statuses    a status leaves a caller's transcript as it was
  transcript  the verifier's transcript ends in the model prover's state
  sizes       zk_plonk_lookup_sizes equals the model's counts; for d = 4 .. 24 and every schedule the fused proof is smaller than the pair's two
              proofs by one single-table opening, two step-0 shares and 5 d round elements
  header      the protocol's text and the exports
  fixture     tests/golden/plonk_lookup_proof.bin, what tools/plonk_lookup_selftest.hip reads, is the model's proof and verifies

Commitments cannot exist without a device: the kernel and the prover run in tests/test_gpu_plonk_lookup.py."""
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
import _ntt_model as NM
import _plonk_lookup_model as KL
from oracle import pymodel as M

zk = G.import_package()
P64, P8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
p64 = lambda a: a.ctypes.data_as(P64) if a is not None and a.size else None
p8 = lambda a: a.ctypes.data_as(P8) if a is not None else None
NEW_NAMES = ("zk_plonk_lookup_round", "zk_plonk_lookup_sizes", "zk_plonk_lookup_prove", "zk_plonk_lookup_verify", "zk_plonk_lookup_last_stats")
SCHEDULES = [(1, False), (2, False), (2, True)]              # (log_arity, grouped)
# (field, d, b, f, coset, l, looked): d = 1 .. 4 on both fields; l among 0, 1, 3 and 2^d; no, some and all rows lookup rows
CASES = [(0, 1, 1, 0, False, 0, "all"), (3, 1, 2, 0, True, 1, "some"), (3, 1, 1, 0, False, 2, "none"), (0, 2, 2, 0, True, 3, "some"), (3, 2, 1, 1, False, 4, "all"),
         (3, 2, 1, 0, False, 1, "none"), (0, 3, 1, 1, False, 8, "some"), (3, 3, 2, 0, True, 3, "all"), (3, 3, 1, 2, True, 0, "none"), (0, 4, 2, 0, True, 3, "some"),
         (3, 4, 1, 2, False, 16, "all"), (0, 4, 1, 3, False, 1, "none")]
Q = 4
case_id = lambda c: "-".join(str(v) if isinstance(v, str) else str(int(v)) for v in c)
sched_id = lambda s: "a%d%s" % (s[0], "g" if s[1] else "")
runs = lambda case, sched: sched[0] == 1 or case[1] - case[3] >= 2
GRID = [pytest.param(c, s, id=case_id(c) + "-" + sched_id(s)) for c in CASES for s in SCHEDULES if runs(c, s)]
ARRAYS = ("own_roots", "h_roots", "polys", "ys", "open_polys", "roots", "final", "values", "paths")

hasher = functools.partial(FC.hasher, zk, True)
padded = functools.partial(FC.padded, room=16384)
coset_of = functools.partial(FC.coset_of, mul=71)


@functools.lru_cache(maxsize=None)
def statement(field, d, b, with_coset, grouped, l, looked, false_gate=False, false_wiring=False, miss=None, unselect=False):
    """-> (the fifteen model commitments, the public values)"""
    p = NM.MODULUS[field]
    tabs, pub = KL.circuit(field, d, 6100 + 13 * d + field + l, l, looked, false_gate=false_gate, false_wiring=false_wiring, miss=miss)
    if unselect:                                              # the missing row (and a row wired to hold its triple) with qK = 0: a true statement
        t = tuple(tabs[j][miss] for j in range(3))
        tabs[11] = [0 if tuple(tabs[j][x] for j in range(3)) == t else v for x, v in enumerate(tabs[11])]
    assert KL.satisfied(tabs, pub, p) == (not false_gate, not false_wiring, miss is None or unselect)
    coset = coset_of(field, d, b, with_coset)
    return tuple((GM if grouped else PM).commit(field, t, b, coset, hasher()) for t in tabs), tuple(pub)


@functools.lru_cache(maxsize=None)
def proof(case, sched, cheat=None, **false):
    field, d, b, f, with_coset, l, looked = case
    cms, pub = statement(field, d, b, with_coset, sched[1], l, looked, **false)
    return KL.prove(list(cms), list(pub), f, Q, sched[0], hasher=hasher(), cheat=cheat)


def lib_verify(pr, fl=None, tr=None, g=0, nonce=0, pub=None, npublic=None, **over):
    """zk_plonk_lookup_verify on the model's proof `pr` (flat arrays `fl`) -> (status, ok); pub: the verifier's own public values ((l, 4))"""
    op = pr["opening"]
    fl = KL.flat(zk, pr) if fl is None else fl
    s = {n: op[n] for n in ("d", "b", "f", "Q", "a")}
    s["lg"] = 2 if op["grouped"] else 0
    s.update({n: v for n, v in over.items() if n in s})
    coset = over.get("coset", op["coset"])
    cm = None if coset is None else zk.from_ints(op["field"], [coset])[0]
    pub = fl["pub"] if pub is None else pub
    npublic = pub.shape[0] if npublic is None else npublic
    ok = C.c_int(-1)
    rc = zk.lib().zk_plonk_lookup_verify(over.get("field", op["field"]), p8(fl["own_roots"]), p64(pub), npublic, s["d"], s["b"], s["f"], s["Q"], s["a"], s["lg"], p64(cm),
                                         None if tr is None else tr._h, p8(fl["h_roots"]), p64(fl["polys"]), p64(fl["ys"]), p64(fl["open_polys"]), p8(fl["roots"]),
                                         p64(fl["final"]), p64(fl["values"]), p8(fl["paths"]), g, nonce, C.byref(ok))
    return rc, ok.value


def wrapper_proof(pr, fl, g=0, nonce=0):
    """zk.plonk_lookup.PlonkLookupProof holding the model's arrays"""
    op = pr["opening"]
    cs = zk.from_ints(op["field"], [op["coset"]])[0]
    o = zk.plonk_lookup.PlonkLookupProof(op["field"], op["d"], op["b"], op["f"], op["Q"], coset=cs, log_arity=op["a"], grouped=op["grouped"], grinding_bits=g)
    assert o.round_polys.shape == fl["polys"].shape == (op["d"], 5, 4) and o.drawn.shape == fl["drawn"].shape and o.challenges.shape == fl["challenges"].shape
    assert o.h_roots.shape == fl["h_roots"].shape == (5, 32)
    q = o.opening
    assert isinstance(q, zk.fri.FriMlWideOpening)
    assert q.roots.shape == fl["roots"].shape and q.query_values.shape == fl["values"].shape and q.query_paths.shape == fl["paths"].shape
    assert q.ys.shape == (20, 1, 4) and q.round_polys.shape == fl["open_polys"].shape
    o.round_polys, o.drawn, o.challenges, o.h_roots = fl["polys"], fl["drawn"], fl["challenges"], fl["h_roots"]
    q.ys, q.round_polys, q.roots, q.final_table, q.query_values, q.query_paths = fl["ys"].reshape(20, 1, 4), fl["open_polys"], fl["roots"], fl["final"], fl["values"], fl["paths"]
    q.pow_nonce = nonce
    return o


def test_new_exports_and_the_header():
    lib = zk.lib()
    header = open(G.ROOT + "/include/zkmle.h").read()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in header, name
    assert "Plonk with lookups: gate, wiring, public inputs and lookup rows in one sumcheck" in header and "zk_plonk_lookup_stats" in header
    for text in ('"ZCPL"', "alpha^3 PIeval(tau)", "k = 20 in the order of the fifteen, then M, H0,", "plonk_lookup_round_kernel", "ONE pair", "as a count and not a proof",
                 "zk_fri_ml_open_batch_wide_pow"):
        assert text in header, text
    for name in ("prove", "verify", "round", "sizes", "last_stats", "PlonkLookupProof", "table_columns", "sigma_from_cycles"):
        assert hasattr(zk.plonk_lookup, name), name
    assert zk.PlonkLookupProof is zk.plonk_lookup.PlonkLookupProof
    assert zk.plonk_lookup.table_columns is zk.lookup.table_columns and zk.plonk_lookup.sigma_from_cycles is zk.wiring.sigma_from_cycles


def test_the_circuit_builder():
    for field in (0, 3):
        p = NM.MODULUS[field]
        for l in (0, 1, 3, 16):
            for looked in ("none", "some", "all"):
                tabs, pub = KL.circuit(field, 4, 43 + field, l, looked)
                assert len(tabs) == 15 and len(pub) == l and KL.satisfied(tabs, pub, p) == (True, True, True)
                assert sum(tabs[11]) == {"none": 0, "all": 16}.get(looked, sum(tabs[11])) and set(tabs[11]) <= {0, 1}
                assert all(tabs[4][x] == 1 and tabs[0][x] == pub[x] for x in range(l))
            assert KL.satisfied(*KL.circuit(field, 4, 43 + field, l, false_gate=True), p) == (False, True, True)
            assert KL.satisfied(*KL.circuit(field, 4, 43 + field, l, false_wiring=True), p) == (True, False, True)
            for looked in ("none", "some", "all"):
                tabs, pub = KL.circuit(field, 4, 43 + field, l, looked, miss=5)
                assert KL.satisfied(tabs, pub, p) == (True, True, False)
                a, b, c = (tabs[j][5] for j in range(3))       # the table holds the row with one more in the third column, and not the row
                rows = set(zip(tabs[12], tabs[13], tabs[14]))
                assert (a, b, (c + 1) % p) in rows and (a, b, c) not in rows


@pytest.mark.parametrize("case,sched", GRID)
def test_model_proofs_pass_the_model_verifier_and_the_library_verifier(case, sched):
    field, d, b, f, with_coset, l, looked = case
    a, grouped = sched
    p = NM.MODULUS[field]
    pr = proof(case, sched)
    assert KL.verify(pr, hasher=hasher()) == (True, None)
    assert pr["own_first_sum"] == 0 and pr["misses"] == 0     # the model's own polynomial, PI inside, sums to 0 on a satisfied circuit
    alpha, tau = pr["drawn"][2], pr["drawn"][4:]
    c = alpha ** 3 * KL.public_eval(pr["pub"], tau, p) % p
    assert all((g[0] + g[1]) % p == (c if k == 0 else KL.interpolate5(pr["polys"][k - 1], pr["challenges"][k - 1], p)) for k, g in enumerate(pr["polys"]))
    assert (c != 0) == (l > 0) and pr["opening"]["points"] == [pr["challenges"][::-1]] and pr["opening"]["k"] == 20
    fl = KL.flat(zk, pr)
    assert fl["pub"].shape == (l, 4) and fl["h_roots"].shape == (5, 32) and lib_verify(pr, fl) == (0, 1)
    if not with_coset:
        assert lib_verify(pr, fl, coset=None) == (0, 1)
    got = (fl["polys"].size // 4, fl["h_roots"].shape[0], fl["roots"].shape[0], fl["final"].shape[0], fl["values"].size // 4, fl["paths"].size, fl["open_polys"].size // 4)
    assert KL.sizes(d, b, f, Q, a, grouped) == got == zk.plonk_lookup.sizes(d, b, f, Q, a, grouped)
    o = wrapper_proof(pr, fl)
    assert zk.plonk_lookup.verify(pr["roots"], fl["pub"], o)
    assert not zk.plonk_lookup.verify(pr["roots"][::-1], fl["pub"], o)
    assert zk.plonk_lookup.verify(pr["roots"], None, o) is (l == 0)
    assert np.array_equal(o.point[0], fl["points"][0]) and np.array_equal(o.ys, fl["ys"])


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_the_public_values_are_part_of_the_statement(sched):
    for case in (CASES[9], CASES[10], CASES[3] if sched[0] == 1 else CASES[7]):
        field, d, l = case[0], case[1], case[5]
        p, rng = NM.MODULUS[field], random.Random(case[1] + l)
        pr = proof(case, sched)
        fl = KL.flat(zk, pr)
        n = 1 << d
        for x in sorted({0, l - 1, rng.randrange(l)}):        # one public value changed
            wrong = list(pr["pub"])
            wrong[x] = (wrong[x] + 1) % p
            assert lib_verify(pr, fl, pub=KL.mont(zk, field, wrong)) == (0, 0), (case, x)
            assert KL.verify(pr, pub=wrong, hasher=hasher())[0] is False
        room = np.concatenate([fl["pub"], np.zeros((1, 4), np.uint64)])
        assert lib_verify(pr, fl, pub=room, npublic=l) == (0, 1)
        assert lib_verify(pr, fl, pub=room, npublic=l - 1) == (0, 0)          # l off by one: the tag and the absorbed values change
        assert KL.verify(pr, pub=pr["pub"][:-1], hasher=hasher())[0] is False
        if l < n:
            assert lib_verify(pr, fl, pub=room, npublic=l + 1) == (0, 0)      # one more value, a zero: the same PI table, another statement
            assert KL.verify(pr, pub=pr["pub"] + [0], hasher=hasher())[0] is False
        big = fl["pub"].copy()                                                # a public value >= p: not a status
        big[l - 1] = np.uint64(0xFFFFFFFFFFFFFFFF)
        assert lib_verify(pr, fl, pub=big) == (0, 0)
        big[l - 1] = np.frombuffer(p.to_bytes(32, "little"), np.uint64)
        assert lib_verify(pr, fl, pub=big) == (0, 0)
        assert KL.verify(pr, pub=pr["pub"][:-1] + [p + pr["pub"][-1]], hasher=hasher())[0] is False


def test_statuses_come_before_the_transcript_is_touched():
    from zkmle_amd import _lib as L
    pr = proof(CASES[7], SCHEDULES[0])
    fl = KL.flat(zk, pr)
    t = zk.Transcript()
    t.append(b"the caller's own")
    before = t.export_state().copy()
    for name in ARRAYS:
        class Without(dict):
            def __getitem__(self, key, name=name):
                return None if key == name else dict.__getitem__(self, key)
        assert lib_verify(pr, Without(fl), t, pub=fl["pub"])[0] == L.ZK_E_ARG, name
    op = pr["opening"]
    lib = zk.lib()
    assert lib.zk_plonk_lookup_verify(op["field"], p8(fl["own_roots"]), p64(fl["pub"]), 3, 3, 2, 0, Q, 1, 0, None, t._h, p8(fl["h_roots"]), p64(fl["polys"]), p64(fl["ys"]),
                                      p64(fl["open_polys"]), p8(fl["roots"]), p64(fl["final"]), p64(fl["values"]), p8(fl["paths"]), 0, 0, None) == L.ZK_E_ARG
    big = padded(fl)
    for over, want in ((dict(field=7), L.ZK_E_ARG), (dict(field=-1), L.ZK_E_ARG), (dict(field=1, coset=None), L.ZK_E_RANGE), (dict(field=2, coset=None), L.ZK_E_RANGE),
                       (dict(coset=0), L.ZK_E_ARG), (dict(d=NM.two_adicity(3) - 1, b=2), L.ZK_E_RANGE), (dict(d=31, b=2), L.ZK_E_RANGE), (dict(d=32, b=1), L.ZK_E_RANGE),
                       (dict(d=0), L.ZK_E_ARG), (dict(f=3), L.ZK_E_ARG), (dict(b=0), L.ZK_E_ARG), (dict(Q=0), L.ZK_E_ARG), (dict(a=3), L.ZK_E_ARG),
                       (dict(lg=2), L.ZK_E_ARG), (dict(lg=1), L.ZK_E_ARG), (dict(a=2, f=2), L.ZK_E_ARG)):
        assert lib_verify(pr, big, t, pub=fl["pub"], **over) == (want, -1), over
    assert lib_verify(pr, big, t, pub=fl["pub"], g=33)[0] == L.ZK_E_ARG
    assert lib_verify(pr, big, t, pub=np.zeros((9, 4), np.uint64)) == (L.ZK_E_ARG, -1)
    assert lib_verify(pr, big, t, pub=np.zeros((0, 4), np.uint64), npublic=1) == (L.ZK_E_ARG, -1)
    assert np.array_equal(t.export_state(), before)
    assert lib_verify(pr, fl, t) == (0, 0) and not np.array_equal(t.export_state(), before)   # bound to a fresh transcript; ZK_OK moves it


SPOTS = ("polys", "ys", "own_roots", "h_roots", "roots", "open_polys", "final", "values", "paths")


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
@pytest.mark.parametrize("name", SPOTS)
def test_one_flipped_bit_is_rejected(name, sched):
    for case in (CASES[9], CASES[8] if sched[0] == 1 else CASES[7]):
        pr = proof(case, sched)
        base = KL.flat(zk, pr)
        rng = random.Random(43 * len(name) + case[1] + sched[0])
        flat_size = base[name].size
        spots = {0, flat_size - 1} | {rng.randrange(flat_size) for _ in range(6)}
        if name == "h_roots":                                 # each of the five helper roots
            spots |= {32 * j + rng.randrange(32) for j in range(5)}
        for at in sorted(spots):
            fl = {n: v.copy() for n, v in base.items()}
            view = fl[name].reshape(-1)
            view[at] ^= view.dtype.type(1 << rng.randrange(8 if view.dtype == np.uint8 else 64))
            assert lib_verify(pr, fl) == (0, 0), (case, name, at)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_swapped_roots_and_another_d_are_rejected(sched):
    case = CASES[9]                                           # d = 4, f = 0, l = 3
    pr = proof(case, sched)
    base = KL.flat(zk, pr)
    for i, j in ((0, 1), (3, 4), (8, 9), (0, 8), (2, 7), (11, 3), (12, 13), (0, 12), (14, 10)):   # .. qK with qM; T0 with T1; A with T0; T2 with SC
        sw = {n: v.copy() for n, v in base.items()}
        sw["own_roots"][[i, j]] = sw["own_roots"][[j, i]]
        assert lib_verify(pr, sw) == (0, 0), (i, j)
        sw["roots"][[i, j]] = sw["roots"][[j, i]]             # ... and the proof's copy with them
        assert lib_verify(pr, sw) == (0, 0), (i, j)
        sw["ys"][[i, j]] = sw["ys"][[j, i]]                   # ... and the claims: the statement's transcript has the roots in another order
        assert lib_verify(pr, sw) == (0, 0), (i, j)
        roots = list(pr["roots"])
        roots[i], roots[j] = roots[j], roots[i]
        assert KL.verify(pr, roots=roots, hasher=hasher())[0] is False
    for i, j in ((0, 1), (1, 2), (3, 4), (0, 4)):             # two helper roots: M with H0; H0 with H1; H2 with HL; M with HL
        sw = {n: v.copy() for n, v in base.items()}
        sw["h_roots"][[i, j]] = sw["h_roots"][[j, i]]
        assert lib_verify(pr, sw) == (0, 0)
    big = padded(base)
    assert lib_verify(pr, big, pub=base["pub"]) == (0, 1)
    assert lib_verify(pr, big, pub=base["pub"], d=5) == (0, 0) and lib_verify(pr, big, pub=base["pub"], d=3) == (0, 0)
    assert lib_verify(pr, big, pub=base["pub"], f=1) == (0, 0) and lib_verify(pr, big, pub=base["pub"], Q=Q + 1) == (0, 0)
    assert lib_verify(pr, big, pub=base["pub"], b=1) == (0, 0)


@pytest.mark.parametrize("field", (0, 3))
@pytest.mark.parametrize("d", (1, 2, 3, 4))
def test_false_statements_and_the_cheating_provers_are_rejected(field, d):
    l = (1, 0, 3, 16)[d - 1]
    case = (field, d, 1, 0, d % 2 == 0, l, ("some", "all", "none", "some")[d - 1])
    x = (1 << d) - 1
    for sched in SCHEDULES:
        if not runs(case, sched):
            continue
        for false, cheat in ((dict(false_gate=True), "wiring"), (dict(false_wiring=True), "wiring"), (dict(miss=x), "lookup")):
            pr = proof(case, sched, **false)
            assert KL.verify(pr, hasher=hasher()) == (False, 0), false
            assert pr["own_first_sum"] != 0 and lib_verify(pr) == (0, 0), false
            assert (pr["misses"] >= 1) if "miss" in false else pr["misses"] == 0   # rows wired to row x hold its triple and miss with it
            ch = proof(case, sched, cheat, **false)
            ok, failed = KL.verify(ch, hasher=hasher())
            assert not ok and 1 <= failed <= d, false         # a later round's sum, or the last claim: never the opening, which is honest
            assert lib_verify(ch) == (0, 0), false
        # the row that differs in the third column only, with qK = 0: accepted
        pr = proof(case, sched, miss=x, unselect=True)
        assert pr["misses"] == 0 and KL.verify(pr, hasher=hasher()) == (True, None) and lib_verify(pr) == (0, 1)
        # the cheating provers on a true statement: the lookup's changes nothing (no miss); H = 0 is not what the helper step says unless S = id
        ch = proof(case, sched, "lookup")
        assert lib_verify(ch) == (0, 1) and ch["polys"] == proof(case, sched)["polys"]
        ch = proof(case, sched, "wiring")
        assert lib_verify(ch) == (0, int(KL.verify(ch, hasher=hasher())[0]))


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_the_proof_of_work_nonce(sched):
    field, d, b, f, with_coset, l, looked = case = CASES[10]  # d = 4, f = 2, l = 16
    G_BITS = 4
    cms, pub = statement(field, d, b, with_coset, sched[1], l, looked)
    mt = KL.pow_transcript(d, f, G_BITS)
    pr = KL.prove(list(cms), list(pub), f, Q, sched[0], mt, hasher())
    w = pr["nonce"]
    assert mt.pow_ok and mt.nonce == w
    assert KL.verify(pr, tr=KL.pow_transcript(d, f, G_BITS, w), hasher=hasher()) == (True, None)
    fl = KL.flat(zk, pr)
    assert lib_verify(pr, fl, g=G_BITS, nonce=w) == (0, 1)
    assert lib_verify(pr, fl, g=G_BITS, nonce=w + 1) == (0, 0) and lib_verify(pr, fl, g=G_BITS, nonce=(w - 1) % (1 << 64)) == (0, 0)
    assert lib_verify(pr, fl, g=G_BITS + 1, nonce=w) == (0, 0) and lib_verify(pr, fl) == (0, 0)
    assert KL.verify(pr, tr=KL.pow_transcript(d, f, G_BITS, w + 1), hasher=hasher())[0] is False
    plain = proof(case, sched)
    assert lib_verify(plain, g=G_BITS, nonce=w) == (0, 0)     # indices drawn without the step
    o = wrapper_proof(pr, fl, G_BITS, w)
    assert zk.plonk_lookup.verify(pr["roots"], fl["pub"], o)
    o.opening.pow_nonce = w + 1
    assert not zk.plonk_lookup.verify(pr["roots"], fl["pub"], o)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_a_callers_transcript(sched):
    field, d, b, f, with_coset, l, looked = CASES[7]
    prior = b"what the caller had absorbed before"
    cms, pub = statement(field, d, b, with_coset, sched[1], l, looked)
    mt = M.Transcript()
    mt.append(prior)
    pr = KL.prove(list(cms), list(pub), f, Q, sched[0], mt, hasher())
    vt = M.Transcript()
    vt.append(prior)
    assert KL.verify(pr, tr=vt, hasher=hasher()) == (True, None) and vt.buf == mt.buf
    t, want = zk.Transcript(), zk.Transcript()
    t.append(prior)
    assert lib_verify(pr, tr=t) == (0, 1)
    want.append(bytes(mt.buf))
    assert np.array_equal(t.export_state(), want.export_state())   # the verifier's transcript ends in the model prover's state
    assert lib_verify(pr) == (0, 0)                           # the proof is bound to the prior content
    t2 = zk.Transcript()
    t2.append(prior + b"!")
    assert lib_verify(pr, tr=t2) == (0, 0)


def test_sizes_and_the_count_against_the_pair():
    from zkmle_amd import _lib as L
    lib = zk.lib()

    def sizes(d, b, f, q, a, lg):
        out = [C.c_size_t(0) for _ in range(7)]
        rc = lib.zk_plonk_lookup_sizes(d, b, f, q, a, lg, *[C.byref(o) for o in out])
        return rc, tuple(int(o.value) for o in out)

    for d in (1, 2, 3, 4, 6, 10, 24):
        for b in (1, 2):
            for f in range(0, d):
                for q in (1, 8, 64):
                    for a, grouped in SCHEDULES:
                        if a == 2 and d - f < 2:
                            assert sizes(d, b, f, q, a, 2 * grouped)[0] == L.ZK_E_ARG
                            continue
                        want = (5 * d, 5) + zk.fri.ml_sizes_wide(d, b, f, q, log_arity=a, grouped=grouped, k=20)
                        assert sizes(d, b, f, q, a, 2 * grouped) == (0, want) and KL.sizes(d, b, f, q, a, grouped) == want
                        assert zk.plonk_lookup.sizes(d, b, f, q, a, grouped) == want
    for d, b, f, q, a, lg in ((0, 1, 0, 4, 1, 0), (3, 0, 0, 4, 1, 0), (3, 1, 3, 4, 1, 0), (3, 1, 0, 0, 1, 0), (3, 1, 0, 4, 0, 0), (3, 1, 0, 4, 3, 0), (3, 1, 0, 4, 1, 2)):
        assert sizes(d, b, f, q, a, lg)[0] == L.ZK_E_ARG
    assert sizes(40, 1, 0, 8, 1, 0)[0] == L.ZK_E_RANGE
    assert lib.zk_plonk_lookup_sizes(4, 1, 0, 8, 2, 2, None, None, None, None, None, None, None) == 0
    with pytest.raises(ValueError):
        zk.plonk_lookup.sizes(4, 1, 0, 8, log_arity=1, grouped=True)

    # the proof's bytes: 32 per element and per root, the paths as they are; the nonce's 8 bytes when there is one are the same on both sides
    def total(s):
        nround, nh, nroots, nfinal, nvalues, pbytes, nopen = s
        return 32 * (nround + nh + nroots + nfinal + nvalues + nopen) + pbytes

    b, q = 2, 64
    for d in range(4, 25):
        f = min(6, d - 2)
        for a, grouped in SCHEDULES:
            fused, plonk, lookup = zk.plonk_lookup.sizes(d, b, f, q, a, grouped), zk.plonk.sizes(d, b, f, q, a, grouped), zk.lookup.sizes(d, b, f, q, a, grouped)
            one = zk.fri.ml_sizes(d, b, f, q, a, grouped)     # a single-table opening: nroots, nfinal, nvalues, path_bytes, nround
            two = zk.fri.ml_sizes(d, b, f, q, a, grouped, k=2)
            share = 32 * (two[2] - one[2]) + (two[3] - one[3])   # step 0's share of one more commitment: its values and its path bytes
            own_root = 32                                       # ... and its root
            # claims: 20 against 14 + 9
            t_fused, t_pair = total(fused) + 32 * 20, total(plonk) + total(lookup) + 32 * 23
            single = 32 * (one[0] + one[1] + one[2] + one[4]) + one[3]
            # 23 commitments' step-0 shares and roots become 20, one opening's fixed part goes, and 5 d round elements; 3 claims fewer
            assert t_pair - t_fused == single + 2 * (share + own_root) + 32 * 5 * d + 32 * 3, (d, a, grouped)
            assert t_fused < t_pair


def test_prover_and_hook_statuses_without_a_device():
    from zkmle_amd import _lib as L
    lib = zk.lib()
    h = {}
    for field, n in ((0, 1), (0, 2), (0, 4), (0, 8), (0, 6), (1, 8), (3, 4)):
        h[field, n] = C.c_void_p()
        L.check(lib.zk_table_wrap(field, C.c_void_p(0x1000), n, C.byref(h[field, n])))
    g5 = np.full(20, 7, np.uint64)
    outs = (C.c_void_p * 21)()
    one = zk.from_ints(0, [1])[0]
    unreduced = np.full(4, 0xFFFFFFFFFFFFFFFF, np.uint64)

    def rnd(tabs, r=None, o=outs, g=g5, el=None, step=0):
        arr = (C.c_void_p * 21)(*[None if t is None else t.value for t in tabs])
        el = [one] * 5 if el is None else el
        return lib.zk_plonk_lookup_round(arr, *[p64(e) for e in el], step, p64(r), o, p64(g))

    t4, t8 = h[0, 4], h[0, 8]
    assert lib.zk_plonk_lookup_round(None, p64(one), p64(one), p64(one), p64(one), p64(one), 0, None, outs, p64(g5)) == L.ZK_E_ARG
    for i in range(21):
        tabs = [t4] * 21
        tabs[i] = None
        assert rnd(tabs) == L.ZK_E_ARG
        tabs[i] = h[3, 4]
        assert rnd(tabs) == L.ZK_E_ARG
        if i:
            tabs[i] = t8
            assert rnd(tabs) == L.ZK_E_LEN_MISMATCH
    assert rnd([t4] * 21, g=None) == L.ZK_E_ARG and rnd([t4] * 21, r=one, o=None) == L.ZK_E_ARG and rnd([h[1, 8]] * 21) == L.ZK_E_ARG
    assert rnd([h[0, 6]] * 21) == L.ZK_E_NOT_POW2
    assert rnd([h[0, 1]] * 21) == L.ZK_E_ARG and rnd([h[0, 2]] * 21, r=one) == L.ZK_E_ARG and rnd([t4] * 21, r=unreduced) == L.ZK_E_ARG
    for i in range(5):
        el = [one] * 5
        el[i] = None
        assert rnd([t4] * 21, el=el) == L.ZK_E_ARG
        el[i] = unreduced
        assert rnd([t4] * 21, el=el) == L.ZK_E_ARG
    assert rnd([t4] * 21, step=31) == L.ZK_E_ARG and rnd([t4] * 21, step=33) == L.ZK_E_ARG
    import torch
    if not torch.cuda.is_available():
        assert rnd([h[0, 2]] * 21) == L.ZK_E_NO_DEVICE and rnd([t4] * 21, r=one) == L.ZK_E_NO_DEVICE
    assert (g5 == 7).all() and not any(outs)
    w = lambda n: np.full(n, 7, np.uint64)
    bufs = [w(128) for _ in range(9)]
    r8, hr = np.full(64 * 32, 7, np.uint8), np.full(160, 7, np.uint8)
    prove = lambda cms: lib.zk_plonk_lookup_prove(cms, None, 0, 0, 4, 1, 0, None, p8(hr), p64(bufs[0]), p64(bufs[1]), p64(bufs[2]), p64(bufs[3]), p64(bufs[4]),
                                                  p64(bufs[5]), p8(r8), p64(bufs[6]), None, None, p64(bufs[7]), p8(r8), None)
    assert prove(None) == L.ZK_E_ARG and prove((C.c_void_p * 15)()) == L.ZK_E_ARG
    assert all((x == 7).all() for x in bufs) and (r8 == 7).all() and (hr == 7).all()
    assert lib.zk_plonk_lookup_last_stats(None) == L.ZK_E_ARG
    for t in h.values():
        lib.zk_table_free(t)


def test_the_selftest_fixture_is_the_models_proof():
    import importlib.util
    path = os.path.join(G.ROOT, "tests", "golden", "make_plonk_lookup_fixture.py")
    spec = importlib.util.spec_from_file_location("make_plonk_lookup_fixture", path)
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    with open(mk.OUT, "rb") as fh:
        stored = fh.read()
    assert stored == mk.fixture_bytes(zk) and len(stored) < 24 << 10
    pr = mk.model_proof(zk)
    assert len(pr["pub"]) == mk.L_PUBLIC > 0 and pr["opening"]["k"] == 20
    assert KL.verify(pr, tr=KL.pow_transcript(mk.D, mk.F, mk.G_BITS, pr["nonce"]), hasher=mk.hasher(zk)) == (True, None)
    assert lib_verify(pr, g=mk.G_BITS, nonce=pr["nonce"]) == (0, 1)
