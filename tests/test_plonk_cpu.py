"""CPU: the host side of the Plonk proof over FRI commitments (include/zkmle.h "Plonk: gate, wiring and public inputs in one sumcheck").
Everything compares byte for byte against the big-integer model of tests/_plonk_model.py, which keeps the public inputs in an explicit table
inside the zerocheck (claimed sum 0):

  proofs      zk_plonk_verify and zk.plonk.verify accept the model's proofs at d = 1 .. 4 on both fields under the three schedules (log_arity 1;
              2; 2 with grouped leaves), with l among 0, 1, 3 and 2^d public values
  rejected    one flipped bit in every array of the proof (the helper roots among them); one public value changed; l off by one; two roots
              swapped; d + 1 and d - 1; a false gate row; a false wiring; a public value >= p; a nonce off by one; the cheating prover that
              commits H = 0 and sends g_0(1) = c - g_0(0)
  statuses    a status leaves a caller's transcript as it was
  transcript  the verifier's transcript ends in the model prover's state
  public      zk_plonk_public_eval equals the model for l = 0, 1, 2^d - 1, 2^d and a random tau
  sizes       zk_plonk_sizes equals the model's counts
  header      the protocol's text and the exports
  fixture     tests/golden/plonk_proof.bin, what tools/plonk_selftest.hip reads, is the model's proof and verifies

Commitments cannot exist without a device: the kernel and the prover run in tests/test_gpu_plonk.py."""
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
import _plonk_model as KM
from oracle import pymodel as M

zk = G.import_package()
P64, P8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
p64 = lambda a: a.ctypes.data_as(P64) if a is not None and a.size else None
p8 = lambda a: a.ctypes.data_as(P8) if a is not None else None
NEW_NAMES = ("zk_plonk_round", "zk_plonk_public_eval", "zk_plonk_sizes", "zk_plonk_prove", "zk_plonk_verify", "zk_plonk_last_stats")
SCHEDULES = [(1, False), (2, False), (2, True)]              # (log_arity, grouped)
# (field, d, b, f, coset, l): d = 1 .. 4 on both fields; l among 0, 1, 3 and 2^d; log_arity 2 runs where R = d - f >= 2
CASES = [(0, 1, 1, 0, False, 0), (3, 1, 2, 0, True, 1), (3, 1, 1, 0, False, 2), (0, 2, 2, 0, True, 3), (3, 2, 1, 1, False, 4), (3, 2, 1, 0, False, 1),
         (0, 3, 1, 1, False, 8), (3, 3, 2, 0, True, 3), (3, 3, 1, 2, True, 0), (0, 4, 2, 0, True, 3), (3, 4, 1, 2, False, 16), (0, 4, 1, 3, False, 1)]
Q = 4
case_id = lambda c: "-".join(str(int(v)) for v in c)
sched_id = lambda s: "a%d%s" % (s[0], "g" if s[1] else "")
runs = lambda case, sched: sched[0] == 1 or case[1] - case[3] >= 2
GRID = [pytest.param(c, s, id=case_id(c) + "-" + sched_id(s)) for c in CASES for s in SCHEDULES if runs(c, s)]
ARRAYS = ("own_roots", "h_roots", "polys", "ys", "open_polys", "roots", "final", "values", "paths")

hasher = functools.partial(FC.hasher, zk, True)
padded = functools.partial(FC.padded, room=16384)
coset_of = functools.partial(FC.coset_of, mul=67)


@functools.lru_cache(maxsize=None)
def statement(field, d, b, with_coset, grouped, l, false_gate=False, false_wiring=False):
    """-> (the eleven model commitments, the public values)"""
    p = NM.MODULUS[field]
    tabs, pub = KM.circuit(field, d, 5100 + 13 * d + field + l, l, false_gate=false_gate, false_wiring=false_wiring)
    assert KM.satisfied(tabs, pub, p) == (not false_gate, not false_wiring)
    coset = coset_of(field, d, b, with_coset)
    return tuple((GM if grouped else PM).commit(field, t, b, coset, hasher()) for t in tabs), tuple(pub)


@functools.lru_cache(maxsize=None)
def proof(case, sched, false_gate=False, false_wiring=False, cheat=False):
    field, d, b, f, with_coset, l = case
    cms, pub = statement(field, d, b, with_coset, sched[1], l, false_gate, false_wiring)
    return KM.prove(list(cms), list(pub), f, Q, sched[0], hasher=hasher(), cheat=cheat)


def lib_verify(pr, fl=None, tr=None, g=0, nonce=0, pub=None, npublic=None, **over):
    """zk_plonk_verify on the model's proof `pr` (flat arrays `fl`) -> (status, ok); pub: the verifier's own public values (an (l, 4) array)"""
    op = pr["opening"]
    fl = KM.flat(zk, pr) if fl is None else fl
    s = {n: op[n] for n in ("d", "b", "f", "Q", "a")}
    s["lg"] = 2 if op["grouped"] else 0
    s.update({n: v for n, v in over.items() if n in s})
    coset = over.get("coset", op["coset"])
    cm = None if coset is None else zk.from_ints(op["field"], [coset])[0]
    pub = fl["pub"] if pub is None else pub
    npublic = pub.shape[0] if npublic is None else npublic
    ok = C.c_int(-1)
    rc = zk.lib().zk_plonk_verify(over.get("field", op["field"]), p8(fl["own_roots"]), p64(pub), npublic, s["d"], s["b"], s["f"], s["Q"], s["a"], s["lg"], p64(cm),
                                  None if tr is None else tr._h, p8(fl["h_roots"]), p64(fl["polys"]), p64(fl["ys"]), p64(fl["open_polys"]), p8(fl["roots"]),
                                  p64(fl["final"]), p64(fl["values"]), p8(fl["paths"]), g, nonce, C.byref(ok))
    return rc, ok.value


def wrapper_proof(pr, fl, g=0, nonce=0):
    """zk.plonk.PlonkProof holding the model's arrays"""
    op = pr["opening"]
    cs = zk.from_ints(op["field"], [op["coset"]])[0]
    o = zk.plonk.PlonkProof(op["field"], op["d"], op["b"], op["f"], op["Q"], coset=cs, log_arity=op["a"], grouped=op["grouped"], grinding_bits=g)
    assert o.round_polys.shape == fl["polys"].shape == (op["d"], 5, 4) and o.drawn.shape == fl["drawn"].shape and o.challenges.shape == fl["challenges"].shape
    assert o.h_roots.shape == fl["h_roots"].shape == (3, 32)
    q = o.opening
    assert isinstance(q, zk.fri.FriMlBatchOpening)
    assert q.roots.shape == fl["roots"].shape and q.query_values.shape == fl["values"].shape and q.query_paths.shape == fl["paths"].shape
    assert q.ys.shape == (14, 1, 4) and q.round_polys.shape == fl["open_polys"].shape
    o.round_polys, o.drawn, o.challenges, o.h_roots = fl["polys"], fl["drawn"], fl["challenges"], fl["h_roots"]
    q.ys, q.round_polys, q.roots, q.final_table, q.query_values, q.query_paths = fl["ys"].reshape(14, 1, 4), fl["open_polys"], fl["roots"], fl["final"], fl["values"], fl["paths"]
    q.pow_nonce = nonce
    return o


def test_new_exports_and_the_header():
    lib = zk.lib()
    header = open(G.ROOT + "/include/zkmle.h").read()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in header, name
    assert "Plonk: gate, wiring and public inputs in one sumcheck" in header and "zk_plonk_stats" in header
    for text in ('"ZCPK"', "c = alpha^3 PIeval(tau)", "k = 14 in the order A, B, C, qM, qL, qR, qO, qC, SA, SB,", "plonk_round_kernel"):
        assert text in header, text
    for name in ("prove", "verify", "round", "public_eval", "sizes", "last_stats", "PlonkProof"):
        assert hasattr(zk.plonk, name), name
    assert zk.PlonkProof is zk.plonk.PlonkProof


def test_the_circuit_builder():
    for field in (0, 3):
        p = NM.MODULUS[field]
        for l in (0, 1, 3, 32):
            for kind in ("random", "identity", "3-cycle"):
                tabs, pub = KM.circuit(field, 5, 41 + field, l, kind)
                assert len(tabs) == 11 and len(pub) == l and KM.satisfied(tabs, pub, p) == (True, True)
                assert all(tabs[4][x] == 1 and not any(tabs[j][x] for j in (3, 5, 6, 7)) and tabs[0][x] == pub[x] for x in range(l))
            assert KM.satisfied(*KM.circuit(field, 5, 41 + field, l, false_gate=True), p) == (False, True)
            assert KM.satisfied(*KM.circuit(field, 5, 41 + field, l, false_wiring=True), p) == (True, False)
            if l:
                wrong = list(pub)
                wrong[l - 1] = (wrong[l - 1] + 1) % p
                assert KM.satisfied(tabs, wrong, p) == (False, True)


@pytest.mark.parametrize("case,sched", GRID)
def test_model_proofs_pass_the_model_verifier_and_the_library_verifier(case, sched):
    field, d, b, f, with_coset, l = case
    a, grouped = sched
    p = NM.MODULUS[field]
    pr = proof(case, sched)
    assert KM.verify(pr, hasher=hasher()) == (True, None)
    assert pr["own_first_sum"] == 0                           # the model's own polynomial, PI inside, sums to 0 on a satisfied circuit
    alpha, tau = pr["drawn"][2], pr["drawn"][4:]
    c = alpha ** 3 * KM.public_eval(pr["pub"], tau, p) % p
    assert all((g[0] + g[1]) % p == (c if k == 0 else KM.interpolate5(pr["polys"][k - 1], pr["challenges"][k - 1], p)) for k, g in enumerate(pr["polys"]))
    assert (c != 0) == (l > 0) and pr["opening"]["points"] == [pr["challenges"][::-1]]
    fl = KM.flat(zk, pr)
    assert fl["pub"].shape == (l, 4) and lib_verify(pr, fl) == (0, 1)
    if not with_coset:
        assert lib_verify(pr, fl, coset=None) == (0, 1)
    got = (fl["polys"].size // 4, fl["h_roots"].shape[0], fl["roots"].shape[0], fl["final"].shape[0], fl["values"].size // 4, fl["paths"].size, fl["open_polys"].size // 4)
    assert KM.sizes(d, b, f, Q, a, grouped) == got == zk.plonk.sizes(d, b, f, Q, a, grouped)
    o = wrapper_proof(pr, fl)
    assert zk.plonk.verify(pr["roots"], fl["pub"], o)
    assert not zk.plonk.verify(pr["roots"][::-1], fl["pub"], o)
    assert zk.plonk.verify(pr["roots"], None, o) is (l == 0)
    assert np.array_equal(o.point[0], fl["points"][0]) and np.array_equal(o.ys, fl["ys"])


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_the_public_values_are_part_of_the_statement(sched):
    for case in (CASES[9], CASES[10], CASES[3] if sched[0] == 1 else CASES[7]):
        field, d, l = case[0], case[1], case[5]
        p, rng = NM.MODULUS[field], random.Random(case[1] + l)
        pr = proof(case, sched)
        fl = KM.flat(zk, pr)
        n = 1 << d
        for x in sorted({0, l - 1, rng.randrange(l)}):        # one public value changed
            wrong = list(pr["pub"])
            wrong[x] = (wrong[x] + 1) % p
            assert lib_verify(pr, fl, pub=KM.mont(zk, field, wrong)) == (0, 0), (case, x)
            assert KM.verify(pr, pub=wrong, hasher=hasher())[0] is False
            flipped = fl["pub"].copy()
            flipped[x, rng.randrange(4)] ^= np.uint64(1 << rng.randrange(60))
            assert lib_verify(pr, fl, pub=flipped) == (0, 0), (case, x)
        room = np.concatenate([fl["pub"], np.zeros((1, 4), np.uint64)])
        assert lib_verify(pr, fl, pub=room, npublic=l) == (0, 1)
        assert lib_verify(pr, fl, pub=room, npublic=l - 1) == (0, 0)          # l off by one: the tag and the absorbed values change
        assert KM.verify(pr, pub=pr["pub"][:-1], hasher=hasher())[0] is False
        if l < n:
            assert lib_verify(pr, fl, pub=room, npublic=l + 1) == (0, 0)      # one more value, a zero: the same PI table, another statement
            assert KM.verify(pr, pub=pr["pub"] + [0], hasher=hasher())[0] is False
        big = fl["pub"].copy()                                                # a public value >= p: not a status
        big[l - 1] = np.uint64(0xFFFFFFFFFFFFFFFF)
        assert lib_verify(pr, fl, pub=big) == (0, 0)
        modulus = np.frombuffer(p.to_bytes(32, "little"), np.uint64)
        big[l - 1] = modulus
        assert lib_verify(pr, fl, pub=big) == (0, 0)
        assert KM.verify(pr, pub=pr["pub"][:-1] + [p + pr["pub"][-1]], hasher=hasher())[0] is False


def test_statuses_come_before_the_transcript_is_touched():
    from zkmle_amd import _lib as L
    pr = proof(CASES[7], SCHEDULES[0])
    fl = KM.flat(zk, pr)
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
    assert lib.zk_plonk_verify(op["field"], p8(fl["own_roots"]), p64(fl["pub"]), 3, 3, 2, 0, Q, 1, 0, None, t._h, p8(fl["h_roots"]), p64(fl["polys"]), p64(fl["ys"]),
                               p64(fl["open_polys"]), p8(fl["roots"]), p64(fl["final"]), p64(fl["values"]), p8(fl["paths"]), 0, 0, None) == L.ZK_E_ARG
    big = padded(fl)
    for over, want in ((dict(field=7), L.ZK_E_ARG), (dict(field=-1), L.ZK_E_ARG), (dict(field=1, coset=None), L.ZK_E_RANGE), (dict(field=2, coset=None), L.ZK_E_RANGE),
                       (dict(coset=0), L.ZK_E_ARG), (dict(d=NM.two_adicity(3) - 1, b=2), L.ZK_E_RANGE), (dict(d=31, b=2), L.ZK_E_RANGE),
                       (dict(d=0), L.ZK_E_ARG), (dict(f=3), L.ZK_E_ARG), (dict(b=0), L.ZK_E_ARG), (dict(Q=0), L.ZK_E_ARG), (dict(a=3), L.ZK_E_ARG),
                       (dict(lg=2), L.ZK_E_ARG), (dict(lg=1), L.ZK_E_ARG), (dict(a=2, f=2), L.ZK_E_ARG)):
        assert lib_verify(pr, big, t, pub=fl["pub"], **over) == (want, -1), over
    assert lib_verify(pr, big, t, pub=fl["pub"], g=33)[0] == L.ZK_E_ARG
    # the public inputs' own statuses: more values than rows, and no array where values are announced
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
        base = KM.flat(zk, pr)
        rng = random.Random(41 * len(name) + case[1] + sched[0])
        flat_size = base[name].size
        spots = {0, flat_size - 1} | {rng.randrange(flat_size) for _ in range(6)}
        for at in sorted(spots):
            fl = {n: v.copy() for n, v in base.items()}
            view = fl[name].reshape(-1)
            view[at] ^= view.dtype.type(1 << rng.randrange(8 if view.dtype == np.uint8 else 64))
            assert lib_verify(pr, fl) == (0, 0), (case, name, at)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_swapped_roots_and_another_d_are_rejected(sched):
    case = CASES[9]                                           # d = 4, f = 0, l = 3
    pr = proof(case, sched)
    base = KM.flat(zk, pr)
    for i, j in ((0, 1), (3, 4), (8, 9), (0, 8), (2, 7)):     # A with B; qM with qL; SA with SB; A with SA; C with qC
        sw = {n: v.copy() for n, v in base.items()}
        sw["own_roots"][[i, j]] = sw["own_roots"][[j, i]]
        assert lib_verify(pr, sw) == (0, 0), (i, j)
        sw["roots"][[i, j]] = sw["roots"][[j, i]]             # ... and the proof's copy with them
        assert lib_verify(pr, sw) == (0, 0), (i, j)
        sw["ys"][[i, j]] = sw["ys"][[j, i]]                   # ... and the claims: the statement's transcript has the roots in another order
        assert lib_verify(pr, sw) == (0, 0), (i, j)
        roots = list(pr["roots"])
        roots[i], roots[j] = roots[j], roots[i]
        assert KM.verify(pr, roots=roots, hasher=hasher())[0] is False
    sw = {n: v.copy() for n, v in base.items()}
    sw["h_roots"][[0, 1]] = sw["h_roots"][[1, 0]]             # two helper roots
    assert lib_verify(pr, sw) == (0, 0)
    big = padded(base)
    assert lib_verify(pr, big, pub=base["pub"]) == (0, 1)
    assert lib_verify(pr, big, pub=base["pub"], d=5) == (0, 0) and lib_verify(pr, big, pub=base["pub"], d=3) == (0, 0)
    assert lib_verify(pr, big, pub=base["pub"], f=1) == (0, 0) and lib_verify(pr, big, pub=base["pub"], Q=Q + 1) == (0, 0)
    assert lib_verify(pr, big, pub=base["pub"], b=1) == (0, 0)


@pytest.mark.parametrize("field", (0, 3))
@pytest.mark.parametrize("d", (1, 2, 3, 4))
def test_false_statements_and_the_cheating_prover_are_rejected(field, d):
    l = (1, 0, 3, 16)[d - 1]
    case = (field, d, 1, 0, d % 2 == 0, l)
    for sched in SCHEDULES:
        if not runs(case, sched):
            continue
        for false in (dict(false_gate=True), dict(false_wiring=True)):
            pr = proof(case, sched, **false)
            assert KM.verify(pr, hasher=hasher()) == (False, 0), false
            assert pr["own_first_sum"] != 0 and lib_verify(pr) == (0, 0), false
            ch = proof(case, sched, cheat=True, **false)
            ok, failed = KM.verify(ch, hasher=hasher())
            assert not ok and 1 <= failed <= d, false         # a later round's sum, or the last claim: never the opening, which is honest
            assert lib_verify(ch) == (0, 0), false
        # the cheating prover on a true statement too: H = 0 is not what the helper step says unless S = id
        ch = proof(case, sched, cheat=True)
        assert lib_verify(ch) == (0, int(KM.verify(ch, hasher=hasher())[0]))


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_the_proof_of_work_nonce(sched):
    field, d, b, f, with_coset, l = case = CASES[10]          # d = 4, f = 2, l = 16
    G_BITS = 4
    cms, pub = statement(field, d, b, with_coset, sched[1], l)
    mt = KM.pow_transcript(d, f, G_BITS)
    pr = KM.prove(list(cms), list(pub), f, Q, sched[0], mt, hasher())
    w = pr["nonce"]
    assert mt.pow_ok and mt.nonce == w
    assert KM.verify(pr, tr=KM.pow_transcript(d, f, G_BITS, w), hasher=hasher()) == (True, None)
    fl = KM.flat(zk, pr)
    assert lib_verify(pr, fl, g=G_BITS, nonce=w) == (0, 1)
    assert lib_verify(pr, fl, g=G_BITS, nonce=w + 1) == (0, 0) and lib_verify(pr, fl, g=G_BITS, nonce=(w - 1) % (1 << 64)) == (0, 0)
    assert lib_verify(pr, fl, g=G_BITS + 1, nonce=w) == (0, 0) and lib_verify(pr, fl) == (0, 0)
    assert KM.verify(pr, tr=KM.pow_transcript(d, f, G_BITS, w + 1), hasher=hasher())[0] is False
    plain = proof(case, sched)
    assert lib_verify(plain, g=G_BITS, nonce=w) == (0, 0)     # indices drawn without the step
    o = wrapper_proof(pr, fl, G_BITS, w)
    assert zk.plonk.verify(pr["roots"], fl["pub"], o)
    o.opening.pow_nonce = w + 1
    assert not zk.plonk.verify(pr["roots"], fl["pub"], o)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_a_callers_transcript(sched):
    field, d, b, f, with_coset, l = CASES[7]
    prior = b"what the caller had absorbed before"
    cms, pub = statement(field, d, b, with_coset, sched[1], l)
    mt = M.Transcript()
    mt.append(prior)
    pr = KM.prove(list(cms), list(pub), f, Q, sched[0], mt, hasher())
    vt = M.Transcript()
    vt.append(prior)
    assert KM.verify(pr, tr=vt, hasher=hasher()) == (True, None) and vt.buf == mt.buf
    t, want = zk.Transcript(), zk.Transcript()
    t.append(prior)
    assert lib_verify(pr, tr=t) == (0, 1)
    want.append(bytes(mt.buf))
    assert np.array_equal(t.export_state(), want.export_state())   # the verifier's transcript ends in the model prover's state
    assert lib_verify(pr) == (0, 0)                           # the proof is bound to the prior content
    t2 = zk.Transcript()
    t2.append(prior + b"!")
    assert lib_verify(pr, tr=t2) == (0, 0)


@pytest.mark.parametrize("field", (0, 3))
def test_public_eval_equals_the_model(field):
    from zkmle_amd import _lib as L
    p, rng = NM.MODULUS[field], random.Random(77 + field)
    for d in (1, 2, 3, 5, 7):
        n = 1 << d
        tau = [rng.randrange(p) for _ in range(d)]
        tau_m = KM.mont(zk, field, tau)
        for l in sorted({0, 1, 3 % n, n // 2, n - 1, n}):
            pub = [rng.randrange(p) for _ in range(l)]
            got = zk.plonk.public_eval(field, KM.mont(zk, field, pub) if l else None, tau_m)
            assert np.array_equal(got, KM.mont(zk, field, [KM.public_eval(pub, tau, p)])[0]), (d, l)
        # Boolean tau: the value itself, or 0 past the end
        x = rng.randrange(n)
        bits = KM.mont(zk, field, [(x >> (d - 1 - i)) & 1 for i in range(d)])
        pub = [rng.randrange(1, p) for _ in range(n)]
        assert np.array_equal(zk.plonk.public_eval(field, KM.mont(zk, field, pub), bits), KM.mont(zk, field, [pub[x]])[0])
        assert np.array_equal(zk.plonk.public_eval(field, KM.mont(zk, field, pub[:x]) if x else None, bits), np.zeros(4, np.uint64))
    lib, out = zk.lib(), np.full(4, 7, np.uint64)
    one, bad = KM.mont(zk, field, [1, 1, 1]), np.full((1, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
    ev = lambda f, pub, l, tau, d, o: lib.zk_plonk_public_eval(f, p64(pub), l, p64(tau), d, p64(o) if o is not None else None)
    assert ev(field, one, 3, one, 1, out) == L.ZK_E_ARG       # l > 2^d
    assert ev(field, None, 1, one, 2, out) == L.ZK_E_ARG and ev(field, one, 1, None, 2, out) == L.ZK_E_ARG and ev(field, one, 1, one, 2, None) == L.ZK_E_ARG
    assert ev(field, one, 1, one, 0, out) == L.ZK_E_ARG and ev(field, one, 1, one, 33, out) == L.ZK_E_ARG and ev(1, one, 1, one, 2, out) == L.ZK_E_ARG
    assert ev(field, bad, 1, one, 2, out) == L.ZK_E_ARG and ev(field, one, 1, bad, 1, out) == L.ZK_E_ARG
    assert (out == 7).all()
    assert ev(field, None, 0, one, 2, out) == 0 and not out.any()


def test_sizes():
    from zkmle_amd import _lib as L
    lib = zk.lib()

    def sizes(d, b, f, q, a, lg):
        out = [C.c_size_t(0) for _ in range(7)]
        rc = lib.zk_plonk_sizes(d, b, f, q, a, lg, *[C.byref(o) for o in out])
        return rc, tuple(int(o.value) for o in out)

    for d in (1, 2, 3, 4, 6, 10, 24):
        for b in (1, 2):
            for f in range(0, d):
                for q in (1, 8, 64):
                    for a, grouped in SCHEDULES:
                        if a == 2 and d - f < 2:
                            assert sizes(d, b, f, q, a, 2 * grouped)[0] == L.ZK_E_ARG
                            continue
                        want = (5 * d, 3) + zk.fri.ml_sizes(d, b, f, q, log_arity=a, grouped=grouped, k=14)
                        assert sizes(d, b, f, q, a, 2 * grouped) == (0, want) and KM.sizes(d, b, f, q, a, grouped) == want
                        assert zk.plonk.sizes(d, b, f, q, a, grouped) == want
    for d, b, f, q, a, lg in ((0, 1, 0, 4, 1, 0), (3, 0, 0, 4, 1, 0), (3, 1, 3, 4, 1, 0), (3, 1, 0, 0, 1, 0), (3, 1, 0, 4, 0, 0), (3, 1, 0, 4, 3, 0), (3, 1, 0, 4, 1, 2)):
        assert sizes(d, b, f, q, a, lg)[0] == L.ZK_E_ARG
    assert sizes(40, 1, 0, 8, 1, 0)[0] == L.ZK_E_RANGE
    assert lib.zk_plonk_sizes(4, 1, 0, 8, 2, 2, None, None, None, None, None, None, None) == 0
    with pytest.raises(ValueError):
        zk.plonk.sizes(4, 1, 0, 8, log_arity=1, grouped=True)


def test_prover_and_hook_statuses_without_a_device():
    from zkmle_amd import _lib as L
    lib = zk.lib()
    h = {}
    for field, n in ((0, 1), (0, 2), (0, 4), (0, 8), (0, 6), (1, 8), (3, 4)):
        h[field, n] = C.c_void_p()
        L.check(lib.zk_table_wrap(field, C.c_void_p(0x1000), n, C.byref(h[field, n])))
    g5 = np.full(20, 7, np.uint64)
    outs = (C.c_void_p * 15)()
    one = zk.from_ints(0, [1])[0]
    unreduced = np.full(4, 0xFFFFFFFFFFFFFFFF, np.uint64)

    def rnd(tabs, r=None, o=outs, g=g5, el=None, step=0):
        arr = (C.c_void_p * 15)(*[None if t is None else t.value for t in tabs])
        el = [one] * 5 if el is None else el
        return lib.zk_plonk_round(arr, *[p64(e) for e in el], step, p64(r), o, p64(g))

    t4, t8 = h[0, 4], h[0, 8]
    assert lib.zk_plonk_round(None, p64(one), p64(one), p64(one), p64(one), p64(one), 0, None, outs, p64(g5)) == L.ZK_E_ARG
    for i in range(15):
        tabs = [t4] * 15
        tabs[i] = None
        assert rnd(tabs) == L.ZK_E_ARG
        tabs[i] = h[3, 4]
        assert rnd(tabs) == L.ZK_E_ARG
        if i:
            tabs[i] = t8
            assert rnd(tabs) == L.ZK_E_LEN_MISMATCH
    assert rnd([t4] * 15, g=None) == L.ZK_E_ARG and rnd([t4] * 15, r=one, o=None) == L.ZK_E_ARG and rnd([h[1, 8]] * 15) == L.ZK_E_ARG
    assert rnd([h[0, 6]] * 15) == L.ZK_E_NOT_POW2
    assert rnd([h[0, 1]] * 15) == L.ZK_E_ARG and rnd([h[0, 2]] * 15, r=one) == L.ZK_E_ARG and rnd([t4] * 15, r=unreduced) == L.ZK_E_ARG
    for i in range(5):
        el = [one] * 5
        el[i] = None
        assert rnd([t4] * 15, el=el) == L.ZK_E_ARG
        el[i] = unreduced
        assert rnd([t4] * 15, el=el) == L.ZK_E_ARG
    assert rnd([t4] * 15, step=31) == L.ZK_E_ARG and rnd([t4] * 15, step=33) == L.ZK_E_ARG
    import torch
    if not torch.cuda.is_available():
        assert rnd([h[0, 2]] * 15) == L.ZK_E_NO_DEVICE and rnd([t4] * 15, r=one) == L.ZK_E_NO_DEVICE
    assert (g5 == 7).all() and not any(outs)
    w = lambda n: np.full(n, 7, np.uint64)
    bufs = [w(64) for _ in range(9)]
    r8, hr = np.full(64 * 32, 7, np.uint8), np.full(96, 7, np.uint8)
    prove = lambda cms: lib.zk_plonk_prove(cms, None, 0, 0, 4, 1, 0, None, p8(hr), p64(bufs[0]), p64(bufs[1]), p64(bufs[2]), p64(bufs[3]), p64(bufs[4]), p64(bufs[5]),
                                           p8(r8), p64(bufs[6]), None, None, p64(bufs[7]), p8(r8), None)
    assert prove(None) == L.ZK_E_ARG and prove((C.c_void_p * 11)()) == L.ZK_E_ARG
    assert all((x == 7).all() for x in bufs) and (r8 == 7).all() and (hr == 7).all()
    assert lib.zk_plonk_last_stats(None) == L.ZK_E_ARG
    for t in h.values():
        lib.zk_table_free(t)


def test_the_selftest_fixture_is_the_models_proof():
    import importlib.util
    path = os.path.join(G.ROOT, "tests", "golden", "make_plonk_fixture.py")
    spec = importlib.util.spec_from_file_location("make_plonk_fixture", path)
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    with open(mk.OUT, "rb") as fh:
        stored = fh.read()
    assert stored == mk.fixture_bytes(zk) and len(stored) < 24 << 10
    pr = mk.model_proof(zk)
    assert len(pr["pub"]) == mk.L_PUBLIC > 0
    assert KM.verify(pr, tr=KM.pow_transcript(mk.D, mk.F, mk.G_BITS, pr["nonce"]), hasher=mk.hasher(zk)) == (True, None)
    assert lib_verify(pr, g=mk.G_BITS, nonce=pr["nonce"]) == (0, 1)
