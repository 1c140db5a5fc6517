"""CPU: the host side of the zerocheck of a Plonk gate over eight FRI commitments (include/zkmle.h "Zerocheck of a Plonk gate over committed
tables").  Everything compares byte for byte against the big-integer model of tests/_zerocheck_gate_model.py:

  proofs      the model round-trips at d = 1 .. 4 on both fields under the three schedules (log_arity 1; 2; 2 with grouped leaves), with and
              without a coset, on satisfied circuits (additions, multiplications, constant rows, rows of random selectors);
              zk_zerocheck_gate_verify and zk.zerocheck.verify_gate accept the model's proofs
  statuses    NULL, a bad field, d + log_blowup over the two-adicity, a zero coset: a status, and a caller's transcript is as it was
  rejected    one flipped bit in each part of the proof and in a root the verifier holds; two roots swapped (A with B, qL with qR, A with
              qM), alone, with the proof's copy of them, and with the claims as well; d shown as d + 1 and d - 1; the model prover on a
              false statement (the first check fails) and the prover that hides it from the first check (a later one fails, while the
              opening alone still verifies); the proof-of-work nonce off by one
  transcript  a caller's transcript ends in the model's state on ZK_OK, and another prefix gives another tau
  sizes       zk_zerocheck_gate_sizes equals the model's counts
  fixture     tests/golden/zerocheck_gate_proof.bin, what tools/zerocheck_selftest.hip reads as its second fixture, is the model's proof

Commitments cannot exist without a device: the round kernel and the prover run in tests/test_gpu_zerocheck_gate.py."""
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
import _zerocheck_gate_model as ZG
from oracle import pymodel as M

zk = G.import_package()
P64, P8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
p64 = lambda a: a.ctypes.data_as(P64) if a is not None else None
p8 = lambda a: a.ctypes.data_as(P8) if a is not None else None
NEW_NAMES = ("zk_zerocheck_gate_round", "zk_zerocheck_gate_sizes", "zk_zerocheck_gate_prove", "zk_zerocheck_gate_verify")
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


@functools.lru_cache(maxsize=None)
def commitments(field, d, b, with_coset, grouped, false_at=None):
    coset = coset_of(field, d, b, with_coset)
    return tuple((GM if grouped else PM).commit(field, t, b, coset, hasher()) for t in ZG.circuit(field, 1 << d, 9700 + 17 * d + field, false_at))


@functools.lru_cache(maxsize=None)
def proof(case, sched, false_at=None, cheat=False):
    field, d, b, f, with_coset = case
    return ZG.prove(list(commitments(field, d, b, with_coset, sched[1], false_at)), f, Q, sched[0], hasher=hasher(), cheat=cheat)


def lib_verify(pr, fl=None, tr=None, g=0, nonce=0, **over):
    """zk_zerocheck_gate_verify on the model's proof `pr` (flat arrays `fl`) -> (status, ok)"""
    op = pr["opening"]
    fl = ZG.flat(zk, pr) if fl is None else fl
    s = {n: op[n] for n in ("d", "b", "f", "Q", "a")}
    s["lg"] = 2 if op["grouped"] else 0
    s.update({n: v for n, v in over.items() if n in s})
    coset = over.get("coset", op["coset"])
    cm = None if coset is None else zk.from_ints(op["field"], [coset])[0]
    ok = C.c_int(-1)
    rc = zk.lib().zk_zerocheck_gate_verify(over.get("field", op["field"]), p8(fl["own_roots"]), s["d"], s["b"], s["f"], s["Q"], s["a"], s["lg"], p64(cm),
                                           None if tr is None else tr._h, p64(fl["polys"]), p64(fl["ys"]), p64(fl["open_polys"]), p8(fl["roots"]),
                                           p64(fl["final"]), p64(fl["values"]), p8(fl["paths"]), g, nonce, C.byref(ok))
    return rc, ok.value


def wrapper_proof(pr, fl, g=0, nonce=0):
    """zk.zerocheck.ZerocheckGateProof holding the model's arrays"""
    op = pr["opening"]
    cs = zk.from_ints(op["field"], [op["coset"]])[0]
    o = zk.zerocheck.ZerocheckGateProof(op["field"], op["d"], op["b"], op["f"], op["Q"], coset=cs, log_arity=op["a"], grouped=op["grouped"], grinding_bits=g)
    assert o.round_polys.shape == fl["polys"].shape == (op["d"], 5, 4) and o.tau.shape == fl["tau"].shape and o.challenges.shape == fl["challenges"].shape
    q = o.opening
    assert isinstance(q, zk.fri.FriMlBatchOpening)
    assert q.roots.shape == fl["roots"].shape and q.query_values.shape == fl["values"].shape and q.query_paths.shape == fl["paths"].shape
    assert q.ys.shape == (8, 1, 4) and q.round_polys.shape == fl["open_polys"].shape
    o.round_polys, o.tau, o.challenges = fl["polys"], fl["tau"], fl["challenges"]
    q.ys, q.round_polys, q.roots, q.final_table, q.query_values, q.query_paths = fl["ys"].reshape(8, 1, 4), fl["open_polys"], fl["roots"], fl["final"], fl["values"], fl["paths"]
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
    assert "Zerocheck of a Plonk gate over committed tables" in header
    for name in ("gate_round", "prove_gate", "verify_gate", "gate_sizes", "last_stats", "ZerocheckGateProof"):
        assert hasattr(zk.zerocheck, name), name


def test_the_circuit_generator_makes_satisfied_rows_of_every_kind():
    for field in (0, 3):
        p = NM.MODULUS[field]
        cols = ZG.circuit(field, 64, 77 + field)
        assert all(ZG.gate(*row) % p == 0 for row in zip(*cols))
        sel = [v for col in cols[3:] for v in col]
        assert sum(v in (0, 1, p - 1) for v in sel) > len(sel) // 2   # selectors sit mostly at 0, 1 and p - 1
        assert any(qm == 1 for qm in cols[3]) and any(ql == 1 and qr == 1 for ql, qr in zip(cols[4], cols[5])) and any(qc not in (0, 1, p - 1) for qc in cols[7])
        bad = ZG.circuit(field, 64, 77 + field, false_at=9)
        assert [ZG.gate(*row) % p == 0 for row in zip(*bad)].count(False) == 1


@pytest.mark.parametrize("case,sched", GRID)
def test_model_proofs_pass_the_model_verifier_and_the_library_verifier(case, sched):
    field, d, b, f, with_coset = case
    a, grouped = sched
    p = NM.MODULUS[field]
    pr = proof(case, sched)
    assert ZG.verify(pr, hasher=hasher()) == (True, None)
    assert len(pr["polys"]) == d and all(len(g) == 5 for g in pr["polys"])
    assert all((g[0] + g[1]) % p == (0 if l == 0 else ZG.interpolate5(pr["polys"][l - 1], pr["challenges"][l - 1], p)) for l, g in enumerate(pr["polys"]))
    assert pr["opening"]["points"] == [pr["challenges"][::-1]]
    fl = ZG.flat(zk, pr)
    assert lib_verify(pr, fl) == (0, 1)
    if not with_coset:
        assert lib_verify(pr, fl, coset=None) == (0, 1)
    got = (fl["polys"].size // 4, fl["roots"].shape[0], fl["final"].shape[0], fl["values"].size // 4, fl["paths"].size, fl["open_polys"].size // 4)
    assert ZG.sizes(d, b, f, Q, a, grouped) == got == zk.zerocheck.gate_sizes(d, b, f, Q, a, grouped)
    o = wrapper_proof(pr, fl)
    assert zk.zerocheck.verify_gate(pr["roots"], o)
    assert not zk.zerocheck.verify_gate(pr["roots"][::-1], o)
    assert np.array_equal(o.point[0], fl["points"][0]) and np.array_equal(o.ys, fl["ys"])


def test_statuses_come_before_the_transcript_is_touched():
    from zkmle_amd import _lib as L
    pr = proof(CASES[6], SCHEDULES[0])
    fl = ZG.flat(zk, pr)
    t = zk.Transcript()
    t.append(b"the caller's own")
    before = t.export_state().copy()
    for name in ("own_roots", "polys", "ys", "open_polys", "roots", "final", "values", "paths"):
        class Without(dict):
            def __getitem__(self, key, name=name):
                return None if key == name else dict.__getitem__(self, key)
        assert lib_verify(pr, Without(fl), t)[0] == L.ZK_E_ARG, name
    op = pr["opening"]
    lib = zk.lib()
    assert lib.zk_zerocheck_gate_verify(op["field"], p8(fl["own_roots"]), 3, 2, 0, Q, 1, 0, None, t._h, p64(fl["polys"]), p64(fl["ys"]), p64(fl["open_polys"]),
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


SPOTS = ("polys", "ys", "own_roots", "roots", "open_polys", "final", "values", "paths")


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
@pytest.mark.parametrize("name", SPOTS)
def test_one_flipped_bit_is_rejected(name, sched):
    for case in (CASES[8], CASES[7] if sched[0] == 1 else CASES[6]):
        pr = proof(case, sched)
        base = ZG.flat(zk, pr)
        rng = random.Random(37 * len(name) + case[1] + sched[0])
        flat_size = base[name].size
        spots = {0, flat_size - 1} | {rng.randrange(flat_size) for _ in range(6)}
        for at in sorted(spots):
            fl = {n: v.copy() for n, v in base.items()}
            view = fl[name].reshape(-1)
            view[at] ^= view.dtype.type(1 << rng.randrange(8 if view.dtype == np.uint8 else 64))
            assert lib_verify(pr, fl) == (0, 0), (case, name, at)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_swapped_roots_and_another_d_are_rejected(sched):
    case = CASES[8]                                           # d = 4, f = 0
    pr = proof(case, sched)
    base = ZG.flat(zk, pr)
    for i, j in ((0, 1), (4, 5), (0, 3)):                     # A with B; qL with qR; A with qM
        sw = {n: v.copy() for n, v in base.items()}
        sw["own_roots"][[i, j]] = sw["own_roots"][[j, i]]
        assert lib_verify(pr, sw) == (0, 0), (i, j)
        sw["roots"][[i, j]] = sw["roots"][[j, i]]             # ... and the proof's copy with them
        assert lib_verify(pr, sw) == (0, 0), (i, j)
        sw["ys"][[i, j]] = sw["ys"][[j, i]]                   # ... and the claims: the statement's transcript has the roots in another order
        assert lib_verify(pr, sw) == (0, 0), (i, j)
        assert ZG.verify(pr, roots=swapped(pr["roots"], i, j), hasher=hasher())[0] is False
    big = padded(base)
    assert lib_verify(pr, big) == (0, 1)
    assert lib_verify(pr, big, d=5) == (0, 0) and lib_verify(pr, big, d=3) == (0, 0)
    assert lib_verify(pr, big, f=1) == (0, 0) and lib_verify(pr, big, Q=Q + 1) == (0, 0) and lib_verify(pr, big, b=1) == (0, 0)


@pytest.mark.parametrize("field", (0, 3))
@pytest.mark.parametrize("d", (1, 2, 3, 4))
def test_a_false_statement_fails_the_first_check_and_a_hidden_one_a_later_check(field, d):
    case = (field, d, 1, 0, d % 2 == 0)
    for sched in SCHEDULES:
        if not runs(case, sched):
            continue
        at = (5 * d + field) % (1 << d)
        pr = proof(case, sched, false_at=at)
        assert ZG.verify(pr, hasher=hasher()) == (False, 0)
        assert lib_verify(pr) == (0, 0)
        ch = proof(case, sched, false_at=at, cheat=True)
        ok, failed = ZG.verify(ch, hasher=hasher())
        assert not ok and 1 <= failed <= d                   # a later round's sum, or the last claim: never the opening, which is honest
        assert lib_verify(ch) == (0, 0)
        # the opening alone is a good one: the claims are the tables' values
        fl = ZG.flat(zk, ch)
        ok_open = C.c_int(-1)
        op = ch["opening"]
        vt = M.Transcript()
        ZG._statement(vt, ch["roots"], d, NM.MODULUS[field])
        for g in ch["polys"]:
            for e in g:
                vt.append(ZG.be32(e))
            vt.challenge(NM.MODULUS[field])
        t = zk.Transcript()
        t.append(bytes(vt.buf))
        cs = zk.from_ints(field, [op["coset"]])[0]
        assert zk.lib().zk_fri_ml_verify_batch(field, p8(fl["own_roots"]), 8, d, 1, 0, Q, op["a"], 2 if op["grouped"] else 0, p64(cs), p64(fl["points"]), 1,
                                               p64(fl["ys"]), t._h, p64(fl["open_polys"]), p8(fl["roots"]), p64(fl["final"]), p64(fl["values"]),
                                               p8(fl["paths"]), C.byref(ok_open)) == 0 and ok_open.value == 1


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_the_proof_of_work_nonce(sched):
    field, d, b, f, with_coset = case = CASES[9]              # d = 4, f = 2
    G_BITS = 4
    cms = list(commitments(field, d, b, with_coset, sched[1]))
    mt = ZG.pow_transcript(d, f, G_BITS)
    pr = ZG.prove(cms, f, Q, sched[0], mt, hasher())
    w = pr["nonce"]
    assert mt.pow_ok and mt.nonce == w
    assert ZG.verify(pr, tr=ZG.pow_transcript(d, f, G_BITS, w), hasher=hasher()) == (True, None)
    fl = ZG.flat(zk, pr)
    assert lib_verify(pr, fl, g=G_BITS, nonce=w) == (0, 1)
    assert lib_verify(pr, fl, g=G_BITS, nonce=w + 1) == (0, 0) and lib_verify(pr, fl, g=G_BITS, nonce=(w - 1) % (1 << 64)) == (0, 0)
    assert lib_verify(pr, fl, g=G_BITS + 1, nonce=w) == (0, 0) and lib_verify(pr, fl) == (0, 0)
    assert ZG.verify(pr, tr=ZG.pow_transcript(d, f, G_BITS, w + 1), hasher=hasher())[0] is False
    plain = proof(case, sched)
    assert lib_verify(plain, g=G_BITS, nonce=w) == (0, 0)     # indices drawn without the step
    o = wrapper_proof(pr, fl, G_BITS, w)
    assert zk.zerocheck.verify_gate(pr["roots"], o)
    o.opening.pow_nonce = w + 1
    assert not zk.zerocheck.verify_gate(pr["roots"], o)


@pytest.mark.parametrize("sched", SCHEDULES, ids=sched_id)
def test_a_callers_transcript(sched):
    field, d, b, f, with_coset = CASES[6]
    prior = b"what the caller had absorbed before"
    cms = list(commitments(field, d, b, with_coset, sched[1]))
    mt = M.Transcript()
    mt.append(prior)
    pr = ZG.prove(cms, f, Q, sched[0], mt, hasher())
    vt = M.Transcript()
    vt.append(prior)
    assert ZG.verify(pr, tr=vt, hasher=hasher()) == (True, None) and vt.buf == mt.buf
    t, want = zk.Transcript(), zk.Transcript()
    t.append(prior)
    assert lib_verify(pr, tr=t) == (0, 1)
    want.append(bytes(mt.buf))
    assert np.array_equal(t.export_state(), want.export_state())
    assert lib_verify(pr) == (0, 0)                           # the proof is bound to the prior content
    other = M.Transcript()
    other.append(prior + b"!")
    pr2 = ZG.prove(cms, f, Q, sched[0], other, hasher())
    assert pr2["tau"] != pr["tau"] and pr["tau"] != proof(CASES[6], sched)["tau"]
    t2 = zk.Transcript()
    t2.append(prior + b"!")
    assert lib_verify(pr, tr=t2) == (0, 0) and lib_verify(pr2, tr=t2) == (0, 0)   # t2 has moved on: a transcript proves once


def test_sizes():
    from zkmle_amd import _lib as L
    lib = zk.lib()

    def sizes(d, b, f, q, a, lg):
        out = [C.c_size_t(0) for _ in range(6)]
        rc = lib.zk_zerocheck_gate_sizes(d, b, f, q, a, lg, *[C.byref(o) for o in out])
        return rc, tuple(int(o.value) for o in out)

    for d in (1, 2, 3, 4, 6, 10, 24):
        for b in (1, 2):
            for f in range(0, d):
                for q in (1, 8, 64):
                    for a, grouped in SCHEDULES:
                        if a == 2 and d - f < 2:
                            assert sizes(d, b, f, q, a, 2 * grouped)[0] == L.ZK_E_ARG
                            continue
                        want = (5 * d,) + zk.fri.ml_sizes(d, b, f, q, log_arity=a, grouped=grouped, k=8)
                        assert sizes(d, b, f, q, a, 2 * grouped) == (0, want) and ZG.sizes(d, b, f, q, a, grouped) == want
                        assert zk.zerocheck.gate_sizes(d, b, f, q, a, grouped) == want
    for d, b, f, q, a, lg in ((0, 1, 0, 4, 1, 0), (3, 0, 0, 4, 1, 0), (3, 1, 3, 4, 1, 0), (3, 1, 0, 0, 1, 0), (3, 1, 0, 4, 0, 0), (3, 1, 0, 4, 3, 0), (3, 1, 0, 4, 1, 2)):
        assert sizes(d, b, f, q, a, lg)[0] == L.ZK_E_ARG
    assert sizes(40, 1, 0, 8, 1, 0)[0] == L.ZK_E_RANGE
    assert lib.zk_zerocheck_gate_sizes(4, 1, 0, 8, 2, 2, None, None, None, None, None, None) == 0
    with pytest.raises(ValueError):
        zk.zerocheck.gate_sizes(4, 1, 0, 8, log_arity=1, grouped=True)


def test_prover_and_round_statuses_without_a_device():
    from zkmle_amd import _lib as L
    lib = zk.lib()
    h = {}
    for field, n in ((0, 1), (0, 2), (0, 4), (0, 8), (0, 6), (1, 8), (3, 4)):
        h[field, n] = C.c_void_p()
        L.check(lib.zk_table_wrap(field, C.c_void_p(0x1000), n, C.byref(h[field, n])))
    g5 = np.full(20, 7, np.uint64)
    outs = (C.c_void_p * 9)()
    one = zk.from_ints(0, [1])[0]
    unreduced = np.full(4, 0xFFFFFFFFFFFFFFFF, np.uint64)

    def rnd(tabs, r=None, o=outs, g=g5):
        arr = (C.c_void_p * 9)(*[None if t is None else t.value for t in tabs])
        return lib.zk_zerocheck_gate_round(arr, p64(r), o, p64(g))

    t4, t8 = h[0, 4], h[0, 8]
    assert lib.zk_zerocheck_gate_round(None, None, outs, p64(g5)) == L.ZK_E_ARG
    for i in range(9):
        tabs = [t4] * 9
        tabs[i] = None
        assert rnd(tabs) == L.ZK_E_ARG
        tabs[i] = h[3, 4]
        assert rnd(tabs) == L.ZK_E_ARG
        if i:
            tabs[i] = t8
            assert rnd(tabs) == L.ZK_E_LEN_MISMATCH
    assert rnd([t4] * 9, g=None) == L.ZK_E_ARG and rnd([t4] * 9, r=one, o=None) == L.ZK_E_ARG and rnd([h[1, 8]] * 9) == L.ZK_E_ARG
    assert rnd([h[0, 6]] * 9) == L.ZK_E_NOT_POW2
    assert rnd([h[0, 1]] * 9) == L.ZK_E_ARG and rnd([h[0, 2]] * 9, r=one) == L.ZK_E_ARG and rnd([t4] * 9, r=unreduced) == L.ZK_E_ARG
    import torch
    if not torch.cuda.is_available():
        assert rnd([h[0, 2]] * 9) == L.ZK_E_NO_DEVICE and rnd([t4] * 9, r=one) == L.ZK_E_NO_DEVICE
    assert (g5 == 7).all() and not any(outs)
    w = lambda n: np.full(n, 7, np.uint64)
    bufs = [w(64) for _ in range(9)]
    r8 = np.full(64 * 32, 7, np.uint8)
    prove = lambda cms: lib.zk_zerocheck_gate_prove(cms, 0, 4, 1, 0, None, p64(bufs[0]), p64(bufs[1]), p64(bufs[2]), p64(bufs[3]), p64(bufs[4]), p64(bufs[5]),
                                                    p8(r8), p64(bufs[6]), None, None, p64(bufs[7]), p8(r8), None)
    assert prove(None) == L.ZK_E_ARG and prove((C.c_void_p * 8)()) == L.ZK_E_ARG
    assert all((x == 7).all() for x in bufs) and (r8 == 7).all()
    for t in h.values():
        lib.zk_table_free(t)


def test_the_selftest_fixture_is_the_models_proof():
    import importlib.util
    path = os.path.join(G.ROOT, "tests", "golden", "make_zerocheck_gate_fixture.py")
    spec = importlib.util.spec_from_file_location("make_zerocheck_gate_fixture", path)
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    with open(mk.OUT, "rb") as fh:
        stored = fh.read()
    assert stored == mk.fixture_bytes(zk) and len(stored) < 64 << 10
    pr = mk.model_proof(zk)
    assert ZG.verify(pr, tr=ZG.pow_transcript(mk.D, mk.F, mk.G_BITS, pr["nonce"]), hasher=mk.hasher(zk)) == (True, None)
    assert lib_verify(pr, g=mk.G_BITS, nonce=pr["nonce"]) == (0, 1)
