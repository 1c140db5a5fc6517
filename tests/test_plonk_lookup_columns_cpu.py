"""CPU: the host side of the Plonk proof with lookup rows on COLUMN commitments (include/zkmle.h "Plonk with lookups on column commitments").
Everything compares byte for byte against the big-integer model of tests/_plonk_lookup_columns_model.py:

  proofs      zk_plonk_lookup_verify_columns and zk.plonk_lookup.verify_columns accept the model's proofs at d = 2 .. 5 on both fields with
              d - log_final = 2, even and odd, l among 0, 1, 3, with and without grinding bits
  rejected    one flipped bit in every array of the proof; the witness and the circuit root swapped; M's root and the helpers' swapped; a
              step-0 value moved to another column; a wrong public value and one >= p (*ok = 0, status ZK_OK); d + 1 and d - 1; a wrong nonce;
              a false gate, a false wiring and a missed lookup row, and the model's two cheating provers on them
  statuses    decided before the transcript moves; the transcript ends in the model prover's state on ZK_OK
  sizes       zk_plonk_lookup_sizes_columns equals zk_fri_ml_sizes_columns for the widths 3, 12, 1, 4 with nround = 5 d and nhroots = 2; at
              d = 24, b = 2, f = 6, Q = 64 the path bytes are 442 368; the whole proof against the proof on fifteen commitments
  helpers     on circuits without a zero denominator the model's single-denominator helper_tables equal _plonk_lookup_model.helper_tables
              entry for entry; where exactly one denominator of a pair is zero the two differ and the entry is 0; where both are, both are 0
  fixture     tests/golden/plonk_lookup_columns_proof.bin, what tools/plonk_lookup_columns_selftest.hip reads, is the model's proof and verifies

Commitments cannot exist without a device: the kernel and the prover run in tests/test_gpu_plonk_lookup_helpers.py and
tests/test_gpu_plonk_lookup_columns.py."""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest

import __graft_entry__ as G
import _fri_ml_cases as FC
import _fri_ml_columns_model as CM
import _ntt_model as NM
import _plonk_lookup_columns_model as KC
import _plonk_lookup_model as KL
from oracle import pymodel as M

zk = G.import_package()
P64, P8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
p64 = lambda a: a.ctypes.data_as(P64) if a is not None and a.size else None
p8 = lambda a: a.ctypes.data_as(P8) if a is not None else None
NEW_NAMES = ("zk_plonk_lookup_helpers", "zk_plonk_lookup_helpers_batch", "zk_plonk_lookup_sizes_columns", "zk_plonk_lookup_prove_columns",
             "zk_plonk_lookup_verify_columns", "zk_plonk_lookup_columns_last_stats")
# (field, d, b, f, coset, l, looked, bits): d = 2 .. 5 on both fields; R = d - f is 2 (one step), even and odd; l among 0, 1, 3
CASES = [(0, 2, 1, 0, False, 0, "all", 0),       # R = 2
         (3, 2, 2, 0, True, 1, "some", 4),       # R = 2
         (0, 3, 1, 0, True, 3, "some", 0),       # R = 3
         (3, 3, 2, 1, False, 0, "none", 0),      # R = 2
         (0, 4, 2, 0, True, 3, "some", 4),       # R = 4
         (3, 4, 1, 1, False, 1, "all", 0),       # R = 3
         (3, 4, 1, 2, True, 0, "some", 0),       # R = 2
         (0, 5, 1, 0, False, 1, "some", 0),      # R = 5
         (3, 5, 1, 1, True, 3, "all", 4),        # R = 4
         (0, 5, 2, 3, True, 0, "none", 0)]       # R = 2
Q = 3
case_id = lambda c: "-".join(str(v) if isinstance(v, str) else str(int(v)) for v in c)
ARRAYS = ("own_roots", "h_roots", "polys", "ys", "open_polys", "roots", "final", "values", "paths")
padded = functools.partial(FC.padded, room=16384)
coset_of = functools.partial(FC.coset_of, mul=73)


@functools.lru_cache(maxsize=None)
def hasher():
    return CM.check_host_keccak(zk)


@functools.lru_cache(maxsize=None)
def statement(field, d, b, with_coset, l, looked, false_gate=False, false_wiring=False, miss=None):
    """-> (the witness and the circuit model commitment, the public values)"""
    p = NM.MODULUS[field]
    tabs, pub = KC.circuit(field, d, 7300 + 17 * d + field + l, l, looked, false_gate=false_gate, false_wiring=false_wiring, miss=miss)
    assert KC.satisfied(tabs, pub, p) == (not false_gate, not false_wiring, miss is None)
    return KC.commitments(field, tabs, b, coset_of(field, d, b, with_coset), hasher()) + (tuple(pub),)


@functools.lru_cache(maxsize=None)
def proof(case, cheat=None, prefix=b"", **false):
    field, d, b, f, with_coset, l, looked, bits = case
    wit, cir, pub = statement(field, d, b, with_coset, l, looked, **false)
    tr = KC.pow_transcript(d, f, bits, prefix=prefix) if bits else M.Transcript()
    if not bits:
        tr.append(prefix)
    return KC.prove(wit, cir, list(pub), f, Q, tr, hasher(), cheat=cheat)


def model_verify(pr, case, prefix=b"", **kw):
    d, f, bits = case[1], case[3], case[7]
    tr = KC.pow_transcript(d, f, bits, pr["nonce"], prefix=prefix) if bits else M.Transcript()
    if not bits:
        tr.append(prefix)
    return KC.verify(pr, tr=tr, hasher=hasher(), **kw)


def lib_verify(pr, fl=None, tr=None, g=None, nonce=None, pub=None, npublic=None, case=None, **over):
    """zk_plonk_lookup_verify_columns on the model's proof `pr` (flat arrays `fl`) -> (status, ok); pub: the verifier's own public values"""
    op = pr["opening"]
    fl = KC.flat(zk, pr) if fl is None else fl
    s = {n: op[n] for n in ("d", "b", "f", "Q")}
    s.update({n: v for n, v in over.items() if n in s})
    coset = over.get("coset", op["coset"])
    cm = None if coset is None else zk.from_ints(op["field"], [coset])[0]
    pub = fl["pub"] if pub is None else pub
    npublic = pub.shape[0] if npublic is None else npublic
    g = (case[7] if case else 0) if g is None else g
    nonce = pr["nonce"] if nonce is None else nonce
    own = fl["own_roots"]
    wr, cr = (None, None) if own is None else (own.reshape(-1)[:32], own.reshape(-1)[32:])
    ok = C.c_int(-1)
    rc = zk.lib().zk_plonk_lookup_verify_columns(over.get("field", op["field"]), p8(wr), p8(cr), p64(pub), npublic, s["d"], s["b"], s["f"], s["Q"], p64(cm),
                                                 None if tr is None else tr._h, p8(fl["h_roots"]), p64(fl["polys"]), p64(fl["ys"]), p64(fl["open_polys"]),
                                                 p8(fl["roots"]), p64(fl["final"]), p64(fl["values"]), p8(fl["paths"]), g, nonce, C.byref(ok))
    return rc, ok.value


def wrapper_proof(pr, fl, g=0):
    """zk.plonk_lookup.PlonkLookupColumnsProof holding the model's arrays"""
    op = pr["opening"]
    cs = zk.from_ints(op["field"], [op["coset"]])[0]
    o = zk.plonk_lookup.PlonkLookupColumnsProof(op["field"], op["d"], op["b"], op["f"], op["Q"], coset=cs, grinding_bits=g)
    assert o.round_polys.shape == fl["polys"].shape == (op["d"], 5, 4) and o.drawn.shape == fl["drawn"].shape and o.challenges.shape == fl["challenges"].shape
    assert o.h_roots.shape == fl["h_roots"].shape == (2, 32)
    q = o.opening
    assert isinstance(q, zk.fri.FriColumnsOpening) and q.widths == [3, 12, 1, 4]
    assert q.roots.shape == fl["roots"].shape and q.query_values.shape == fl["values"].shape and q.query_paths.shape == fl["paths"].shape
    assert q.ys.shape == (20, 1, 4) and q.round_polys.shape == fl["open_polys"].shape
    o.round_polys, o.drawn, o.challenges, o.h_roots = fl["polys"], fl["drawn"], fl["challenges"], fl["h_roots"]
    q.ys, q.round_polys, q.roots, q.final_table, q.query_values, q.query_paths = fl["ys"].reshape(20, 1, 4), fl["open_polys"], fl["roots"], fl["final"], fl["values"], fl["paths"]
    q.pow_nonce = pr["nonce"]
    return o


def test_new_exports_and_the_header():
    lib = zk.lib()
    header = open(G.ROOT + "/include/zkmle.h").read()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in header, name
    assert "Plonk with lookups on column commitments" in header
    for text in ('"ZCLC"', "widths 3, 12, 1, 4", "plonk_lookup_helpers_kernel", "SINGLE-DENOMINATOR", "exactly ONE of the pair is zero", "zk_fri_ml_open_columns_pow",
                 "as a count and not a proof"):
        assert text in header, text
    for name in ("prove_columns", "verify_columns", "helpers", "helpers_batch", "sizes_columns", "columns_last_stats", "PlonkLookupColumnsProof"):
        assert hasattr(zk.plonk_lookup, name), name
    assert zk.PlonkLookupColumnsProof is zk.plonk_lookup.PlonkLookupColumnsProof
    assert 1 <= zk.plonk_lookup.helpers_batch() <= 32


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_model_proofs_pass_the_model_verifier_and_the_library_verifier(case):
    field, d, b, f, with_coset, l, looked, bits = case
    p = NM.MODULUS[field]
    pr = proof(case)
    assert model_verify(pr, case) == (True, None)
    assert pr["own_first_sum"] == 0 and pr["misses"] == 0
    alpha, tau = pr["drawn"][2], pr["drawn"][4:]
    c = alpha ** 3 * KL.public_eval(pr["pub"], tau, p) % p
    assert all((g[0] + g[1]) % p == (c if k == 0 else KC.interpolate5(pr["polys"][k - 1], pr["challenges"][k - 1], p)) for k, g in enumerate(pr["polys"]))
    assert (c != 0) == (l > 0) and pr["opening"]["points"] == [pr["challenges"][::-1]] and pr["opening"]["widths"] == [3, 12, 1, 4]
    fl = KC.flat(zk, pr)
    assert fl["pub"].shape == (l, 4) and fl["h_roots"].shape == (2, 32) and lib_verify(pr, fl, case=case) == (0, 1)
    if not with_coset:
        assert lib_verify(pr, fl, case=case, coset=None) == (0, 1)
    if bits:
        assert lib_verify(pr, fl, g=0) == (0, 0)
    got = (fl["polys"].size // 4, fl["h_roots"].shape[0], fl["roots"].shape[0], fl["final"].shape[0], fl["values"].size // 4, fl["paths"].size, fl["open_polys"].size // 4)
    assert KC.sizes(d, b, f, Q) == got == zk.plonk_lookup.sizes_columns(d, b, f, Q)
    o = wrapper_proof(pr, fl, bits)
    assert zk.plonk_lookup.verify_columns(pr["roots"][0], pr["roots"][1], fl["pub"], o)
    assert not zk.plonk_lookup.verify_columns(pr["roots"][1], pr["roots"][0], fl["pub"], o)
    assert zk.plonk_lookup.verify_columns(pr["roots"][0], pr["roots"][1], None, o) is (l == 0)
    assert np.array_equal(o.point[0], fl["points"][0]) and np.array_equal(o.ys, fl["ys"])


SPOTS = ("polys", "ys", "own_roots", "h_roots", "roots", "open_polys", "final", "values", "paths")


@pytest.mark.parametrize("name", SPOTS)
def test_one_flipped_bit_is_rejected(name):
    for case in (CASES[4], CASES[5], CASES[3]):
        pr = proof(case)
        base = KC.flat(zk, pr)
        rng = random.Random(47 * len(name) + case[1])
        flat_size = base[name].size
        spots = {0, flat_size - 1} | {rng.randrange(flat_size) for _ in range(6)}
        if name in ("h_roots", "own_roots"):                  # each of the two roots
            spots |= {32 * j + rng.randrange(32) for j in range(2)}
        for at in sorted(spots):
            fl = {n: v.copy() for n, v in base.items()}
            view = fl[name].reshape(-1)
            view[at] ^= view.dtype.type(1 << rng.randrange(8 if view.dtype == np.uint8 else 64))
            assert lib_verify(pr, fl, case=case) == (0, 0), (case, name, at)


def test_swapped_roots_moved_values_and_another_d_are_rejected():
    for case in (CASES[4], CASES[5]):
        pr = proof(case)
        base = KC.flat(zk, pr)
        K = 20
        # the witness root and the circuit root
        sw = {n: v.copy() for n, v in base.items()}
        sw["own_roots"][[0, 1]] = sw["own_roots"][[1, 0]]
        assert lib_verify(pr, sw, case=case) == (0, 0)
        sw["roots"][[0, 1]] = sw["roots"][[1, 0]]             # ... and the proof's copy with them
        assert lib_verify(pr, sw, case=case) == (0, 0)
        assert model_verify(pr, case, roots=pr["roots"][::-1])[0] is False
        # M's root and the helpers'
        sw = {n: v.copy() for n, v in base.items()}
        sw["h_roots"][[0, 1]] = sw["h_roots"][[1, 0]]
        assert lib_verify(pr, sw, case=case) == (0, 0)
        sw["roots"][[2, 3]] = sw["roots"][[3, 2]]
        assert lib_verify(pr, sw, case=case) == (0, 0)
        # a step-0 value moved to another column: inside one commitment, and across two
        per = base["values"].shape[1]
        assert base["values"].shape == (Q, per, 4) and per >= 4 * K
        for a, b_ in ((0, 1), (3, 14), (2, 3), (15, 16), (16, 19)):
            for q in (0, Q - 1):
                mv = {n: v.copy() for n, v in base.items()}
                if np.array_equal(mv["values"][q, 4 * a], mv["values"][q, 4 * b_]):
                    continue
                mv["values"][q, [4 * a, 4 * b_]] = mv["values"][q, [4 * b_, 4 * a]]
                assert lib_verify(pr, mv, case=case) == (0, 0), (a, b_, q)
        # two claims swapped
        mv = {n: v.copy() for n, v in base.items()}
        mv["ys"][[0, 1]] = mv["ys"][[1, 0]]
        assert lib_verify(pr, mv, case=case) == (0, 0)
        big = padded(base)
        d, f = case[1], case[3]
        assert lib_verify(pr, big, pub=base["pub"], case=case) == (0, 1)
        assert lib_verify(pr, big, pub=base["pub"], case=case, d=d + 1) == (0, 0) and lib_verify(pr, big, pub=base["pub"], case=case, d=d - 1) == (0, 0)
        assert lib_verify(pr, big, pub=base["pub"], case=case, f=f + 1) == (0, 0) and lib_verify(pr, big, pub=base["pub"], case=case, Q=Q + 1) == (0, 0)
        assert lib_verify(pr, big, pub=base["pub"], case=case, b=case[2] + 1) == (0, 0)


def test_the_public_values_are_part_of_the_statement():
    for case in (CASES[2], CASES[4], CASES[5]):
        field, d, l = case[0], case[1], case[5]
        p, rng = NM.MODULUS[field], random.Random(d + l)
        pr = proof(case)
        fl = KC.flat(zk, pr)
        for x in sorted({0, l - 1, rng.randrange(l)}):        # one public value changed
            wrong = list(pr["pub"])
            wrong[x] = (wrong[x] + 1) % p
            assert lib_verify(pr, fl, pub=KC.mont(zk, field, wrong), case=case) == (0, 0), (case, x)
            assert model_verify(pr, case, pub=wrong)[0] is False
        room = np.concatenate([fl["pub"], np.zeros((1, 4), np.uint64)])
        assert lib_verify(pr, fl, pub=room, npublic=l, case=case) == (0, 1)
        assert lib_verify(pr, fl, pub=room, npublic=l - 1, case=case) == (0, 0)
        assert lib_verify(pr, fl, pub=room, npublic=l + 1, case=case) == (0, 0)
        big = fl["pub"].copy()                                # a public value >= p: not a status
        big[l - 1] = np.uint64(0xFFFFFFFFFFFFFFFF)
        assert lib_verify(pr, fl, pub=big, case=case) == (0, 0)
        big[l - 1] = np.frombuffer(p.to_bytes(32, "little"), np.uint64)
        assert lib_verify(pr, fl, pub=big, case=case) == (0, 0)
        assert model_verify(pr, case, pub=pr["pub"][:-1] + [p + pr["pub"][-1]])[0] is False


def test_statuses_come_before_the_transcript_is_touched():
    from zkmle_amd import _lib as L
    case = CASES[5]                                           # BN254 Fr, d = 4, b = 1, f = 1, no coset, l = 1
    pr = proof(case)
    fl = KC.flat(zk, pr)
    t = zk.Transcript()
    t.append(b"the caller's own")
    before = t.export_state().copy()
    for name in ARRAYS:
        class Without(dict):
            def __getitem__(self, key, name=name):
                return None if key == name else dict.__getitem__(self, key)
        assert lib_verify(pr, Without(fl), t, pub=fl["pub"])[0] == L.ZK_E_ARG, name
    lib = zk.lib()
    own = fl["own_roots"].reshape(-1)
    assert lib.zk_plonk_lookup_verify_columns(3, p8(own[:32]), p8(own[32:]), p64(fl["pub"]), 1, 4, 1, 1, Q, None, t._h, p8(fl["h_roots"]), p64(fl["polys"]), p64(fl["ys"]),
                                              p64(fl["open_polys"]), p8(fl["roots"]), p64(fl["final"]), p64(fl["values"]), p8(fl["paths"]), 0, 0, None) == L.ZK_E_ARG
    big = padded(fl)
    for over, want in ((dict(field=7), L.ZK_E_ARG), (dict(field=-1), L.ZK_E_ARG), (dict(field=1, coset=None), L.ZK_E_RANGE), (dict(field=2, coset=None), L.ZK_E_RANGE),
                       (dict(coset=0), L.ZK_E_ARG), (dict(d=NM.two_adicity(3) - 1, b=2), L.ZK_E_RANGE), (dict(d=31, b=2), L.ZK_E_RANGE), (dict(d=32, b=1), L.ZK_E_ARG),
                       (dict(d=40, b=1), L.ZK_E_ARG), (dict(d=0), L.ZK_E_ARG), (dict(f=4), L.ZK_E_ARG), (dict(f=3), L.ZK_E_ARG), (dict(b=0), L.ZK_E_ARG),
                       (dict(b=9), L.ZK_E_ARG), (dict(Q=0), L.ZK_E_ARG), (dict(Q=4097), L.ZK_E_ARG)):
        assert lib_verify(pr, big, t, pub=fl["pub"], **over) == (want, -1), over
    assert lib_verify(pr, big, t, pub=fl["pub"], g=33)[0] == L.ZK_E_ARG
    assert lib_verify(pr, big, t, pub=np.zeros((17, 4), np.uint64)) == (L.ZK_E_ARG, -1)
    assert lib_verify(pr, big, t, pub=np.zeros((0, 4), np.uint64), npublic=1) == (L.ZK_E_ARG, -1)
    assert np.array_equal(t.export_state(), before)
    assert lib_verify(pr, fl, t) == (0, 0) and not np.array_equal(t.export_state(), before)   # bound to a fresh transcript; ZK_OK moves it


@pytest.mark.parametrize("field", (0, 3))
@pytest.mark.parametrize("d", (2, 3, 4))
def test_false_statements_and_the_cheating_provers_are_rejected(field, d):
    l = (0, 3, 1)[d - 2]
    case = (field, d, 1, 0, d % 2 == 0, l, ("all", "none", "some")[d - 2], 0)
    x = (1 << d) - 1
    for false, cheat in ((dict(false_gate=True), "wiring"), (dict(false_wiring=True), "wiring"), (dict(miss=x), "lookup")):
        pr = proof(case, **false)
        assert model_verify(pr, case) == (False, 0), false
        assert pr["own_first_sum"] != 0 and lib_verify(pr) == (0, 0), false
        assert (pr["misses"] >= 1) if "miss" in false else pr["misses"] == 0
        ch = proof(case, cheat, **false)
        ok, failed = model_verify(ch, case)
        assert not ok and 1 <= failed <= d, false             # a later round's sum, or the last claim: never the opening, which is honest
        assert lib_verify(ch) == (0, 0), false
    ch = proof(case, "lookup")                                # on a true statement the lookup's cheat changes nothing
    assert lib_verify(ch) == (0, 1) and ch["polys"] == proof(case)["polys"]


def test_the_proof_of_work_nonce():
    for case in (CASES[1], CASES[4], CASES[8]):
        bits = case[7]
        pr = proof(case)
        w = pr["nonce"]
        fl = KC.flat(zk, pr)
        assert lib_verify(pr, fl, g=bits, nonce=w) == (0, 1)
        assert lib_verify(pr, fl, g=bits, nonce=w + 1) == (0, 0) and lib_verify(pr, fl, g=bits, nonce=(w - 1) % (1 << 64)) == (0, 0)
        assert lib_verify(pr, fl, g=bits + 1, nonce=w) == (0, 0) and lib_verify(pr, fl, g=0, nonce=w) == (0, 0)
        d, f = case[1], case[3]
        assert KC.verify(pr, tr=KC.pow_transcript(d, f, bits, w + 1), hasher=hasher())[0] is False
        plain = proof(case[:7] + (0,))
        assert lib_verify(plain, g=bits, nonce=w) == (0, 0)   # indices drawn without the step
        o = wrapper_proof(pr, fl, bits)
        assert zk.plonk_lookup.verify_columns(pr["roots"][0], pr["roots"][1], fl["pub"], o)
        o.opening.pow_nonce = w + 1
        assert not zk.plonk_lookup.verify_columns(pr["roots"][0], pr["roots"][1], fl["pub"], o)


@pytest.mark.parametrize("case", (CASES[2], CASES[8]), ids=case_id)
def test_a_callers_transcript(case):
    prior = b"what the caller had absorbed before"
    pr = proof(case, prefix=prior)
    assert model_verify(pr, case, prefix=prior) == (True, None)
    field, d, b, f, with_coset, l, looked, bits = case
    wit, cir, pub = statement(field, d, b, with_coset, l, looked)
    mt = KC.pow_transcript(d, f, bits, pr["nonce"], prefix=prior) if bits else M.Transcript()
    if not bits:
        mt.append(prior)
    again = KC.prove(wit, cir, list(pub), f, Q, mt, hasher())
    assert again["polys"] == pr["polys"] and again["opening"]["indices"] == pr["opening"]["indices"]
    t, want = zk.Transcript(), zk.Transcript()
    t.append(prior)
    assert lib_verify(pr, tr=t, case=case) == (0, 1)
    want.append(bytes(mt.buf))
    assert np.array_equal(t.export_state(), want.export_state())   # the verifier's transcript ends in the model prover's state
    assert lib_verify(pr, case=case) == (0, 0)                # the proof is bound to the prior content
    t2 = zk.Transcript()
    t2.append(prior + b"!")
    assert lib_verify(pr, tr=t2, case=case) == (0, 0)


def test_sizes_and_the_count_against_fifteen_commitments():
    from zkmle_amd import _lib as L
    lib = zk.lib()

    def sizes(d, b, f, q):
        out = [C.c_size_t(0) for _ in range(7)]
        rc = lib.zk_plonk_lookup_sizes_columns(d, b, f, q, *[C.byref(o) for o in out])
        return rc, tuple(int(o.value) for o in out)

    for d in (2, 3, 4, 6, 10, 24):
        for b in (1, 2):
            for f in range(0, d):
                for q in (1, 8, 64):
                    if d - f < 2:
                        assert sizes(d, b, f, q)[0] == L.ZK_E_ARG
                        continue
                    want = (5 * d, 2) + zk.fri.columns_sizes((3, 12, 1, 4), d, b, f, q)
                    assert sizes(d, b, f, q) == (0, want) and KC.sizes(d, b, f, q) == want and zk.plonk_lookup.sizes_columns(d, b, f, q) == want
    for d, b, f, q in ((0, 1, 0, 4), (1, 1, 0, 4), (3, 0, 0, 4), (3, 1, 3, 4), (3, 1, 2, 4), (3, 1, 0, 0), (32, 1, 0, 4), (40, 1, 0, 4), (0xFFFFFFFF, 1, 0, 4)):
        assert sizes(d, b, f, q)[0] == L.ZK_E_ARG, (d, b, f, q)
    assert sizes(31, 2, 0, 8)[0] == L.ZK_E_RANGE
    assert lib.zk_plonk_lookup_sizes_columns(4, 1, 0, 8, None, None, None, None, None, None, None) == 0
    assert sizes(24, 2, 6, 64)[1][5] == 442368                # the path bytes at d = 24, b = 2, f = 6, Q = 64

    # the proof's bytes: 32 per element and per root, the paths as they are, the twenty claims; against the proof on fifteen grouped commitments
    def total(s):
        nround, nh, nroots, nfinal, nvalues, pbytes, nopen = s
        return 32 * (nround + nh + nroots + nfinal + nvalues + nopen + 20) + pbytes

    for d in (20, 24):
        cols, fifteen = zk.plonk_lookup.sizes_columns(d, 2, 6, 64), zk.plonk_lookup.sizes(d, 2, 6, 64, 2, True)
        assert cols[4] == fifteen[4] and cols[3] == fifteen[3] and cols[6] == fifteen[6] and cols[0] == fifteen[0]   # the same values, final table and rounds
        assert fifteen[5] - cols[5] == 16 * 64 * (d + 2 - 2) * 32          # sixteen step-0 paths a query fewer
        assert total(fifteen) - total(cols) == 16 * 64 * d * 32 + 32 * (3 + 16)   # and 3 helper roots and 16 of the opening's roots
    assert zk.plonk_lookup.sizes(24, 2, 6, 64, 2, True)[5] == 1228800


def compare_definitions(tabs, beta, gamma, p, m):
    """the two definitions on the fifteen tables: an entry differs exactly where ONE denominator of its pair is zero, and is 0 there in the
    single-denominator form -> (the old tables, the new ones, the number of entries that differ)"""
    n = len(tabs[0])
    o, w = KL.helper_tables(tabs, beta, gamma, p, m), KC.helper_tables(tabs, beta, gamma, p, m)
    assert o[0] == w[0] == m
    differ = 0
    for y in range(n):
        pairs = [((beta + tabs[j][y] + gamma * (j * n + y)) % p, (beta + tabs[j][y] + gamma * tabs[8 + j][y]) % p) for j in range(3)]
        pairs.append(((beta + tabs[0][y] + gamma * tabs[1][y] + gamma * gamma * tabs[2][y]) % p, (beta + tabs[12][y] + gamma * tabs[13][y] + gamma * gamma * tabs[14][y]) % p))
        for j, (a, b) in enumerate(pairs):
            one_zero = (a == 0) != (b == 0)
            if a == 0 or b == 0:
                assert w[1 + j][y] == 0
            if a == 0 and b == 0:
                assert o[1 + j][y] == 0
            # with one zero the old entry is the other denominator's fraction: not 0 unless its multiplier (qK or M) is
            assert o[1 + j][y] == w[1 + j][y] or one_zero, (j, y)
            differ += o[1 + j][y] != w[1 + j][y]
    return o, w, differ


@pytest.mark.parametrize("field", (0, 3))
def test_the_two_definitions_of_the_helper_tables(field):
    p, rng = NM.MODULUS[field], random.Random(91 + field)
    for d in (2, 3, 5):
        n = 1 << d
        tabs, pub = KC.circuit(field, d, 555 + d + field, 1, "some")
        beta, gamma = rng.randrange(p), rng.randrange(1, p)
        m = KL.helper_tables(tabs, beta, gamma, p)[0]
        assert compare_definitions(tabs, beta, gamma, p, m)[2] == 0   # no denominator is zero: entry for entry
        assert KL.helper_tables(tabs, beta, gamma, p) == KC.helper_tables(tabs, beta, gamma, p)
        x = rng.randrange(n)
        # exactly one of a pair is zero: Did_0 at row x (cells wired to it hold its value: their Dsig is zero, alone, too)
        b1 = (-tabs[0][x] - gamma * x) % p
        if tabs[8][x] != x:
            o, w, differ = compare_definitions(tabs, b1, gamma, p, m)
            assert w[1][x] == 0 and o[1][x] != 0 and differ >= 1
        # both are zero: S = id at that row
        t2 = [list(t) for t in tabs]
        t2[8][x] = x
        o, w, _ = compare_definitions(t2, b1, gamma, p, m)
        assert o[1][x] == w[1][x] == 0
        # Dw only: beta = -(A + gamma B + gamma^2 C)[x]
        b3 = (-tabs[0][x] - gamma * tabs[1][x] - gamma * gamma * tabs[2][x]) % p
        o, w, _ = compare_definitions(tabs, b3, gamma, p, m)
        dt = (b3 + tabs[12][x] + gamma * tabs[13][x] + gamma * gamma * tabs[14][x]) % p
        assert w[4][x] == 0 and (dt == 0 or o[4][x] == (-m[x] * pow(dt, -1, p)) % p)


def test_prover_and_hook_statuses_without_a_device():
    from zkmle_amd import _lib as L
    lib = zk.lib()
    h = {}
    for field, n in ((0, 1), (0, 2), (0, 4), (0, 8), (0, 6), (1, 8), (3, 4)):
        h[field, n] = C.c_void_p()
        L.check(lib.zk_table_wrap(field, C.c_void_p(0x1000), n, C.byref(h[field, n])))
    one = zk.from_ints(0, [1])[0]
    unreduced = np.full(4, 0xFFFFFFFFFFFFFFFF, np.uint64)
    outs = (C.c_void_p * 4)()

    def run(tabs, beta=one, gamma=one, o=outs):
        arr = (C.c_void_p * 11)(*[None if t is None else t.value for t in tabs])
        return lib.zk_plonk_lookup_helpers(arr, p64(beta), p64(gamma), o)

    t4, t8 = h[0, 4], h[0, 8]
    assert lib.zk_plonk_lookup_helpers(None, p64(one), p64(one), outs) == L.ZK_E_ARG
    for i in range(11):
        tabs = [t4] * 11
        tabs[i] = None
        assert run(tabs) == L.ZK_E_ARG
        tabs[i] = h[3, 4]
        assert run(tabs) == L.ZK_E_ARG                        # mixed fields
        if i:
            tabs[i] = t8
            assert run(tabs) == L.ZK_E_LEN_MISMATCH           # mixed lengths
    assert run([t4] * 11, beta=None) == L.ZK_E_ARG and run([t4] * 11, gamma=None) == L.ZK_E_ARG and run([t4] * 11, o=None) == L.ZK_E_ARG
    assert run([t4] * 11, beta=unreduced) == L.ZK_E_ARG and run([t4] * 11, gamma=unreduced) == L.ZK_E_ARG
    assert run([h[1, 8]] * 11) == L.ZK_E_ARG and run([h[0, 6]] * 11) == L.ZK_E_NOT_POW2 and run([h[0, 1]] * 11) == L.ZK_E_ARG
    arr = (C.c_void_p * 11)(*[t4.value] * 11)                 # the four handles inside the array that is read
    for at in (0, 4, 7, 10):
        alias = C.cast(C.byref(arr, 8 * at), C.POINTER(C.c_void_p))
        assert lib.zk_plonk_lookup_helpers(arr, p64(one), p64(one), alias) == L.ZK_E_ARG
    assert all(v == t4.value for v in arr)
    import torch
    if not torch.cuda.is_available():
        assert run([t4] * 11) == L.ZK_E_NO_DEVICE
    assert not any(outs)
    w = lambda n: np.full(n, 7, np.uint64)
    bufs = [w(128) for _ in range(9)]
    r8, hr = np.full(64 * 32, 7, np.uint8), np.full(64, 7, np.uint8)
    prove = lambda a, b: lib.zk_plonk_lookup_prove_columns(a, b, None, 0, 0, 4, 0, None, p8(hr), p64(bufs[0]), p64(bufs[1]), p64(bufs[2]), p64(bufs[3]), p64(bufs[4]),
                                                          p64(bufs[5]), p8(r8), p64(bufs[6]), None, None, p64(bufs[7]), p8(r8), None)
    assert prove(None, None) == L.ZK_E_ARG
    assert all((x == 7).all() for x in bufs) and (r8 == 7).all() and (hr == 7).all()
    assert lib.zk_plonk_lookup_columns_last_stats(None) == L.ZK_E_ARG
    for t in h.values():
        lib.zk_table_free(t)


def test_the_selftest_fixture_is_the_models_proof():
    import importlib.util
    path = os.path.join(G.ROOT, "tests", "golden", "make_plonk_lookup_columns_fixture.py")
    spec = importlib.util.spec_from_file_location("make_plonk_lookup_columns_fixture", path)
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    with open(mk.OUT, "rb") as fh:
        stored = fh.read()
    assert stored == mk.fixture_bytes(zk) and len(stored) < 16 << 10
    assert (mk.FIELD, mk.D, mk.L_PUBLIC, mk.G_BITS) == (3, 4, 1, 4) and mk.COSET != 1
    pr = mk.model_proof(zk)
    assert len(pr["pub"]) == 1 and pr["opening"]["widths"] == [3, 12, 1, 4]
    assert KC.verify(pr, tr=KC.pow_transcript(mk.D, mk.F, mk.G_BITS, pr["nonce"]), hasher=mk.hasher(zk)) == (True, None)
    assert lib_verify(pr, g=mk.G_BITS, nonce=pr["nonce"]) == (0, 1)
