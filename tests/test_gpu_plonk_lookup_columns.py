"""GPU: the Plonk proof with lookup rows on COLUMN commitments (csrc/plonk_helpers.cuh, csrc/zkmle_plonk_lookup_columns.hip; include/zkmle.h
"Plonk with lookups on column commitments"), over BLS12-381 Fr and BN254 Fr.  Everything is byte for byte against
tests/_plonk_lookup_columns_model.py; no tolerance anywhere.

  prove      every output array equals the model's at d = 2 .. 6 on both fields with d - log_final = 2, even and odd, l among 0, 1, 3, grinding
             bits 0 and 6, with and without a coset, and on a caller's transcript with a prefix; the host verifier accepts it and rejects it
             with the two roots swapped; the two input commitments' tables and roots are what they were; a second proof is identical
  helpers    the proof's two helper roots are those of fri.commit_columns on the multiplicities hook's table and on the helpers hook's four
  misses     on a circuit with missed rows the stats' `misses` equals the model's count and the proof is rejected; a false gate and a false
             wiring are proved with ZK_OK and rejected
  refusals   widths other than 3 and 12, commitments of different shape, d - log_final < 2, grinding_bits = 33, the public inputs' shape and an
             unreduced public value: ZK_E_ARG, nothing written, the transcript as it was; d > 31 by the size function"""
import ctypes as C

import numpy as np
import pytest

import _fri_ml_cases as FC
import _fri_ml_columns_model as CM
import _ntt_model as NM
import _plonk_lookup_columns_model as KC
from oracle import pymodel as M
from test_gpu_fri import table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
Q = 5
PREFIX = b"before the circuit"


def hasher(zk):
    return CM.check_host_keccak(zk)


def elem(zk, field, v):
    return zk.from_ints(field, [v])[0]


def gpu_commitments(zk, field, tabs, b, coset):
    cs = None if coset == 1 else elem(zk, field, coset)
    dev = [table_of(zk, field, t) for t in tabs]
    return zk.fri.commit_columns(dev[:3], b, cs), zk.fri.commit_columns(dev[3:], b, cs)


def root_now(zk, cm):
    from zkmle_amd import _lib as L
    root = np.zeros(32, np.uint8)
    L.check(zk.lib().zk_fri_columns_root(cm._h, L.p8(root)))
    return root.tobytes()


def transcripts(d, f, bits, prefix, nonce=None):
    tr = KC.pow_transcript(d, f, bits, nonce, prefix=prefix) if bits else M.Transcript()
    if not bits:
        tr.append(prefix)
    return tr


def assert_same_proof(zk, got, pr):
    fl = KC.flat(zk, pr)
    op = got.opening
    for name, arr in (("h_roots", got.h_roots), ("drawn", got.drawn), ("polys", got.round_polys), ("challenges", got.challenges), ("ys", got.ys), ("gamma", op.gamma),
                      ("open_polys", op.round_polys), ("roots", op.roots), ("final", op.final_table), ("open_challenges", op.challenges),
                      ("indices", op.query_indices), ("values", op.query_values), ("paths", op.query_paths)):
        assert arr.shape == fl[name].shape and np.array_equal(arr, fl[name]), name
    assert op.pow_nonce == pr["nonce"]
    assert np.array_equal(got.point[0], fl["points"][0])
    return fl


def prove_case(zk, field, d, b, f, with_coset, l, looked="some", bits=0, prefix=b"", check_helpers=False, **false):
    p = NM.MODULUS[field]
    coset = FC.coset_of(field, d, b, with_coset, 79)
    tabs, pub = KC.circuit(field, d, 21000 + 29 * d + field + l, l, looked, **false)
    assert KC.satisfied(tabs, pub, p) == (not false.get("false_gate"), not false.get("false_wiring"), false.get("miss") is None)
    wit, cir = KC.commitments(field, tabs, b, coset, hasher(zk))
    pr = KC.prove(wit, cir, pub, f, Q, transcripts(d, f, bits, prefix), hasher(zk))
    honest = not false
    assert KC.verify(pr, tr=transcripts(d, f, bits, prefix, pr["nonce"]), hasher=hasher(zk))[0] is honest
    gw, gc = gpu_commitments(zk, field, tabs, b, coset)
    pm = to_mont(zk, field, pub) if l else None
    try:
        assert gw.root == wit["root"] and gc.root == cir["root"] and (gw.k, gc.k) == (3, 12)
        before = [gw.table(j).evaluated_values for j in range(3)] + [gc.table(j).evaluated_values for j in range(12)]
        words = [gw.codeword(j).evaluated_values for j in range(3)] + [gc.codeword(j).evaluated_values for j in range(12)]
        t = v = None
        if prefix:
            t, v = zk.Transcript(), zk.Transcript()
            t.append(prefix)
            v.append(prefix)
        got = zk.plonk_lookup.prove_columns(gw, gc, pm, f, Q, transcript=t, grinding_bits=bits)
        assert isinstance(got, zk.plonk_lookup.PlonkLookupColumnsProof) and isinstance(got.opening, zk.fri.FriColumnsOpening) and got.round_polys.shape == (d, 5, 4)
        assert_same_proof(zk, got, pr)
        st = zk.plonk_lookup.columns_last_stats()
        assert st["rounds"] == d and st["ms_total"] > 0 and st["misses"] == pr["misses"] and (pr["misses"] >= 1) == ("miss" in false)
        assert zk.plonk_lookup.verify_columns(gw.root, gc.root, pm, got, transcript=v) is honest
        if prefix:
            want = zk.Transcript()
            want.append(prefix)
            assert zk.plonk_lookup.verify_columns(gw.root, gc.root, pm, got, transcript=want) is honest
            assert np.array_equal(t.export_state(), v.export_state()) and np.array_equal(t.export_state(), want.export_state())
            assert not zk.plonk_lookup.verify_columns(gw.root, gc.root, pm, got)       # bound to the prior content
        sv = None
        if prefix:
            sv = zk.Transcript()
            sv.append(prefix)
        assert not zk.plonk_lookup.verify_columns(gc.root, gw.root, pm, got, transcript=sv)   # the two roots the other way round
        # the two commitments were only read: tables, codewords and roots are what they were
        after = [gw.table(j).evaluated_values for j in range(3)] + [gc.table(j).evaluated_values for j in range(12)]
        assert all(np.array_equal(a, c) for a, c in zip(before, after)) and all(np.array_equal(a, to_mont(zk, field, t)) for a, t in zip(after, tabs))
        after = [gw.codeword(j).evaluated_values for j in range(3)] + [gc.codeword(j).evaluated_values for j in range(12)]
        assert all(np.array_equal(a, c) for a, c in zip(words, after))
        assert root_now(zk, gw) == wit["root"] and root_now(zk, gc) == cir["root"]
        if check_helpers:                                     # the two helper roots from the hooks on their own
            dev = [table_of(zk, field, x) for x in tabs]
            m, misses = zk.lookup.multiplicities([dev[j] for j in (0, 1, 2, 11, 12, 13, 14)])
            hs = zk.plonk_lookup.helpers([dev[j] for j in (0, 1, 2, 8, 9, 10, 11, 12, 13, 14)] + [m], got.drawn[0], got.drawn[1])
            cs = None if coset == 1 else elem(zk, field, coset)
            for j, cols in enumerate(([m], list(hs))):
                c = zk.fri.commit_columns(cols, b, cs)
                try:
                    assert c.root == got.h_roots[j].tobytes(), j
                finally:
                    c.free()
            assert misses == pr["misses"]
            again = zk.plonk_lookup.prove_columns(gw, gc, pm, f, Q, grinding_bits=bits) if not prefix else None
            if again is not None:
                assert_same_proof(zk, again, pr)
    finally:
        gw.free()
        gc.free()


# d = 2 .. 6: R = d - f is 2 (one step), even and odd; both fields; l among 0, 1, 3; grinding 0 and 6; with and without a coset; a prefix
GRID = [(0, 2, 1, 0, False, 0, "all", 0, b""),        # R = 2
        (3, 2, 2, 0, True, 1, "some", 6, b""),        # R = 2
        (3, 3, 1, 0, False, 3, "some", 0, PREFIX),    # R = 3
        (0, 3, 2, 1, True, 0, "none", 0, b""),        # R = 2
        (0, 4, 1, 0, True, 1, "some", 6, PREFIX),     # R = 4
        (3, 4, 1, 1, False, 3, "all", 0, b""),        # R = 3
        (3, 5, 2, 0, True, 3, "some", 0, b""),        # R = 5
        (0, 5, 1, 3, False, 1, "all", 6, b""),        # R = 2
        (0, 6, 1, 0, False, 3, "some", 0, b""),       # R = 6
        (3, 6, 2, 1, True, 0, "some", 6, PREFIX),     # R = 5
        (3, 6, 1, 2, False, 1, "none", 0, b"")]       # R = 4
grid_id = lambda c: "f%d-d%d-b%d-f%d-c%d-l%d-%s-g%d-%s" % (c[:8] + ("prefix" if c[8] else "fresh",))


@pytest.mark.parametrize("case", GRID, ids=grid_id)
def test_prove_equals_the_model(zk, case):
    field, d, b, f, with_coset, l, looked, bits, prefix = case
    prove_case(zk, field, d, b, f, with_coset, l, looked, bits, prefix, check_helpers=d in (4, 6))


@pytest.mark.parametrize("field", (0, 3))
def test_false_statements_are_proved_and_not_verified(zk, field):
    d = 5
    for false in (dict(miss=7), dict(miss=(1 << d) - 1), dict(false_gate=True), dict(false_wiring=True)):
        prove_case(zk, field, d, 1, 1, field == 3, 3, "some", **false)


def test_refusals_write_nothing(zk):
    from zkmle_amd import _lib as L
    lib = zk.lib()
    nq = 8
    rnd = lambda field, d, seed: zk.MultilinearPolynomial.random(field, 1 << d, seed)
    mk = lambda field, d, b, coset, k, seed: zk.fri.commit_columns([rnd(field, d, seed + j) for j in range(k)], b, coset)
    wit, cir = mk(3, 4, 1, None, 3, 100), mk(3, 4, 1, None, 12, 200)
    others = {"witness of two": (mk(3, 4, 1, None, 2, 300), cir), "witness of four": (mk(3, 4, 1, None, 4, 310), cir), "circuit of eleven": (wit, mk(3, 4, 1, None, 11, 320)),
              "circuit of thirteen": (wit, mk(3, 4, 1, None, 13, 330)), "the two the other way round": (cir, wit), "another d": (wit, mk(3, 5, 1, None, 12, 340)),
              "another blow-up": (mk(3, 4, 2, None, 3, 350), cir), "another field": (wit, mk(0, 4, 1, None, 12, 360)),
              "another coset": (wit, mk(3, 4, 1, elem(zk, 3, 5), 12, 370))}
    FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
    w = lambda n: np.full(n, FILL, np.uint64)
    by = lambda n: np.full(n, 0xA5, np.uint8)
    hr, drawn, polys, chal, ys, gamma, opolys, roots, fin, ochal, idx, vals, paths = (by(64), w(4 * 9), w(20 * 5), w(4 * 5), w(80), w(4), w(12 * 5), by(32 * 16), w(4 << 5),
                                                                                       w(4 * 5), w(nq), w(4 * nq * 100), by(32 * nq * 64))
    outs = (hr, drawn, polys, chal, ys, gamma, opolys, roots, fin, ochal, idx, vals, paths)
    nonce = C.c_uint64(0xA5)
    t = zk.Transcript()
    t.append(b"untouched")
    before = t.export_state().copy()
    good_pub = zk.from_ints(3, [5, 6, 7])

    def raw(a, b, f=0, g=0, pub=good_pub, l=None, q=nq):
        l = (0 if pub is None else pub.shape[0]) if l is None else l
        return lib.zk_plonk_lookup_prove_columns(None if a is None else a._h, None if b is None else b._h, None if pub is None else L.p64(pub), l, f, q, g, t._h, L.p8(hr),
                                                 L.p64(drawn), L.p64(polys), L.p64(chal), L.p64(ys), L.p64(gamma), L.p64(opolys), L.p8(roots), L.p64(fin), L.p64(ochal),
                                                 L.p64(idx), L.p64(vals), L.p8(paths), C.byref(nonce))

    def refused(a, b, what, **kw):
        assert raw(a, b, **kw) == L.ZK_E_ARG, what
        assert all((o == (FILL if o.dtype == np.uint64 else 0xA5)).all() for o in outs) and nonce.value == 0xA5, what
        assert np.array_equal(t.export_state(), before), what

    try:
        for what, (a, b) in others.items():
            refused(a, b, what)
        refused(None, cir, "no witness")
        refused(wit, None, "no circuit")
        for kw in (dict(f=3), dict(f=4), dict(g=33), dict(q=0), dict(q=4097)):
            refused(wit, cir, kw, **kw)                       # d - log_final < 2, and the opener's own
        refused(wit, cir, "npublic > 2^d", pub=zk.from_ints(3, list(range(17))))
        refused(wit, cir, "no array with npublic > 0", pub=None, l=1)
        unreduced = good_pub.copy()
        unreduced[1] = np.uint64(0xFFFFFFFFFFFFFFFF)
        refused(wit, cir, "an unreduced public value", pub=unreduced)
        # d > 31 cannot be committed: by the size function
        sizes = lambda d, b, f: lib.zk_plonk_lookup_sizes_columns(d, b, f, nq, None, None, None, None, None, None, None)
        assert sizes(32, 1, 0) == L.ZK_E_ARG and sizes(33, 1, 6) == L.ZK_E_ARG and sizes(4, 1, 3) == L.ZK_E_ARG and sizes(4, 1, 2) == 0
        # what was refused in one company is still good for a proof in another (of a false statement: the tables are random)
        got = zk.plonk_lookup.prove_columns(wit, cir, good_pub, 2, nq)
        assert not zk.plonk_lookup.verify_columns(wit.root, cir.root, good_pub, got)
    finally:
        for a, b in list(others.values()) + [(wit, cir)]:
            a.free()
            b.free()
