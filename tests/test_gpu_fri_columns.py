"""GPU: the commitment to several tables under one Merkle tree and the multilinear opening of several such commitments together
(csrc/merkle_columns.cuh, csrc/zkmle_fri_pcs.hip zk_fri_commit_columns, csrc/zkmle_fri_ml.hip zk_fri_ml_open_columns_pow; include/zkmle.h "Column
commitments opened together"), over BLS12-381 Fr and BN254 Fr.  Everything is byte for byte against tests/_fri_ml_columns_model.py; no
tolerance anywhere.

  commitment  the root against the model for k = 1, 2, 3, 17 and 32; at k = 1 the root of zk_fri_commit_grouped(.., 2); the codeword accessor
              equals zk_uni_low_degree_extend of the table accessor, which equals the input; the input tables are only read; the statistics
  opening     zk_fri_ml_open_columns_pow equals the model in every output array for the widths [1], [3], [2, 1], [17] and [11, 3, 1, 4] at
              d = 3 .. 8 and d = 12, on both fields, P among 1, 2, 8, R = 2, even and odd, with and without a coset, on a caller's transcript
              that is left in the verifier's end state; twice with 8 bits of proof of work; every proof passes zk_fri_ml_verify_columns_pow,
              and fails it with the roots rotated or a claim changed
  refusals    mixed d, blow-up, coset or field, K > 32, R < 2, NULL: ZK_E_ARG, nothing written, the transcript untouched"""
import ctypes as C

import numpy as np
import pytest

import _fri_ml_cases as FC
import _fri_ml_columns_model as CM
import _ntt_model as NM
from test_fri_columns_cpu import hasher, pow_transcript
from test_gpu_fri import table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
Q = 6
FIELDS = (0, 3)
WIDTHS = ((1,), (3,), (2, 1), (17,), (11, 3, 1, 4))


def elem(zk, field, v):
    return zk.from_ints(field, [v])[0]


def model_commitments(field, d, b, coset, widths, seed):
    return [CM.commit(field, [NM.random_ints(field, 1 << d, seed + 101 * j + 7 * c) for c in range(w)], b, coset, hasher()) for j, w in enumerate(widths)]


def gpu_commitment(zk, cm):
    cs = None if cm["coset"] == 1 else elem(zk, cm["field"], cm["coset"])
    return zk.fri.commit_columns([table_of(zk, cm["field"], t) for t in cm["coeffs"]], cm["b"], cs)


# ---- the commitment ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_coset", (False, True), ids=("plain", "coset"))
@pytest.mark.parametrize("field", FIELDS)
def test_the_commitment_equals_the_model(zk, field, with_coset):
    for d, b in ((1, 1), (2, 1), (5, 2), (9, 1)):
        coset = FC.coset_of(field, d, b, with_coset, mul=71)
        cs = None if coset == 1 else elem(zk, field, coset)
        ints = [NM.random_ints(field, 1 << d, 9100 + 13 * d + field + c) for c in range(32)]
        tables = [table_of(zk, field, t) for t in ints]
        before = [t.evaluated_values for t in tables]
        for k in (1, 2, 3, 17, 32):
            want = CM.commit(field, ints[:k], b, coset, hasher())
            with zk.fri.commit_columns(tables[:k], b, cs) as cm:
                assert cm.k == k and cm.d == d and cm.log_blowup == b and cm.root == want["root"], (d, k)
                st = zk.fri.columns_last_stats()
                assert st["columns"] == k and st["ms_total"] > 0 and min(st["ms_extend"], st["ms_leaves"], st["ms_nodes"]) >= 0
                for j in sorted({0, k // 2, k - 1}):
                    assert np.array_equal(cm.table(j).evaluated_values, before[j])
                    assert np.array_equal(cm.codeword(j).evaluated_values, zk.ntt.low_degree_extend(tables[j], b, cs).evaluated_values), (d, k, j)
                    assert np.array_equal(cm.codeword(j).evaluated_values, to_mont(zk, field, want["codeword"][j]))
                with pytest.raises(zk.ZkError):
                    cm.codeword(k)
                if k == 1:
                    with zk.fri.commit(tables[0], b, cs, log_group=2) as one:
                        assert one.root == cm.root
        assert all(np.array_equal(t.evaluated_values, v) for t, v in zip(tables, before))   # only read


# ---- the opening ---------------------------------------------------------------------------------------------------------------------------
def assert_same_opening(got, fl):
    for name, arr in (("ys", got.ys), ("gamma", got.gamma), ("polys", got.round_polys), ("roots", got.roots), ("final", got.final_table),
                      ("challenges", got.challenges), ("indices", got.query_indices), ("values", got.query_values), ("paths", got.query_paths)):
        assert arr.shape == fl[name].shape and np.array_equal(arr, fl[name]), name


def open_case(zk, field, d, b, f, with_coset, widths, P, g_bits=0):
    p = NM.MODULUS[field]
    pts = FC.points_for(field, d, P, 113 * d + field + sum(widths))
    pm = to_mont(zk, field, [v for z in pts for v in z]).reshape(P, d, 4)
    coset = FC.coset_of(field, d, b, with_coset, mul=71)
    cms = model_commitments(field, d, b, coset, widths, 9700 + 19 * d + field)
    gcs = [gpu_commitment(zk, cm) for cm in cms]
    try:
        prior = b"a caller's own"
        tr = pow_transcript(d, f, g_bits, prefix=prior)
        op = CM.open_columns(cms, pts, f, Q, tr, hasher())
        fl = CM.flat(zk, op)
        t = zk.Transcript()
        t.append(prior)
        got = zk.fri.open_columns(gcs, pm, f, Q, transcript=t, grinding_bits=g_bits)
        assert got.widths == list(widths) and got.pow_nonce == (tr.nonce if g_bits else 0)
        assert_same_opening(got, fl)
        vt = pow_transcript(d, f, g_bits, got.pow_nonce, prior)
        assert CM.verify(op, vt, hasher())
        end, v = zk.Transcript(), zk.Transcript()
        end.append(bytes(vt.buf))
        assert np.array_equal(t.export_state(), end.export_state())   # the prover leaves the caller's transcript in the verifier's end state
        roots = [gc.root for gc in gcs]
        v.append(prior)
        assert roots == op["own_roots"] and zk.fri.verify_columns(roots, widths, pm, got, v)
        assert np.array_equal(v.export_state(), end.export_state())
        st = zk.fri.ml_last_stats()
        assert st["rounds"] == d - f and st["queries"] == Q

        def fresh():
            x = zk.Transcript()
            x.append(prior)
            return x

        if len(widths) > 1:
            assert not zk.fri.verify_columns(roots[1:] + roots[:1], widths, pm, got, fresh())
            if len(set(widths)) > 1:
                assert not zk.fri.verify_columns(roots, widths[1:] + widths[:1], pm, got, fresh())
        assert not zk.fri.verify_columns(roots, widths, pm, got)  # bound to the prior content
        K = sum(widths)
        got.ys[K - 1, 0] = to_mont(zk, field, [(op["ys"][K - 1][0] + 1) % p])[0]
        assert not zk.fri.verify_columns(roots, widths, pm, got, fresh())
    finally:
        for gc in gcs:
            gc.free()


# d = 3 .. 8 and 12 on the five width lists; the field, the blow-up, the coset, log_final and P rotate.  R = 2: (3, f = 1), (4, f = 2), (8, f = 6)
def grid():
    out = []
    for d in (3, 4, 5, 6, 7, 8):
        for s, widths in enumerate(WIDTHS):
            n = d + s
            f = (0, 1, d - 2)[n % 3]
            P = (1, 2, 8)[(n // 2) % 3] if d <= 5 else (1, 2)[n % 2]
            out.append(pytest.param(FIELDS[n % 2], d, 1 + n % 2, f, n % 4 < 2, widths, P, id="f%d-d%d-f%d-w%s-P%d" % (FIELDS[n % 2], d, f, "_".join(map(str, widths)), P)))
    out.append(pytest.param(0, 12, 1, 6, True, (2, 1), 2, id="f0-d12-f6-w2_1-P2"))
    out.append(pytest.param(3, 12, 2, 5, False, (3,), 1, id="f3-d12-f5-w3-P1"))
    return out


@pytest.mark.parametrize("field,d,b,f,with_coset,widths,P", grid())
def test_the_opening_equals_the_model(zk, field, d, b, f, with_coset, widths, P):
    open_case(zk, field, d, b, f, with_coset, widths, P)


@pytest.mark.parametrize("field,d,b,f,widths", [(3, 6, 2, 1, (11, 3, 1, 4)), (0, 5, 1, 3, (2, 1))])
def test_the_opening_with_proof_of_work(zk, field, d, b, f, widths):
    open_case(zk, field, d, b, f, True, widths, 2, g_bits=8)


def test_refusals_write_nothing(zk):
    from zkmle_amd import _lib as L
    lib = zk.lib()
    nq = 4
    mk = lambda field, d, b, coset, k, seed: zk.fri.commit_columns([zk.MultilinearPolynomial.random(field, 1 << d, seed + c) for c in range(k)], b, coset)
    base = [mk(3, 4, 1, None, 2, 1), mk(3, 4, 1, None, 1, 11), mk(3, 4, 1, None, 3, 21)]
    others = {"d": mk(3, 5, 1, None, 2, 31), "blow-up": mk(3, 4, 2, None, 2, 41), "field": mk(0, 4, 1, None, 2, 51), "coset": mk(3, 4, 1, elem(zk, 3, 5), 2, 61)}
    big = [mk(3, 4, 1, None, 16, 71), mk(3, 4, 1, None, 17, 91)]
    FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
    w = lambda n: np.full(n, FILL, np.uint64)
    by = lambda n: np.full(n, 0xA5, np.uint8)
    ys, gamma, polys, roots, fin, chal, idx, vals, paths = w(4 * 40), w(4), w(12 * 4), by(32 * 40), w(4 << 4), w(4 * 4), w(nq), w(4 * nq * 160), by(32 * nq * 400)
    outs = (ys, gamma, polys, roots, fin, chal, idx, vals, paths)
    nonce = C.c_uint64(0xA5)
    pts = zk.from_ints(3, [3, 4, 5, 6]).reshape(1, 4, 4)
    t = zk.Transcript()
    t.append(b"untouched")
    before = t.export_state().copy()

    def raw(cms, m=None, f=0, g=0, drop=None, null_cms=False):
        arr = (C.c_void_p * 33)(*[c._h if c is not None else None for c in cms])
        a = [L.p64(pts), 1, f, nq, g, t._h, L.p64(ys), L.p64(gamma), L.p64(polys), L.p8(roots), L.p64(fin), L.p64(chal), L.p64(idx), L.p64(vals), L.p8(paths), C.byref(nonce)]
        if drop is not None:
            a[drop] = None
        return lib.zk_fri_ml_open_columns_pow(None if null_cms else arr, len(cms) if m is None else m, *a)

    def refused(what, *a, **kw):
        assert raw(*a, **kw) == L.ZK_E_ARG, what
        assert all((o == (FILL if o.dtype == np.uint64 else 0xA5)).all() for o in outs) and nonce.value == 0xA5, what
        assert np.array_equal(t.export_state(), before), what

    try:
        refused("m = 0", base, m=0)
        refused("m = 33", [base[j % 3] for j in range(33)])
        refused("K = 33", big)
        refused("K = 34", [big[0], big[0], base[0]])
        refused("R < 2", base, f=3)
        refused("f = d", base, f=4)
        refused("33 bits", base, g=33)
        refused("no commitments", base, null_cms=True)
        refused("a null commitment", [base[0], None, base[2]])
        for at, what in ((0, "points"), (6, "ys"), (8, "round_polys"), (9, "roots"), (10, "final_table"), (13, "query_values"), (14, "query_paths")):
            refused("NULL " + what, base, drop=at)
        for kind, other in others.items():
            for place in (0, 2):
                cms = list(base)
                cms[place] = other
                refused((kind, place), cms)
        # what was refused in one company is still good in another: the same commitment may stand in several places
        cms = [big[0], base[0], base[0], base[2], base[1], base[2], base[2], base[1]]   # K = 16 + 2 + 2 + 3 + 1 + 3 + 3 + 1 = 31
        got = zk.fri.open_columns(cms, pts, 0, nq)
        assert zk.fri.verify_columns([c.root for c in cms], [c.k for c in cms], pts, got)
        got = zk.fri.open_columns(cms + [base[1]], pts, 2, nq)   # K = 32, R = 2
        assert zk.fri.verify_columns([c.root for c in cms + [base[1]]], [c.k for c in cms] + [1], pts, got)
    finally:
        for c in base + big + list(others.values()):
            c.free()
