"""CPU: the host side of column commitments (include/zkmle.h "Merkle commitment of several columns", "Column commitments opened together").
Everything compares against tests/_fri_ml_columns_model.py:

  leaf        zk_merkle_verify_columns accepts the model's leaf and path for every k in 1 .. 32 on both fields and rejects a moved value, a
              neighbour's index, another k and an unreduced element; at k = 1 it is zk_merkle_verify_grouped(.., 2)
  accepts     zk_fri_ml_verify_columns_pow accepts the model's openings at d = 2 .. 5 on both fields for the widths [1], [3], [2, 1], [17] and
              [11, 3, 1, 4], P among 1, 2, 8, R = 2 (one step), R even and R odd, with and without 8 bits of proof of work, and leaves the
              caller's transcript where the model's verifier leaves its own
  rejects     *ok = 0 for a flipped bit in every array, a step-0 value moved to another column of the same leaf, two columns swapped inside one
              commitment, the widths [2, 1] read as [1, 2], swapped roots, a path of another commitment, d +- 1, a wrong nonce, an unreduced
              element
  refuses     ZK_E_ARG for K = 33, m = 0, a zero width, and the rest of the statuses that precede the transcript
  sizes       zk_fri_ml_sizes_columns equals the model's counts and, at m = K = 1, zk_fri_ml_sizes_batch(1, .., 2, 2)

Commitments cannot exist without a device: the kernel, the commitment and the prover run in tests/test_gpu_merkle_columns.py and
test_gpu_fri_columns.py."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import __graft_entry__ as G
import _fri_ml_cases as FC
import _fri_ml_columns_model as CM
import _fri_ml_family_model as FAM
import _grind_model as GR
import _merkle_model as MM
import _ntt_model as NM
from oracle import pymodel as M

zk = G.import_package()
P64, P8, P32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
p64 = lambda a: a.ctypes.data_as(P64) if a is not None else None
p8 = lambda a: a.ctypes.data_as(P8) if a is not None else None
NEW_NAMES = ("zk_merkle_build_columns", "zk_mle_merkle_root_columns", "zk_merkle_verify_columns", "zk_fri_commit_columns", "zk_fri_columns_free",
             "zk_fri_columns_root", "zk_fri_columns_count", "zk_fri_columns_table", "zk_fri_columns_codeword", "zk_fri_columns_last_stats",
             "zk_fri_ml_sizes_columns", "zk_fri_ml_open_columns_pow", "zk_fri_ml_verify_columns_pow")
Q, BITS = 3, 8
ARG, RANGE = -7, -6
# (field, d, b, f, coset, widths, P, bits): d = 2 .. 5 on both fields; R = 2 is a single step, R = 4 even, R = 3 and 5 end in the pair-leaf step
CASES = [(0, 2, 1, 0, False, (1,), 1, 0),            # R = 2
         (3, 3, 1, 0, True, (3,), 2, 0),             # R = 3
         (0, 4, 2, 0, True, (2, 1), 8, 0),           # R = 4
         (3, 5, 1, 2, False, (17,), 1, BITS),        # R = 3
         (0, 5, 1, 0, True, (11, 3, 1, 4), 2, BITS),  # R = 5
         (3, 4, 1, 2, False, (11, 3, 1, 4), 1, 0),   # R = 2
         (0, 3, 2, 1, False, (17,), 2, 0),           # R = 2
         (3, 4, 1, 0, True, (2, 1), 1, BITS),        # R = 4
         (0, 5, 2, 1, False, (3,), 8, 0),            # R = 4
         (3, 2, 2, 0, True, (1,), 2, BITS)]          # R = 2
case_id = lambda c: "f%d-d%d-b%d-f%d-c%d-w%s-P%d-g%d" % (c[0], c[1], c[2], c[3], c[4], "_".join(map(str, c[5])), c[6], c[7])


@functools.lru_cache(maxsize=None)
def hasher():
    return CM.check_host_keccak(zk)


class FastPow(GR.PowTranscript):
    """tests/_grind_model.py's PowTranscript with the nonce search on the checked host hash: 8 bits are some 256 candidates"""

    def sample(self):
        if self.bits and self.count == self.at and self.nonce is None:
            M.Transcript.append(self, GR.tag(self.bits))
            base, w = bytes(self.buf), 0
            while not GR.leading_zero(hasher()(base + GR.be64(w)), self.bits):
                w += 1
            M.Transcript.append(self, GR.be64(w))
            assert GR.leading_zero(M.Transcript.sample(self), self.bits)
            self.nonce, self.pow_ok = w, True
            self.count += 1
            return M.Transcript.sample(self)
        return super().sample()


def pow_transcript(d, f, bits, nonce=None, prefix=b""):
    tr = FastPow(bits, 1 + (d - f), nonce)
    tr.append(prefix)
    return tr


@functools.lru_cache(maxsize=None)
def commitment(field, d, b, with_coset, k, j):
    coset = FC.coset_of(field, d, b, with_coset, mul=67)
    tables = [NM.random_ints(field, 1 << d, 7700 + 31 * d + field + 101 * j + 7 * c) for c in range(k)]
    return CM.commit(field, tables, b, coset, hasher())


@functools.lru_cache(maxsize=None)
def opening(case, prefix=b""):
    """-> (the model's opening on a transcript that holds `prefix`, the nonce)"""
    field, d, b, f, with_coset, widths, P, bits = case
    cms = [commitment(field, d, b, with_coset, w, j) for j, w in enumerate(widths)]
    tr = pow_transcript(d, f, bits, prefix=prefix)
    op = CM.open_columns(cms, FC.points_for(field, d, P, 37 * d + field + sum(widths)), f, Q, tr, hasher())
    return op, (tr.nonce if bits else 0)


def lib_verify(op, fl=None, tr=None, g=0, nonce=0, **over):
    """zk_fri_ml_verify_columns_pow on the model's opening `op` (flat arrays `fl`) -> (status, ok)"""
    fl = CM.flat(zk, op) if fl is None else fl
    s = {n: op[n] for n in ("d", "b", "f", "Q")}
    s.update({n: v for n, v in over.items() if n in s})
    widths = over.get("widths", op["widths"])
    m = over.get("m", len(widths))
    wa = (C.c_uint32 * max(len(widths), 1))(*widths)
    cs = zk.from_ints(op["field"], [op["coset"]])[0]
    ok = C.c_int(-1)
    rc = zk.lib().zk_fri_ml_verify_columns_pow(over.get("field", op["field"]), p8(fl["own_roots"]), wa, m, s["d"], s["b"], s["f"], s["Q"], g, p64(cs), p64(fl["points"]),
                                               over.get("P", len(op["points"])), p64(fl["ys"]), None if tr is None else tr._h, p64(fl["polys"]), p8(fl["roots"]),
                                               p64(fl["final"]), p64(fl["values"]), p8(fl["paths"]), nonce, C.byref(ok))
    return rc, ok.value


def test_new_exports_and_the_header():
    lib = zk.lib()
    header = open(G.ROOT + "/include/zkmle.h").read()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in header, name
    assert "Column commitments opened together" in header and "Merkle commitment of several columns" in header and "#define ZK_FRI_COLUMNS_MAX 32" in header
    for name in ("commit_columns", "FriColumns", "columns_sizes", "open_columns", "FriColumnsOpening", "verify_columns", "columns_last_stats"):
        assert hasattr(zk.fri, name), name
    assert hasattr(zk.merkle, "columns_root") and hasattr(zk.MerkleTree, "build_columns") and hasattr(zk.MerkleTree, "verify_columns")


# ---- the leaf ------------------------------------------------------------------------------------------------------------------------------
def leaf_verify(field, root, depth, index, k, el, path):
    ok = C.c_int(-1)
    buf = path if path.size else np.zeros(32, np.uint8)
    rc = zk.lib().zk_merkle_verify_columns(field, p8(np.frombuffer(root, np.uint8).copy()), depth, index, k, p64(el), p8(buf), C.byref(ok))
    return rc, ok.value


@pytest.mark.parametrize("field", (0, 3))
def test_the_leaf_verifier_against_the_model_for_every_k(field):
    p, n = NM.MODULUS[field], 16                              # 4 leaves, depth 2
    cols = [MM.random_ints(field, n, 5200 + 3 * field + c) for c in range(32)]
    assert [CM.blocks(k) for k in (1, 2, 16, 17, 18, 32)] == [1, 2, 16, 17, 17, 31]
    for k in range(1, 33):
        levels = CM.levels_of(cols[:k], hasher())
        root = levels[-1][0]
        for j in (0, 3):
            quads = [[c[j + s * 4] for s in range(4)] for c in cols[:k]]
            path = MM.path_of(levels, j)
            assert CM.verify_leaf(root, j, quads, path, hasher())
            el = CM.mont(zk, field, [v for q in quads for v in q])
            pa = np.frombuffer(b"".join(path), np.uint8).copy()
            assert leaf_verify(field, root, 2, j, k, el, pa) == (0, 1), (k, j)
            assert zk.MerkleTree.verify_columns(field, root, j, el.reshape(k, 4, 4), pa)
            assert leaf_verify(field, root, 2, j ^ 1, k, el, pa) == (0, 0)
            moved = el.copy()
            moved[[0, 4 * k - 1]] = moved[[4 * k - 1, 0]]     # the first and last element of the leaf change places
            assert leaf_verify(field, root, 2, j, k, moved, pa) == (0, int(np.array_equal(moved, el)))
            if k > 1:
                assert leaf_verify(field, root, 2, j, k - 1, el, pa) == (0, 0)
            big = el.copy()
            big[4 * k - 1] = np.frombuffer(int(p).to_bytes(32, "little"), np.uint64)   # p itself: not reduced
            assert leaf_verify(field, root, 2, j, k, big, pa) == (0, 0)
            if k == 1:                                        # the grouped quad leaf byte for byte
                ok = C.c_int(-1)
                assert zk.lib().zk_merkle_verify_grouped(field, p8(np.frombuffer(root, np.uint8).copy()), 2, j, 2, p64(el), p8(pa), C.byref(ok)) == 0 and ok.value == 1
                assert root == FAM.levels_of(cols[0], 2, hasher())[-1][0]
    # depth 0: the root is the leaf
    one = CM.levels_of([c[:4] for c in cols[:17]], hasher())
    assert len(one) == 1 and leaf_verify(field, one[0][0], 0, 0, 17, CM.mont(zk, field, [v for c in cols[:17] for v in c[:4]]), np.zeros(0, np.uint8)) == (0, 1)


def test_the_leaf_verifiers_statuses():
    el, pa, root = np.zeros((4 * 33, 4), np.uint64), np.zeros(64, np.uint8), bytes(32)
    assert leaf_verify(0, root, 2, 0, 0, el, pa)[0] == ARG and leaf_verify(0, root, 2, 0, 33, el, pa)[0] == ARG
    assert leaf_verify(1, root, 2, 0, 1, el, pa)[0] == ARG and leaf_verify(2, root, 2, 0, 1, el, pa)[0] == ARG and leaf_verify(9, root, 2, 0, 1, el, pa)[0] == ARG
    assert leaf_verify(0, root, 2, 4, 1, el, pa)[0] == RANGE and leaf_verify(0, root, 64, 0, 1, el, pa)[0] == RANGE
    ok = C.c_int(-1)
    lib = zk.lib()
    assert lib.zk_merkle_verify_columns(0, None, 2, 0, 1, p64(el), p8(pa), C.byref(ok)) == ARG and lib.zk_merkle_verify_columns(0, p8(pa), 2, 0, 1, None, p8(pa), C.byref(ok)) == ARG
    assert lib.zk_merkle_verify_columns(0, p8(pa), 2, 0, 1, p64(el), None, C.byref(ok)) == ARG and lib.zk_merkle_verify_columns(0, p8(pa), 2, 0, 1, p64(el), p8(pa), None) == ARG
    assert ok.value == -1


# ---- the opening's verifier ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_verifier_accepts_the_models_openings(case):
    field, d, b, f, with_coset, widths, P, bits = case
    prior = b"a caller's own"
    op, nonce = opening(case, prior)
    vt = pow_transcript(d, f, bits, nonce, prior)
    assert CM.verify(op, vt, hasher()) and (vt.pow_ok or not bits)
    fl = CM.flat(zk, op)
    want = CM.sizes(widths, d, b, f, Q)
    assert want == (fl["roots"].shape[0], fl["final"].shape[0], fl["values"].size // 4, fl["paths"].size, fl["polys"].size // 4)
    assert zk.fri.columns_sizes(widths, d, b, f, Q) == want
    t = zk.Transcript()
    t.append(prior)
    assert lib_verify(op, fl, t, g=bits, nonce=nonce) == (0, 1)
    end = zk.Transcript()                                     # the caller's transcript ends where the model's verifier ends
    end.append(bytes(vt.buf))
    assert np.array_equal(t.export_state(), end.export_state())
    assert lib_verify(op, fl, g=bits, nonce=nonce) == (0, 0)  # bound to the prior content
    if bits:
        t2 = zk.Transcript()
        t2.append(prior)
        assert lib_verify(op, fl, t2, g=bits, nonce=nonce + 1) == (0, 0)
        t3 = zk.Transcript()
        t3.append(prior)
        assert lib_verify(op, fl, t3) == (0, 0)               # without the step the indices are others
    # the Python wrapper
    cs = zk.from_ints(field, [op["coset"]])[0]
    o = zk.fri.FriColumnsOpening(field, widths, P, d, b, f, Q, coset=cs, grinding_bits=bits)
    assert o.roots.shape == fl["roots"].shape and o.query_values.shape == fl["values"].shape and o.query_paths.shape == fl["paths"].shape and o.ys.shape == fl["ys"].shape
    o.ys, o.round_polys, o.roots, o.final_table, o.query_values, o.query_paths, o.pow_nonce = fl["ys"], fl["polys"], fl["roots"], fl["final"], fl["values"], fl["paths"], nonce
    t4 = zk.Transcript()
    t4.append(prior)
    assert zk.fri.verify_columns(op["own_roots"], widths, fl["points"], o, t4)
    assert not zk.fri.verify_columns(op["own_roots"], widths, fl["points"], o)


def plain_case(case):
    """the case without a prior transcript: what the tampering tests start from -> (op, nonce, flat, bits)"""
    op, nonce = opening(case)
    return op, nonce, CM.flat(zk, op), case[7]


@pytest.mark.parametrize("case", [CASES[2], CASES[4], CASES[5]], ids=case_id)
def test_one_flipped_bit_anywhere_is_rejected(case):
    op, nonce, base, bits = plain_case(case)
    assert lib_verify(op, base, g=bits, nonce=nonce) == (0, 1)
    rng = random.Random(97 + case[1])
    m, K, R, L = len(op["widths"]), sum(op["widths"]), op["d"] - op["f"], op["d"] + op["b"]
    per_q = base["paths"].size // Q
    spots = [("ys", (c, rng.randrange(len(op["points"])), rng.randrange(4))) for c in range(K)]
    spots += [("points", (0, rng.randrange(op["d"]), rng.randrange(4)))]
    spots += [("polys", (l, i, rng.randrange(4))) for l in range(R) for i in range(3)]
    spots += [("roots", (s, rng.randrange(32))) for s in range(base["roots"].shape[0])]
    spots += [("own_roots", (j, rng.randrange(32))) for j in range(m)]
    spots += [("final", (j, rng.randrange(4))) for j in range(1 << op["f"])]
    spots += [("values", (rng.randrange(Q), v, rng.randrange(4))) for v in range(base["values"].shape[1])]
    spots += [("paths", (q * per_q + 32 * at + rng.randrange(32),)) for q in (0, Q - 1) for at in (0, (L - 2) * m - 1, per_q // 32 - 1)]
    for name, at in spots:
        assert lib_verify(op, FC.tampered(base, name, at, rng), g=bits, nonce=nonce) == (0, 0), (name, at)


def test_values_columns_widths_roots_and_paths_out_of_place():
    case = CASES[5]                                           # widths 11, 3, 1, 4
    op, nonce, base, bits = plain_case(case)
    widths, L = list(op["widths"]), op["d"] + op["b"]
    copy = lambda: {n: v.copy() for n, v in base.items()}
    # a step-0 value moved to another column of the same leaf: sides 1 of columns 0 and 1 (both of commitment 0) change places in one query
    fl = copy()
    fl["values"][1, [0 * 4 + 1, 1 * 4 + 1]] = fl["values"][1, [1 * 4 + 1, 0 * 4 + 1]]
    assert lib_verify(op, fl) == (0, 0)
    # two columns swapped inside one commitment, consistently: their quads in every query and their claims
    fl = copy()
    a, bb = 11, 13                                            # the first and last column of commitment 1
    fl["values"][:, list(range(4 * a, 4 * a + 4)) + list(range(4 * bb, 4 * bb + 4))] = fl["values"][:, list(range(4 * bb, 4 * bb + 4)) + list(range(4 * a, 4 * a + 4))]
    fl["ys"][[a, bb]] = fl["ys"][[bb, a]]
    assert lib_verify(op, fl) == (0, 0)
    # swapped roots, in the verifier's own copy alone and in both copies
    fl = copy()
    fl["own_roots"][[0, 1]] = fl["own_roots"][[1, 0]]
    assert lib_verify(op, fl) == (0, 0)
    fl["roots"][[0, 1]] = fl["roots"][[1, 0]]
    assert lib_verify(op, fl) == (0, 0)
    # a path of another commitment: the step-0 paths of commitments 0 and 1 change places in one query
    fl = copy()
    per_q, n0 = fl["paths"].size // Q, 32 * (L - 2)
    pq = fl["paths"][per_q:2 * per_q]
    first, second = pq[:n0].copy(), pq[n0:2 * n0].copy()
    pq[:n0], pq[n0:2 * n0] = second, first
    assert lib_verify(op, fl) == (0, 0)
    assert lib_verify(op, base) == (0, 1)
    # the widths [2, 1] read as [1, 2], and as [3]
    op2, nonce2, base2, bits2 = plain_case(CASES[7])
    assert lib_verify(op2, base2, g=bits2, nonce=nonce2) == (0, 1)
    assert lib_verify(op2, base2, g=bits2, nonce=nonce2, widths=[1, 2]) == (0, 0)
    assert lib_verify(op2, FC.padded(base2), g=bits2, nonce=nonce2, widths=[3]) == (0, 0)
    assert lib_verify(op2, base2, g=bits2, nonce=nonce2 ^ 1) == (0, 0) and lib_verify(op2, base2, g=bits2 - 1, nonce=nonce2) == (0, 0)


@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=case_id)
def test_another_d_and_unreduced_elements(case):
    op, nonce, base, bits = plain_case(case)
    big = FC.padded(base, room=1 << 16)
    assert lib_verify(op, big) == (0, 1)
    assert lib_verify(op, big, d=op["d"] + 1) == (0, 0) and lib_verify(op, big, d=op["d"] - 1) == (0, 0)
    assert lib_verify(op, big, b=op["b"] + 1) == (0, 0) and lib_verify(op, big, Q=Q - 1) == (0, 0) and lib_verify(op, big, f=op["f"] + 1) == (0, 0)
    pl = np.frombuffer(int(NM.MODULUS[op["field"]]).to_bytes(32, "little"), np.uint64)
    for name in ("ys", "polys", "final", "values", "points"):
        fl = {n: v.copy() for n, v in base.items()}
        fl[name].reshape(-1, 4)[-1] = pl                      # p itself
        assert lib_verify(op, fl) == (0, 0), name
        fl[name].reshape(-1, 4)[-1] = 0xFFFFFFFFFFFFFFFF
        assert lib_verify(op, fl) == (0, 0), name


def test_the_statuses_come_before_the_transcript():
    from zkmle_amd import _lib as L
    lib = zk.lib()
    assert (L.ZK_E_ARG, L.ZK_E_RANGE) == (ARG, RANGE)
    op, nonce, base, bits = plain_case(CASES[2])
    fl = FC.padded(base, room=1 << 16)
    t = zk.Transcript()
    before = t.export_state().copy()
    for over in (dict(widths=[17, 16]), dict(widths=[33]), dict(widths=[2, 1], m=0), dict(widths=[2, 0]), dict(widths=[0]), dict(widths=[1] * 33), dict(P=0), dict(P=9),
                 dict(f=op["d"] - 1), dict(f=op["d"]), dict(b=0), dict(b=9), dict(Q=0), dict(Q=4097), dict(d=0), dict(field=7)):
        assert lib_verify(op, fl, t, **over)[0] == ARG, over
    assert lib_verify(op, fl, t, g=33)[0] == ARG
    assert lib_verify(op, fl, t, field=1)[0] == RANGE and lib_verify(op, fl, t, field=2)[0] == RANGE and lib_verify(op, fl, t, d=33)[0] == RANGE and lib_verify(op, fl, t, d=31, b=2)[0] == RANGE
    assert lib_verify(op, fl, widths=[16, 16])[0] == 0        # K = 32 is served
    ok = C.c_int(-1)
    wa, cs = (C.c_uint32 * 2)(2, 1), zk.from_ints(0, [op["coset"]])[0]
    args = [p8(fl["own_roots"]), wa, 2, op["d"], op["b"], op["f"], Q, 0, p64(cs), p64(fl["points"]), 8, p64(fl["ys"]), t._h, p64(fl["polys"]), p8(fl["roots"]),
            p64(fl["final"]), p64(fl["values"]), p8(fl["paths"]), 0, C.byref(ok)]
    for at in (0, 1, 9, 11, 13, 14, 15, 16, 17, 19):          # every pointer in turn
        a = list(args)
        a[at] = None
        assert lib.zk_fri_ml_verify_columns_pow(0, *a) == ARG, at
    zero = np.zeros(4, np.uint64)
    a = list(args)
    a[8] = p64(zero)
    assert lib.zk_fri_ml_verify_columns_pow(0, *a) == ARG     # a zero coset
    assert ok.value == -1 and np.array_equal(t.export_state(), before)
    assert lib.zk_fri_ml_verify_columns_pow(0, *args) == 0 and ok.value == 1   # the untouched transcript still verifies the opening
    # the prover and the commitment as far as they go without a device: the argument errors first, and nothing written
    w = lambda n: np.full(n, 7, np.uint64)
    pts, ys, gamma, pl, rt, fn_, vl, pa = w(64 * 4), w(33 * 4), w(4), w(64 * 12), np.full(96 * 32, 7, np.uint8), w(4 << 10), w(1 << 12), np.full(1 << 12, 7, np.uint8)
    nul, nonce_ = (C.c_void_p * 33)(), C.c_uint64(7)
    opn = lambda cms, m: lib.zk_fri_ml_open_columns_pow(cms, m, p64(pts), 1, 0, 4, 0, None, p64(ys), p64(gamma), p64(pl), p8(rt), p64(fn_), None, None, p64(vl), p8(pa), C.byref(nonce_))
    assert opn(nul, 0) == ARG and opn(nul, 33) == ARG and opn(nul, 2) == ARG and opn(None, 1) == ARG
    assert all((a == 7).all() for a in (ys, gamma, pl, rt, fn_, vl, pa)) and nonce_.value == 7
    h = [C.c_void_p() for _ in range(5)]
    for hh, (field, n) in zip(h, ((0, 8), (0, 8), (0, 4), (3, 8), (0, 6))):
        L.check(lib.zk_table_wrap(field, C.c_void_p(0x1000), n, C.byref(hh)))
    arr = lambda *hs: (C.c_void_p * 33)(*hs)
    out, root = C.c_void_p(), np.zeros(32, np.uint8)
    com = lambda tabs, k, b=1, coset=None: lib.zk_fri_commit_columns(tabs, k, b, coset, C.byref(out))
    assert com(arr(h[0]), 0) == ARG and com(arr(h[0]), 33) == ARG and com(None, 1) == ARG and com(arr(h[0], None), 2) == ARG and com(arr(h[0], h[3]), 2) == ARG
    assert com(arr(h[0]), 1, 0) == ARG and com(arr(h[0]), 1, 9) == ARG and com(arr(h[0]), 1, 1, p64(zero)) == ARG
    assert lib.zk_fri_commit_columns(arr(h[0]), 1, 1, None, None) == ARG
    assert com(arr(h[0], h[2]), 2) == L.ZK_E_LEN_MISMATCH and com(arr(h[4], h[4]), 2) == L.ZK_E_NOT_POW2
    for fn in (lambda tabs, k: lib.zk_merkle_build_columns(tabs, k, C.byref(out)), lambda tabs, k: lib.zk_mle_merkle_root_columns(tabs, k, p8(root))):
        assert fn(arr(h[0]), 0) == ARG and fn(arr(h[0]), 33) == ARG and fn(None, 1) == ARG and fn(arr(h[0], None), 2) == ARG and fn(arr(h[0], h[3]), 2) == ARG
        assert fn(arr(h[0], h[2]), 2) == L.ZK_E_LEN_MISMATCH and fn(arr(h[4], h[4]), 2) == L.ZK_E_NOT_POW2
    import torch
    if not torch.cuda.is_available():
        assert com(arr(h[0], h[1]), 2) == L.ZK_E_NO_DEVICE and lib.zk_mle_merkle_root_columns(arr(h[0], h[1]), 2, p8(root)) == L.ZK_E_NO_DEVICE
    assert not out.value and not root.any()
    assert lib.zk_fri_columns_count(None) == 0 and lib.zk_fri_columns_free(None) == 0 and lib.zk_fri_columns_root(None, p8(root)) == ARG
    assert lib.zk_fri_columns_table(None, 0, C.byref(out)) == ARG and lib.zk_fri_columns_codeword(None, 0, C.byref(out)) == ARG and lib.zk_fri_columns_last_stats(None) == ARG
    for hh in h:
        lib.zk_table_free(hh)


def test_sizes():
    lib = zk.lib()

    def sizes(widths, d, b, f, q, m=None):
        out = [C.c_size_t(0) for _ in range(5)]
        wa = (C.c_uint32 * max(len(widths), 1))(*widths)
        return lib.zk_fri_ml_sizes_columns(wa, len(widths) if m is None else m, d, b, f, q, *[C.byref(o) for o in out]), tuple(int(o.value) for o in out)

    for widths in ([1], [3], [2, 1], [17], [11, 3, 1, 4], [12, 3, 1, 4], [1] * 32, [32]):
        for d, b, f, q in ((2, 1, 0, 1), (3, 1, 0, 4), (6, 1, 0, 8), (6, 2, 1, 8), (24, 2, 6, 64)):
            assert sizes(widths, d, b, f, q) == (0, CM.sizes(widths, d, b, f, q)), (widths, d)
    for d, b, f, q in ((2, 1, 0, 1), (5, 2, 0, 3), (24, 2, 6, 64)):   # one commitment of one column is the grouped batch of one
        out = [C.c_size_t(0) for _ in range(5)]
        assert lib.zk_fri_ml_sizes_batch(1, d, b, f, q, 2, 2, *[C.byref(o) for o in out]) == 0
        assert sizes([1], d, b, f, q) == (0, tuple(int(o.value) for o in out))
    # the path bytes of the twenty columns of four commitments against twenty commitments, d = 24, b = 2, f = 6, Q = 64
    cols, wide = sizes([12, 3, 1, 4], 24, 2, 6, 64)[1], zk.fri.ml_sizes_wide(24, 2, 6, 64, 2, True, k=20)
    assert wide[3] - cols[3] == 16 * 64 * 24 * 32 and cols[:3] == (wide[0] - 16,) + wide[1:3] and cols[4] == wide[4]
    for widths, m in (([], None), ([0], None), ([2, 0, 1], None), ([33], None), ([17, 16], None), ([1] * 33, None), ([1], 0)):
        assert sizes(widths, 6, 1, 0, 8, m)[0] == ARG, widths
    assert lib.zk_fri_ml_sizes_columns(None, 1, 6, 1, 0, 8, *[None] * 5) == ARG
    assert sizes([2, 1], 6, 1, 5, 8)[0] == ARG and sizes([2, 1], 6, 0, 0, 8)[0] == ARG and sizes([2, 1], 6, 1, 0, 0)[0] == ARG   # R < 2, b, Q
    wa = (C.c_uint32 * 2)(2, 1)
    assert lib.zk_fri_ml_sizes_columns(wa, 2, 6, 1, 0, 8, *[None] * 5) == 0
