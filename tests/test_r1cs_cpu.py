"""CPU: the host side of an R1CS instance (include/zkmle.h "R1CS instance: sparse matrices times a table") against the integer model of
tests/_r1cs_model.py.  Creating an instance needs no device.

  digest     zk_r1cs_digest equals the model's on both fields, whatever order the entries come in; another value, another position, an entry
             moved from A to B and another shape each give another digest
  refusals   every refusal of zk_r1cs_create returns ZK_E_ARG: a row or column out of range, an unreduced value, a duplicate (row, column) in
             one matrix (the same pair in two matrices is fine), s or d out of range, a field without a domain, a NULL
  bins       zk_r1cs_shape reports the rows and columns above ZK_R1CS_ROW_SPLIT: a row of 32 entries is not one, a row of 33 is; a column
             counts the three matrices' entries together
  device     the two passes refuse a table of another field or length before they look for a device, and without one return ZK_E_NO_DEVICE

The kernels run in tests/test_gpu_r1cs.py."""
import ctypes as C
import random

import numpy as np
import pytest

import __graft_entry__ as G
import _ntt_model as NM
import _r1cs_model as RM

zk = G.import_package()
FIELDS = (0, 3)
NEW_NAMES = ("zk_r1cs_create", "zk_r1cs_free", "zk_r1cs_digest", "zk_r1cs_shape", "zk_r1cs_matvec", "zk_r1cs_bind_rows", "zk_r1cs_last_stats")


def triple(field, m):
    return [e[0] for e in m], [e[1] for e in m], zk.from_ints(field, [e[2] for e in m])


def instance(field, s, d, mats):
    return zk.R1CS(field, s, d, *(triple(field, m) for m in mats))


def create_status(field, s, d, mats, raw_vals=None):
    """zk_r1cs_create's status on integer matrices; raw_vals[k]: limbs handed over as they are in place of matrix k's values"""
    L = zk.lib()
    keep, rp, cp, vp, nnz = [], [], [], [], []
    for k, m in enumerate(mats):
        r, c = np.array([e[0] for e in m], np.uint32), np.array([e[1] for e in m], np.uint32)
        v = raw_vals[k] if raw_vals and raw_vals[k] is not None else zk.from_ints(field if field in FIELDS else 0, [e[2] for e in m])
        keep += [r, c, v]
        rp.append(r.ctypes.data_as(C.POINTER(C.c_uint32)))
        cp.append(c.ctypes.data_as(C.POINTER(C.c_uint32)))
        vp.append(v.ctypes.data_as(C.POINTER(C.c_uint64)))
        nnz.append(len(m))
    h = C.c_void_p()
    rc = L.zk_r1cs_create(field, s, d, (C.POINTER(C.c_uint32) * 3)(*rp), (C.POINTER(C.c_uint32) * 3)(*cp), (C.POINTER(C.c_uint64) * 3)(*vp),
                          (C.c_size_t * 3)(*nnz), C.byref(h))
    if rc == 0:
        assert L.zk_r1cs_free(h) == 0
    else:
        assert not h.value
    return rc


def test_the_new_symbols_are_exported():
    lib = C.CDLL(zk.library_path())
    assert all(hasattr(lib, n) for n in NEW_NAMES)


@pytest.mark.parametrize("field", FIELDS)
def test_digest_equals_the_model_whatever_the_entry_order(field):
    p = NM.MODULUS[field]
    s, d = 4, 5
    mats = [RM.random_matrix(field, s, d, 3, 100 + k + field) for k in range(3)]
    mats[1] = mats[1][:7]
    want = RM.digest(field, s, d, mats)
    assert instance(field, s, d, mats).digest == want
    rng = random.Random(7 + field)
    for _ in range(3):
        shuffled = [rng.sample(m, len(m)) for m in mats]
        assert instance(field, s, d, shuffled).digest == want
    r, c, v = mats[0][0]
    others = {
        "value": [[(r, c, (v + 1) % p)] + mats[0][1:], mats[1], mats[2]],
        "moved to B": [mats[0][:-1], mats[1] + [mats[0][-1]], mats[2]] if (mats[0][-1][0], mats[0][-1][1]) not in {(e[0], e[1]) for e in mats[1]} else None,
        "empty C": [mats[0], mats[1], []],
    }
    for what, other in others.items():
        if other is not None:
            got = instance(field, s, d, other).digest
            assert got == RM.digest(field, s, d, other) and got != want, what
    assert instance(field, s, d + 1, mats).digest == RM.digest(field, s, d + 1, mats) != want
    assert instance(field, s, d, [[], [], []]).digest == RM.digest(field, s, d, [[], [], []])


@pytest.mark.parametrize("field", FIELDS)
def test_every_refusal_of_create(field):
    p = NM.MODULUS[field]
    s, d = 3, 4
    ok = [[(0, 0, 1), (7, 15, p - 1)], [(0, 0, 5)], []]
    assert create_status(field, s, d, ok) == 0                                  # the same pair in A and B, the last row and column, an empty C
    assert create_status(field, s, d, [[(8, 0, 1)], [], []]) == -7              # row = 2^s
    assert create_status(field, s, d, [[], [(0, 16, 1)], []]) == -7             # column = 2^d
    assert create_status(field, s, d, [[], [], [(1, 2, 3), (4, 5, 6), (1, 2, 9)]]) == -7   # a duplicate, apart in the list
    limbs = np.array([[(p >> (64 * k)) & (2 ** 64 - 1) for k in range(4)]], np.uint64)   # the limbs of p itself
    assert create_status(field, s, d, [[(1, 1, 0)], [], []], raw_vals=[limbs, None, None]) == -7
    assert create_status(field, s, d, [[(1, 1, 0)], [], []], raw_vals=[np.full((1, 4), 2 ** 64 - 1, np.uint64), None, None]) == -7
    for bad_s, bad_d in ((0, 4), (3, 1), (29, 4), (3, 29)):
        assert create_status(field, bad_s, bad_d, [[], [], []]) == -7
    for bad_field in (1, 2, 4, -1):
        assert create_status(bad_field, s, d, [[], [], []]) == -7
    L = zk.lib()
    assert L.zk_r1cs_create(field, s, d, None, None, None, None, C.byref(C.c_void_p())) == -7
    assert L.zk_r1cs_digest(None, None) == -7 and L.zk_r1cs_shape(None, None, None, None, None, None) == -7
    assert L.zk_r1cs_free(None) == 0


def test_the_bins_split_above_the_threshold():
    field, s, d = 0, 3, 7
    T = RM.ROW_SPLIT
    assert zk.r1cs.ROW_SPLIT == T
    A = [(0, c, 1) for c in range(T - 1)] + [(1, c, 1) for c in range(T)] + [(2, c, 1) for c in range(T + 1)]
    B = [(5, c, 2) for c in range(1 << d)]
    # rows 0, 1, 2 of A hold T - 1, T, T + 1 entries and row 5 of B is full; column 100 holds 5 + 1 + 8 entries: three matrices of 8 rows stay below T
    Cm = [(r, 100, 3) for r in range(8)]
    mats = [A + [(r, 100, 1) for r in range(3, 8)], B, Cm]
    sh = instance(field, s, d, mats).shape
    assert sh["field"] == field and sh["log_rows"] == s and sh["log_cols"] == d and sh["nnz"] == tuple(len(m) for m in mats)
    assert (sh["block_rows"], sh["block_cols"]) == RM.lengths(s, d, mats) == (2, 0)
    # a column above the threshold needs more than 32 entries over three matrices of 2^s rows: s = 4 gives up to 48
    s = 4
    col = lambda k, n: [(r, 9, k + 1) for r in range(n)]
    for na, nb, nc, want in ((16, 16, 0, 0), (16, 16, 1, 1), (11, 11, 10, 0), (11, 11, 11, 1)):
        mats = [col(0, na), col(1, nb), col(2, nc)]
        sh = instance(field, s, d, mats).shape
        assert (sh["block_rows"], sh["block_cols"]) == RM.lengths(s, d, mats) == (0, want), (na, nb, nc)


def test_the_passes_check_their_arguments_before_the_device():
    import torch
    L = zk.lib()
    inst = instance(0, 3, 4, [[(0, 0, 1)], [], []])
    assert L.zk_r1cs_matvec(inst._h, None, None) == -7
    assert L.zk_r1cs_bind_rows(inst._h, None, None, 0, None) == -7
    p = NM.MODULUS[0]
    rx = zk.from_ints(0, [1, 2, 3])
    bad = np.array([[(p >> (64 * k)) & (2 ** 64 - 1) for k in range(4)]], np.uint64)
    out = C.c_void_p()
    as64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.zk_r1cs_bind_rows(inst._h, as64(rx), as64(bad), 0, C.byref(out)) == -7        # rho = p
    assert L.zk_r1cs_bind_rows(inst._h, as64(np.concatenate([rx[:2], bad])), as64(rx), 0, C.byref(out)) == -7
    if not torch.cuda.is_available():
        assert L.zk_r1cs_bind_rows(inst._h, as64(rx), as64(rx), 0, C.byref(out)) == -9     # ZK_E_NO_DEVICE: no CPU fallback
        assert not out.value
