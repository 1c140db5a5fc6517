"""GPU: the two sparse passes of an R1CS instance (csrc/r1cs.cuh, csrc/zkmle_r1cs.hip; include/zkmle.h "R1CS instance: sparse matrices times a
table") over BLS12-381 Fr and BN254 Fr, byte for byte against the integer model of tests/_r1cs_model.py; no tolerance anywhere.

  shapes    one list of instances serves both passes: zk_r1cs_matvec runs on an instance as it is, zk_r1cs_bind_rows (full = 1) on its transpose,
            so a row of n entries is also a column of n entries.  s = d = 8 unless the case needs more columns than that: empty rows and an
            empty matrix; one-entry rows; rows of ROW_SPLIT - 1, ROW_SPLIT, ROW_SPLIT + 1 entries (the last lane row, the first workgroup
            row); rows of kRawTermsMax, + 1, twice, twice + 1 entries (70, 71, 140, 141 and 169, 170, 338, 339: d = 9 holds the longest)
            with every value and every operand p - 1, the lengths at which a missed reduction overflows; one full row; every row pointing at
            one column; s = 1; the same entry in A, B and C
  operands  bind_rows at rho = 0 and p - 1 and rx all zero and all p - 1; the witness half equals the first half of the full table
  stride    s = 12, d = 13, three entries a row, at the default grid and again under ZK_R1CS_BLOCKS=1 (read at every call): every lane
            takes 48 items, and a planted long row puts the workgroup kernel on a second item too"""
import random

import numpy as np
import pytest

import _ntt_model as NM
import _r1cs_model as RM
from test_gpu_fri import table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
FIELDS = (0, 3)
T = RM.ROW_SPLIT


def instance(zk, field, s, d, mats):
    return zk.R1CS(field, s, d, *(([e[0] for e in m], [e[1] for e in m], zk.from_ints(field, [e[2] for e in m])) for m in mats))


def check_matvec(zk, field, s, d, mats, z, what):
    inst = instance(zk, field, s, d, mats)
    zt = table_of(zk, field, z)
    got = zk.r1cs.matvec(inst, zt)
    for g, w in zip(got, RM.matvec(field, s, mats, z)):
        assert len(g) == 1 << s and np.array_equal(g.evaluated_values, to_mont(zk, field, w)), what
    assert np.array_equal(zt.evaluated_values, to_mont(zk, field, z)), what


def check_bind(zk, field, s, d, mats, rx, rho, what, inst=None):
    inst = inst or instance(zk, field, s, d, mats)
    full = zk.r1cs.bind_rows(inst, zk.from_ints(field, rx), zk.from_ints(field, [rho])[0], full=True)
    want = RM.bind_rows(field, s, d, mats, rx, rho, full=True)
    assert len(full) == 1 << d and np.array_equal(full.evaluated_values, to_mont(zk, field, want)), what
    half = zk.r1cs.bind_rows(inst, zk.from_ints(field, rx), zk.from_ints(field, [rho])[0])
    assert len(half) == 1 << (d - 1) and np.array_equal(half.evaluated_values, to_mont(zk, field, want[:1 << (d - 1)])), what
    return inst


def row(r, n, v, rng=None, d=None):
    """n entries in row r: the columns 0 .. n - 1, or with rng n distinct ones below 2^d; value v, or with v = None random"""
    cols = rng.sample(range(1 << d), n) if rng else range(n)
    return [(r, c, v) for c in cols]


def shapes(field):
    """(name, s, d, [A, B, C], operand): operand = None for a random table, or the one value every entry of it takes"""
    p = NM.MODULUS[field]
    rng = random.Random(8800 + field)
    val = lambda: rng.randrange(p)
    K = RM.RAW_TERMS_MAX[field]
    out = []
    sparse = [(r, rng.randrange(256), val()) for r in range(0, 256, 3)]
    out.append(("empty rows and an empty matrix", 8, 8, [sparse, [], [(255, 255, val())]], None))
    out.append(("one-entry rows", 8, 8, [[(r, (7 * r + k) % 256, val()) for r in range(256)] for k in range(3)], None))
    edge = [e for r, n in ((3, T - 1), (4, T), (5, T + 1), (200, T + 1)) for e in row(r, n, None, rng, 8)]
    edge = [(r, c, val()) for r, c, _ in edge]
    out.append(("rows at the bin boundary", 8, 8, [edge, [(r, c, val()) for r, c, _ in edge if r != 4], edge[:T - 1]], None))
    dk = 8 if 2 * K + 1 <= 256 else 9
    for op in (p - 1, None):
        long_rows = [e for r, n in ((1, K), (2, K + 1), (130, 2 * K), (131, 2 * K + 1)) for e in row(r, n, p - 1 if op else val(), rng, dk)]
        out.append(("rows at the reduction bound, %s" % ("all p - 1" if op else "random"), 8, dk, [long_rows, long_rows[K:], long_rows[:K + 1]], op))
    out.append(("one full row", 8, 8, [[(77, c, val()) for c in range(256)], [(77, c, p - 1) for c in range(256)], []], None))
    out.append(("every row at one column", 8, 8, [[(r, 9, val()) for r in range(256)], [(r, 255, val()) for r in range(256)], [(r, 0, p - 1) for r in range(256)]], None))
    out.append(("s = 1", 1, 8, [[(0, 5, val()), (1, 5, val())], [(1, c, val()) for c in range(100)], []], None))
    same = [(r, (r * 5) % 256, val()) for r in range(256)] + [(9, c, val()) for c in range(60) if c != 45]
    out.append(("the same entries in A, B and C", 8, 8, [same, same, same], None))
    return out


@pytest.mark.parametrize("field", FIELDS)
def test_matvec_equals_the_model(zk, field):
    for name, s, d, mats, op in shapes(field):
        z = [op] * (1 << d) if op is not None else NM.random_ints(field, 1 << d, 8900 + s + d + field)
        check_matvec(zk, field, s, d, mats, z, name)
    check_matvec(zk, field, 8, 8, shapes(field)[2][3], [0] * 256, "z all zero")


@pytest.mark.parametrize("field", FIELDS)
def test_bind_rows_equals_the_model_on_the_transposed_shapes(zk, field):
    p = NM.MODULUS[field]
    rng = random.Random(9000 + field)
    for name, d, s, mats, op in shapes(field):                # transposed: the rows become columns, 2^s rows and 2^d columns change places
        if d < 2:
            continue
        mats = [RM.transpose(m) for m in mats]
        rx = [p - 1] * s if op is not None else [rng.randrange(p) for _ in range(s)]
        rho = p - 1 if op is not None else rng.randrange(p)
        check_bind(zk, field, s, d, mats, rx, rho, name)
    name, s, d, mats, _ = shapes(field)[-2]                   # "s = 1" has no transpose (d >= 2): two rows as they are
    check_bind(zk, field, s, d, mats, [rng.randrange(p)], rng.randrange(p), name)


@pytest.mark.parametrize("field", FIELDS)
def test_bind_rows_at_the_edge_operands(zk, field):
    p = NM.MODULUS[field]
    rng = random.Random(9100 + field)
    s, d = 8, 8
    name, _, _, mats, _ = shapes(field)[2]
    mats = [RM.transpose(m) + [(r, 17, rng.randrange(p)) for r in range(256)] for m in mats]      # the boundary columns and a full column in each matrix
    inst = None
    for rho in (0, 1, p - 1, rng.randrange(p)):
        for rx in ([0] * s, [p - 1] * s, [1] * s, [rng.choice((0, 1, p - 1, rng.randrange(p))) for _ in range(s)]):
            inst = check_bind(zk, field, s, d, mats, rx, rho, (rho, rx[:2]), inst)


@pytest.mark.parametrize("field", FIELDS)
def test_the_second_trip_of_the_grid_stride_loops(zk, field, monkeypatch):
    p = NM.MODULUS[field]
    s, d = 12, 13
    rng = random.Random(9200 + field)
    mats = [RM.random_matrix(field, s, d, 3, 9300 + k + field) for k in range(3)]
    for k, r in ((0, 11), (1, 4000), (2, 11)):                # long rows for the workgroup kernel: three items on one workgroup under the cap
        have = {c for rr, c, _ in mats[k] if rr == r}
        mats[k] += [(r, c, rng.randrange(p)) for c in rng.sample(sorted(set(range(1 << d)) - have), 300)]
    z = NM.random_ints(field, 1 << d, 9400 + field)
    rx = [rng.randrange(p) for _ in range(d)]
    tr = [RM.transpose(m) for m in mats]
    for cap in (None, "1"):
        if cap:
            monkeypatch.setenv("ZK_R1CS_BLOCKS", cap)
        else:
            monkeypatch.delenv("ZK_R1CS_BLOCKS", raising=False)
        check_matvec(zk, field, s, d, mats, z, ("cap", cap))
        check_bind(zk, field, d, s, tr, rx, rng.randrange(p), ("cap", cap))


def test_the_passes_refuse_a_table_of_another_shape(zk):
    inst = instance(zk, 0, 3, 4, [[(0, 0, 1)], [], []])
    with pytest.raises(zk.ZkError) as e:
        zk.r1cs.matvec(inst, table_of(zk, 0, [1] * 8))
    assert e.value.code == -2                                 # ZK_E_LEN_MISMATCH
    with pytest.raises(zk.ZkError) as e:
        zk.r1cs.matvec(inst, table_of(zk, 3, [1] * 16))
    assert e.value.code == -7
