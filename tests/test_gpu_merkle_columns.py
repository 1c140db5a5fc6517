"""GPU: the Merkle tree over several columns (csrc/merkle_columns.cuh merkle_leaf_columns_kernel; include/zkmle.h "Merkle commitment of several
columns") against the model of tests/_fri_ml_columns_model.py, byte for byte, over BLS12-381 Fr and BN254 Fr.

  every k   k = 1 .. 32 at len 2^2 (one leaf: depth 0, root = leaf) and 2^4: the smallest sizes that reach every position of the message's end
            in the rate -- k = 1 (the pad in the rate's last word), 16, 17 (a last block of the carry byte and the pad alone), 18 and 32 among
            them; the root in build mode and in root-only mode, EVERY node through the paths of all leaves, the paths checked by
            zk_merkle_verify_columns; the input tables are only read
  2^12      k = 1, 2, 17 and 32: 2^10 leaves, several workgroups and the first merkle_node_kernel launch
  tables    random with 0, 1 and p - 1 among the entries; all 0; all p - 1
  k = 1     the root of zk_mle_merkle_root_grouped(t, 2), and its every path
  stride    one child process (tests/_columns_worker.py) with ZK_MERKLE_COLUMNS_BLOCKS=2: trees over 2^12 entries at k = 3 and 17 on the
            second trip of the kernel's grid-stride loop
  statuses  ZK_E_ARG, ZK_E_LEN_MISMATCH, ZK_E_NOT_POW2 in that order"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _fri_ml_columns_model as CM
import _merkle_model as MM
import _ntt_model as NM
from test_gpu_fri import table_of, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
FIELDS = (0, 3)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_tree(zk, field, cols, hasher, every_path=True):
    """the library's tree over `cols` (canonical ints) against the model's: root, root-only root, every node, paths by the host verifier"""
    k, n = len(cols), len(cols[0])
    part, depth = n >> 2, n.bit_length() - 3
    levels = CM.levels_of(cols, hasher)
    want = levels[-1][0]
    dev = [table_of(zk, field, c) for c in cols]
    before = [t.evaluated_values for t in dev]
    tree = zk.MerkleTree.build_columns(dev)
    assert tree.depth == depth and tree.columns == k
    assert tree.root() == want, k
    assert zk.merkle.columns_root(dev) == want, k
    paths = tree.open(np.arange(part))
    assert paths.shape == (part, depth, 32)
    for l in range(depth):                                    # every node below the root is some leaf's sibling at its level
        lv = np.frombuffer(b"".join(levels[l]), np.uint8).reshape(-1, 32)
        assert np.array_equal(paths[:, l], lv[(np.arange(part) >> l) ^ 1]), (k, l)
    if depth == 0:
        assert want == levels[0][0]
    mont = np.stack([b.reshape(4, part, -1) for b in before])  # mont[c, s, j] = f_c[j + s part]
    for j in (range(part) if every_path and part <= 4 else sorted({0, part - 1, part // 2})):
        assert zk.MerkleTree.verify_columns(field, want, j, mont[:, :, j], paths[j]), (k, j)
        if part > 1:
            assert not zk.MerkleTree.verify_columns(field, want, j ^ 1, mont[:, :, j], paths[j])
            assert not zk.MerkleTree.verify_columns(field, want, j, mont[:, :, j ^ 1], paths[j])
    assert all(np.array_equal(t.evaluated_values, b) for t, b in zip(dev, before))   # only read
    return want, dev, paths


@pytest.mark.parametrize("loglen", (2, 4))
@pytest.mark.parametrize("field", FIELDS)
def test_every_k_equals_the_model(zk, field, loglen):
    hasher = CM.check_host_keccak(zk)
    cols = [MM.random_ints(field, 1 << loglen, 8100 + 100 * field + 10 * loglen + c) for c in range(32)]
    for k in range(1, 33):
        check_tree(zk, field, cols[:k], hasher)


@pytest.mark.parametrize("k", (1, 2, 17, 32))
@pytest.mark.parametrize("field", FIELDS)
def test_two_to_the_twelve(zk, field, k):
    hasher = CM.check_host_keccak(zk)
    check_tree(zk, field, [MM.random_ints(field, 1 << 12, 8300 + 100 * field + c) for c in range(k)], hasher)


@pytest.mark.parametrize("field", FIELDS)
def test_constant_tables(zk, field):
    hasher = CM.check_host_keccak(zk)
    p = NM.MODULUS[field]
    for loglen, ks in ((2, range(1, 33)), (4, range(1, 33)), (12, (1, 17, 32))):
        for v in (0, p - 1):
            for k in ks:
                cur = hasher(b"\x00" + CM.be32(v) * (4 * k))  # every level of constant tables is one digest repeated
                for _ in range(loglen - 2):
                    cur = hasher(b"\x01" + cur + cur)
                dev = [table_of(zk, field, [v] * (1 << loglen))] * k
                assert zk.merkle.columns_root(dev) == cur, (loglen, k, v == 0)
    # zeros beside p - 1 beside random: every column keeps its place
    n = 16
    cols = [[0] * n, [p - 1] * n, MM.random_ints(field, n, 8500 + field), [p - 1] * n, [0] * n]
    check_tree(zk, field, cols, hasher)


@pytest.mark.parametrize("field", FIELDS)
def test_one_column_is_the_grouped_quad_tree(zk, field):
    for loglen in (2, 3, 4, 10, 12):
        poly = table_of(zk, field, MM.random_ints(field, 1 << loglen, 8600 + field + loglen))
        grouped, cols = zk.MerkleTree.build(poly, log_group=2), zk.MerkleTree.build_columns([poly])
        assert cols.depth == grouped.depth == loglen - 2
        assert cols.root() == grouped.root() == zk.merkle_root(poly, log_group=2) == zk.merkle.columns_root([poly])
        idx = np.arange(1 << (loglen - 2))
        assert np.array_equal(cols.open(idx), grouped.open(idx))


def test_the_second_trip_of_the_grid_stride_loop():
    e = dict(os.environ, ZK_MERKLE_COLUMNS_BLOCKS="2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_columns_worker.py")], capture_output=True, text=True, env=e, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["trips"] == 2, out
    assert out["mismatches"] == [] and out["checked"] == 8, out


def test_the_statuses(zk):
    from zkmle_amd import _lib as L
    t8 = [table_of(zk, 0, MM.random_ints(0, 8, 40 + j)) for j in range(33)]
    t4, t2 = table_of(zk, 0, [1, 2, 3, 4]), table_of(zk, 0, [1, 2])
    other, fq, wide = table_of(zk, 3, MM.random_ints(3, 8, 50)), table_of(zk, 2, MM.random_ints(2, 8, 51)), table_of(zk, 1, MM.random_ints(1, 8, 52))

    def code(fn, tables):
        with pytest.raises(L.ZkError) as e:
            fn(tables)
        return e.value.code

    for fn in (zk.MerkleTree.build_columns, zk.merkle.columns_root):
        assert code(fn, t8) == L.ZK_E_ARG                     # k = 33
        assert code(fn, []) == L.ZK_E_ARG
        assert code(fn, [t8[0], other]) == L.ZK_E_ARG and code(fn, [fq]) == L.ZK_E_ARG and code(fn, [wide]) == L.ZK_E_ARG
        assert code(fn, [t2]) == L.ZK_E_ARG and code(fn, [t8[0], t2]) == L.ZK_E_ARG   # len < 4 before the lengths are compared
        assert code(fn, [t8[0], t4]) == L.ZK_E_LEN_MISMATCH
        fn(t8[:32])
    # a length that is no power of two: a view of six of a table's eight entries
    import ctypes as C
    h = C.c_void_p()
    L.check(zk.lib().zk_table_wrap(0, C.c_void_p(zk.lib().zk_table_device_ptr(t8[0]._h)), 6, C.byref(h)))
    out, root = C.c_void_p(), np.zeros(32, np.uint8)
    arr = (C.c_void_p * 2)(h, h)
    assert zk.lib().zk_merkle_build_columns(arr, 2, C.byref(out)) == L.ZK_E_NOT_POW2 and zk.lib().zk_mle_merkle_root_columns(arr, 2, L.p8(root)) == L.ZK_E_NOT_POW2
    assert not out.value and not root.any()
    zk.lib().zk_table_free(h)
    tree = zk.MerkleTree.build_columns(t8[:3])
    with pytest.raises(L.ZkError) as e:
        tree.open([2])                                        # 2 leaves: an index is a leaf's
    assert e.value.code == L.ZK_E_RANGE
