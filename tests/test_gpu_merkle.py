"""GPU: the Keccak-256 Merkle commitment of a table (csrc/merkle.cuh: one hash per lane).  Root-only mode, the built tree's root and every
opened path equal the Python model of tests/_merkle_model.py byte for byte for all four fields and every length 2^0 .. 2^12; at 2^20 the
root equals the one hashed on the host; at 2^22 and 2^24, where no host model is affordable, the two modes agree and random openings
pass the host-side zk_merkle_verify."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as G
import _merkle_model as MM

pytestmark = pytest.mark.gpu
FIELDS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def zk():
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    return zk


def small_table(zk, field, logn):
    ints = MM.random_ints(field, 1 << logn, 7000 + 16 * field + logn)
    return ints, zk.from_ints(field, ints)


@pytest.mark.parametrize("field", FIELDS)
def test_root_tree_and_paths_equal_the_model(zk, field):
    esz = MM.ELEMENT_BYTES[field]
    host = MM.check_host_keccak(zk)
    rng = np.random.default_rng(field)
    for logn in range(13):
        n = 1 << logn
        ints, mont = small_table(zk, field, logn)
        levels = MM.levels_of([v.to_bytes(esz, "big") for v in ints], MM.M.keccak256 if n <= MM.PURE_PYTHON_MAX else host)
        want = levels[-1][0]
        poly = zk.MultilinearPolynomial(field, mont)
        assert zk.merkle_root(poly) == want, (field, logn)
        tree = zk.MerkleTree.build(poly)
        assert tree.depth == logn and tree.root() == want, (field, logn)
        idx = list(range(min(n, 256))) + ([int(i) for i in rng.integers(256, n, 64)] if n > 256 else [])
        paths = tree.open(idx)
        assert paths.shape == (len(idx), logn, 32)
        for q, i in enumerate(idx):
            assert [paths[q, l].tobytes() for l in range(logn)] == MM.path_of(levels, i), (field, logn, i)
        for q in (0, len(idx) - 1):
            assert zk.MerkleTree.verify(field, want, idx[q], mont[idx[q]], paths[q]) is True


def test_open_and_root_status_codes(zk):
    from zkmle_amd import _lib as L
    lib = zk.lib()
    _, mont = small_table(zk, 0, 4)
    tree = zk.MerkleTree.build(zk.MultilinearPolynomial(0, mont))
    with pytest.raises(zk.ZkError) as ei:
        tree.open([3, 16])
    assert ei.value.code == L.ZK_E_RANGE
    assert tree.open([]).shape == (0, 4, 32)
    three = zk.MultilinearPolynomial.vector(0, mont[:3])                      # not a power of two
    out = np.zeros(32, np.uint8)
    assert lib.zk_mle_merkle_root(three._h, L.p8(out)) == L.ZK_E_NOT_POW2
    h = C.c_void_p()
    assert lib.zk_merkle_build(three._h, C.byref(h)) == L.ZK_E_NOT_POW2
    assert lib.zk_mle_merkle_root(three._h, None) == L.ZK_E_ARG


@pytest.mark.parametrize("field", [0, 1])
def test_2p20_root_equals_the_host_hashed_one(zk, field):
    n = 1 << 20
    poly = zk.MultilinearPolynomial.random(field, n, 0x3E4C1E + field)
    data = poly.convert_to_bytes()
    want = MM.root_of_bytes(data, MM.ELEMENT_BYTES[field], zk)
    assert zk.merkle_root(poly) == want
    tree = zk.MerkleTree.build(poly)
    assert tree.root() == want and tree.depth == 20


@pytest.mark.parametrize("logn", [22, 24])
def test_large_trees_are_consistent_and_open(zk, logn):
    field, n = 0, 1 << logn
    poly = zk.MultilinearPolynomial.random(field, n, 0xA11CE + logn)
    root = zk.merkle_root(poly)
    tree = zk.MerkleTree.build(poly)
    assert tree.root() == root and tree.depth == logn
    rng = np.random.default_rng(logn)
    idx = [0, n - 1] + [int(i) for i in rng.integers(0, n, 62)]
    paths = tree.open(idx)
    # the opened entries, fetched through small views of the table
    from zkmle_amd import _lib as L
    lib = zk.lib()
    base = lib.zk_table_device_ptr(poly._h)
    els = []
    for i in idx:
        h = C.c_void_p()
        L.check(lib.zk_table_wrap(field, C.c_void_p(base + 32 * i), 1, C.byref(h)))
        e = np.zeros(4, np.uint64)
        L.check(lib.zk_table_download(h, L.p64(e)))
        L.check(lib.zk_table_free(h))
        els.append(e)
    for q, i in enumerate(idx):
        assert zk.MerkleTree.verify(field, root, i, els[q], paths[q]) is True, i
    changed = els[5].copy()
    changed[1] ^= np.uint64(1 << 9)
    assert zk.MerkleTree.verify(field, root, idx[5], changed, paths[5]) is False
    assert zk.MerkleTree.verify(field, root, idx[5] ^ 1, els[5], paths[5]) is False


def test_wrapped_table_and_stream_give_the_same_root(zk):
    import torch
    from zkmle_amd import _lib as L
    lib = zk.lib()
    field, n = 0, 1 << 14
    poly = zk.MultilinearPolynomial.random(field, n, 0x57EA)
    want = zk.merkle_root(poly)
    h = C.c_void_p()
    L.check(lib.zk_table_wrap(field, C.c_void_p(lib.zk_table_device_ptr(poly._h)), n, C.byref(h)))   # a non-owning view
    view = zk.MultilinearPolynomial(field, _handle=h)
    assert zk.merkle_root(view) == want
    stream = torch.cuda.Stream()
    L.check(lib.zk_set_stream(C.c_void_p(stream.cuda_stream)))
    try:
        assert zk.merkle_root(view) == want
        tree = zk.MerkleTree.build(view)
        assert tree.root() == want
        del tree
    finally:
        L.check(lib.zk_set_stream(None))
    assert zk.merkle_root(poly) == want
