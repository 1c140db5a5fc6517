"""Keccak-256 Merkle commitment of an HBM table (extension: the reference's merkle_tree/ crate is empty; bytes in include/zkmle.h).

  leaf_i = Keccak256(0x00 || convert_to_bytes(e_i)),  node = Keccak256(0x01 || left || right),  root = the node of level log2(len)

With `log_group` = 1 or 2 (32-byte fields) a leaf holds the 2 or 4 entries a FRI fold reads together, e_j, e_{j + len >> log_group}, ..:
a quarter of the hashes, and one path opens the whole group (include/zkmle.h "Merkle commitment with grouped leaves").

`merkle_root(poly)` keeps nothing but the root (what the committed provers bind their transcript to); `MerkleTree.build(poly)` keeps
every level in HBM and opens any number of entries with one kernel and one download; `MerkleTree.verify` is host code.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .mle import limbs


def merkle_root(poly, log_group=0):
    """the 32-byte root of a MultilinearPolynomial's table, root-only mode; log_group: the leaves hold 2^log_group entries each"""
    out = np.zeros(32, np.uint8)
    if log_group == 0:
        L.check(L.lib().zk_mle_merkle_root(poly._h, L.p8(out)))
    else:
        L.check(L.lib().zk_mle_merkle_root_grouped(poly._h, log_group, L.p8(out)))
    return out.tobytes()


def columns_root(tables):
    """the 32-byte root of the ONE tree over the k <= 32 tables (one scalar field, one length 2^d >= 4), root-only mode: leaf j holds
    tables[c][j + s len / 4], s < 4, of every column c (include/zkmle.h "Merkle commitment of several columns")"""
    out = np.zeros(32, np.uint8)
    L.check(L.lib().zk_mle_merkle_root_columns((C.c_void_p * len(tables))(*[t._h for t in tables]), len(tables), L.p8(out)))
    return out.tobytes()


class MerkleTree:
    def __init__(self, handle, field, length, log_group=0):
        self._h, self.field, self.length, self.log_group = handle, field, length, log_group
        self.depth = int(L.lib().zk_merkle_depth(handle))

    @classmethod
    def build(cls, poly, log_group=0):
        """log_group = 1, 2: length >> log_group leaves; open() takes leaf indices and a path authenticates the leaf's 2^log_group entries"""
        h = C.c_void_p()
        if log_group == 0:
            L.check(L.lib().zk_merkle_build(poly._h, C.byref(h)))
        else:
            L.check(L.lib().zk_merkle_build_grouped(poly._h, log_group, C.byref(h)))
        return cls(h, poly.field, len(poly), log_group)

    @classmethod
    def build_columns(cls, tables):
        """ONE tree over k tables: length >> 2 leaves; open() takes leaf indices and a path authenticates the leaf's 4 k entries"""
        h = C.c_void_p()
        L.check(L.lib().zk_merkle_build_columns((C.c_void_p * len(tables))(*[t._h for t in tables]), len(tables), C.byref(h)))
        tree = cls(h, tables[0].field, len(tables[0]), 2)
        tree.columns = len(tables)
        return tree

    @staticmethod
    def verify_columns(field, root, index, elements, path):
        """host only: do the (k, 4, limbs) `elements` of leaf `index` -- column, then side -- hash up `path` ((depth, 32) bytes) to `root`?"""
        root = np.frombuffer(bytes(root), np.uint8).copy()
        if root.shape[0] != 32:
            raise L.ZkError(L.ZK_E_ARG, "a Merkle root is 32 bytes")
        path = np.ascontiguousarray(path, np.uint8).reshape(-1, 32)
        el = np.ascontiguousarray(elements, np.uint64)
        if el.ndim != 3 or el.shape[1:] != (4, limbs(field)):
            raise L.ZkError(L.ZK_E_ARG, "the elements are a (k, 4, limbs) array")
        ok = C.c_int(0)
        buf = path if path.size else np.zeros(32, np.uint8)
        L.check(L.lib().zk_merkle_verify_columns(field, L.p8(root), path.shape[0], int(index), el.shape[0], L.p64(el), L.p8(buf), C.byref(ok)))
        return bool(ok.value)

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                L.lib().zk_merkle_free(self._h)
            except Exception:
                pass
            self._h = None

    def root(self):
        out = np.zeros(32, np.uint8)
        L.check(L.lib().zk_merkle_root(self._h, L.p8(out)))
        return out.tobytes()

    def open(self, indices):
        """-> (len(indices), depth, 32) uint8: for each index its authentication path, the leaf's sibling first"""
        idx = np.ascontiguousarray(indices, np.uint64).reshape(-1)
        out = np.zeros((idx.shape[0], self.depth, 32), np.uint8)
        buf = out if out.size else np.zeros(32, np.uint8)
        L.check(L.lib().zk_merkle_open(self._h, idx.ctypes.data_as(C.POINTER(C.c_size_t)), idx.shape[0], L.p8(buf)))
        return out

    @staticmethod
    def verify(field, root, index, element, path, log_group=0):
        """host only: does `element` (Montgomery limbs) at `index` hash up `path` ((depth, 32) bytes) to `root`?  log_group = 1, 2: `element` is
        the (2^log_group, limbs) entries of leaf `index` in the leaf's order"""
        root = np.frombuffer(bytes(root), np.uint8).copy()
        if root.shape[0] != 32:
            raise L.ZkError(L.ZK_E_ARG, "a Merkle root is 32 bytes")
        path = np.ascontiguousarray(path, np.uint8).reshape(-1, 32)
        el = np.ascontiguousarray(element, np.uint64).reshape(-1)
        if el.shape[0] != limbs(field) << log_group:
            raise L.ZkError(L.ZK_E_ARG, "element has the wrong number of limbs")
        ok = C.c_int(0)
        buf = path if path.size else np.zeros(32, np.uint8)
        if log_group == 0:
            L.check(L.lib().zk_merkle_verify(field, L.p8(root), path.shape[0], int(index), L.p64(el), L.p8(buf), C.byref(ok)))
        else:
            L.check(L.lib().zk_merkle_verify_grouped(field, L.p8(root), path.shape[0], int(index), log_group, L.p64(el), L.p8(buf), C.byref(ok)))
        return bool(ok.value)
