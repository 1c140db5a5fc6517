"""Python model of the Merkle commitment and of the committed transcript (helpers of tests/test_merkle_cpu.py, test_gpu_merkle.py and
test_gpu_sumcheck_committed.py).  The definition is the one of include/zkmle.h:

  leaf_i = Keccak256(0x00 || e_i as canonical big-endian bytes),  node = Keccak256(0x01 || left || right),  level 0 = the leaves.

The hash is oracle/pymodel.py's pure-Python Keccak-256.  It costs about a millisecond a call, so trees of more than PURE_PYTHON_MAX leaves
are hashed with the library's HOST zk_keccak256 instead: host code pinned by the reference KATs, independent of the device permutation under
test, and checked here against the pure-Python one on inputs of the three sizes a tree hashes."""
import ctypes as C
import hashlib

import numpy as np

from oracle import pymodel as M

PURE_PYTHON_MAX = 1 << 10
ELEMENT_BYTES = {0: 32, 1: 48, 2: 32, 3: 32}
MODULUS = {0: M.P["bls12_381_fr"], 1: M.P["bls12_381_fq"], 2: M.P["bn254_fq"], 3: M.P["bn254_fr"]}
_ROOTS = {}


def host_keccak(zk):
    """the library's host Keccak-256 as bytes -> bytes"""
    lib = zk.lib()
    lib.zk_keccak256.argtypes = [C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint8)]
    lib.zk_keccak256.restype = C.c_int
    out = (C.c_uint8 * 32)()

    def h(data):
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        assert lib.zk_keccak256(buf, len(data), out) == 0
        return bytes(out)
    return h


def check_host_keccak(zk):
    h = host_keccak(zk)
    for n in (33, 49, 65):
        for seed in range(3):
            data = bytes((seed * 131 + 7 * i + n) & 0xFF for i in range(n))
            assert h(data) == M.keccak256(data), (n, seed)
    return h


def levels_of(leaf_bytes, hasher=M.keccak256):
    """leaf_bytes: list of per-element byte strings -> list of levels (lists of 32-byte digests), level 0 first, the root's level last"""
    lv = [hasher(b"\x00" + e) for e in leaf_bytes]
    out = [lv]
    while len(lv) > 1:
        lv = [hasher(b"\x01" + lv[2 * j] + lv[2 * j + 1]) for j in range(len(lv) // 2)]
        out.append(lv)
    return out


def path_of(levels, index):
    return [levels[l][(index >> l) ^ 1] for l in range(len(levels) - 1)]


def verify_path(root, index, leaf, path, hasher=M.keccak256):
    cur = hasher(b"\x00" + leaf)
    for l, sib in enumerate(path):
        cur = hasher(b"\x01" + (sib + cur if (index >> l) & 1 else cur + sib))
    return cur == root


def cut(data, esz):
    data = bytes(data)
    assert len(data) % esz == 0
    return [data[i:i + esz] for i in range(0, len(data), esz)]


def root_of_bytes(data, esz, zk=None):
    """the root of the table whose convert_to_bytes is `data`; big trees through the host Keccak (zk given), results cached"""
    leaves = cut(data, esz)
    key = (esz, hashlib.sha256(bytes(data)).digest())
    if key not in _ROOTS:
        big = len(leaves) > PURE_PYTHON_MAX
        assert not big or zk is not None, "a tree this large needs the host Keccak"
        _ROOTS[key] = levels_of(leaves, check_host_keccak(zk) if big else M.keccak256)[-1][0]
    return _ROOTS[key]


def committed_transcript_class(esz, zk=None, prior=b""):
    """oracle/pymodel.py's Transcript with ONE change: its first append is replaced by the Merkle root of those bytes cut into leaves
    of `esz` bytes.  `prior`: what the transcript had absorbed before the prover was called."""

    class CommittedTranscript(M.Transcript):
        last_root = None

        def __init__(self):
            super().__init__()
            self.buf += prior
            self._bound = False

        def append(self, data):
            if not self._bound:
                self._bound = True
                data = root_of_bytes(data, esz, zk)
                CommittedTranscript.last_root = data
            super().append(data)

    return CommittedTranscript


class patched_transcript:
    """with patched_transcript(cls): oracle/pymodel.py's provers build `cls()` where they build Transcript()"""

    def __init__(self, cls):
        self.cls = cls

    def __enter__(self):
        self.old = M.Transcript
        M.Transcript = self.cls
        return self.cls

    def __exit__(self, *exc):
        M.Transcript = self.old


def to_limbs(field, value):
    """canonical int -> the canonical u64 limbs (NOT Montgomery)"""
    n = ELEMENT_BYTES[field] // 8
    return np.array([(value >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(n)], np.uint64)


def random_ints(field, n, seed, special=True):
    """n canonical values; with `special`, the entries 0, 1 and p - 1 are among them (as far as n allows)"""
    import random
    rng = random.Random(seed)
    p = MODULUS[field]
    v = [rng.randrange(p) for _ in range(n)]
    if special:
        sp = (0, 1, p - 1)
        if n >= 4:
            v[n - 1], v[0], v[n // 2] = sp
        else:                                              # one or two entries: which of the three depends on the seed
            for k in range(n):
                v[k] = sp[(seed + k) % 3]
    return v
