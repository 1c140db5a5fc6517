"""Model of the hash table of the lookup's multiplicity count (csrc/lookup.cuh; include/zkmle.h zk_lookup_hash_slots), a helper of
tests/test_lookup_hash_cpu.py and test_gpu_lookup_hash.py.  Plain Python and numpy; nothing here touches the library.

  hash        murmur3_x86_32 of a row's 96 stored bytes (the 24 little-endian 32-bit limbs of T0, T1, T2 in that order) with seed 0x5EED.
              `murmur3_32(data, seed)` is the scalar definition on any byte string (the published vectors are checked on it);
              `hash_rows(limbs)` is the same function vectorised over rows of whole 32-bit words
  home        h & (cap - 1), cap a power of two
  Table       the linear-probing table over the DISTINCT triples of a list of rows.  The set of occupied slots of such a table does not depend
              on the order the triples arrive in; which triple ends in which slot does.  Only order-independent facts are exposed: `occupied`,
              `home[key]`, `first[key]` (the smallest index of a triple), `walk(row)` (for a triple that is NOT in the table: the number of
              occupied slots from its home to the first empty one) and what follows from them
  check_slots what a device table must satisfy whatever the arrival order was
  candidates  rows drawn from a fixed seed AS STORED WORDS, in chunks that can be drawn again; the top 32-bit limb of every element is below
              2^27, so every element is below both scalar moduli (their top limbs are 0x73EDA753 and 0x30644E72) and one set of stored rows serves
              BLS12-381 Fr and BN254 Fr.  `pool_hashes()` hashes 2^20 of them once per process (about a second)"""
import functools

import numpy as np

SEED = 0x5EED
LIMBS = 24                                                    # three elements of eight 32-bit limbs
EMPTY = 0xFFFFFFFF
C1, C2, C3 = np.uint32(0xCC9E2D51), np.uint32(0x1B873593), np.uint32(0xE6546B64)
M32 = 0xFFFFFFFF


def murmur3_32(data, seed):
    """murmur3_x86_32 of a byte string, as published"""
    rotl = lambda x, k: ((x << k) | (x >> (32 - k))) & M32
    h, n = seed & M32, len(data)
    for i in range(0, n - n % 4, 4):
        k = int.from_bytes(data[i:i + 4], "little")
        k = rotl(k * 0xCC9E2D51 & M32, 15) * 0x1B873593 & M32
        h = (rotl(h ^ k, 13) * 5 + 0xE6546B64) & M32
    if n % 4:
        k = int.from_bytes(data[n - n % 4:], "little")
        h ^= rotl(k * 0xCC9E2D51 & M32, 15) * 0x1B873593 & M32
    h ^= n
    h = (h ^ (h >> 16)) * 0x85EBCA6B & M32
    h = (h ^ (h >> 13)) * 0xC2B2AE35 & M32
    return h ^ (h >> 16)


def _rotl(x, k):
    return (x << np.uint32(k)) | (x >> np.uint32(32 - k))


def hash_rows(limbs, seed=SEED):
    """(rows, words) uint32 -> (rows,) uint32: murmur3_x86_32 of each row's words as little-endian bytes"""
    limbs = np.asarray(limbs, np.uint32)
    assert limbs.ndim == 2
    h = np.full(limbs.shape[0], seed, np.uint32)
    for k in range(limbs.shape[1]):
        w = _rotl(limbs[:, k] * C1, 15) * C2
        h = _rotl(h ^ w, 13) * np.uint32(5) + C3
    h = h ^ np.uint32(4 * limbs.shape[1])
    h = (h ^ (h >> np.uint32(16))) * np.uint32(0x85EBCA6B)
    h = (h ^ (h >> np.uint32(13))) * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def home(h, cap):
    assert cap >= 2 and cap & (cap - 1) == 0
    return h & (cap - 1)


def key(row):
    return np.asarray(row, np.uint32).tobytes()


def columns(rows):
    """(n, 24) uint32 -> the three columns as (n, 4) uint64 arrays of stored words"""
    rows = np.ascontiguousarray(rows, np.uint32)
    return [np.ascontiguousarray(rows[:, 8 * j:8 * j + 8]).view(np.uint64) for j in range(3)]


def stored_ints(col):
    """(n, 4) uint64 stored words -> the integers the words spell (NOT the field elements they stand for: only equality matters)"""
    return [int(a) | int(b) << 64 | int(c) << 128 | int(d) << 192 for a, b, c, d in np.asarray(col, np.uint64).tolist()]


class Table:
    """the table of `rows` ((n, 24) uint32, repeats allowed) at `cap` slots"""

    def __init__(self, rows, cap):
        rows = np.asarray(rows, np.uint32)
        assert rows.ndim == 2 and rows.shape[1] == LIMBS
        self.cap, self.n = cap, len(rows)
        hs = home(hash_rows(rows), cap)
        self.first, self.home = {}, {}
        for y, row in enumerate(rows):
            k = row.tobytes()
            if k not in self.first:
                self.first[k], self.home[k] = y, int(hs[y])
        assert 2 * len(self.first) <= cap
        occ = np.zeros(cap, bool)
        for k in self.first:                                  # any order gives this set
            s = self.home[k]
            while occ[s]:
                s = (s + 1) & (cap - 1)
            occ[s] = True
        self.occupied = occ

    def steps(self, h):
        """the occupied slots from h on, cyclically, before the first empty one"""
        k = 0
        while self.occupied[(h + k) & (self.cap - 1)]:
            k += 1
        return k

    def walk(self, row):
        """for a triple that is not in the table: (its home, the number of occupied slots it passes before the empty one)"""
        assert key(row) not in self.first
        h = int(home(hash_rows(np.asarray(row, np.uint32)[None, :]), self.cap)[0])
        return h, self.steps(h)

    def homes_in(self, lo, hi):
        """the number of distinct triples whose home is in [lo, hi)"""
        return sum(1 for h in self.home.values() if lo <= h < hi)

    def past_the_wrap(self, w):
        """a lower bound, good for every arrival order, on the number of triples that sit at a slot below their home: the triples whose home is
        in the last w slots, less the w slots there are for them before the end"""
        return max(0, self.homes_in(self.cap - w, self.cap) - w)


def check_slots(slots, rows, table):
    """what holds for the slots of a device table over `rows` whatever the arrival order was; raises AssertionError with the first thing wrong"""
    slots, rows = np.asarray(slots, np.uint32), np.asarray(rows, np.uint32)
    cap, mask = table.cap, table.cap - 1
    assert slots.shape == (cap,), "the slots are cap words"
    full = slots != EMPTY
    assert np.array_equal(full, table.occupied), "the occupied set differs from the model's at slots %s" % np.flatnonzero(full != table.occupied)[:8]
    at = np.flatnonzero(full)
    ys = slots[at]
    assert (ys < len(rows)).all(), "a slot holds an index that is no row"
    keys = [rows[y].tobytes() for y in ys]
    for s, y, k in zip(at, ys, keys):
        assert table.first[k] == y, "slot %d holds index %d, not the smallest index %d of its triple" % (s, y, table.first[k])
    assert len(set(keys)) == len(keys) == len(table.first), "a triple is in no slot or in two"
    run = np.zeros(cap, np.int64)                             # the occupied slots that end at s, cyclically (cap: never, the table is half empty)
    k = 0
    for s in list(range(cap)) * 2:
        k = k + 1 if full[s] else 0
        run[s] = max(run[s], k)
    for s, k in zip(at, keys):
        assert ((int(s) - table.home[k]) & mask) < run[s], "an empty slot lies between home %d and slot %d" % (table.home[k], s)


# ---- candidates ---------------------------------------------------------------------------------------------------------------------------
POOL_LOG, CHUNK_LOG = 20, 16
TOP = (1 << 27) - 1


def chunk(c, stream=0):
    """candidate rows c 2^16 .. (c + 1) 2^16 - 1 as stored words"""
    a = np.random.default_rng([0x10CA7, stream, c]).integers(0, 1 << 32, size=(1 << CHUNK_LOG, LIMBS), dtype=np.uint32)
    a[:, 7::8] &= np.uint32(TOP)
    return a


@functools.lru_cache(maxsize=None)
def pool_hashes():
    h = np.concatenate([hash_rows(chunk(c)) for c in range(1 << (POOL_LOG - CHUNK_LOG))])
    h.setflags(write=False)
    return h


def pool_rows(idx):
    """the candidate rows of the given numbers, in that order"""
    idx = np.asarray(idx, np.int64)
    out = np.empty((len(idx), LIMBS), np.uint32)
    for c in np.unique(idx >> CHUNK_LOG):
        sel = np.flatnonzero(idx >> CHUNK_LOG == c)
        out[sel] = chunk(int(c))[idx[sel] & ((1 << CHUNK_LOG) - 1)]
    return out


def pool_with_home(cap, lo, hi):
    """the numbers of the candidates whose home at `cap` is in [lo, hi), ascending"""
    h = home(pool_hashes(), cap)
    return np.flatnonzero((h >= lo) & (h < hi))
