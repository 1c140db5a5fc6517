"""The planted inputs of tests/test_lookup_hash_cpu.py (which proves that each does what its name says) and tests/test_gpu_lookup_hash.py (which
runs them): tables whose rows are chosen by WHERE THEY HASH, found among the candidates of tests/_lookup_hash_model.py.  Rows are stored words
((n, 24) uint32: T0, T1, T2 of a row side by side).  A case is a dict:

  T           the table's rows, n of them; cap = 2 n
  witnesses   a list of (W, qk): the witness rows and, per row, 1 (looked up), 0, or 2 (a selector that is neither: not counted)
  ..          what the CPU test proves about it: the window of homes, the planted rows' places, the rows that are in no table row

Every builder is deterministic and cached per process; the arrays are shared and must not be written."""
import functools

import numpy as np

import _lookup_hash_model as HM

WAVE, GROUP = 64, 256


class Pool:
    """hands out each candidate at most once"""

    def __init__(self, cap):
        self.cap, self.used = cap, np.zeros(1 << HM.POOL_LOG, bool)

    def available(self, lo, hi):
        idx = HM.pool_with_home(self.cap, lo, hi)
        return int((~self.used[idx]).sum())

    def take(self, count, lo=None, hi=None):
        idx = np.arange(1 << HM.POOL_LOG) if lo is None else HM.pool_with_home(self.cap, lo, hi)
        idx = idx[~self.used[idx]][:count]
        assert len(idx) == count, "the pool has too few candidates with a home in [%s, %s)" % (lo, hi)
        self.used[idx] = True
        return HM.pool_rows(idx)


def place(n, planted, fill):
    """the table with planted[i] at index i (a dict) and the rows of `fill` at the other indices in order"""
    T = np.empty((n, HM.LIMBS), np.uint32)
    free = np.ones(n, bool)
    for i, row in planted.items():
        assert free[i], "two planted rows at index %d" % i
        T[i], free[i] = row, False
    assert free.sum() == len(fill)
    T[free] = fill
    return T


def frozen(case):
    for v in case.values():
        for a in (v if isinstance(v, (list, tuple)) else [v]):
            for b in (a if isinstance(a, tuple) else [a]):
                if isinstance(b, np.ndarray):
                    b.setflags(write=False)
    return case


def every_row_once(T, seed):
    """every table row looked up once, row x holding table row perm[x]"""
    perm = np.random.default_rng(seed).permutation(len(T))
    return T[perm].copy(), np.ones(len(T), np.int64)


@functools.lru_cache(maxsize=None)
def one_home(n):
    """n distinct rows, all with home cap - 1: the chain is half the table and all of it but one slot lies past the wrap"""
    cap = 2 * n
    rows = Pool(cap).take(n + 1, cap - 1, cap)
    T, absent = rows[:n], rows[n]
    W1, q1 = every_row_once(T, 100 + n)
    W2 = W1.copy()
    W2[n // 2] = absent
    return frozen(dict(name="one home at the end, n = %d" % n, T=T, witnesses=[(W1, q1), (W2, q1.copy())], window=(cap - 1, cap), cluster=np.arange(n), absent=absent[None, :]))


CLUSTER = 320                                                 # five whole waves of table rows


@functools.lru_cache(maxsize=None)
def packed(where):
    """n = 2^10: 320 distinct rows with their home in four adjacent slots, at the indices 0 .. 319 (the last four slots: "tail"; the four below
    cap / 2: "middle", the same chain without the wrap).  Witnesses: every table row once; a whole wave of 64 rows that are in no table row, with
    homes in the window, and 70 more scattered among hits; (tail only) six waves with one target each, a planted row, their neighbours mixing hits,
    misses, qK = 0 and qK = 2"""
    n, cap = 1 << 10, 1 << 11
    lo, hi = (cap - 4, cap) if where == "tail" else (cap // 2 - 4, cap // 2)
    pool = Pool(cap)
    cl, wave_abs, sc_cl, sc_rnd = pool.take(CLUSTER, lo, hi), pool.take(64, lo, hi), pool.take(35, lo, hi), pool.take(35)
    T = np.concatenate([cl, pool.take(n - CLUSTER)])
    rng = np.random.default_rng(200 + lo)
    witnesses = [every_row_once(T, 201 + lo)]
    # a wave of misses and 70 scattered ones
    looked = np.where(rng.integers(0, 2, n) == 1, rng.integers(0, CLUSTER, n), rng.integers(0, n, n))
    W, qk = T[looked].copy(), np.ones(n, np.int64)
    qk[np.arange(n) % 11 == 3] = 0
    wave = np.arange(5 * WAVE, 6 * WAVE)
    W[wave], qk[wave] = wave_abs, 1
    rest = np.setdiff1d(np.arange(n), wave)
    at = rng.choice(rest, 70, replace=False)
    W[at], qk[at] = np.concatenate([sc_cl, sc_rnd]), 1
    witnesses.append((W, qk))
    case = dict(name="%s cluster, packed" % where, T=T, window=(lo, hi), cluster=np.arange(CLUSTER), absent=np.concatenate([wave_abs, sc_cl]), miss_wave=wave,
                scattered=np.sort(at))
    if where == "tail":
        waves, targets = (2, 5, 7, 9, 12, 14), (CLUSTER - 1, CLUSTER - 2, CLUSTER - 3, CLUSTER // 2, 1, 0)
        absent = np.concatenate([wave_abs, sc_cl, sc_rnd])
        x = np.arange(n)
        W = T[rng.integers(0, n, n)].copy()
        qk = np.where(x % 4 == 1, 0, np.where(x % 8 == 6, 2, 1))
        miss = x[x % 4 == 0]
        W[miss] = absent[np.arange(len(miss)) % len(absent)]
        for w, t in zip(waves, targets):
            W[w * WAVE:(w + 1) * WAVE], qk[w * WAVE:(w + 1) * WAVE] = T[t], 1
        witnesses.append((W, qk))
        case.update(target_waves=waves, targets=targets)
    return frozen(dict(case, witnesses=witnesses))


@functools.lru_cache(maxsize=None)
def strided():
    """n = 2^14: the planted rows one per wave, at the indices 64 k (every fourth of them at a stride of 256: one per workgroup), their homes in
    the last w slots, w = 8 unless the candidates give fewer than 144 such rows.  Every table row is looked up once, but 16 witness rows hold rows
    that are in no table row and have their home in the window"""
    n, cap = 1 << 14, 1 << 15
    pool = Pool(cap)
    w = next(w for w in (8, 16, 32) if pool.available(cap - w, cap) >= 144)
    count = min(pool.available(cap - w, cap) - 16, n // WAVE)
    cl, absent = pool.take(count, cap - w, cap), pool.take(16, cap - w, cap)
    at = WAVE * np.arange(count)
    T = place(n, dict(zip(at.tolist(), cl)), pool.take(n - count))
    W, qk = every_row_once(T, 300)
    xs = np.random.default_rng(301).choice(n, 16, replace=False)
    W[xs] = absent
    return frozen(dict(name="tail cluster, strided", T=T, witnesses=[(W, qk)], window=(cap - w, cap), cluster=at, absent=absent))


@functools.lru_cache(maxsize=None)
def copies(n):
    """workgroup 0 is 256 distinct rows with their home in the last w slots (w = 4 at n = 2^10); 64 of them stand twice more in the table, each
    copy in another workgroup and so in another wave.  For the first 32 the smallest index is j itself; for the other 32 it is one of the last
    eight lanes of a wave of workgroup 0, behind 56 other planted rows of that wave"""
    cap, groups = 2 * n, n // GROUP
    pool = Pool(cap)
    w = next(w for w in (4, 8, 16, 32) if pool.available(cap - w, cap) >= GROUP + 16)
    cl = pool.take(GROUP, cap - w, cap)
    first = [j if j < 32 else WAVE * ((j - 32) // 8) + 56 + (j - 32) % 8 for j in range(64)]
    second = [GROUP * (1 + j % (groups // 2 - 1 or 1)) + (4 * j + 1) % GROUP for j in range(64)]
    third = [GROUP * (groups // 2 + (j // 32 if groups == 4 else j % 32)) + (8 * j + 6) % GROUP + j // 32 for j in range(64)]
    planted = {}
    for j in range(64):
        for i in (first[j], second[j], third[j]):
            assert i not in planted
            planted[i] = cl[j]
    others = [i for i in range(GROUP) if i not in planted]
    planted.update(zip(others, cl[64:]))
    T = place(n, planted, pool.take(n - len(planted)))
    rng = np.random.default_rng(400 + n)
    pick = np.array([first, second, third])
    looked = np.where(rng.integers(0, 2, n) == 1, pick[rng.integers(0, 3, n), rng.integers(0, 64, n)], rng.integers(0, n, n))
    looked[:64] = third                                       # each copied row at least once, by its largest index
    W, qk = T[looked].copy(), np.where(np.arange(n) % 13 == 5, 0, 1)
    return frozen(dict(name="copies inside a cluster, n = %d" % n, T=T, witnesses=[(W, qk)], window=(cap - w, cap), cluster=np.arange(GROUP),
                       copies=np.array([first, second, third]).T))


TWIN_KINDS = ("any limbs", "T2 only", "the top two limbs of T0 only")


@functools.lru_cache(maxsize=None)
def twin_pairs():
    """-> (a, b, kind): 50 pairs of distinct rows with equal 32-bit hashes.  34 among the candidates (they differ everywhere); 8 that differ in
    T2 only and 8 that differ only in the two top stored limbs of T0, each found among 2^19 variants of one row.  (No pair can differ in ONE limb
    only: murmur3 is a bijection of every single 32-bit word for fixed others.)"""
    def equal_hashes(h, count):
        order = np.argsort(h, kind="stable")
        hit = np.flatnonzero(h[order][1:] == h[order][:-1])
        hit = hit[np.concatenate([[True], np.diff(hit) > 1])][:count]      # disjoint pairs
        assert len(hit) == count, "too few pairs of equal hashes"
        return order[hit], order[hit + 1]

    i, j = equal_hashes(HM.pool_hashes(), 34)
    a, b, kind = [HM.pool_rows(i)], [HM.pool_rows(j)], [0] * 34
    for k, cols in ((1, slice(16, 24)), (2, slice(6, 8))):
        rng = np.random.default_rng([0x7717, k])
        var = np.repeat(HM.chunk(0, stream=1)[k:k + 1], 1 << 19, axis=0)
        var[:, cols] = rng.integers(0, 1 << 32, size=(1 << 19, cols.stop - cols.start), dtype=np.uint32)
        var[:, 7::8] &= np.uint32(HM.TOP)
        i, j = equal_hashes(HM.hash_rows(var), 8)
        a.append(var[i])
        b.append(var[j])
        kind += [k] * 8
    order = np.random.default_rng(0x7718).permutation(50)
    return np.concatenate(a)[order], np.concatenate(b)[order], np.array(kind)[order]


@functools.lru_cache(maxsize=None)
def twins():
    """n = 2^10.  Pair p has its first twin at index 2 p.  p < 25: the second twin is in the table too, at 500 + 3 p, and the first is looked up
    p + 1 times, the second p + 2 times.  p >= 25: the second twin is in no table row and is looked up once (twice for even p): a miss, never a
    hit on its twin; the first is looked up once"""
    n = 1 << 10
    a, b, kind = twin_pairs()
    planted = {2 * p: a[p] for p in range(50)}
    planted.update({500 + 3 * p: b[p] for p in range(25)})
    pool = Pool(2 * n)
    T = place(n, planted, pool.take(n - 75))
    rows = []
    for p in range(50):
        rows += [a[p]] * (p + 1 if p < 25 else 1) + [b[p]] * (p + 2 if p < 25 else 2 - p % 2)
    rows = np.array(rows)
    W, qk = pool.take(n), np.zeros(n, np.int64)
    at = np.random.default_rng(500).choice(n, len(rows), replace=False)
    W[at], qk[at] = rows, 1
    return frozen(dict(name="full-hash twins", T=T, witnesses=[(W, qk)], pairs=(a, b, kind), absent=b[25:]))


@functools.lru_cache(maxsize=None)
def small_tail(n=128, count=40):
    """the packed tail cluster scaled to cap = 256: `count` distinct rows with their home in the last four slots at the indices 0 .. count - 1"""
    cap = 2 * n
    pool = Pool(cap)
    T = np.concatenate([pool.take(count, cap - 4, cap), pool.take(n - count)])
    return frozen(dict(name="tail cluster at cap = %d" % cap, T=T, witnesses=[], window=(cap - 4, cap), cluster=np.arange(count)))
