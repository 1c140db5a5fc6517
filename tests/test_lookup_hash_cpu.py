"""CPU: the planted inputs of tests/test_gpu_lookup_hash.py do what their names say, proved on the model of tests/_lookup_hash_model.py before any
GPU test compares anything with them (in the manner of test_foldk_shadow_cpu.py and test_msm_shadow_cpu.py).  Every property is one that holds
whatever order the rows arrive in:

  model        murmur3's published vectors; hash_rows is the scalar definition on rows of words; Table's occupied set under several insertion
               orders; check_slots accepts every sequential table and refuses a displaced row, a larger index, a lost triple, a doubled one
  one home     n = 2, 4, 8, 64 (and 128, the prover's case): n distinct rows, every home cap - 1; the occupied slots are cap - 1 and 0 .. n - 2, so
               n - 1 rows sit past the wrap; the row that is in no table row has home cap - 1 and walks n slots
  packed       n = 2^10, tail and middle: 320 distinct rows at the indices 0 .. 319 with their home in four slots; tail: at least 316 rows past the
               wrap in every arrival order, every miss of the wave of 64 and 35 of the scattered 70 walks more than 300 slots and across the end;
               middle: the same walks, none across the end, no chain of the table wraps
  strided      n = 2^14: at least 128 distinct rows at the indices 64 k, home in the last w slots; at least their number less w past the wrap; the 16
               misses walk at least that many slots and across the end
  copies       n = 2^10 and 2^14: each of 64 planted rows at three indices, in three workgroups; the smallest is in workgroup 0, for half of them in
               the last eight lanes of its wave behind 56 other planted rows; the model's M is zero at the other copies
  twins        50 pairs of distinct rows with equal 32-bit hashes; among the 25 pairs with both twins in the table and among the 25 with one there
               are pairs that differ in T2 only and pairs that differ only in the two top stored limbs of T0; no pair differs in one limb only,
               and none can: murmur3 is a bijection of any one word
  one target   six waves whose 64 rows all hold one planted row, six different ones: at most four of them sit before the wrap

zk_lookup_hash_slots' statuses that need no device are in tests/test_lookup_cpu.py with the other hooks'."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as G
import _lookup_hash_cases as HC
import _lookup_hash_model as HM
import _lookup_model as LM

zk = G.import_package()
VECTORS = ((b"", 0, 0), (b"", 1, 0x514E28B7), (b"", 0xFFFFFFFF, 0x81F16F39), (b"test", 0, 0xBA6BD213), (b"Hello, world!", 0x9747B28C, 0x24884CBA),
           (b"The quick brown fox jumps over the lazy dog", 0x9747B28C, 0x2FA826CD))


def model_m(case, k, p=1 << 256):
    """the dict model on the stored integers of witness k -> (M, misses)"""
    W, qk = case["witnesses"][k]
    tabs = [HM.stored_ints(c) for c in HM.columns(W)] + [[int(v) for v in qk]] + [HM.stored_ints(c) for c in HM.columns(case["T"])]
    return LM.multiplicities(tabs, p)


def table_of(case):
    return HM.Table(case["T"], 2 * len(case["T"]))


def test_the_hash_model_reproduces_murmur3s_vectors():
    for data, seed, want in VECTORS:
        assert HM.murmur3_32(data, seed) == want, (data, seed)
    rows = HM.chunk(3)[:200]
    assert HM.hash_rows(rows).tolist() == [HM.murmur3_32(r.tobytes(), HM.SEED) for r in rows]
    words = np.frombuffer(b"The quick brown fox jumps over the lazy dog!", np.uint32)[None, :]      # 44 bytes: whole words
    assert int(HM.hash_rows(words, 0x9747B28C)[0]) == HM.murmur3_32(words.tobytes(), 0x9747B28C)
    assert (HM.chunk(5)[:, 7::8] < 1 << 27).all() and np.array_equal(HM.chunk(5), HM.chunk(5))
    assert np.array_equal(HM.pool_rows([5 << 16 | 9, 3, 5 << 16 | 9]), np.stack([HM.chunk(5)[9], HM.chunk(0)[3], HM.chunk(5)[9]]))
    assert int(HM.home(np.uint32(0xFFFFFFF5), 16)) == 5
    # the stored words of a candidate are below both moduli
    for field in (0, 3):
        flat = HM.columns(rows)[2]
        assert np.array_equal(zk.from_ints(field, zk.to_ints(field, flat)), flat)


def sequential(rows, cap, order):
    """the slots after the rows arrive one at a time in `order`, as the insert kernel treats each"""
    slots = np.full(cap, HM.EMPTY, np.uint32)
    hs = HM.home(HM.hash_rows(rows), cap)
    for y in order:
        s = int(hs[y])
        while True:
            if slots[s] == HM.EMPTY:
                slots[s] = y
                break
            if np.array_equal(rows[slots[s]], rows[y]):
                slots[s] = min(slots[s], y)
                break
            s = (s + 1) & (cap - 1)
    return slots


def test_the_occupied_set_does_not_depend_on_the_order():
    rng = np.random.default_rng(7)
    for n, cap in ((2, 4), (8, 16), (64, 128), (300, 1024)):
        rows = HM.chunk(1)[rng.integers(0, 3 * n // 4 + 1, n)]         # repeats among them
        tbl = HM.Table(rows, cap)
        assert tbl.occupied.sum() == len(tbl.first) == len({r.tobytes() for r in rows})
        seen = set()
        for order in (range(n), range(n - 1, -1, -1), rng.permutation(n), rng.permutation(n)):
            slots = sequential(rows, cap, [int(y) for y in order])
            HM.check_slots(slots, rows, tbl)
            seen.add(slots.tobytes())
            perm = np.array([int(y) for y in order])
            assert np.array_equal(HM.Table(rows[perm], cap).occupied, tbl.occupied)
        assert n < 8 or len(seen) > 1                                  # the contents do depend on it
    # one cluster across the wrap, and what check_slots refuses
    case = HC.one_home(8)
    rows, tbl = case["T"], table_of(case)
    good = sequential(rows, 16, range(8))
    HM.check_slots(good, rows, tbl)
    assert good[15] == 0 and good[:7].tolist() == list(range(1, 8))
    twice = np.concatenate([rows[:4], rows[:4]])
    t2 = HM.Table(twice, 16)
    ok = sequential(twice, 16, range(7, -1, -1))
    HM.check_slots(ok, twice, t2)
    bad = {"moved": good.copy(), "lost": good.copy(), "doubled": good.copy(), "no row": good.copy(), "larger index": ok.copy()}
    bad["moved"][[6, 8]] = bad["moved"][[8, 6]]
    bad["lost"][3] = HM.EMPTY
    bad["doubled"][3] = good[4]
    bad["no row"][2] = 8
    at = int(np.flatnonzero(ok == 1)[0])
    bad["larger index"][at] = 5
    for what, slots in bad.items():
        with pytest.raises(AssertionError):
            HM.check_slots(slots, twice if what == "larger index" else rows, t2 if what == "larger index" else tbl)


@pytest.mark.parametrize("n", (2, 4, 8, 64, 128))
def test_one_home_at_the_end(n):
    case, cap = HC.one_home(n), 2 * n
    tbl = table_of(case)
    assert len(tbl.first) == n and set(tbl.home.values()) == {cap - 1} and case["window"] == (cap - 1, cap)
    assert np.flatnonzero(tbl.occupied).tolist() == list(range(n - 1)) + [cap - 1]
    assert tbl.past_the_wrap(1) == n - 1                       # every row but one sits below its home, and so does every lookup but one
    assert tbl.walk(case["absent"][0]) == (cap - 1, n)         # across the end: cap - 1 + n > cap
    assert model_m(case, 0) == ([1] * n, 0)
    m, misses = model_m(case, 1)
    assert misses == 1 and sorted(m) == [0] + [1] * (n - 1)


@pytest.mark.parametrize("where", ("tail", "middle"))
def test_packed_cluster(where):
    case = HC.packed(where)
    n, cap = 1 << 10, 1 << 11
    lo, hi = case["window"]
    tbl = table_of(case)
    assert hi - lo == 4 and hi == (cap if where == "tail" else cap // 2) and len(tbl.first) == n
    assert case["cluster"].tolist() == list(range(320)) and all(lo <= tbl.home[HM.key(case["T"][i])] < hi for i in case["cluster"])
    assert tbl.homes_in(lo, hi) >= 320 and tbl.steps(lo) >= 320
    if where == "tail":
        assert tbl.past_the_wrap(4) >= 316
    else:
        assert tbl.steps(lo) < cap - lo and not (tbl.occupied[0] and tbl.occupied[cap - 1])        # no chain of this table crosses the end
    assert len(case["absent"]) == 99
    for row in case["absent"]:
        h, k = tbl.walk(row)
        assert lo <= h < hi and k > 300 and (h + k >= cap) == (where == "tail")
    assert model_m(case, 0) == ([1] * n, 0)
    W, qk = case["witnesses"][1]
    wave = case["miss_wave"]
    assert wave.tolist() == list(range(320, 384)) and wave[0] % 64 == 0 and np.array_equal(W[wave], case["absent"][:64]) and (qk[wave] == 1).all()
    assert len(case["scattered"]) == 70 and not set(case["scattered"]) & set(wave) and (qk[case["scattered"]] == 1).all()
    m, misses = model_m(case, 1)
    assert misses == 134 and sum(m) == int((qk == 1).sum()) - 134 and (qk == 0).sum() > 50
    miss = np.array([HM.key(r) not in tbl.first and q == 1 for r, q in zip(W, qk)])
    assert sorted(np.flatnonzero(miss)) == sorted(set(wave) | set(case["scattered"]))
    for w in range(n // 64):                                   # no other wave is all misses: the scattered ones take the per-lane path
        assert w == 5 or 0 < miss[64 * w:64 * w + 64].sum() < 64 or not miss[64 * w:64 * w + 64].any()
        assert w == 5 or (~miss[64 * w:64 * w + 64]).any()


def test_one_target_waves_inside_the_tail_cluster():
    case = HC.packed("tail")
    tbl = table_of(case)
    W, qk = case["witnesses"][2]
    lo, hi = case["window"]
    assert len(set(case["targets"])) == 6 and all(t < 320 for t in case["targets"])
    for w, t in zip(case["target_waves"], case["targets"]):
        assert (W[64 * w:64 * w + 64] == case["T"][t]).all() and (qk[64 * w:64 * w + 64] == 1).all()
        assert lo <= tbl.home[HM.key(case["T"][t])] < hi
    # six planted rows, four slots before the end: at least two of the six waves find their row past the wrap, whatever the order
    m, misses = model_m(case, 2)
    assert all(m[t] >= 64 for t in case["targets"])
    for w in range(16):
        if w not in case["target_waves"]:
            q, rows = qk[64 * w:64 * w + 64], W[64 * w:64 * w + 64]
            hit = [HM.key(r) in tbl.first for r in rows]
            assert {0, 1, 2} <= set(q.tolist()) and any(h and v == 1 for h, v in zip(hit, q)) and any(not h and v == 1 for h, v in zip(hit, q))
    assert misses == sum(1 for w in range(16) if w not in case["target_waves"]) * 16


def test_strided_cluster():
    case = HC.strided()
    n, cap = 1 << 14, 1 << 15
    lo, hi = case["window"]
    tbl = table_of(case)
    at = case["cluster"]
    assert hi == cap and hi - lo in (8, 16, 32) and len(tbl.first) == n
    assert len(at) >= 128 and (at % 64 == 0).all() and len(set(at // 64)) == len(at) and (at % 256 == 0).sum() >= 32
    assert all(lo <= tbl.home[HM.key(case["T"][i])] < hi for i in at)
    assert tbl.past_the_wrap(hi - lo) >= len(at) - (hi - lo) >= 96
    for row in case["absent"]:
        h, k = tbl.walk(row)
        assert lo <= h < hi and k >= len(at) - (hi - lo) and h + k >= cap
    m, misses = model_m(case, 0)
    assert misses == 16 and sorted(m) == [0] * 16 + [1] * (n - 16)


@pytest.mark.parametrize("n", (1 << 10, 1 << 14))
def test_copies_inside_a_cluster(n):
    case = HC.copies(n)
    cap = 2 * n
    lo, hi = case["window"]
    tbl = table_of(case)
    T = case["T"]
    assert hi == cap and len(tbl.first) == n - 128 and tbl.homes_in(lo, hi) >= 256 and tbl.past_the_wrap(hi - lo) >= 256 - (hi - lo)
    assert all(lo <= tbl.home[HM.key(T[i])] < hi for i in range(256)) and len({HM.key(T[i]) for i in range(256)}) == 256
    m, misses = model_m(case, 0)
    late = 0
    for j, (a, b, c) in enumerate(case["copies"].tolist()):
        assert HM.key(T[a]) == HM.key(T[b]) == HM.key(T[c]) and tbl.first[HM.key(T[a])] == a < b < c
        assert a < 256 and len({a // 256, b // 256, c // 256}) == 3            # three workgroups, and so three waves
        assert m[a] >= 1 and m[b] == 0 and m[c] == 0
        late += a % 64 >= 56
    assert late == 32 and misses == 0


def test_full_hash_twins():
    a, b, kind = HC.twin_pairs()
    assert a.shape == b.shape == (50, 24) and np.array_equal(HM.hash_rows(a), HM.hash_rows(b))
    assert len({HM.key(r) for r in np.concatenate([a, b])}) == 100
    assert (a[:, 7::8] < 1 << 27).all() and (b[:, 7::8] < 1 << 27).all()
    differ = a != b
    for half in (slice(0, 25), slice(25, 50)):
        assert set(kind[half].tolist()) == {0, 1, 2}
    for p in range(50):
        where = set(np.flatnonzero(differ[p]).tolist())
        assert len(where) >= 2                                 # one differing word cannot keep the hash
        if kind[p] == 1:
            assert where <= set(range(16, 24))
        if kind[p] == 2:
            assert where == {6, 7}                             # the two top stored limbs of T0
    # a bijection of each word: 2^12 values of one limb, the top one of T0 among them, give 2^12 hashes
    for limb in (0, 7, 23):
        var = np.repeat(a[:1], 1 << 12, axis=0)
        var[:, limb] = np.arange(1 << 12)
        assert len(set(HM.hash_rows(var).tolist())) == 1 << 12
    case = HC.twins()
    tbl, T = table_of(case), case["T"]
    assert len(tbl.first) == 1 << 10
    want = [0] * (1 << 10)
    for p in range(50):
        assert HM.key(T[2 * p]) == HM.key(a[p]) and tbl.home[HM.key(a[p])] == int(HM.home(HM.hash_rows(b[p:p + 1]), 1 << 11)[0])
        if p < 25:
            assert HM.key(T[500 + 3 * p]) == HM.key(b[p])
            want[2 * p], want[500 + 3 * p] = p + 1, p + 2
        else:
            assert HM.key(b[p]) not in tbl.first and tbl.walk(b[p])[1] >= 1      # it meets at least its twin
            want[2 * p] = 1
    assert model_m(case, 0) == (want, sum(2 - p % 2 for p in range(25, 50)))


def test_the_small_tail_cluster():
    case = HC.small_tail()
    tbl = table_of(case)
    assert case["window"] == (252, 256) and len(tbl.first) == 128 and tbl.homes_in(252, 256) >= 40 and tbl.past_the_wrap(4) >= 36
    assert all(252 <= tbl.home[HM.key(case["T"][i])] for i in range(40))


def test_the_wrapper_takes_three_tables():
    with pytest.raises(ValueError):
        zk.lookup.hash_slots([None] * 2)
