"""GPU: the hash table of the lookup's multiplicity count (csrc/lookup.cuh lookup_insert_kernel, lookup_count_kernel, lookup_hash; launched by
csrc/lookup_driver.cuh) on tables whose rows are chosen by WHERE THEY HASH, over BLS12-381 Fr and BN254 Fr.  tests/test_gpu_lookup.py chooses the
values of the rows and leaves their slots to chance: half-full tables with uniform homes have insert probes of at most 21, 31 and 33 slots at
n = 2^6, 2^10 and 2^14 (40 simulated tables each) and step from slot cap - 1 to slot 0 in 9, 6 and 4 of the 40, with chains of a few slots.  Here
the rows come from tests/_lookup_hash_cases.py, found with the model of the hash in tests/_lookup_hash_model.py; tests/test_lookup_hash_cpu.py
proves what each case plants.  Everything is byte for byte; no tolerance anywhere.

Every case: the rows are uploaded as stored words; zk_lookup_hash_slots (the provers' own set-up and insert launch) twice, and each time the
occupied set equals the model's -- which ties the device's hash and probing to the model's: were they different, this would fail and the planted
cases would not silently be random ones --, every occupied slot holds the smallest index of its triple, every distinct triple is in exactly one
slot, and no empty slot lies between a triple's home and its slot (which triple sits where in a chain depends on the arrival order and is not
compared); then, per witness, zk_lookup_multiplicities twice with M and misses equal to the dict model's (tests/_lookup_model.py on the stored
integers: only equality matters; qK of a counted row is the stored one); the inputs are read back unchanged.

  one home     n = 2, 4, 8, 2^6: every row's home is cap - 1; the chain is half the table, all but one slot past the wrap; a miss walks n slots
  packed       n = 2^10: 320 rows with their home in the last four slots at the indices 0 .. 319 (whole waves compete for the same empty slots);
               a whole wave of misses with homes there (the one-target shortcut with target "empty" after more than 300 slots through the wrap)
               and 70 scattered ones; and the same around cap / 2, the long chain without the wrap
  one target   six waves whose rows all hold one planted row (the shortcut with a hit inside a long wrapped chain), neighbours mixing hits,
               misses, qK = 0 and qK = 2
  strided      n = 2^14: one planted row per wave and per workgroup, homes in the last slots
  copies       n = 2^10, 2^14: 64 planted rows three times each, in three workgroups; M at the smallest index, zero at the other copies
  twins        50 pairs with equal 32-bit hashes, 25 with both twins in the table and 25 with one: the other is a miss, never a hit on its twin
  provers      zk.lookup.prove at d = 7 on a one-home table and zk.plonk_lookup.prove at d = 7 on a tail cluster at cap = 256: every output
               equals the Python model's and the host verifier accepts"""
import random

import numpy as np
import pytest

import _fri_ml_cases as FC
import _fri_pcs_model as PM
import _lookup_hash_cases as HC
import _lookup_hash_model as HM
import _lookup_model as LM
import _ntt_model as NM
import _plonk_lookup_model as KL
import _plonk_model as KM
import _zerocheck_gate_model as ZG
import test_gpu_lookup as TL
import test_gpu_plonk_lookup as TP
from test_gpu_fri import table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
FIELDS = (0, 3)
CASES = [(HC.one_home, 2), (HC.one_home, 4), (HC.one_home, 8), (HC.one_home, 64), (HC.packed, "tail"), (HC.packed, "middle"), (HC.strided,), (HC.copies, 1 << 10),
         (HC.copies, 1 << 14), (HC.twins,)]
_reference = {}


def reference(case):
    """the model's table and, per witness, the dict model's (M, misses) on the stored integers: once per case, for both fields"""
    if case["name"] not in _reference:
        T = [HM.stored_ints(c) for c in HM.columns(case["T"])]
        wants = [LM.multiplicities([HM.stored_ints(c) for c in HM.columns(W)] + [[int(v) for v in qk]] + T, 1 << 256) for W, qk in case["witnesses"]]
        _reference[case["name"]] = (HM.Table(case["T"], 2 * len(case["T"])), wants)
    return _reference[case["name"]]


def upload(zk, field, rows):
    return [zk.MultilinearPolynomial(field, np.ascontiguousarray(c)) for c in HM.columns(rows)]


def selector(zk, field, qk):
    """0 -> zero, 1 -> the stored one, 2 -> the stored two"""
    return zk.MultilinearPolynomial(field, np.ascontiguousarray(zk.from_ints(field, [0, 1, 2])[np.asarray(qk)]))


def run_case(zk, field, case):
    T, n = case["T"], len(case["T"])
    tbl, wants = reference(case)
    dev_t = upload(zk, field, T)
    for turn in range(2):
        slots = zk.lookup.hash_slots(dev_t)
        assert slots.dtype == np.uint32
        HM.check_slots(slots, T, tbl)
    for (W, qk), (want, lost) in zip(case["witnesses"], wants):
        dev = upload(zk, field, W) + [selector(zk, field, qk)] + dev_t
        before = [t.evaluated_values.copy() for t in dev]
        want_m = to_mont(zk, field, want)
        for turn in range(2):
            m, misses = zk.lookup.multiplicities(dev)
            assert len(m) == n and np.array_equal(m.evaluated_values, want_m), (case["name"], turn)
            assert misses == lost, (case["name"], turn)
        for t, b, c in zip(dev, before, HM.columns(W) + [before[3]] + HM.columns(T)):
            assert np.array_equal(t.evaluated_values, b) and np.array_equal(b, c), case["name"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join([c[0].__name__] + [str(a) for a in c[1:]]))
@pytest.mark.parametrize("field", FIELDS)
def test_planted_tables(zk, field, case):
    run_case(zk, field, case[0](*case[1:]))


# ---- through the provers ------------------------------------------------------------------------------------------------------------------
def ints_of(zk, field, rows):
    """the three columns of stored rows as the integers they stand for in `field`; their stored form is the planted words again"""
    out = []
    for c in HM.columns(rows):
        ints = [int(v) for v in zk.to_ints(field, np.ascontiguousarray(c))]
        assert np.array_equal(to_mont(zk, field, ints), c)
        out.append(ints)
    return out


@pytest.mark.parametrize("field", FIELDS)
def test_lookup_prove_on_a_one_home_table(zk, field):
    d, b, f, a = 7, 1, 1, 1
    case = HC.one_home(1 << d)
    W, qk = case["witnesses"][0]
    tabs = ints_of(zk, field, W) + [[int(v) for v in qk]] + ints_of(zk, field, case["T"])
    assert LM.multiplicities(tabs, NM.MODULUS[field]) == ([1] * (1 << d), 0)
    cms = [PM.commit(field, t, b, 1, TL.hasher(zk)) for t in tabs]
    pr = LM.prove(cms, f, TL.Q, a, None, TL.hasher(zk))
    assert LM.verify(pr, hasher=TL.hasher(zk)) == (True, None)
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    try:
        HM.check_slots(zk.lookup.hash_slots([table_of(zk, field, t) for t in tabs[4:]]), case["T"], reference(case)[0])
        got = TL.lookup_prove(zk, gcs, f, a)
        TL.assert_same_proof(zk, got, pr)
        assert zk.lookup.verify([gc.root for gc in gcs], got) and zk.lookup.last_stats()["misses"] == 0
    finally:
        for gc in gcs:
            gc.free()


@pytest.mark.parametrize("field", FIELDS)
def test_plonk_lookup_prove_on_a_tail_cluster(zk, field):
    """a circuit whose wiring is one 3-cycle; the rows 3 .. 62 are lookup rows: cells no cycle passes through hold a table row, the selectors are
    random with qC solved for them.  The first 40 look up the 40 planted rows, the others rows anywhere in the table"""
    d, b, f, a, l = 7, 1, 1, 1, 2
    p, n, rng = NM.MODULUS[field], 1 << d, random.Random(18700 + field)
    case = HC.small_tail()
    T = ints_of(zk, field, case["T"])
    tabs, pub = KM.circuit(field, d, 18800 + field, l, "3-cycle")
    qK = [0] * n
    for x in range(3, 63):
        y = x - 3 if x - 3 < 40 else rng.randrange(n)
        row = [rng.randrange(p) for _ in range(4)]
        for j in range(3):
            tabs[j][x] = T[j][y]
        row.append(-ZG.gate(T[0][y], T[1][y], T[2][y], *row, 0) % p)
        for j, v in enumerate(row):
            tabs[3 + j][x] = v
        qK[x] = 1
    tabs = tabs + [qK] + T
    assert KL.satisfied(tabs, pub, p) == (True, True, True)
    m, misses = LM.multiplicities(KL.lookup_tables(tabs), p)
    assert misses == 0 and all(v >= 1 for v in m[:40]) and sum(m) == 60
    cms = [PM.commit(field, t, b, 1, TP.hasher(zk)) for t in tabs]
    pr = KL.prove(cms, pub, f, TP.Q, a, None, TP.hasher(zk))
    assert KL.verify(pr, hasher=TP.hasher(zk)) == (True, None)
    gcs = [FC.gpu_commitment(zk, cm) for cm in cms]
    pm = to_mont(zk, field, pub)
    try:
        HM.check_slots(zk.lookup.hash_slots([table_of(zk, field, t) for t in T]), case["T"], HM.Table(case["T"], 2 * n))
        got = TP.gpu_prove(zk, gcs, pm, f, a)
        TP.assert_same_proof(zk, got, pr)
        assert zk.plonk_lookup.verify([gc.root for gc in gcs], pm, got) and zk.plonk_lookup.last_stats()["misses"] == 0
        assert TP.check_helpers(zk, field, cms, got, b, 1, False) == 0
    finally:
        for gc in gcs:
            gc.free()
