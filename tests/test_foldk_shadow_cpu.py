"""CPU: the integer model of the weighted-sum fold (tests/_foldk_shadow_model.py) and the inputs tests/test_gpu_foldk_edges.py plants.

The model's raw_mont_reduce is checked against a limb-by-limb restatement of the kernel's; the bound floor(2^(29 L) / p) is pinned per
field; and for every committed nonce the model shows lanes at or above 2 p in exactly the forms that summed more terms than the bound
(256 and 128 per reduction on BLS12-381 Fr), and in none once a reduction takes at most 64 terms, nor in the forms that never did."""
import functools
import json
import os
import random

import pytest

import _foldk_shadow_model as FM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = {s[0]: s for s in FM.SHAPES}


@functools.lru_cache(maxsize=None)
def table(field, kind, logn):
    return FM.make_table(field, kind, 1 << logn)


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "foldk_hot_transcripts.json")) as f:
        return json.load(f)["fields"]


def test_terms_per_reduction_bound_per_field():
    assert [FM.terms_max(f) for f in (0, 2, 3)] == [70, 169, 169]
    assert FM.terms_max(1) == 41291124
    for f in range(4):
        p, R = FM.MODULUS[f], FM.radix(f)
        assert FM.terms_max(f) * p < R < (FM.terms_max(f) + 1) * p
    assert [FM.chunk_terms(0, t) for t in (32, 64, 128, 256)] == [32, 64, 64, 64]
    assert [FM.chunk_terms(3, t) for t in (64, 128, 256)] == [64, 128, 128]


def limbwise_mont_reduce(field, acc):
    """csrc/mle_kernels.cuh raw_mont_reduce on normalized 29-bit columns"""
    L, p = FM.ULIMBS[field], FM.MODULUS[field]
    mask = (1 << 29) - 1
    inv = (-pow(p, -1, 1 << 29)) % (1 << 29)
    c = [(acc >> (29 * i)) & mask for i in range(2 * L - 1)] + [acc >> (29 * (2 * L - 1))]
    pl = [(p >> (29 * i)) & mask for i in range(L)]
    for i in range(L):
        m = (c[i] * inv) & mask
        for j in range(L):
            c[i + j] += m * pl[j]
        assert c[i] & mask == 0
        c[i + 1] += c[i] >> 29
    assert all(x < 1 << 64 for x in c)
    return sum(c[L + j] << (29 * j) for j in range(L))


@pytest.mark.parametrize("field", [0, 3])
def test_integer_formula_is_the_limbwise_reduction(field):
    rng = random.Random(7 + field)
    p, R = FM.MODULUS[field], FM.radix(field)
    for acc in [0, p * p, 256 * (p - 1) * (p - 1), R * p - 1] + [rng.randrange(256 * p * p) for _ in range(200)]:
        v = FM.raw_mont_reduce(field, acc)
        assert v == limbwise_mont_reduce(field, acc)
        assert v % p == acc * pow(R, -1, p) % p and acc // R <= v < acc // R + p + 1


@pytest.mark.parametrize("field", [0, 3])
def test_model_of_the_kernel_equals_the_exact_fold_inside_the_bound(field):
    rng = random.Random(11)
    p = FM.MODULUS[field]
    for K, form in ((3, "unsplit"), (5, "unsplit"), (6, "split2"), (7, "split2"), (8, "split8")):
        tab = [rng.choice([0, p - 1, rng.randrange(p)]) for _ in range(4 << K)]
        rs = [rng.randrange(p) for _ in range(K)]
        pl = FM.parts(form, K)
        assert max(len(rg) for rg in pl) <= FM.terms_max(field)
        assert FM.over_range_lanes(field, tab, K, rs, pl) == []
        assert FM.kernel_result(field, tab, K, rs, pl) == FM.fold_exact(field, tab, K, rs)
        # the fold of K variables one at a time (oracle/pymodel.py partial_evaluate, variable 0 first)
        cur = tab
        for r in rs:
            cur = FM.M.partial_evaluate(cur, 0, r, p)
        assert cur == FM.fold_exact(field, tab, K, rs)


@pytest.mark.parametrize("shape", FM.HOT)
def test_committed_nonces_send_lanes_over_range_in_the_forms_above_the_bound(shape):
    """BLS12-381 Fr: 256 terms (unsplit K = 8) and 128 terms (unsplit K = 7, each half of split2 K = 8) per reduction"""
    field = 0
    _, K, logn, _, form = SHAPE[shape]
    p, R = FM.MODULUS[field], FM.radix(field)
    legacy = FM.parts(form, K)
    assert len(legacy[0]) > FM.terms_max(field)
    fixed = FM.parts(form, K, FM.chunk_terms(field, len(legacy[0])))
    assert len(fixed[0]) == 64 and len(fixed) * 64 == 1 << K
    for kind in FM.KINDS:
        entry = fixture()[str(field)][shape][kind]
        tab = table(field, kind, logn)
        rs = FM.first_challenges(field, tab, K, entry["nonce"])
        assert max(FM.weight_sums(field, rs, legacy)) > R, (shape, kind)
        hot = FM.over_range_lanes(field, tab, K, rs, legacy)
        assert len(hot) == entry["lanes"] and len(hot) >= FM.lanes_required(shape, kind), (shape, kind, len(hot))
        want = FM.fold_exact(field, tab, K, rs)
        old = FM.kernel_result(field, tab, K, rs, legacy)
        # what the old forms left: the exact element wherever every part was in range, a congruent one at or above p in the lanes over range
        hs = set(hot)
        assert all(old[j] == want[j] for j in range(len(want)) if j not in hs)
        assert all((old[j] - want[j]) % p == 0 for j in hot)          # (split2: the closing fe_add may absorb one half's extra p)
        assert sum(1 for v in old if v >= p) == entry["stored_at_or_above_p"] >= (1 if FM.lanes_required(shape, kind) else 0)
        assert FM.over_range_lanes(field, tab, K, rs, fixed) == []
        assert FM.kernel_result(field, tab, K, rs, fixed) == want


@pytest.mark.parametrize("shape", [s[0] for s in FM.SHAPES if s[0] not in FM.HOT])
def test_forms_inside_the_bound_stay_in_range_on_the_planted_tables(shape):
    _, K, logn, _, form = SHAPE[shape]
    for field in (0, 3):
        pl = FM.parts(form, K)
        assert len(pl[0]) <= FM.terms_max(field)
        for kind in ("all_pm1", "near"):
            tab = table(field, kind, logn)
            rs = FM.first_challenges(field, tab, K, 0)
            assert FM.over_range_lanes(field, tab, K, rs, pl) == []


def test_bn254_forms_after_the_fix_are_inside_the_bound():
    for shape in FM.HOT:
        _, K, _, _, form = SHAPE[shape]
        per = len(FM.parts(form, K)[0])
        assert FM.chunk_terms(3, per) <= FM.terms_max(3)
