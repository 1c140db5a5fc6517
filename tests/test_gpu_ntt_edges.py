"""GPU: the number-theoretic transform (csrc/ntt.cuh) on structured tables, which uniform values never produce: butterflies whose
difference is 0, whose sum wraps to 0, whose product is 0; whole tiles of p - 1; deltas, whose output is a pure power of the twiddle and
the twist, so that an index error has nothing to cancel against.  All four transforms (forward, inverse, coset forward, coset inverse),
both scalar fields, one size for every plan of zkmle_ntt.hip make_plan:

  2^0, 2^1, 2^2, 2^10 one launch | 2^11 two passes | 2^13 the first two-level twist table | 2^16 three passes | 2^9 with 4-bit digits

Up to 2^13 the reference is tests/_ntt_model.py, unchanged.  A delta at i is compared with the closed form written out here with Python
integers -- forward out[k] = c^i w^(i k), inverse out[j] = c^-j w^(-i j) / n -- at every size above and, forward and coset forward, at
2^20.  Everything is byte for byte."""
import os
import random

import numpy as np
import pytest

import _ntt_model as NM
from test_gpu_ntt import table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

gpu = pytest.mark.gpu                                      # the two closed-form checks below need no device
FIELDS = (0, 3)
MODEL_LOGS = (0, 1, 2, 10, 11, 13)
DELTA_LOGS = MODEL_LOGS + (16,)


def cosets_of(field, logn):
    """(name, c): p - 1, w_n, w_2n and an element of order dividing n that is not w_n (w_n^3; w_2 = -1 at n = 2; 1 at n = 1)"""
    p = NM.MODULUS[field]
    w = NM.root_of_unity(field, logn)
    return [("p - 1", p - 1), ("w_n", w), ("w_2n", NM.root_of_unity(field, logn + 1)), ("c^n = 1", pow(w, 3, p))]


def transform_and_compare(zk, field, poly, values, inverse, coset, what):
    cm = None if coset is None else zk.from_ints(field, [coset])[0]
    got = zk.ntt.ntt(poly, inverse, cm).evaluated_values
    want = to_mont(zk, field, NM.ntt(field, values, inverse, 1 if coset is None else coset))
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert got.shape == want.shape and bad.size == 0, (what, bad[:8].tolist(), bad.size)
    return got


def structured_tables(field, logn):
    p, n = NM.MODULUS[field], 1 << logn
    h = n // 2
    rnd = NM.random_ints(field, n, 7700 + logn + field)
    out = [("all 0", [0] * n), ("all p - 1", [p - 1] * n), ("constant", [rnd[0] or 5] * n), ("alternating 1, p - 1", ([1, p - 1] * n)[:n]),
           ("upper half zero", rnd[:h] + [0] * (n - h)), ("lower half zero", [0] * h + rnd[h:])]
    for k in sorted({0, 1 % n, h, n - 1}):                    # the forward transform of these is the delta at k: almost every butterfly cancels
        delta = [0] * n
        delta[k] = 1
        out.append(("inverse transform of the delta at %d" % k, NM.ntt(field, delta, True)))
    return out


def run_structured(zk, field, logn):
    cosets = cosets_of(field, logn)
    for j, (tname, values) in enumerate(structured_tables(field, logn)):
        poly = table_of(zk, field, to_mont(zk, field, values))
        cname, c = cosets[j % 4]
        for inverse in (False, True):
            got = transform_and_compare(zk, field, poly, values, inverse, None, (field, logn, tname, inverse, "no coset"))
            transform_and_compare(zk, field, poly, values, inverse, c, (field, logn, tname, inverse, cname))
            if tname.startswith("inverse transform of the delta") and not inverse:
                k = int(tname.rsplit(" ", 1)[1])
                assert not got[np.arange(len(values)) != k].any() and np.array_equal(got[k], zk.from_ints(field, [1])[0]), tname


@gpu
@pytest.mark.parametrize("logn", MODEL_LOGS)
@pytest.mark.parametrize("field", FIELDS)
def test_structured_tables_transform_as_the_model(zk, field, logn):
    """every table under the four transforms; the coset rotates with the table, so each of the four is met at least twice a size"""
    run_structured(zk, field, logn)


@gpu
@pytest.mark.parametrize("field", FIELDS)
def test_structured_tables_under_plans_of_more_passes(zk, field):
    assert "ZK_NTT_MAX_DIGIT_BITS" not in os.environ
    os.environ["ZK_NTT_MAX_DIGIT_BITS"] = "4"
    try:
        run_structured(zk, field, 9)
        run_deltas(zk, field, 9)
    finally:
        del os.environ["ZK_NTT_MAX_DIGIT_BITS"]


@gpu
@pytest.mark.parametrize("logn", MODEL_LOGS)
@pytest.mark.parametrize("field", FIELDS)
def test_every_coset_on_a_uniform_table_and_a_table_of_p_minus_1(zk, field, logn):
    p, n = NM.MODULUS[field], 1 << logn
    for tname, values in (("uniform", NM.random_ints(field, n, 7800 + logn + field)), ("all p - 1", [p - 1] * n)):
        poly = table_of(zk, field, to_mont(zk, field, values))
        for cname, c in cosets_of(field, logn) + [("explicit 1", 1)]:
            for inverse in (False, True):
                got = transform_and_compare(zk, field, poly, values, inverse, c, (field, logn, tname, inverse, cname))
                if c == 1:                                    # the bytes that no coset gives
                    assert np.array_equal(got, zk.ntt.ntt(poly, inverse, None).evaluated_values), (field, logn, tname, inverse)


# ---- deltas against the closed form ----------------------------------------------------------------------------------------------------
def powers(p, first, ratio, n):
    out, x = [], first % p
    for _ in range(n):
        out.append(x)
        x = x * ratio % p
    return out


def delta_closed_form(field, logn, i, inverse, c):
    """the transform of the table that is 1 at i and 0 elsewhere"""
    p, n = NM.MODULUS[field], 1 << logn
    w = NM.root_of_unity(field, logn)
    if not inverse:
        return powers(p, pow(c, i, p), pow(w, i, p), n)                               # out[k] = c^i w^(i k)
    return powers(p, pow(n, -1, p), pow(c, -1, p) * pow(w, -i, p) % p, n)             # out[j] = c^-j w^(-i j) / n


def delta_positions(n):
    return sorted({0, 1 % n, max(n // 2 - 1, 0), n // 2, n - 1})


def run_deltas(zk, field, logn, positions=None, transforms=((False, False), (False, True), (True, False), (True, True))):
    p, n = NM.MODULUS[field], 1 << logn
    c = random.Random(7900 + logn + field).randrange(2, p)
    cm, one = zk.from_ints(field, [c])[0], zk.from_ints(field, [1])[0]
    for i in delta_positions(n) if positions is None else positions:
        data = np.zeros((n, 4), np.uint64)
        data[i] = one
        poly = table_of(zk, field, data)
        for inverse, with_coset in transforms:
            got = zk.ntt.ntt(poly, inverse, cm if with_coset else None).evaluated_values
            want = to_mont(zk, field, delta_closed_form(field, logn, i, inverse, c if with_coset else 1))
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (field, logn, i, inverse, with_coset, bad[:8].tolist(), bad.size)


def test_the_closed_form_is_the_models_transform_of_a_delta():
    for field in FIELDS:
        for logn in (0, 1, 2, 5):
            for i in delta_positions(1 << logn):
                delta = [0] * (1 << logn)
                delta[i] = 1
                for inverse in (False, True):
                    for c in (1, 12345):
                        assert delta_closed_form(field, logn, i, inverse, c) == NM.ntt(field, delta, inverse, c)


@gpu
@pytest.mark.parametrize("logn", DELTA_LOGS)
@pytest.mark.parametrize("field", FIELDS)
def test_deltas_transform_to_pure_powers(zk, field, logn):
    run_deltas(zk, field, logn)


@gpu
@pytest.mark.parametrize("i", delta_positions(1 << 20))
@pytest.mark.parametrize("field", FIELDS)
def test_deltas_transform_to_pure_powers_at_2p20(zk, field, i):
    run_deltas(zk, field, 20, positions=(i,), transforms=((False, False), (False, True)))


# ---- the low-degree extension ----------------------------------------------------------------------------------------------------------
def extension_of_all_p_minus_1(field, logn, lb, c):
    """closed form: -(1 + x + .. + x^(n - 1)) at x = c w_N^k, N = n 2^lb: -(x^n - 1) / (x - 1), and -n at x = 1"""
    p, n, N = NM.MODULUS[field], 1 << logn, 1 << (logn + lb)
    xs = powers(p, c, NM.root_of_unity(field, logn + lb), N)
    xn = powers(p, pow(c, n, p), NM.root_of_unity(field, lb), 1 << lb)                # x^n has period 2^lb in k
    return [(-n) % p if x == 1 else (1 - xn[k & ((1 << lb) - 1)]) * pow(x - 1, -1, p) % p for k, x in enumerate(xs)]


def test_the_closed_form_of_the_extension_is_the_models():
    for field in FIELDS:
        p = NM.MODULUS[field]
        for logn, lb in ((0, 1), (3, 2), (4, 8)):
            for c in (1, 777, NM.root_of_unity(field, logn + lb)):
                want = NM.ntt(field, [p - 1] * (1 << logn) + [0] * ((1 << (logn + lb)) - (1 << logn)), False, c)
                assert extension_of_all_p_minus_1(field, logn, lb, c) == want


@gpu
@pytest.mark.parametrize("lb", (1, 2, 8))
@pytest.mark.parametrize("logn", (0, 3, 10))
@pytest.mark.parametrize("field", FIELDS)
def test_low_degree_extension_of_a_table_of_p_minus_1(zk, field, logn, lb):
    """reference: the model's transform of the padded table; at 2^10 x 2^8 = 2^18 entries, where the model takes four seconds a
    transform, the closed form above (checked against the model at small sizes by the test before this one)"""
    p, n, N = NM.MODULUS[field], 1 << logn, 1 << (logn + lb)
    poly = table_of(zk, field, to_mont(zk, field, [p - 1] * n))
    c = random.Random(8000 + logn + lb + field).randrange(2, p)
    for coset in (None, c):
        got = zk.low_degree_extend(poly, lb, None if coset is None else zk.from_ints(field, [coset])[0])
        if logn + lb <= 13:
            want = NM.ntt(field, [p - 1] * n + [0] * (N - n), False, coset or 1)
        else:
            want = extension_of_all_p_minus_1(field, logn, lb, coset or 1)
        assert len(got) == N and np.array_equal(got.evaluated_values, to_mont(zk, field, want)), (field, logn, lb, coset is not None)
