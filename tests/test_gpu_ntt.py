"""GPU: the number-theoretic transform (csrc/ntt.cuh) over BLS12-381 Fr and BN254 Fr.

Sizes the model reaches (tests/_ntt_model.py, Python integers): forward, inverse, coset forward and coset inverse equal the model element
for element for every 2^0 .. 2^14, 2^16 and 2^20.  PATH_FIRST_SIZE names the smallest size at which the library takes each of its plans
(zkmle_ntt.hip make_plan) and every one of them is such a size.  Plans of more than three passes start at 2^25 entries, where no model
reaches; they run the same two kernels with more middle passes, and ZK_NTT_MAX_DIGIT_BITS (fewer levels a pass) brings them to 2^9 .. 2^14.

Sizes it does not reach (2^21 .. 2^24, BLS12-381 Fr): each is tied to the size below by the radix-2 split of the WHOLE output,
out[2k] = NTT(lo + hi)[k], out[2k + 1] = cosetNTT(lo - hi; c = w_n)[k], bit for bit: by induction from the model-checked 2^20 every
output is covered.  At 2^24 also inverse(forward(x)) = x and 16 outputs equal the C oracle's Horner evaluation at c w^k."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import __graft_entry__ as G
import _ntt_model as NM
from oracle import oracle as O

pytestmark = pytest.mark.gpu
FIELDS = (0, 3)
MODEL_SIZES = tuple(range(15)) + (16, 20)
PATH_FIRST_SIZE = {"one launch, no level": 0, "one launch, one level (no twiddle)": 1, "one launch": 2, "two passes": 11, "three passes": 16}


@pytest.fixture(scope="module")
def zk():
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    return zk


def to_mont(zk, field, ints):
    """canonical ints -> Montgomery limbs (len, limbs), without a Python loop per limb"""
    nl = zk.limbs(field)
    canon = np.frombuffer(b"".join(v.to_bytes(8 * nl, "little") for v in ints), np.uint64).reshape(-1, nl).copy()
    out = np.zeros_like(canon)
    from zkmle_amd import _lib as L
    L.check(zk.lib().zk_vec_from_canonical(field, L.p64(canon), canon.shape[0], L.p64(out)))
    return out


def table_of(zk, field, mont):
    return zk.MultilinearPolynomial.vector(field, mont)


def test_every_plan_starts_at_a_model_compared_size():
    assert set(PATH_FIRST_SIZE.values()) <= set(MODEL_SIZES)
    assert "ZK_NTT_MAX_DIGIT_BITS" not in os.environ


@pytest.mark.parametrize("logn", MODEL_SIZES)
@pytest.mark.parametrize("field", FIELDS)
def test_all_four_transforms_equal_the_model(zk, field, logn):
    n, p = 1 << logn, NM.MODULUS[field]
    v = NM.random_ints(field, n, 1000 * field + logn)
    c = random.Random(5 * logn + field).randrange(2, p)
    cm = zk.from_ints(field, [c])[0]
    poly = table_of(zk, field, to_mont(zk, field, v))
    for inverse in (False, True):
        for coset, coset_m in ((1, None), (c, cm)):
            want = to_mont(zk, field, NM.ntt(field, v, inverse, coset))
            got = zk.ntt.ntt(poly, inverse, coset_m).evaluated_values
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (field, logn, inverse, coset != 1, bad[:8], bad.size)
    assert np.array_equal(poly.evaluated_values, to_mont(zk, field, v))              # zk.ntt.ntt leaves its input alone


@pytest.mark.parametrize("cap,logn", [(4, 9), (4, 13), (4, 14), (3, 13), (5, 14), (7, 16)])
def test_plans_of_more_passes_equal_the_model(zk, cap, logn):
    """three to five passes (digits of at most `cap` bits) on sizes the model reaches: what 2^25 entries and up run"""
    field, n, p = 0, 1 << logn, NM.MODULUS[0]
    v = NM.random_ints(field, n, 4000 + 16 * cap + logn)
    c = random.Random(cap * logn).randrange(2, p)
    cm = zk.from_ints(field, [c])[0]
    poly = table_of(zk, field, to_mont(zk, field, v))
    os.environ["ZK_NTT_MAX_DIGIT_BITS"] = str(cap)
    try:
        got = [zk.ntt.ntt(poly, inverse, cm).evaluated_values for inverse in (False, True)]
    finally:
        del os.environ["ZK_NTT_MAX_DIGIT_BITS"]
    for inverse in (False, True):
        assert np.array_equal(got[inverse], to_mont(zk, field, NM.ntt(field, v, inverse, c))), (cap, logn, inverse)
        assert np.array_equal(got[inverse], zk.ntt.ntt(poly, inverse, cm).evaluated_values)


@pytest.mark.parametrize("field", (1, 2))
def test_fq_fields_have_lengths_one_and_two(zk, field):
    from zkmle_amd import _lib as L
    p = NM.MODULUS[field]
    for n in (1, 2):
        for seed in range(3):
            v = NM.random_ints(field, n, 50 * field + 7 * n + seed)
            c = random.Random(seed).randrange(2, p)
            poly = table_of(zk, field, to_mont(zk, field, v))
            for inverse in (False, True):
                for coset, cm in ((1, None), (c, zk.from_ints(field, [c])[0])):
                    assert zk.ntt.ntt(poly, inverse, cm).to_ints() == NM.ntt(field, v, inverse, coset), (field, n, inverse, coset != 1)
    four = table_of(zk, field, zk.from_ints(field, [1, 2, 3, 4]))
    assert zk.lib().zk_ntt(four._h, 0, None) == L.ZK_E_RANGE
    three = table_of(zk, 0, zk.from_ints(0, [1, 2, 3]))
    assert zk.lib().zk_ntt(three._h, 0, None) == L.ZK_E_NOT_POW2
    assert zk.lib().zk_ntt(four._h, 0, L.p64(np.zeros(zk.limbs(field), np.uint64))) == L.ZK_E_ARG


def halves(zk, poly):
    """non-owning views of the two halves of a table"""
    from zkmle_amd import _lib as L
    lib, n, esz = zk.lib(), len(poly), 8 * zk.limbs(poly.field)
    out = []
    for k in range(2):
        h = C.c_void_p()
        L.check(lib.zk_table_wrap(poly.field, C.c_void_p(poly.device_ptr + k * (n // 2) * esz), n // 2, C.byref(h)))
        out.append(zk.MultilinearPolynomial(poly.field, _handle=h))
    return out


@pytest.mark.parametrize("logn", (21, 22, 23, 24))
def test_large_sizes_are_tied_to_the_size_below(zk, logn):
    field, n, p = 0, 1 << logn, NM.MODULUS[0]
    x = zk.MultilinearPolynomial.random(field, n, 0x177 + logn)
    lo, hi = halves(zk, x)
    s = zk.MultilinearPolynomial.add_polynomials(lo, hi)
    d = zk.MultilinearPolynomial.linear_combination([lo, hi], zk.from_ints(field, [1, -1]))
    out = zk.ntt.ntt(x).evaluated_values
    zk.ntt.ntt_inplace(s)
    zk.ntt.ntt_inplace(d, coset=zk.root_of_unity(field, logn))
    assert np.array_equal(out[0::2], s.evaluated_values), logn
    assert np.array_equal(out[1::2], d.evaluated_values), logn
    del s, d, out
    if logn != 24:
        return
    c = random.Random(24).randrange(2, p)
    cm = zk.from_ints(field, [c])[0]
    host = x.evaluated_values
    y = zk.ntt.ntt(x, coset=cm)
    got = y.evaluated_values
    w = NM.root_of_unity(field, logn)
    rng = random.Random(2424)
    ks = [0, 1, n // 2 - 1, n // 2, n - 1] + [rng.randrange(n) for _ in range(11)]
    for k in ks:
        z = O.from_ints(field, [c * pow(w, k, p) % p])[0]
        assert np.array_equal(got[k], O.uni_evaluate(field, host, z)), k
    zk.ntt.ntt_inplace(y, inverse=True, coset=cm)
    assert np.array_equal(y.evaluated_values, host)
    plain = zk.ntt.ntt(x)
    zk.ntt.ntt_inplace(plain, inverse=True)
    assert np.array_equal(plain.evaluated_values, host)


@pytest.mark.parametrize("field", FIELDS)
def test_low_degree_extension_equals_the_transform_of_the_padded_table(zk, field):
    p = NM.MODULUS[field]
    cases = [(logn, lb) for logn in (0, 1, 5, 9, 10, 11, 13, 14) for lb in (1, 2, 3)] + [(16, 3), (18, 3), (20, 1), (20, 2)]
    for logn, lb in cases:
        n = 1 << logn
        data = np.zeros((n, zk.limbs(field)), np.uint64)
        from zkmle_amd import _lib as L
        L.check(zk.lib().zk_host_fill_random(field, 0x1DE + logn, 0, n, L.p64(data)))
        poly = table_of(zk, field, data)
        padded = table_of(zk, field, np.concatenate([data, np.zeros(((n << lb) - n, data.shape[1]), np.uint64)]))
        cm = zk.from_ints(field, [random.Random(logn + lb).randrange(2, p)])[0]
        for coset in (None, cm):
            got = zk.low_degree_extend(poly, lb, coset)
            assert len(got) == n << lb
            assert np.array_equal(got.evaluated_values, zk.ntt.ntt(padded, False, coset).evaluated_values), (field, logn, lb, coset is not None)
        if logn <= 9:                                                        # and the codeword is what the model says
            want = NM.ntt(field, zk.to_ints(field, data) + [0] * ((n << lb) - n), False, 1)
            assert zk.low_degree_extend(poly, lb).to_ints() == want
    assert np.array_equal(zk.low_degree_extend(poly, 0).evaluated_values, zk.ntt.ntt(poly).evaluated_values)


@pytest.mark.parametrize("field", FIELDS)
def test_product_of_coefficient_tables(zk, field):
    from zkmle_amd import _lib as L
    p = NM.MODULUS[field]
    for logn in (0, 1, 2, 5, 9, 10):
        n = 1 << logn
        a, b = NM.random_ints(field, n, 600 + logn), NM.random_ints(field, n, 700 + logn)
        got = zk.poly_mul(table_of(zk, field, to_mont(zk, field, a)), table_of(zk, field, to_mont(zk, field, b)))
        assert len(got) == 2 * n and got.to_ints() == NM.poly_mul(field, a, b), (field, logn)
    n = 1 << 20
    a, b = zk.MultilinearPolynomial.random(field, n, 0xA + field), zk.MultilinearPolynomial.random(field, n, 0xB + field)
    prod = zk.poly_mul(a, b)
    ha, hb, hp = a.evaluated_values, b.evaluated_values, prod.evaluated_values
    assert hp.shape[0] == 2 * n and not hp[2 * n - 1].any()
    rng = random.Random(field)
    for _ in range(4):
        z = O.from_ints(field, [rng.randrange(p)])[0]
        assert np.array_equal(O.uni_evaluate(field, hp, z), O.fe_op(field, "mul", O.uni_evaluate(field, ha, z), O.uni_evaluate(field, hb, z)))
    h = C.c_void_p()
    short = zk.MultilinearPolynomial.random(field, 4, 1)
    assert zk.lib().zk_uni_mul(a._h, short._h, C.byref(h)) == L.ZK_E_LEN_MISMATCH


def test_wrapped_table_stream_and_host_buffers_give_the_same_bytes(zk):
    import torch
    from zkmle_amd import _lib as L
    lib = zk.lib()
    field, n = 0, 1 << 17
    poly = zk.MultilinearPolynomial.random(field, n, 0x57EA)
    cm = zk.from_ints(field, [12345])[0]
    want = [zk.ntt.ntt(poly, inverse, cm).evaluated_values for inverse in (False, True)]
    work = poly.clone()
    h = C.c_void_p()
    L.check(lib.zk_table_wrap(field, C.c_void_p(work.device_ptr), n, C.byref(h)))
    view = zk.MultilinearPolynomial(field, _handle=h)
    zk.ntt.ntt_inplace(view, False, cm)
    assert np.array_equal(work.evaluated_values, want[0])
    stream = torch.cuda.Stream()
    L.check(lib.zk_set_stream(C.c_void_p(stream.cuda_stream)))
    try:
        for inverse in (False, True):
            assert np.array_equal(zk.ntt.ntt(poly, inverse, cm).evaluated_values, want[inverse])
        assert np.array_equal(zk.low_degree_extend(poly, 1, cm).evaluated_values[0::2], want[0])
    finally:
        L.check(lib.zk_set_stream(None))
    host = poly.evaluated_values
    out = np.zeros_like(host)
    for inverse in (False, True):
        L.check(lib.zk_host_ntt(field, L.p64(host), n, int(inverse), L.p64(cm), L.p64(out)))
        assert np.array_equal(out, want[inverse])
    L.check(lib.zk_release_cached_memory())
    assert np.array_equal(zk.ntt.ntt(poly, False, cm).evaluated_values, want[0])


def test_two_threads_transform_concurrently(zk):
    import threading
    import torch
    lib = zk.lib()
    field = 0
    jobs = []
    for k in range(2):
        poly = zk.MultilinearPolynomial.random(field, 1 << (17 + 2 * k), 0x7EAD + k)
        cm = zk.from_ints(field, [77 + k])[0]
        jobs.append((poly, cm, [zk.ntt.ntt(poly, inverse, cm).evaluated_values for inverse in (False, True)]))
    streams = [torch.cuda.Stream() for _ in jobs]
    errors = []

    def work(job, stream):
        poly, cm, want = job
        try:
            lib.zk_set_stream(C.c_void_p(stream.cuda_stream))
            for _ in range(4):
                for inverse in (False, True):
                    assert np.array_equal(zk.ntt.ntt(poly, inverse, cm).evaluated_values, want[inverse])
        except Exception as e:      # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(j, st)) for j, st in zip(jobs, streams)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
