"""CPU: the host side of the number-theoretic transform (include/zkmle.h "number-theoretic transform").  The Python model of
tests/_ntt_model.py is checked against itself (the O(n^2) sum against the recursive split, up to 2^8) and against the C oracle's Horner
evaluation at c w^k (2^10); the library's roots of unity equal the model's for every field and size and have exact order; the transform's
precondition codes come in the header's order, all before the device check."""
import ctypes as C
import random

import numpy as np
import pytest

import __graft_entry__ as G
import _ntt_model as NM
from oracle import oracle as O

zk = G.import_package()
P64 = C.POINTER(C.c_uint64)
p64 = lambda a: a.ctypes.data_as(P64) if a is not None else None


def test_new_exports_are_present():
    lib = zk.lib()
    for name in ("zk_ntt_two_adicity", "zk_ntt_root_of_unity", "zk_ntt", "zk_host_ntt", "zk_uni_low_degree_extend", "zk_uni_mul"):
        assert hasattr(lib, name), name
        assert name + "(" in open(G.ROOT + "/include/zkmle.h").read(), name
    for name in ("two_adicity", "root_of_unity", "ntt", "ntt_inplace", "low_degree_extend", "poly_mul"):
        assert callable(getattr(zk.ntt, name)), name
    for name in ("two_adicity", "root_of_unity", "ntt_inplace", "low_degree_extend", "poly_mul"):
        assert getattr(zk, name) is getattr(zk.ntt, name), name


@pytest.mark.parametrize("field", [0, 3])
def test_model_dft_equals_model_ntt(field):
    p = NM.MODULUS[field]
    for logn in range(9):
        v = NM.random_ints(field, 1 << logn, 31 * field + logn)
        c = random.Random(logn).randrange(1, p)
        for coset in (1, c):
            f = NM.ntt(field, v, False, coset)
            assert f == NM.dft(field, v, False, coset), (logn, coset != 1)
            assert NM.ntt(field, f, True, coset) == v and NM.dft(field, f, True, coset) == v, (logn, coset != 1)


@pytest.mark.parametrize("field", [0, 3])
def test_model_equals_the_oracles_horner_evaluation(field):
    p, logn = NM.MODULUS[field], 10
    n = 1 << logn
    v = NM.random_ints(field, n, 77 + field)
    c = random.Random(field).randrange(2, p)
    w = NM.root_of_unity(field, logn)
    coeffs = O.from_ints(field, v)
    for coset in (1, c):
        out = NM.ntt(field, v, False, coset)
        for k in list(range(0, n, 37)) + [1, n // 2 - 1, n // 2, n - 1]:
            x = O.from_ints(field, [coset * pow(w, k, p) % p])[0]
            assert O.to_ints(field, O.uni_evaluate(field, coeffs, x).reshape(1, -1)) == [out[k]], (coset != 1, k)


def test_two_adicity():
    lib = zk.lib()
    for field, want in enumerate((32, 1, 1, 28)):
        s = C.c_uint32(99)
        assert lib.zk_ntt_two_adicity(field, C.byref(s)) == 0 and s.value == want == NM.two_adicity(field)
        assert zk.two_adicity(field) == want
    from zkmle_amd import _lib as L
    assert lib.zk_ntt_two_adicity(0, None) == L.ZK_E_ARG
    assert lib.zk_ntt_two_adicity(4, C.byref(C.c_uint32())) == L.ZK_E_ARG


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_roots_of_unity_equal_the_model_and_have_exact_order(field):
    from zkmle_amd import _lib as L
    p, s = NM.MODULUS[field], NM.two_adicity(field)
    for logn in range(s + 1):
        w = zk.to_ints(field, zk.root_of_unity(field, logn).reshape(1, -1))[0]
        assert w == NM.root_of_unity(field, logn), logn
        assert pow(w, 1 << logn, p) == 1 and (logn == 0 or pow(w, 1 << (logn - 1), p) == p - 1), logn
    out = np.zeros(zk.limbs(field), np.uint64)
    assert zk.lib().zk_ntt_root_of_unity(field, s + 1, p64(out)) == L.ZK_E_RANGE
    assert zk.lib().zk_ntt_root_of_unity(field, 0, None) == L.ZK_E_ARG


def test_precondition_codes_come_before_the_device_check():
    import torch
    from zkmle_amd import _lib as L
    lib = zk.lib()
    for field in (0, 1, 2, 3):
        nl = zk.limbs(field)
        data = zk.from_ints(field, list(range(1, 9)))
        out = np.zeros((8, nl), np.uint64)
        zero, one = np.zeros(nl, np.uint64), zk.from_ints(field, [1])[0]
        call = lambda n, coset, i=data, o=out: lib.zk_host_ntt(field, p64(i), n, 0, p64(coset), p64(o))
        assert call(4, zero) == L.ZK_E_ARG                       # a zero coset, whatever the length
        assert call(6, zero) == L.ZK_E_ARG
        assert call(4, None, None) == L.ZK_E_ARG and call(4, None, data, None) == L.ZK_E_ARG
        assert lib.zk_host_ntt(7, p64(data), 4, 0, None, p64(out)) == L.ZK_E_ARG
        assert call(6, None) == L.ZK_E_NOT_POW2 and call(6, one) == L.ZK_E_NOT_POW2 and call(0, None) == L.ZK_E_NOT_POW2
        if field in (1, 2):
            assert call(4, None) == L.ZK_E_RANGE and call(8, one) == L.ZK_E_RANGE
        if not torch.cuda.is_available():
            assert call(2, None) == L.ZK_E_NO_DEVICE and call(1, one) == L.ZK_E_NO_DEVICE
            if field in (0, 3):
                assert call(4, one) == L.ZK_E_NO_DEVICE
    assert lib.zk_ntt(None, 0, None) == L.ZK_E_ARG
    assert lib.zk_uni_low_degree_extend(None, 1, None, None) == L.ZK_E_ARG
    assert lib.zk_uni_mul(None, None, None) == L.ZK_E_ARG
