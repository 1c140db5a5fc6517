"""Number-theoretic transform of an HBM table (extension: the reference's fft/ crate is empty; definition in include/zkmle.h).

  forward  out[k] = sum_i in[i] c^i w_n^(i k),  w_n = (g^t)^(2^s / n)  with  p - 1 = 2^s t:  arkworks' Radix2EvaluationDomain
  inverse  the exact inverse map

A `MultilinearPolynomial` serves as a plain device table here: coefficients in, evaluations at c w_n^k out, both in natural order.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .mle import MultilinearPolynomial, _elem, limbs


def two_adicity(field):
    s = C.c_uint32(0)
    L.check(L.lib().zk_ntt_two_adicity(field, C.byref(s)))
    return int(s.value)


def root_of_unity(field, log_n):
    """w_n for n = 2^log_n, Montgomery limbs"""
    out = np.zeros(limbs(field), np.uint64)
    L.check(L.lib().zk_ntt_root_of_unity(field, log_n, L.p64(out)))
    return out


def _coset(field, coset):
    return None if coset is None else L.p64(_elem(field, coset))


def ntt_inplace(poly, inverse=False, coset=None):
    L.check(L.lib().zk_ntt(poly._h, 1 if inverse else 0, _coset(poly.field, coset)))
    return poly


def ntt(poly, inverse=False, coset=None):
    """a new table: the transform of `poly`, which is left as it is"""
    return ntt_inplace(poly.clone(), inverse, coset)


def low_degree_extend(poly, log_blowup, coset=None):
    """the len(poly) * 2^log_blowup evaluations of the coefficient table `poly` at c w^k: its Reed-Solomon codeword"""
    h = C.c_void_p()
    L.check(L.lib().zk_uni_low_degree_extend(poly._h, log_blowup, _coset(poly.field, coset), C.byref(h)))
    return MultilinearPolynomial(poly.field, _handle=h)


def poly_mul(a, b):
    """the 2 n coefficients of the product of two coefficient tables of n entries each"""
    h = C.c_void_p()
    L.check(L.lib().zk_uni_mul(a._h, b._h, C.byref(h)))
    return MultilinearPolynomial(a.field, _handle=h)


def evaluate_at(poly, z):
    """sum_i poly[i] z^i of the coefficient table `poly`, on the device: one element (Montgomery limbs)"""
    out = np.zeros(limbs(poly.field), np.uint64)
    L.check(L.lib().zk_uni_evaluate_device(poly._h, L.p64(_elem(poly.field, z)), L.p64(out)))
    return out
