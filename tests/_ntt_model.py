"""Python model of the number-theoretic transform (helper of tests/test_ntt_cpu.py and test_gpu_ntt.py).  The definition is the one of
include/zkmle.h, which is arkworks' Radix2EvaluationDomain:

  p - 1 = 2^s t (t odd),  w_{2^s} = g^t,  w_n = w_{2^s}^(2^s / n),   forward  out[k] = sum_i in[i] c^i w_n^(i k),  inverse = its inverse map.

Everything is Python integers mod p: `dft` is the O(n^2) sum as written, `ntt` the recursive radix-2 split.  Nothing here knows how the
library cuts a transform into passes."""
import random
import sys

from oracle import pymodel as M

MODULUS = {0: M.P["bls12_381_fr"], 1: M.P["bls12_381_fq"], 2: M.P["bn254_fq"], 3: M.P["bn254_fr"]}
GENERATOR = {0: 7, 3: 5}                                   # multiplicative generators of the two scalar fields


def two_adicity(field):
    v, s = MODULUS[field] - 1, 0
    while v % 2 == 0:
        v //= 2
        s += 1
    return s


def root_of_unity(field, log_n):
    """w_n, n = 2^log_n <= 2^s"""
    p, s = MODULUS[field], two_adicity(field)
    assert log_n <= s
    top = pow(GENERATOR[field], (p - 1) >> s, p) if s > 1 else p - 1      # the Fq fields: w_2 = -1
    return pow(top, 1 << (s - log_n), p)


def dft(field, values, inverse=False, coset=1):
    p, n = MODULUS[field], len(values)
    w = root_of_unity(field, n.bit_length() - 1)
    if not inverse:
        return [sum(v * pow(coset, i, p) * pow(w, i * k, p) for i, v in enumerate(values)) % p for k in range(n)]
    wi, ni, ci = pow(w, p - 2, p), pow(n, p - 2, p), pow(coset, p - 2, p)
    return [sum(v * pow(wi, i * k, p) for k, v in enumerate(values)) * ni * pow(ci, i, p) % p for i in range(n)]


def _rec(p, a, w):
    n = len(a)
    if n == 1:
        return a
    w2 = w * w % p
    e, o = _rec(p, a[0::2], w2), _rec(p, a[1::2], w2)
    out, t, h = [0] * n, 1, n // 2
    for k in range(h):
        x = t * o[k] % p
        out[k] = (e[k] + x) % p
        out[k + h] = (e[k] - x) % p
        t = t * w % p
    return out


def ntt(field, values, inverse=False, coset=1):
    p, n = MODULUS[field], len(values)
    assert n and n & (n - 1) == 0
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 200))
    w = root_of_unity(field, n.bit_length() - 1)
    if not inverse:
        a, c = [], 1
        for v in values:
            a.append(v * c % p)
            c = c * coset % p
        return _rec(p, a, w)
    out = _rec(p, list(values), pow(w, p - 2, p))
    f, ci = pow(n, p - 2, p), pow(coset, p - 2, p)
    for i in range(n):
        out[i] = out[i] * f % p
        f = f * ci % p
    return out


def poly_mul(field, a, b):
    """schoolbook product: len(a) + len(b) coefficients (the top one zero)"""
    p = MODULUS[field]
    out = [0] * (len(a) + len(b))
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % p
    return out


def random_ints(field, n, seed, special=True):
    """n canonical values; with `special`, 0, 1 and p - 1 are among them as far as n allows"""
    rng = random.Random(seed)
    p = MODULUS[field]
    v = [rng.randrange(p) for _ in range(n)]
    if special:
        for k, s in enumerate((0, 1, p - 1)):
            if n > k + 1:
                v[(k * n) // 3 + 1] = s
    return v
