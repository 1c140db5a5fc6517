"""Python model of the multilinear opening of a FRI commitment at several points FOLDED BY 4 (helper of tests/test_fri_ml_arity_cpu.py and
test_gpu_fri_ml_arity.py).  The definition is the one of include/zkmle.h "FRI commitment opened with a fold arity", log_arity = 2; the
prover, the verifier, `sizes` and `flat` are those of tests/_fri_ml_family_model.py under its protocol ARITY:

  layers       the even l < R are committed: ceil(R / 2) roots.  A step starts at an even l: a fold by 4 to f_{l+2} if l + 2 <= R, else
               (R odd, l = R - 1) the fold by 2 to the final layer
  transcript   FRI's header, the arity (4 bytes), root_0, P, the points, the y_p, gamma, (g_l, r_l, root_{l+1} only if l + 1 is even and
               below R)*, T_R, Q indices mod N / 4
  answers      per query, per step, the sides s = 0 .. 3 (or 0, 1): f_l[j + s N_l / sides], j = i mod N_l / sides, and their paths

What is this module's alone is the four-point formula on a whole codeword.  Everything is Python integers; nothing here knows how the
library works."""
import functools

import _fri_ml_family_model as FAM
import _ntt_model as NM
from oracle import pymodel as M

fold2 = FAM.fold2
verify = functools.partial(FAM.verify_family, FAM.ARITY)
flat = functools.partial(FAM.flat, FAM.ARITY)


def open_points(cm, points, f, Q, tr=None, hasher=M.keccak256):
    """-> the opening as a dict; `cm` is a tests/_fri_pcs_model.py commitment, points a list of P lists of d ints; `tr` is advanced"""
    return FAM.open_family(FAM.ARITY, [cm], points, f, Q, tr, hasher)


def fold4_formula(field, table, r0, r1, coset=1):
    """the four-point formula on a codeword of len >= 4 on {coset w_len^k} -> len / 4 entries"""
    p, n = NM.MODULUS[field], len(table)
    q = n // 4
    w = NM.root_of_unity(field, n.bit_length() - 1)
    iota = pow(w, q, p)
    out = []
    for k in range(q):
        x = coset * pow(w, k, p) % p
        u0 = fold2(table[k], table[k + 2 * q], r0, x, p)
        u1 = fold2(table[k + q], table[k + 3 * q], r0, iota * x % p, p)
        out.append(fold2(u0, u1, r1, x * x % p, p))
    return out


def steps(L, R):
    """[(l, sides)] of the steps of an opening with R rounds"""
    return FAM.steps(L, R, 2)


def sizes(d, b, f, Q):
    """(nroots, nfinal, nvalues, path_bytes, nround) by the header's formulas"""
    return FAM.sizes(1, d, b, f, Q, 2, False)
