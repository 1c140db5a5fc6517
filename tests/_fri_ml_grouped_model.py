"""Python model of the Merkle tree with GROUPED leaves and of the multilinear opening of a FRI commitment over such trees (helper of
tests/test_fri_ml_grouped_cpu.py, test_gpu_merkle_grouped.py and test_gpu_fri_ml_grouped.py).  The definitions are those of include/zkmle.h
"Merkle commitment with grouped leaves" and "FRI commitment opened with grouped leaves"; the prover, the verifier, `sizes` and `flat` are
those of tests/_fri_ml_family_model.py under its protocol GROUPED:

  leaf         leaf_j = Keccak256(0x00 || be(e[j]) || be(e[j + part]) || ..), part = len >> log_group, j < part; nodes as ever over part leaves
  commitment   the codeword of tests/_fri_pcs_model.py under the tree with log_group = 2
  opening      the fold-by-4 opening of tests/_fri_ml_arity_model.py with three differences: the transcript takes 8 bytes (the arity 2, then a
               1) where that one takes 4; every committed layer is hashed with its leaves grouped by the sides of the step that starts
               there (4, or 2 for the final fold-2 step when R is odd); a step's answer holds ONE path, that of leaf j = i mod part

What is this module's alone is the commitment and the check of the host hash at the quad leaf's length.  Everything is Python integers;
nothing here knows how the library works."""
import functools

import _fri_ml_arity_model as AM
import _fri_ml_family_model as FAM
import _fri_model as FM
import _merkle_model as MM
import _ntt_model as NM
from oracle import pymodel as M

be32 = FM.be32
leaf_bytes, levels_of, verify_leaf = FAM.leaf_bytes, FAM.levels_of, FAM.verify_leaf
steps = AM.steps
verify = functools.partial(FAM.verify_family, FAM.GROUPED)
flat = functools.partial(FAM.flat, FAM.GROUPED)             # the C ABI's layout: a step's paths are a list of ONE path here


def check_host_keccak(zk):
    """tests/_merkle_model.py check_host_keccak, and the host hash at the quad leaf's 129 bytes too"""
    h = MM.check_host_keccak(zk)
    for seed in range(3):
        data = bytes((seed * 57 + 11 * i + 129) & 0xFF for i in range(129))
        assert h(data) == M.keccak256(data), seed
    return h


def commit(field, coeffs, b, coset=1, hasher=M.keccak256, log_group=2):
    p = NM.MODULUS[field]
    cw = FM.extend(field, coeffs, b, coset)
    levels = levels_of(cw, log_group, hasher)
    return {"field": field, "d": len(coeffs).bit_length() - 1, "b": b, "coset": coset % p, "coeffs": list(coeffs), "codeword": cw, "levels": levels,
            "root": levels[-1][0], "log_group": log_group}


def sizes(d, b, f, Q):
    """(nroots, nfinal, nvalues, path_bytes, nround): the arity model's with one path of L - l - log_sides digests per step"""
    return FAM.sizes(1, d, b, f, Q, 2, True)


def open_points(cm, points, f, Q, tr=None, hasher=M.keccak256):
    """-> the opening as a dict; `cm` is a commit() of this module, points a list of P lists of d ints; `tr` is advanced"""
    return FAM.open_family(FAM.GROUPED, [cm], points, f, Q, tr, hasher)
