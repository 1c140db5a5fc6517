"""Zerocheck of a product over three FRI commitments (include/zkmle.h "Zerocheck of a product of committed tables").

  `prove_mul(cA, cB, cC, ..)` proves that the committed tables satisfy C[x] = A[x] B[x] at every index: a sumcheck of
  sum_x eq(x, tau) (A[x] B[x] - C[x]) = 0 at a random tau, one fused pass per round (csrc/zerocheck.cuh), and ONE batch opening of the three
  commitments (fri.open_multilinear_batch's protocol) at the point the rounds leave, on the same transcript.  The prover does not check the
  relation: a false statement gets a proof that does not verify.  `verify_mul` is host code and needs nothing but the three roots.
  `mul_round` is one round pass on its own.  Proving runs on the GPU (there is no CPU path)."""
import ctypes as C

import numpy as np

from . import _lib as L
from . import fri
from .mle import MultilinearPolynomial, _elem, limbs


class _Stats(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("ms_eq", C.c_float), ("ms_rounds", C.c_float), ("ms_opening", C.c_float), ("ms_total", C.c_float)]


def sizes(d, log_blowup, log_final, nqueries, log_arity=1, grouped=False):
    """-> (nzc_round, nroots, nfinal, nvalues, path_bytes, nround): the 4 d elements of the zerocheck's round polynomials, then the counts of
    fri.ml_sizes(.., k=3), the opening of the three commitments"""
    out = [C.c_size_t(0) for _ in range(6)]
    if grouped and log_arity != 2:
        raise ValueError("grouped leaves need log_arity=2")
    L.check(L.lib().zk_zerocheck_sizes(d, log_blowup, log_final, nqueries, log_arity, 2 if grouped else 0, *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def mul_round(A, B, Cc, E, r=None):
    """one round pass on its own.  r = None: -> g4 (4, limbs) = g(0), g(1), g(2), g(3) of sum_x' E (A B - C) along the last variable, nothing
    folded.  Otherwise -> (A', B', C', E', g4): the four tables folded by r in their last variable, g4 of the folded four."""
    g4 = np.zeros((4, limbs(A.field)), np.uint64)
    if r is None:
        L.check(L.lib().zk_zerocheck_mul_round(A._h, B._h, Cc._h, E._h, None, None, L.p64(g4)))
        return g4
    outs = (C.c_void_p * 4)()
    L.check(L.lib().zk_zerocheck_mul_round(A._h, B._h, Cc._h, E._h, L.p64(_elem(A.field, r)), outs, L.p64(g4)))
    return tuple(MultilinearPolynomial(A.field, _handle=C.c_void_p(h)) for h in outs) + (g4,)


class ZerocheckMulProof:
    """tau (d, limbs) and challenges (d, limbs) are what the prover's transcript gave (diagnostic: the verifier derives its own; the opening's
    point is the challenges reversed); round_polys (d, 4, limbs); ys (3, limbs) = the values of A, B, C at the point; opening: the
    fri.FriMlBatchOpening of the three commitments there (its ys are the same array)."""

    def __init__(self, field, d, log_blowup, log_final, nqueries, coset=None, log_arity=1, grouped=False, grinding_bits=0):
        n = limbs(field)
        self.field, self.d = field, d
        self.tau = np.zeros((d, n), np.uint64)
        self.round_polys = np.zeros((d, 4, n), np.uint64)
        self.challenges = np.zeros((d, n), np.uint64)
        self.opening = fri.FriMlBatchOpening(field, 3, 1, d, log_blowup, log_final, nqueries, coset, log_arity, grouped, grinding_bits)

    @property
    def ys(self):
        return self.opening.ys[:, 0]

    @property
    def point(self):
        """(1, d, limbs): where the three tables are opened"""
        return np.ascontiguousarray(self.challenges[::-1])[None]


def prove_mul(cA, cB, cC, log_final, nqueries, log_arity=1, transcript=None, grinding_bits=0):
    """the proof that the tables of the three commitments (same field, size, blow-up, coset and leaf grouping; grouped ones need log_arity=2)
    satisfy C = A o B.  grinding_bits: the opening's proof-of-work step (fri.open_multilinear_batch)"""
    grouped = getattr(cA, "log_group", 0) != 0
    if grouped and log_arity != 2:
        raise ValueError("commitments with grouped leaves are opened with log_arity=2")
    pr = ZerocheckMulProof(cA.field, cA.d, cA.log_blowup, log_final, nqueries, cA.coset, log_arity, grouped, grinding_bits)
    op, nonce = pr.opening, C.c_uint64(0)
    L.check(L.lib().zk_zerocheck_mul_prove(cA._h, cB._h, cC._h, log_final, nqueries, log_arity, grinding_bits, fri._handle(transcript), L.p64(pr.tau),
                                           L.p64(pr.round_polys), L.p64(pr.challenges), *fri._prover_outputs(op), C.byref(nonce)))
    op.pow_nonce = int(nonce.value)
    return pr


def verify_mul(roots, proof, transcript=None):
    """host only: `roots` = the roots of A, B, C (32 bytes each)"""
    op, ok = proof.opening, C.c_int(0)
    rf, _, ys, arrays = fri._verifier_inputs(op, roots, op.ys, k=3)
    rp = np.ascontiguousarray(proof.round_polys, np.uint64)
    L.check(L.lib().zk_zerocheck_mul_verify(op.field, rf, op.d, op.log_blowup, op.log_final, op.nqueries, op.log_arity, 2 if op.grouped else 0, op._coset(),
                                            fri._handle(transcript), L.p64(rp), L.p64(ys), *arrays, getattr(op, "grinding_bits", 0),
                                            getattr(op, "pow_nonce", 0), C.byref(ok)))
    return bool(ok.value)


def last_stats():
    """milliseconds of the calling thread's last prove_mul: the eq table, the rounds, the opening, and the host clock over the call"""
    st = _Stats()
    L.check(L.lib().zk_zerocheck_last_stats(C.byref(st)))
    return {name: getattr(st, name) for name, _ in _Stats._fields_}
