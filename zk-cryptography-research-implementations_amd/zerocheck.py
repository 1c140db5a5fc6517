"""Zerocheck of a product over three FRI commitments (include/zkmle.h "Zerocheck of a product of committed tables").

  `prove_mul(cA, cB, cC, ..)` proves that the committed tables satisfy C[x] = A[x] B[x] at every index: a sumcheck of
  sum_x eq(x, tau) (A[x] B[x] - C[x]) = 0 at a random tau, one fused pass per round (csrc/zerocheck.cuh), and ONE batch opening of the three
  commitments (fri.open_multilinear_batch's protocol) at the point the rounds leave, on the same transcript.  The prover does not check the
  relation: a false statement gets a proof that does not verify.  `verify_mul` is host code and needs nothing but the three roots.
  `mul_round` is one round pass on its own.  Proving runs on the GPU (there is no CPU path).

  `prove_gate(wires, selectors, ..)` is the same over EIGHT commitments (include/zkmle.h "Zerocheck of a Plonk gate over committed tables"): the
  wires A, B, C and the selectors qM, qL, qR, qO, qC satisfy qM A B + qL A + qR B + qO C + qC = 0 at every index.  The round message is a
  quartic at five nodes; `verify_gate`, `gate_round`, `gate_sizes` and `ZerocheckGateProof` are the counterparts of the names above."""
import ctypes as C

import numpy as np

from . import _lib as L
from . import fri
from .mle import MultilinearPolynomial, _elem, limbs


class _Stats(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("ms_eq", C.c_float), ("ms_rounds", C.c_float), ("ms_opening", C.c_float), ("ms_total", C.c_float)]


def _sizes(fn, d, log_blowup, log_final, nqueries, log_arity, grouped):
    out = [C.c_size_t(0) for _ in range(6)]
    if grouped and log_arity != 2:
        raise ValueError("grouped leaves need log_arity=2")
    L.check(fn(d, log_blowup, log_final, nqueries, log_arity, 2 if grouped else 0, *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def sizes(d, log_blowup, log_final, nqueries, log_arity=1, grouped=False):
    """-> (nzc_round, nroots, nfinal, nvalues, path_bytes, nround): the 4 d elements of the zerocheck's round polynomials, then the counts of
    fri.ml_sizes(.., k=3), the opening of the three commitments"""
    return _sizes(L.lib().zk_zerocheck_sizes, d, log_blowup, log_final, nqueries, log_arity, grouped)


def gate_sizes(d, log_blowup, log_final, nqueries, log_arity=1, grouped=False):
    """as `sizes` for the gate: 5 d elements of round polynomials, then the counts of fri.ml_sizes(.., k=8)"""
    return _sizes(L.lib().zk_zerocheck_gate_sizes, d, log_blowup, log_final, nqueries, log_arity, grouped)


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


def gate_round(tables, r=None):
    """one round pass of the gate on its own; tables = (A, B, C, qM, qL, qR, qO, qC, E).  r = None: -> g5 (5, limbs) = g(0) .. g(4) of
    sum_x' E (qM A B + qL A + qR B + qO C + qC) along the last variable, nothing folded.  Otherwise -> (the nine tables folded by r in their
    last variable, g5 of the folded nine)."""
    if len(tables) != 9:
        raise ValueError("the gate's pass takes nine tables: A, B, C, qM, qL, qR, qO, qC, E")
    field = tables[0].field
    g5 = np.zeros((5, limbs(field)), np.uint64)
    ins = (C.c_void_p * 9)(*[t._h for t in tables])
    if r is None:
        L.check(L.lib().zk_zerocheck_gate_round(ins, None, None, L.p64(g5)))
        return g5
    outs = (C.c_void_p * 9)()
    L.check(L.lib().zk_zerocheck_gate_round(ins, L.p64(_elem(field, r)), outs, L.p64(g5)))
    return tuple(MultilinearPolynomial(field, _handle=C.c_void_p(h)) for h in outs), g5


class ZerocheckMulProof:
    """tau (d, limbs) and challenges (d, limbs) are what the prover's transcript gave (diagnostic: the verifier derives its own; the opening's
    point is the challenges reversed); round_polys (d, 4, limbs); ys (3, limbs) = the values of A, B, C at the point; opening: the
    fri.FriMlBatchOpening of the three commitments there (its ys are the same array)."""

    K, NODES = 3, 4                                           # commitments; nodes of a round polynomial

    def __init__(self, field, d, log_blowup, log_final, nqueries, coset=None, log_arity=1, grouped=False, grinding_bits=0):
        n = limbs(field)
        self.field, self.d = field, d
        self.tau = np.zeros((d, n), np.uint64)
        self.round_polys = np.zeros((d, self.NODES, n), np.uint64)
        self.challenges = np.zeros((d, n), np.uint64)
        self.opening = fri.FriMlBatchOpening(field, self.K, 1, d, log_blowup, log_final, nqueries, coset, log_arity, grouped, grinding_bits)

    @property
    def ys(self):
        return self.opening.ys[:, 0]

    @property
    def point(self):
        """(1, d, limbs): where the tables are opened"""
        return np.ascontiguousarray(self.challenges[::-1])[None]


class ZerocheckGateProof(ZerocheckMulProof):
    """as ZerocheckMulProof for the gate: round_polys (d, 5, limbs); ys (8, limbs) = the values of A, B, C, qM, qL, qR, qO, qC at the point;
    opening: the fri.FriMlBatchOpening of the eight commitments there"""
    K, NODES = 8, 5


def _prove(cls, call, cms, log_final, nqueries, log_arity, transcript, grinding_bits):
    c0 = cms[0]
    grouped = getattr(c0, "log_group", 0) != 0
    if grouped and log_arity != 2:
        raise ValueError("commitments with grouped leaves are opened with log_arity=2")
    pr = cls(c0.field, c0.d, c0.log_blowup, log_final, nqueries, c0.coset, log_arity, grouped, grinding_bits)
    op, nonce = pr.opening, C.c_uint64(0)
    L.check(call(log_final, nqueries, log_arity, grinding_bits, fri._handle(transcript), L.p64(pr.tau), L.p64(pr.round_polys), L.p64(pr.challenges),
                 *fri._prover_outputs(op), C.byref(nonce)))
    op.pow_nonce = int(nonce.value)
    return pr


def _verify(fn, roots, proof, transcript):
    op, ok = proof.opening, C.c_int(0)
    rf, _, ys, arrays = fri._verifier_inputs(op, roots, op.ys, k=proof.K)
    rp = np.ascontiguousarray(proof.round_polys, np.uint64)
    L.check(fn(op.field, rf, op.d, op.log_blowup, op.log_final, op.nqueries, op.log_arity, 2 if op.grouped else 0, op._coset(), fri._handle(transcript), L.p64(rp),
               L.p64(ys), *arrays, getattr(op, "grinding_bits", 0), getattr(op, "pow_nonce", 0), C.byref(ok)))
    return bool(ok.value)


def prove_mul(cA, cB, cC, log_final, nqueries, log_arity=1, transcript=None, grinding_bits=0):
    """the proof that the tables of the three commitments (same field, size, blow-up, coset and leaf grouping; grouped ones need log_arity=2)
    satisfy C = A o B.  grinding_bits: the opening's proof-of-work step (fri.open_multilinear_batch)"""
    fn = L.lib().zk_zerocheck_mul_prove
    return _prove(ZerocheckMulProof, lambda *rest: fn(cA._h, cB._h, cC._h, *rest), (cA, cB, cC), log_final, nqueries, log_arity, transcript, grinding_bits)


def prove_gate(wires, selectors, log_final, nqueries, log_arity=1, transcript=None, grinding_bits=0):
    """the proof that the tables of the eight commitments, wires = (A, B, C) and selectors = (qM, qL, qR, qO, qC), all of one shape as for
    prove_mul, satisfy qM A B + qL A + qR B + qO C + qC = 0 at every index"""
    cms = tuple(wires) + tuple(selectors)
    if len(wires) != 3 or len(selectors) != 5:
        raise ValueError("the gate takes three wires (A, B, C) and five selectors (qM, qL, qR, qO, qC)")
    fn, arr = L.lib().zk_zerocheck_gate_prove, (C.c_void_p * 8)(*[c._h for c in cms])
    return _prove(ZerocheckGateProof, lambda *rest: fn(arr, *rest), cms, log_final, nqueries, log_arity, transcript, grinding_bits)


def verify_mul(roots, proof, transcript=None):
    """host only: `roots` = the roots of A, B, C (32 bytes each)"""
    return _verify(L.lib().zk_zerocheck_mul_verify, roots, proof, transcript)


def verify_gate(roots, proof, transcript=None):
    """host only: `roots` = the roots of A, B, C, qM, qL, qR, qO, qC (32 bytes each)"""
    return _verify(L.lib().zk_zerocheck_gate_verify, roots, proof, transcript)


def last_stats():
    """milliseconds of the calling thread's last prove_mul or prove_gate: the eq table, the rounds, the opening, and the host clock over the call"""
    st = _Stats()
    L.check(L.lib().zk_zerocheck_last_stats(C.byref(st)))
    return {name: getattr(st, name) for name, _ in _Stats._fields_}
