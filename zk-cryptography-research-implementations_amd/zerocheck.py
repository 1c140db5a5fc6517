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

from . import _lib as L
from . import _zerocheck_family as F


class _Stats(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("ms_eq", C.c_float), ("ms_rounds", C.c_float), ("ms_opening", C.c_float), ("ms_total", C.c_float)]


def sizes(d, log_blowup, log_final, nqueries, log_arity=1, grouped=False):
    """-> (nzc_round, nroots, nfinal, nvalues, path_bytes, nround): the 4 d elements of the zerocheck's round polynomials, then the counts of
    fri.ml_sizes(.., k=3), the opening of the three commitments"""
    return F.sizes_of(L.lib().zk_zerocheck_sizes, 6, d, log_blowup, log_final, nqueries, log_arity, grouped)


def gate_sizes(d, log_blowup, log_final, nqueries, log_arity=1, grouped=False):
    """as `sizes` for the gate: 5 d elements of round polynomials, then the counts of fri.ml_sizes(.., k=8)"""
    return F.sizes_of(L.lib().zk_zerocheck_gate_sizes, 6, d, log_blowup, log_final, nqueries, log_arity, grouped)


def mul_round(A, B, Cc, E, r=None):
    """one round pass on its own.  r = None: -> g4 (4, limbs) = g(0), g(1), g(2), g(3) of sum_x' E (A B - C) along the last variable, nothing
    folded.  Otherwise -> (A', B', C', E', g4): the four tables folded by r in their last variable, g4 of the folded four."""
    fn = L.lib().zk_zerocheck_mul_round                       # takes the four tables one by one
    out = F.round_pass(lambda ins, *rest: fn(*ins, *rest), (A, B, Cc, E), (), None, r, 4)
    return out if r is None else out[0] + (out[1],)


def gate_round(tables, r=None):
    """one round pass of the gate on its own; tables = (A, B, C, qM, qL, qR, qO, qC, E).  r = None: -> g5 (5, limbs) = g(0) .. g(4) of
    sum_x' E (qM A B + qL A + qR B + qO C + qC) along the last variable, nothing folded.  Otherwise -> (the nine tables folded by r in their
    last variable, g5 of the folded nine)."""
    if len(tables) != 9:
        raise ValueError("the gate's pass takes nine tables: A, B, C, qM, qL, qR, qO, qC, E")
    return F.round_pass(L.lib().zk_zerocheck_gate_round, tables, (), None, r, 5)


class ZerocheckMulProof(F.Proof):
    """tau (d, limbs) and challenges (d, limbs) are what the prover's transcript gave (diagnostic: the verifier derives its own; the opening's
    point is the challenges reversed); round_polys (d, 4, limbs); ys (3, limbs) = the values of A, B, C at the point; opening: the
    fri.FriMlBatchOpening of the three commitments there (its ys are the same array)."""

    K, NODES = 3, 4                                           # commitments; nodes of a round polynomial


class ZerocheckGateProof(ZerocheckMulProof):
    """as ZerocheckMulProof for the gate: round_polys (d, 5, limbs); ys (8, limbs) = the values of A, B, C, qM, qL, qR, qO, qC at the point;
    opening: the fri.FriMlBatchOpening of the eight commitments there"""
    K, NODES = 8, 5


def prove_mul(cA, cB, cC, log_final, nqueries, log_arity=1, transcript=None, grinding_bits=0):
    """the proof that the tables of the three commitments (same field, size, blow-up, coset and leaf grouping; grouped ones need log_arity=2)
    satisfy C = A o B.  grinding_bits: the opening's proof-of-work step (fri.open_multilinear_batch)"""
    fn = L.lib().zk_zerocheck_mul_prove
    return F.prove_with(ZerocheckMulProof, lambda *rest: fn(cA._h, cB._h, cC._h, *rest), cA, log_final, nqueries, log_arity, transcript, grinding_bits)


def prove_gate(wires, selectors, log_final, nqueries, log_arity=1, transcript=None, grinding_bits=0):
    """the proof that the tables of the eight commitments, wires = (A, B, C) and selectors = (qM, qL, qR, qO, qC), all of one shape as for
    prove_mul, satisfy qM A B + qL A + qR B + qO C + qC = 0 at every index"""
    cms = tuple(wires) + tuple(selectors)
    if len(wires) != 3 or len(selectors) != 5:
        raise ValueError("the gate takes three wires (A, B, C) and five selectors (qM, qL, qR, qO, qC)")
    fn, arr = L.lib().zk_zerocheck_gate_prove, (C.c_void_p * 8)(*[c._h for c in cms])
    return F.prove_with(ZerocheckGateProof, lambda *rest: fn(arr, *rest), cms[0], log_final, nqueries, log_arity, transcript, grinding_bits)


def verify_mul(roots, proof, transcript=None):
    """host only: `roots` = the roots of A, B, C (32 bytes each)"""
    return F.verify_with(L.lib().zk_zerocheck_mul_verify, proof, roots, transcript)


def verify_gate(roots, proof, transcript=None):
    """host only: `roots` = the roots of A, B, C, qM, qL, qR, qO, qC (32 bytes each)"""
    return F.verify_with(L.lib().zk_zerocheck_gate_verify, proof, roots, transcript)


def last_stats():
    """milliseconds of the calling thread's last prove_mul or prove_gate: the eq table, the rounds, the opening, and the host clock over the call"""
    return F.stats_of(L.lib().zk_zerocheck_last_stats, _Stats)
