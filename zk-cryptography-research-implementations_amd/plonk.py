"""A Plonk proof over FRI commitments: gate, wiring and public inputs in ONE sumcheck (include/zkmle.h "Plonk: gate, wiring and public inputs
in one sumcheck").

  `prove(wires, selectors, sigmas, public_inputs, ..)` proves that the eleven committed tables A, B, C, qM, qL, qR, qO, qC, SA, SB, SC satisfy
  qM A B + qL A + qR B + qO C + qC = PI at every row (PI[x] = public_inputs[x] for x < l, 0 otherwise: a row x < l with qL = 1 and no other
  selector says A[x] = public_inputs[x]) and that A, B, C take one value on every cycle of the permutation SA, SB, SC describe (zk.wiring).  The
  wiring's three helper tables are computed and committed on the GPU, one sumcheck whose round is one fused pass over fifteen tables
  (csrc/plonk.cuh) proves both parts -- the public inputs are only its claimed sum -- and ONE batch opening of the fourteen commitments at the
  point the rounds leave ends the proof, all on one transcript.  The prover does not check the statement: a false one gets a proof that does
  not verify.  `verify` is host code and needs nothing but the eleven roots and the public values.  `round` is the kernel on its own and
  `public_eval` the verifier's sum_x public_inputs[x] eq(x, tau).  Proving runs on the GPU (there is no CPU path)."""
import ctypes as C

import numpy as np

from . import _lib as L
from . import _zerocheck_family as F
from .mle import limbs
from .wiring import _Stats

WIRES, SELECTORS, GIVEN, OPENED, TABLES, NODES = 3, 5, 11, 14, 15, 5


def _public(field, public_inputs):
    """-> (the values as an (l, limbs) array, its pointer or None when there is none)"""
    n = limbs(field)
    pub = np.zeros((0, n), np.uint64) if public_inputs is None else np.ascontiguousarray(public_inputs, np.uint64).reshape(-1, n)
    return pub, (L.p64(pub) if pub.shape[0] else None)


def sizes(d, log_blowup, log_final, nqueries, log_arity=1, grouped=False):
    """-> (nround, nhroots, nroots, nfinal, nvalues, path_bytes, nopen_round): the 5 d elements of the round polynomials, the 3 helper roots,
    then the counts of fri.ml_sizes(.., k=14), the opening of the fourteen commitments"""
    return F.sizes_of(L.lib().zk_plonk_sizes, 7, d, log_blowup, log_final, nqueries, log_arity, grouped)


def public_eval(field, public_inputs, tau):
    """host only: sum_{x < l} public_inputs[x] eq(x, tau), variable 0 the most significant index bit; tau: (d, limbs)"""
    pub, pp = _public(field, public_inputs)
    tau = np.ascontiguousarray(tau, np.uint64).reshape(-1, limbs(field))
    out = np.zeros(limbs(field), np.uint64)
    L.check(L.lib().zk_plonk_public_eval(field, pp, pub.shape[0], L.p64(tau), tau.shape[0], L.p64(out)))
    return out


def round(tables, beta, gamma, alpha, mu, id_base=0, log_step=0, r=None):
    """one round pass on its own; tables = (A, B, C, qM, qL, qR, qO, qC, SA, SB, SC, H0, H1, H2, E).  r = None: -> g5 (5, limbs) = g(0) .. g(4) of
    the summand along the last variable, nothing folded.  Otherwise -> (the fifteen tables folded by r in their last variable, g5 of the folded
    fifteen).  The id tables are those of zk.wiring.round."""
    if len(tables) != TABLES:
        raise ValueError("the pass takes fifteen tables: A, B, C, qM, qL, qR, qO, qC, SA, SB, SC, H0, H1, H2, E")
    return F.round_pass(L.lib().zk_plonk_round, tables, (beta, gamma, alpha, mu, id_base), log_step, r, NODES)


class PlonkProof(F.Proof):
    """h_roots (3, 32): the helper commitments' roots; round_polys (d, 5, limbs); ys (14, limbs) = the values of A, B, C, qM, qL, qR, qO, qC, SA,
    SB, SC, H0, H1, H2 at the point; opening: the fri.FriMlBatchOpening of the fourteen commitments there (its ys are the same array).  drawn
    (4 + d, limbs) = beta, gamma, alpha, mu, tau and challenges (d, limbs) are what the prover's transcript gave (diagnostic: the verifier
    derives its own; the opening's point is the challenges reversed).  The public values are the statement's, not the proof's."""

    K, NODES, HELPER_ROOTS, DRAWN = OPENED, NODES, WIRES, 4


def prove(wires, selectors, sigmas, public_inputs, log_final, nqueries, log_arity=1, transcript=None, grinding_bits=0):
    """the proof for the eleven commitments wires = (A, B, C), selectors = (qM, qL, qR, qO, qC) and sigmas = (SA, SB, SC), all of one shape
    (field, size, blow-up, coset and leaf grouping; grouped ones need log_arity=2), and the public values public_inputs ((l, limbs), l <= 2^d, or
    None).  grinding_bits: the opening's proof-of-work step (fri.open_multilinear_batch)"""
    cms = tuple(wires) + tuple(selectors) + tuple(sigmas)
    if len(wires) != WIRES or len(selectors) != SELECTORS or len(sigmas) != WIRES:
        raise ValueError("the proof takes three wires (A, B, C), five selectors (qM, qL, qR, qO, qC) and three permutation tables (SA, SB, SC)")
    fn, arr = L.lib().zk_plonk_prove, (C.c_void_p * GIVEN)(*[c._h for c in cms])
    return F.prove_with(PlonkProof, lambda *rest: fn(arr, *rest), cms[0], log_final, nqueries, log_arity, transcript, grinding_bits,
                        lambda: _public(cms[0].field, public_inputs))


def verify(roots, public_inputs, proof, transcript=None):
    """host only: `roots` = the roots of A, B, C, qM, qL, qR, qO, qC, SA, SB, SC (32 bytes each); public_inputs as for prove"""
    if len(roots) != GIVEN:
        raise L.ZkError(L.ZK_E_ARG, "one 32-byte Merkle root per commitment: A, B, C, qM, qL, qR, qO, qC, SA, SB, SC")
    return F.verify_with(L.lib().zk_plonk_verify, proof, roots, transcript, lambda: _public(proof.opening.field, public_inputs))


def last_stats():
    """milliseconds of the calling thread's last prove: the helper tables, their commitments, the eq table, the rounds, the opening, and the
    host clock over the call"""
    return F.stats_of(L.lib().zk_plonk_last_stats, _Stats)
