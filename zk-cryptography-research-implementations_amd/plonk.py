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
from . import fri
from .mle import MultilinearPolynomial, _elem, limbs
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
    out = [C.c_size_t(0) for _ in range(7)]
    if grouped and log_arity != 2:
        raise ValueError("grouped leaves need log_arity=2")
    L.check(L.lib().zk_plonk_sizes(d, log_blowup, log_final, nqueries, log_arity, 2 if grouped else 0, *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


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
    field = tables[0].field
    g5 = np.zeros((NODES, limbs(field)), np.uint64)
    ins = (C.c_void_p * TABLES)(*[t._h for t in tables])
    ch = [L.p64(_elem(field, v)) for v in (beta, gamma, alpha, mu, id_base)]
    if r is None:
        L.check(L.lib().zk_plonk_round(ins, *ch, log_step, None, None, L.p64(g5)))
        return g5
    outs = (C.c_void_p * TABLES)()
    L.check(L.lib().zk_plonk_round(ins, *ch, log_step, L.p64(_elem(field, r)), outs, L.p64(g5)))
    return tuple(MultilinearPolynomial(field, _handle=C.c_void_p(h)) for h in outs), g5


class PlonkProof:
    """h_roots (3, 32): the helper commitments' roots; round_polys (d, 5, limbs); ys (14, limbs) = the values of A, B, C, qM, qL, qR, qO, qC, SA,
    SB, SC, H0, H1, H2 at the point; opening: the fri.FriMlBatchOpening of the fourteen commitments there (its ys are the same array).  drawn
    (4 + d, limbs) = beta, gamma, alpha, mu, tau and challenges (d, limbs) are what the prover's transcript gave (diagnostic: the verifier
    derives its own; the opening's point is the challenges reversed).  The public values are the statement's, not the proof's."""

    K, NODES = OPENED, NODES

    def __init__(self, field, d, log_blowup, log_final, nqueries, coset=None, log_arity=1, grouped=False, grinding_bits=0):
        n = limbs(field)
        self.field, self.d = field, d
        self.h_roots = np.zeros((WIRES, 32), np.uint8)
        self.drawn = np.zeros((4 + d, n), np.uint64)
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


def prove(wires, selectors, sigmas, public_inputs, log_final, nqueries, log_arity=1, transcript=None, grinding_bits=0):
    """the proof for the eleven commitments wires = (A, B, C), selectors = (qM, qL, qR, qO, qC) and sigmas = (SA, SB, SC), all of one shape
    (field, size, blow-up, coset and leaf grouping; grouped ones need log_arity=2), and the public values public_inputs ((l, limbs), l <= 2^d, or
    None).  grinding_bits: the opening's proof-of-work step (fri.open_multilinear_batch)"""
    cms = tuple(wires) + tuple(selectors) + tuple(sigmas)
    if len(wires) != WIRES or len(selectors) != SELECTORS or len(sigmas) != WIRES:
        raise ValueError("the proof takes three wires (A, B, C), five selectors (qM, qL, qR, qO, qC) and three permutation tables (SA, SB, SC)")
    c0 = cms[0]
    grouped = getattr(c0, "log_group", 0) != 0
    if grouped and log_arity != 2:
        raise ValueError("commitments with grouped leaves are opened with log_arity=2")
    pub, pp = _public(c0.field, public_inputs)
    pr = PlonkProof(c0.field, c0.d, c0.log_blowup, log_final, nqueries, c0.coset, log_arity, grouped, grinding_bits)
    op, nonce = pr.opening, C.c_uint64(0)
    arr = (C.c_void_p * GIVEN)(*[c._h for c in cms])
    L.check(L.lib().zk_plonk_prove(arr, pp, pub.shape[0], log_final, nqueries, log_arity, grinding_bits, fri._handle(transcript), L.p8(pr.h_roots), L.p64(pr.drawn),
                                   L.p64(pr.round_polys), L.p64(pr.challenges), *fri._prover_outputs(op), C.byref(nonce)))
    op.pow_nonce = int(nonce.value)
    return pr


def verify(roots, public_inputs, proof, transcript=None):
    """host only: `roots` = the roots of A, B, C, qM, qL, qR, qO, qC, SA, SB, SC (32 bytes each); public_inputs as for prove"""
    op, ok = proof.opening, C.c_int(0)
    if len(roots) != GIVEN:
        raise L.ZkError(L.ZK_E_ARG, "one 32-byte Merkle root per commitment: A, B, C, qM, qL, qR, qO, qC, SA, SB, SC")
    hr = np.ascontiguousarray(proof.h_roots, np.uint8)
    if hr.shape != (WIRES, 32):
        raise L.ZkError(L.ZK_E_ARG, "three 32-byte helper roots")
    pub, pp = _public(op.field, public_inputs)
    # the opening's roots and claims are those of the fourteen; only the eleven are the verifier's own
    rf, _, ys, arrays = fri._verifier_inputs(op, list(roots) + [hr[j].tobytes() for j in range(WIRES)], op.ys, k=proof.K)
    rp = np.ascontiguousarray(proof.round_polys, np.uint64)
    L.check(L.lib().zk_plonk_verify(op.field, rf, pp, pub.shape[0], op.d, op.log_blowup, op.log_final, op.nqueries, op.log_arity, 2 if op.grouped else 0, op._coset(),
                                    fri._handle(transcript), L.p8(hr), L.p64(rp), L.p64(ys), *arrays, getattr(op, "grinding_bits", 0), getattr(op, "pow_nonce", 0),
                                    C.byref(ok)))
    return bool(ok.value)


def last_stats():
    """milliseconds of the calling thread's last prove: the helper tables, their commitments, the eq table, the rounds, the opening, and the
    host clock over the call"""
    st = _Stats()
    L.check(L.lib().zk_plonk_last_stats(C.byref(st)))
    return {name: getattr(st, name) for name, _ in _Stats._fields_}
