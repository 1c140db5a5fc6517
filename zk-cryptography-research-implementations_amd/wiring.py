"""Plonk's wiring over FRI commitments: a permutation check (include/zkmle.h "Wiring: a permutation check over committed tables").

  `prove(wires, sigmas, ..)` proves that the three committed wire tables A, B, C take one value on every cycle of the permutation that the three
  committed tables SA, SB, SC describe: cell (j, x) of n = 2^d rows has the global index j n + x, and S_j[x] is the global index it is wired to.
  The argument is the logarithmic-derivative one: three helper tables H_j = 1 / (beta + W_j + gamma id_j) - 1 / (beta + W_j + gamma S_j) are
  computed and committed on the GPU (csrc/wiring.cuh), one sumcheck shows that they are those fractions and that they sum to zero, and ONE
  batch opening of the nine commitments (fri.open_multilinear_batch's protocol) at the point the rounds leave ends the proof, all on one
  transcript.  The prover does not check the statement: a false one gets a proof that does not verify.  `verify` is host code and needs
  nothing but the six roots.  `fractions` and `round` are the two kernels on their own.  Proving runs on the GPU (there is no CPU path).

  `sigma_from_cycles(d, cycles)` and `identity_sigma(d)` build the S tables as integers on the host."""
import ctypes as C

import numpy as np

from . import _lib as L
from . import _zerocheck_family as F
from .mle import MultilinearPolynomial, _elem

WIRES, OPENED, NODES = 3, 9, 5


class _Stats(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("ms_fractions", C.c_float), ("ms_commit", C.c_float), ("ms_eq", C.c_float), ("ms_rounds", C.c_float),
                ("ms_opening", C.c_float), ("ms_total", C.c_float)]


def identity_sigma(d):
    """-> [SA, SB, SC] as lists of integers: every cell is wired to itself, S_j[x] = j 2^d + x"""
    n = 1 << d
    return [list(range(j * n, (j + 1) * n)) for j in range(WIRES)]


def sigma_from_cycles(d, cycles):
    """-> [SA, SB, SC] as lists of integers.  `cycles`: lists of cells (j, x), wire j < 3 and row x < 2^d; each cell of a cycle is wired to the
    next one and the last to the first.  Cells that no cycle lists are fixed points; a cell may be listed once."""
    n = 1 << d
    sig = np.arange(WIRES * n, dtype=np.int64)
    seen = set()
    for cyc in cycles:
        cells = [int(j) * n + int(x) for j, x in cyc]
        for (j, x), c in zip(cyc, cells):
            if not (0 <= j < WIRES and 0 <= x < n) or c in seen:
                raise ValueError("a cycle lists cells (wire < 3, row < 2^d), each at most once")
            seen.add(c)
        for c, nxt in zip(cells, cells[1:] + cells[:1]):
            sig[c] = nxt
    return [[int(v) for v in sig[j * n:(j + 1) * n]] for j in range(WIRES)]


def sizes(d, log_blowup, log_final, nqueries, log_arity=1, grouped=False):
    """-> (nround, nhroots, nroots, nfinal, nvalues, path_bytes, nopen_round): the 5 d elements of the round polynomials, the 3 helper roots,
    then the counts of fri.ml_sizes(.., k=9), the opening of the nine commitments"""
    return F.sizes_of(L.lib().zk_wiring_sizes, 7, d, log_blowup, log_final, nqueries, log_arity, grouped)


def fractions(W, S, first, beta, gamma):
    """the helper table of one wire on its own: H[x] = inv0(beta + W[x] + gamma (first + x)) - inv0(beta + W[x] + gamma S[x]), inv0(0) = 0"""
    h = C.c_void_p()
    L.check(L.lib().zk_wiring_fractions(W._h, S._h, int(first), L.p64(_elem(W.field, beta)), L.p64(_elem(W.field, gamma)), C.byref(h)))
    return MultilinearPolynomial(W.field, _handle=h)


def round(tables, beta, gamma, alpha, mu, id_base=0, log_step=0, r=None):
    """one round pass on its own; tables = (A, B, C, SA, SB, SC, H0, H1, H2, E).  r = None: -> g5 (5, limbs) = g(0) .. g(4) of the wiring's
    summand along the last variable, nothing folded.  Otherwise -> (the ten tables folded by r in their last variable, g5 of the folded ten).
    The id tables that go with the tables the sums are taken over are id_j[x] = j 2^d + id_base + 2^log_step x, d = log2 of their length +
    log_step."""
    if len(tables) != 10:
        raise ValueError("the wiring's pass takes ten tables: A, B, C, SA, SB, SC, H0, H1, H2, E")
    return F.round_pass(L.lib().zk_wiring_round, tables, (beta, gamma, alpha, mu, id_base), log_step, r, NODES)


class WiringProof(F.Proof):
    """h_roots (3, 32): the helper commitments' roots; round_polys (d, 5, limbs); ys (9, limbs) = the values of A, B, C, SA, SB, SC, H0, H1, H2
    at the point; opening: the fri.FriMlBatchOpening of the nine commitments there (its ys are the same array).  drawn (4 + d, limbs) = beta,
    gamma, alpha, mu, tau and challenges (d, limbs) are what the prover's transcript gave (diagnostic: the verifier derives its own; the
    opening's point is the challenges reversed)."""

    K, NODES, HELPER_ROOTS, DRAWN = OPENED, NODES, WIRES, 4


def prove(wires, sigmas, log_final, nqueries, log_arity=1, transcript=None, grinding_bits=0):
    """the proof that the tables of the six commitments, wires = (A, B, C) and sigmas = (SA, SB, SC), all of one shape (field, size, blow-up,
    coset and leaf grouping; grouped ones need log_arity=2), satisfy W(sigma(c)) = W(c) at every cell.  grinding_bits: the opening's
    proof-of-work step (fri.open_multilinear_batch)"""
    cms = tuple(wires) + tuple(sigmas)
    if len(wires) != WIRES or len(sigmas) != WIRES:
        raise ValueError("the wiring takes three wires (A, B, C) and three permutation tables (SA, SB, SC)")
    fn, arr = L.lib().zk_wiring_prove, (C.c_void_p * 6)(*[c._h for c in cms])
    return F.prove_with(WiringProof, lambda *rest: fn(arr, *rest), cms[0], log_final, nqueries, log_arity, transcript, grinding_bits)


def verify(roots, proof, transcript=None):
    """host only: `roots` = the roots of A, B, C, SA, SB, SC (32 bytes each)"""
    if len(roots) != 6:
        raise L.ZkError(L.ZK_E_ARG, "one 32-byte Merkle root per commitment: A, B, C, SA, SB, SC")
    return F.verify_with(L.lib().zk_wiring_verify, proof, roots, transcript)


def last_stats():
    """milliseconds of the calling thread's last prove: the helper tables, their commitments, the eq table, the rounds, the opening, and the
    host clock over the call"""
    return F.stats_of(L.lib().zk_wiring_last_stats, _Stats)
