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
from . import fri
from .mle import MultilinearPolynomial, _elem, limbs

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
    out = [C.c_size_t(0) for _ in range(7)]
    if grouped and log_arity != 2:
        raise ValueError("grouped leaves need log_arity=2")
    L.check(L.lib().zk_wiring_sizes(d, log_blowup, log_final, nqueries, log_arity, 2 if grouped else 0, *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


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
    field = tables[0].field
    g5 = np.zeros((NODES, limbs(field)), np.uint64)
    ins = (C.c_void_p * 10)(*[t._h for t in tables])
    ch = [L.p64(_elem(field, v)) for v in (beta, gamma, alpha, mu, id_base)]
    if r is None:
        L.check(L.lib().zk_wiring_round(ins, *ch, log_step, None, None, L.p64(g5)))
        return g5
    outs = (C.c_void_p * 10)()
    L.check(L.lib().zk_wiring_round(ins, *ch, log_step, L.p64(_elem(field, r)), outs, L.p64(g5)))
    return tuple(MultilinearPolynomial(field, _handle=C.c_void_p(h)) for h in outs), g5


class WiringProof:
    """h_roots (3, 32): the helper commitments' roots; round_polys (d, 5, limbs); ys (9, limbs) = the values of A, B, C, SA, SB, SC, H0, H1, H2
    at the point; opening: the fri.FriMlBatchOpening of the nine commitments there (its ys are the same array).  drawn (4 + d, limbs) = beta,
    gamma, alpha, mu, tau and challenges (d, limbs) are what the prover's transcript gave (diagnostic: the verifier derives its own; the
    opening's point is the challenges reversed)."""

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


def prove(wires, sigmas, log_final, nqueries, log_arity=1, transcript=None, grinding_bits=0):
    """the proof that the tables of the six commitments, wires = (A, B, C) and sigmas = (SA, SB, SC), all of one shape (field, size, blow-up,
    coset and leaf grouping; grouped ones need log_arity=2), satisfy W(sigma(c)) = W(c) at every cell.  grinding_bits: the opening's
    proof-of-work step (fri.open_multilinear_batch)"""
    cms = tuple(wires) + tuple(sigmas)
    if len(wires) != WIRES or len(sigmas) != WIRES:
        raise ValueError("the wiring takes three wires (A, B, C) and three permutation tables (SA, SB, SC)")
    c0 = cms[0]
    grouped = getattr(c0, "log_group", 0) != 0
    if grouped and log_arity != 2:
        raise ValueError("commitments with grouped leaves are opened with log_arity=2")
    pr = WiringProof(c0.field, c0.d, c0.log_blowup, log_final, nqueries, c0.coset, log_arity, grouped, grinding_bits)
    op, nonce = pr.opening, C.c_uint64(0)
    arr = (C.c_void_p * 6)(*[c._h for c in cms])
    L.check(L.lib().zk_wiring_prove(arr, log_final, nqueries, log_arity, grinding_bits, fri._handle(transcript), L.p8(pr.h_roots), L.p64(pr.drawn),
                                    L.p64(pr.round_polys), L.p64(pr.challenges), *fri._prover_outputs(op), C.byref(nonce)))
    op.pow_nonce = int(nonce.value)
    return pr


def verify(roots, proof, transcript=None):
    """host only: `roots` = the roots of A, B, C, SA, SB, SC (32 bytes each)"""
    op, ok = proof.opening, C.c_int(0)
    if len(roots) != 6:
        raise L.ZkError(L.ZK_E_ARG, "one 32-byte Merkle root per commitment: A, B, C, SA, SB, SC")
    hr = np.ascontiguousarray(proof.h_roots, np.uint8)
    if hr.shape != (WIRES, 32):
        raise L.ZkError(L.ZK_E_ARG, "three 32-byte helper roots")
    # the opening's roots and claims are those of the nine; only the six are the verifier's own
    rf, _, ys, arrays = fri._verifier_inputs(op, list(roots) + [hr[j].tobytes() for j in range(WIRES)], op.ys, k=proof.K)
    rp = np.ascontiguousarray(proof.round_polys, np.uint64)
    L.check(L.lib().zk_wiring_verify(op.field, rf, op.d, op.log_blowup, op.log_final, op.nqueries, op.log_arity, 2 if op.grouped else 0, op._coset(),
                                     fri._handle(transcript), L.p8(hr), L.p64(rp), L.p64(ys), *arrays, getattr(op, "grinding_bits", 0), getattr(op, "pow_nonce", 0),
                                     C.byref(ok)))
    return bool(ok.value)


def last_stats():
    """milliseconds of the calling thread's last prove: the helper tables, their commitments, the eq table, the rounds, the opening, and the
    host clock over the call"""
    st = _Stats()
    L.check(L.lib().zk_wiring_last_stats(C.byref(st)))
    return {name: getattr(st, name) for name, _ in _Stats._fields_}
