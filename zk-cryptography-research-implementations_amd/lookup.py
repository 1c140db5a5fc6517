"""Table lookups over FRI commitments: a logUp argument (include/zkmle.h "Lookup: rows of a committed table").

  `prove(wires, selector, table, ..)` proves that every row x with qK[x] = 1 of the three committed wire tables A, B, C is a row of the
  committed table (T0, T1, T2): (A[x], B[x], C[x]) = (T0[y], T1[y], T2[y]) for some y.  The argument is the logarithmic-derivative one: the
  multiplicity table M (how often each table row is used, counted on the GPU by a hash table and credited to the smallest index of a repeated
  row) and ONE helper table H = qK / (beta + A + gamma B + gamma^2 C) - M / (beta + T0 + gamma T1 + gamma^2 T2) are computed and committed on
  the GPU (csrc/lookup.cuh), one sumcheck shows that H is those fractions and that it sums to zero, and ONE batch opening of the nine
  commitments (fri.open_multilinear_batch's protocol) at the point the rounds leave ends the proof, all on one transcript.  The prover does
  not check the statement: a false one gets a proof that does not verify (and last_stats()["misses"] >= 1).  `verify` is host code and needs
  nothing but the seven roots.  `multiplicities`, `fractions` and `round` are the kernels on their own.  Proving runs on the GPU (there is no
  CPU path).

  `table_columns(d, rows)` pads a list of triples to 2^d rows by repeating the last one and returns the three columns."""
import ctypes as C

import numpy as np

from . import _lib as L
from . import _zerocheck_family as F
from .mle import MultilinearPolynomial, _elem

GIVEN, HELPERS, OPENED, NODES = 7, 2, 9, 5


class _Stats(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("misses", C.c_uint64), ("ms_multiplicities", C.c_float), ("ms_fractions", C.c_float), ("ms_commit", C.c_float),
                ("ms_eq", C.c_float), ("ms_rounds", C.c_float), ("ms_opening", C.c_float), ("ms_total", C.c_float)]


def table_columns(d, rows):
    """-> [T0, T1, T2] as lists of 2^d integers: the triples `rows` (at least one, at most 2^d), padded by repeating the last one"""
    rows = [tuple(int(v) for v in row) for row in rows]
    n = 1 << d
    if not rows or len(rows) > n or any(len(row) != 3 for row in rows):
        raise ValueError("a table is 1 .. 2^d rows of three values")
    rows = rows + [rows[-1]] * (n - len(rows))
    return [[row[j] for row in rows] for j in range(3)]


def sizes(d, log_blowup, log_final, nqueries, log_arity=1, grouped=False):
    """-> (nround, nhroots, nroots, nfinal, nvalues, path_bytes, nopen_round): the 5 d elements of the round polynomials, the 2 helper roots,
    then the counts of fri.ml_sizes(.., k=9), the opening of the nine commitments"""
    return F.sizes_of(L.lib().zk_lookup_sizes, 7, d, log_blowup, log_final, nqueries, log_arity, grouped)


def multiplicities(tables):
    """tables = (A, B, C, qK, T0, T1, T2) -> (M, misses): M[y] = the number of rows x with qK[x] = 1 whose triple is the table's row y, credited
    to the smallest y of a repeated row; misses = the number of rows with qK = 1 whose triple is in no table row"""
    if len(tables) != GIVEN:
        raise ValueError("the multiplicities take seven tables: A, B, C, qK, T0, T1, T2")
    m, misses = C.c_void_p(), C.c_uint64(0)
    ins = (C.c_void_p * GIVEN)(*[t._h for t in tables])
    L.check(L.lib().zk_lookup_multiplicities(ins, C.byref(m), C.byref(misses)))
    return MultilinearPolynomial(tables[0].field, _handle=m), int(misses.value)


def hash_slots(tables):
    """zk_lookup_hash_slots (include/zkmle.h), a test hook: tables = (T0, T1, T2) of n rows -> the 2 n slots of the hash table as the insert pass
    of `multiplicities` and of the provers leaves it, a uint32 array; a slot holds the index of a table row or 0xFFFFFFFF (empty)"""
    if len(tables) != 3:
        raise ValueError("the hash table takes three tables: T0, T1, T2")
    slots = np.empty(2 * len(tables[0]), np.uint32)
    ins = (C.c_void_p * 3)(*[t._h for t in tables])
    L.check(L.lib().zk_lookup_hash_slots(ins, slots.ctypes.data_as(C.POINTER(C.c_uint32))))
    return slots


def fractions(tables, beta, gamma):
    """the helper table on its own; tables = (A, B, C, qK, T0, T1, T2, M): H[x] = qK[x] inv0(beta + A[x] + gamma B[x] + gamma^2 C[x])
    - M[x] inv0(beta + T0[x] + gamma T1[x] + gamma^2 T2[x]), inv0(0) = 0"""
    if len(tables) != GIVEN + 1:
        raise ValueError("the helper table takes eight tables: A, B, C, qK, T0, T1, T2, M")
    field = tables[0].field
    h = C.c_void_p()
    ins = (C.c_void_p * (GIVEN + 1))(*[t._h for t in tables])
    L.check(L.lib().zk_lookup_fractions(ins, L.p64(_elem(field, beta)), L.p64(_elem(field, gamma)), C.byref(h)))
    return MultilinearPolynomial(field, _handle=h)


def round(tables, beta, gamma, mu, r=None):
    """one round pass on its own; tables = (A, B, C, qK, T0, T1, T2, M, H, E).  r = None: -> g5 (5, limbs) = g(0) .. g(4) of the lookup's
    summand along the last variable, nothing folded.  Otherwise -> (the ten tables folded by r in their last variable, g5 of the folded ten)."""
    if len(tables) != 10:
        raise ValueError("the lookup's pass takes ten tables: A, B, C, qK, T0, T1, T2, M, H, E")
    return F.round_pass(L.lib().zk_lookup_round, tables, (beta, gamma, mu), None, r, NODES)


class LookupProof(F.Proof):
    """h_roots (2, 32): the roots of the commitments to M and H; round_polys (d, 5, limbs); ys (9, limbs) = the values of A, B, C, qK, T0, T1,
    T2, M, H at the point; opening: the fri.FriMlBatchOpening of the nine commitments there (its ys are the same array).  drawn (3 + d, limbs)
    = beta, gamma, mu, tau and challenges (d, limbs) are what the prover's transcript gave (diagnostic: the verifier derives its own; the
    opening's point is the challenges reversed)."""

    K, NODES, HELPER_ROOTS, DRAWN = OPENED, NODES, HELPERS, 3


def prove(wires, selector, table, log_final, nqueries, log_arity=1, transcript=None, grinding_bits=0):
    """the proof that the tables of the seven commitments, wires = (A, B, C), selector = qK and table = (T0, T1, T2), all of one shape (field,
    size, blow-up, coset and leaf grouping; grouped ones need log_arity=2), satisfy: every row with qK = 1 is a row of the table.
    grinding_bits: the opening's proof-of-work step (fri.open_multilinear_batch)"""
    if len(wires) != 3 or len(table) != 3:
        raise ValueError("the lookup takes three wires (A, B, C), the selector qK and three table columns (T0, T1, T2)")
    cms = tuple(wires) + (selector,) + tuple(table)
    fn, arr = L.lib().zk_lookup_prove, (C.c_void_p * GIVEN)(*[c._h for c in cms])
    return F.prove_with(LookupProof, lambda *rest: fn(arr, *rest), cms[0], log_final, nqueries, log_arity, transcript, grinding_bits)


def verify(roots, proof, transcript=None):
    """host only: `roots` = the roots of A, B, C, qK, T0, T1, T2 (32 bytes each)"""
    if len(roots) != GIVEN:
        raise L.ZkError(L.ZK_E_ARG, "one 32-byte Merkle root per commitment: A, B, C, qK, T0, T1, T2")
    return F.verify_with(L.lib().zk_lookup_verify, proof, roots, transcript)


def last_stats():
    """the calling thread's last prove: the rows with qK = 1 whose triple is in no table row, and milliseconds of the multiplicity count, the
    helper table, the two commitments, the eq table, the rounds, the opening, and the host clock over the call"""
    return F.stats_of(L.lib().zk_lookup_last_stats, _Stats)
