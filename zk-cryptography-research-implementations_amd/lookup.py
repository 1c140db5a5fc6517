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
from . import fri
from .mle import MultilinearPolynomial, _elem, limbs

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
    out = [C.c_size_t(0) for _ in range(7)]
    if grouped and log_arity != 2:
        raise ValueError("grouped leaves need log_arity=2")
    L.check(L.lib().zk_lookup_sizes(d, log_blowup, log_final, nqueries, log_arity, 2 if grouped else 0, *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def multiplicities(tables):
    """tables = (A, B, C, qK, T0, T1, T2) -> (M, misses): M[y] = the number of rows x with qK[x] = 1 whose triple is the table's row y, credited
    to the smallest y of a repeated row; misses = the number of rows with qK = 1 whose triple is in no table row"""
    if len(tables) != GIVEN:
        raise ValueError("the multiplicities take seven tables: A, B, C, qK, T0, T1, T2")
    m, misses = C.c_void_p(), C.c_uint64(0)
    ins = (C.c_void_p * GIVEN)(*[t._h for t in tables])
    L.check(L.lib().zk_lookup_multiplicities(ins, C.byref(m), C.byref(misses)))
    return MultilinearPolynomial(tables[0].field, _handle=m), int(misses.value)


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
    field = tables[0].field
    g5 = np.zeros((NODES, limbs(field)), np.uint64)
    ins = (C.c_void_p * 10)(*[t._h for t in tables])
    ch = [L.p64(_elem(field, v)) for v in (beta, gamma, mu)]
    if r is None:
        L.check(L.lib().zk_lookup_round(ins, *ch, None, None, L.p64(g5)))
        return g5
    outs = (C.c_void_p * 10)()
    L.check(L.lib().zk_lookup_round(ins, *ch, L.p64(_elem(field, r)), outs, L.p64(g5)))
    return tuple(MultilinearPolynomial(field, _handle=C.c_void_p(h)) for h in outs), g5


class LookupProof:
    """h_roots (2, 32): the roots of the commitments to M and H; round_polys (d, 5, limbs); ys (9, limbs) = the values of A, B, C, qK, T0, T1,
    T2, M, H at the point; opening: the fri.FriMlBatchOpening of the nine commitments there (its ys are the same array).  drawn (3 + d, limbs)
    = beta, gamma, mu, tau and challenges (d, limbs) are what the prover's transcript gave (diagnostic: the verifier derives its own; the
    opening's point is the challenges reversed)."""

    K, NODES = OPENED, NODES

    def __init__(self, field, d, log_blowup, log_final, nqueries, coset=None, log_arity=1, grouped=False, grinding_bits=0):
        n = limbs(field)
        self.field, self.d = field, d
        self.h_roots = np.zeros((HELPERS, 32), np.uint8)
        self.drawn = np.zeros((3 + d, n), np.uint64)
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


def prove(wires, selector, table, log_final, nqueries, log_arity=1, transcript=None, grinding_bits=0):
    """the proof that the tables of the seven commitments, wires = (A, B, C), selector = qK and table = (T0, T1, T2), all of one shape (field,
    size, blow-up, coset and leaf grouping; grouped ones need log_arity=2), satisfy: every row with qK = 1 is a row of the table.
    grinding_bits: the opening's proof-of-work step (fri.open_multilinear_batch)"""
    if len(wires) != 3 or len(table) != 3:
        raise ValueError("the lookup takes three wires (A, B, C), the selector qK and three table columns (T0, T1, T2)")
    cms = tuple(wires) + (selector,) + tuple(table)
    c0 = cms[0]
    grouped = getattr(c0, "log_group", 0) != 0
    if grouped and log_arity != 2:
        raise ValueError("commitments with grouped leaves are opened with log_arity=2")
    pr = LookupProof(c0.field, c0.d, c0.log_blowup, log_final, nqueries, c0.coset, log_arity, grouped, grinding_bits)
    op, nonce = pr.opening, C.c_uint64(0)
    arr = (C.c_void_p * GIVEN)(*[c._h for c in cms])
    L.check(L.lib().zk_lookup_prove(arr, log_final, nqueries, log_arity, grinding_bits, fri._handle(transcript), L.p8(pr.h_roots), L.p64(pr.drawn),
                                    L.p64(pr.round_polys), L.p64(pr.challenges), *fri._prover_outputs(op), C.byref(nonce)))
    op.pow_nonce = int(nonce.value)
    return pr


def verify(roots, proof, transcript=None):
    """host only: `roots` = the roots of A, B, C, qK, T0, T1, T2 (32 bytes each)"""
    op, ok = proof.opening, C.c_int(0)
    if len(roots) != GIVEN:
        raise L.ZkError(L.ZK_E_ARG, "one 32-byte Merkle root per commitment: A, B, C, qK, T0, T1, T2")
    hr = np.ascontiguousarray(proof.h_roots, np.uint8)
    if hr.shape != (HELPERS, 32):
        raise L.ZkError(L.ZK_E_ARG, "two 32-byte helper roots")
    # the opening's roots and claims are those of the nine; only the seven are the verifier's own
    rf, _, ys, arrays = fri._verifier_inputs(op, list(roots) + [hr[j].tobytes() for j in range(HELPERS)], op.ys, k=proof.K)
    rp = np.ascontiguousarray(proof.round_polys, np.uint64)
    L.check(L.lib().zk_lookup_verify(op.field, rf, op.d, op.log_blowup, op.log_final, op.nqueries, op.log_arity, 2 if op.grouped else 0, op._coset(),
                                     fri._handle(transcript), L.p8(hr), L.p64(rp), L.p64(ys), *arrays, getattr(op, "grinding_bits", 0), getattr(op, "pow_nonce", 0),
                                     C.byref(ok)))
    return bool(ok.value)


def last_stats():
    """the calling thread's last prove: the rows with qK = 1 whose triple is in no table row, and milliseconds of the multiplicity count, the
    helper table, the two commitments, the eq table, the rounds, the opening, and the host clock over the call"""
    st = _Stats()
    L.check(L.lib().zk_lookup_last_stats(C.byref(st)))
    return {name: getattr(st, name) for name, _ in _Stats._fields_}
