"""A Plonk proof with lookup rows over FRI commitments: gate, wiring, public inputs and a lookup into a committed table in ONE sumcheck with ONE
opening (include/zkmle.h "Plonk with lookups: gate, wiring, public inputs and lookup rows in one sumcheck").

  `prove(wires, selectors, sigmas, lookup_selector, table, public_inputs, ..)` proves for the fifteen committed tables A, B, C, qM, qL, qR, qO,
  qC, SA, SB, SC, qK, T0, T1, T2 what zk.plonk.prove proves for the first eleven and what zk.lookup.prove proves for A, B, C, qK, T0, T1, T2:
  the gate with the public inputs on the first rows, the wiring, and that every row with qK = 1 is a row of the table.  The multiplicities, the
  wiring's three helper tables and the lookup's one are computed and committed on the GPU, one sumcheck whose round is one fused pass over
  twenty-one tables (csrc/plonk_lookup.cuh) proves all three parts, and ONE wide batch opening of the twenty commitments
  (fri.open_multilinear_batch_wide) at the point the rounds leave ends the proof, all on one transcript.  The prover does not check the
  statement: a false one gets a proof that does not verify, and `last_stats()["misses"]` counts the rows whose triple is in no table row.
  `verify` is host code and needs nothing but the fifteen roots and the public values.  `round` is the kernel on its own.  `table_columns` and
  `sigma_from_cycles` are zk.lookup's and zk.wiring's.  Proving runs on the GPU (there is no CPU path).

  `prove_columns(witness, circuit, public_inputs, ..)` is the same statement on TWO column commitments (include/zkmle.h "Plonk with lookups on
  column commitments"): witness = fri.commit_columns((A, B, C), ..) and circuit = fri.commit_columns((qM, qL, qR, qO, qC, SA, SB, SC, qK, T0, T1,
  T2), ..), the circuit preprocessed once.  The four helper tables are made by ONE kernel (`helpers` is that kernel on its own) and committed as
  one four-column commitment, M as a one-column one, and fri.open_columns of the four commitments ends the proof.  `verify_columns` is host code
  and holds the witness root, the circuit root and the public values."""
import ctypes as C

from . import _lib as L
from . import _zerocheck_family as F
from . import fri
from .lookup import _Stats, table_columns  # noqa: F401
from .mle import MultilinearPolynomial, _elem
from .plonk import _public
from .wiring import sigma_from_cycles  # noqa: F401

WIRES, SELECTORS, COLUMNS, GIVEN, HELPERS, OPENED, TABLES, NODES = 3, 5, 3, 15, 5, 20, 21, 5
ORDER = "A, B, C, qM, qL, qR, qO, qC, SA, SB, SC, qK, T0, T1, T2"


def sizes(d, log_blowup, log_final, nqueries, log_arity=1, grouped=False):
    """-> (nround, nhroots, nroots, nfinal, nvalues, path_bytes, nopen_round): the 5 d elements of the round polynomials, the 5 helper roots,
    then the counts of fri.ml_sizes_wide(.., k=20), the opening of the twenty commitments"""
    return F.sizes_of(L.lib().zk_plonk_lookup_sizes, 7, d, log_blowup, log_final, nqueries, log_arity, grouped)


def round(tables, beta, gamma, alpha, mu, id_base=0, log_step=0, r=None):
    """one round pass on its own; tables = (A, B, C, qM, qL, qR, qO, qC, SA, SB, SC, qK, T0, T1, T2, M, H0, H1, H2, HL, E).  r = None: -> g5
    (5, limbs) = g(0) .. g(4) of the summand along the last variable, nothing folded.  Otherwise -> (the twenty-one tables folded by r in their
    last variable, g5 of the folded ones).  The id tables are those of zk.wiring.round."""
    if len(tables) != TABLES:
        raise ValueError("the pass takes twenty-one tables: " + ORDER + ", M, H0, H1, H2, HL, E")
    return F.round_pass(L.lib().zk_plonk_lookup_round, tables, (beta, gamma, alpha, mu, id_base), log_step, r, NODES)


class PlonkLookupProof(F.Proof):
    """h_roots (5, 32): the roots of M, H0, H1, H2, HL; round_polys (d, 5, limbs); ys (20, limbs) = the values of the fifteen and of M, H0, H1,
    H2, HL at the point; opening: the fri.FriMlWideOpening of the twenty commitments there (its ys are the same array).  drawn (4 + d, limbs) =
    beta, gamma, alpha, mu, tau and challenges (d, limbs) are what the prover's transcript gave (diagnostic: the verifier derives its own; the
    opening's point is the challenges reversed).  The public values are the statement's, not the proof's."""

    K, NODES, HELPER_ROOTS, DRAWN, OPENING = OPENED, NODES, HELPERS, 4, fri.FriMlWideOpening


def prove(wires, selectors, sigmas, lookup_selector, table, public_inputs, log_final, nqueries, log_arity=1, transcript=None, grinding_bits=0):
    """the proof for the fifteen commitments wires = (A, B, C), selectors = (qM, qL, qR, qO, qC), sigmas = (SA, SB, SC), lookup_selector = qK and
    table = (T0, T1, T2), all of one shape (field, size, blow-up, coset and leaf grouping; grouped ones need log_arity=2), and the public values
    public_inputs ((l, limbs), l <= 2^d, or None).  grinding_bits: the opening's proof-of-work step"""
    if len(wires) != WIRES or len(selectors) != SELECTORS or len(sigmas) != WIRES or len(table) != COLUMNS:
        raise ValueError("the proof takes three wires, five selectors, three permutation tables, the lookup selector and three table columns: " + ORDER)
    cms = tuple(wires) + tuple(selectors) + tuple(sigmas) + (lookup_selector,) + tuple(table)
    fn, arr = L.lib().zk_plonk_lookup_prove, (C.c_void_p * GIVEN)(*[c._h for c in cms])
    return F.prove_with(PlonkLookupProof, lambda *rest: fn(arr, *rest), cms[0], log_final, nqueries, log_arity, transcript, grinding_bits,
                        lambda: _public(cms[0].field, public_inputs))


def verify(roots, public_inputs, proof, transcript=None):
    """host only: `roots` = the fifteen roots (32 bytes each) in the order A, B, C, qM, qL, qR, qO, qC, SA, SB, SC, qK, T0, T1, T2;
    public_inputs as for prove"""
    if len(roots) != GIVEN:
        raise L.ZkError(L.ZK_E_ARG, "one 32-byte Merkle root per commitment: " + ORDER)
    return F.verify_with(L.lib().zk_plonk_lookup_verify, proof, roots, transcript, lambda: _public(proof.opening.field, public_inputs))


def last_stats():
    """the calling thread's last prove: `misses` (rows with qK = 1 whose triple is in no table row) and milliseconds of the multiplicity count,
    the four helper tables, the five commitments together, the eq table, the rounds, the opening, and the host clock over the call"""
    return F.stats_of(L.lib().zk_plonk_lookup_last_stats, _Stats)


# ---- on column commitments ------------------------------------------------------------------------------------------------------------------
WIDTHS = (3, 12, 1, 4)                                       # witness, circuit, M, the helpers: the twenty in the order above
HELPER_INPUTS = "A, B, C, SA, SB, SC, qK, T0, T1, T2, M"


def helpers(tables, beta, gamma):
    """the four helper tables in one pass; tables = (A, B, C, SA, SB, SC, qK, T0, T1, T2, M) -> (H0, H1, H2, HL) in the single-denominator
    form: H_j = (Dsig_j - Did_j) inv0(Did_j Dsig_j), HL = (qK Dt - M Dw) inv0(Dw Dt), inv0(0) = 0"""
    if len(tables) != 11:
        raise ValueError("the helper pass takes eleven tables: " + HELPER_INPUTS)
    field = tables[0].field
    ins, outs = (C.c_void_p * 11)(*[t._h for t in tables]), (C.c_void_p * 4)()
    L.check(L.lib().zk_plonk_lookup_helpers(ins, L.p64(_elem(field, beta)), L.p64(_elem(field, gamma)), outs))
    return tuple(MultilinearPolynomial(field, _handle=C.c_void_p(h)) for h in outs)


def helpers_batch():
    """the rows a lane of the helper kernel takes; its tile is 256 times as many"""
    return int(L.lib().zk_plonk_lookup_helpers_batch())


def sizes_columns(d, log_blowup, log_final, nqueries):
    """-> (nround, nhroots, nroots, nfinal, nvalues, path_bytes, nopen_round): the 5 d elements of the round polynomials, the 2 helper roots,
    then the counts of fri.columns_sizes((3, 12, 1, 4), ..)"""
    return F.sizes_of(L.lib().zk_plonk_lookup_sizes_columns, 7, d, log_blowup, log_final, nqueries)


class PlonkLookupColumnsProof(F.Proof):
    """h_roots (2, 32): the roots of M and of the helpers' four-column commitment; round_polys (d, 5, limbs); ys (20, limbs) = the values of the
    twenty columns at the point, in the order of PlonkLookupProof's; opening: the fri.FriColumnsOpening of the four commitments of widths 3, 12,
    1, 4 there (its ys are the same array).  drawn and challenges as PlonkLookupProof's.  The public values are the statement's."""

    K, NODES, HELPER_ROOTS, DRAWN, OPENING = OPENED, NODES, 2, 4, fri.FriColumnsOpening

    def __init__(self, field, d, log_blowup, log_final, nqueries, coset=None, grinding_bits=0):
        self._allocate(field, d, fri.FriColumnsOpening(field, WIDTHS, 1, d, log_blowup, log_final, nqueries, coset, grinding_bits))


def prove_columns(witness, circuit, public_inputs, log_final, nqueries, transcript=None, grinding_bits=0):
    """the proof for the column commitments witness = (A, B, C) and circuit = (qM, qL, qR, qO, qC, SA, SB, SC, qK, T0, T1, T2) of one shape
    (fri.commit_columns) and the public values public_inputs ((l, limbs), l <= 2^d, or None); d - log_final >= 2"""
    fn = L.lib().zk_plonk_lookup_prove_columns
    return F.prove_with(PlonkLookupColumnsProof, lambda *rest: fn(witness._h, circuit._h, *rest), witness, log_final, nqueries, None, transcript, grinding_bits,
                        lambda: _public(witness.field, public_inputs))


def verify_columns(witness_root, circuit_root, public_inputs, proof, transcript=None):
    """host only: the two roots (32 bytes each) as the verifier holds them; public_inputs as for prove_columns"""
    return F.verify_with(L.lib().zk_plonk_lookup_verify_columns, proof, [witness_root, circuit_root], transcript,
                         lambda: _public(proof.opening.field, public_inputs))


def columns_last_stats():
    """last_stats for the calling thread's last prove_columns: ms_fractions is the one helper kernel, ms_commit the two helper commitments"""
    return F.stats_of(L.lib().zk_plonk_lookup_columns_last_stats, _Stats)
