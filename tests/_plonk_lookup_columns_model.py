"""Python model of the Plonk proof with lookup rows on COLUMN commitments (helper of tests/test_plonk_lookup_columns_cpu.py,
test_gpu_plonk_lookup_helpers.py and test_gpu_plonk_lookup_columns.py).  The definition is the one of
include/zkmle.h "Plonk with lookups on column commitments".  Built by import on _plonk_lookup_model (the circuits, round_g5, the relation's
summand) and on _fri_ml_columns_model (commit, open_columns, verify); the helper tables are its own, in the single-denominator form:

  commitments  witness = _fri_ml_columns_model.commit of (A, B, C); circuit = that of (qM, qL, qR, qO, qC, SA, SB, SC, qK, T0, T1, T2)
  statement    "ZCLC" be32(d) be32(l) in one append, the witness root, the circuit root, the l public values as 32-byte big-endian elements
  M            _lookup_model.multiplicities; committed as ONE column; its root appended; then beta, gamma
  helpers      H_j[x] = (Dsig_j - Did_j) inv0(Did_j Dsig_j),  HL[x] = (qK Dt - M Dw) inv0(Dw Dt), inv0(0) = 0; committed as ONE commitment of four
               columns; its root appended; then alpha, mu, tau_0 .. tau_{d-1}
  the sum      _plonk_lookup_model's, unchanged: round_g5 on the twenty-one tables with the explicit id and PI tables
  opening      _fri_ml_columns_model.open_columns of the four commitments (widths 3, 12, 1, 4) at z, z[d - 1 - l] = r_l, on the same transcript
  verifier     _plonk_lookup_model's checks on the twenty claims as they stand, then the columns opening's verifier with the roots witness,
               circuit, M, helpers

`prove(.., cheat=..)` has _plonk_lookup_model's two cheating provers.  Everything is Python integers; nothing here knows how the library works."""
import functools

import _fri_ml_columns_model as CM
import _lookup_model as LM
import _plonk_lookup_model as KL
import _zerocheck_family_model as F
from oracle import pymodel as M

be32 = F.be32
WIRES, GIVEN, K, NODES = KL.WIRES, KL.GIVEN, KL.K, KL.NODES
WIDTHS = (3, 12, 1, 4)
circuit, satisfied, pow_transcript, mont, interpolate5 = KL.circuit, KL.satisfied, KL.pow_transcript, KL.mont, KL.interpolate5
inv0 = F.inv0


def tag(d, l):
    return b"ZCLC" + int(d).to_bytes(4, "big") + int(l).to_bytes(4, "big")


def helper_inputs(given, m):
    """A, B, C, SA, SB, SC, qK, T0, T1, T2, M of the fifteen and M: what the helper kernel reads"""
    return [given[j] for j in (0, 1, 2, 8, 9, 10, 11, 12, 13, 14)] + [m]


def helpers_of(tabs, beta, gamma, p):
    """-> [H0, H1, H2, HL] from the eleven integer tables A, B, C, SA, SB, SC, qK, T0, T1, T2, M: ONE inverse per entry, of the product of its
    two denominators"""
    n = len(tabs[0])
    hs = []
    for j in range(WIRES):
        col = []
        for x in range(n):
            did, dsig = beta + tabs[j][x] + gamma * (j * n + x), beta + tabs[j][x] + gamma * tabs[3 + j][x]
            col.append((dsig - did) * inv0(did * dsig, p) % p)
        hs.append(col)
    A, B, C, qK, T0, T1, T2, m = tabs[0], tabs[1], tabs[2], tabs[6], tabs[7], tabs[8], tabs[9], tabs[10]
    hl = []
    for x in range(n):
        dw, dt = beta + A[x] + gamma * B[x] + gamma * gamma * C[x], beta + T0[x] + gamma * T1[x] + gamma * gamma * T2[x]
        hl.append((qK[x] * dt - m[x] * dw) * inv0(dw * dt, p) % p)
    return hs + [hl]


def helper_tables(given, beta, gamma, p, m=None):
    """-> [M, H0, H1, H2, HL] from the fifteen integer tables (m: a multiplicity table to use in M's place): _plonk_lookup_model.helper_tables
    with the single-denominator definition"""
    m = LM.multiplicities(KL.lookup_tables(given), p)[0] if m is None else m
    return [m] + helpers_of(helper_inputs(given, m), beta, gamma, p)


def commitments(field, tabs, b, coset=1, hasher=M.keccak256):
    """-> (witness, circuit): the two model column commitments of the fifteen tables"""
    return CM.commit(field, tabs[:3], b, coset, hasher), CM.commit(field, tabs[3:], b, coset, hasher)


def helper_phase(i, tabs, ch, p, cheat):
    """_plonk_lookup_model's helper phases with the helper tables of this file; the proof's dict keeps the five tables as `helpers`"""
    new, more = KL.helper_phase(i, tabs, ch, p, cheat, helper_tables)
    return new, dict(more, helpers=[tabs[GIVEN]] + new) if i == 1 else more


PROTO = KL.PROTO._replace(tag=tag, phases=((1, 2), (1, 2)), helpers=helper_phase, opening=CM, widths=WIDTHS)
flat = functools.partial(F.flat, PROTO)
_statement = lambda tr, roots, d, pub, p: F.statement(PROTO, tr, roots, d, p, pub)


def prove(wit, cir, pub, f, Q, tr=None, hasher=M.keccak256, cheat=None):
    """-> the proof as a dict; wit, cir: the model column commitments; pub: the public values; `tr` is advanced.  The statement is not checked."""
    assert wit["k"] == 3 and cir["k"] == 12 and all(cir[n] == wit[n] for n in ("field", "d", "b", "coset"))
    return F.prove_rounds(PROTO, [wit, cir], pub, f, Q, 2, tr, hasher, cheat)


def verify(pr, roots=None, pub=None, tr=None, hasher=M.keccak256):
    """`roots`, `pub`: the verifier's own two roots and its public values, the proof's unless given -> (ok, the number of the first check that
    failed or None): 0 the first round's sum (or a public value outside the field), l >= 1 round l's, d the last claim, d + 1 the opening"""
    return F.replay(PROTO, pr, roots, pub, tr, hasher)


def sizes(d, b, f, Q):
    """(nround, nhroots) + the columns model's five counts for the widths 3, 12, 1, 4"""
    return F.sizes(PROTO, d, b, f, Q)
