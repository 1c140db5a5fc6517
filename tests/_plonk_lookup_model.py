"""Python model of the Plonk proof with lookup rows over FRI commitments (helper of tests/test_plonk_lookup_cpu.py, test_gpu_plonk_lookup.py and
_plonk_lookup_worker.py).  The definition is the one of include/zkmle.h "Plonk with lookups: gate, wiring, public inputs and lookup rows in one
sumcheck"; the fifteen given tables are always in the order A, B, C, qM, qL, qR, qO, qC, SA, SB, SC, qK, T0, T1, T2 and the twenty opened ones in
that order followed by M, H0, H1, H2, HL.  Built on _plonk_model (the gate, the wiring, the explicit id and PI tables), _lookup_model (the
multiplicities, the helper table, the lookup's summand) and _fri_ml_wide_model (the opening of twenty):

  statement    "ZCPL" be32(d) be32(l) in one append, the fifteen roots, the l public values as 32-byte big-endian elements
  M            _lookup_model.multiplicities on A, B, C, qK, T0, T1, T2; committed, the root appended; then beta, gamma -- ONE pair
  helpers      H0, H1, H2 = _wiring_model.fractions, HL = _lookup_model.fractions, with that pair; the four roots in that order; then alpha, mu,
               tau_0 .. tau_{d-1}
  the sum      with the explicit PI and id tables, F = _plonk_model.summand (PI inside, claimed sum 0) on the plonk proof's fifteen
               + _lookup_model.summand on the lookup's nine with mu^2 in mu's place and alpha^4 E in E's.  A round's message is the round
               polynomial of F plus that of alpha^3 E PI, as in _plonk_model
  round l      binds the LAST variable, the message at X = 0 .. 4; then r_l; every table is folded by mle_fold_last
  opening      _fri_ml_wide_model.open_batch of the twenty at z, z[d - 1 - l] = r_l, on the same transcript
  verifier     g_0(0) + g_0(1) = alpha^3 sum_x PI[x] E_0[x];  g_l(0) + g_l(1) = g_{l-1}(r_{l-1});  the last claim against the summand without PI
               on the twenty values;  the opening's verifier.  A public value outside [0, p) is rejected.

`prove(.., cheat="wiring")` is 7n's cheating prover (H_j = 0, g_0(1) = c - g_0(0)); `cheat="lookup"` the lookup's (every miss credited to row
0 of M, HL formed from it honestly, g_0(1) = c - g_0(0)).
`circuit(field, d, seed, l, looked, ..)` builds a satisfied instance from _plonk_model.circuit's rows and a chosen set of lookup rows.
Everything is Python integers; nothing here knows how the library works."""
import functools
import random

import _fri_ml_wide_model as WB
import _lookup_model as LM
import _ntt_model as NM
import _plonk_model as PM
import _wiring_model as WM
import _zerocheck_family_model as F
from oracle import pymodel as M

be32 = F.be32
WIRES, GIVEN, HELPERS, K, NODES, TABLES = 3, 15, 5, 20, 5, 21
PLONK_PLACES = tuple(range(11)) + (16, 17, 18, 20)           # the plonk proof's fifteen (.., H0, H1, H2, E) among the twenty-one
LOOKUP_PLACES = (0, 1, 2, 11, 12, 13, 14, 15, 19)            # the lookup's nine (A, B, C, qK, T0, T1, T2, M, H) among them
E_PLACE = 20
interpolate5, eq_at, id_at, commit_like, mont = F.interpolate, F.eq_at, F.id_at, F.commit_like, F.mont
pi_table, public_eval = PM.pi_table, PM.public_eval


def tag(d, l):
    return b"ZCPL" + int(d).to_bytes(4, "big") + int(l).to_bytes(4, "big")


def lookup_tables(tabs):
    """A, B, C, qK, T0, T1, T2 of the fifteen"""
    return [tabs[j] for j in LOOKUP_PLACES[:7]]


def circuit(field, d, seed, l=0, looked="some", kind="random", false_gate=False, false_wiring=False, miss=None):
    """-> (the fifteen tables, the l public values).  The first eleven are _plonk_model.circuit's.  looked: "none", "some" (about half the rows)
    or "all": the rows with qK = 1.  The table holds their triples (A, B, C)[x] -- each once, in a shuffled order, with up to two random rows
    more where there is room -- padded by _lookup_model.table_columns; with no lookup row it is one random row.  miss = x: row x gets qK = 1
    (or keeps it) and the table loses every row equal to its triple but gains the triple with one more in the third column only"""
    p, rng, n = NM.MODULUS[field], random.Random(seed ^ 0x4C4B), 1 << d
    tabs, pub = PM.circuit(field, d, seed, l, kind, false_gate, false_wiring)
    rows_x = [] if looked == "none" else list(range(n)) if looked == "all" else [x for x in range(n) if rng.randrange(2)]
    qK = [1 if x in set(rows_x) else 0 for x in range(n)]
    triple = lambda x: (tabs[0][x], tabs[1][x], tabs[2][x])
    rows = list(dict.fromkeys(triple(x) for x in rows_x))
    rng.shuffle(rows)
    while len(rows) < min(n, max(1, len(rows) + 2)) and (not rows or rng.randrange(2)):
        rows.append(tuple(rng.randrange(p) for _ in range(3)))
    if not rows:
        rows = [tuple(rng.randrange(p) for _ in range(3))]
    if miss is not None:
        t = triple(miss)
        qK[miss] = 1
        rows = [r for r in rows if r != t] + [(t[0], t[1], (t[2] + 1) % p)]
    return tabs + [qK] + LM.table_columns(d, rows), pub


def satisfied(tabs, pub, p):
    """(the gate, the wiring, the lookup) on the fifteen integer tables"""
    return PM.satisfied(tabs[:11], pub, p) + (LM.satisfied(lookup_tables(tabs), p),)


def summand(v, ids, ch, pi=0):
    """F at one (possibly non-Boolean) point: v = the values of the twenty-one tables there, ids of the three id tables, pi of the PI table"""
    beta, gamma, alpha, mu = ch
    e = v[E_PLACE]
    return PM.summand([v[j] for j in PLONK_PLACES], ids, ch, pi) + LM.summand([v[j] for j in LOOKUP_PLACES], alpha ** 4 * e, (beta, gamma, mu * mu))


def round_g5(tabs, ids, ch, p, pi=None):
    """-> (the message g(0) .. g(4) as the protocol sends it, the round polynomial of F itself at the five nodes), straight from the definition;
    tabs: the twenty-one; ids: the three id tables; pi: the PI table (all zero when None)"""
    return PM.round_g5(tabs, ids, ch, p, pi, summand, E_PLACE)


def helper_tables(given, beta, gamma, p, m=None):
    """-> [M, H0, H1, H2, HL] from the fifteen integer tables (m: a multiplicity table to use in M's place)"""
    n = len(given[0])
    lk = lookup_tables(given)
    m = LM.multiplicities(lk, p)[0] if m is None else m
    hs = [WM.fractions(given[j], given[8 + j], j * n, beta, gamma, p) for j in range(WIRES)]
    return [m] + hs + [LM.fractions(lk + [m], beta, gamma, p)]


def helper_phase(i, tabs, ch, p, cheat, helper_tables=helper_tables):
    """the family's helper phases: M from the fifteen (cheat "lookup": every miss credited to row 0), then H0, H1, H2, HL from them, M and
    beta, gamma (cheat "wiring": H_j = 0)"""
    assert cheat in (None, "wiring", "lookup")
    if i == 1:
        new = helper_tables(tabs[:GIVEN], ch[0], ch[1], p, tabs[GIVEN])[1:]
        return ([[0] * len(tabs[0])] * WIRES + new[WIRES:] if cheat == "wiring" else new), {}
    m, misses = LM.multiplicities(lookup_tables(tabs), p)
    if cheat == "lookup":
        m[0] = (m[0] + misses) % p
    return [m], {"misses": misses}


PROTO = F.Proto(tag, GIVEN, NODES, 0, ((1, 2), (4, 2)), helper_phase, summand, lambda tabs, x, ch, p: round_g5(tabs, x[:WIRES], ch, p, x[WIRES]),
                PM.explicit_tables, PM.claimed_sum, WB)
pow_transcript, sizes, flat = (functools.partial(fn, PROTO) for fn in (F.pow_transcript, F.sizes, F.flat))     # 4 + 2 d + 1 + R samples, as in the plonk proof
_statement = lambda tr, roots, d, pub, p: F.statement(PROTO, tr, roots, d, p, pub)
_helpers = functools.partial(F.helpers, PROTO)               # -> [beta, gamma, alpha, mu, tau]


def prove(cms, pub, f, Q, a=1, tr=None, hasher=M.keccak256, cheat=None):
    """-> the proof as a dict; `cms`: the model commitments of the fifteen (all alike); `pub`: the public values; `tr` is advanced.  The
    statement is not checked."""
    return F.prove_rounds(PROTO, cms, pub, f, Q, a, tr, hasher, cheat)


def verify(pr, roots=None, pub=None, tr=None, hasher=M.keccak256):
    """`roots`, `pub`: the verifier's own fifteen and its public values, the proof's unless given -> (ok, the number of the first check that
    failed or None): 0 the first round's sum (or a public value outside the field), l >= 1 round l's, d the last claim, d + 1 the opening"""
    return F.replay(PROTO, pr, roots, pub, tr, hasher)
