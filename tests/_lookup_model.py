"""Python model of the lookup argument over FRI commitments (helper of tests/test_lookup_cpu.py and test_gpu_lookup.py).  The definition is
the one of include/zkmle.h "Lookup: rows of a committed table"; the seven given tables are always in the order A, B, C, qK, T0, T1, T2 and
the nine opened ones in the order A, B, C, qK, T0, T1, T2, M, H:

  statement    "ZCLK" be32(d), the seven roots
  M            M[y] = the number of rows x with qK[x] = 1 and (A, B, C)[x] = (T0, T1, T2)[y], credited to the SMALLEST y of a repeated row (a dict
               from the triple to its first index); a row whose triple is nowhere is counted nowhere (`misses`); committed with the shape of
               the seven, the root appended; then beta, gamma
  H            H[x] = qK[x] inv0(beta + A + gamma B + gamma^2 C) - M[x] inv0(beta + T0 + gamma T1 + gamma^2 T2), inv0(0) = 0; committed, the root
               appended; then mu, tau_0 .. tau_{d-1}
  round l      binds the LAST variable: g_l(X) = sum_x' [ mu H + E (H Dw Dt - qK Dt + M Dw) ] at (x', X) with Y(x', X) the line through Y[2x'] and
               Y[2x'+1]; sent at X = 0, 1, 2, 3, 4; then r_l; every table is folded by mle_fold_last
  point        z[d - 1 - l] = r_l
  opening      tests/_fri_ml_batch_model.py open_batch of the nine at the one point z on the same transcript (through _grind_model's
               PowTranscript when the proof-of-work step is asked for)
  verifier     g_0(0) + g_0(1) = 0;  g_l(0) + g_l(1) = g_{l-1}(r_{l-1}) by Lagrange's formula through the five nodes;  the last claim against
               the relation on the nine values;  the opening's verifier

`prove(.., cheat=True)` is the prover that commits a false M (every miss is credited to row 0), forms H from it honestly (the zerocheck part
of the sum is then 0 and the sum of H is not) and hides that from the first check: it sends g_0(1) = -g_0(0) and is honest afterwards.  The
first check passes, a later one fails, and the opening alone verifies.
`instance(field, d, seed, rows, looked)` builds a satisfied instance from a list of table rows and a choice of looked-up rows.
Everything is Python integers; nothing here knows how the library works."""
import functools
import random

import _fri_ml_batch_model as BM
import _ntt_model as NM
import _zerocheck_family_model as F
from oracle import pymodel as M

be32, inv0, eq_at, commit_like, interpolate5 = F.be32, F.inv0, F.eq_at, F.commit_like, F.interpolate
GIVEN, HELPERS, K, NODES = 7, 2, 9, 5


def tag(d):
    return b"ZCLK" + int(d).to_bytes(4, "big")


def table_columns(d, rows):
    """[T0, T1, T2]: the triples padded to 2^d by repeating the last one"""
    rows = list(rows) + [rows[-1]] * ((1 << d) - len(rows))
    return [[row[j] for row in rows] for j in range(3)]


def instance(field, d, seed, rows=None, looked=None):
    """-> [A, B, C, qK, T0, T1, T2], satisfied.  rows: the table's triples (1 .. 2^d of them; random ones in random number by default), padded by
    repeating the last; looked: {x: index into rows} = the rows with qK = 1 and the table row each holds (about two thirds of the rows by
    default); every other row has qK = 0 and a random triple"""
    p, rng, n = NM.MODULUS[field], random.Random(seed), 1 << d
    if rows is None:
        rows = [tuple(rng.randrange(p) for _ in range(3)) for _ in range(rng.randint(1, n))]
    if looked is None:
        looked = {x: rng.randrange(len(rows)) for x in range(n) if rng.randrange(3)}
    wires = [[rng.randrange(p) for _ in range(n)] for _ in range(3)]
    qK = [0] * n
    for x, y in looked.items():
        qK[x] = 1
        for j in range(3):
            wires[j][x] = rows[y][j] % p
    return wires + [qK] + table_columns(d, [tuple(v % p for v in row) for row in rows])


def falsified(tabs, x, p, selected=True):
    """row x holds table row 0 with one more in the third column only; qK[x] = 1 (selected) or 0"""
    out = [list(t) for t in tabs]
    out[0][x], out[1][x], out[2][x], out[3][x] = tabs[4][0], tabs[5][0], (tabs[6][0] + 1) % p, 1 if selected else 0
    return out


def multiplicities(tabs, p):
    """-> (M, misses) by a dict from the triple to its smallest index"""
    A, B, C, qK, T0, T1, T2 = tabs[:GIVEN]
    first = {}
    for y, row in enumerate(zip(T0, T1, T2)):
        first.setdefault(tuple(v % p for v in row), y)
    m, misses = [0] * len(A), 0
    for x, row in enumerate(zip(A, B, C)):
        if qK[x] % p == 1:
            y = first.get(tuple(v % p for v in row))
            if y is None:
                misses += 1
            else:
                m[y] += 1
    return m, misses


def satisfied(tabs, p):
    return multiplicities(tabs, p)[1] == 0


def denominators(tabs, x, beta, gamma):
    A, B, C, _, T0, T1, T2 = tabs[:GIVEN]
    return beta + A[x] + gamma * B[x] + gamma * gamma * C[x], beta + T0[x] + gamma * T1[x] + gamma * gamma * T2[x]


def fractions(tabs, beta, gamma, p):
    """H from the eight tables A, B, C, qK, T0, T1, T2, M"""
    out = []
    for x in range(len(tabs[0])):
        dw, dt = denominators(tabs, x, beta, gamma)
        out.append((tabs[3][x] * inv0(dw, p) - tabs[7][x] * inv0(dt, p)) % p)
    return out


def summand(v, e, ch):
    """the summand at one (possibly non-Boolean) point: v = the values of A, B, C, qK, T0, T1, T2, M, H there, e = E's"""
    beta, gamma, mu = ch
    dw = beta + v[0] + gamma * v[1] + gamma * gamma * v[2]
    dt = beta + v[4] + gamma * v[5] + gamma * gamma * v[6]
    return mu * v[8] + e * (v[8] * dw * dt - v[3] * dt + v[7] * dw)


def round_g5(tabs, ch, p):
    """g(0) .. g(4) along the last variable, straight from the definition; tabs: A, B, C, qK, T0, T1, T2, M, H, E"""
    g = [0] * NODES
    for x in range(len(tabs[0]) // 2):
        for X in range(NODES):
            v = [t[2 * x] + X * (t[2 * x + 1] - t[2 * x]) for t in tabs]
            g[X] += summand(v[:K], v[K], ch)
    return [v % p for v in g]


def helper_phase(i, tabs, ch, p, cheat):
    """the family's helper phases: M from the seven (a cheating prover credits every miss to row 0), then H from the eight and beta, gamma"""
    if i == 1:
        return [fractions(tabs, ch[0], ch[1], p)], {}
    m, misses = multiplicities(tabs, p)
    if cheat:
        m[0] = (m[0] + misses) % p
    return [m], {"misses": misses, "M": m}


PROTO = F.Proto(tag, GIVEN, NODES, 0, ((1, 2), (1, 1)), helper_phase, lambda v, ids, ch: summand(v[:K], v[K], ch),
                lambda tabs, extra, ch, p: (round_g5(tabs, ch, p), None), opening=BM)
pow_transcript, sizes, flat = (functools.partial(fn, PROTO) for fn in (F.pow_transcript, F.sizes, F.flat))
_helpers = functools.partial(F.helpers, PROTO)               # -> [beta, gamma, mu, tau]


def _statement(tr, roots, d):
    F.statement(PROTO, tr, roots, d, None)


def prove(cms, f, Q, a=1, tr=None, hasher=M.keccak256, cheat=False, commit=None):
    """-> the proof as a dict; `cms`: the model commitments of the seven (tests/_fri_pcs_model.py, or _fri_ml_grouped_model.py's, all alike);
    `commit(table)`: the model commitment of a helper table with their shape (commit_like on the first by default); `tr` is advanced.  The
    statement is not checked."""
    return F.prove_rounds(PROTO, cms, (), f, Q, a, tr, hasher, cheat, commit)


def verify(pr, roots=None, tr=None, hasher=M.keccak256):
    """`roots`: the verifier's own seven, the proof's unless given -> (ok, the number of the first check that failed or None): 0 the first
    round's sum, l >= 1 round l's, d the last claim, d + 1 the opening"""
    return F.replay(PROTO, pr, roots, None, tr, hasher)
