"""Python model of the permutation check over FRI commitments (helper of tests/test_wiring_cpu.py and test_gpu_wiring.py).  The definition
is the one of include/zkmle.h "Wiring: a permutation check over committed tables"; the six given tables are always in the order A, B, C, SA,
SB, SC and the nine opened ones in the order A, B, C, SA, SB, SC, H0, H1, H2:

  statement    "ZCPW" be32(d), the six roots; then beta, gamma
  helpers      H_j[x] = inv0(beta + W_j[x] + gamma (j n + x)) - inv0(beta + W_j[x] + gamma S_j[x]), inv0(0) = 0; each committed with the shape of
               the six; the three roots appended; then alpha, mu, tau_0 .. tau_{d-1}
  round l      binds the LAST variable: g_l(X) = sum_x' [ mu (H_0 + H_1 + H_2) + E sum_j alpha^j (H_j Did_j Dsig_j - gamma (S_j - ID_j)) ] at
               (x', X) with Y(x', X) the line through Y[2x'] and Y[2x'+1] and ID_j the EXPLICIT table j n + x folded like every other one; sent
               at X = 0, 1, 2, 3, 4; then r_l; every table is folded by mle_fold_last
  point        z[d - 1 - l] = r_l
  opening      tests/_fri_ml_batch_model.py open_batch of the nine at the one point z on the same transcript (through _grind_model's
               PowTranscript when the proof-of-work step is asked for)
  verifier     g_0(0) + g_0(1) = 0;  g_l(0) + g_l(1) = g_{l-1}(r_{l-1}) by Lagrange's formula through the five nodes;  the last claim against
               the relation on the nine values with id_j(z) = j 2^d + sum_i 2^(d-1-i) z_i;  the opening's verifier

`prove(.., cheat=True)` is the prover that commits to H = 0 (no fraction betrays the false cell, and the multiset part of the sum is 0) and,
because the zerocheck part of the sum is then not 0 unless S = id, hides that from the first check as the zerochecks' cheating provers do: it
sends g_0(1) = -g_0(0) and is honest afterwards.  The first check passes, a later one fails, and the opening alone verifies.
`wiring(field, d, seed)` draws a random permutation of the 3 n cells and one random value per cycle.
Everything is Python integers; nothing here knows how the library works."""
import functools
import random

import _fri_ml_batch_model as BM
import _ntt_model as NM
import _zerocheck_family_model as F
from oracle import pymodel as M

be32, eq_at, inv0, id_tables, id_at, commit_like = F.be32, F.eq_at, F.inv0, F.id_tables, F.id_at, F.commit_like
interpolate5 = F.interpolate                                 # the quartic through (0, g[0]) .. (4, g[4]) at r
WIRES, GIVEN, K, NODES = 3, 6, 9, 5


def tag(d):
    return b"ZCPW" + int(d).to_bytes(4, "big")


def cycles_of(sigma):
    """the cycles of the permutation `sigma` (a list over the 3 n cells), each as a list of cells"""
    seen, out = set(), []
    for c in range(len(sigma)):
        if c in seen:
            continue
        cyc = []
        while c not in seen:
            seen.add(c)
            cyc.append(c)
            c = sigma[c]
        out.append(cyc)
    return out


def wiring(field, d, seed, false=False, sigma=None):
    """-> ([A, B, C], [SA, SB, SC]): a random permutation of the 3 n cells (or `sigma`) and one random value per cycle.  false: one cell of a
    cycle of length >= 2 holds one more than its cycle's value (the permutation is redrawn until it has such a cycle)"""
    p, rng, n = NM.MODULUS[field], random.Random(seed), 1 << d
    while True:
        sig = list(range(WIRES * n)) if sigma is None else list(sigma)
        if sigma is None:
            rng.shuffle(sig)
        cyc = cycles_of(sig)
        long = [c for c in cyc if len(c) >= 2]
        if long or not false:
            break
    w = [0] * (WIRES * n)
    for c in cyc:
        v = rng.randrange(p)
        for cell in c:
            w[cell] = v
    if false:
        cell = rng.choice(rng.choice(long))
        w[cell] = (w[cell] + 1) % p
    return [w[j * n:(j + 1) * n] for j in range(WIRES)], [sig[j * n:(j + 1) * n] for j in range(WIRES)]


def satisfied(ws, ss, p):
    flat = [v for t in ws for v in t]
    return all(flat[s] % p == v % p for t, st in zip(ws, ss) for v, s in zip(t, st))


def fractions(W, S, first, beta, gamma, p):
    return [(inv0(beta + w + gamma * (first + x), p) - inv0(beta + w + gamma * s, p)) % p for x, (w, s) in enumerate(zip(W, S))]


def summand(ws, ss, hs, ids, e, ch):
    """the summand at one (possibly non-Boolean) point: the values of the three W, S, H, ID there and of E"""
    beta, gamma, alpha, mu = ch
    zc = sum(alpha ** j * (h * (beta + w + gamma * i) * (beta + w + gamma * s) - gamma * (s - i)) for j, (w, s, h, i) in enumerate(zip(ws, ss, hs, ids)))
    return mu * sum(hs) + e * zc


def round_g5(tabs, ids, ch, p):
    """g(0) .. g(4) along the last variable, straight from the definition; tabs: A, B, C, SA, SB, SC, H0, H1, H2, E; ids: the three id tables"""
    g = [0] * NODES
    for x in range(len(tabs[0]) // 2):
        for X in range(NODES):
            v = [t[2 * x] + X * (t[2 * x + 1] - t[2 * x]) for t in tabs]
            i = [t[2 * x] + X * (t[2 * x + 1] - t[2 * x]) for t in ids]
            g[X] += summand(v[0:3], v[3:6], v[6:9], i, v[9], ch)
    return [v % p for v in g]


def helper_phase(i, tabs, ch, p, cheat):
    """the family's helper phase: H0, H1, H2 from A, B, C, SA, SB, SC at the first places of `tabs` and beta, gamma; all zero when cheating"""
    n = len(tabs[0])
    return [[0] * n if cheat else fractions(tabs[j], tabs[GIVEN - WIRES + j], j * n, ch[0], ch[1], p) for j in range(WIRES)], {}


PROTO = F.Proto(tag, GIVEN, NODES, 2, ((WIRES, 2),), helper_phase, lambda v, ids, ch: summand(v[0:3], v[3:6], v[6:9], ids, v[9], ch),
                lambda tabs, ids, ch, p: (round_g5(tabs, ids, ch, p), None), lambda d, pub: id_tables(d), opening=BM)
pow_transcript, sizes, flat = (functools.partial(fn, PROTO) for fn in (F.pow_transcript, F.sizes, F.flat))
_statement, _helpers = functools.partial(F.statement, PROTO), functools.partial(F.helpers, PROTO)      # -> [beta, gamma]; -> [alpha, mu, tau]


def prove(cms, f, Q, a=1, tr=None, hasher=M.keccak256, cheat=False, commit=None):
    """-> the proof as a dict; `cms`: the model commitments of the six (tests/_fri_pcs_model.py, or _fri_ml_grouped_model.py's, all alike);
    `commit(table)`: the model commitment of a helper table with their shape (commit_like on the first by default); `tr` is advanced.  The
    statement is not checked."""
    return F.prove_rounds(PROTO, cms, (), f, Q, a, tr, hasher, cheat, commit)


def verify(pr, roots=None, tr=None, hasher=M.keccak256):
    """`roots`: the verifier's own six, the proof's unless given -> (ok, the number of the first check that failed or None): 0 the first
    round's sum, l >= 1 round l's, d the last claim, d + 1 the opening"""
    return F.replay(PROTO, pr, roots, None, tr, hasher)
