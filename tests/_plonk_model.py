"""Python model of the Plonk proof over FRI commitments (helper of tests/test_plonk_cpu.py, test_gpu_plonk.py and _plonk_worker.py).  The
definition is the one of include/zkmle.h "Plonk: gate, wiring and public inputs in one sumcheck"; the eleven given tables are always in the
order A, B, C, qM, qL, qR, qO, qC, SA, SB, SC and the fourteen opened ones in that order followed by H0, H1, H2.  Built on _wiring_model (the
helper tables, the wiring's summand, the id tables), _zerocheck_gate_model (the gate) and _fri_ml_batch_model (the opening):

  statement    "ZCPK" be32(d) be32(l) in one append, the eleven roots, the l public values as 32-byte big-endian elements; then beta, gamma
  helpers      _wiring_model's: H_j, their commitments, the three roots; then alpha, mu, tau_0 .. tau_{d-1}
  the sum      the model keeps the public inputs where the statement has them, INSIDE the zerocheck: with the EXPLICIT table PI (pi_x for x < l,
               0 otherwise) and the explicit id tables, folded like every other table, the polynomial that is summed is
                   F = mu (H_0 + H_1 + H_2) + E [ sum_j alpha^j (H_j Did_j Dsig_j - gamma (S_j - ID_j)) + alpha^3 (gate(A, B, C, q..) - PI) ]
               and its claimed sum is 0.  The protocol sends the round polynomial of F + alpha^3 E PI, whose claimed sum is alpha^3 sum_x E PI:
               the model forms a round's message as (the round polynomial of F) + (the round polynomial of alpha^3 E PI from the folded explicit
               PI table) and asserts for a satisfied circuit that F's own first message sums to 0.  That these bytes are the library's, which never
               sees a PI table, checks the step that takes the public inputs to the claimed side.
  round l      binds the LAST variable, the message at X = 0 .. 4; then r_l; every table is folded by mle_fold_last
  opening      open_batch of the fourteen at z, z[d - 1 - l] = r_l, on the same transcript
  verifier     g_0(0) + g_0(1) - alpha^3 sum_x PI[x] E_0[x] = 0 on the explicit tables;  g_l(0) + g_l(1) = g_{l-1}(r_{l-1});  the last claim against the
               summand without PI on the fourteen values;  the opening's verifier.  A public value outside [0, p) is rejected.

`prove(.., cheat=True)` is _wiring_model's cheating prover here: it commits H = 0 and sends g_0(1) = c - g_0(0).
`circuit(field, d, seed, l, ..)` builds a small wired circuit whose first l rows are public-input rows.
Everything is Python integers; nothing here knows how the library works."""
import functools
import random

import _fri_ml_batch_model as BM
import _fri_ml_model as ML
import _ntt_model as NM
import _wiring_model as WM
import _zerocheck_family_model as F
import _zerocheck_gate_model as ZG
from oracle import pymodel as M

be32, mont = F.be32, F.mont
WIRES, GIVEN, K, NODES, TABLES = 3, 11, 14, 5, 15
W_PLACES, Q_PLACES, S_PLACES, H_PLACES, E_PLACE = (0, 1, 2), (3, 4, 5, 6, 7), (8, 9, 10), (11, 12, 13), 14
interpolate5, eq_at, id_at, commit_like = F.interpolate, F.eq_at, F.id_at, F.commit_like


def tag(d, l):
    return b"ZCPK" + int(d).to_bytes(4, "big") + int(l).to_bytes(4, "big")


def pi_table(pub, d):
    return list(pub) + [0] * ((1 << d) - len(pub))


def public_eval(pub, tau, p):
    """sum_{x < l} pi_x eq(x, tau) straight from the definition: variable 0 is the most significant index bit"""
    d, out = len(tau), 0
    for x, v in enumerate(pub):
        out += v * eq_at([(x >> (d - 1 - i)) & 1 for i in range(d)], tau, p)
    return out % p


def sigma_of(kind, d):
    """the permutation of the 3 n cells of one kind: the identity, one 3-cycle across A, B, C; None for a random one"""
    n = 1 << d
    if kind == "random":
        return None
    sig = list(range(WIRES * n))
    if kind == "3-cycle":
        a, b, c = 0 * n + (n - 1), 1 * n + 0, 2 * n + (n // 2)
        sig[a], sig[b], sig[c] = b, c, a
    return sig


def circuit(field, d, seed, l=0, kind="random", false_gate=False, false_wiring=False):
    """-> (the eleven tables, the l public values).  The wires take one random value per cycle of the wiring (_wiring_model.wiring); row x < l is a
    public-input row (qL = 1, the other selectors 0, pi_x = A[x]); a later row is an addition (qL = qR = 1, qO = p - 1), a multiplication (qM = 1,
    qO = p - 1) or a row of random selectors, each with qC solved for the wires' values.  false_gate: qC of one row is one more; false_wiring:
    one cell of a cycle holds one more than its cycle's value (and the selectors are solved for the wires as they then are)"""
    p, rng, n = NM.MODULUS[field], random.Random(seed ^ 0x504C), 1 << d
    assert 0 <= l <= n
    ws, ss = WM.wiring(field, d, seed, false_wiring, sigma_of(kind, d))
    sel = [[0] * n for _ in range(5)]
    for x in range(n):
        a, b, c = ws[0][x], ws[1][x], ws[2][x]
        if x < l:
            row = [0, 1, 0, 0, 0]
        else:
            which = (x - l) % 3 if x - l < 3 else rng.randrange(3)
            row = [0, 1, 1, p - 1] if which == 0 else [1, 0, 0, p - 1] if which == 1 else [rng.randrange(p) for _ in range(4)]
            row.append(-ZG.gate(a, b, c, *row, 0) % p)
        for col, v in zip(sel, row):
            col[x] = v
    pub = [ws[0][x] for x in range(l)]
    if false_gate:
        x = rng.randrange(n)
        sel[4][x] = (sel[4][x] + 1) % p
    return ws + sel + ss, pub


def satisfied(tabs, pub, p):
    """both parts of the statement on the eleven integer tables"""
    d = len(tabs[0]).bit_length() - 1
    rows = zip(*tabs[:8], pi_table(pub, d))
    return all((ZG.gate(*row[:8]) - row[8]) % p == 0 for row in rows), WM.satisfied(tabs[0:3], tabs[8:11], p)


def summand(v, ids, ch, pi=0):
    """F at one (possibly non-Boolean) point: v = the values of the fifteen tables there, ids of the three id tables, pi of the PI table"""
    beta, gamma, alpha, mu = ch
    ws, qs, ss, hs, e = [v[i] for i in W_PLACES], [v[i] for i in Q_PLACES], [v[i] for i in S_PLACES], [v[i] for i in H_PLACES], v[E_PLACE]
    return WM.summand(ws, ss, hs, ids, e, ch) + e * alpha ** 3 * (ZG.gate(*ws, *qs) - pi)


def round_g5(tabs, ids, ch, p, pi=None, summand=summand, E_PLACE=E_PLACE):
    """-> (the message g(0) .. g(4) as the protocol sends it, the round polynomial of F itself at the five nodes), straight from the definition;
    tabs: the fifteen; ids: the three id tables; pi: the PI table (all zero when None).  summand, E_PLACE: a wider relation's, _plonk_lookup_model's"""
    alpha = ch[2]
    pi = [0] * len(tabs[0]) if pi is None else pi
    line = lambda t, x, X: t[2 * x] + X * (t[2 * x + 1] - t[2 * x])
    f, moved = [0] * NODES, [0] * NODES
    for x in range(len(tabs[0]) // 2):
        for X in range(NODES):
            v, i, q = [line(t, x, X) for t in tabs], [line(t, x, X) for t in ids], line(pi, x, X)
            f[X] += summand(v, i, ch, q)
            moved[X] += alpha ** 3 * v[E_PLACE] * q
    return [(a + b) % p for a, b in zip(f, moved)], [a % p for a in f]


def claimed_sum(pub, tau, ch, p):
    """alpha^3 sum_x PI[x] E[x] on the explicit tables, which is alpha^3 public_eval"""
    out = ch[2] ** 3 * sum(a * b for a, b in zip(pi_table(pub, len(tau)), ML.eq_table(tau, p))) % p
    assert out == ch[2] ** 3 * public_eval(pub, tau, p) % p
    return out


def explicit_tables(d, pub):
    return F.id_tables(d) + [pi_table(pub, d)]


PROTO = F.Proto(tag, GIVEN, NODES, 2, ((WIRES, 2),), lambda i, tabs, ch, p, cheat: WM.helper_phase(i, tabs[:3] + tabs[8:11], ch, p, cheat), summand,
                lambda tabs, x, ch, p: round_g5(tabs, x[:WIRES], ch, p, x[WIRES]), explicit_tables, claimed_sum, BM)
pow_transcript, sizes, flat = (functools.partial(fn, PROTO) for fn in (F.pow_transcript, F.sizes, F.flat))
_statement = lambda tr, roots, d, pub, p: F.statement(PROTO, tr, roots, d, p, pub)      # -> [beta, gamma]


def prove(cms, pub, f, Q, a=1, tr=None, hasher=M.keccak256, cheat=False):
    """-> the proof as a dict; `cms`: the model commitments of the eleven (all alike); `pub`: the public values; `tr` is advanced.  The
    statement is not checked."""
    return F.prove_rounds(PROTO, cms, pub, f, Q, a, tr, hasher, cheat)


def verify(pr, roots=None, pub=None, tr=None, hasher=M.keccak256):
    """`roots`, `pub`: the verifier's own eleven and its public values, the proof's unless given -> (ok, the number of the first check that failed
    or None): 0 the first round's sum (or a public value outside the field), l >= 1 round l's, d the last claim, d + 1 the opening"""
    return F.replay(PROTO, pr, roots, pub, tr, hasher)
