"""Python model of the zerocheck of a Plonk gate over eight FRI commitments (helper of tests/test_zerocheck_gate_cpu.py and
test_gpu_zerocheck_gate.py).  The definition is the one of include/zkmle.h "Zerocheck of a Plonk gate over committed tables"; the eight
tables are always in the order A, B, C, qM, qL, qR, qO, qC:

  statement    "ZCPG" be32(d), the eight roots; then tau_0 .. tau_{d-1}, d challenges
  round l      binds the LAST variable: g_l(X) = sum_x' E_l (qM_l A_l B_l + qL_l A_l + qR_l B_l + qO_l C_l + qC_l) at (x', X) with Y(x', X) the
               line through Y[2x'] and Y[2x'+1], sent at X = 0, 1, 2, 3, 4; then r_l; every table is folded by mle_fold_last
  point        z[d - 1 - l] = r_l
  opening      tests/_fri_ml_batch_model.py open_batch of the eight at the one point z on the same transcript (through _grind_model's
               PowTranscript when the proof-of-work step is asked for)
  verifier     g_0(0) + g_0(1) = 0;  g_l(0) + g_l(1) = g_{l-1}(r_{l-1}) by the quartic through the five nodes;
               g_{d-1}(r_{d-1}) = eq(z, tau) (y_qM y_A y_B + y_qL y_A + y_qR y_B + y_qO y_C + y_qC);  the opening's verifier

`prove(.., cheat=True)` is the prover that hides a false statement from the first check: it sends g_0(1) = -g_0(0) and is honest afterwards.
`circuit(field, n, seed)` makes a satisfied statement whose selectors sit mostly at 0, 1 and p - 1.
Everything is Python integers; nothing here knows how the library works."""
import functools
import random

import _fri_ml_batch_model as BM
import _ntt_model as NM
import _zerocheck_family_model as F
from oracle import pymodel as M

be32, eq_at, interpolate5 = F.be32, F.eq_at, F.interpolate             # the quartic through (0, g[0]) .. (4, g[4]) at r
K, NODES = 8, 5


def tag(d):
    return b"ZCPG" + int(d).to_bytes(4, "big")


def gate(a, b, c, qm, ql, qr, qo, qc):
    return qm * a * b + ql * a + qr * b + qo * c + qc


def circuit(field, n, seed, false_at=None):
    """-> [A, B, C, qM, qL, qR, qO, qC], n rows that satisfy the gate: additions (qL = qR = 1, qO = p - 1), multiplications (qM = 1,
    qO = p - 1), constant rows (qL = 1, qC = -c, A = c) and rows of random selectors with qO != 0 and C solved for; the first four rows are
    one of each where n allows.  false_at: qC at that row is one more, so the gate is 1 there whatever the row's kind"""
    p, rng = NM.MODULUS[field], random.Random(seed)
    cols = [[] for _ in range(K)]
    for x in range(n):
        kind = x % 4 if x < 4 else rng.randrange(4)
        a, b = rng.randrange(p), rng.randrange(p)
        if kind == 0:
            row = (a, b, (a + b) % p, 0, 1, 1, p - 1, 0)
        elif kind == 1:
            row = (a, b, a * b % p, 1, 0, 0, p - 1, 0)
        elif kind == 2:
            row = (a, b, rng.randrange(p), 0, 1, 0, 0, -a % p)
        else:
            qm, ql, qr, qc = (rng.randrange(p) for _ in range(4))
            qo = rng.randrange(1, p)
            row = (a, b, -(qm * a * b + ql * a + qr * b + qc) * pow(qo, -1, p) % p, qm, ql, qr, qo, qc)
        assert gate(*row) % p == 0
        for col, v in zip(cols, row):
            col.append(v)
    if false_at is not None:
        cols[7][false_at] = (cols[7][false_at] + 1) % p
    return cols


def round_g5(tabs, p):
    """g(0) .. g(4) of sum_x' E gate(A, B, C, qM, qL, qR, qO, qC) along the last variable, straight from the definition; tabs: the eight, then E"""
    g = [0] * NODES
    for x in range(len(tabs[0]) // 2):
        for X in range(NODES):
            *w, e = (t[2 * x] + X * (t[2 * x + 1] - t[2 * x]) for t in tabs)
            g[X] += e * gate(*w)
    return [v % p for v in g]


PROTO = F.Proto(tag, K, NODES, summand=lambda v, ids, ch: v[K] * gate(*v[:K]), message=lambda tabs, extra, ch, p: (round_g5(tabs, p), None), opening=BM)
pow_transcript, sizes, flat = (functools.partial(fn, PROTO) for fn in (F.pow_transcript, F.sizes, F.flat))


def _statement(tr, roots, d, p):
    return F.helpers(PROTO, tr, [], d, p, F.statement(PROTO, tr, roots, d, p))[-1]


def prove(cms, f, Q, a=1, tr=None, hasher=M.keccak256, cheat=False):
    """-> the proof as a dict; `cms`: the model commitments of the eight (tests/_fri_pcs_model.py, or _fri_ml_grouped_model.py's, all alike);
    `tr` is advanced.  The relation is not checked."""
    return F.prove_rounds(PROTO, cms, (), f, Q, a, tr, hasher, cheat)


def verify(pr, roots=None, tr=None, hasher=M.keccak256):
    """`roots`: the verifier's own eight, the proof's unless given -> (ok, the number of the first check that failed or None): 0 the first
    round's sum, l >= 1 round l's, d the last claim, d + 1 the opening"""
    return F.replay(PROTO, pr, roots, None, tr, hasher)
