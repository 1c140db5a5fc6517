"""Python model of the zerocheck of a product over three FRI commitments (helper of tests/test_zerocheck_cpu.py and test_gpu_zerocheck.py).
The definition is the one of include/zkmle.h "Zerocheck of a product of committed tables":

  statement    "ZCML" be32(d), the roots of A, B, C; then tau_0 .. tau_{d-1}, d challenges
  round l      binds the LAST variable: g_l(X) = sum_x' E_l(x', X) (A_l(x', X) B_l(x', X) - C_l(x', X)) with Y(x', X) the line through Y[2x'] and
               Y[2x'+1], sent at X = 0, 1, 2, 3; then r_l; every table is folded by mle_fold_last
  point        z[d - 1 - l] = r_l
  opening      tests/_fri_ml_batch_model.py open_batch of (A, B, C) at the one point z on the same transcript (through _grind_model's
               PowTranscript when the proof-of-work step is asked for)
  verifier     g_0(0) + g_0(1) = 0;  g_l(0) + g_l(1) = g_{l-1}(r_{l-1});  g_{d-1}(r_{d-1}) = eq(z, tau) (yA yB - yC);  the opening's verifier

`prove(.., cheat=True)` is the prover that hides a false statement from the first check: it sends g_0(1) = -g_0(0) and is honest afterwards.
Everything is Python integers; nothing here knows how the library works."""
import functools

import _fri_ml_batch_model as BM
import _zerocheck_family_model as F
from oracle import pymodel as M

be32, eq_at, interpolate4 = F.be32, F.eq_at, F.interpolate             # the cubic through (0, g[0]) .. (3, g[3]) at r


def tag(d):
    return b"ZCML" + int(d).to_bytes(4, "big")


def round_g4(A, B, C, E, p):
    """g(0), g(1), g(2), g(3) of sum_x' E (A B - C) along the last variable, straight from the definition"""
    g = [0, 0, 0, 0]
    for x in range(len(A) // 2):
        for X in range(4):
            a, b, c, e = (t[2 * x] + X * (t[2 * x + 1] - t[2 * x]) for t in (A, B, C, E))
            g[X] += e * (a * b - c)
    return [v % p for v in g]


PROTO = F.Proto(tag, 3, 4, summand=lambda v, ids, ch: v[3] * (v[0] * v[1] - v[2]), message=lambda tabs, extra, ch, p: (round_g4(*tabs, p), None),
                opening=BM)
pow_transcript, sizes, flat = (functools.partial(fn, PROTO) for fn in (F.pow_transcript, F.sizes, F.flat))


def _statement(tr, roots, d, p):
    return F.helpers(PROTO, tr, [], d, p, F.statement(PROTO, tr, roots, d, p))[-1]


def prove(cms, f, Q, a=1, tr=None, hasher=M.keccak256, cheat=False):
    """-> the proof as a dict; `cms`: the model commitments of A, B, C (tests/_fri_pcs_model.py, or _fri_ml_grouped_model.py's, all alike);
    `tr` is advanced.  The relation is not checked."""
    return F.prove_rounds(PROTO, cms, (), f, Q, a, tr, hasher, cheat)


def verify(pr, roots=None, tr=None, hasher=M.keccak256):
    """`roots`: the verifier's own three, the proof's unless given -> (ok, the number of the first check that failed or None): 0 the first
    round's sum, l >= 1 round l's, d the last claim, d + 1 the opening"""
    return F.replay(PROTO, pr, roots, None, tr, hasher)
