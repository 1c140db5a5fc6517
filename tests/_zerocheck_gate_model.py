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
import random

import numpy as np

import _fri_ml_batch_model as BM
import _fri_ml_model as ML
import _grind_model as GR
import _ntt_model as NM
from oracle import pymodel as M

be32 = ML.be32
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


def interpolate5(g, r, p):
    """the quartic through (0, g[0]) .. (4, g[4]) at r, by Lagrange's formula"""
    out = 0
    for i in range(NODES):
        num, den = 1, 1
        for j in range(NODES):
            if j != i:
                num, den = num * (r - j) % p, den * (i - j) % p
        out += g[i] * num * pow(den, -1, p)
    return out % p


def eq_at(z, tau, p):
    out = 1
    for a, b in zip(z, tau):
        out = out * ML.eq1(a, b, p) % p
    return out


def _statement(tr, roots, d, p):
    tr.append(tag(d))
    for r in roots:
        tr.append(r)
    return [tr.challenge(p) for _ in range(d)]


def pow_transcript(d, f, bits, nonce=None, prefix=b""):
    """the transcript of a proof with the proof-of-work step: it stands in front of the first index, sample number d (tau) + d (the rounds) + 1
    (the opening's gamma) + R (its rounds)"""
    tr = GR.PowTranscript(bits, 2 * d + 1 + (d - f), nonce)
    tr.append(prefix)
    return tr


def prove(cms, f, Q, a=1, tr=None, hasher=M.keccak256, cheat=False):
    """-> the proof as a dict; `cms`: the model commitments of the eight (tests/_fri_pcs_model.py, or _fri_ml_grouped_model.py's, all alike);
    `tr` is advanced.  The relation is not checked."""
    field, d = cms[0]["field"], cms[0]["d"]
    assert len(cms) == K
    p = NM.MODULUS[field]
    tr = M.Transcript() if tr is None else tr
    roots = [c["root"] for c in cms]
    tau = _statement(tr, roots, d, p)
    tabs = [list(c["coeffs"]) for c in cms] + [ML.eq_table(tau, p)]
    polys, rs = [], []
    for l in range(d):
        g = round_g5(tabs, p)
        if cheat and l == 0:
            g[1] = -g[0] % p
        polys.append(g)
        for e in g:
            tr.append(be32(e))
        r = tr.challenge(p)
        rs.append(r)
        tabs = [ML.mle_fold_last(field, t, r) for t in tabs]
    z = rs[::-1]
    op = BM.open_batch(cms, [z], f, Q, a, tr, hasher)
    assert [row[0] for row in op["ys"]] == [t[0] for t in tabs[:K]] and tabs[K][0] == eq_at(z, tau, p)
    return {"field": field, "d": d, "roots": roots, "tau": tau, "polys": polys, "challenges": rs, "opening": op,
            "nonce": getattr(tr, "nonce", None) or 0}


def verify(pr, roots=None, tr=None, hasher=M.keccak256):
    """`roots`: the verifier's own eight, the proof's unless given -> (ok, the number of the first check that failed or None): 0 the first
    round's sum, l >= 1 round l's, d the last claim, d + 1 the opening"""
    field, d, op = pr["field"], pr["d"], pr["opening"]
    p = NM.MODULUS[field]
    tr = M.Transcript() if tr is None else tr
    roots = pr["roots"] if roots is None else roots
    tau = _statement(tr, roots, d, p)
    cur, rs, failed = 0, [], None
    for l in range(d):
        g = pr["polys"][l]
        for e in g:
            tr.append(be32(e % p))
        if failed is None and (any(not 0 <= e < p for e in g) or (g[0] + g[1]) % p != cur):
            failed = l
        rs.append(tr.challenge(p))
        cur = interpolate5(g, rs[l], p)
    z = rs[::-1]
    ys = [row[0] for row in op["ys"]]
    if failed is None and cur != eq_at(z, tau, p) * gate(*ys) % p:
        failed = d
    good = BM.verify(dict(op, own_roots=list(roots), points=[z]), tr, hasher) and getattr(tr, "pow_ok", None) is not False
    if failed is None and not good:
        failed = d + 1
    return failed is None, failed


def sizes(d, b, f, Q, a=1, grouped=False):
    """(nzc_round,) + the batch model's five counts at k = 8"""
    return (NODES * d,) + BM.sizes(K, d, b, f, Q, a, grouped)


def flat(zk, pr):
    """the proof as the C outputs: tau (d, 4), polys (d, 5, 4), challenges (d, 4), own_roots (8, 32), and the opening's arrays of
    _fri_ml_batch_model.flat under their names there with ys as (8, 4) and the opening's round polynomials as open_polys / open_challenges"""
    field, d = pr["field"], pr["d"]

    def mont(ints):
        canon = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), np.uint64).reshape(-1, 4).copy()
        out = np.zeros_like(canon)
        assert zk.lib().zk_vec_from_canonical(field, canon.ctypes.data_as(zk._lib.u64p), canon.shape[0], out.ctypes.data_as(zk._lib.u64p)) == 0
        return out

    fl = BM.flat(zk, pr["opening"])
    fl["open_polys"], fl["open_challenges"] = fl.pop("polys"), fl.pop("challenges")
    fl["ys"] = fl["ys"].reshape(K, 4)
    fl.update(tau=mont(pr["tau"]), polys=mont([e for g in pr["polys"] for e in g]).reshape(d, NODES, 4), challenges=mont(pr["challenges"]))
    return fl
