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
import numpy as np

import _fri_ml_batch_model as BM
import _fri_ml_model as ML
import _grind_model as GR
import _ntt_model as NM
from oracle import pymodel as M

be32 = ML.be32


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


def interpolate4(g, r, p):
    """the cubic through (0, g[0]) .. (3, g[3]) at r, by Lagrange's formula"""
    out = 0
    for i in range(4):
        num, den = 1, 1
        for j in range(4):
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
    """-> the proof as a dict; `cms`: the model commitments of A, B, C (tests/_fri_pcs_model.py, or _fri_ml_grouped_model.py's, all alike);
    `tr` is advanced.  The relation is not checked."""
    field, d = cms[0]["field"], cms[0]["d"]
    p = NM.MODULUS[field]
    tr = M.Transcript() if tr is None else tr
    roots = [c["root"] for c in cms]
    tau = _statement(tr, roots, d, p)
    A, B, C = (list(c["coeffs"]) for c in cms)
    E = ML.eq_table(tau, p)
    polys, rs = [], []
    for l in range(d):
        g = round_g4(A, B, C, E, p)
        if cheat and l == 0:
            g[1] = -g[0] % p
        polys.append(g)
        for e in g:
            tr.append(be32(e))
        r = tr.challenge(p)
        rs.append(r)
        A, B, C, E = (ML.mle_fold_last(field, t, r) for t in (A, B, C, E))
    z = rs[::-1]
    op = BM.open_batch(cms, [z], f, Q, a, tr, hasher)
    assert [row[0] for row in op["ys"]] == [A[0], B[0], C[0]] and E[0] == eq_at(z, tau, p)
    return {"field": field, "d": d, "roots": roots, "tau": tau, "polys": polys, "challenges": rs, "opening": op,
            "nonce": getattr(tr, "nonce", None) or 0}


def verify(pr, roots=None, tr=None, hasher=M.keccak256):
    """`roots`: the verifier's own three, the proof's unless given -> (ok, the number of the first check that failed or None): 0 the first
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
        cur = interpolate4(g, rs[l], p)
    z = rs[::-1]
    ya, yb, yc = (row[0] for row in op["ys"])
    if failed is None and cur != eq_at(z, tau, p) * (ya * yb - yc) % p:
        failed = d
    good = BM.verify(dict(op, own_roots=list(roots), points=[z]), tr, hasher) and getattr(tr, "pow_ok", None) is not False
    if failed is None and not good:
        failed = d + 1
    return failed is None, failed


def sizes(d, b, f, Q, a=1, grouped=False):
    """(nzc_round,) + the batch model's five counts at k = 3"""
    return (4 * d,) + BM.sizes(3, d, b, f, Q, a, grouped)


def flat(zk, pr):
    """the proof as the C outputs: tau (d, 4), polys (d, 4, 4), challenges (d, 4), own_roots (3, 32), and the opening's arrays of
    _fri_ml_batch_model.flat under their names there with ys as (3, 4) and the opening's round polynomials as open_polys / open_challenges"""
    field, d = pr["field"], pr["d"]

    def mont(ints):
        canon = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), np.uint64).reshape(-1, 4).copy()
        out = np.zeros_like(canon)
        assert zk.lib().zk_vec_from_canonical(field, canon.ctypes.data_as(zk._lib.u64p), canon.shape[0], out.ctypes.data_as(zk._lib.u64p)) == 0
        return out

    fl = BM.flat(zk, pr["opening"])
    fl["open_polys"], fl["open_challenges"] = fl.pop("polys"), fl.pop("challenges")
    fl["ys"] = fl["ys"].reshape(3, 4)
    fl.update(tau=mont(pr["tau"]), polys=mont([e for g in pr["polys"] for e in g]).reshape(d, 4, 4), challenges=mont(pr["challenges"]))
    return fl
