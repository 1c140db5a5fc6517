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
import random

import numpy as np

import _fri_ml_batch_model as BM
import _fri_ml_model as ML
import _grind_model as GR
import _ntt_model as NM
import _wiring_model as WM
from oracle import pymodel as M

be32 = ML.be32
inv0, interpolate5, eq_at, commit_like = WM.inv0, WM.interpolate5, WM.eq_at, WM.commit_like
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


def pow_transcript(d, f, bits, nonce=None, prefix=b""):
    """the transcript of a proof with the proof-of-work step: it stands in front of the first index, sample number 2 (beta, gamma) + 1 (mu) + d
    (tau) + d (the rounds) + 1 (the opening's gamma) + R (its rounds)"""
    tr = GR.PowTranscript(bits, 3 + 2 * d + 1 + (d - f), nonce)
    tr.append(prefix)
    return tr


def _statement(tr, roots, d):
    tr.append(tag(d))
    for r in roots:
        tr.append(r)


def _helpers(tr, h_roots, d, p):
    tr.append(h_roots[0])
    beta, gamma = tr.challenge(p), tr.challenge(p)
    tr.append(h_roots[1])
    mu = tr.challenge(p)
    return beta, gamma, mu, [tr.challenge(p) for _ in range(d)]


def prove(cms, f, Q, a=1, tr=None, hasher=M.keccak256, cheat=False, commit=None):
    """-> the proof as a dict; `cms`: the model commitments of the seven (tests/_fri_pcs_model.py, or _fri_ml_grouped_model.py's, all alike);
    `commit(table)`: the model commitment of a helper table with their shape (commit_like on the first by default); `tr` is advanced.  The
    statement is not checked."""
    field, d = cms[0]["field"], cms[0]["d"]
    assert len(cms) == GIVEN
    p = NM.MODULUS[field]
    tr = M.Transcript() if tr is None else tr
    roots = [c["root"] for c in cms]
    commit = (lambda t: commit_like(cms[0], t, hasher)) if commit is None else commit
    _statement(tr, roots, d)
    given = [list(c["coeffs"]) for c in cms]
    m, misses = multiplicities(given, p)
    if cheat:
        m[0] = (m[0] + misses) % p
    mcm = commit(m)
    tr.append(mcm["root"])
    beta, gamma = tr.challenge(p), tr.challenge(p)
    h = fractions(given + [m], beta, gamma, p)
    hcm = commit(h)
    tr.append(hcm["root"])
    mu = tr.challenge(p)
    tau = [tr.challenge(p) for _ in range(d)]
    ch = (beta, gamma, mu)
    tabs = given + [m, h, ML.eq_table(tau, p)]
    polys, rs = [], []
    for l in range(d):
        g = round_g5(tabs, ch, p)
        if cheat and l == 0:
            g[1] = -g[0] % p
        polys.append(g)
        for e in g:
            tr.append(be32(e))
        r = tr.challenge(p)
        rs.append(r)
        tabs = [ML.mle_fold_last(field, t, r) for t in tabs]
    z = rs[::-1]
    op = BM.open_batch(list(cms) + [mcm, hcm], [z], f, Q, a, tr, hasher)
    assert [row[0] for row in op["ys"]] == [t[0] for t in tabs[:K]] and tabs[K][0] == eq_at(z, tau, p)
    return {"field": field, "d": d, "roots": roots, "h_roots": [mcm["root"], hcm["root"]], "drawn": [beta, gamma, mu] + tau, "polys": polys, "challenges": rs,
            "opening": op, "misses": misses, "M": m, "nonce": getattr(tr, "nonce", None) or 0}


def verify(pr, roots=None, tr=None, hasher=M.keccak256):
    """`roots`: the verifier's own seven, the proof's unless given -> (ok, the number of the first check that failed or None): 0 the first
    round's sum, l >= 1 round l's, d the last claim, d + 1 the opening"""
    field, d, op = pr["field"], pr["d"], pr["opening"]
    p = NM.MODULUS[field]
    tr = M.Transcript() if tr is None else tr
    roots = pr["roots"] if roots is None else roots
    _statement(tr, roots, d)
    beta, gamma, mu, tau = _helpers(tr, pr["h_roots"], d, p)
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
    want = summand(ys, eq_at(z, tau, p), (beta, gamma, mu)) % p
    if failed is None and cur != want:
        failed = d
    good = BM.verify(dict(op, own_roots=list(roots) + list(pr["h_roots"]), points=[z]), tr, hasher) and getattr(tr, "pow_ok", None) is not False
    if failed is None and not good:
        failed = d + 1
    return failed is None, failed


def sizes(d, b, f, Q, a=1, grouped=False):
    """(nround, nhroots) + the batch model's five counts at k = 9"""
    return (NODES * d, HELPERS) + BM.sizes(K, d, b, f, Q, a, grouped)


def flat(zk, pr):
    """the proof as the C outputs: drawn (3 + d, 4), polys (d, 5, 4), challenges (d, 4), own_roots (7, 32), h_roots (2, 32), and the opening's
    arrays of _fri_ml_batch_model.flat under their names there with ys as (9, 4) and the opening's round polynomials as open_polys /
    open_challenges"""
    field, d = pr["field"], pr["d"]

    def mont(ints):
        canon = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), np.uint64).reshape(-1, 4).copy()
        out = np.zeros_like(canon)
        assert zk.lib().zk_vec_from_canonical(field, canon.ctypes.data_as(zk._lib.u64p), canon.shape[0], out.ctypes.data_as(zk._lib.u64p)) == 0
        return out

    fl = BM.flat(zk, pr["opening"])
    fl["open_polys"], fl["open_challenges"] = fl.pop("polys"), fl.pop("challenges")
    fl["ys"] = fl["ys"].reshape(K, 4)
    fl["own_roots"] = np.frombuffer(b"".join(pr["roots"]), np.uint8).reshape(GIVEN, 32).copy()
    fl["h_roots"] = np.frombuffer(b"".join(pr["h_roots"]), np.uint8).reshape(HELPERS, 32).copy()
    fl.update(drawn=mont(pr["drawn"]), polys=mont([e for g in pr["polys"] for e in g]).reshape(d, NODES, 4), challenges=mont(pr["challenges"]))
    return fl
