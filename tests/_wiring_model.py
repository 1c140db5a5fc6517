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
import random

import numpy as np

import _fri_ml_batch_model as BM
import _fri_ml_grouped_model as GM
import _fri_ml_model as ML
import _fri_pcs_model as PM
import _grind_model as GR
import _ntt_model as NM
from oracle import pymodel as M

be32 = ML.be32
WIRES, GIVEN, K, NODES = 3, 6, 9, 5


def tag(d):
    return b"ZCPW" + int(d).to_bytes(4, "big")


def inv0(a, p):
    return 0 if a % p == 0 else pow(a, -1, p)


def id_tables(d):
    n = 1 << d
    return [[j * n + x for x in range(n)] for j in range(WIRES)]


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


def id_at(j, z, d, p):
    """the closed form of the multilinear extension of id_j at z: variable 0 is the most significant index bit"""
    return (j * (1 << d) + sum((1 << (d - 1 - i)) * zi for i, zi in enumerate(z))) % p


def _statement(tr, roots, d, p):
    tr.append(tag(d))
    for r in roots:
        tr.append(r)
    return tr.challenge(p), tr.challenge(p)


def _helpers(tr, h_roots, d, p):
    for r in h_roots:
        tr.append(r)
    alpha, mu = tr.challenge(p), tr.challenge(p)
    return alpha, mu, [tr.challenge(p) for _ in range(d)]


def pow_transcript(d, f, bits, nonce=None, prefix=b""):
    """the transcript of a proof with the proof-of-work step: it stands in front of the first index, sample number 2 (beta, gamma) + 2 (alpha,
    mu) + d (tau) + d (the rounds) + 1 (the opening's gamma) + R (its rounds)"""
    tr = GR.PowTranscript(bits, 4 + 2 * d + 1 + (d - f), nonce)
    tr.append(prefix)
    return tr


def commit_like(cm, table, hasher):
    """the model commitment of `table` with the shape of the model commitment `cm`"""
    mod = GM if cm.get("log_group", 0) else PM
    return mod.commit(cm["field"], table, cm["b"], cm["coset"], hasher)


def prove(cms, f, Q, a=1, tr=None, hasher=M.keccak256, cheat=False, commit=None):
    """-> the proof as a dict; `cms`: the model commitments of the six (tests/_fri_pcs_model.py, or _fri_ml_grouped_model.py's, all alike);
    `commit(table)`: the model commitment of a helper table with their shape (commit_like on the first by default); `tr` is advanced.  The
    statement is not checked."""
    field, d = cms[0]["field"], cms[0]["d"]
    assert len(cms) == GIVEN
    p, n = NM.MODULUS[field], 1 << d
    tr = M.Transcript() if tr is None else tr
    roots = [c["root"] for c in cms]
    beta, gamma = _statement(tr, roots, d, p)
    ws, ss = [list(c["coeffs"]) for c in cms[:3]], [list(c["coeffs"]) for c in cms[3:]]
    hs = [[0] * n for _ in range(WIRES)] if cheat else [fractions(ws[j], ss[j], j * n, beta, gamma, p) for j in range(WIRES)]
    commit = (lambda t: commit_like(cms[0], t, hasher)) if commit is None else commit
    hcms = [commit(h) for h in hs]
    h_roots = [c["root"] for c in hcms]
    alpha, mu, tau = _helpers(tr, h_roots, d, p)
    ch = (beta, gamma, alpha, mu)
    tabs, ids = ws + ss + hs + [ML.eq_table(tau, p)], id_tables(d)
    polys, rs = [], []
    for l in range(d):
        g = round_g5(tabs, ids, ch, p)
        if cheat and l == 0:
            g[1] = -g[0] % p
        polys.append(g)
        for e in g:
            tr.append(be32(e))
        r = tr.challenge(p)
        rs.append(r)
        tabs = [ML.mle_fold_last(field, t, r) for t in tabs]
        ids = [ML.mle_fold_last(field, t, r) for t in ids]
    z = rs[::-1]
    op = BM.open_batch(list(cms) + hcms, [z], f, Q, a, tr, hasher)
    assert [row[0] for row in op["ys"]] == [t[0] for t in tabs[:K]] and tabs[K][0] == eq_at(z, tau, p)
    assert [t[0] for t in ids] == [id_at(j, z, d, p) for j in range(WIRES)]
    return {"field": field, "d": d, "roots": roots, "h_roots": h_roots, "drawn": [beta, gamma, alpha, mu] + tau, "polys": polys, "challenges": rs, "opening": op,
            "nonce": getattr(tr, "nonce", None) or 0}


def verify(pr, roots=None, tr=None, hasher=M.keccak256):
    """`roots`: the verifier's own six, the proof's unless given -> (ok, the number of the first check that failed or None): 0 the first
    round's sum, l >= 1 round l's, d the last claim, d + 1 the opening"""
    field, d, op = pr["field"], pr["d"], pr["opening"]
    p = NM.MODULUS[field]
    tr = M.Transcript() if tr is None else tr
    roots = pr["roots"] if roots is None else roots
    beta, gamma = _statement(tr, roots, d, p)
    alpha, mu, tau = _helpers(tr, pr["h_roots"], d, p)
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
    want = summand(ys[0:3], ys[3:6], ys[6:9], [id_at(j, z, d, p) for j in range(WIRES)], eq_at(z, tau, p), (beta, gamma, alpha, mu)) % p
    if failed is None and cur != want:
        failed = d
    good = BM.verify(dict(op, own_roots=list(roots) + list(pr["h_roots"]), points=[z]), tr, hasher) and getattr(tr, "pow_ok", None) is not False
    if failed is None and not good:
        failed = d + 1
    return failed is None, failed


def sizes(d, b, f, Q, a=1, grouped=False):
    """(nround, nhroots) + the batch model's five counts at k = 9"""
    return (NODES * d, WIRES) + BM.sizes(K, d, b, f, Q, a, grouped)


def flat(zk, pr):
    """the proof as the C outputs: drawn (4 + d, 4), polys (d, 5, 4), challenges (d, 4), own_roots (6, 32), h_roots (3, 32), and the opening's
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
    fl["h_roots"] = np.frombuffer(b"".join(pr["h_roots"]), np.uint8).reshape(WIRES, 32).copy()
    fl.update(drawn=mont(pr["drawn"]), polys=mont([e for g in pr["polys"] for e in g]).reshape(d, NODES, 4), challenges=mont(pr["challenges"]))
    return fl
