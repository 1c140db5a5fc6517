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
import random

import numpy as np

import _fri_ml_model as ML
import _fri_ml_wide_model as WB
import _lookup_model as LM
import _ntt_model as NM
import _plonk_model as PM
import _wiring_model as WM
from oracle import pymodel as M

be32 = ML.be32
WIRES, GIVEN, HELPERS, K, NODES, TABLES = 3, 15, 5, 20, 5, 21
PLONK_PLACES = tuple(range(11)) + (16, 17, 18, 20)           # the plonk proof's fifteen (.., H0, H1, H2, E) among the twenty-one
LOOKUP_PLACES = (0, 1, 2, 11, 12, 13, 14, 15, 19)            # the lookup's nine (A, B, C, qK, T0, T1, T2, M, H) among them
E_PLACE = 20
interpolate5, eq_at, id_at, commit_like = WM.interpolate5, WM.eq_at, WM.id_at, WM.commit_like
pow_transcript = WM.pow_transcript                           # 4 + 2 d + 1 + R samples stand before the first index, as in the plonk proof
pi_table, public_eval, mont = PM.pi_table, PM.public_eval, PM.mont


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


def _statement(tr, roots, d, pub, p):
    tr.append(tag(d, len(pub)))
    for r in roots:
        tr.append(r)
    for v in pub:
        tr.append(be32(v % p))


def _helpers(tr, h_roots, d, p):
    """the five helper roots and what is drawn behind them -> beta, gamma, alpha, mu, tau"""
    tr.append(h_roots[0])
    beta, gamma = tr.challenge(p), tr.challenge(p)
    for r in h_roots[1:]:
        tr.append(r)
    alpha, mu = tr.challenge(p), tr.challenge(p)
    return beta, gamma, alpha, mu, [tr.challenge(p) for _ in range(d)]


def helper_tables(given, beta, gamma, p, m=None):
    """-> [M, H0, H1, H2, HL] from the fifteen integer tables (m: a multiplicity table to use in M's place)"""
    n = len(given[0])
    lk = lookup_tables(given)
    m = LM.multiplicities(lk, p)[0] if m is None else m
    hs = [WM.fractions(given[j], given[8 + j], j * n, beta, gamma, p) for j in range(WIRES)]
    return [m] + hs + [LM.fractions(lk + [m], beta, gamma, p)]


def prove(cms, pub, f, Q, a=1, tr=None, hasher=M.keccak256, cheat=None):
    """-> the proof as a dict; `cms`: the model commitments of the fifteen (all alike); `pub`: the public values; `tr` is advanced.  The
    statement is not checked."""
    field, d = cms[0]["field"], cms[0]["d"]
    assert len(cms) == GIVEN and len(pub) <= 1 << d and cheat in (None, "wiring", "lookup")
    p, n = NM.MODULUS[field], 1 << d
    tr = M.Transcript() if tr is None else tr
    roots = [c["root"] for c in cms]
    _statement(tr, roots, d, pub, p)
    given = [list(c["coeffs"]) for c in cms]
    m, misses = LM.multiplicities(lookup_tables(given), p)
    if cheat == "lookup":
        m[0] = (m[0] + misses) % p
    mcm = commit_like(cms[0], m, hasher)
    tr.append(mcm["root"])
    beta, gamma = tr.challenge(p), tr.challenge(p)
    helpers = helper_tables(given, beta, gamma, p, m)
    if cheat == "wiring":
        helpers[1:4] = [[0] * n for _ in range(WIRES)]
    hcms = [mcm] + [commit_like(cms[0], h, hasher) for h in helpers[1:]]
    h_roots = [c["root"] for c in hcms]
    for r in h_roots[1:]:
        tr.append(r)
    alpha, mu = tr.challenge(p), tr.challenge(p)
    tau = [tr.challenge(p) for _ in range(d)]
    ch = (beta, gamma, alpha, mu)
    tabs, ids, pi = given + helpers + [ML.eq_table(tau, p)], WM.id_tables(d), pi_table(pub, d)
    claimed = alpha ** 3 * sum(a_ * b_ for a_, b_ in zip(pi, tabs[E_PLACE])) % p
    assert claimed == alpha ** 3 * public_eval(pub, tau, p) % p
    polys, rs, own_sums = [], [], []
    for l in range(d):
        g, own = round_g5(tabs, ids, ch, p, pi)
        own_sums.append((own[0] + own[1]) % p)
        if cheat and l == 0:
            g[1] = (claimed - g[0]) % p
        polys.append(g)
        for e in g:
            tr.append(be32(e))
        r = tr.challenge(p)
        rs.append(r)
        tabs = [ML.mle_fold_last(field, t, r) for t in tabs]
        ids = [ML.mle_fold_last(field, t, r) for t in ids]
        pi = ML.mle_fold_last(field, pi, r)
    z = rs[::-1]
    op = WB.open_batch(list(cms) + hcms, [z], f, Q, a, tr, hasher)
    assert [row[0] for row in op["ys"]] == [t[0] for t in tabs[:K]] and tabs[K][0] == eq_at(z, tau, p)
    return {"field": field, "d": d, "roots": roots, "pub": list(pub), "h_roots": h_roots, "drawn": [beta, gamma, alpha, mu] + tau, "polys": polys, "challenges": rs,
            "opening": op, "misses": misses, "nonce": getattr(tr, "nonce", None) or 0, "own_first_sum": own_sums[0] if own_sums else 0}


def verify(pr, roots=None, pub=None, tr=None, hasher=M.keccak256):
    """`roots`, `pub`: the verifier's own fifteen and its public values, the proof's unless given -> (ok, the number of the first check that
    failed or None): 0 the first round's sum (or a public value outside the field), l >= 1 round l's, d the last claim, d + 1 the opening"""
    field, d, op = pr["field"], pr["d"], pr["opening"]
    p = NM.MODULUS[field]
    tr = M.Transcript() if tr is None else tr
    roots = pr["roots"] if roots is None else roots
    pub = pr["pub"] if pub is None else pub
    _statement(tr, roots, d, pub, p)
    beta, gamma, alpha, mu, tau = _helpers(tr, pr["h_roots"], d, p)
    failed = 0 if any(not 0 <= v < p for v in pub) or len(pub) > 1 << d else None
    cur = alpha ** 3 * sum(a * b for a, b in zip(pi_table(pub, d), ML.eq_table(tau, p))) % p if len(pub) <= 1 << d else 0
    rs = []
    for l in range(d):
        g = pr["polys"][l]
        for e in g:
            tr.append(be32(e % p))
        if failed is None and (any(not 0 <= e < p for e in g) or (g[0] + g[1] - cur) % p != 0):
            failed = l
        rs.append(tr.challenge(p))
        cur = interpolate5(g, rs[l], p)
    z = rs[::-1]
    ys = [row[0] for row in op["ys"]]
    want = summand(ys + [eq_at(z, tau, p)], [id_at(j, z, d, p) for j in range(WIRES)], (beta, gamma, alpha, mu)) % p
    if failed is None and cur != want:
        failed = d
    good = WB.verify(dict(op, own_roots=list(roots) + list(pr["h_roots"]), points=[z]), tr, hasher)
    if failed is None and not good:
        failed = d + 1
    return failed is None, failed


def sizes(d, b, f, Q, a=1, grouped=False):
    """(nround, nhroots) + the batch model's five counts at k = 20"""
    return (NODES * d, HELPERS) + WB.sizes(K, d, b, f, Q, a, grouped)


def flat(zk, pr):
    """the proof as the C outputs: drawn (4 + d, 4), polys (d, 5, 4), challenges (d, 4), own_roots (15, 32), h_roots (5, 32), pub (l, 4), and the
    opening's arrays of _fri_ml_batch_model.flat under their names there with ys as (20, 4) and the opening's round polynomials as open_polys /
    open_challenges"""
    field, d = pr["field"], pr["d"]
    fl = WB.flat(zk, pr["opening"])
    fl["open_polys"], fl["open_challenges"] = fl.pop("polys"), fl.pop("challenges")
    fl["ys"] = fl["ys"].reshape(K, 4)
    fl["own_roots"] = np.frombuffer(b"".join(pr["roots"]), np.uint8).reshape(GIVEN, 32).copy()
    fl["h_roots"] = np.frombuffer(b"".join(pr["h_roots"]), np.uint8).reshape(HELPERS, 32).copy()
    fl.update(drawn=mont(zk, field, pr["drawn"]), polys=mont(zk, field, [e for g in pr["polys"] for e in g]).reshape(d, NODES, 4),
              challenges=mont(zk, field, pr["challenges"]), pub=mont(zk, field, pr["pub"]))
    return fl
