"""Python model of the Plonk proof with lookup rows on COLUMN commitments (helper of tests/test_plonk_lookup_columns_cpu.py,
test_gpu_plonk_lookup_helpers.py and test_gpu_plonk_lookup_columns.py).  The definition is the one of
include/zkmle.h "Plonk with lookups on column commitments".  Built by import on _plonk_lookup_model (the circuits, round_g5, the relation's
summand) and on _fri_ml_columns_model (commit, open_columns, verify); the helper tables are its own, in the single-denominator form:

  commitments  witness = _fri_ml_columns_model.commit of (A, B, C); circuit = that of (qM, qL, qR, qO, qC, SA, SB, SC, qK, T0, T1, T2)
  statement    "ZCLC" be32(d) be32(l) in one append, the witness root, the circuit root, the l public values as 32-byte big-endian elements
  M            _lookup_model.multiplicities; committed as ONE column; its root appended; then beta, gamma
  helpers      H_j[x] = (Dsig_j - Did_j) inv0(Did_j Dsig_j),  HL[x] = (qK Dt - M Dw) inv0(Dw Dt), inv0(0) = 0; committed as ONE commitment of four
               columns; its root appended; then alpha, mu, tau_0 .. tau_{d-1}
  the sum      _plonk_lookup_model's, unchanged: round_g5 on the twenty-one tables with the explicit id and PI tables
  opening      _fri_ml_columns_model.open_columns of the four commitments (widths 3, 12, 1, 4) at z, z[d - 1 - l] = r_l, on the same transcript
  verifier     _plonk_lookup_model's checks on the twenty claims as they stand, then the columns opening's verifier with the roots witness,
               circuit, M, helpers

`prove(.., cheat=..)` has _plonk_lookup_model's two cheating provers.  Everything is Python integers; nothing here knows how the library works."""
import numpy as np

import _fri_ml_columns_model as CM
import _fri_ml_model as ML
import _lookup_model as LM
import _ntt_model as NM
import _plonk_lookup_model as KL
import _wiring_model as WM
from oracle import pymodel as M

be32 = ML.be32
WIRES, GIVEN, K, NODES = KL.WIRES, KL.GIVEN, KL.K, KL.NODES
WIDTHS = (3, 12, 1, 4)
circuit, satisfied, pow_transcript, mont, interpolate5 = KL.circuit, KL.satisfied, KL.pow_transcript, KL.mont, KL.interpolate5
inv0 = WM.inv0


def tag(d, l):
    return b"ZCLC" + int(d).to_bytes(4, "big") + int(l).to_bytes(4, "big")


def helper_inputs(given, m):
    """A, B, C, SA, SB, SC, qK, T0, T1, T2, M of the fifteen and M: what the helper kernel reads"""
    return [given[j] for j in (0, 1, 2, 8, 9, 10, 11, 12, 13, 14)] + [m]


def helpers_of(tabs, beta, gamma, p):
    """-> [H0, H1, H2, HL] from the eleven integer tables A, B, C, SA, SB, SC, qK, T0, T1, T2, M: ONE inverse per entry, of the product of its
    two denominators"""
    n = len(tabs[0])
    hs = []
    for j in range(WIRES):
        col = []
        for x in range(n):
            did, dsig = beta + tabs[j][x] + gamma * (j * n + x), beta + tabs[j][x] + gamma * tabs[3 + j][x]
            col.append((dsig - did) * inv0(did * dsig, p) % p)
        hs.append(col)
    A, B, C, qK, T0, T1, T2, m = tabs[0], tabs[1], tabs[2], tabs[6], tabs[7], tabs[8], tabs[9], tabs[10]
    hl = []
    for x in range(n):
        dw, dt = beta + A[x] + gamma * B[x] + gamma * gamma * C[x], beta + T0[x] + gamma * T1[x] + gamma * gamma * T2[x]
        hl.append((qK[x] * dt - m[x] * dw) * inv0(dw * dt, p) % p)
    return hs + [hl]


def helper_tables(given, beta, gamma, p, m=None):
    """-> [M, H0, H1, H2, HL] from the fifteen integer tables (m: a multiplicity table to use in M's place): _plonk_lookup_model.helper_tables
    with the single-denominator definition"""
    m = LM.multiplicities(KL.lookup_tables(given), p)[0] if m is None else m
    return [m] + helpers_of(helper_inputs(given, m), beta, gamma, p)


def commitments(field, tabs, b, coset=1, hasher=M.keccak256):
    """-> (witness, circuit): the two model column commitments of the fifteen tables"""
    return CM.commit(field, tabs[:3], b, coset, hasher), CM.commit(field, tabs[3:], b, coset, hasher)


def _statement(tr, roots, d, pub, p):
    tr.append(tag(d, len(pub)))
    for r in roots:
        tr.append(r)
    for v in pub:
        tr.append(be32(v % p))


def prove(wit, cir, pub, f, Q, tr=None, hasher=M.keccak256, cheat=None):
    """-> the proof as a dict; wit, cir: the model column commitments; pub: the public values; `tr` is advanced.  The statement is not checked."""
    field, d, b, coset = (wit[n] for n in ("field", "d", "b", "coset"))
    assert wit["k"] == 3 and cir["k"] == 12 and all(cir[n] == wit[n] for n in ("field", "d", "b", "coset"))
    assert len(pub) <= 1 << d and cheat in (None, "wiring", "lookup")
    p, n = NM.MODULUS[field], 1 << d
    tr = M.Transcript() if tr is None else tr
    roots = [wit["root"], cir["root"]]
    _statement(tr, roots, d, pub, p)
    given = [list(t) for t in wit["coeffs"]] + [list(t) for t in cir["coeffs"]]
    m, misses = LM.multiplicities(KL.lookup_tables(given), p)
    if cheat == "lookup":
        m[0] = (m[0] + misses) % p
    mcm = CM.commit(field, [m], b, coset, hasher)
    tr.append(mcm["root"])
    beta, gamma = tr.challenge(p), tr.challenge(p)
    helpers = helper_tables(given, beta, gamma, p, m)
    if cheat == "wiring":
        helpers[1:4] = [[0] * n for _ in range(WIRES)]
    hcm = CM.commit(field, helpers[1:], b, coset, hasher)
    h_roots = [mcm["root"], hcm["root"]]
    tr.append(hcm["root"])
    alpha, mu = tr.challenge(p), tr.challenge(p)
    tau = [tr.challenge(p) for _ in range(d)]
    ch = (beta, gamma, alpha, mu)
    tabs, ids, pi = given + helpers + [ML.eq_table(tau, p)], WM.id_tables(d), KL.pi_table(pub, d)
    claimed = alpha ** 3 * KL.public_eval(pub, tau, p) % p
    polys, rs, own_sums = [], [], []
    for l in range(d):
        g, own = KL.round_g5(tabs, ids, ch, p, pi)
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
    op = CM.open_columns([wit, cir, mcm, hcm], [z], f, Q, tr, hasher)
    assert [row[0] for row in op["ys"]] == [t[0] for t in tabs[:K]] and op["widths"] == list(WIDTHS)
    return {"field": field, "d": d, "roots": roots, "pub": list(pub), "h_roots": h_roots, "drawn": [beta, gamma, alpha, mu] + tau, "polys": polys, "challenges": rs,
            "opening": op, "misses": misses, "nonce": getattr(tr, "nonce", None) or 0, "own_first_sum": own_sums[0] if own_sums else 0, "helpers": helpers}


def verify(pr, roots=None, pub=None, tr=None, hasher=M.keccak256):
    """`roots`, `pub`: the verifier's own two roots and its public values, the proof's unless given -> (ok, the number of the first check that
    failed or None): 0 the first round's sum (or a public value outside the field), l >= 1 round l's, d the last claim, d + 1 the opening"""
    field, d, op = pr["field"], pr["d"], pr["opening"]
    p = NM.MODULUS[field]
    tr = M.Transcript() if tr is None else tr
    roots = pr["roots"] if roots is None else roots
    pub = pr["pub"] if pub is None else pub
    _statement(tr, roots, d, pub, p)
    tr.append(pr["h_roots"][0])
    beta, gamma = tr.challenge(p), tr.challenge(p)
    tr.append(pr["h_roots"][1])
    alpha, mu = tr.challenge(p), tr.challenge(p)
    tau = [tr.challenge(p) for _ in range(d)]
    failed = 0 if any(not 0 <= v < p for v in pub) or len(pub) > 1 << d else None
    cur = alpha ** 3 * sum(a * b for a, b in zip(KL.pi_table(pub, d), ML.eq_table(tau, p))) % p if len(pub) <= 1 << d else 0
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
    want = KL.summand(ys + [KL.eq_at(z, tau, p)], [KL.id_at(j, z, d, p) for j in range(WIRES)], (beta, gamma, alpha, mu)) % p
    if failed is None and cur != want:
        failed = d
    good = CM.verify(dict(op, own_roots=list(roots) + list(pr["h_roots"]), widths=list(WIDTHS), points=[z]), tr, hasher)
    if failed is None and not good:
        failed = d + 1
    return failed is None, failed


def sizes(d, b, f, Q):
    """(nround, nhroots) + the columns model's five counts for the widths 3, 12, 1, 4"""
    return (NODES * d, 2) + CM.sizes(list(WIDTHS), d, b, f, Q)


def flat(zk, pr):
    """the proof as the C outputs: drawn (4 + d, 4), polys (d, 5, 4), challenges (d, 4), own_roots (2, 32), h_roots (2, 32), pub (l, 4), and the
    opening's arrays of _fri_ml_columns_model.flat under their names there with ys as (20, 4) and the opening's round polynomials as open_polys /
    open_challenges"""
    field, d = pr["field"], pr["d"]
    fl = CM.flat(zk, pr["opening"])
    fl["open_polys"], fl["open_challenges"] = fl.pop("polys"), fl.pop("challenges")
    fl["ys"] = fl["ys"].reshape(K, 4)
    fl["own_roots"] = np.frombuffer(b"".join(pr["roots"]), np.uint8).reshape(2, 32).copy()
    fl["h_roots"] = np.frombuffer(b"".join(pr["h_roots"]), np.uint8).reshape(2, 32).copy()
    fl.update(drawn=mont(zk, field, pr["drawn"]), polys=mont(zk, field, [e for g in pr["polys"] for e in g]).reshape(d, NODES, 4),
              challenges=mont(zk, field, pr["challenges"]), pub=mont(zk, field, pr["pub"]))
    return fl
