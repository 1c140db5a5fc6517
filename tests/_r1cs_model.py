"""Python-integer model of the R1CS instance (include/zkmle.h "R1CS instance: sparse matrices times a table"): the digest, the products
A z, B z, C z and the rows bound at a point.  A matrix is a list of (row, col, value) with values in 0 .. p - 1; an instance is (s, d, [A, B, C]).
Nothing here shares code with the library."""
import random

import _ntt_model as NM
from oracle import pymodel as M

ROW_SPLIT = 32
RAW_TERMS_MAX = {0: 70, 3: 169}       # floor(2^261 / p): the most products one lazy reduction can take


def digest(field, s, d, mats):
    data = b"R1CSMAT" + field.to_bytes(4, "big") + s.to_bytes(4, "big") + d.to_bytes(4, "big")
    for m in mats:
        data += len(m).to_bytes(8, "big")
        for r, c, v in sorted(m):
            data += r.to_bytes(4, "big") + c.to_bytes(4, "big") + v.to_bytes(32, "big")
    return M.keccak256(data)


def matvec(field, s, mats, z):
    p = NM.MODULUS[field]
    out = []
    for m in mats:
        t = [0] * (1 << s)
        for r, c, v in m:
            t[r] = (t[r] + v * z[c]) % p
        out.append(t)
    return out


def eq_table(field, point):
    """eq(point, x) for x < 2^len(point), point[0] the most significant index bit"""
    p = NM.MODULUS[field]
    t = [1]
    for r in point:
        t = [w for e in t for w in (e * (1 - r) % p, e * r % p)]
    return t


def bind_rows(field, s, d, mats, rx, rho, full=False):
    p = NM.MODULUS[field]
    E = eq_table(field, rx)
    n = 1 << (d if full else d - 1)
    out = [0] * n
    for k, m in enumerate(mats):
        w = pow(rho, k, p)
        for r, c, v in m:
            if c < n:
                out[c] = (out[c] + w * v % p * E[r]) % p
    return out


def lengths(s, d, mats):
    """(rows above ROW_SPLIT among the 3 2^s, columns above it among the 2^d: a column's length is the three matrices' together)"""
    rows, cols = {}, {}
    for k, m in enumerate(mats):
        for r, c, _ in m:
            rows[(k, r)] = rows.get((k, r), 0) + 1
            cols[c] = cols.get(c, 0) + 1
    return sum(1 for n in rows.values() if n > ROW_SPLIT), sum(1 for n in cols.values() if n > ROW_SPLIT)


def random_matrix(field, s, d, per_row, seed, special=True):
    """per_row distinct columns in every row; values random, a few of them 0, 1 and p - 1 when `special`"""
    p = NM.MODULUS[field]
    rng = random.Random(seed)
    m = []
    for r in range(1 << s):
        for c in rng.sample(range(1 << d), per_row):
            v = rng.choice((0, 1, p - 1)) if special and rng.randrange(8) == 0 else rng.randrange(p)
            m.append((r, c, v))
    rng.shuffle(m)
    return m


def transpose(m):
    return [(c, r, v) for r, c, v in m]


# ---- the Spartan chain (include/zkmle.h "R1CS satisfiability: Spartan over a FRI commitment") ------------------------------------------------
import _fri_ml_model as ML  # noqa: E402
import _fri_ml_weighted_model as WM  # noqa: E402
import _zerocheck_family_model as ZF  # noqa: E402
import _zerocheck_model as ZM  # noqa: E402

be32 = ZF.be32


def xvec(field, d, public):
    """the public half of z: (1, pi_1 .. pi_l, 0, ..)"""
    half = 1 << (d - 1)
    assert len(public) < half
    return [1] + [v % NM.MODULUS[field] for v in public] + [0] * (half - 1 - len(public))


def satisfied_instance(field, s, d, npublic, seed, violate=None):
    """(mats, w, public) with (A z) o (B z) = C z for z = (w || 1, public, 0 ..): row r multiplies two random combinations of earlier witness
    entries, a public value or the constant; C's row has one entry, the next witness entry not yet defined, which takes the product's value
    (once the witness half is used up: the constant's column with the product as its value).  violate = r: the instance with C's entry in row
    r changed, which w no longer satisfies in that row"""
    p, rng = NM.MODULUS[field], random.Random(seed)
    half, rows = 1 << (d - 1), 1 << s
    public = [rng.randrange(p) for _ in range(npublic)]
    w, x = [rng.randrange(p) for _ in range(half)], xvec(field, d, public)
    free = max(2, half // 4)                                  # the entries below `free` are inputs; the rows define entries from `free` up
    A, B, Cm = [], [], []
    defined = free

    def combo(r, limit):
        cols = rng.sample(range(limit), min(2, limit)) + [half + rng.randrange(npublic + 1)]
        return [(r, c, rng.choice((1, p - 1, rng.randrange(p)))) for c in sorted(set(cols))]

    for r in range(rows):
        a, b = combo(r, defined), combo(r, defined)
        z = w + x
        va, vb = (sum(v * z[c] for _, c, v in m) % p for m in (a, b))
        if defined < half:                                    # C's row: the new witness entry, which takes the product's value
            w[defined] = va * vb % p
            c = [(r, defined, 1)]
            defined += 1
        else:                                                 # no entry left to define: C's row is the product as a multiple of the constant
            c = [(r, half, va * vb % p)]
        A += a
        B += b
        Cm += c
    if violate is not None:                                   # C's one entry in that row is one more: that row alone does not hold (unless its product is 0)
        r, c, v = Cm[violate]
        Cm[violate] = (r, c, (v + 1) % p)
    return [A, B, Cm], w, public


def is_satisfied(field, s, d, mats, w, public):
    p = NM.MODULUS[field]
    a, b, c = matvec(field, s, mats, w + xvec(field, d, public))
    return all(x * y % p == v for x, y, v in zip(a, b, c))


def public_terms(field, s, d, mats, public, rx, rho, rs):
    """(c_pub, w_final) as the verifier computes them; rs: the opening's R challenges"""
    p, half, R = NM.MODULUS[field], 1 << (d - 1), len(rs)
    E, x = eq_table(field, rx), xvec(field, d, public)
    P = eq_table(field, list(reversed(rs)))                  # bit l of the index <-> r_l, bit 0 the least significant
    c_pub, wf = 0, [0] * (half >> R)
    for k, m in enumerate(mats):
        wgt = pow(rho, k, p)
        for r, c, v in m:
            term = wgt * v % p * E[r] % p
            if c >= half:
                c_pub += term * x[c - half]
            else:
                wf[c >> R] = (wf[c >> R] + term * P[c & ((1 << R) - 1)]) % p
    return c_pub % p, wf


def _statement(tr, field, s, d, mats, root, public):
    p = NM.MODULUS[field]
    tr.append(b"R1CS" + s.to_bytes(4, "big") + d.to_bytes(4, "big") + len(public).to_bytes(4, "big"))
    tr.append(digest(field, s, d, mats))
    tr.append(root)
    for v in public:
        tr.append(be32(v % p))
    return [tr.challenge(p) for _ in range(s)]


def prove(field, s, d, mats, cmW, public, f, Q, a=1, tr=None, hasher=M.keccak256, grind=None):
    """-> the proof as a dict; cmW: the model commitment of w (d - 1 variables).  The relation is not checked."""
    p = NM.MODULUS[field]
    assert cmW["d"] == d - 1 and cmW["field"] == field
    tr = M.Transcript() if tr is None else tr
    tau = _statement(tr, field, s, d, mats, cmW["root"], public)
    z = list(cmW["coeffs"]) + xvec(field, d, public)
    tabs = matvec(field, s, mats, z) + [eq_table(field, tau)]
    polys, rs = [], []
    for _ in range(s):
        g = ZM.round_g4(*tabs, p)
        polys.append(g)
        for e in g:
            tr.append(be32(e))
        r = tr.challenge(p)
        rs.append(r)
        tabs = [ML.mle_fold_last(field, t, r) for t in tabs]
    rx = list(reversed(rs))
    vs = [t[0] for t in tabs[:3]]
    for v in vs:
        tr.append(be32(v))
    rho = tr.challenge(p)
    Mw = bind_rows(field, s, d, mats, rx, rho)
    op = WM.open_weighted(cmW, Mw, f, Q, a, tr, hasher, grind)
    return {"field": field, "s": s, "d": d, "public": list(public), "tau": tau, "polys": polys, "challenges": rs, "vs": vs, "rho": rho, "opening": op}


def verify(pr, mats, root, public, tr=None, hasher=M.keccak256, grind_check=None):
    field, s, d, op = pr["field"], pr["s"], pr["d"], pr["opening"]
    p = NM.MODULUS[field]
    tr = M.Transcript() if tr is None else tr
    tau = _statement(tr, field, s, d, mats, root, public)
    ok, claim, rs = all(0 <= v < p for v in list(public) + list(pr["vs"]) + [e for g in pr["polys"] for e in g]), 0, []
    for g in pr["polys"]:
        for e in g:
            tr.append(be32(e % p))
        ok = ok and (g[0] + g[1]) % p == claim
        rs.append(tr.challenge(p))
        claim = ZF.interpolate(g, rs[-1], p)
    rx = list(reversed(rs))
    va, vb, vc = pr["vs"]
    ok = ok and claim == ZF.eq_at(rx, tau, p) * (va * vb - vc) % p
    for v in pr["vs"]:
        tr.append(be32(v % p))
    rho = tr.challenge(p)
    c_pub, wf = public_terms(field, s, d, mats, public, rx, rho, op["challenges"])
    ok = ok and op["c"] == (va + rho * vb + rho * rho * vc - c_pub) % p
    opened = WM.verify_weighted(dict(op, root=root, w_final=wf), tr, hasher, grind_check)
    return bool(ok and opened)


def flat(zk, pr):
    """the proof in the C ABI's layout: polys (s, 4, 4), vs (3, 4), tau, challenges (s, 4), rho (4,), and `opening` = _fri_ml_weighted_model.flat"""
    f = pr["field"]
    return {"polys": zk.from_ints(f, [e for g in pr["polys"] for e in g]).reshape(pr["s"], 4, 4), "vs": zk.from_ints(f, pr["vs"]), "tau": zk.from_ints(f, pr["tau"]),
            "challenges": zk.from_ints(f, pr["challenges"]), "rho": zk.from_ints(f, [pr["rho"]])[0], "opening": WM.flat(zk, pr["opening"])}
