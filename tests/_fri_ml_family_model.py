"""Python model of the FAMILY of multilinear openings of FRI commitments at several points: the prover loop, the verifier, `sizes` and `flat`
once, for the protocols of include/zkmle.h "FRI commitment opened at several points", ".. with a fold arity", ".. with grouped leaves" and
"FRI commitments opened together".  tests/_fri_ml_{points,arity,grouped,batch}_model.py bind their public names to it; it is built on
tests/_fri_ml_model.py, _fri_model.py and _merkle_model.py alone, so the helpers those four share (weights, round_g3, fold2, steps, the
grouped leaves) live here and are re-exported there.  A protocol is a Proto; the protocols differ in three places only:

  statement    FRI's header, the Proto's tag (and k, for a batch), the k roots, P, the points, the k P claims table-major, ONE gamma
                 several points  no tag        arity 2  be32(2)        grouped leaves  be32(2) be32(1)        batch  "BTCH" a grouped, then k
  schedule     steps(L, R, a): log_arity 1 folds by 2 and commits every layer; 2 folds by 4 from every even l (by 2 to the final layer when R
               is odd) and commits the even layers.  Ungrouped, a step's answer has one path per side; grouped, the layer is hashed with its
               leaves grouped by the step's sides and the answer has ONE path of L - l - log_sides digests
  step 0       alpha = gamma^P;  claim_0 = sum_j alpha^j sum_p gamma^p y_{j,p};  T = sum_j alpha^j T_j;  f_0 = sum_j alpha^j f_j;  per query
               every commitment's own values and path(s).  One table is k = 1

  weights      W_0[x] = sum_p gamma^p eq(x, z^p);  W_{l+1} = mle_fold_last(W_l, r_l), as T_{l+1} from T_l
  round l      g_l(X) = sum_x' (W_l[2x'] + X (W_l[2x'+1] - W_l[2x'])) (T_l[2x'] + X (T_l[2x'+1] - T_l[2x'])), sent at X = 0, 1, 2; then r_l, and
               the root of layer l + 1 if a step starts there
  fold by 4    u0 = fold2(f[k], f[k + N_l/2]; r_l, x), u1 = fold2(f[k + N_l/4], f[k + 3 N_l/4]; r_l, i x), f_{l+2}[k] = fold2(u0, u1; r_{l+1}, x^2)
               with fold2(a, b; r, x) = (1 - r)(a + b) / 2 + r (a - b) / (2 x), x = c_l w_l^k, i = w_l^(N_l / 4)
  verifier     the sumcheck's checks; sum_j T_R[j] W_R[j] = the last claim with W_R from the points alone; per query and step the paths, and
               the step's fold formula against the next step's value (or T_R read as coefficients)

The prover builds EVERY layer with the two-point fold of _fri_ml_model.py; the verifier combines the opened layer-0 values and uses the step
formulas, so an opening that passes ties the two together.  `open_family(.., false_y=(p, v))` opens with table 0's claim p replaced by v:
round 0's polynomial is shifted so that g_0(0) + g_0(1) equals the false claim_0 and everything else is run honestly.  Everything is Python
integers; nothing here knows how the library works."""
import collections

import numpy as np

import _fri_ml_model as ML
import _fri_model as FM
import _merkle_model as MM
import _ntt_model as NM
from oracle import pymodel as M

be32 = FM.be32
be4 = lambda v: int(v).to_bytes(4, "big")
KMAX = 16

# tag: what the statement absorbs behind the header; batch: k and k roots follow, the dict has own_roots / a / grouped / k and ys as rows
Proto = collections.namedtuple("Proto", "tag log_arity grouped batch")
POINTS, ARITY, GROUPED = Proto(b"", 1, False, False), Proto(be4(2), 2, False, False), Proto(be4(2) + be4(1), 2, True, False)


def batch(a, grouped):
    return Proto(b"BTCH" + be4(a) + be4(bool(grouped)), a, bool(grouped), True)


# ---- the pieces --------------------------------------------------------------------------------------------------------------------------
def weights(points, gamma, p):
    """W_0: the gamma-combination of the points' eq tables"""
    n = 1 << len(points[0])
    out, gp = [0] * n, 1
    for z in points:
        out = [(o + gp * e) % p for o, e in zip(out, ML.eq_table(z, p))]
        gp = gp * gamma % p
    return out


def round_g3(T, W, p):
    """g(0), g(1), g(2) of the product of the two tables' last-variable lines"""
    g = [0, 0, 0]
    for x in range(len(T) // 2):
        t0, t1, w0, w1 = T[2 * x], T[2 * x + 1], W[2 * x], W[2 * x + 1]
        for X in (0, 1, 2):
            g[X] += (w0 + X * (w1 - w0)) * (t0 + X * (t1 - t0))
    return [v % p for v in g]


def fold2(a, b, r, x, p):
    return ((1 - r) * (a + b) * pow(2, p - 2, p) + r * (a - b) * pow(2 * x, -1, p)) % p


def steps(L, R, a):
    """[(l, sides)] of the steps of an opening with R rounds at log_arity a"""
    return [(l, 2) for l in range(R)] if a == 1 else [(l, 4 if l + 2 <= R else 2) for l in range(0, R, 2)]


def leaf_bytes(values, log_group):
    """the messages of the grouped leaves (without the tag) of a table of canonical ints"""
    part = len(values) >> log_group
    assert part >= 1 and part << log_group == len(values)
    return [b"".join(be32(values[j + s * part]) for s in range(1 << log_group)) for j in range(part)]


def levels_of(values, log_group, hasher=M.keccak256):
    return MM.levels_of(leaf_bytes(values, log_group), hasher)


def verify_leaf(root, index, group, path, hasher=M.keccak256):
    """group: the leaf's 2^log_group canonical ints in the leaf's order"""
    return MM.verify_path(root, index, b"".join(be32(v) for v in group), path, hasher)


def _path_len(L, l, sides, grouped):
    return L - l - (sides.bit_length() - 1) if grouped else L - l


def sizes(k, d, b, f, Q, a=1, grouped=False):
    """(nroots, nfinal, nvalues, path_bytes, nround) by the header's formulas"""
    L, R = d + b, d - f
    st = steps(L, R, a)
    per_path = lambda l, s: _path_len(L, l, s, grouped) * (1 if grouped else s)
    values = sum(s for _, s in st) + (k - 1) * st[0][1]
    digests = sum(per_path(l, s) for l, s in st) + (k - 1) * per_path(*st[0])
    return k + len(st) - 1, 1 << f, Q * values, 32 * Q * digests, 3 * R


def _statement(tr, proto, field, d, b, f, Q, coset, own_roots, points, ys):
    """absorbs the statement (ys: one row of claims per commitment) -> gamma"""
    p = NM.MODULUS[field]
    tr.append(FM.header(d, b, f, Q, coset))
    tr.append(proto.tag + (be4(len(own_roots)) if proto.batch else b""))
    for r in own_roots:
        tr.append(r)
    tr.append(be4(len(points)))
    for z in points:
        for v in z:
            tr.append(be32(v % p))
    for row in ys:
        for y in row:
            tr.append(be32(y % p))
    return tr.challenge(p)


def _index_mod(N, a):
    return N if a == 1 else N // 2                           # FM.sample_index(tr, n) takes the sample mod n / 2


def _own(op, proto):
    """(the commitments' roots, the claims as rows) of an opening's dict"""
    return (op["own_roots"], op["ys"]) if proto.batch else ([op["root"]], [op["ys"]])


# ---- the prover --------------------------------------------------------------------------------------------------------------------------
def open_family(proto, cms, points, f, Q, tr=None, hasher=M.keccak256, false_y=None):
    """-> the opening as a dict; `cms`: k commitments of tests/_fri_pcs_model.py (ungrouped) or of _fri_ml_grouped_model.py (all grouped), one
    unless proto.batch; points a list of P lists of d ints; `tr` is advanced"""
    c0, k, P = cms[0], len(cms), len(points)
    field, d, b, coset = (c0[n] for n in ("field", "d", "b", "coset"))
    a, grouped = proto.log_arity, proto.grouped
    assert all(c["field"] == field and c["d"] == d and c["b"] == b and c["coset"] == coset and (c.get("log_group", 0) == 2) == grouped for c in cms)
    p, L, R = NM.MODULUS[field], d + b, d - f
    N = 1 << L
    assert 1 <= k <= (KMAX if proto.batch else 1) and 1 <= P <= 8 and all(len(z) == d and all(0 <= v < p for v in z) for z in points)
    assert 0 <= f < d and 1 <= Q <= 4096 and a in (1, 2) and (a == 2 or not grouped) and (a == 1 or R >= 2)
    tr = M.Transcript() if tr is None else tr
    ys = [[ML.mle_evaluate(field, c["coeffs"], z) for z in points] for c in cms]
    claimed = [list(row) for row in ys]
    if false_y is not None:
        claimed[0][false_y[0]] = false_y[1] % p
    own = [c["root"] for c in cms]
    gamma = _statement(tr, proto, field, d, b, f, Q, coset, own, points, claimed)
    alpha = pow(gamma, P, p)
    shift = sum(pow(gamma, j * P + q, p) * (claimed[j][q] - ys[j][q]) for j in range(k) for q in range(P)) % p
    T = [sum(pow(alpha, j, p) * c["coeffs"][x] for j, c in enumerate(cms)) % p for x in range(1 << d)]
    W = weights(points, gamma, p)
    st = steps(L, R, a)
    sides_at = dict(st)
    layers, trees, roots = {0: [sum(pow(alpha, j, p) * c["codeword"][x] for j, c in enumerate(cms)) % p for x in range(N)]}, {}, list(own)
    polys, rs, c = [], [], coset % p
    for l in range(R):
        g = round_g3(T, W, p)
        if l == 0:
            g[0] = (g[0] + shift) % p                        # a false claim needs a round 0 that sums to it
        polys.append(g)
        for e in g:
            tr.append(be32(e))
        r = tr.challenge(p)
        rs.append(r)
        T, W = ML.mle_fold_last(field, T, r), ML.mle_fold_last(field, W, r)
        layers[l + 1] = ML.fold(field, layers[l], r, c)
        c = c * c % p
        if l + 1 < R and l + 1 in sides_at:
            lg = sides_at[l + 1].bit_length() - 1
            trees[l + 1] = levels_of(layers[l + 1], lg, hasher) if grouped else MM.levels_of([be32(e) for e in layers[l + 1]], hasher)
            roots.append(trees[l + 1][-1][0])
            tr.append(roots[-1])
    final = T
    for e in final:
        tr.append(be32(e))
    indices = [FM.sample_index(tr, _index_mod(N, a)) for _ in range(Q)]
    values, paths = [], []                                   # per query: step 0 once per commitment, then the later steps
    for i in indices:
        for l, sides in st:
            part = (N >> l) // sides
            j = i % part
            sources = [(cm["codeword"], cm["levels"]) for cm in cms] if l == 0 else [(layers[l], trees[l])]
            for table, tree in sources:
                values.append([table[j + s * part] for s in range(sides)])
                paths.append([MM.path_of(tree, j)] if grouped else [MM.path_of(tree, j + s * part) for s in range(sides)])
    op = {"field": field, "d": d, "b": b, "f": f, "Q": Q, "coset": coset % p}
    op.update({"a": a, "grouped": grouped, "k": k, "own_roots": own, "ys": claimed} if proto.batch else {"root": own[0], "ys": claimed[0]})
    op.update({"points": [list(z) for z in points], "gamma": gamma, "polys": polys, "roots": roots, "final": final, "challenges": rs,
               "indices": indices, "values": values, "paths": paths})
    return op


# ---- the verifier ------------------------------------------------------------------------------------------------------------------------
def verify_family(proto, op, tr=None, hasher=M.keccak256):
    field, d, b, f, Q, coset, points = (op[n] for n in ("field", "d", "b", "f", "Q", "coset", "points"))
    a, grouped = proto.log_arity, proto.grouped
    own, ys = _own(op, proto)
    k = op["k"] if proto.batch else 1
    p, L, R = NM.MODULUS[field], d + b, d - f
    N, P = 1 << L, len(points)
    w = NM.root_of_unity(field, L)
    tr = M.Transcript() if tr is None else tr
    if not 1 <= k <= KMAX or len(own) != k or len(ys) != k or any(len(row) != P for row in ys) or not 1 <= P <= 8:
        return False
    if a not in (1, 2) or (grouped and a != 2) or (a == 2 and R < 2):
        return False
    st = steps(L, R, a)
    gamma = _statement(tr, proto, field, d, b, f, Q, coset, own, points, ys)
    later = {l: k + s - 1 for s, (l, _) in enumerate(st) if s}       # the root of layer l in op["roots"]
    rs = []
    for l in range(R):
        for e in op["polys"][l]:
            tr.append(be32(e % p))
        rs.append(tr.challenge(p))
        if l + 1 < R and l + 1 in later:
            tr.append(op["roots"][later[l + 1]])
    for e in op["final"]:
        tr.append(be32(e % p))
    indices = [FM.sample_index(tr, _index_mod(N, a)) for _ in range(Q)]
    every = ([v for z in points for v in z] + [y for row in ys for y in row] + [e for g in op["polys"] for e in g] + list(op["final"])
             + [v for vs in op["values"] for v in vs])
    if any(not 0 <= v < p for v in every) or list(op["roots"][:k]) != list(own) or len(op["roots"]) != k + len(st) - 1:
        return False
    alpha = pow(gamma, P, p)
    claim = sum(pow(gamma, j * P + q, p) * ys[j][q] for j in range(k) for q in range(P)) % p
    for l in range(R):
        g = op["polys"][l]
        if (g[0] + g[1]) % p != claim:
            return False
        claim = ML.interpolate3(g, rs[l], p)
    end = 0
    for q, z in enumerate(points):                           # W_R[j] = sum_p gamma^p A^p_R eq(j; z^p_0 .. z^p_{f-1})
        A = pow(gamma, q, p)
        for l in range(R):
            A = A * ML.eq1(rs[l], z[d - 1 - l], p) % p
        end += A * sum(t * e for t, e in zip(op["final"], ML.eq_table(z[:f], p)))
    if end % p != claim:
        return False
    iota = pow(w, N // 4, p)
    per = k + len(st) - 1                                     # answers of one query
    if len(op["values"]) != Q * per or len(op["paths"]) != Q * per:
        return False

    def opened(root, l, sides, j, vals, pths):
        part = (N >> l) // sides
        if len(vals) != sides or len(pths) != (1 if grouped else sides) or any(len(pt) != _path_len(L, l, sides, grouped) for pt in pths):
            return False
        if grouped:
            return verify_leaf(root, j, vals, pths[0], hasher)
        return all(MM.verify_path(root, j + s * part, be32(vals[s]), pths[s], hasher) for s in range(sides))

    for q, i in enumerate(indices):
        ans = lambda t: (op["values"][q * per + t], op["paths"][q * per + t])
        for s, (l, sides) in enumerate(st):
            part = (N >> l) // sides
            j = i % part
            if s == 0:
                vals = [0] * sides
                for t in range(k):
                    vt, pt = ans(t)
                    if not opened(own[t], 0, sides, j, vt, pt):
                        return False
                    vals = [(u + pow(alpha, t, p) * v) % p for u, v in zip(vals, vt)]
            else:
                vals, pt = ans(k + s - 1)
                if not opened(op["roots"][k + s - 1], l, sides, j, vals, pt):
                    return False
            x = pow(coset, 1 << l, p) * pow(w, j << l, p) % p
            if sides == 4:
                u0, u1 = fold2(vals[0], vals[2], rs[l], x, p), fold2(vals[1], vals[3], rs[l], iota * x % p, p)
                v, ln = fold2(u0, u1, rs[l + 1], x * x % p, p), l + 2
            else:
                v, ln = fold2(vals[0], vals[1], rs[l], x, p), l + 1
            if ln < R:
                npart = (N >> ln) // st[s + 1][1]
                want = op["values"][q * per + k + s][j // npart]
            else:
                x2 = pow(coset, 1 << R, p) * pow(w, j << R, p) % p
                want = sum(e * pow(x2, n, p) for n, e in enumerate(op["final"])) % p
            if v != want:
                return False
    return True


# ---- the C ABI's layout ------------------------------------------------------------------------------------------------------------------
def flat(proto, zk, op):
    """the opening in the C ABI's layout: points (P, d, 4), gamma (4,), polys (R, 3, 4), roots (k + steps - 1, 32), final (m, 4), challenges
    (R, 4), indices (Q,), values (Q, per, 4) -- (Q, R, 2, 4) for one table at log_arity 1 -- and paths (bytes), per query, per step, per side;
    one table: root (32,) and ys (P, 4); a batch: own_roots (k, 32) and ys (k, P, 4)"""
    field, d, R, Q, P = op["field"], op["d"], op["d"] - op["f"], op["Q"], len(op["points"])
    own, ys = _own(op, proto)

    def mont(ints):
        canon = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), np.uint64).reshape(-1, 4).copy()
        out = np.zeros_like(canon)
        assert zk.lib().zk_vec_from_canonical(field, canon.ctypes.data_as(zk._lib.u64p), canon.shape[0], out.ctypes.data_as(zk._lib.u64p)) == 0
        return out

    own_roots = np.frombuffer(b"".join(own), np.uint8).reshape(-1, 32).copy()
    fl = {
        "points": mont([v for z in op["points"] for v in z]).reshape(P, d, 4),
        "ys": mont([y for row in ys for y in row]).reshape(len(ys), P, 4),
        "gamma": mont([op["gamma"]])[0],
        "polys": mont([e for g in op["polys"] for e in g]).reshape(R, 3, 4),
        "roots": np.frombuffer(b"".join(op["roots"]), np.uint8).reshape(-1, 32).copy(),
        "final": mont(op["final"]),
        "challenges": mont(op["challenges"]),
        "indices": np.array(op["indices"], np.uint64),
        "values": mont([v for vs in op["values"] for v in vs]).reshape(Q, -1, 4),
        "paths": np.frombuffer(b"".join(b"".join(pt) for pths in op["paths"] for pt in pths), np.uint8).copy(),
    }
    if proto.batch:
        fl["own_roots"] = own_roots
    else:
        fl["root"], fl["ys"] = own_roots[0], fl["ys"][0]
        if proto.log_arity == 1:
            fl["values"] = fl["values"].reshape(Q, R, 2, 4)
    return fl
