"""Python model of the multilinear opening of SEVERAL FRI commitments with one proof (helper of tests/test_fri_ml_batch_cpu.py and
test_gpu_fri_ml_batch.py), built on the helpers of tests/_fri_ml_points_model.py, _fri_ml_arity_model.py and _fri_ml_grouped_model.py, none of
which it changes.  The definition is the one of include/zkmle.h "FRI commitments opened together":

  schedules    (log_arity 1, ungrouped), (2, ungrouped), (2, grouped): the steps of the single-table protocols
  transcript   FRI's header, "BTCH" a grouped k (16 bytes), the k roots, P, the points, the k P claims table-major, ONE gamma, then the rounds,
               the later roots, T_R and the indices as in the single-table protocol of the schedule
  combination  alpha = gamma^P;  claim_0 = sum_j alpha^j sum_p gamma^p y_{j,p};  T = sum_j alpha^j T_j;  f_0 = sum_j alpha^j f_j
  answers      step 0: per commitment its own values and its own path(s); steps s >= 1 as in the single-table protocol
  roots        the k commitments' first, then the later layers'

The prover builds every layer of the combined codeword with the two-point fold of _fri_ml_model.py; the verifier combines the opened layer-0
values and uses the step formulas, so an opening that passes ties the two together.  Everything is Python integers; nothing here knows how the
library works."""
import numpy as np

import _fri_ml_arity_model as AM
import _fri_ml_grouped_model as GM
import _fri_ml_model as ML
import _fri_ml_points_model as PT
import _fri_model as FM
import _merkle_model as MM
import _ntt_model as NM
from oracle import pymodel as M

be32 = FM.be32
KMAX = 16


def steps(L, R, a):
    """[(l, sides)] of the steps of an opening with R rounds at log_arity a"""
    return [(l, 2) for l in range(R)] if a == 1 else AM.steps(L, R)


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


def _statement(tr, field, d, b, f, Q, coset, a, grouped, roots, points, ys):
    p = NM.MODULUS[field]
    tr.append(FM.header(d, b, f, Q, coset))
    tr.append(b"BTCH" + a.to_bytes(4, "big") + int(bool(grouped)).to_bytes(4, "big") + len(roots).to_bytes(4, "big"))
    for r in roots:
        tr.append(r)
    tr.append(len(points).to_bytes(4, "big"))
    for z in points:
        for v in z:
            tr.append(be32(v % p))
    for row in ys:
        for y in row:
            tr.append(be32(y % p))
    return tr.challenge(p)


def _tree(layer, sides, grouped, hasher):
    return GM.levels_of(layer, sides.bit_length() - 1, hasher) if grouped else MM.levels_of([be32(e) for e in layer], hasher)


def _index_mod(N, a):
    return N if a == 1 else N // 2                           # FM.sample_index(tr, n) takes the sample mod n / 2


def open_batch(cms, points, f, Q, a=1, tr=None, hasher=M.keccak256):
    """-> the opening as a dict; `cms`: k commitments of tests/_fri_pcs_model.py (ungrouped) or of _fri_ml_grouped_model.py (all grouped), points
    a list of P lists of d ints; `tr` is advanced"""
    c0, k, P = cms[0], len(cms), len(points)
    field, d, b, coset = (c0[n] for n in ("field", "d", "b", "coset"))
    grouped = c0.get("log_group", 0) == 2
    assert all(c["field"] == field and c["d"] == d and c["b"] == b and c["coset"] == coset and (c.get("log_group", 0) == 2) == grouped for c in cms)
    p, L, R = NM.MODULUS[field], d + b, d - f
    N = 1 << L
    assert 1 <= k <= KMAX and 1 <= P <= 8 and all(len(z) == d and all(0 <= v < p for v in z) for z in points) and 0 <= f < d and 1 <= Q <= 4096
    assert a in (1, 2) and (a == 2 or not grouped) and (a == 1 or R >= 2)
    tr = M.Transcript() if tr is None else tr
    ys = [[ML.mle_evaluate(field, c["coeffs"], z) for z in points] for c in cms]
    own = [c["root"] for c in cms]
    gamma = _statement(tr, field, d, b, f, Q, coset, a, grouped, own, points, ys)
    alpha = pow(gamma, P, p)
    T = [sum(pow(alpha, j, p) * c["coeffs"][x] for j, c in enumerate(cms)) % p for x in range(1 << d)]
    W = PT.weights(points, gamma, p)
    st = steps(L, R, a)
    sides_at = dict(st)
    layers, trees, roots = {0: [sum(pow(alpha, j, p) * c["codeword"][x] for j, c in enumerate(cms)) % p for x in range(N)]}, {}, list(own)
    polys, rs, c = [], [], coset % p
    for l in range(R):
        g = PT.round_g3(T, W, p)
        polys.append(g)
        for e in g:
            tr.append(be32(e))
        r = tr.challenge(p)
        rs.append(r)
        T, W = ML.mle_fold_last(field, T, r), ML.mle_fold_last(field, W, r)
        layers[l + 1] = ML.fold(field, layers[l], r, c)
        c = c * c % p
        if l + 1 < R and l + 1 in sides_at:
            trees[l + 1] = _tree(layers[l + 1], sides_at[l + 1], grouped, hasher)
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
    return {"field": field, "d": d, "b": b, "f": f, "Q": Q, "coset": coset % p, "a": a, "grouped": grouped, "k": k, "own_roots": own,
            "points": [list(z) for z in points], "ys": ys, "gamma": gamma, "polys": polys, "roots": roots, "final": final, "challenges": rs,
            "indices": indices, "values": values, "paths": paths}


def verify(op, tr=None, hasher=M.keccak256):
    field, d, b, f, Q, coset, a, grouped, k, points, ys = (op[n] for n in ("field", "d", "b", "f", "Q", "coset", "a", "grouped", "k", "points", "ys"))
    p, L, R = NM.MODULUS[field], d + b, d - f
    N, P = 1 << L, len(points)
    w = NM.root_of_unity(field, L)
    tr = M.Transcript() if tr is None else tr
    if not 1 <= k <= KMAX or len(op["own_roots"]) != k or len(ys) != k or any(len(row) != P for row in ys) or not 1 <= P <= 8:
        return False
    if a not in (1, 2) or (grouped and a != 2) or (a == 2 and R < 2):
        return False
    st = steps(L, R, a)
    gamma = _statement(tr, field, d, b, f, Q, coset, a, grouped, op["own_roots"], points, ys)
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
    if any(not 0 <= v < p for v in every) or list(op["roots"][:k]) != list(op["own_roots"]) or len(op["roots"]) != k + len(st) - 1:
        return False
    alpha = pow(gamma, P, p)
    claim = sum(pow(gamma, j * P + q, p) * ys[j][q] for j in range(k) for q in range(P)) % p
    for l in range(R):
        g = op["polys"][l]
        if (g[0] + g[1]) % p != claim:
            return False
        claim = ML.interpolate3(g, rs[l], p)
    end = 0
    for q, z in enumerate(points):
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
            return GM.verify_leaf(root, j, vals, pths[0], hasher)
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
                    if not opened(op["own_roots"][t], 0, sides, j, vt, pt):
                        return False
                    vals = [(u + pow(alpha, t, p) * v) % p for u, v in zip(vals, vt)]
            else:
                vals, pt = ans(k + s - 1)
                if not opened(op["roots"][k + s - 1], l, sides, j, vals, pt):
                    return False
            x = pow(coset, 1 << l, p) * pow(w, j << l, p) % p
            if sides == 4:
                u0, u1 = AM.fold2(vals[0], vals[2], rs[l], x, p), AM.fold2(vals[1], vals[3], rs[l], iota * x % p, p)
                v, ln = AM.fold2(u0, u1, rs[l + 1], x * x % p, p), l + 2
            else:
                v, ln = AM.fold2(vals[0], vals[1], rs[l], x, p), l + 1
            if ln < R:
                npart = (N >> ln) // st[s + 1][1]
                want = op["values"][q * per + k + s][j // npart]
            else:
                x2 = pow(coset, 1 << R, p) * pow(w, j << R, p) % p
                want = sum(e * pow(x2, n, p) for n, e in enumerate(op["final"])) % p
            if v != want:
                return False
    return True


def flat(zk, op):
    """the opening in the C ABI's layout: own_roots (k, 32), points (P, d, 4), ys (k, P, 4), gamma (4,), polys (R, 3, 4), roots (k + steps - 1, 32),
    final (m, 4), challenges (R, 4), indices (Q,), values (Q, per, 4), paths (bytes)"""
    field, d, R, Q, P, k = op["field"], op["d"], op["d"] - op["f"], op["Q"], len(op["points"]), op["k"]

    def mont(ints):
        canon = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), np.uint64).reshape(-1, 4).copy()
        out = np.zeros_like(canon)
        assert zk.lib().zk_vec_from_canonical(field, canon.ctypes.data_as(zk._lib.u64p), canon.shape[0], out.ctypes.data_as(zk._lib.u64p)) == 0
        return out

    return {
        "own_roots": np.frombuffer(b"".join(op["own_roots"]), np.uint8).reshape(-1, 32).copy(),
        "points": mont([v for z in op["points"] for v in z]).reshape(P, d, 4),
        "ys": mont([y for row in op["ys"] for y in row]).reshape(k, P, 4),
        "gamma": mont([op["gamma"]])[0],
        "polys": mont([e for g in op["polys"] for e in g]).reshape(R, 3, 4),
        "roots": np.frombuffer(b"".join(op["roots"]), np.uint8).reshape(-1, 32).copy(),
        "final": mont(op["final"]),
        "challenges": mont(op["challenges"]),
        "indices": np.array(op["indices"], np.uint64),
        "values": mont([v for vs in op["values"] for v in vs]).reshape(Q, -1, 4),
        "paths": np.frombuffer(b"".join(b"".join(pt) for pths in op["paths"] for pt in pths), np.uint8).copy(),
    }
