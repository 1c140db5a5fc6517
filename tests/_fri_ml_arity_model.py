"""Python model of the multilinear opening of a FRI commitment at several points FOLDED BY 4 (helper of tests/test_fri_ml_arity_cpu.py and
test_gpu_fri_ml_arity.py), built on the helpers of tests/_fri_ml_points_model.py and _fri_ml_model.py.  The definition is the one of
include/zkmle.h "FRI commitment opened with a fold arity", log_arity = 2:

  layers       the even l < R are committed: ceil(R / 2) roots.  A step starts at an even l: a fold by 4 to f_{l+2} if l + 2 <= R, else
               (R odd, l = R - 1) the fold by 2 to the final layer
  transcript   FRI's header, the arity (4 bytes), root_0, P, the points, the y_p, gamma, (g_l, r_l, root_{l+1} only if l + 1 is even and
               below R)*, T_R, Q indices mod N / 4
  fold by 4    u0 = fold(f[k], f[k + N_l/2]; r_l, x), u1 = fold(f[k + N_l/4], f[k + 3 N_l/4]; r_l, i x), f_{l+2}[k] = fold(u0, u1; r_{l+1}, x^2)
               with fold(a, b; r, x) = (1 - r)(a + b) / 2 + r (a - b) / (2 x), x = c_l w_l^k, i = w_l^(N_l / 4)
  answers      per query, per step, the sides s = 0 .. 3 (or 0, 1): f_l[j + s N_l / sides], j = i mod N_l / sides, and their paths

The sumcheck is the several-point protocol's, unchanged.  The prover below builds EVERY layer with the two-point fold of _fri_ml_model.py
(the odd ones only to get to the even ones); the verifier uses the four-point formula, so an opening that passes ties the two together.
Everything is Python integers; nothing here knows how the library works."""
import numpy as np

import _fri_ml_model as ML
import _fri_ml_points_model as PT
import _fri_model as FM
import _merkle_model as MM
import _ntt_model as NM
from oracle import pymodel as M

be32 = FM.be32


def fold2(a, b, r, x, p):
    return ((1 - r) * (a + b) * pow(2, p - 2, p) + r * (a - b) * pow(2 * x, -1, p)) % p


def fold4_formula(field, table, r0, r1, coset=1):
    """the four-point formula on a codeword of len >= 4 on {coset w_len^k} -> len / 4 entries"""
    p, n = NM.MODULUS[field], len(table)
    q = n // 4
    w = NM.root_of_unity(field, n.bit_length() - 1)
    iota = pow(w, q, p)
    out = []
    for k in range(q):
        x = coset * pow(w, k, p) % p
        u0 = fold2(table[k], table[k + 2 * q], r0, x, p)
        u1 = fold2(table[k + q], table[k + 3 * q], r0, iota * x % p, p)
        out.append(fold2(u0, u1, r1, x * x % p, p))
    return out


def steps(L, R):
    """[(l, sides)] of the steps of an opening with R rounds"""
    return [(l, 4 if l + 2 <= R else 2) for l in range(0, R, 2)]


def sizes(d, b, f, Q):
    """(nroots, nfinal, nvalues, path_bytes, nround) by the header's formulas"""
    L, R = d + b, d - f
    return ((R + 1) // 2, 1 << f, Q * (4 * (R // 2) + 2 * (R % 2)), 32 * Q * sum(s * (L - l) for l, s in steps(L, R)), 3 * R)


def _statement(tr, field, d, b, f, Q, coset, root, points, ys):
    p = NM.MODULUS[field]
    tr.append(FM.header(d, b, f, Q, coset))
    tr.append((2).to_bytes(4, "big"))
    tr.append(root)
    tr.append(len(points).to_bytes(4, "big"))
    for z in points:
        for v in z:
            tr.append(be32(v % p))
    for y in ys:
        tr.append(be32(y % p))
    return tr.challenge(p)


def open_points(cm, points, f, Q, tr=None, hasher=M.keccak256):
    """-> the opening as a dict; `cm` is a tests/_fri_pcs_model.py commitment, points a list of P lists of d ints; `tr` is advanced"""
    field, d, b, coset = (cm[k] for k in ("field", "d", "b", "coset"))
    p, L, R = NM.MODULUS[field], d + b, d - f
    N = 1 << L
    assert 1 <= len(points) <= 8 and all(len(z) == d and all(0 <= v < p for v in z) for z in points) and 0 <= f and R >= 2 and 1 <= Q <= 4096
    tr = M.Transcript() if tr is None else tr
    ys = [ML.mle_evaluate(field, cm["coeffs"], z) for z in points]
    gamma = _statement(tr, field, d, b, f, Q, coset, cm["root"], points, ys)
    T, W = list(cm["coeffs"]), PT.weights(points, gamma, p)
    layers, trees, roots = {0: list(cm["codeword"])}, {0: cm["levels"]}, [cm["root"]]
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
        if l + 1 < R and (l + 1) % 2 == 0:
            trees[l + 1] = MM.levels_of([be32(e) for e in layers[l + 1]], hasher)
            roots.append(trees[l + 1][-1][0])
            tr.append(roots[-1])
    final = T
    for e in final:
        tr.append(be32(e))
    indices = [FM.sample_index(tr, N // 2) for _ in range(Q)]        # sample_index(tr, n) takes the sample mod n / 2: here mod N / 4
    values, paths = [], []
    for i in indices:
        for l, sides in steps(L, R):
            part = (N >> l) // sides
            j = i % part
            values.append([layers[l][j + s * part] for s in range(sides)])
            paths.append([MM.path_of(trees[l], j + s * part) for s in range(sides)])
    return {"field": field, "d": d, "b": b, "f": f, "Q": Q, "coset": coset % p, "root": cm["root"], "points": [list(z) for z in points], "ys": ys,
            "gamma": gamma, "polys": polys, "roots": roots, "final": final, "challenges": rs, "indices": indices, "values": values, "paths": paths}


def verify(op, tr=None, hasher=M.keccak256):
    field, d, b, f, Q, coset, points, ys = (op[k] for k in ("field", "d", "b", "f", "Q", "coset", "points", "ys"))
    p, L, R = NM.MODULUS[field], d + b, d - f
    N = 1 << L
    w = NM.root_of_unity(field, L)
    tr = M.Transcript() if tr is None else tr
    gamma = _statement(tr, field, d, b, f, Q, coset, op["root"], points, ys)
    rs = []
    for l in range(R):
        for e in op["polys"][l]:
            tr.append(be32(e % p))
        rs.append(tr.challenge(p))
        if l + 1 < R and (l + 1) % 2 == 0:
            tr.append(op["roots"][(l + 1) // 2])
    for e in op["final"]:
        tr.append(be32(e % p))
    indices = [FM.sample_index(tr, N // 2) for _ in range(Q)]
    every = [v for z in points for v in z] + list(ys) + [e for g in op["polys"] for e in g] + list(op["final"]) + [v for vs in op["values"] for v in vs]
    if any(not 0 <= v < p for v in every) or op["roots"][0] != op["root"] or not 1 <= len(points) <= 8 or len(ys) != len(points) or R < 2:
        return False
    claim = sum(pow(gamma, k, p) * y for k, y in enumerate(ys)) % p
    for l in range(R):
        g = op["polys"][l]
        if (g[0] + g[1]) % p != claim:
            return False
        claim = ML.interpolate3(g, rs[l], p)
    end = 0
    for k, z in enumerate(points):
        A = pow(gamma, k, p)
        for l in range(R):
            A = A * ML.eq1(rs[l], z[d - 1 - l], p) % p
        end += A * sum(t * e for t, e in zip(op["final"], ML.eq_table(z[:f], p)))
    if end % p != claim:
        return False
    st = steps(L, R)
    iota = pow(w, N // 4, p)
    for q, i in enumerate(indices):
        for s, (l, sides) in enumerate(st):
            part = (N >> l) // sides
            j = i % part
            vals, pths = op["values"][q * len(st) + s], op["paths"][q * len(st) + s]
            if len(vals) != sides or len(pths) != sides or any(len(pt) != L - l for pt in pths):
                return False
            if not all(MM.verify_path(op["roots"][l // 2], j + k * part, be32(vals[k]), pths[k], hasher) for k in range(sides)):
                return False
            x = pow(coset, 1 << l, p) * pow(w, j << l, p) % p
            if sides == 4:
                u0, u1 = fold2(vals[0], vals[2], rs[l], x, p), fold2(vals[1], vals[3], rs[l], iota * x % p, p)
                v, ln = fold2(u0, u1, rs[l + 1], x * x % p, p), l + 2
            else:
                v, ln = fold2(vals[0], vals[1], rs[l], x, p), l + 1
            if ln < R:
                npart = (N >> ln) // st[s + 1][1]
                want = op["values"][q * len(st) + s + 1][j // npart]
            else:
                x2 = pow(coset, 1 << R, p) * pow(w, j << R, p) % p
                want = sum(e * pow(x2, k, p) for k, e in enumerate(op["final"])) % p
            if v != want:
                return False
    return True


def flat(zk, op):
    """the opening in the C ABI's layout: as tests/_fri_ml_points_model.py flat with roots (ceil(R / 2), 32), values (Q, per, 4) and the paths
    per query, per step, per side"""
    field, d, R, Q, P = op["field"], op["d"], op["d"] - op["f"], op["Q"], len(op["points"])

    def mont(ints):
        canon = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), np.uint64).reshape(-1, 4).copy()
        out = np.zeros_like(canon)
        assert zk.lib().zk_vec_from_canonical(field, canon.ctypes.data_as(zk._lib.u64p), canon.shape[0], out.ctypes.data_as(zk._lib.u64p)) == 0
        return out

    return {
        "root": np.frombuffer(op["root"], np.uint8).copy(),
        "points": mont([v for z in op["points"] for v in z]).reshape(P, d, 4),
        "ys": mont(op["ys"]),
        "gamma": mont([op["gamma"]])[0],
        "polys": mont([e for g in op["polys"] for e in g]).reshape(R, 3, 4),
        "roots": np.frombuffer(b"".join(op["roots"]), np.uint8).reshape(-1, 32).copy(),
        "final": mont(op["final"]),
        "challenges": mont(op["challenges"]),
        "indices": np.array(op["indices"], np.uint64),
        "values": mont([v for vs in op["values"] for v in vs]).reshape(Q, -1, 4),
        "paths": np.frombuffer(b"".join(b"".join(pt) for pths in op["paths"] for pt in pths), np.uint8).copy(),
    }
