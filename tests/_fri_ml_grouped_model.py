"""Python model of the Merkle tree with GROUPED leaves and of the multilinear opening of a FRI commitment over such trees (helper of
tests/test_fri_ml_grouped_cpu.py, test_gpu_merkle_grouped.py and test_gpu_fri_ml_grouped.py), built on tests/_fri_ml_arity_model.py,
_merkle_model.py and _fri_pcs_model.py, none of which it changes.  The definitions are those of include/zkmle.h "Merkle commitment with
grouped leaves" and "FRI commitment opened with grouped leaves":

  leaf         leaf_j = Keccak256(0x00 || be(e[j]) || be(e[j + part]) || ..), part = len >> log_group, j < part; nodes as ever over part leaves
  commitment   the codeword of tests/_fri_pcs_model.py under the tree with log_group = 2
  opening      the fold-by-4 opening of tests/_fri_ml_arity_model.py with three differences: the transcript takes 8 bytes (the arity 2, then a
               1) where that one takes 4; every committed layer is hashed with its leaves grouped by the sides of the step that starts
               there (4, or 2 for the final fold-2 step when R is odd); a step's answer holds ONE path, that of leaf j = i mod part

Everything is Python integers; nothing here knows how the library works."""
import _fri_ml_arity_model as AM
import _fri_ml_model as ML
import _fri_ml_points_model as PT
import _fri_model as FM
import _merkle_model as MM
import _ntt_model as NM
from oracle import pymodel as M

be32 = FM.be32
flat = AM.flat              # the C ABI's layout: a step's paths are a list of ONE path here
steps = AM.steps


def check_host_keccak(zk):
    """tests/_merkle_model.py check_host_keccak, and the host hash at the quad leaf's 129 bytes too"""
    h = MM.check_host_keccak(zk)
    for seed in range(3):
        data = bytes((seed * 57 + 11 * i + 129) & 0xFF for i in range(129))
        assert h(data) == M.keccak256(data), seed
    return h


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


def commit(field, coeffs, b, coset=1, hasher=M.keccak256, log_group=2):
    p = NM.MODULUS[field]
    cw = FM.extend(field, coeffs, b, coset)
    levels = levels_of(cw, log_group, hasher)
    return {"field": field, "d": len(coeffs).bit_length() - 1, "b": b, "coset": coset % p, "coeffs": list(coeffs), "codeword": cw, "levels": levels,
            "root": levels[-1][0], "log_group": log_group}


def sizes(d, b, f, Q):
    """(nroots, nfinal, nvalues, path_bytes, nround): the arity model's with one path of L - l - log_sides digests per step"""
    L, R = d + b, d - f
    nroots, nfinal, nvalues, _, nround = AM.sizes(d, b, f, Q)
    return nroots, nfinal, nvalues, 32 * Q * sum(L - l - (sides.bit_length() - 1) for l, sides in steps(L, R)), nround


def _statement(tr, field, d, b, f, Q, coset, root, points, ys):
    p = NM.MODULUS[field]
    tr.append(FM.header(d, b, f, Q, coset))
    tr.append((2).to_bytes(4, "big") + (1).to_bytes(4, "big"))
    tr.append(root)
    tr.append(len(points).to_bytes(4, "big"))
    for z in points:
        for v in z:
            tr.append(be32(v % p))
    for y in ys:
        tr.append(be32(y % p))
    return tr.challenge(p)


def open_points(cm, points, f, Q, tr=None, hasher=M.keccak256):
    """-> the opening as a dict; `cm` is a commit() of this module, points a list of P lists of d ints; `tr` is advanced"""
    field, d, b, coset = (cm[k] for k in ("field", "d", "b", "coset"))
    p, L, R = NM.MODULUS[field], d + b, d - f
    N = 1 << L
    assert cm["log_group"] == 2 and 1 <= len(points) <= 8 and all(len(z) == d and all(0 <= v < p for v in z) for z in points)
    assert 0 <= f and R >= 2 and 1 <= Q <= 4096
    tr = M.Transcript() if tr is None else tr
    ys = [ML.mle_evaluate(field, cm["coeffs"], z) for z in points]
    gamma = _statement(tr, field, d, b, f, Q, coset, cm["root"], points, ys)
    T, W = list(cm["coeffs"]), PT.weights(points, gamma, p)
    sides_at = dict(steps(L, R))
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
            trees[l + 1] = levels_of(layers[l + 1], sides_at[l + 1].bit_length() - 1, hasher)
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
            paths.append([MM.path_of(trees[l], j)])
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
            if len(vals) != sides or len(pths) != 1 or len(pths[0]) != L - l - (sides.bit_length() - 1):
                return False
            if not verify_leaf(op["roots"][l // 2], j, vals, pths[0], hasher):
                return False
            x = pow(coset, 1 << l, p) * pow(w, j << l, p) % p
            if sides == 4:
                u0, u1 = AM.fold2(vals[0], vals[2], rs[l], x, p), AM.fold2(vals[1], vals[3], rs[l], iota * x % p, p)
                v, ln = AM.fold2(u0, u1, rs[l + 1], x * x % p, p), l + 2
            else:
                v, ln = AM.fold2(vals[0], vals[1], rs[l], x, p), l + 1
            if ln < R:
                npart = (N >> ln) // st[s + 1][1]
                want = op["values"][q * len(st) + s + 1][j // npart]
            else:
                x2 = pow(coset, 1 << R, p) * pow(w, j << R, p) % p
                want = sum(e * pow(x2, k, p) for k, e in enumerate(op["final"])) % p
            if v != want:
                return False
    return True
