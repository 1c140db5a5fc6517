"""Python model of the multilinear opening of a FRI commitment (helper of tests/test_fri_ml_cpu.py and test_gpu_fri_ml.py).  The definition
is the one of include/zkmle.h "FRI commitment opened as a multilinear polynomial":

  commitment   tests/_fri_pcs_model.py commit(T, b, c): the entries of the evaluation table T read as coefficients
  claim        y = the multilinear extension of T at z = (z_0 .. z_{d-1}), variable 0 the most significant index bit
  round l      binds the LOWEST index bit of T_l (variable v = d - 1 - l):  S_X = sum_x' E_l[x'] T_l[2x' + X] with E_l the eq table of
               (z_0 .. z_{v-1});  g_l(X) = A_l eq1(X, z_v) (S_0 + X (S_1 - S_0)), sent at X = 0, 1, 2;  r_l = challenge;
               T_{l+1}[i] = (1 - r_l) T_l[2i] + r_l T_l[2i+1];  f_{l+1}[k] = (1 - r_l) (f_l[k] + f_l[k+h]) / 2 + r_l (f_l[k] - f_l[k+h]) / (2 c_l w_l^k)
  transcript   FRI's header, root_0, z, y, (g_l, r_l, root_{l+1})*, the m entries of T_R, Q indices
  verifier     the sumcheck's checks, A_R MLE(T_R)(z_0 .. z_{f-1}) = the last claim, and FRI's query checks with the fold above

Everything is Python integers; nothing here knows how the library works.  `open_at(.., false_y=..)` opens with a claim that is not the
evaluation: round 0's polynomial is shifted so that g_0(0) + g_0(1) equals the false claim and everything else is run honestly."""
import numpy as np

import _fri_model as FM
import _merkle_model as MM
import _ntt_model as NM
from oracle import pymodel as M

be32 = FM.be32


def eq1(a, b, p):
    return (a * b + (1 - a) * (1 - b)) % p


def eq_table(z, p):
    """eq(z, x) over len(z) variables, variable 0 the most significant bit of x"""
    t = [1]
    for zi in z:
        t = [v for e in t for v in (e * (1 - zi) % p, e * zi % p)]
    return t


def mle_evaluate(field, table, z):
    """zk_mle_evaluate: successive folds of variable 0"""
    p, t = NM.MODULUS[field], list(table)
    for zi in z:
        h = len(t) // 2
        t = [(t[j] + zi * (t[j + h] - t[j])) % p for j in range(h)]
    assert len(t) == 1
    return t[0]


def mle_fold_last(field, table, r):
    """zk_mle_fold(table, var = last, r)"""
    p = NM.MODULUS[field]
    return [((1 - r) * table[2 * i] + r * table[2 * i + 1]) % p for i in range(len(table) // 2)]


def fold(field, table, r, coset=1):
    """one Lagrange-form fold of a codeword of len >= 2 on {coset w_len^k}"""
    p, n = NM.MODULUS[field], len(table)
    h = n // 2
    w = NM.root_of_unity(field, n.bit_length() - 1)
    inv2 = pow(2, p - 2, p)
    out, x = [], coset % p
    for k in range(h):
        a, b = table[k], table[k + h]
        out.append(((1 - r) * (a + b) * inv2 + r * (a - b) * pow(2 * x, -1, p)) % p)
        x = x * w % p
    return out


def sizes(d, b, f, Q):
    return FM.sizes(d, b, f, Q) + (3 * (d - f),)


def interpolate3(g, r, p):
    """the quadratic through (0, g[0]), (1, g[1]), (2, g[2]) at r"""
    inv2 = pow(2, p - 2, p)
    return (g[0] * (r - 1) * (r - 2) * inv2 - g[1] * r * (r - 2) + g[2] * r * (r - 1) * inv2) % p


def open_at(cm, z, f, Q, tr=None, false_y=None, hasher=M.keccak256):
    """-> the opening as a dict; `cm` is a tests/_fri_pcs_model.py commitment, z a list of d ints; `tr` is advanced"""
    field, d, b, coset = (cm[k] for k in ("field", "d", "b", "coset"))
    p, L, R = NM.MODULUS[field], d + b, d - f
    N = 1 << L
    assert len(z) == d and 0 <= f < d and 1 <= Q <= 4096 and all(0 <= v < p for v in z)
    tr = M.Transcript() if tr is None else tr
    tr.append(FM.header(d, b, f, Q, coset))
    tr.append(cm["root"])
    for v in z:
        tr.append(be32(v))
    y = mle_evaluate(field, cm["coeffs"], z)
    claimed = y if false_y is None else false_y % p
    tr.append(be32(claimed))
    T, layers, trees, roots = [list(cm["coeffs"])], [list(cm["codeword"])], [cm["levels"]], [cm["root"]]
    polys, rs, A, c = [], [], 1, coset % p
    for l in range(R):
        v = d - 1 - l
        E = eq_table(z[:v], p)
        S = [sum(E[x] * T[l][2 * x + X] for x in range(len(E))) % p for X in (0, 1)]
        g = [A * eq1(X, z[v], p) * (S[0] + X * (S[1] - S[0])) % p for X in (0, 1, 2)]
        if l == 0 and false_y is not None:                   # the false claim needs a round 0 that sums to it
            g[0] = (g[0] + claimed - y) % p
        polys.append(g)
        for e in g:
            tr.append(be32(e))
        r = tr.challenge(p)
        rs.append(r)
        A = A * eq1(r, z[v], p) % p
        T.append(mle_fold_last(field, T[l], r))
        layers.append(fold(field, layers[l], r, c))
        c = c * c % p
        if l + 1 < R:
            lv = MM.levels_of([be32(e) for e in layers[l + 1]], hasher)
            trees.append(lv)
            roots.append(lv[-1][0])
            tr.append(roots[l + 1])
    final = T[R]
    for e in final:
        tr.append(be32(e))
    indices = [FM.sample_index(tr, N) for _ in range(Q)]
    values, paths = [], []
    for i in indices:
        for l in range(R):
            h = (N >> l) // 2
            j = i % h
            values.append((layers[l][j], layers[l][j + h]))
            paths.append((MM.path_of(trees[l], j), MM.path_of(trees[l], j + h)))
    return {"field": field, "d": d, "b": b, "f": f, "Q": Q, "coset": coset % p, "root": cm["root"], "z": list(z), "y": claimed, "polys": polys,
            "roots": roots, "final": final, "challenges": rs, "indices": indices, "values": values, "paths": paths, "layers": layers, "tables": T}


def verify(op, tr=None, hasher=M.keccak256):
    field, d, b, f, Q, coset, z = (op[k] for k in ("field", "d", "b", "f", "Q", "coset", "z"))
    p, L, R = NM.MODULUS[field], d + b, d - f
    N = 1 << L
    w = NM.root_of_unity(field, L)
    tr = M.Transcript() if tr is None else tr
    tr.append(FM.header(d, b, f, Q, coset))
    tr.append(op["root"])
    for v in z:
        tr.append(be32(v % p))
    tr.append(be32(op["y"] % p))
    rs = []
    for l in range(R):
        for e in op["polys"][l]:
            tr.append(be32(e % p))
        rs.append(tr.challenge(p))
        if l + 1 < R:
            tr.append(op["roots"][l + 1])
    for e in op["final"]:
        tr.append(be32(e % p))
    indices = [FM.sample_index(tr, N) for _ in range(Q)]
    every = list(z) + [op["y"]] + [e for g in op["polys"] for e in g] + list(op["final"]) + [v for pair in op["values"] for v in pair]
    if any(not 0 <= v < p for v in every) or op["roots"][0] != op["root"]:
        return False
    claim, A = op["y"], 1
    for l in range(R):
        g = op["polys"][l]
        if (g[0] + g[1]) % p != claim:
            return False
        claim = interpolate3(g, rs[l], p)
        A = A * eq1(rs[l], z[d - 1 - l], p) % p
    if A * mle_evaluate(field, op["final"], z[:f]) % p != claim:
        return False
    inv2 = pow(2, p - 2, p)
    for q, i in enumerate(indices):
        for l in range(R):
            h = (N >> l) // 2
            j = i % h
            (lo, hi), (plo, phi) = op["values"][q * R + l], op["paths"][q * R + l]
            if len(plo) != L - l or len(phi) != L - l:
                return False
            if not MM.verify_path(op["roots"][l], j, be32(lo), plo, hasher) or not MM.verify_path(op["roots"][l], j + h, be32(hi), phi, hasher):
                return False
            x = pow(coset, 1 << l, p) * pow(w, j << l, p) % p
            v = ((1 - rs[l]) * (lo + hi) * inv2 + rs[l] * (lo - hi) * pow(2 * x, -1, p)) % p
            if l + 1 < R:
                want = op["values"][q * R + l + 1][0 if j < h // 2 else 1]
            else:
                x2 = pow(coset, 1 << R, p) * pow(w, j << R, p) % p
                want = sum(e * pow(x2, k, p) for k, e in enumerate(op["final"])) % p
            if v != want:
                return False
    return True


# ---- the basic sumcheck that ends in such an opening ------------------------------------------------------------------------------------
def sumcheck_prove(cm, f, Q, tr=None, hasher=M.keccak256):
    """prover.rs:35-71 with the first append replaced by the commitment's root, then the opening at the challenges on the same transcript"""
    field, p = cm["field"], NM.MODULUS[cm["field"]]
    tr = M.Transcript() if tr is None else tr
    tr.append(cm["root"])
    t = list(cm["coeffs"])
    claimed = sum(t) % p
    tr.append(be32(claimed))
    rounds, chal = [], []
    while len(t) > 1:
        h = len(t) // 2
        e0, e1 = sum(t[:h]) % p, sum(t[h:]) % p
        rounds.append((e0, e1))
        tr.append(be32(e0))
        tr.append(be32(e1))
        r = tr.challenge(p)
        chal.append(r)
        t = [(t[j] + r * (t[j + h] - t[j])) % p for j in range(h)]
    return {"claimed_sum": claimed, "rounds": rounds, "challenges": chal, "opening": open_at(cm, chal, f, Q, tr, hasher=hasher)}


def sumcheck_verify(pr, root, tr=None, hasher=M.keccak256):
    op = pr["opening"]
    p = NM.MODULUS[op["field"]]
    tr = M.Transcript() if tr is None else tr
    tr.append(root)
    cur, good = pr["claimed_sum"], True
    tr.append(be32(cur % p))
    chal = []
    for e0, e1 in pr["rounds"]:
        good = good and (e0 + e1) % p == cur and 0 <= e0 < p and 0 <= e1 < p
        tr.append(be32(e0 % p))
        tr.append(be32(e1 % p))
        r = tr.challenge(p)
        chal.append(r)
        cur = (e0 + r * (e1 - e0)) % p
    good = good and cur == op["y"] and len(chal) == op["d"] and 0 <= pr["claimed_sum"] < p
    return verify(dict(op, root=root, z=chal), tr, hasher) and good


def flat(zk, op):
    """the opening in the C ABI's layout: root (32,) u8, z (d, 4) and y (4,) u64 Montgomery, polys (R, 3, 4), roots (R, 32) u8, final (m, 4),
    challenges (R, 4), indices (Q,) u64, values (Q, R, 2, 4), paths (path_bytes,) u8"""
    field, R, Q = op["field"], op["d"] - op["f"], op["Q"]

    def mont(ints):
        canon = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), np.uint64).reshape(-1, 4).copy()
        out = np.zeros_like(canon)
        assert zk.lib().zk_vec_from_canonical(field, canon.ctypes.data_as(zk._lib.u64p), canon.shape[0], out.ctypes.data_as(zk._lib.u64p)) == 0
        return out

    return {
        "root": np.frombuffer(op["root"], np.uint8).copy(),
        "z": mont(op["z"]),
        "y": mont([op["y"]])[0],
        "polys": mont([e for g in op["polys"] for e in g]).reshape(R, 3, 4),
        "roots": np.frombuffer(b"".join(op["roots"]), np.uint8).reshape(R, 32).copy(),
        "final": mont(op["final"]),
        "challenges": mont(op["challenges"]),
        "indices": np.array(op["indices"], np.uint64),
        "values": mont([v for pair in op["values"] for v in pair]).reshape(Q, R, 2, 4),
        "paths": np.frombuffer(b"".join(b"".join(lo) + b"".join(hi) for lo, hi in op["paths"]), np.uint8).copy(),
    }
