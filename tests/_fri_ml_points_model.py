"""Python model of the multilinear opening of a FRI commitment at SEVERAL points (helper of tests/test_fri_ml_points_cpu.py and
test_gpu_fri_ml_points.py), built on the helpers of tests/_fri_ml_model.py.  The definition is the one of include/zkmle.h "FRI commitment
opened at several points":

  claims       y_p = the multilinear extension of T at z^p, p < P
  transcript   FRI's header, root_0, P (4 bytes), the points point-major, y_0 .. y_{P-1}, gamma, (g_l, r_l, root_{l+1})*, T_R, Q indices
  weights      W_0[x] = sum_p gamma^p eq(x, z^p);  W_{l+1} = mle_fold_last(W_l, r_l), as T_{l+1} from T_l
  round l      g_l(X) = sum_x' (W_l[2x'] + X (W_l[2x'+1] - W_l[2x'])) (T_l[2x'] + X (T_l[2x'+1] - T_l[2x'])), sent at X = 0, 1, 2
  verifier     claim_0 = sum_p gamma^p y_p; the sumcheck's checks; sum_j T_R[j] W_R[j] = the last claim with W_R from the points alone; FRI's
               query checks with the Lagrange fold

Everything is Python integers; nothing here knows how the library works.  `open_points(.., false_y=(p, v))` opens with claim p replaced by v:
round 0's polynomial is shifted so that g_0(0) + g_0(1) equals the false claim_0 and everything else is run honestly.

The second half is the transcript SCHEDULE of the succinct sparse GKR proof (zk_gkr_sparse_prove_succinct): oracle/pymodel.py gkr_prove_wide
opens a transcript of its own and cannot start from one that holds the root, so the oracle here is a replay -- every challenge re-derived
from the proof's elements in the order the header pins, root first."""
import numpy as np

import _fri_ml_model as ML
import _fri_model as FM
import _merkle_model as MM
import _ntt_model as NM
from oracle import pymodel as M

be32 = FM.be32


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


def round_polys(field, table, points, gamma, rs):
    """the round polynomials of the weight-table form on GIVEN challenges rs -> (polys, T_R)"""
    p = NM.MODULUS[field]
    T, W, polys = list(table), weights(points, gamma, p), []
    for r in rs:
        polys.append(round_g3(T, W, p))
        T, W = ML.mle_fold_last(field, T, r), ML.mle_fold_last(field, W, r)
    return polys, T


def _statement(tr, field, d, b, f, Q, coset, root, points, ys):
    p = NM.MODULUS[field]
    tr.append(FM.header(d, b, f, Q, coset))
    tr.append(root)
    tr.append(len(points).to_bytes(4, "big"))
    for z in points:
        for v in z:
            tr.append(be32(v % p))
    for y in ys:
        tr.append(be32(y % p))
    return tr.challenge(p)


def open_points(cm, points, f, Q, tr=None, false_y=None, hasher=M.keccak256):
    """-> the opening as a dict; `cm` is a tests/_fri_pcs_model.py commitment, points a list of P lists of d ints; `tr` is advanced"""
    field, d, b, coset = (cm[k] for k in ("field", "d", "b", "coset"))
    p, L, R = NM.MODULUS[field], d + b, d - f
    N = 1 << L
    assert 1 <= len(points) <= 8 and all(len(z) == d and all(0 <= v < p for v in z) for z in points) and 0 <= f < d and 1 <= Q <= 4096
    tr = M.Transcript() if tr is None else tr
    ys = [ML.mle_evaluate(field, cm["coeffs"], z) for z in points]
    claimed = list(ys)
    if false_y is not None:
        claimed[false_y[0]] = false_y[1] % p
    gamma = _statement(tr, field, d, b, f, Q, coset, cm["root"], points, claimed)
    shift = sum(pow(gamma, k, p) * (c - y) for k, (c, y) in enumerate(zip(claimed, ys))) % p
    T, W = [list(cm["coeffs"])], weights(points, gamma, p)
    layers, trees, roots = [list(cm["codeword"])], [cm["levels"]], [cm["root"]]
    polys, rs, c = [], [], coset % p
    for l in range(R):
        g = round_g3(T[l], W, p)
        if l == 0:
            g[0] = (g[0] + shift) % p                        # a false claim needs a round 0 that sums to it
        polys.append(g)
        for e in g:
            tr.append(be32(e))
        r = tr.challenge(p)
        rs.append(r)
        T.append(ML.mle_fold_last(field, T[l], r))
        W = ML.mle_fold_last(field, W, r)
        layers.append(ML.fold(field, layers[l], r, c))
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
    return {"field": field, "d": d, "b": b, "f": f, "Q": Q, "coset": coset % p, "root": cm["root"], "points": [list(z) for z in points], "ys": claimed,
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
        if l + 1 < R:
            tr.append(op["roots"][l + 1])
    for e in op["final"]:
        tr.append(be32(e % p))
    indices = [FM.sample_index(tr, N) for _ in range(Q)]
    every = [v for z in points for v in z] + list(ys) + [e for g in op["polys"] for e in g] + list(op["final"]) + [v for pair in op["values"] for v in pair]
    if any(not 0 <= v < p for v in every) or op["roots"][0] != op["root"] or not 1 <= len(points) <= 8 or len(ys) != len(points):
        return False
    claim = sum(pow(gamma, k, p) * y for k, y in enumerate(ys)) % p
    for l in range(R):
        g = op["polys"][l]
        if (g[0] + g[1]) % p != claim:
            return False
        claim = ML.interpolate3(g, rs[l], p)
    end = 0
    for k, z in enumerate(points):                           # W_R[j] = sum_p gamma^p A^p_R eq(j; z^p_0 .. z^p_{f-1})
        A = pow(gamma, k, p)
        for l in range(R):
            A = A * ML.eq1(rs[l], z[d - 1 - l], p) % p
        end += A * sum(t * e for t, e in zip(op["final"], ML.eq_table(z[:f], p)))
    if end % p != claim:
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


def flat(zk, op):
    """the opening in the C ABI's layout (tests/_fri_ml_model.py flat): points (P, d, 4), ys (P, 4) and gamma (4,) in place of z and y"""
    single = dict(op, z=[v for z in op["points"] for v in z], y=op["gamma"])
    fl = ML.flat(zk, single)
    P, d = len(op["points"]), op["d"]
    fl["points"] = fl.pop("z").reshape(P, d, 4)
    fl["gamma"] = fl.pop("y")
    canon = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in op["ys"]), np.uint64).reshape(-1, 4).copy()
    ys = np.zeros_like(canon)
    assert zk.lib().zk_vec_from_canonical(op["field"], canon.ctypes.data_as(zk._lib.u64p), canon.shape[0], ys.ctypes.data_as(zk._lib.u64p)) == 0
    fl["ys"] = ys
    return fl


# ---- the transcript schedule of the succinct sparse GKR proof ---------------------------------------------------------------------------
def gkr_succinct_replay(p, root, circuit_output, out_bits0, layer_claims, layer_coeffs, wb, wc):
    """Every challenge of zk_gkr_sparse_prove_succinct's GKR part, re-derived from the proof's integers: the commitment's root is absorbed FIRST,
    then gkr_protocol.rs' appends unchanged (oracle/pymodel.py gkr_prove_wide's order): the output layer's bytes, out_bits0 output challenges,
    per layer its claim and its rounds' little-endian coefficients with a challenge after each, and between layers wb, alpha, wc, beta.
    layer_coeffs[l]: the layer's round polynomials (coefficient lists).  -> dict(output_challenges, challenges (per layer), alpha, beta)"""
    t = M.Transcript()
    t.append(root)
    t.append(b"".join(be32(v) for v in circuit_output))
    out = {"output_challenges": [t.challenge(p) for _ in range(out_bits0)], "challenges": [], "alpha": [], "beta": []}
    nl = len(layer_coeffs)
    for l in range(nl):
        t.append(be32(layer_claims[l]))
        chal = []
        for co in layer_coeffs[l]:
            t.append(b"".join(M.le32(c) for c in co))
            chal.append(t.challenge(p))
        out["challenges"].append(chal)
        if l + 1 < nl:
            t.append(be32(wb[l]))
            out["alpha"].append(t.challenge(p))
            t.append(be32(wc[l]))
            out["beta"].append(t.challenge(p))
    return out
