"""Python model of the Merkle tree over several COLUMNS, of the commitment to k tables under one such tree and of the multilinear opening of
several such commitments together (helper of tests/test_fri_columns_cpu.py, test_gpu_merkle_columns.py and test_gpu_fri_columns.py).  The
definitions are those of include/zkmle.h "Merkle commitment of several columns" and "Column commitments opened together":

  leaf         leaf_j = Keccak256(0x00 || for c < k: for s < 4: be(f_c[j + s part])), part = len >> 2, j < part; nodes as ever over part leaves
  commitment   the k codewords of tests/_fri_pcs_model.py's extension under ONE such tree
  opening      the grouped fold-by-4 batch opening of tests/_fri_ml_family_model.py over all K = sum w_i columns with three differences: the
               statement's line is "COLS", 2, m and the m widths, followed by the m roots; a query's step 0 holds the K columns' quads but
               ONE path per commitment, whose leaf is hashed from all of that commitment's quads; m roots lead `roots`

The pieces the protocols share (weights, round_g3, fold2, steps) are the family model's, imported; the prover builds every layer with the
two-point fold and the verifier uses the step formulas, so an opening that passes ties the two together.  Everything is Python integers;
nothing here knows how the library works."""
import numpy as np

import _fri_ml_family_model as FAM
import _fri_ml_grouped_model as GM
import _fri_ml_model as ML
import _fri_model as FM
import _grind_model as GR
import _merkle_model as MM
import _ntt_model as NM
from oracle import pymodel as M

be32, be4 = FM.be32, FAM.be4
KMAX = 32                                                    # columns of one commitment, and of one opening
A = 2                                                        # the only schedule: fold by 4 on grouped leaves


def blocks(k):
    """B(k): the permutations a leaf of k columns costs"""
    return (1 + 128 * k) // 136 + 1


def check_host_keccak(zk):
    """tests/_fri_ml_grouped_model.py check_host_keccak, and the host hash at leaves of 2, 17 and 32 columns: several blocks, the message's end
    one byte into a block, and the longest"""
    h = GM.check_host_keccak(zk)
    for k in (2, 17, 32):
        n = 1 + 128 * k
        data = bytes((k * 29 + 13 * i + n) & 0xFF for i in range(n))
        assert h(data) == M.keccak256(data), k
    return h


def leaf_messages(columns):
    """the leaves' messages (without the tag) of k columns of canonical ints"""
    n = len(columns[0])
    part = n >> 2
    assert 1 <= len(columns) <= KMAX and part >= 1 and all(len(c) == n for c in columns) and part << 2 == n
    return [b"".join(be32(c[j + s * part]) for c in columns for s in range(4)) for j in range(part)]


def levels_of(columns, hasher=M.keccak256):
    return MM.levels_of(leaf_messages(columns), hasher)


def verify_leaf(root, index, quads, path, hasher=M.keccak256):
    """quads: per column the leaf's 4 canonical ints"""
    return MM.verify_path(root, index, b"".join(be32(v) for q in quads for v in q), path, hasher)


def commit(field, tables, b, coset=1, hasher=M.keccak256):
    """tables: k lists of 2^d canonical ints"""
    p = NM.MODULUS[field]
    cws = [FM.extend(field, t, b, coset) for t in tables]
    levels = levels_of(cws, hasher)
    return {"field": field, "d": len(tables[0]).bit_length() - 1, "b": b, "coset": coset % p, "k": len(tables), "coeffs": [list(t) for t in tables],
            "codeword": cws, "levels": levels, "root": levels[-1][0]}


def sizes(widths, d, b, f, Q):
    """(nroots, nfinal, nvalues, path_bytes, nround) by the header's formulas"""
    m, K, L = len(widths), sum(widths), d + b
    nroots, nfinal, nvalues, path_bytes, nround = FAM.sizes(1, d, b, f, Q, A, True)
    return m + nroots - 1, nfinal, nvalues + 4 * Q * (K - 1), path_bytes + 32 * Q * (L - 2) * (m - 1), nround


def _statement(tr, field, d, b, f, Q, coset, widths, own_roots, points, ys):
    """absorbs the statement (ys: one row of claims per column, global order) -> gamma"""
    p = NM.MODULUS[field]
    tr.append(FM.header(d, b, f, Q, coset))
    tr.append(b"COLS" + be4(A) + be4(len(widths)) + b"".join(be4(w) for w in widths))
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


def open_columns(cms, points, f, Q, tr=None, hasher=M.keccak256):
    """-> the opening as a dict; `cms`: m commit()s of this module; points a list of P lists of d ints; `tr` is advanced"""
    c0, m, P = cms[0], len(cms), len(points)
    field, d, b, coset = (c0[n] for n in ("field", "d", "b", "coset"))
    assert all(c["field"] == field and c["d"] == d and c["b"] == b and c["coset"] == coset for c in cms)
    widths = [c["k"] for c in cms]
    K = sum(widths)
    p, L, R = NM.MODULUS[field], d + b, d - f
    N = 1 << L
    assert 1 <= m and K <= KMAX and 1 <= P <= 8 and all(len(z) == d and all(0 <= v < p for v in z) for z in points)
    assert 0 <= f < d and 1 <= Q <= 4096 and R >= 2
    tr = M.Transcript() if tr is None else tr
    tables = [t for c in cms for t in c["coeffs"]]              # the K columns in global order
    codewords = [w for c in cms for w in c["codeword"]]
    ys = [[ML.mle_evaluate(field, t, z) for z in points] for t in tables]
    own = [c["root"] for c in cms]
    gamma = _statement(tr, field, d, b, f, Q, coset, widths, own, points, ys)
    alpha = pow(gamma, P, p)
    T = [sum(pow(alpha, j, p) * t[x] for j, t in enumerate(tables)) % p for x in range(1 << d)]
    W = FAM.weights(points, gamma, p)
    st = FAM.steps(L, R, A)
    sides_at = dict(st)
    layers, trees, roots = {0: [sum(pow(alpha, j, p) * w[x] for j, w in enumerate(codewords)) % p for x in range(N)]}, {}, list(own)
    polys, rs, c = [], [], coset % p
    for l in range(R):
        g = FAM.round_g3(T, W, p)
        polys.append(g)
        for e in g:
            tr.append(be32(e))
        r = tr.challenge(p)
        rs.append(r)
        T, W = ML.mle_fold_last(field, T, r), ML.mle_fold_last(field, W, r)
        layers[l + 1] = ML.fold(field, layers[l], r, c)
        c = c * c % p
        if l + 1 < R and l + 1 in sides_at:
            trees[l + 1] = FAM.levels_of(layers[l + 1], sides_at[l + 1].bit_length() - 1, hasher)
            roots.append(trees[l + 1][-1][0])
            tr.append(roots[-1])
    final = T
    for e in final:
        tr.append(be32(e))
    indices = [FM.sample_index(tr, N // 2) for _ in range(Q)]   # FM.sample_index takes the sample mod n / 2: positions of N / 4
    values, paths = [], []                                   # per query: step 0's K quads and m paths, then the later steps' one each
    for i in indices:
        for l, sides in st:
            part = (N >> l) // sides
            j = i % part
            if l == 0:
                values += [[w[j + s * part] for s in range(4)] for w in codewords]
                paths += [MM.path_of(cm["levels"], j) for cm in cms]
            else:
                values.append([layers[l][j + s * part] for s in range(sides)])
                paths.append(MM.path_of(trees[l], j))
    return {"field": field, "d": d, "b": b, "f": f, "Q": Q, "coset": coset % p, "widths": widths, "own_roots": own, "ys": ys,
            "points": [list(z) for z in points], "gamma": gamma, "polys": polys, "roots": roots, "final": final, "challenges": rs, "indices": indices,
            "values": values, "paths": paths}


def verify(op, tr=None, hasher=M.keccak256):
    field, d, b, f, Q, coset, points, widths = (op[n] for n in ("field", "d", "b", "f", "Q", "coset", "points", "widths"))
    own, ys = op["own_roots"], op["ys"]
    m, K = len(widths), sum(widths)
    p, L, R = NM.MODULUS[field], d + b, d - f
    N, P = 1 << L, len(points)
    w = NM.root_of_unity(field, L)
    tr = M.Transcript() if tr is None else tr
    if m < 1 or any(x < 1 for x in widths) or K > KMAX or len(own) != m or len(ys) != K or any(len(row) != P for row in ys) or not 1 <= P <= 8 or R < 2:
        return False
    st = FAM.steps(L, R, A)
    gamma = _statement(tr, field, d, b, f, Q, coset, widths, own, points, ys)
    later = {l: m + s - 1 for s, (l, _) in enumerate(st) if s}       # the root of layer l in op["roots"]
    rs = []
    for l in range(R):
        for e in op["polys"][l]:
            tr.append(be32(e % p))
        rs.append(tr.challenge(p))
        if l + 1 < R and l + 1 in later:
            tr.append(op["roots"][later[l + 1]])
    for e in op["final"]:
        tr.append(be32(e % p))
    indices = [FM.sample_index(tr, N // 2) for _ in range(Q)]
    if getattr(tr, "pow_ok", None) is False:
        return False
    every = ([v for z in points for v in z] + [y for row in ys for y in row] + [e for g in op["polys"] for e in g] + list(op["final"])
             + [v for vs in op["values"] for v in vs])
    if any(not 0 <= v < p for v in every) or list(op["roots"][:m]) != list(own) or len(op["roots"]) != m + len(st) - 1:
        return False
    alpha = pow(gamma, P, p)
    claim = sum(pow(gamma, c * P + q, p) * ys[c][q] for c in range(K) for q in range(P)) % p
    for l in range(R):
        g = op["polys"][l]
        if (g[0] + g[1]) % p != claim:
            return False
        claim = ML.interpolate3(g, rs[l], p)
    end = 0
    for q, z in enumerate(points):
        Aq = pow(gamma, q, p)
        for l in range(R):
            Aq = Aq * ML.eq1(rs[l], z[d - 1 - l], p) % p
        end += Aq * sum(t * e for t, e in zip(op["final"], ML.eq_table(z[:f], p)))
    if end % p != claim:
        return False
    iota = pow(w, N // 4, p)
    per_v, per_p = K + len(st) - 1, m + len(st) - 1          # quads and paths of one query
    if len(op["values"]) != Q * per_v or len(op["paths"]) != Q * per_p:
        return False
    for q, i in enumerate(indices):
        vq, pq = op["values"][q * per_v:(q + 1) * per_v], op["paths"][q * per_p:(q + 1) * per_p]
        for s, (l, sides) in enumerate(st):
            part = (N >> l) // sides
            j = i % part
            if s == 0:
                col = 0
                for t, wd in enumerate(widths):
                    quads = vq[col:col + wd]
                    if any(len(x) != 4 for x in quads) or len(pq[t]) != L - 2 or not verify_leaf(own[t], j, quads, pq[t], hasher):
                        return False
                    col += wd
                vals = [sum(pow(alpha, c, p) * vq[c][sd] for c in range(K)) % p for sd in range(4)]
            else:
                vals, pt = vq[K + s - 1], pq[m + s - 1]
                if len(vals) != sides or len(pt) != L - l - (sides.bit_length() - 1) or not FAM.verify_leaf(op["roots"][m + s - 1], j, vals, pt, hasher):
                    return False
            x = pow(coset, 1 << l, p) * pow(w, j << l, p) % p
            if sides == 4:
                u0, u1 = FAM.fold2(vals[0], vals[2], rs[l], x, p), FAM.fold2(vals[1], vals[3], rs[l], iota * x % p, p)
                v, ln = FAM.fold2(u0, u1, rs[l + 1], x * x % p, p), l + 2
            else:
                v, ln = FAM.fold2(vals[0], vals[1], rs[l], x, p), l + 1
            if ln < R:
                npart = (N >> ln) // st[s + 1][1]
                want = vq[K + s][j // npart]
            else:
                x2 = pow(coset, 1 << R, p) * pow(w, j << R, p) % p
                want = sum(e * pow(x2, n, p) for n, e in enumerate(op["final"])) % p
            if v != want:
                return False
    return True


def mont(zk, field, ints):
    """canonical ints -> (n, 4) Montgomery limbs, the C ABI's elements"""
    canon = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), np.uint64).reshape(-1, 4).copy()
    out = np.zeros_like(canon)
    assert zk.lib().zk_vec_from_canonical(field, canon.ctypes.data_as(zk._lib.u64p), canon.shape[0], out.ctypes.data_as(zk._lib.u64p)) == 0
    return out


def flat(zk, op):
    """the opening in the C ABI's layout: points (P, d, 4), ys (K, P, 4), gamma (4,), polys (R, 3, 4), own_roots (m, 32), roots (m + steps - 1,
    32), final (2^f, 4), challenges (R, 4), indices (Q,), values (Q, per, 4) and paths (bytes), per query step 0 first"""
    field, d, R, Q, P = op["field"], op["d"], op["d"] - op["f"], op["Q"], len(op["points"])
    mt = lambda ints: mont(zk, field, ints)
    return {
        "points": mt([v for z in op["points"] for v in z]).reshape(P, d, 4),
        "ys": mt([y for row in op["ys"] for y in row]).reshape(len(op["ys"]), P, 4),
        "gamma": mt([op["gamma"]])[0],
        "polys": mt([e for g in op["polys"] for e in g]).reshape(R, 3, 4),
        "own_roots": np.frombuffer(b"".join(op["own_roots"]), np.uint8).reshape(-1, 32).copy(),
        "roots": np.frombuffer(b"".join(op["roots"]), np.uint8).reshape(-1, 32).copy(),
        "final": mt(op["final"]),
        "challenges": mt(op["challenges"]),
        "indices": np.array(op["indices"], np.uint64),
        "values": mt([v for vs in op["values"] for v in vs]).reshape(Q, -1, 4),
        "paths": np.frombuffer(b"".join(b"".join(pt) for pt in op["paths"]), np.uint8).copy(),
    }


def pow_transcript(d, f, bits, nonce=None, prefix=b""):
    """a transcript with the proof-of-work step in front of the first index: sample number 1 (gamma) + R (the rounds)"""
    tr = GR.PowTranscript(bits, 1 + (d - f), nonce)
    tr.append(prefix)
    return tr
