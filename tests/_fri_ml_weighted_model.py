"""Python model of the opening of a FRI commitment against a caller's weight table (include/zkmle.h "FRI commitment opened against a weight
table"): the statement  sum_x T[x] W_0[x] = c  for the committed table T and any table W_0 of the same length.  It is the several-point
protocol of tests/_fri_ml_family_model.py with the points taken out: behind root_0 (and the arity line, where the schedule has one) the
transcript takes the 4 bytes "WGHT" and then c = g_0(0) + g_0(1), which comes out of round 0; the weight table is NOT absorbed (the caller
has bound it).  The verifier is handed c, the R challenges as the proof carries them and w_final = W_R, the caller's fold of W_0 by those
challenges; it refuses a proof whose replayed challenges differ from the carried ones.  Built on the family model's pieces; Python integers only."""
import _fri_ml_family_model as FF
import _fri_ml_model as ML
import _fri_model as FM
import _merkle_model as MM
import _ntt_model as NM
from oracle import pymodel as M

be32, be4 = FF.be32, FF.be4
SCHEDULE_TAG = {(1, False): b"", (2, False): be4(2), (2, True): be4(2) + be4(1)}


def fold_weights(field, W0, challenges):
    """W_R: W_0 folded over the last variable once per challenge"""
    W = list(W0)
    for r in challenges:
        W = ML.mle_fold_last(field, W, r)
    return W


def _statement(tr, field, d, b, f, Q, coset, a, grouped, root):
    tr.append(FM.header(d, b, f, Q, coset))
    if SCHEDULE_TAG[(a, grouped)]:
        tr.append(SCHEDULE_TAG[(a, grouped)])
    tr.append(root)
    tr.append(b"WGHT")


def open_weighted(cm, W0, f, Q, a=1, tr=None, hasher=M.keccak256, grind=None, false_c=None):
    """-> the opening as a dict; cm: a commitment of _fri_pcs_model.py, or of _fri_ml_grouped_model.py for the grouped schedule (a = 2);
    grind(tr) -> nonce runs the proof-of-work step where the protocol has it; false_c: the claim sent in place of the true one, round 0
    shifted to sum to it"""
    field, d, b, coset = (cm[n] for n in ("field", "d", "b", "coset"))
    grouped = cm.get("log_group", 0) == 2
    p, L, R = NM.MODULUS[field], d + b, d - f
    N = 1 << L
    assert len(W0) == 1 << d and 0 <= f < d and a in (1, 2) and (a == 2 or not grouped) and (a == 1 or R >= 2)
    tr = M.Transcript() if tr is None else tr
    _statement(tr, field, d, b, f, Q, coset, a, grouped, cm["root"])
    T, W = list(cm["coeffs"]), [w % p for w in W0]
    st = FF.steps(L, R, a)
    sides_at = dict(st)
    layers, trees, roots = {0: cm["codeword"]}, {0: cm["levels"]}, [cm["root"]]
    polys, rs, c, claim = [], [], coset % p, None
    for l in range(R):
        g = FF.round_g3(T, W, p)
        if l == 0:
            claim = (g[0] + g[1]) % p
            if false_c is not None:
                g[0] = (g[0] + false_c - claim) % p
                claim = false_c % p
            tr.append(be32(claim))
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
            trees[l + 1] = FF.levels_of(layers[l + 1], lg, hasher) if grouped else MM.levels_of([be32(e) for e in layers[l + 1]], hasher)
            roots.append(trees[l + 1][-1][0])
            tr.append(roots[-1])
    for e in T:
        tr.append(be32(e))
    nonce = grind(tr) if grind else 0
    indices = [FM.sample_index(tr, FF._index_mod(N, a)) for _ in range(Q)]
    values, paths = [], []
    for i in indices:
        for l, sides in st:
            part = (N >> l) // sides
            j = i % part
            values.append([layers[l][j + s * part] for s in range(sides)])
            paths.append([MM.path_of(trees[l], j)] if grouped else [MM.path_of(trees[l], j + s * part) for s in range(sides)])
    return {"field": field, "d": d, "b": b, "f": f, "Q": Q, "coset": coset % p, "a": a, "grouped": grouped, "root": cm["root"], "c": claim,
            "polys": polys, "roots": roots, "final": T, "challenges": rs, "w_final": W, "nonce": nonce, "indices": indices, "values": values,
            "paths": paths}


def verify_weighted(op, tr=None, hasher=M.keccak256, grind_check=None):
    """op carries c, challenges and w_final as the verifier is handed them; grind_check(tr, nonce) -> bool replays the proof-of-work step"""
    field, d, b, f, Q, coset, a, grouped = (op[n] for n in ("field", "d", "b", "f", "Q", "coset", "a", "grouped"))
    p, L, R = NM.MODULUS[field], d + b, d - f
    N = 1 << L
    w = NM.root_of_unity(field, L)
    tr = M.Transcript() if tr is None else tr
    if a not in (1, 2) or (grouped and a != 2) or (a == 2 and R < 2) or len(op["challenges"]) != R or len(op["w_final"]) != 1 << f:
        return False
    st = FF.steps(L, R, a)
    _statement(tr, field, d, b, f, Q, coset, a, grouped, op["root"])
    tr.append(be32(op["c"] % p))
    later = {l: s for s, (l, _) in enumerate(st) if s}
    rs = []
    for l in range(R):
        for e in op["polys"][l]:
            tr.append(be32(e % p))
        rs.append(tr.challenge(p))
        if l + 1 < R and l + 1 in later:
            tr.append(op["roots"][later[l + 1]])
    for e in op["final"]:
        tr.append(be32(e % p))
    pow_ok = grind_check(tr, op["nonce"]) if grind_check else True
    indices = [FM.sample_index(tr, FF._index_mod(N, a)) for _ in range(Q)]
    every = [op["c"]] + list(op["challenges"]) + list(op["w_final"]) + [e for g in op["polys"] for e in g] + list(op["final"]) + [v for vs in op["values"] for v in vs]
    if not pow_ok or any(not 0 <= v < p for v in every) or op["roots"][0] != op["root"] or len(op["roots"]) != len(st):
        return False
    if rs != list(op["challenges"]):                        # what makes a w_final computed from the carried challenges sound
        return False
    claim = op["c"]
    for l in range(R):
        g = op["polys"][l]
        if (g[0] + g[1]) % p != claim:
            return False
        claim = ML.interpolate3(g, rs[l], p)
    if sum(t * e for t, e in zip(op["final"], op["w_final"])) % p != claim:
        return False
    iota = pow(w, N // 4, p)
    per = len(st)
    if len(op["values"]) != Q * per or len(op["paths"]) != Q * per:
        return False
    for q, i in enumerate(indices):
        for s, (l, sides) in enumerate(st):
            part = (N >> l) // sides
            j = i % part
            vals, pths = op["values"][q * per + s], op["paths"][q * per + s]
            if len(vals) != sides or len(pths) != (1 if grouped else sides) or any(len(pt) != FF._path_len(L, l, sides, grouped) for pt in pths):
                return False
            if grouped:
                if not FF.verify_leaf(op["roots"][s], j, vals, pths[0], hasher):
                    return False
            elif not all(MM.verify_path(op["roots"][s], j + t * part, be32(vals[t]), pths[t], hasher) for t in range(sides)):
                return False
            x = pow(coset, 1 << l, p) * pow(w, j << l, p) % p
            if sides == 4:
                u0, u1 = FF.fold2(vals[0], vals[2], rs[l], x, p), FF.fold2(vals[1], vals[3], rs[l], iota * x % p, p)
                v, ln = FF.fold2(u0, u1, rs[l + 1], x * x % p, p), l + 2
            else:
                v, ln = FF.fold2(vals[0], vals[1], rs[l], x, p), l + 1
            if ln < R:
                npart = (N >> ln) // st[s + 1][1]
                want = op["values"][q * per + s + 1][j // npart]
            else:
                x2 = pow(coset, 1 << R, p) * pow(w, j << R, p) % p
                want = sum(e * pow(x2, n, p) for n, e in enumerate(op["final"])) % p
            if v != want:
                return False
    return True


def sizes(d, b, f, Q, a=1, grouped=False):
    """(nroots, nfinal, nvalues, path_bytes, nround): one table's sizes of the family model"""
    return FF.sizes(1, d, b, f, Q, a, grouped)


def flat(zk, op):
    """the opening in the C ABI's layout: c (4,), polys (R, 3, 4), roots (steps, 32), final (m, 4), challenges (R, 4), w_final (m, 4), indices
    (Q,), values (Q, per, 4), paths (bytes)"""
    field, R, Q = op["field"], op["d"] - op["f"], op["Q"]

    def mont(ints):
        return zk.from_ints(field, [int(v) for v in ints])

    return {
        "root": bytes(op["root"]),
        "c": mont([op["c"]])[0],
        "polys": mont([e for g in op["polys"] for e in g]).reshape(R, 3, 4),
        "roots": b"".join(op["roots"]),
        "final": mont(op["final"]),
        "challenges": mont(op["challenges"]),
        "w_final": mont(op["w_final"]),
        "indices": list(op["indices"]),
        "values": mont([v for vs in op["values"] for v in vs]).reshape(Q, -1, 4),
        "paths": b"".join(b"".join(pt) for pths in op["paths"] for pt in pths),
    }
