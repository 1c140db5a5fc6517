"""Python model of the FRI low-degree proof (helper of tests/test_fri_cpu.py and test_gpu_fri.py).  The definition is the one of
include/zkmle.h "FRI low-degree proof":

  layer 0        f_0[k] = f(c w^k), k < N = 2^(d + b), w = w_N;   layer l: N >> l entries on {c_l w_l^k}, c_l = c^(2^l), w_l = w^(2^l)
  fold           f_{l+1}[k] = (f_l[k] + f_l[k + h]) / 2 + beta_l (f_l[k] - f_l[k + h]) / (2 c_l w_l^k),  h = N_l / 2
  commitments    root_l of layer l < R = d - f (tests/_merkle_model.py); layer R leaves as its m = 2^f low coefficients
  transcript     48-byte header, root_0, (beta_l, root_{l+1})*, the m coefficients, Q indices mod N / 2

Everything is Python integers on tests/_ntt_model.py and tests/_merkle_model.py; nothing here knows how the library works.  A proof is a
dict of ints and bytes; `flat` lays it out as the C ABI does."""
import numpy as np

import _merkle_model as MM
import _ntt_model as NM
from oracle import pymodel as M


def be32(v):
    return int(v).to_bytes(32, "big")


def fold(field, table, beta, coset=1):
    """one fold of a table of len >= 2 on {coset w_len^k}"""
    p, n = NM.MODULUS[field], len(table)
    h = n // 2
    w = NM.root_of_unity(field, n.bit_length() - 1)
    inv2 = pow(2, p - 2, p)
    out, x = [], coset % p
    for k in range(h):
        a, b = table[k], table[k + h]
        out.append(((a + b) * inv2 + beta * (a - b) * pow(2 * x, -1, p)) % p)
        x = x * w % p
    return out


def extend(field, coeffs, log_blowup, coset=1):
    """zk_uni_low_degree_extend: the evaluations of the coefficient table at coset w^k, k < len << log_blowup"""
    return NM.ntt(field, list(coeffs) + [0] * ((len(coeffs) << log_blowup) - len(coeffs)), False, coset)


def sizes(d, b, f, Q):
    R, L = d - f, d + b
    return R, 1 << f, Q * R * 2, Q * 32 * sum(2 * (L - l) for l in range(R))


def header(d, b, f, Q, coset):
    return b"".join(int(v).to_bytes(4, "big") for v in (d, b, f, Q)) + be32(coset)


def sample_index(tr, N):
    return int.from_bytes(tr.sample(), "little") % (N // 2)


def prove_codeword(field, codeword, b, f, Q, coset=1, tr=None, hasher=M.keccak256):
    """-> the proof as a dict; `tr` (an oracle/pymodel.py Transcript) is advanced"""
    p, N = NM.MODULUS[field], len(codeword)
    L = N.bit_length() - 1
    d = L - b
    R = d - f
    assert 1 <= b <= 8 and 0 <= f < d and 1 <= Q <= 4096 and coset % p
    tr = M.Transcript() if tr is None else tr
    tr.append(header(d, b, f, Q, coset))
    layers, trees, roots, betas = [list(codeword)], [], [], []
    c = coset % p
    for l in range(R):
        lv = MM.levels_of([be32(v) for v in layers[l]], hasher)
        trees.append(lv)
        roots.append(lv[-1][0])
        tr.append(roots[l])
        betas.append(tr.challenge(p))
        layers.append(fold(field, layers[l], betas[l], c))
        c = c * c % p
    final = NM.ntt(field, layers[R], True, c)[:1 << f]
    for hj in final:
        tr.append(be32(hj))
    indices = [sample_index(tr, N) for _ in range(Q)]
    values, paths = [], []
    for i in indices:
        for l in range(R):
            h = (N >> l) // 2
            j = i % h
            values.append((layers[l][j], layers[l][j + h]))
            paths.append((MM.path_of(trees[l], j), MM.path_of(trees[l], j + h)))
    return {"field": field, "d": d, "b": b, "f": f, "Q": Q, "coset": coset % p, "roots": roots, "final": final, "betas": betas,
            "indices": indices, "values": values, "paths": paths, "layers": layers}


def prove(field, coeffs, b, f, Q, coset=1, tr=None, hasher=M.keccak256):
    return prove_codeword(field, extend(field, coeffs, b, coset), b, f, Q, coset, tr, hasher)


def verify(pr, tr=None, hasher=M.keccak256):
    field, d, b, f, Q, coset = (pr[k] for k in ("field", "d", "b", "f", "Q", "coset"))
    p, L, R = NM.MODULUS[field], d + b, d - f
    N = 1 << L
    w = NM.root_of_unity(field, L)
    tr = M.Transcript() if tr is None else tr
    tr.append(header(d, b, f, Q, coset))
    tr.append(pr["roots"][0])
    betas = []
    for l in range(R):
        betas.append(tr.challenge(p))
        if l + 1 < R:
            tr.append(pr["roots"][l + 1])
    for hj in pr["final"]:
        tr.append(be32(hj))
    indices = [sample_index(tr, N) for _ in range(Q)]
    if any(not 0 <= v < p for v in pr["final"]) or any(not 0 <= v < p for pair in pr["values"] for v in pair):
        return False
    inv2 = pow(2, p - 2, p)
    for q, i in enumerate(indices):
        for l in range(R):
            h = (N >> l) // 2
            j = i % h
            (lo, hi), (plo, phi) = pr["values"][q * R + l], pr["paths"][q * R + l]
            if len(plo) != L - l or len(phi) != L - l:
                return False
            if not MM.verify_path(pr["roots"][l], j, be32(lo), plo, hasher) or not MM.verify_path(pr["roots"][l], j + h, be32(hi), phi, hasher):
                return False
            x = pow(coset, 1 << l, p) * pow(w, j << l, p) % p
            v = ((lo + hi) * inv2 + betas[l] * (lo - hi) * pow(2 * x, -1, p)) % p
            if l + 1 < R:
                want = pr["values"][q * R + l + 1][0 if j < h // 2 else 1]
            else:
                x2 = pow(coset, 1 << R, p) * pow(w, j << R, p) % p
                want = sum(hj * pow(x2, k, p) for k, hj in enumerate(pr["final"])) % p
            if v != want:
                return False
    return True


def flat(zk, pr):
    """the proof in the C ABI's layout: roots (R, 32) u8, final (m, 4) u64 Montgomery, betas (R, 4), indices (Q,) u64, values (Q, R, 2, 4),
    paths (path_bytes,) u8"""
    field, R, Q = pr["field"], pr["d"] - pr["f"], pr["Q"]

    def mont(ints):
        canon = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), np.uint64).reshape(-1, 4).copy()
        out = np.zeros_like(canon)
        assert zk.lib().zk_vec_from_canonical(field, canon.ctypes.data_as(zk._lib.u64p), canon.shape[0], out.ctypes.data_as(zk._lib.u64p)) == 0
        return out

    return {
        "roots": np.frombuffer(b"".join(pr["roots"]), np.uint8).reshape(R, 32).copy(),
        "final": mont(pr["final"]),
        "betas": mont(pr["betas"]),
        "indices": np.array(pr["indices"], np.uint64),
        "values": mont([v for pair in pr["values"] for v in pair]).reshape(Q, R, 2, 4),
        "paths": np.frombuffer(b"".join(b"".join(lo) + b"".join(hi) for lo, hi in pr["paths"]), np.uint8).copy(),
    }
