"""Python model of the evaluation opening of FRI-committed polynomials (helper of tests/test_fri_pcs_cpu.py and test_gpu_fri_pcs.py).  The
definition is the one of include/zkmle.h "FRI polynomial commitment":

  commitment   root of the Merkle tree (tests/_merkle_model.py) of the codeword f(c w^i), i < N = 2^(d + b) (tests/_fri_model.py extend)
  opening      y_j = f_j(z);  transcript: k as 4 big-endian bytes, the k roots, z, the y_j;  gamma = challenge;
               q[i] = (sum_j gamma^j (f_j[i] - y_j)) / (c w^i - z);  the FRI proof of q (tests/_fri_model.py prove_codeword) on the same
               transcript;  for every query i_q, side s and j: f_j[i_q + s N/2] and its path against root_j
  verifier     replays the transcript, runs the FRI verifier, checks the paths and, at every opened position,
               sum_j gamma^j (v_j - y_j) = (x - z) * (FRI's layer-0 value there)

Everything is Python integers; nothing here knows how the library works.  `open_at(.., false_ys=..)` opens with claimed values that are not
the evaluations: the quotient is computed as defined from the false claim and FRI is run honestly on it."""
import numpy as np

import _fri_model as FM
import _merkle_model as MM
import _ntt_model as NM
from oracle import pymodel as M

be32 = FM.be32


def in_domain(field, z, d, b, coset=1):
    p = NM.MODULUS[field]
    return pow(z * pow(coset, -1, p) % p, 1 << (d + b), p) == 1


def evaluate(field, coeffs, z):
    p, acc = NM.MODULUS[field], 0
    for a in reversed(coeffs):
        acc = (acc * z + a) % p
    return acc


def commit(field, coeffs, b, coset=1, hasher=M.keccak256):
    p = NM.MODULUS[field]
    cw = FM.extend(field, coeffs, b, coset)
    levels = MM.levels_of([be32(v) for v in cw], hasher)
    return {"field": field, "d": len(coeffs).bit_length() - 1, "b": b, "coset": coset % p, "coeffs": list(coeffs), "codeword": cw, "levels": levels,
            "root": levels[-1][0]}


def sizes(k, d, b, f, Q):
    return FM.sizes(d, b, f, Q) + (Q * 2 * k, Q * 2 * k * (d + b) * 32)


def challenge(tr, field, roots, z, ys):
    tr.append(len(roots).to_bytes(4, "big"))
    for r in roots:
        tr.append(r)
    tr.append(be32(z))
    for y in ys:
        tr.append(be32(y))
    return tr.challenge(NM.MODULUS[field])


def quotient(cms, z, ys, gamma):
    c0 = cms[0]
    field, L = c0["field"], c0["d"] + c0["b"]
    p, N, w = NM.MODULUS[field], 1 << L, NM.root_of_unity(field, L)
    out, x = [], c0["coset"]
    for i in range(N):
        num, g = 0, 1
        for cm, y in zip(cms, ys):
            num += g * (cm["codeword"][i] - y)
            g = g * gamma % p
        out.append(num % p * pow(x - z, -1, p) % p)
        x = x * w % p
    return out


def open_at(cms, z, f, Q, tr=None, false_ys=None, hasher=M.keccak256):
    """-> the opening as a dict; `false_ys` {j: value} replaces the claimed y_j"""
    c0 = cms[0]
    field, d, b, coset = (c0[k] for k in ("field", "d", "b", "coset"))
    assert all((cm["field"], cm["d"], cm["b"], cm["coset"]) == (field, d, b, coset) for cm in cms) and 1 <= len(cms) <= 64
    p = NM.MODULUS[field]
    z %= p
    assert not in_domain(field, z, d, b, coset)
    ys = [evaluate(field, cm["coeffs"], z) for cm in cms]
    for j, v in (false_ys or {}).items():
        ys[j] = v % p
    tr = M.Transcript() if tr is None else tr
    roots = [cm["root"] for cm in cms]
    gamma = challenge(tr, field, roots, z, ys)
    q = quotient(cms, z, ys, gamma)
    fri = FM.prove_codeword(field, q, b, f, Q, coset, tr, hasher)
    N = 1 << (d + b)
    opened, paths = [], []
    for i in fri["indices"]:
        for s in range(2):
            pos = i + s * (N // 2)
            for cm in cms:
                opened.append(cm["codeword"][pos])
                paths.append(MM.path_of(cm["levels"], pos))
    return {"field": field, "k": len(cms), "d": d, "b": b, "f": f, "Q": Q, "coset": coset, "roots_f": roots, "z": z, "ys": ys, "gamma": gamma,
            "quotient": q, "fri": fri, "opened": opened, "opened_paths": paths}


def verify(op, tr=None, hasher=M.keccak256):
    field, k, d, b, f, Q, coset, z = (op[n] for n in ("field", "k", "d", "b", "f", "Q", "coset", "z"))
    p, L = NM.MODULUS[field], d + b
    N, R = 1 << L, d - f
    tr = M.Transcript() if tr is None else tr
    gamma = challenge(tr, field, op["roots_f"], z, op["ys"])
    fri = dict(op["fri"], field=field, d=d, b=b, f=f, Q=Q, coset=coset)
    rest = M.Transcript()
    rest.buf = bytearray(tr.buf)
    if not FM.verify(fri, tr, hasher):
        return False
    # the indices the FRI verifier sampled: replay its transcript steps on the copy
    rest.append(FM.header(d, b, f, Q, coset))
    rest.append(fri["roots"][0])
    for l in range(R):
        rest.challenge(p)
        if l + 1 < R:
            rest.append(fri["roots"][l + 1])
    for hj in fri["final"]:
        rest.append(be32(hj))
    indices = [FM.sample_index(rest, N) for _ in range(Q)]
    if not 0 <= z < p or any(not 0 <= v < p for v in op["ys"]) or any(not 0 <= v < p for v in op["opened"]):
        return False
    if len(op["roots_f"]) != k or len(op["ys"]) != k or len(op["opened"]) != Q * 2 * k:
        return False
    w = NM.root_of_unity(field, L)
    for q, i in enumerate(indices):
        for s in range(2):
            pos = i + s * (N // 2)
            num, g = 0, 1
            for j in range(k):
                v, path = op["opened"][(q * 2 + s) * k + j], op["opened_paths"][(q * 2 + s) * k + j]
                if len(path) != L or not MM.verify_path(op["roots_f"][j], pos, be32(v), path, hasher):
                    return False
                num += g * (v - op["ys"][j])
                g = g * gamma % p
            x = coset * pow(w, pos, p) % p
            if num % p != (x - z) * fri["values"][q * R][s] % p:
                return False
    return True


def flat(zk, op):
    """the opening in the C ABI's layout: FM.flat's arrays of the FRI proof plus roots_f (k, 32) u8, z (4,) and ys (k, 4) u64 Montgomery,
    opened (Q, 2, k, 4) u64, opened_paths (Q 2 k L 32,) u8"""
    field, k, Q = op["field"], op["k"], op["Q"]

    def mont(ints):
        canon = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), np.uint64).reshape(-1, 4).copy()
        out = np.zeros_like(canon)
        assert zk.lib().zk_vec_from_canonical(field, canon.ctypes.data_as(zk._lib.u64p), canon.shape[0], out.ctypes.data_as(zk._lib.u64p)) == 0
        return out

    fl = FM.flat(zk, dict(op["fri"], field=field))
    fl.update({
        "roots_f": np.frombuffer(b"".join(op["roots_f"]), np.uint8).reshape(k, 32).copy(),
        "z": mont([op["z"]])[0],
        "ys": mont(op["ys"]),
        "opened": mont(op["opened"]).reshape(Q, 2, k, 4),
        "opened_paths": np.frombuffer(b"".join(b"".join(path) for path in op["opened_paths"]), np.uint8).copy(),
    })
    return fl
