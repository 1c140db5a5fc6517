"""Tables that put chosen operands in front of the multilinear FRI folds (csrc/fri_ml.cuh), as Python integers.  Helper of
tests/test_fri_ml_edges_cpu.py and tests/test_gpu_fri_ml_edges.py; nothing here knows how the library works.

Lane k < h = n / 2 of a fold of a length-n codeword on {c w_n^k} reads a = f[k] and b = f[k + h] and forms

    S = (a + b) / 2,   T = w^-k (a - b) - c (a + b),   g[k] = S + gamma T,   gamma = r / (2 c).

`unfold` inverts that: it gives the pair (a, b) whose lane sees a chosen S and T.  With S, T and gamma the real values of a committed witness
(tests/golden/fri_fold_witnesses.json, stored form: tests/_fri_witness.py) the lane's last step is one that needs the SECOND subtraction of
fe_from_u_below_2p.  A fold by 4 is the same fold on its first layer, h = 2 q: first-fold lane k < q is pair 0 of output lane k (entries k and
k + 2q, twiddle w^-k), first-fold lane k + q is pair 1 of output lane k (entries k + q and k + 3q, twiddle w^-(k + q)).

  plant_fold, plant_fold4   write the witnesses into chosen lanes of a table and return the challenge that makes gamma the witness's
  fold_target               a table whose fold is a given list: what a fold by 4 hands to its second stage
  structured_table          the nine tables of tests/test_gpu_fri_edges.py, T = 0 in every lane, stored S = stored T = p - 1 in every
                            lane, and for a fold by 4 a first fold with u0 = u1 and with u0 + u1 = p in every output lane
  cosets_of, challenges_of  the shifts none, an explicit 1, p - 1, 1 / 2, w_N, w_2N (w_4 for a fold by 4: c^2 = p - 1) and the challenges
                            0, 1, p - 1, 2 c, p - 2 c: gamma = 0, 1 and p - 1 among them"""
import functools
import random

import _fri_witness as W
import _ntt_model as NM
from test_gpu_fri_edges import structured_tables


def stored_operands(field, n, k, c, a, b):
    """-> (s, t): the halved sum and the operand T of lane k as the integers of their STORED form, what the kernel multiplies and adds"""
    p = NM.MODULUS[field]
    wk = pow(NM.root_of_unity(field, n.bit_length() - 1), -k, p)
    return W.stored(field, (a + b) * pow(2, -1, p)), W.stored(field, (wk * (a - b) - c * (a + b)) % p)


def _pair(p, c, wk, S, T):
    half = (T + 2 * c * S) * wk * pow(2, -1, p) % p
    return (S + half) % p, (S - half) % p


def unfold(field, n, k, c, S, T):
    """-> (a, b), the canonical entries k and k + n / 2 with a + b = 2 S and a - b = (T + 2 c S) w^k"""
    p = NM.MODULUS[field]
    return _pair(p, c, pow(NM.root_of_unity(field, n.bit_length() - 1), k, p), S % p, T % p)


def unfold_all(field, n, c, Ss, Ts):
    """the table whose lane k sees Ss[k] and Ts[k]"""
    p, h = NM.MODULUS[field], n // 2
    w, wk, out = NM.root_of_unity(field, n.bit_length() - 1), 1, [0] * n
    for k in range(h):
        out[k], out[k + h] = _pair(p, c, wk, Ss[k] % p, Ts[k] % p)
        wk = wk * w % p
    return out


# ---- the second subtraction ------------------------------------------------------------------------------------------------------------
def fold_lanes(h):
    """lanes 0, 255, 256 and the last, as far as a fold of h lanes has them"""
    return sorted(k for k in {0, 255, 256, h - 1} if k < h)


def fold4_lanes(q):
    """first-fold lanes of a fold by 4 of q output lanes: with q >= 512, output lanes 0, 255 and q - 1 get both pairs, 256 pair 0 alone"""
    return sorted(k for k in {0, 255, 256, q - 1, q, q + 255, 2 * q - 1} if k < 2 * q)


def fold_ts(field, lanes):
    """{lane: t}: the file's t's in turn, as tests/test_gpu_fri_edges.py witness_table takes them"""
    ts = W.load(field)[2]
    return {k: ts[j % len(ts)] for j, k in enumerate(sorted(set(lanes)))}


def fold4_ts(field, q, lanes):
    """{first-fold lane: t}: the file's t's in turn over the OUTPUT lanes, so that both pairs of an output lane carry the same t"""
    ts = W.load(field)[2]
    outs = sorted({k % q for k in lanes})
    return {k: ts[outs.index(k % q) % len(ts)] for k in lanes}


def witness_output(field, t):
    """s + gamma t mod p as a stored integer: what a lane planted with t leaves"""
    gamma, s, _ = W.load(field)
    return (s + W.real(field, gamma) * t) % NM.MODULUS[field]


def _plant(field, values, ts, c):
    n = len(values)
    gamma, s, _ = W.load(field)
    for k, t in ts.items():
        values[k], values[k + n // 2] = unfold(field, n, k, c, W.real(field, s), W.real(field, t))
    return 2 * c * W.real(field, gamma) % NM.MODULUS[field]


def plant_fold(field, values, lanes, c=1):
    """writes a witness into each lane of `lanes` (< len(values) / 2) -> r = 2 c gamma"""
    return _plant(field, values, fold_ts(field, lanes), c)


def plant_fold4(field, values, lanes, c=1):
    """the same on the lanes of the first fold (< len(values) / 2 = 2 q) of a fold by 4 -> r0 = 2 c gamma"""
    return _plant(field, values, fold4_ts(field, len(values) // 4, lanes), c)


# ---- a fold with a chosen result -------------------------------------------------------------------------------------------------------
def fold_target(field, n, c, r, wanted, seed):
    """a length-n table on {c w^k} whose fold by r is `wanted` (n / 2 entries): each lane has a random S and T = (wanted - S) / gamma.
    gamma = 0 keeps S alone, so there S = wanted and T is random."""
    p, h = NM.MODULUS[field], n // 2
    assert len(wanted) == h
    rng = random.Random(seed)
    gamma = r * pow(2 * c, -1, p) % p
    if gamma == 0:
        return unfold_all(field, n, c, wanted, [rng.randrange(p) for _ in range(h)])
    Ss = [rng.randrange(p) for _ in range(h)]
    ginv = pow(gamma, -1, p)
    return unfold_all(field, n, c, Ss, [(v - S) * ginv for v, S in zip(wanted, Ss)])


# ---- structured tables -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nine(field, logn):
    return tuple(structured_tables(field, logn))


FOLD4_ONLY = ("u0 == u1", "u0 + u1 == p")


def table_names(by4=False):
    return [name for name, _ in _nine(0, 1)] + ["t == 0", "stored s == t == p - 1"] + (list(FOLD4_ONLY) if by4 else [])


def structured_table(field, logn, name, c=1, r0=None):
    """one table by name, canonical values; do not change it (the nine are cached).  c: the coset the fold will use (1: none), which "t == 0"
    and "stored s == t == p - 1" are built for; r0: the first challenge of the fold by 4, which the two FOLD4_ONLY tables are built for"""
    p, n = NM.MODULUS[field], 1 << logn
    h = n // 2
    rng = random.Random(8700 + 16 * logn + field)
    if name == "t == 0":                                                                  # a - b = c (a + b) w^k
        return unfold_all(field, n, c, [rng.randrange(p) for _ in range(h)], [0] * h)
    if name == "stored s == t == p - 1":
        top = W.real(field, p - 1)
        return unfold_all(field, n, c, [top] * h, [top] * h)
    if name in FOLD4_ONLY:
        u = [rng.randrange(1, p) for _ in range(h // 2)]
        return fold_target(field, n, c, r0, u + (u if name == "u0 == u1" else [p - v for v in u]), 8600 + logn + field)
    return dict(_nine(field, logn))[name]


# ---- cosets and challenges -------------------------------------------------------------------------------------------------------------
def coset_names(by4=False):
    return ["none", "explicit 1", "p - 1", "1 / 2", "w_N", "w_2N"] + (["w_4"] if by4 else [])


def coset_of(field, logn, name):
    """-> the shift, None for "none": the library is then given no coset at all, and with "explicit 1" the element 1"""
    p = NM.MODULUS[field]
    return {"none": None, "explicit 1": 1, "p - 1": p - 1, "1 / 2": pow(2, -1, p), "w_N": NM.root_of_unity(field, logn),
            "w_2N": NM.root_of_unity(field, logn + 1), "w_4": NM.root_of_unity(field, 2)}[name]


def challenges_of(field, c):
    """r = 0, 1, p - 1, 2 c, p - 2 c: gamma = r / (2 c) = 0, 1 and p - 1 among them.  Always five, equal ones included (c = 1 / 2), so that
    two such lists rotate against each other in full.  The second challenge of a fold by 4: challenges_of(field, c^2)"""
    p = NM.MODULUS[field]
    return [0, 1, p - 1, 2 * c % p, (p - 2 * c) % p]
