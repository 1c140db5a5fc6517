"""Integer model of the weighted-sum fold of K variables (csrc/mle_kernels.cuh foldk_seg_sums_kernel, foldk_seg_sums_split2_kernel,
foldk_split_kernel): out[j] = sum_i eq_i(r) in[j + i n], i < 2^K, accumulated as raw integer products and reduced once per part.
Helper of tests/test_foldk_shadow_cpu.py, tests/test_gpu_foldk_edges.py and tests/golden/make_foldk_hot_transcripts.py.

Table entries are STORED integers (x 2^256 mod p, what the limbs of a table hold); challenges are real values.  A part of T terms
accumulates acc = sum stored_i w_i with the canonical weights w_i = eq_i(r) 2^(29 L) mod p; raw_mont_reduce leaves
(acc + m p) / 2^(29 L), m = -acc / p mod 2^(29 L), which is below acc / 2^(29 L) + p; u_reduce_once subtracts p at most once, so the
stored result is canonical only if that value is below 2 p.  For canonical entries this is guaranteed when T p < 2^(29 L), that is for
T <= floor(2^(29 L) / p) terms (terms_max): the weights are residues, their integer sum can be anything up to T p."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import pymodel as M                                                       # noqa: E402

MODULUS = {0: M.P["bls12_381_fr"], 1: M.P["bls12_381_fq"], 2: M.P["bn254_fq"], 3: M.P["bn254_fr"]}
ULIMBS = {0: 9, 1: 14, 2: 9, 3: 9}                     # 29-bit limbs of the scan's form (csrc/ufield.cuh UParams::L)
STD_BITS = {0: 256, 1: 384, 2: 256, 3: 256}            # the stored form's radix


def radix(field):
    return 1 << (29 * ULIMBS[field])


def terms_max(field):
    """the most terms one raw_mont_reduce + u_reduce_once finishes for ANY canonical entries and weights"""
    return radix(field) // MODULUS[field]


def chunk_terms(field, terms):
    """terms per reduction of a part of `terms` (a power of two) inputs after the fix: the largest power of two within terms_max"""
    c = terms
    while c > terms_max(field):
        c //= 2
    return c


def stored(field, value):
    return value * (1 << STD_BITS[field]) % MODULUS[field]


def real(field, st):
    p = MODULUS[field]
    return st * pow(1 << STD_BITS[field], -1, p) % p


def eq_weights(field, rs):
    """eq_i(r) for i < 2^K, variable 0 = the most significant bit of i (real values)"""
    p = MODULUS[field]
    w = [1]
    for r in rs:
        w = [x * f % p for x in w for f in ((1 - r) % p, r)]
    return w


def scan_weights(field, rs):
    """the weights as the kernels keep them in LDS: eq_i(r) 2^(29 L) mod p, canonical"""
    p, R = MODULUS[field], radix(field)
    return [e * R % p for e in eq_weights(field, rs)]


def raw_mont_reduce(field, acc):
    """acc / 2^(29 L) mod p the way the limb-wise reduction leaves it: NOT reduced below p"""
    p, R = MODULUS[field], radix(field)
    m = (-acc * pow(p, -1, R)) % R
    v = acc + m * p
    assert v % R == 0
    return v // R


# ---- the forms: which inputs share one reduction ------------------------------------------------------------------------------------
def parts(form, K, per_reduction=None):
    """index ranges (of i < 2^K), one per Montgomery reduction.  form: "unsplit" (one lane per output), "split2" (two lanes, halves),
    "split8" (foldk_split_kernel, eight lanes).  per_reduction: a cap on the terms of one reduction (the fix); None = the whole lane part."""
    lanes = {"unsplit": 1, "split2": 2, "split8": 8}[form]
    per = (1 << K) // lanes
    step = per if per_reduction is None else min(per, per_reduction)
    return [range(a, a + step) for a in range(0, 1 << K, step)]


def lane_values(field, table, n, j, weights, part_list):
    """the value every part of output j holds before u_reduce_once"""
    return [raw_mont_reduce(field, sum(table[j + i * n] * weights[i] for i in rg)) for rg in part_list]


def over_range_lanes(field, table, K, rs, part_list):
    """the outputs j with a part at or above 2 p before the last conditional subtraction"""
    p = MODULUS[field]
    n = len(table) >> K
    w = scan_weights(field, rs)
    return [j for j in range(n) if any(v >= 2 * p for v in lane_values(field, table, n, j, w, part_list))]


def weight_sums(field, rs, part_list):
    """W of every part: the integer sum of its weights"""
    w = scan_weights(field, rs)
    return [sum(w[i] for i in rg) for rg in part_list]


def fold_exact(field, table, K, rs):
    """sum_i eq_i(r) in[j + i n] mod p on the stored integers (the fold is linear: the stored form of the folded value)"""
    p = MODULUS[field]
    n = len(table) >> K
    e = eq_weights(field, rs)
    return [sum(e[i] * table[j + i * n] for i in range(1 << K)) % p for j in range(n)]


def kernel_result(field, table, K, rs, part_list):
    """what the kernel stores with these parts: every part reduced once, the parts added in the field (exact for canonical parts)"""
    p = MODULUS[field]
    n = len(table) >> K
    w = scan_weights(field, rs)
    out = []
    for j in range(n):
        acc = None
        for v in lane_values(field, table, n, j, w, part_list):
            v = v - p if v >= p else v                                 # u_reduce_once
            if acc is None:
                acc = v
            else:                                                      # fe_add: one conditional subtraction
                acc += v
                acc = acc - p if acc >= p else acc
        out.append(acc)
    return out


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
def _splitmix(seed):
    x = seed & (2 ** 64 - 1)
    while True:
        x = (x + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        yield z ^ (z >> 31)


KINDS = ("all_pm1", "const_high", "mix", "near", "uniform")


def make_table(field, kind, length, seed=1):
    """stored integers.  all_pm1: every entry p - 1; const_high: one constant above 0.99 p; mix: {0, p - 1, a draw from
    [p - 2^200, p)}; near: every entry a draw from [p - 2^200, p); uniform: the control, uniform below p."""
    p = MODULUS[field]
    g = _splitmix(seed * 1000003 + length)

    def draw(bits):
        v = 0
        for _ in range((bits + 63) // 64):
            v = (v << 64) | next(g)
        return v & ((1 << bits) - 1)
    if kind == "all_pm1":
        return [p - 1] * length
    if kind == "const_high":
        return [p - (1 << 199) - 0xC0FFEE] * length
    if kind == "mix":
        out = []
        for _ in range(length):
            c = next(g) % 3
            out.append(0 if c == 0 else p - 1 if c == 1 else p - 1 - draw(200))
        return out
    if kind == "near":
        return [p - 1 - draw(200) for _ in range(length)]
    if kind == "uniform":
        return [draw(p.bit_length() + 64) % p for _ in range(length)]
    raise ValueError(kind)


# ---- the transcript of the rounds handle: what steers the challenges -------------------------------------------------------------------
def nonce_bytes(nonce):
    return b"foldk-hot-" + int(nonce).to_bytes(8, "little")


def first_challenges(field, table, K, nonce):
    """the first K challenges of a basic sumcheck on `table` (stored integers) whose transcript starts with nonce_bytes(nonce) where the
    reference's prover appends the table (prover.rs:38-58; oracle/pymodel.py sumcheck_basic_prove)"""
    p = MODULUS[field]
    n = len(table) >> K
    S = [real(field, sum(table[s * n:(s + 1) * n]) % p) for s in range(1 << K)]
    return challenges_from_sums(field, S, nonce)


def challenges_from_sums(field, S, nonce):
    p = MODULUS[field]
    nb = (p.bit_length() + 63) // 64 * 8
    t = M.Transcript()
    t.append(nonce_bytes(nonce))
    t.append(M.be32(sum(S) % p, nb))
    rs = []
    S = list(S)
    while len(S) > 1:
        h = len(S) // 2
        t.append(M.be32(sum(S[:h]) % p, nb) + M.be32(sum(S[h:]) % p, nb))
        r = t.challenge(p)
        rs.append(r)
        S = [(S[j] + r * (S[h + j] - S[j])) % p for j in range(h)]
    return rs


# ---- the cases of tests/test_gpu_foldk_edges.py ------------------------------------------------------------------------------------------
# (name, K, log2 of the input, m_next, form before the fix, needs K = 8 switched on).  Which kernel a shape takes is decided in
# fold_pass (csrc/zkmle_sumcheck.hip) and launch_foldk (csrc/fold_multi.h), kBlock = 256:
#   m_next = 0, k >= 4, output <= 2^13                        -> foldk_split_kernel (eight lanes per output)
#   m_next >= 1, k >= 5, output >> m_next >= 128, output < 2^18 -> foldk_seg_sums_split2_kernel
#   otherwise                                                  -> foldk_seg_sums_kernel (one lane per output)
SHAPES = (
    ("unsplit_k8", 8, 14, 1, "unsplit"),          # output 2^6, segments of 32 (< 128): one lane per output, 256 terms
    ("unsplit_k7", 7, 15, 2, "unsplit"),          # output 2^8, segments of 64: one lane per output, 128 terms
    ("split2_k8", 8, 17, 1, "split2"),            # output 2^9, segments of 256: two lanes per output, 128 terms each
    ("split2_k7", 7, 16, 1, "split2"),            # the default path's form: 64 terms each
    ("split2_k6", 6, 15, 1, "split2"),            # 32 terms each
    ("unsplit_k5", 5, 11, 1, "unsplit"),          # output 2^6: one lane per output, 32 terms
    ("split8_k8", 8, 14, 0, "split8"),            # output 2^6, no sums: eight lanes per output, 32 terms each
)
HOT = ("unsplit_k8", "unsplit_k7", "split2_k8")   # the forms with more than terms_max(0) = 70 terms per reduction before the fix
MIN_HOT_LANES = 8


def lanes_required(name, kind):
    """the over-range outputs a BLS12-381 Fr case must have in the model of its form before the fix.
    256 terms (W near 128 p +- 5 p against 2^261 = 70.66 p): every kind but the uniform control (6e-4 a lane there).
    128 terms (W of 73 .. 78 p at the committed nonces): the `near` tables only.  A constant table c folds to c whatever the
    challenges (the eq_i sum to 1), so its lanes hold c + k p below c W / 2^261 + p and reach 2 p only for W > 2^261 (1 + p / c),
    about 141.3 p, which 128 terms cannot give; and a third of a `mix` table is zero, which leaves its lanes the weight of some 85
    terms, 57 p +- 3 p.  Those cases assert W > 2^261, equality and canonicity."""
    if name not in HOT or kind == "uniform":
        return 0
    if name != "unsplit_k8" and kind != "near":
        return 0
    return MIN_HOT_LANES
