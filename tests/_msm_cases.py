"""Scenarios that steer the MSM's additions into equal, opposite and infinite operands (shared by tests/test_msm_shadow_cpu.py and
tests/test_gpu_msm_group_law.py).  Every base is a known multiple m_i of G (|m_i| <= 64, 0 = infinity; the precomputed scenario adds a few
[2^(c w)] G), every scalar is given by its signed digits, so that the digit kernels put chosen points into chosen buckets.

A scenario is a function of the window c and returns a list of Case(name, m, s, precompute): bases as multiples, canonical scalars,
and whether it is meant for the window-shifted copies (run before and after bases.precompute(c)).  n <= 2^12 throughout."""
from collections import namedtuple

import _msm_shadow_model as SM

R = SM.R
Case = namedtuple("Case", "name m s precompute")
MAX_SLOTS = 1 << 12
WINDOWS = (4, 9, 13, 18)                                     # the forms: halving quads; all-quad two-stage; lane + quad; tail


class Grid:
    """the buckets a scenario may fill: slot j < nslots <-> bucket b of every window.  Up to c = 13 that is every bucket; at c = 18
    (2^17 buckets, 2^12 terms) it is 16 rows h of all 256 columns l, the rows chosen so that every level of the reduction over h and
    of the weighted tail (pairs 256, 128, ... apart) finds both of its operands filled"""

    def __init__(self, c):
        self.c, self.nb, self.nwin = c, 1 << (c - 1), SM.nwindows(c)
        self.top_max = (R >> (c * (self.nwin - 1))) - 1      # a top digit up to here keeps the scalar below r
        self.nslots = min(self.nb, MAX_SLOTS)
        self.k = (c - 1) // 2 if c >= 6 else 0
        self.L = 1 << self.k

    def bucket(self, slot):
        if self.nb <= MAX_SLOTS:
            return slot
        hv, l = divmod(slot, self.L)
        H = self.nb // self.L
        return ((hv % 4) + (H // 4) * (hv // 4)) * self.L + l

    def digit(self, w, b, sign):
        """the digit that puts (sign * base) into bucket b of window w, or 0 where no digit does"""
        d = sign * (b + 1)
        if w == self.nwin - 1:
            return d if 0 < d <= self.top_max else 0
        return d if -self.nb <= d < self.nb else 0

    def scalar(self, digits, wins=None):
        """the scalar with these signed digits; where they sum to a negative number, a digit +1 above the windows in use makes it positive
        (one more entry, the base itself, in bucket 0 there)"""
        digits = list(digits)
        if SM.from_digits(digits, self.c) < 0:
            digits[self.nwin - 1 if wins is None else max(wins) + 1] += 1
        s = SM.from_digits(digits, self.c)
        assert 0 <= s < R and SM.signed_digits(s, self.c) == list(digits), (self.c, digits)
        return s


def _by_sign(c, name, sign_of, base_of, wins=None, precompute=False):
    """one term per slot: the base base_of(slot), and in window w the digit that puts sign_of(w, slot) * base into the slot's bucket"""
    g = Grid(c)
    m, s = [], []
    for slot in range(g.nslots):
        b = g.bucket(slot)
        base = base_of(slot)
        flip = b == g.nb - 1 and base != 0                   # magnitude 2^(c-1) exists as a negative digit only: negate the base instead
        digits = [g.digit(w, b, (-1 if flip else 1) * sign_of(w, slot)) if (wins is None or w in wins) else 0 for w in range(g.nwin)]
        m.append(-base if flip else base)
        s.append(g.scalar(digits, wins))
    return Case(name, m, s, precompute)


def uniform(c, wins=None, precompute=False):
    """one entry G per bucket: every bucket sum is the same point, every addition of every level is P + P"""
    return [_by_sign(c, "uniform", lambda w, j: 1, lambda j: 1, wins, precompute)]


def cancelling(c, wins=None, precompute=False):
    """G where bit t of the bucket's slot is clear, -G where it is set: opposite operands at the level that folds bit t, infinity plus
    infinity above it.  t = the top bit is the issue's 'cancelling halves'; the other t move the cancellation into the later levels
    and into the columns / rows of the two-stage form.  Once through negated bases, once through negative digits on G."""
    g = Grid(c)
    nbits = g.nslots.bit_length() - 1
    out = []
    for t in sorted({nbits - 1, nbits - 2, g.k, g.k - 1, 0} & set(range(nbits))):
        out.append(_by_sign(c, "cancel_bases_bit%d" % t, lambda w, j: 1, lambda j, t=t: -1 if (j >> t) & 1 else 1, wins, precompute))
        out.append(_by_sign(c, "cancel_digits_bit%d" % t, lambda w, j, t=t: -1 if (j >> t) & 1 else 1, lambda j: 1, wins, precompute))
    return out


def _kind(c, w, j):
    g = Grid(c)
    hv, l = divmod(j, g.L)
    return (l + 2 * hv + (l >> 2) + (hv >> 1) + w) % 5


def checkerboard(c, wins=None, precompute=False):
    """bucket by bucket empty, G, -G, G again or a distinct (3 + b mod 59) G: neighbouring quads of one wave take different cases"""
    out = []
    for v in range(3):
        def sign_of(w, j, v=v):
            kd = _kind(c, w + v, j) if v < 2 else (j + w) % 5
            return (0, 1, -1, 1, 1)[kd]
        base_of = (lambda j: 3 + j % 59 if j % 5 == 4 else 1) if v != 1 else (lambda j: 1)
        out.append(_by_sign(c, "checkerboard%d" % v, sign_of, base_of, wins, precompute))
    return out


def accumulation(c, wins=None, precompute=False):
    """-> two cases, without and with the heavy buckets (one heavy bucket sends EVERY bucket of the call through the regroup kernel)

    several entries per bucket: the multisets {P, P}, {P, -P}, {P, P, P}, {P, inf, P}, {P, P, -2P}, {inf, inf}, a run of two-entry buckets {Q, -Q},
    {Q, Q}, {Q, inf}, {inf, inf} behind odd-sized ones (every 16th is cut by a run boundary: its two partials meet in the combine kernel), a heavy bucket of 17 x 32 + 8 copies of G (more than 16 segments: equal
    partials in the regroup and in the combine) and a heavy bucket of 40 G and 40 -G.  Group g goes to bucket g mod nb in the
    windows w with w mod per = g div nb (per = 1 once there are enough buckets)."""
    g = Grid(c)
    groups = [[(19, 1)]]                                     # lists of (base, sign); a single entry first: the pairs below start at an odd position
    for i, shape in enumerate(("PP", "PN", "PPP", "PIP", "PPD", "II") * 2):
        p = 2 + i
        groups.append({"PP": [(p, 1), (p, 1)], "PN": [(p, 1), (-p, 1)] if i < 6 else [(p, 1), (p, -1)], "PPP": [(p, 1)] * 3,
                       "PIP": [(p, 1), (0, 1), (p, 1)], "PPD": [(p, 1), (p, 1), (2 * p, -1)], "II": [(0, 1), (0, -1)]}[shape])
    for i in range(85):                                      # pairs: run boundaries are 16 of them apart and so cut every one of the five kinds
        q = 20 + i % 40
        groups.append(([(q, 1), (-q, 1)], [(q, 1), (q, 1)], [(q, 1), (0, 1)], [(q, 1), (q, -1)], [(0, 1), (0, 1)])[i % 5])
    heavy = [[(1, 1)] * (17 * 32 + 8), [(1, 1)] * 20 + [(-1, -1)] * 20 + [(1, -1)] * 20 + [(-1, 1)] * 20]
    out = []
    for name, grps in (("accumulation", groups), ("accumulation_heavy", groups + heavy)):
        avail = min(g.nb - 1, 128)
        per = (len(grps) + avail - 1) // avail
        m, s = [], []
        for gi, grp in enumerate(grps):
            b, phase = gi % avail, gi // avail
            for base, sign in grp:
                digits = [g.digit(w, b, sign) if w % per == phase and (wins is None or w in wins) else 0 for w in range(g.nwin)]
                m.append(base)
                s.append(g.scalar(digits, wins))
        out.append(Case(name, m, s, precompute))
    return out


def vanishing(c, wins=None, precompute=False):
    """sum s_i m_i = 0 with non-zero window sums: s on G and r - s on G; only one window sum infinite; window sums that meet the Horner
    accumulator as an equal, an opposite and an infinite operand"""
    g = Grid(c)
    out = []
    s0 = 0x1234567890abcdef1234567890abcdef1234567890abcdef1234567890abcd % R
    out.append(Case("vanish_s_and_r_minus_s", [1, 1], [s0, R - s0], precompute))
    out.append(Case("vanish_neg_base", [5, -5, 7], [s0, s0, 0], precompute))
    one = [0] * g.nwin                                       # window 1 alone sums to infinity: d and -d on the same base there
    a, b2 = list(one), list(one)
    a[0], a[1], a[2] = 3, 2, 1
    b2[0], b2[1], b2[2] = 1, -2, 1
    out.append(Case("one_window_infinite", [1, 1], [g.scalar(a), g.scalar(b2)], precompute))
    # Horner: acc <- 2^c acc + S_w.  S_1 = -G and S_0 = -2^c G (digit -2^(c-1) on 2 G) meet as equal operands; with S_0 = +2^c G as opposite
    d1, d0, d2 = list(one), list(one), list(one)
    d1[1], d0[0] = -1, -g.nb
    d1[2] = d0[2] = d2[2] = 1                                # keeps the scalars positive; window 2 sums to G + 2 G - 3 G
    out.append(Case("horner_equal", [1, 2, -3], [g.scalar(d1), g.scalar(d0), g.scalar(d2)], precompute))
    out.append(Case("horner_opposite", [1, -2, 1], [g.scalar(d1), g.scalar(d0), g.scalar(d2)], precompute))
    return out


def weights(c, wins=None, precompute=False):
    """a few buckets whose weights are single bits, so that the sums by the bits of the weight S_j (and with them the operands of the
    combination S_j + 2 S_(j+1)) are chosen one by one: index 1 holds +-2 G, index 2 holds G, index 4 holds -+2 G, index 8 holds G,
    once along the columns (array C) and once along the rows (array D), the signs by the window.  For the one-array sums
    sum_b b A[b] + sum_b A[b] (window sums, host combination): 3 G at index 1 and -2 G at index 2 make the two opposite."""
    g = Grid(c)
    m, s = [], []
    for step in ((1, g.L) if c >= 6 else (1,)):
        for idx, base, signs in ((1, 2, (1, -1, 1, 1)), (2, 1, (1, 1, 0, 1)), (4, 2, (-1, 1, 0, 1)), (8, 1, (1, 1, 1, -1))):
            if idx * step + 1 >= g.nb:
                continue
            digits = [g.digit(w, idx * step, signs[w % 4]) if (wins is None or w in wins) else 0 for w in range(g.nwin)]
            m.append(base)
            s.append(g.scalar(digits, wins))
    out = [Case("weights", m, s, precompute)]
    digits3 = [g.digit(w, 1, 1) if (wins is None or w in wins) else 0 for w in range(g.nwin)]
    digits2 = [g.digit(w, 2, -1) if (wins is None or w in wins) else 0 for w in range(g.nwin)]
    out.append(Case("weights_opposite", [3, 2], [g.scalar(digits3, wins), g.scalar(digits2, wins)], precompute))
    out.append(Case("weights_equal", [1], [g.scalar(digits3, wins)], precompute))       # index 1 alone: sum_b b A[b] = sum_b A[b]
    return out


def precomputed_copies(c):
    """base multiples and digits chosen so that 2^(c w) m_i of different windows collide in the ONE bucket set of the window-shifted copies: the
    term (G, digit d in window v) and the term ([2^(c v)] G, digit +-d in window 0) put equal / opposite points into bucket |d| - 1"""
    g = Grid(c)
    m, s = [], []
    for i in range(48):
        v = 1 + i % 3
        d = 1 + i
        hi, lo = [0] * g.nwin, [0] * g.nwin
        hi[v] = d
        lo[0] = d if i % 4 < 2 else -d
        if lo[0] < 0:
            lo[v + 1] = 1                                    # keeps the scalar positive; lands in bucket 0 as [2^(c (v + 1)) 2^(c v)] G
        m += [1, 1 << (c * v)]
        s += [g.scalar(hi), g.scalar(lo)]
    return [Case("precomputed_copies", m, s, True)]


def scenarios(c, precomputed=False):
    """every case at window c; precomputed: the cases for the one bucket set of bases.precompute(c) (digits in window 0 only, so
    that the shifted copies do not spread the pattern, plus the collisions across windows)"""
    if precomputed:
        wins = (0,)
        return (uniform(c, wins, True) + cancelling(c, wins, True) + checkerboard(c, wins, True) + accumulation(c, wins, True)
                + weights(c, wins, True) + vanishing(c, None, True) + precomputed_copies(c))
    return uniform(c) + cancelling(c) + checkerboard(c) + accumulation(c) + weights(c) + vanishing(c)


# ---- digit edges ------------------------------------------------------------------------------------------------------------------
def edge_scalars(c):
    """scalars at the edges of the signed recoding for window c (all below r)"""
    nwin, half = SM.nwindows(c), 1 << (c - 1)
    out = []
    for d in (half - 1, half, half + 1):                     # that value in every c-bit field (the top ones dropped until it is below r)
        v = sum(d << (c * w) for w in range(nwin))
        while v >= R:
            nwin -= 1
            v = sum(d << (c * w) for w in range(nwin))
        out.append(v)
        nwin = SM.nwindows(c)
    out += [(1 << 254) - 1, R - 1, R - 2]
    for w in (1, 2, nwin // 2, nwin - 1):
        if 0 < c * w < 255 and (1 << (c * w)) < R:
            out += [1 << (c * w), (1 << (c * w)) - 1]
    if c == 2:
        out.append((0x6f << 248) | ((1 << 248) - 1))         # the top digit becomes exactly 2^(c-1) by a carry (top byte 0x6f)
        out.append(0x6f << 248 | (1 << 247))
    return sorted(set(out))
