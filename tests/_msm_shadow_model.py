"""An integer shadow of the Pippenger pipeline (msm_core in csrc/zkmle_kzg.hip): pure Python, no GPU, no ctypes.

When base i is [m_i] G with a small known integer m_i (0 = the point at infinity), every point the pipeline ever holds is a known
multiple of G, so the whole dataflow can be followed on integers mod r: k G = l G exactly when k = l (mod r), k G = -l G exactly when
k + l = 0 (mod r), and k G is infinity exactly when k = 0 (mod r).  Infinity is None here.

shadow(m, s, c, precomputed=False) follows msm_core with the window c (as the caller of zk_msm_g1 gives it) and returns
(result, Tally): the result as an integer mod r (None = infinity), and for every stage -- and for every FORM the launch rule picks
for it, one lane or a quad per addition, by the same work <= 2^13 rule as csrc/msm_reduce.hip -- the number of additions whose
operands are generic / equal / opposite / exactly one infinite / both infinite, the doublings of an infinite operand, and for the
quad forms the number of WAVES (16 consecutive quads running one operation together) whose quads fall into three or more classes.

What is exact, what is claimed.  From the bucket sums A[w][b] onward the dataflow is fixed by the values, so the tally is exact.
Before that the order of the entries inside a bucket is the sort's business, and for msm_bucket_sum_kernel (stage bucket_sum),
msm_partials_regroup_kernel (regroup) and msm_bucket_combine_kernel (combine) only facts that hold for EVERY order are counted:
  * the run structure (which sorted positions a bucket covers, hence how many runs of seg_len entries overlap it and by how much)
    depends on the bucket counts alone and is exact;
  * a bucket whose entries are all the same signed point x: in every run that overlaps it by L entries the lane adds infinity + x,
    then x + x (L >= 2), then k x + x; its partial sums are L x.  If x is infinity every addition there is infinity + infinity;
  * a bucket that lies inside ONE run and holds exactly {x, -x}: infinity + x' and x' + (-x') in either order;
  * a bucket that lies inside one run has ONE partial, the sum of its entries, whatever their order (nothing is claimed for the
    additions that made it unless one of the two cases above applies);
  * a bucket of exactly two entries {x, y} cut by a run boundary: each meets an empty accumulator in its own lane, and the partials are
    x and y in an unknown order.  The regroup kernel adds them to each other (the class is symmetric); the combine kernel adds
    infinity + one of them, then the two to each other (both finite: symmetric; otherwise only the additions common to both orders);
  * every other bucket: nothing is claimed for the three stages; its sum A[w][b] is still exact.
The partial lists of the uniform buckets are known, so their regroup chains and combine chains are exact."""
from collections import Counter, defaultdict

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
CLASSES = ("generic", "equal", "opposite", "one_inf", "inf_inf")
NONGENERIC = CLASSES[1:]
QUAD_LEVEL_WORK = 1 << 13                                    # kQuadLevelWork (csrc/msm_reduce.hip)
BIT_QUADS = 64                                               # kBitQuads (csrc/msm_bits.cuh)
GROUP = 16                                                   # kGroup (msm_core)


def norm(k):
    k %= R
    return k if k else None


def padd(a, b):
    if a is None:
        return b
    if b is None:
        return a
    return norm(a + b)


def pdbl(a):
    return None if a is None else norm(2 * a)


def pneg(a):
    return None if a is None else R - a


def classify(a, b):
    if a is None or b is None:
        return "inf_inf" if a is None and b is None else "one_inf"
    if a == b:
        return "equal"
    return "opposite" if (a + b) % R == 0 else "generic"


class Tally:
    """adds[stage][class], dbls[stage], dbl_inf[stage]; the quad stages' names end in '/quad', and for them mixed_waves() counts the waves
    whose quads fall into three or more classes"""

    def __init__(self):
        self._n = {}                                         # stage -> counts by class index
        self.dbls = Counter()
        self.dbl_inf = Counter()
        self._waves = {}                                     # (stage, key) -> bit set of the classes seen
        self._merged = 0

    @property
    def adds(self):
        out = defaultdict(Counter)
        for st, row in self._n.items():
            out[st].update({c: k for c, k in zip(CLASSES, row) if k})
        return out

    def add(self, stage, a, b, wave=None):
        """count a + b in `stage` (and in the wave `wave` of a quad stage) -> the sum"""
        if a is None:
            cls, r = (4, None) if b is None else (3, b)
        elif b is None:
            cls, r = 3, a
        else:
            r = a + b
            if r >= R:
                r -= R
            cls = 1 if a == b else 0 if r else 2
            r = r or None
        row = self._n.get(stage)
        if row is None:
            row = self._n[stage] = [0] * len(CLASSES)
        row[cls] += 1
        if wave is not None:
            key = (stage, wave)
            self._waves[key] = self._waves.get(key, 0) | (1 << cls)
        return r

    def dbl(self, stage, a):
        self.dbls[stage] += 1
        if a is None:
            self.dbl_inf[stage] += 1
        return pdbl(a)

    def count(self, stage, cls, k=1):
        if k > 0:
            self._n.setdefault(stage, [0] * len(CLASSES))[CLASSES.index(cls)] += k

    def mixed_waves(self):
        out = Counter()
        for (stage, _), classes in self._waves.items():
            if bin(classes).count("1") >= 3:
                out[stage] += 1
        return out

    def merge(self, other):
        for st, row in other._n.items():
            mine = self._n.setdefault(st, [0] * len(CLASSES))
            for i, k in enumerate(row):
                mine[i] += k
        self.dbls.update(other.dbls)
        self.dbl_inf.update(other.dbl_inf)
        self._merged += 1
        for (st, key), classes in other._waves.items():
            self._waves[(st, (self._merged, key))] = classes
        return self

    def table(self):
        mixed, adds = self.mixed_waves(), self.adds
        lines = ["%-22s %9s %9s %9s %9s %9s %8s %6s" % (("stage",) + CLASSES + ("dbl(inf)", "mixed"))]
        for st in sorted(adds):
            lines.append("%-22s %9d %9d %9d %9d %9d %8d %6s" % ((st,) + tuple(adds[st][c] for c in CLASSES)
                                                               + (self.dbl_inf[st], mixed[st] if st.endswith("/quad") else "-")))
        return "\n".join(lines)


# ---- signed recoding (msm_digits_kernel, msmw_digits_hist_kernel) ------------------------------------------------------------------
def nwindows(c):
    return (256 + c - 1) // c


def signed_digits(s, c):
    """W = ceil(256 / c) digits, d_w in [-2^(c-1), 2^(c-1)) below the top window; the top window takes its bits plus the carry as they are"""
    assert 0 <= s < R
    nwin, out, carry = nwindows(c), [], 0
    for w in range(nwin):
        d = ((s >> (w * c)) & ((1 << c) - 1)) + carry
        if d >= (1 << (c - 1)) and w + 1 < nwin:
            d -= 1 << c
            carry = 1
        else:
            carry = 0
        out.append(d)
    return out


def from_digits(digits, c):
    return sum(d << (c * w) for w, d in enumerate(digits))


def pick_window(n):
    lg = n.bit_length() - 1
    if lg >= 19:
        return 16
    if lg >= 14:
        return 13
    return max(lg - 3, 4)


class _Pair(list):
    """the two partial sums of a two-entry bucket cut by a run boundary, in an unknown order"""


# ---- the stages -------------------------------------------------------------------------------------------------------------------
def _form(work):
    return "quad" if work <= QUAD_LEVEL_WORK else "lane"


def _bucket_stages(T, buckets, seg_len):
    """buckets: list (bucket id order) of entry lists (signed multiples, None = a base at infinity) -> A (list of sums)"""
    starts, pos = [], 0
    for e in buckets:
        starts.append(pos)
        pos += len(e)
    partials = []                                            # per bucket: list of partial sums, or None when their split is unknown
    for b, ent in enumerate(buckets):
        if not ent:
            partials.append([])
            continue
        lo, hi = starts[b], starts[b] + len(ent)
        overlaps = [min(hi, (r + 1) * seg_len) - max(lo, r * seg_len) for r in range(lo // seg_len, (hi - 1) // seg_len + 1)]
        uniform = all(x == ent[0] for x in ent)
        if uniform:
            x = ent[0]
            for ln in overlaps:
                acc = None
                for _ in range(ln):
                    acc = T.add("bucket_sum", acc, x)
            partials.append([norm(ln * x) if x is not None else None for ln in overlaps])
        elif len(overlaps) == 1:
            if len(ent) == 2 and ent[0] is not None and classify(ent[0], ent[1]) == "opposite":
                T.count("bucket_sum", "one_inf")
                T.count("bucket_sum", "opposite")
            s = None
            for x in ent:
                s = padd(s, x)
            partials.append([s])
        elif len(ent) == 2:                                  # cut by a run boundary: each entry meets an empty accumulator in its own lane
            T.add("bucket_sum", None, ent[0])
            T.add("bucket_sum", None, ent[1])
            partials.append(_Pair(ent))                      # in an unknown order: only symmetric facts are taken from it below
        else:
            partials.append(None)
    sums = []
    for ent in buckets:
        s = None
        for x in ent:
            s = padd(s, x)
        sums.append(s)
    nparts = [len(buckets[b]) and ((starts[b] + len(buckets[b]) - 1) // seg_len - starts[b] // seg_len + 1) for b in range(len(buckets))]
    while max(nparts, default=0) > GROUP:                    # heavy buckets: sums of up to 16 consecutive partials
        for b, ps in enumerate(partials):
            cnt = nparts[b]
            nparts[b] = (cnt + GROUP - 1) // GROUP
            if ps is None:
                continue
            assert len(ps) == cnt
            if isinstance(ps, _Pair):
                partials[b] = [T.add("regroup", ps[0], ps[1])]   # the class is the same in both orders
                continue
            out = []
            for g in range(0, cnt, GROUP):
                acc = ps[g]
                for x in ps[g + 1:g + GROUP]:
                    acc = T.add("regroup", acc, x)
                out.append(acc)
            partials[b] = out
    for b, ps in enumerate(partials):
        if ps is None:
            continue
        if isinstance(ps, _Pair):                            # infinity + one of them, then that one + the other
            fin = [x for x in ps if x is not None]
            if len(fin) == 2:
                T.count("combine", "one_inf")
                T.count("combine", classify(ps[0], ps[1]))
            else:
                T.count("combine", "one_inf" if fin else "inf_inf", 1 if fin else 2)     # (one infinite: the other addition depends on the order)
            continue
        acc = None
        for x in ps:
            acc = T.add("combine", acc, x)
        assert acc == sums[b]
    return sums


def _reduce_level(T, A, Rr, nwin, size, half, stage):
    """msm_reduce_level_kernel on nwin arrays of `size` slots: A' = A_lo + A_hi, R' = A_hi + 2 (R_lo + R_hi), in place"""
    work = nwin * half
    form = _form(2 * work)
    st = "%s/%s" % (stage, form)
    newA, newR = {}, {}
    for i in range(2 * work):
        second, j = i >= work, i % work
        w, b = divmod(j, half)
        base = w * size
        wave = (half, i // 16, second) if form == "quad" else None
        ahi = A[base + b + half]
        if not second:
            newA[base + b] = T.add(st, A[base + b], ahi, wave and wave + (0,))
        else:
            t = T.add(st, Rr[base + b], Rr[base + b + half], wave and wave + (0,))
            t = T.dbl(st, t)
            newR[base + b] = T.add(st, ahi, t, wave and wave + (2,))
    for k, v in newA.items():
        A[k] = v
    for k, v in newR.items():
        Rr[k] = v


def _tail_kernel(T, X, Y, narrays, mbits, first_half):
    """msm_weighted_tail_kernel: a workgroup of 128 quads per array, every level from first_half down in one launch"""
    st, nquads = "tail/quad", 128
    for a in range(narrays):
        base, half = a << mbits, first_half
        while half >= 1:
            nx, ny = {}, {}
            for item in range(2 * half):
                second = item >= half
                b = item - half if second else item
                wave = (a, half, item // nquads, (item % nquads) // 16, second)
                ahi = X[base + b + half]
                if not second:
                    nx[base + b] = T.add(st, X[base + b], ahi, wave + (0,))
                else:
                    t = T.add(st, Y[base + b], Y[base + b + half], wave + (0,))
                    t = T.dbl(st, t)
                    ny[base + b] = T.add(st, ahi, t, wave + (2,))
            for k, v in nx.items():
                X[k] = v
            for k, v in ny.items():
                Y[k] = v
            half >>= 1


def _bit_sums(T, X, narrays, mbits):
    """msm_bit_sums_kernel<true>: S[a][j] = the plain sum of the entries whose index has bit j set (j = mbits: all of them)"""
    st, S = "bit_sums/quad", []
    for a in range(narrays):
        base, row = a << mbits, []
        for j in range(mbits + 1):
            cnt = (1 << mbits) if j == mbits else (1 << (mbits - 1))
            v = [None] * BIT_QUADS
            for t in range(cnt):
                i = t if j == mbits else (((t >> j) << (j + 1)) | (1 << j) | (t & ((1 << j) - 1)))
                quad = t % BIT_QUADS
                v[quad] = T.add(st, v[quad], X[base + i], (a, j, "acc", t // BIT_QUADS, quad // 16))
            s = BIT_QUADS // 2
            while s >= 1:
                for quad in range(s):
                    v[quad] = T.add(st, v[quad], v[quad + s], (a, j, "tree", s, quad // 16))
                s >>= 1
            row.append(v[0])
        S.append(row)
    return S


def _bit_combine(T, S, narrays, mbits):
    """msm_bit_combine_kernel<3>: sum_j 2^j S_j by pairs of groups, G_g + 2^w G_(g + stride); one wave of 16 quads per array, quad g holds S_g
    (infinity from g = mbits on).  At every step the quads g = 0 mod 2 stride add what quad g + stride doubled and stored in that step:
    those additions are counted, also where both operands are padding.  (The other quads run the same instructions on stale LDS
    contents and drop the result: not counted.)"""
    st, out = "bit_combine/quad", []
    ng = 1
    while ng < mbits:
        ng <<= 1
    for a in range(narrays):
        v = [S[a][g] if g < mbits else None for g in range(16)]
        stride = w = 1
        while stride < ng:
            dv = list(v)
            for g in range(16):
                if (g & (2 * stride - 1)) == stride:
                    for _ in range(w):
                        dv[g] = T.dbl(st, dv[g])
            for g in range(16):
                if (g & (2 * stride - 1)) == 0:
                    v[g] = T.add(st, v[g], dv[g + stride], (a, stride))
            stride <<= 1
            w <<= 1
        out.append(v[0])
    return out


def _window_sums_two_stage(T, A, nwin, c, force_tail):
    cm1 = c - 1
    k = cm1 // 2
    hb = cm1 - k
    mbits = max(hb, k)
    L, H, size = 1 << k, 1 << hb, 1 << cm1
    B = dict(A)
    for lvl in range(mbits):
        hh = (1 << (hb - 1 - lvl)) if lvl < hb else 0
        lh = (1 << (k - 1 - lvl)) if lvl < k else 0
        work1, work2 = nwin * hh * L, nwin * H * lh
        if work1 + work2 == 0:
            continue
        form = _form(work1 + work2)
        st = "plain_level/" + form
        if form == "lane":                                   # the long levels: only the pairs with a finite operand are visited
            for arr, role in ((A, 1), (B, 2)):
                pairs = {}
                for idx in arr:
                    w, r = divmod(idx, size)
                    h, l = divmod(r, L)
                    if role == 1 and h < 2 * hh:
                        pairs[idx - hh * L if h >= hh else idx] = 1
                    elif role == 2 and l < 2 * lh:
                        pairs[idx - lh if l >= lh else idx] = 1
                step = hh * L if role == 1 else lh
                for base in pairs:
                    v = T.add(st, arr.get(base), arr.get(base + step))
                    arr.pop(base + step, None)
                    if v is None:
                        arr.pop(base, None)
                    else:
                        arr[base] = v
                T.count(st, "inf_inf", (work1 if role == 1 else work2) - len(pairs))
            continue
        na, nb_ = {}, {}
        for i in range(work1 + work2):
            wave = (lvl, i // 16, i >= work1)
            if i < work1:
                w, r = divmod(i, hh * L)
                base = w * size + r
                na[base] = T.add(st, A.get(base), A.get(base + hh * L), wave)
            else:
                w, r = divmod(i - work1, H * lh)
                h, l = divmod(r, lh)
                base = w * size + h * L + l
                nb_[base] = T.add(st, B.get(base), B.get(base + lh), wave)
        A.update(na)
        B.update(nb_)
    M = 1 << mbits
    X = [None] * (2 * nwin * M)
    for w in range(nwin):
        for i in range(L):
            X[w * M + i] = A.get(w * size + i)
        for i in range(H):
            X[(nwin + w) * M + i] = B.get(w * size + i * L)
    Y = [None] * len(X)
    if mbits <= 8 and not force_tail:
        S = _bit_sums(T, X, 2 * nwin, mbits)
        weighted = _bit_combine(T, S, 2 * nwin, mbits)
        total = [S[a][mbits] for a in range(2 * nwin)]
    else:
        half = 1 << (mbits - 1)
        while half > 64:
            _reduce_level(T, X, Y, 2 * nwin, M, half, "reduce_level")
            half >>= 1
        _tail_kernel(T, X, Y, 2 * nwin, mbits, half)
        weighted = [Y[a << mbits] for a in range(2 * nwin)]
        total = [X[a << mbits] for a in range(2 * nwin)]
    sums = []
    for w in range(nwin):                                    # host: S_w = 2^k sum_h h D[h] + (sum_l l C[l] + sum_l C[l])
        hi = weighted[nwin + w]
        for _ in range(k):
            hi = T.dbl("host_two_stage", hi)
        sums.append(T.add("host_two_stage", hi, T.add("host_two_stage", weighted[w], total[w])))
    return sums


def shadow(m, s, c, precomputed=False, force_tail=False):
    """m: the bases as multiples of G; s: canonical scalars; c: window bits (2 .. 24; 0 = automatic) -> (result mod r or None, Tally)"""
    n = len(s)
    assert len(m) == n and n >= 1
    if c == 0:
        c = pick_window(n)
    assert 2 <= c <= 24 and (not precomputed or c >= 9)
    nwin1, nb = nwindows(c), 1 << (c - 1)
    nwin = 1 if precomputed else nwin1
    T = Tally()
    buckets = defaultdict(list)                              # bucket id (w * 2^(c-1) + |digit| - 1) -> entries; the sorted order is by bucket id
    for i in range(n):
        for w, d in enumerate(signed_digits(s[i], c)):
            if d == 0:
                continue
            assert abs(d) <= nb and (d > 0 or w + 1 < nwin1)
            x = norm(m[i] << (c * w)) if precomputed else norm(m[i])
            buckets[(0 if precomputed else w) * nb + abs(d) - 1].append(pneg(x) if d < 0 else x)
    seg_len = max(32, (n * nwin1) >> 20)
    A = _bucket_stages(T, [buckets[b] for b in sorted(buckets)], seg_len)
    A = {b: v for b, v in zip(sorted(buckets), A) if v is not None}          # sparse: a missing slot is infinity
    if c >= 6:
        sums = _window_sums_two_stage(T, A, nwin, c, force_tail)
    else:
        A = [A.get(b) for b in range(nwin * nb)]
        Rr = [None] * len(A)
        half = 1 << (c - 2)
        while half >= 1:
            _reduce_level(T, A, Rr, nwin, nb, half, "reduce_level")
            half >>= 1
        sums = [T.add("window_sums", Rr[w * nb], A[w * nb]) for w in range(nwin)]
    if precomputed:
        return sums[0], T
    acc = None
    for w in range(nwin1 - 1, -1, -1):
        for _ in range(c):
            acc = T.dbl("host_horner", acc)
        acc = T.add("host_horner", acc, sums[w])
    return acc, T


def expected(m, s):
    return norm(sum(a * b for a, b in zip(m, s)))
