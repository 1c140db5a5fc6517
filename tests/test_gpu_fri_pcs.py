"""GPU: the evaluation opening of FRI-committed polynomials (csrc/fri_pcs.cuh, csrc/zkmle_fri_pcs.hip) over BLS12-381 Fr and BN254 Fr.
Everything compares byte for byte with the Python models (tests/_fri_pcs_model.py on _fri_model.py, _ntt_model.py, _merkle_model.py); no
tolerance anywhere.

  evaluation   zk_uni_evaluate_device against the model and the host zk_uni_evaluate for every 2^0 .. 2^14 (one run of 8 coefficients and
               its neighbours, one block, several blocks, and 2^13 / 2^14 on both sides of the second power table), z = 0, 1, p - 1, random;
               those launch one lane per run.  The later trips of the kernel's stride loop: with the grid capped at 1 and 2 workgroups
               (ZK_FRI_PCS_EVAL_BLOCKS) 2^11 .. 2^14 take 1, 2, 4, 8 and 1, 1, 2, 4 trips, on random, all p - 1, zero and delta tables
               (the delta at both ends of the second trip's first run pins the power that scales it); at the library's own cap 2^20 (512
               partials: the finishing kernel's second trip) and 2^21 (the main kernel's)
  commit       root = the model's = root_0 of zk_fri_prove; codeword = zk_uni_low_degree_extend
  quotient     every N = 4 .. 2^15 with every T of the batch inversion forced through ZK_FRI_PCS_BATCH (N < 256 T included), k = 1, 2, 5,
               coset or not, a constant polynomial, z = 0, z next to the domain, and the FRI fold witnesses as operands of uni_muladd
  open         the whole flat opening equals the model's and verifies; a caller's transcript; two points one after the other; lifetime"""
import ctypes as C
import functools
import os
import random
import re

import numpy as np
import pytest

import __graft_entry__ as G
import _fri_model as FM
import _fri_pcs_model as PM
import _fri_witness as W
import _ntt_model as NM
from oracle import pymodel as M
from test_gpu_fri import hasher_for, table_of, to_mont, zk  # noqa: F401  (zk: the module's fixture)

pytestmark = pytest.mark.gpu
FIELDS = (0, 3)
BATCHES = (1, 2, 4, 8, 16)
U64P = C.POINTER(C.c_uint64)


class forced_batch:
    """with forced_batch(T): the quotient's batch inversion takes T entries per lane (the library reads the variable per call)"""
    name = "ZK_FRI_PCS_BATCH"

    def __init__(self, t):
        self.t = t

    def __enter__(self):
        self.old = os.environ.get(self.name)
        if self.t is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = str(self.t)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


class eval_cap(forced_batch):
    """with eval_cap(c): the evaluation launches at most c workgroups (read per call); eval_cap(None): the library's own cap"""
    name = "ZK_FRI_PCS_EVAL_BLOCKS"


def elem(zk, field, v):
    return zk.from_ints(field, [v])[0]


def coset_of(field, d, b, with_coset):
    return random.Random(53 * d + b + field).randrange(2, NM.MODULUS[field]) if with_coset else 1


def same(got, want_ints, zk, field, what):
    want = to_mont(zk, field, want_ints)
    have = got.evaluated_values
    bad = np.nonzero((have != want).any(axis=1))[0]
    assert have.shape == want.shape and bad.size == 0, (what, bad[:8].tolist(), bad.size)


# ---- evaluation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", range(0, 15))
@pytest.mark.parametrize("field", FIELDS)
def test_evaluation_equals_the_model_and_the_host(zk, field, logn):
    p, n = NM.MODULUS[field], 1 << logn
    coeffs = NM.random_ints(field, n, 610 * field + logn)
    table, host = table_of(zk, field, coeffs), to_mont(zk, field, coeffs)
    zeros = table_of(zk, field, [0] * n)
    host_evaluate = zk.lib().zk_uni_evaluate
    host_evaluate.argtypes, host_evaluate.restype = [C.c_int, U64P, C.c_size_t, U64P, U64P], C.c_int
    for z in (0, 1, p - 1, random.Random(logn + field).randrange(2, p - 1)):
        zm = elem(zk, field, z)
        got = zk.ntt.evaluate_at(table, zm)
        assert zk.to_ints(field, got.reshape(1, -1)) == [PM.evaluate(field, coeffs, z)], (logn, z)
        ref = np.zeros(4, np.uint64)
        assert host_evaluate(field, host.ctypes.data_as(U64P), n, zm.ctypes.data_as(U64P), ref.ctypes.data_as(U64P)) == 0
        assert np.array_equal(got, ref), (logn, z)
        assert not zk.ntt.evaluate_at(zeros, zm).any()


# The lengths above launch one lane per run.  Past the grid cap a lane of pcs_eval_kernel takes a second run, which it scales by a power of z
# that only that trip reads, and adds to the sum it kept; past 256 partials a lane of pcs_eval_finish_kernel adds a second partial.
def eval_constants():
    """the kernel's own constants, read from csrc/fri_pcs.cuh: the trip counts asserted below follow the code, not a copy of its numbers"""
    src = open(os.path.join(G.PKG_DIR, "csrc", "fri_pcs.cuh")).read()
    block, run, cap = (int(re.search(r"constexpr \w+ %s = (\d+);" % name, src).group(1)) for name in ("kPcsBlock", "kPcsEvalRun", "kPcsEvalMaxBlocks"))
    return block, run, cap


def eval_trips(n, cap=None):
    """(trips of pcs_eval_kernel's stride loop, trips of pcs_eval_finish_kernel's loop, runs a stride covers) for n coefficients"""
    block, run, max_blocks = eval_constants()
    nruns = -(-n // run)
    blocks = min(-(-nruns // block), max_blocks if cap is None else max(1, min(cap, max_blocks)))
    return -(-nruns // (blocks * block)), -(-blocks // block), blocks * block


def host_evaluate(zk, field, host, zm):
    fn = zk.lib().zk_uni_evaluate
    fn.argtypes, fn.restype = [C.c_int, U64P, C.c_size_t, U64P, U64P], C.c_int
    ref = np.zeros(4, np.uint64)
    assert fn(field, host.ctypes.data_as(U64P), len(host), zm.ctypes.data_as(U64P), ref.ctypes.data_as(U64P)) == 0
    return ref


# cap -> log n -> the trips of the stride loop.  Cap 2 at 2^12 is exactly one full trip, and its second trip (2^13) starts at coefficient
# 4096, the first that reads the power table's `hi` half; cap 1's starts at 2048, inside `lo` (at 2^12 there is no `hi` at all).
CAPPED_TRIPS = {1: {11: 1, 12: 2, 13: 4, 14: 8}, 2: {11: 1, 12: 1, 13: 2, 14: 4}}


@pytest.mark.parametrize("logn", range(11, 15))
@pytest.mark.parametrize("cap", (1, 2))
@pytest.mark.parametrize("field", FIELDS)
def test_evaluation_on_the_later_trips_of_a_capped_grid(zk, field, cap, logn):
    p, n = NM.MODULUS[field], 1 << logn
    _, run, _ = eval_constants()
    trips, finish_trips, stride_runs = eval_trips(n, cap)
    assert (trips, finish_trips) == (CAPPED_TRIPS[cap][logn], 1)
    tables = {"random": NM.random_ints(field, n, 620 * field + 10 * logn + cap), "all p - 1": [p - 1] * n, "zero": [0] * n}
    if trips > 1:                                                        # a delta at both ends of the first run that a second trip takes
        s = stride_runs * run
        assert s == 2048 * cap and s + run <= n
        for name, at in (("delta first", s), ("delta last", s + run - 1)):
            tables[name] = [0] * at + [1] + [0] * (n - at - 1)
    zs = (0, 1, p - 1, random.Random(3 * logn + field + cap).randrange(2, p - 1))
    for name, coeffs in tables.items():
        table, host = table_of(zk, field, coeffs), to_mont(zk, field, coeffs)
        for z in zs:
            zm = elem(zk, field, z)
            with eval_cap(cap):
                got = zk.ntt.evaluate_at(table, zm)
            want = PM.evaluate(field, coeffs, z)
            if name.startswith("delta"):
                assert want == pow(z, coeffs.index(1), p)
            assert zk.to_ints(field, got.reshape(1, -1)) == [want], (name, cap, logn, z)
            assert np.array_equal(got, host_evaluate(zk, field, host, zm)), (name, cap, logn, z)
            with eval_cap(None):                                         # the uncapped launch, one run a lane, gives the same element
                assert np.array_equal(got, zk.ntt.evaluate_at(table, zm)), (name, cap, logn, z)


@pytest.mark.parametrize("logn", (20, 21))
@pytest.mark.parametrize("field", FIELDS)
def test_evaluation_at_the_default_cap_past_one_trip(zk, field, logn):
    """2^20 coefficients: the last length of one run a lane, 512 partials, so the finishing kernel's lanes add two each.  2^21: a lane of the
    main kernel takes two runs.  These are the kernels behind every y of an opening at d >= 20."""
    p, n = NM.MODULUS[field], 1 << logn
    assert eval_trips(n)[:2] == {20: (1, 2), 21: (2, 2)}[logn]
    coeffs = NM.random_ints(field, n, 630 * field + logn)
    host = to_mont(zk, field, coeffs)
    table = zk.MultilinearPolynomial.vector(field, host)
    z = random.Random(630 + logn + field).randrange(2, p - 1)
    zm = elem(zk, field, z)
    with eval_cap(None):
        got = zk.ntt.evaluate_at(table, zm)
    assert zk.to_ints(field, got.reshape(1, -1)) == [PM.evaluate(field, coeffs, z)], logn
    assert np.array_equal(got, host_evaluate(zk, field, host, zm)), logn


# ---- commit ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (5, 2), (9, 3), (12, 1)])
@pytest.mark.parametrize("field", FIELDS)
def test_commit_root_and_codeword(zk, field, shape):
    d, b = shape
    with_coset = (d + field) % 2 == 0
    coset = coset_of(field, d, b, with_coset)
    cm = elem(zk, field, coset) if with_coset else None
    coeffs = NM.random_ints(field, 1 << d, 77 * d + field)
    poly = table_of(zk, field, coeffs)
    model = PM.commit(field, coeffs, b, coset, hasher_for(zk, 1 << (d + b)))
    with zk.fri.commit(poly, b, cm) as c:
        assert c.root == model["root"]
        assert c.root == zk.fri.prove(poly, b, 0, 2, cm).roots[0].tobytes()
        assert np.array_equal(c.codeword().evaluated_values, zk.low_degree_extend(poly, b, cm).evaluated_values)
        same(c.codeword(), model["codeword"], zk, field, "codeword")


# ---- quotient --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_codewords(field, L, with_coset, k):
    """k coefficient tables of 2^(L - 1) entries (b = 1) and their model codewords; the last one is a constant polynomial when k > 1"""
    d = L - 1
    coset = coset_of(field, d, 1, with_coset)
    tables = [NM.random_ints(field, 1 << d, 9000 + 100 * L + j + field) for j in range(k)]
    if k > 1:
        tables[-1] = [tables[-1][0]] + [0] * ((1 << d) - 1)
    return coset, tables, [FM.extend(field, t, 1, coset) for t in tables]


def model_quotient(field, L, coset, codewords, z, ys, gamma):
    cms = [{"field": field, "d": L - 1, "b": 1, "coset": coset, "codeword": cw} for cw in codewords]
    return PM.quotient(cms, z, ys, gamma)


@pytest.mark.parametrize("L", range(2, 16))
@pytest.mark.parametrize("field", FIELDS)
def test_quotient_equals_the_model_for_every_batch(zk, field, L):
    """N = 2^L: every T where a lane's slots run past the table (N < 256 T), exactly fill it, and leave several blocks; 2^13 .. 2^15 are past
    the 4096-entry power table.  k, the coset and the point rotate with L; the default T (1 below 2^17) is the T = 1 case."""
    p, N = NM.MODULUS[field], 1 << L
    k = (1, 2, 5)[L % 3]
    with_coset = (L + field) % 2 == 0
    coset, tables, cws = model_codewords(field, L, with_coset, k)
    w = NM.root_of_unity(field, L)
    rng = random.Random(17 * L + field)
    # a random point, 0, and a point next to the domain: c w^i times 3 and 5 (non-roots), so that denominators differ by small factors
    zs = [rng.randrange(2, p), 0, coset * pow(w, rng.randrange(N), p) * (3 if L % 2 else 5) % p]
    z = zs[L % 3]
    assert not PM.in_domain(field, z, L - 1, 1, coset)
    gamma = rng.randrange(p)
    ys = [PM.evaluate(field, t, z) for t in tables]
    want = model_quotient(field, L, coset, cws, z, ys, gamma)
    if k > 1:                                                            # the constant polynomial: its numerator is zero everywhere
        assert all((v - ys[-1]) % p == 0 for v in cws[-1])
    polys = [table_of(zk, field, t) for t in tables]
    cm = elem(zk, field, coset) if with_coset else None
    cms = [zk.fri.commit(q, 1, cm) for q in polys]
    try:
        for T in BATCHES if L <= 13 else (1, 4, 16):
            with forced_batch(T):
                got = zk.fri.quotient(cms, elem(zk, field, z), to_mont(zk, field, ys), elem(zk, field, gamma))
            assert zk.fri.pcs_last_stats()["batch"] == T
            same(got, want, zk, field, (L, T))
        if k == 1:                                                       # a single constant polynomial: q = 0
            const = zk.fri.commit(table_of(zk, field, [7] + [0] * (N // 2 - 1)), 1, cm)
            got = zk.fri.quotient([const], elem(zk, field, z), to_mont(zk, field, [7]), elem(zk, field, gamma))
            assert not got.evaluated_values.any()
            const.free()
    finally:
        for c in cms:
            c.free()


@pytest.mark.parametrize("field", FIELDS)
def test_quotient_at_the_fold_witnesses(zk, field):
    """The quotient's numerator is f_0 + gamma f_1 through the fold's uni_muladd followed by fe_from_u_below_2p.  The committed operands
    (gamma, s, t) of tests/golden/fri_fold_witnesses.json make that sum land at or above 2 p, the path that takes the SECOND subtraction
    (about one lane in 2^28 of a uniform table).  They are planted as f_0[2 m] = s, f_1[2 m] = t (stored form) at four even positions --
    the n even positions of a codeword with b = 1 are free -- with the witness gamma as the opening's gamma."""
    p, d = NM.MODULUS[field], 9
    n, L = 1 << d, d + 1
    gamma_s, s, ts = W.load(field)
    w = NM.root_of_unity(field, L)
    lanes = [0, 255, 256, n - 1]
    evens = [NM.random_ints(field, n, 40 + j + field) for j in range(2)]
    for j, m in enumerate(lanes):
        evens[0][m], evens[1][m] = W.real(field, s), W.real(field, ts[j % len(ts)])
    tables = [NM.ntt(field, e, True) for e in evens]                      # the coefficients whose values on {w_n^m} = {w^(2 m)} are `evens`
    cws = [FM.extend(field, t, 1) for t in tables]
    assert all(cws[j][2 * m] == evens[j][m] for j in range(2) for m in lanes)
    z, gamma = 0x715, W.real(field, gamma_s)
    ys = [PM.evaluate(field, t, z) for t in tables]
    want = model_quotient(field, L, 1, cws, z, ys, gamma)
    cms = [zk.fri.commit(table_of(zk, field, t), 1) for t in tables]
    for T in (1, 8, 16):
        with forced_batch(T):
            got = zk.fri.quotient(cms, elem(zk, field, z), to_mont(zk, field, ys), elem(zk, field, gamma))
        same(got, want, zk, field, ("witness", T))
    for c in cms:
        c.free()


# ---- open ------------------------------------------------------------------------------------------------------------------------------
def assert_same_opening(zk, got, op):
    fl = PM.flat(zk, op)
    pr = got.proof
    for name, arr in (("ys", got.ys), ("roots", pr.roots), ("final", pr.final_coeffs), ("betas", pr.betas), ("indices", pr.query_indices),
                      ("values", pr.query_values), ("paths", pr.query_paths), ("opened", got.opened_values), ("opened_paths", got.opened_paths)):
        assert arr.shape == fl[name].shape and np.array_equal(arr, fl[name]), name


@functools.lru_cache(maxsize=None)
def open_case(field, d, b, k):
    with_coset = (d + field) % 2 == 1
    coset = coset_of(field, d, b, with_coset)
    tables = tuple(tuple(NM.random_ints(field, 1 << d, 5500 + 7 * d + j + field)) for j in range(k))
    return with_coset, coset, tables


@pytest.mark.parametrize("k", (1, 3))
@pytest.mark.parametrize("shape", [(1, 1, 0, 1), (5, 2, 1, 8), (10, 1, 2, 16), (13, 2, 0, 8)])
@pytest.mark.parametrize("field", FIELDS)
def test_opening_equals_the_model_byte_for_byte(zk, field, shape, k):
    d, b, f, Q = shape
    if d == 1:
        Q = 5                                                            # N / 2 = 2 positions: duplicate indices, answered twice
    p = NM.MODULUS[field]
    with_coset, coset, tables = open_case(field, d, b, k)
    hasher = hasher_for(zk, 1 << (d + b))
    z = random.Random(d + 3 * k + field).randrange(2, p)
    prior = b"absorbed before the opening"
    mt = M.Transcript()
    mt.append(prior)
    op = PM.open_at([PM.commit(field, list(t), b, coset, hasher) for t in tables], z, f, Q, mt, hasher=hasher)
    if d == 1:
        assert len(set(op["fri"]["indices"])) < Q
    cm = elem(zk, field, coset) if with_coset else None
    cms = [zk.fri.commit(table_of(zk, field, list(t)), b, cm) for t in tables]
    t = zk.Transcript()
    t.append(prior)
    got = zk.fri.open_at(cms, elem(zk, field, z), f, Q, transcript=t)
    assert_same_opening(zk, got, op)
    want = zk.Transcript()
    want.append(bytes(mt.buf))
    assert np.array_equal(t.export_state(), want.export_state())
    st = zk.fri.pcs_last_stats()
    assert st["polys"] == k and st["batch"] == 1 and st["ms_total"] > 0
    roots = [c.root for c in cms]
    tv = zk.Transcript()
    tv.append(prior)
    assert zk.fri.verify_opening(field, roots, elem(zk, field, z), got, d, b, f, Q, coset=cm, transcript=tv)
    assert np.array_equal(tv.export_state(), want.export_state())
    # bound to the prior content.  At d = 1 with k = 1 the quotient is a constant, which no gamma or beta changes: only the Q one-bit indices
    # bind the proof there, so the verdict without the prior content is the model's, whatever it is
    unbound = zk.fri.verify_opening(field, roots, elem(zk, field, z), got, d, b, f, Q, coset=cm)
    assert unbound == PM.verify(op, M.Transcript(), hasher) and (d == 1 or not unbound)
    for c in cms:
        c.free()


def test_two_openings_of_the_same_commitments_leave_no_state(zk):
    """two points one after the other give what each gives on commitments nobody has opened before (the model starts from nothing)"""
    field, d, b, f, Q = 0, 7, 2, 1, 6
    p = NM.MODULUS[field]
    tables = [NM.random_ints(field, 1 << d, 8800 + j) for j in range(2)]
    model = [PM.commit(field, t, b) for t in tables]
    cms = [zk.fri.commit(table_of(zk, field, t), b) for t in tables]
    first = {}
    for rnd in range(2):
        for z in (0x1234567, p - 2):
            got = zk.fri.open_at(cms, elem(zk, field, z), f, Q)
            assert_same_opening(zk, got, PM.open_at(model, z, f, Q))
            key = [got.ys.tobytes(), got.proof.query_paths.tobytes(), got.opened_paths.tobytes()]
            assert first.setdefault(z, key) == key
    with zk.fri.commit(table_of(zk, field, tables[0]), b) as fresh:      # a fresh commitment of the same table opens to the same bytes
        again = zk.fri.open_at([fresh, cms[1]], elem(zk, field, 0x1234567), f, Q)
        assert [again.ys.tobytes(), again.proof.query_paths.tobytes(), again.opened_paths.tobytes()] == first[0x1234567]
    for c in cms:
        c.free()


def test_commit_open_free_and_commit_again_leaves_the_pool_usable(zk):
    from zkmle_amd import _lib as L
    field, d, b = 3, 11, 2
    poly = zk.MultilinearPolynomial.random(field, 1 << d, 0xC0FE)
    z = elem(zk, field, 0xABCDEF)
    cm = zk.fri.commit(poly, b)
    first = zk.fri.open_at([cm], z, 2, 8)
    cm.free()
    L.check(zk.lib().zk_release_cached_memory())
    cm = zk.fri.commit(poly, b)
    second = zk.fri.open_at([cm], z, 2, 8)
    assert np.array_equal(first.opened_paths, second.opened_paths) and np.array_equal(first.proof.query_paths, second.proof.query_paths)
    assert zk.fri.verify_opening(field, [cm.root], z, second, d, b, 2, 8)
    assert np.array_equal(second.ys[0], zk.ntt.evaluate_at(poly, z))
    cm.free()
    L.check(zk.lib().zk_release_cached_memory())


# ---- the prover's precondition codes that need a commitment -------------------------------------------------------------------------------
def test_a_point_in_the_domain_and_mismatched_commitments_are_refused(zk):
    from zkmle_amd import _lib as L
    field, d, b = 0, 4, 1
    p = NM.MODULUS[field]
    coeffs = NM.random_ints(field, 1 << d, 31)
    c5 = elem(zk, field, 5)
    plain, shifted = zk.fri.commit(table_of(zk, field, coeffs), b), zk.fri.commit(table_of(zk, field, coeffs), b, c5)
    longer, wider = zk.fri.commit(table_of(zk, field, coeffs + coeffs), b), zk.fri.commit(table_of(zk, field, coeffs), b + 1)
    other = zk.fri.commit(table_of(zk, 3, NM.random_ints(3, 1 << d, 32)), b)
    w = NM.root_of_unity(field, d + b)

    def code(fn):
        with pytest.raises(L.ZkError) as e:
            fn()
        return e.value.code

    ys, g = to_mont(zk, field, [1, 2]), elem(zk, field, 9)
    for z in (1, w, pow(w, 7, p)):
        assert code(lambda: zk.fri.open_at([plain], elem(zk, field, z), 0, 4)) == L.ZK_E_ARG
        assert code(lambda: zk.fri.quotient([plain], elem(zk, field, z), ys, g)) == L.ZK_E_ARG
    assert code(lambda: zk.fri.open_at([shifted], elem(zk, field, 5 * w % p), 0, 4)) == L.ZK_E_ARG
    zk.fri.open_at([shifted], elem(zk, field, w), 0, 4)                  # w is outside the shifted domain
    for pair in ([plain, shifted], [plain, longer], [plain, wider], [plain, other]):
        assert code(lambda: zk.fri.open_at(pair, elem(zk, field, 77), 0, 4)) == L.ZK_E_LEN_MISMATCH
        assert code(lambda: zk.fri.quotient(pair, elem(zk, field, 77), ys, g)) == L.ZK_E_LEN_MISMATCH
    assert code(lambda: zk.fri.open_at([plain], elem(zk, field, 77), d, 4)) == L.ZK_E_ARG          # f >= d
    zk.fri.open_at([plain, plain], elem(zk, field, 77), 0, 4)            # a proof after each refused call; a commitment may be passed twice
    for c in (plain, shifted, longer, wider, other):
        c.free()
