"""GPU: the GKR round kernels (csrc/sumcheck_kernels.cuh round_evals_kernel, fold_round_evals_kernel and, through the provers, the
split and two-round forms) at structured operands.  The kernels sum raw products lazily (prod_accumulate / prod_carry every
kProdCarryEvery = 6 products / prodwide_reduce) over operands up to hi - lo + 4 p, and fold with ufold + fe_from_u_below_2p; uniform
tables exercise none of the extremes.  Everything is compared byte for byte with Python integers (oracle/pymodel.py round_evals and
partial_evaluate) or, for whole proofs, with the C oracle: folded tables, e(0) .. e(nfac), and the inputs left unchanged.

Operands (stored = the integer in the table's limbs, real = the field element it stands for):
  real_pm1     every entry the element p - 1
  stored_pm1   every entry the stored integer p - 1
  lo0_hi_max   lower half 0, upper half stored p - 1 (the largest hi - lo), and hi0_lo_max the reverse (the largest hi - lo + 4 p)
  zero_factor  one factor of the first product all zero, the rest stored p - 1
  mix / mix2   every entry one of {0, stored p - 1, a uniform draw}, two seeds
with `value` in 0, 1, p - 1 and a uniform draw; and operands found by search whose fold reaches 2 p before its reduction.  nprod = 2 and 3 (3 products of 2 factors put the carry after six products in the
middle of an index; the API refuses nprod = 1 with ZK_E_NEED_TWO), nfac = 2, and nfac = 3 for the branch without lazy products."""
import random

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import oracle as O
from oracle import pymodel as M

import _foldk_shadow_model as FM

pytestmark = pytest.mark.gpu
KINDS = ("real_pm1", "stored_pm1", "lo0_hi_max", "hi0_lo_max", "zero_factor", "mix", "mix2")


def package():
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    return zk


def to_limbs(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint64).reshape(-1, 4).copy()


def to_ints(arr):
    return [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(arr, np.uint64).reshape(-1, 4)]


def make_tables(field, kind, nprod, nfac, n, seed):
    """tables[prod][fac] of n stored integers"""
    p = FM.MODULUS[field]
    rng = random.Random(1000 * seed + n + 7 * nprod + nfac + (500000 if kind == "mix2" else 0))
    h = n // 2

    def one(pr, f):
        if kind == "real_pm1":
            return [FM.stored(field, p - 1)] * n
        if kind == "stored_pm1":
            return [p - 1] * n
        if kind == "lo0_hi_max":
            return [0] * h + [p - 1] * h
        if kind == "hi0_lo_max":
            return [p - 1] * h + [0] * h
        if kind == "zero_factor":
            return [0] * n if (pr, f) == (0, nfac - 1) else [p - 1] * n
        return [rng.choice((0, p - 1, rng.randrange(p))) for _ in range(n)]
    return [[one(pr, f) for f in range(nfac)] for pr in range(nprod)]


def values_for(field, seed):
    p = FM.MODULUS[field]
    return [0, 1, p - 1, random.Random(seed).randrange(p)]


def check_round(zk, field, kind, nprod, nfac, logn, value, fold, st=None):
    from _sharded_protocol_model import HipSumShard
    p = FM.MODULUS[field]
    n = 1 << logn
    if st is None:
        st = make_tables(field, kind, nprod, nfac, n, logn)
    real = [[[FM.real(field, v) for v in t] for t in prod] for prod in st]
    limbs = [[to_limbs(t) for t in prod] for prod in st]
    shard = HipSumShard(field, [[zk.MultilinearPolynomial(field, a) for a in prod] for prod in limbs])
    tag = (field, kind, nprod, nfac, logn, value, fold)
    if fold:
        folded, ev = shard.fold_round_evals(zk.from_ints(field, [value])[0])
        want_tabs = [[M.partial_evaluate(t, 0, value, p) for t in prod] for prod in real]
        got = folded.download()
        for pr in range(nprod):
            for f in range(nfac):
                assert to_ints(got[pr][f]) == [FM.stored(field, v) for v in want_tabs[pr][f]], tag + (pr, f)
        want_ev = M.round_evals(want_tabs, p)
    else:
        ev = shard.round_evals()
        want_ev = M.round_evals(real, p)
    assert to_ints(ev) == [FM.stored(field, v) for v in want_ev], tag
    for pr in range(nprod):                                              # the inputs are unchanged
        for f in range(nfac):
            assert np.array_equal(shard.tables[pr][f].evaluated_values, limbs[pr][f]), tag


def combos(logn):
    """every kind with nprod 2 and 3 up to 2^9 entries; above, two kinds and one nprod per length, rotating"""
    if logn <= 9:
        return [(k, nprod) for k in KINDS for nprod in (2, 3)]
    return [(KINDS[(logn + i) % len(KINDS)], 2 + (logn + i) % 2) for i in range(2)]


@pytest.mark.parametrize("logn", range(2, 16))
@pytest.mark.parametrize("field", [0, 3])
def test_round_evals_at_structured_operands(field, logn):
    zk = package()
    for kind, nprod in combos(logn):
        check_round(zk, field, kind, nprod, 2, logn, None, False)


@pytest.mark.parametrize("logn", range(3, 16))
@pytest.mark.parametrize("field", [0, 3])
def test_fold_round_evals_at_structured_operands(field, logn):
    zk = package()
    vals = values_for(field, logn)
    for i, (kind, nprod) in enumerate(combos(logn)):
        for value in (vals if logn <= 6 else [vals[(i + logn) % 4]]):
            check_round(zk, field, kind, nprod, 2, logn, value, True)


@pytest.mark.parametrize("logn", [3, 6, 11])
@pytest.mark.parametrize("field", [0, 3])
def test_three_factor_products_at_structured_operands(field, logn):
    zk = package()
    p = FM.MODULUS[field]
    for kind in ("stored_pm1", "hi0_lo_max", "mix"):
        check_round(zk, field, kind, 2, 3, logn, None, False)
        check_round(zk, field, kind, 2, 3, logn, p - 1, True)


@pytest.mark.parametrize("logn", [10, 14])
@pytest.mark.parametrize("field", [0, 3])
def test_fold_whose_value_reaches_2p_before_the_reduction(field, logn):
    """The committed operands (r, a = stored p - 1, b) of tests/golden/gkr_ufold_witnesses.json (tools/find_fold_witness.hip, ufold mode;
    replayed on the host by tests/test_fri_arith_cpu.py) leave ufold at or above 2 p: fe_from_u_below_2p takes its second subtraction for
    the stored output, and the un-reduced pair feeds the lazy products of the evaluations.  Planted in output lanes 0, 255, 256 and the
    last one of every table of a fused pass, which uniform tables reach about once in 2^31 lanes."""
    import _fri_witness as W
    zk = package()
    r, a, bs = W.load(field, "gkr_ufold_witnesses.json")
    n = 1 << logn
    for nprod in (2, 3):
        st = make_tables(field, "mix", nprod, 2, n, 90 + logn)
        k = 0
        for prod in st:
            for t in prod:
                for lane in (0, 255, 256, n // 2 - 1):
                    t[lane], t[lane + n // 2] = a, bs[k % len(bs)]
                    k += 1
        check_round(zk, field, "witness", nprod, 2, logn, FM.real(field, r), True, st=st)


@pytest.mark.parametrize("field", [0, 3])
def test_constant_second_factor_at_structured_operands(field):
    """zk_sumcheck_gkr_rounds_cf with a NULL second table: the proof of the same rounds with that table filled with the constant"""
    zk = package()
    p = FM.MODULUS[field]
    for logn, kind, const in ((4, "stored_pm1", p - 1), (8, "hi0_lo_max", 1), (10, "mix", FM.real(field, p - 1))):
        n = 1 << logn
        st = make_tables(field, kind, 2, 2, n, 50 + logn)
        real = [[[FM.real(field, v) for v in t] for t in prod] for prod in st]
        real[1][1] = [const] * n
        polys = [[zk.MultilinearPolynomial(field, to_limbs(t)) for t in prod] for prod in st]
        cf = zk.from_ints(field, [0, const])
        co, ch, fin = zk.sumcheck.gkr_rounds_const_factors(field, [(polys[0][0], polys[0][1]), (polys[1][0], None)], cf, zk.Transcript())
        t = M.Transcript()
        cur = real
        for rd in range(logn):                                            # sumcheck_gkr_protocol.rs:37-60 (oracle/pymodel.py)
            coeffs = M.lagrange_interpolate([0, 1, 2], M.round_evals(cur, p), p)
            t.append(b"".join(M.le32(c) for c in coeffs))
            r = t.challenge(p)
            assert to_ints(co[rd]) == [FM.stored(field, c) for c in coeffs], (field, logn, rd)
            assert to_ints(ch[rd:rd + 1]) == [FM.stored(field, r)], (field, logn, rd)
            cur = [[M.partial_evaluate(x, 0, r, p) for x in prod] for prod in cur]
        assert to_ints(fin) == [FM.stored(field, x[0]) for prod in cur for x in prod], (field, logn)


@pytest.mark.parametrize("logn", [12, 16])
@pytest.mark.parametrize("kind", ["real_pm1", "stored_pm1", "mix"])
def test_whole_gkr_sumcheck_proofs_at_structured_operands(kind, logn):
    """2 x 2 tables of 2^12 (split rounds, tail) and of 2^16 (two rounds per launch) against the C oracle's proof"""
    zk = package()
    field = 0
    tabs = np.stack([np.stack([to_limbs(t) for t in prod]) for prod in make_tables(field, kind, 2, 2, 1 << logn, 77)])
    sp = zk.SumPolynomial([zk.ProductPolynomial([zk.MultilinearPolynomial(field, t) for t in prod]) for prod in tabs])
    claimed = O.vec_sum(field, O.sumpoly_reduce(field, tabs))
    t_gpu, t_cpu = zk.Transcript(), O.Transcript()
    result = zk.sumcheck.prove(sp, claimed, t_gpu)
    co, chal = O.sumcheck_gkr_prove(field, tabs, claimed, t_cpu)
    assert np.array_equal(result.round_univariate_polynomials, co) and np.array_equal(result.random_challenges, chal)
    assert t_gpu.sample_random_challenge() == t_cpu.sample_random_challenge()
    for pr in range(2):
        for f in range(2):
            assert np.array_equal(sp.product_polynomials[pr].polynomials[f].evaluated_values, tabs[pr][f])
