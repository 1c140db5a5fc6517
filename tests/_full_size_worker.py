"""Child process of tests/test_gpu_full_size_parity.py: full-size proofs under an environment switch that selects other kernels
(ZK_HOST_TRANSCRIPT=0, ZK_FOLD_SPLIT2=0: read once per process).  Every table is rebuilt from its seed, proved on the GPU, and one JSON
line of SHA-256 digests of the proof arrays is printed; the parent compares them with the digests of the oracle's arrays.  No oracle runs
here.  Also the one place the parent takes its seeds, tables, provers and digests from, so both sides prove the same statements.

    python tests/_full_size_worker.py basic:0:24 gkr:0:2x2:22 ..."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import __graft_entry__ as G                                                          # noqa: E402

SEED_BASIC = 0x5EED_F500
SEED_GKR = 0x5EED_F600
GKR_PREFIX = b"full-size parity: the state a caller left"     # the GKR sumcheck starts from a sponge that has absorbed this


def fill(zk, field, out, seed):
    """out (n, limbs), C-contiguous: zk_host_fill_random, the generator every test rebuilds its tables with"""
    assert out.flags.c_contiguous
    assert zk.lib().zk_host_fill_random(field, seed, 0, out.shape[0], out.ctypes.data_as(C.POINTER(C.c_uint64))) == 0


def basic_table(zk, field, logn):
    t = np.empty((1 << logn, zk.limbs(field)), np.uint64)
    fill(zk, field, t, SEED_BASIC + 64 * field + logn)
    return t


def gkr_tables(zk, field, nprod, nfac, logn):
    tabs = np.empty((nprod, nfac, 1 << logn, zk.limbs(field)), np.uint64)
    for p in range(nprod):
        for f in range(nfac):
            fill(zk, field, tabs[p, f], SEED_GKR + 4096 * field + 256 * logn + 16 * p + f)
    return tabs


def prove_basic(zk, field, table):
    """Prover::prove -> (claimed sum, round polynomials, challenges, Verifier::verify)"""
    prover = zk.Prover.init(field, table)
    proof = prover.prove()
    ok = zk.Verifier.init().verify(proof)
    return proof.initial_claimed_sum, proof.round_univariate_polynomials, prover.challenges, ok


def prove_gkr(zk, field, tabs, claimed):
    """sumcheck_gkr_protocol::prove from a transcript that has absorbed GKR_PREFIX -> (coefficients, challenges, the next sample)"""
    MP = zk.MultilinearPolynomial
    sp = zk.SumPolynomial([zk.ProductPolynomial([MP(field, t) for t in prod]) for prod in tabs])
    t = zk.Transcript()
    t.append(GKR_PREFIX)
    res = zk.sumcheck.prove(sp, claimed, t)
    return res.round_univariate_polynomials, res.random_challenges, t.sample_random_challenge()


def digest(a):
    """SHA-256 of the stored limbs (bytes as they are): shape-independent, so (n, L) and (n * L,) agree"""
    if isinstance(a, bytes):
        return hashlib.sha256(a).hexdigest()
    return hashlib.sha256(np.ascontiguousarray(a, np.uint64).tobytes()).hexdigest()


def parse_case(case):
    """'basic:<field>:<log2 n>' or 'gkr:<field>:<products>x<factors>:<log2 n>'"""
    kind, field, *rest = case.split(":")
    if kind == "basic":
        return kind, int(field), int(rest[0])
    nprod, nfac = (int(v) for v in rest[0].split("x"))
    return kind, int(field), nprod, nfac, int(rest[1])


def main(cases):
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    out = {}
    for case in cases:
        spec = parse_case(case)
        if spec[0] == "basic":
            _, field, logn = spec
            table = basic_table(zk, field, logn)
            cs, rp, ch, ok = prove_basic(zk, field, table)
            out[case] = {"claimed": digest(cs), "rounds": digest(rp), "challenges": digest(ch), "verified": ok}
            del table
        else:
            _, field, nprod, nfac, logn = spec
            tabs = gkr_tables(zk, field, nprod, nfac, logn)
            MP = zk.MultilinearPolynomial
            claimed = zk.SumPolynomial([zk.ProductPolynomial([MP(field, t) for t in prod]) for prod in tabs]).add_polynomials_element_wise().sum()
            co, ch, nxt = prove_gkr(zk, field, tabs, claimed)
            out[case] = {"claimed": digest(claimed), "coeffs": digest(co), "challenges": digest(ch), "next_sample": digest(nxt)}
            del tabs
    env = {k: v for k, v in os.environ.items() if k.startswith("ZK_")}
    print(json.dumps({"cases": out, "env": env}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
