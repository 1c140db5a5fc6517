"""Child process of tests/test_gpu_zerocheck.py and tests/test_gpu_zerocheck_gate.py: the second trip of the zerocheck round passes' grid-stride
loops, where a lane keeps its lazy sums (mle_kernels.cuh Wide) alive from one pair to the next.  ZK_REDUCE_BLOCKS is read once per process; the
parent sets it to 64, so that a stride is 64 x 256 = 2^14 lanes and 2^15 pairs take two trips.  argv[1] picks the kernel:

  mul    zk_zerocheck_mul_round   (zerocheck_mul_round_kernel, four tables) against tests/_zerocheck_model.py
  gate   zk_zerocheck_gate_round  (zerocheck_gate_round_kernel, nine tables) against tests/_zerocheck_gate_model.py

On BLS12-381 Fr, in round 0's form at 2^16 entries and in the fold form at 2^17 entries (stride_cases, which tests/_fri_ml_worker.py runs on
its own pass too).  The fold form's sums are taken over the folded tables, so one model evaluation on the fold of the 2^17 serves both forms:
round 0's form runs on those folded tables.  Twice: on random tables with a random r, and with every table all p - 1 and r = p - 1 (the fold
of such a table is all p - 1 again), the largest operands a lane can carry from one trip into the next.  In the fold form the folded tables
are compared with mle_fold_last; in both forms the inputs are read back and compared with what was uploaded.  Prints one JSON line: the cap
the process saw, the trips a lane makes, how many comparisons were made, which differed."""
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

import __graft_entry__ as G  # noqa: E402
import _fri_ml_model as ML  # noqa: E402
import _ntt_model as NM  # noqa: E402
import _plonk_model as KM  # noqa: E402
import _zerocheck_gate_model as ZG  # noqa: E402
import _zerocheck_model as ZM  # noqa: E402

FIELD, LOG_FOLD = 0, 17


def start():
    """-> (the package with the device initialised, the cap of the reduction grids this process runs with)"""
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    return zk, int(os.environ.get("ZK_REDUCE_BLOCKS", "1536"))


def trips_of(pairs, blocks):
    return -(-pairs // (blocks * 256))


def stride_cases(zk, ntab, model, round0, fold, seed, mismatches):
    """model(tables) -> the message in integers; round0(device tables) -> the message; fold(device tables, r) -> (folded tables, message).
    Appends what differed to `mismatches`; -> the number of comparisons made"""
    p, rng = NM.MODULUS[FIELD], random.Random(seed)
    n = 1 << LOG_FOLD
    mont = lambda ints: KM.mont(zk, FIELD, ints)
    checked = 0

    def check(name, same):
        nonlocal checked
        checked += 1
        if not same:
            mismatches.append(name)

    def case(what, tabs, r):
        folded = [ML.mle_fold_last(FIELD, t, r) for t in tabs]
        want = mont(model(folded))
        up, up_folded = [mont(t) for t in tabs], [mont(t) for t in folded]
        dev, dev_folded = ([zk.MultilinearPolynomial.vector(FIELD, m) for m in ms] for ms in (up, up_folded))
        check(what + " round0 2^16: the sums", np.array_equal(round0(dev_folded), want))
        check(what + " round0 2^16: the inputs", all(np.array_equal(t.evaluated_values, m) for t, m in zip(dev_folded, up_folded)))
        outs, g = fold(dev, mont([r])[0])
        check(what + " fold 2^17: the sums", np.array_equal(g, want))
        check(what + " fold 2^17: the folded tables", len(outs) == ntab and all(np.array_equal(o.evaluated_values, m) for o, m in zip(outs, up_folded)))
        check(what + " fold 2^17: the inputs", all(np.array_equal(t.evaluated_values, m) for t, m in zip(dev, up)))

    case("random", [NM.random_ints(FIELD, n, seed + 100 + j) for j in range(ntab)], rng.randrange(p))
    top = [p - 1] * n
    assert ML.mle_fold_last(FIELD, top, p - 1) == [p - 1] * (n // 2)
    case("all p - 1", [top] * ntab, p - 1)
    return checked


def main():
    kernel = sys.argv[1]
    zk, blocks = start()
    p = NM.MODULUS[FIELD]
    if kernel == "mul":
        ntab, model = 4, lambda tabs: ZM.round_g4(*tabs, p)
        round0 = lambda dev: zk.zerocheck.mul_round(*dev)

        def fold(dev, r):
            *outs, g = zk.zerocheck.mul_round(*dev, r=r)
            return outs, g
    else:
        ntab, model = 9, lambda tabs: ZG.round_g5(tabs, p)
        round0 = lambda dev: zk.zerocheck.gate_round(dev)
        fold = lambda dev, r: zk.zerocheck.gate_round(dev, r=r)
    mismatches = []
    checked = stride_cases(zk, ntab, model, round0, fold, 13000, mismatches)
    trips = trips_of((1 << LOG_FOLD) // 4, blocks)
    print(json.dumps({"kernel": kernel, "blocks": blocks, "trips": {"round0": trips, "fold": trips}, "checked": checked, "mismatches": mismatches}))


if __name__ == "__main__":
    main()
