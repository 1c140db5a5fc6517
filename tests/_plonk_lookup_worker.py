"""Child process of tests/test_gpu_plonk_lookup.py: the second trip of the round pass's grid-stride loop, the only place where a lane's gamma id
is advanced across a stride (gnext) -- and, in this pass, comes back from LDS after the lookup's phase first.  ZK_REDUCE_BLOCKS is read once
per process; the parent sets it to 64, so that a stride is 64 x 256 = 2^14 lanes and 2^15 pairs take two trips.  On BLS12-381 Fr, against the
Python-integer model of tests/_plonk_lookup_model.py:

  zk_plonk_lookup_round    round 0's form at 2^16 entries and the fold form at 2^17 entries

The fold form's sums are taken over the folded tables, so one model evaluation on the fold of the 2^17 serves both forms: round 0's form runs on
those folded tables with the same id tables.  Prints one JSON line: the trips a lane makes, how many comparisons were made, which differed."""
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
import _plonk_lookup_model as KL  # noqa: E402

FIELD, LOG_FOLD, LOG_STEP = 0, 17, 1


def main():
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    blocks = int(os.environ.get("ZK_REDUCE_BLOCKS", "1536"))
    p, rng = NM.MODULUS[FIELD], random.Random(17000)
    n = 1 << LOG_FOLD
    mont = lambda ints: KL.mont(zk, FIELD, ints)
    table = lambda ints: zk.MultilinearPolynomial.vector(FIELD, mont(ints))
    tabs = [NM.random_ints(FIELD, n, 17100 + j) for j in range(KL.TABLES)]
    r, id_base = rng.randrange(p), rng.randrange(p)
    ch = tuple(rng.randrange(p) for _ in range(4))
    folded = [ML.mle_fold_last(FIELD, t, r) for t in tabs]
    summed = n // 2                                           # 2^16 entries, 2^15 pairs
    d = LOG_FOLD - 1 + LOG_STEP
    ids = [[(j * (1 << d) + id_base + (1 << LOG_STEP) * x) % p for x in range(summed)] for j in range(3)]
    want = mont(KL.round_g5(folded, ids, ch, p)[0])
    els = [mont([v])[0] for v in ch]
    kw = dict(id_base=mont([id_base])[0], log_step=LOG_STEP)
    dev, dev_folded = [table(t) for t in tabs], [table(t) for t in folded]
    mismatches, checked = [], 0

    def check(name, got):
        nonlocal checked
        checked += 1
        if not np.array_equal(got, want):
            mismatches.append(name)

    check("round0 2^16", zk.plonk_lookup.round(dev_folded, *els, **kw))
    outs, g5 = zk.plonk_lookup.round(dev, *els, r=mont([r])[0], **kw)
    if not all(np.array_equal(o.evaluated_values, f.evaluated_values) for o, f in zip(outs, dev_folded)):
        mismatches.append("fold 2^17: the folded tables")
    check("fold 2^17", g5)
    pairs = summed // 2
    trips = -(-pairs // (blocks * 256))
    print(json.dumps({"trips": {"round0": trips, "fold": trips}, "checked": checked, "mismatches": mismatches}))


if __name__ == "__main__":
    main()
