"""Child process of tests/test_gpu_plonk.py: the second trip of the round passes' grid-stride loop, the only place where a lane's gamma id is
advanced across a stride (gnext).  ZK_REDUCE_BLOCKS is read once per process; the parent sets it to 64, so that a stride is 64 x 256 = 2^14 lanes
and 2^15 pairs take two trips.  On BLS12-381 Fr, against the Python-integer models:

  zk_plonk_round    round 0's form at 2^16 entries and the fold form at 2^17 entries, against _plonk_model
  zk_wiring_round   the same two sizes (the wiring's ten of the same tables), against _wiring_model: its loop has the same step

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
import _plonk_model as KM  # noqa: E402
import _wiring_model as WM  # noqa: E402

FIELD, LOG_FOLD, LOG_STEP = 0, 17, 1
WIRING_PLACES = (0, 1, 2, 8, 9, 10, 11, 12, 13, 14)


def main():
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    blocks = int(os.environ.get("ZK_REDUCE_BLOCKS", "1536"))
    p, rng = NM.MODULUS[FIELD], random.Random(11000)
    n = 1 << LOG_FOLD
    mont = lambda ints: KM.mont(zk, FIELD, ints)
    table = lambda ints: zk.MultilinearPolynomial.vector(FIELD, mont(ints))
    tabs = [NM.random_ints(FIELD, n, 11100 + j) for j in range(15)]
    r, id_base = rng.randrange(p), rng.randrange(p)
    ch = tuple(rng.randrange(p) for _ in range(4))
    folded = [ML.mle_fold_last(FIELD, t, r) for t in tabs]
    summed = n // 2                                           # 2^16 entries, 2^15 pairs
    d = LOG_FOLD - 1 + LOG_STEP
    ids = [[(j * (1 << d) + id_base + (1 << LOG_STEP) * x) % p for x in range(summed)] for j in range(3)]
    want_plonk = mont(KM.round_g5(folded, ids, ch, p)[0])
    want_wiring = mont(WM.round_g5([folded[j] for j in WIRING_PLACES], ids, ch, p))
    els = [mont([v])[0] for v in ch]
    kw = dict(id_base=mont([id_base])[0], log_step=LOG_STEP)
    dev, dev_folded = [table(t) for t in tabs], [table(t) for t in folded]
    mismatches, checked = [], 0

    def check(name, got, want):
        nonlocal checked
        checked += 1
        if not np.array_equal(got, want):
            mismatches.append(name)

    check("plonk round0 2^16", zk.plonk.round(dev_folded, *els, **kw), want_plonk)
    outs, g5 = zk.plonk.round(dev, *els, r=mont([r])[0], **kw)
    if not all(np.array_equal(o.evaluated_values, f.evaluated_values) for o, f in zip(outs, dev_folded)):
        mismatches.append("plonk fold 2^17: the folded tables")
    check("plonk fold 2^17", g5, want_plonk)
    check("wiring round0 2^16", zk.wiring.round([dev_folded[j] for j in WIRING_PLACES], *els, **kw), want_wiring)
    outs, g5 = zk.wiring.round([dev[j] for j in WIRING_PLACES], *els, r=mont([r])[0], **kw)
    if not all(np.array_equal(o.evaluated_values, dev_folded[j].evaluated_values) for o, j in zip(outs, WIRING_PLACES)):
        mismatches.append("wiring fold 2^17: the folded tables")
    check("wiring fold 2^17", g5, want_wiring)
    pairs = summed // 2
    trips = -(-pairs // (blocks * 256))
    print(json.dumps({"trips": {"round0": trips, "fold": trips}, "checked": checked, "mismatches": mismatches}))


if __name__ == "__main__":
    main()
