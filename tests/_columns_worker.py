"""Child process of tests/test_gpu_merkle_columns.py: the second trip of the column leaf kernel's grid-stride loop.  ZK_MERKLE_COLUMNS_BLOCKS is
read once per process; the parent sets it to 2, so that a stride is 2 x 256 lanes and the 2^10 leaves of trees over tables of 2^12 entries take
two trips.  On both scalar fields, at k = 3 and k = 17 (the message's end one byte into a block), against the model of
tests/_fri_ml_columns_model.py: the root in root-only mode, and every leaf of the built tree through the paths of all leaves.  Prints one
JSON line: the trips a lane makes, how many comparisons were made, which differed."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

import __graft_entry__ as G  # noqa: E402
import _fri_ml_columns_model as CM  # noqa: E402
import _ntt_model as NM  # noqa: E402

LOG_LEN = 12


def main():
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    blocks = int(os.environ.get("ZK_MERKLE_COLUMNS_BLOCKS", "16384"))
    hasher = CM.check_host_keccak(zk)
    n = 1 << LOG_LEN
    part = n >> 2
    mismatches, checked = [], 0
    for field in (0, 3):
        cols = [NM.random_ints(field, n, 4400 + 5 * field + c) for c in range(17)]
        dev = [zk.MultilinearPolynomial.vector(field, CM.mont(zk, field, c)) for c in cols]
        for k in (3, 17):
            levels = CM.levels_of(cols[:k], hasher)
            checked += 2
            if zk.merkle.columns_root(dev[:k]) != levels[-1][0]:
                mismatches.append("root f%d k%d" % (field, k))
            paths = zk.MerkleTree.build_columns(dev[:k]).open(np.arange(part))
            lv = np.frombuffer(b"".join(levels[0]), np.uint8).reshape(-1, 32)
            if not np.array_equal(paths[:, 0], lv[np.arange(part) ^ 1]):
                mismatches.append("leaves f%d k%d" % (field, k))
    print(json.dumps({"trips": -(-part // (blocks * 256)), "checked": checked, "mismatches": mismatches}))


if __name__ == "__main__":
    main()
