"""Child process of tests/test_gpu_fri_ml_weighted.py: the opening against a weight table at d = 13 with the reduction grids capped
(ZK_REDUCE_BLOCKS is read once per process; the parent sets it to 64), on both fields, every output against tests/_fri_ml_weighted_model.py.
Prints one JSON line: the cap the process saw, how many arrays were compared, which differed."""
import json

import numpy as np

import _zerocheck_worker as ZW  # puts the repository root and tests/ on sys.path
import _fri_ml_cases as FC  # noqa: E402
import _fri_ml_weighted_model as WM  # noqa: E402
import _ntt_model as NM  # noqa: E402

D, B, F, Q = 13, 1, 2, 4


def main():
    zk, blocks = ZW.start()
    checked, mismatches = 0, []
    for field in (0, 3):
        cm = FC.commitment(field, D, B, 1, 15000 + field, FC.hasher(zk))
        W0 = NM.random_ints(field, 1 << D, 15100 + field)
        op = WM.open_weighted(cm, W0, F, Q, 2, None, FC.hasher(zk))
        fl = WM.flat(zk, op)
        with FC.gpu_commitment(zk, cm) as gcm:
            got = zk.fri.open_weighted(gcm, zk.MultilinearPolynomial.vector(field, zk.from_ints(field, W0)), F, Q, log_arity=2)
        pairs = (("c", got.c, fl["c"]), ("polys", got.round_polys, fl["polys"]), ("roots", got.roots.tobytes(), fl["roots"]), ("final", got.final_table, fl["final"]),
                 ("challenges", got.challenges, fl["challenges"]), ("indices", list(got.query_indices), fl["indices"]),
                 ("values", got.query_values, fl["values"]), ("paths", got.query_paths.tobytes(), fl["paths"]))
        for name, a, b in pairs:
            checked += 1
            same = np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
            if not same:
                mismatches.append((field, name))
        checked += 1
        if not zk.fri.verify_weighted(cm["root"], fl["w_final"], got):
            mismatches.append((field, "the verifier"))
    print(json.dumps({"blocks": blocks, "checked": checked, "mismatches": mismatches}))


if __name__ == "__main__":
    main()
