"""Child process of tests/test_gpu_fri_ml_points.py: the second trip of the grid-stride loops of the multilinear opening's two round passes
(csrc/fri_ml.cuh), where a lane keeps its lazy sums alive from one pair to the next.  ZK_REDUCE_BLOCKS is read once per process; the parent
sets it to 64, so that a stride is 2^14 lanes.  On BLS12-381 Fr, against Python integers:

  fri_ml_round_w_kernel   through zk_fri_ml_round, round 0's form at 2^16 entries and the fold form at 2^17, on random tables and on tables all
                          p - 1 with r = p - 1, against tests/_fri_ml_points_model.py round_g3 (tests/_zerocheck_worker.py stride_cases)
  fri_ml_round_kernel     has no call of its own: through zk_fri_ml_open at d = 17 with two rounds (log_final = 15).  Round 0 (nothing
                          folded) covers 2^16 pairs, four trips; round 1 (the fold form) 2^15, two.  The transcript is the library's: with the
                          two challenges it returns, the three values of each round, the final table and y are recomputed as
                          tests/_fri_ml_model.py open_at defines them; the host verifier accepts the opening.

Prints one JSON line: the cap the process saw, the trips a lane makes, how many comparisons were made, which differed."""
import json
import random

import numpy as np

import _zerocheck_worker as ZW  # puts the repository root and tests/ on sys.path
import _fri_ml_model as ML  # noqa: E402
import _fri_ml_points_model as PT  # noqa: E402
import _ntt_model as NM  # noqa: E402
import _plonk_model as KM  # noqa: E402

FIELD, D, LOG_FINAL, Q = ZW.FIELD, 17, 15, 4


def opening(zk, mismatches):
    """-> the number of comparisons made"""
    p, rng = NM.MODULUS[FIELD], random.Random(14000)
    mont = lambda ints: KM.mont(zk, FIELD, ints)
    coeffs = NM.random_ints(FIELD, 1 << D, 14100)
    z = [rng.randrange(p) for _ in range(D)]
    zm = mont(z)
    with zk.fri.commit(zk.MultilinearPolynomial.vector(FIELD, mont(coeffs)), 1) as cm:
        got = zk.fri.open_multilinear(cm, zm, LOG_FINAL, Q)
        accepted = zk.fri.verify_multilinear(cm.root, zm, got)
    rs = [int(v) for v in zk.to_ints(FIELD, got.challenges)]
    T, A, polys = coeffs, 1, []
    for l, r in enumerate(rs):                                # tests/_fri_ml_model.py open_at, the transcript's challenges given
        v = D - 1 - l
        E = ML.eq_table(z[:v], p)
        S = [sum(E[x] * T[2 * x + X] for x in range(len(E))) % p for X in (0, 1)]
        polys += [A * ML.eq1(X, z[v], p) * (S[0] + X * (S[1] - S[0])) % p for X in (0, 1, 2)]
        A = A * ML.eq1(r, z[v], p) % p
        T = ML.mle_fold_last(FIELD, T, r)
    checks = [("opening: two rounds", len(rs) == D - LOG_FINAL), ("opening: the rounds' values", np.array_equal(got.round_polys.reshape(-1, 4), mont(polys))),
              ("opening: the final table", np.array_equal(got.final_table, mont(T))), ("opening: y", np.array_equal(got.y, mont([ML.mle_evaluate(FIELD, coeffs, z)])[0])),
              ("opening: the verifier", accepted is True)]
    mismatches += [name for name, same in checks if not same]
    return len(checks)


def main():
    zk, blocks = ZW.start()
    p = NM.MODULUS[FIELD]
    mismatches = []

    def fold(dev, r):
        *outs, g = zk.fri.ml_round(*dev, r)
        return outs, g

    checked = ZW.stride_cases(zk, 2, lambda tabs: PT.round_g3(*tabs, p), lambda dev: zk.fri.ml_round(*dev), fold, 14200, mismatches)
    checked += opening(zk, mismatches)
    trips = {"round_w round0": ZW.trips_of((1 << ZW.LOG_FOLD) // 4, blocks), "round_w fold": ZW.trips_of((1 << ZW.LOG_FOLD) // 4, blocks),
             "round round0": ZW.trips_of(1 << (D - 1), blocks), "round fold": ZW.trips_of(1 << (D - 2), blocks)}
    print(json.dumps({"blocks": blocks, "trips": trips, "checked": checked, "mismatches": mismatches}))


if __name__ == "__main__":
    main()
