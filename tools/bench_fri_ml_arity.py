"""Multilinear opening of a FRI commitment at P = 2 points folded by 4 (zk_fri_ml_open_points_arity, log_arity = 2; csrc/fri_ml.cuh
fri_ml_fold4_kernel) against the same opening folded by 2, b = 2, f = 6, Q = 64.  JSON lines (stdout, and appended to --out):
  kind = "open"    one case (field, d): wall_ms of ONE log_arity = 2 opening with zk_fri_ml_last_stats' split, against ONE log_arity = 1 opening of
                   the same commitment in the same process, `arity2_over_arity1` = the ratio of the walls and the ratios of the trees and
                   folds columns.  Every timed opening is verified first (zk_fri_ml_verify_points_arity / zk_fri_ml_verify_points).
  kind = "fold"    zk_fri_ml_fold4 on a codeword of 2^L entries against the two zk_fri_ml_fold calls it replaces (the second on the first's
                   output), with a coset: device events around the calls, their output allocations inside, the best of reps + warmup.
Cases: BLS12-381 Fr at --sizes, BN254 Fr once at --bn254-size; the fold at --fold-sizes (BLS12-381 Fr).  Without --case the tool runs every case
as a fresh child process of its own, each under `timeout`, one after the other, and stops at the first one that fails (what `a && b && c`
does): a case that faults or hangs starts nothing after it.
    python3 tools/bench_fri_ml_arity.py [--sizes 16,20,24] [--bn254-size 20] [--fold-sizes 20,22,24] [--reps 5] [--warmup 2] [--step-timeout 240] [--out FILE]
    python3 tools/bench_fri_ml_arity.py --case open:FIELD:D | fold:FIELD:L ...          one case in this process"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G                                            # noqa: E402

KEYS = ("ms_sumcheck", "ms_folds", "ms_trees", "ms_queries", "ms_total")


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def timed(fn, reps, warmup, sync):
    """median host-clock ms of fn() between two device synchronisations"""
    for _ in range(warmup):
        fn()
    wall = []
    for _ in range(reps):
        sync(); t0 = time.perf_counter()
        fn()
        sync(); wall.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(wall)


def split(stats, warmup, prefix):
    return {prefix + key: round(statistics.median(s[key] for s in stats[warmup:]), 4) for key in KEYS}


def setup():
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    return zk


def run_open(field, d, a):
    import numpy as np
    zk = setup()
    sync = zk.lib().zk_device_synchronize
    b, f, Q = 2, 6, 64
    coset = zk.from_ints(field, [0x5EED])[0]
    table = zk.MultilinearPolynomial.random(field, 1 << d, 0xB00 + 16 * d + field)
    c = zk.fri.commit(table, b, coset)
    pts = np.stack([zk.from_ints(field, [0x1234567 + 977 * i + 31337 * k for i in range(d)]) for k in range(2)])
    stats = {1: [], 2: []}
    for arity in (1, 2):
        op = zk.fri.open_multilinear_points(c, pts, f, Q, log_arity=arity)
        if not zk.fri.verify_multilinear_points(c.root, pts, op):
            raise SystemExit(f"the log_arity = {arity} opening at d = {d} does not verify: nothing is timed")

    def run(arity):
        zk.fri.open_multilinear_points(c, pts, f, Q, log_arity=arity)
        stats[arity].append(zk.fri.ml_last_stats())

    wall = {arity: timed(lambda: run(arity), a.reps, a.warmup, sync) for arity in (2, 1)}
    s1, s2 = split(stats[1], a.warmup, "arity1_"), split(stats[2], a.warmup, "arity2_")
    ratio = lambda key: round(s2["arity2_" + key] / s1["arity1_" + key], 4) if s1["arity1_" + key] else None
    emit({"kind": "open", "field": field, "d": d, "points": 2, "log_blowup": b, "log_final": f, "queries": Q, "verified": True,
          "arity2_wall_ms": round(wall[2], 4), **s2, "arity1_wall_ms": round(wall[1], 4), **s1, "arity2_over_arity1": round(wall[2] / wall[1], 4),
          "trees_ratio": ratio("ms_trees"), "folds_ratio": ratio("ms_folds"), "sumcheck_ratio": ratio("ms_sumcheck")}, a.out)
    c.free()


def run_fold(field, L, a):
    import numpy as np
    import torch
    zk = setup()
    cw = zk.MultilinearPolynomial.random(field, 1 << L, 0xF00 + L + field)
    r0, r1 = zk.from_ints(field, [0xD33B])[0], zk.from_ints(field, [0xBEE5])[0]
    cs, cs2 = zk.from_ints(field, [0x5EED])[0], zk.from_ints(field, [0x5EED * 0x5EED])[0]
    if not np.array_equal(zk.fri.ml_fold4(cw, r0, r1, cs).evaluated_values, zk.fri.ml_fold(zk.fri.ml_fold(cw, r0, cs), r1, cs2).evaluated_values):
        raise SystemExit(f"zk_fri_ml_fold4 at 2^{L} is not two folds: nothing is timed")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def best_of(fn):
        best = 1e30
        for _ in range(a.reps + a.warmup):
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1))
            del out
        return best

    four = best_of(lambda: zk.fri.ml_fold4(cw, r0, r1, cs))
    two = best_of(lambda: zk.fri.ml_fold(zk.fri.ml_fold(cw, r0, cs), r1, cs2))
    n = 1 << L
    emit({"kind": "fold", "field": field, "log_len": L, "coset": True, "fold4_ms": round(four, 4), "two_folds_ms": round(two, 4),
          "fold4_over_two_folds": round(four / two, 4), "fold4_GBps": round(32.0 * (n + n / 4) / (four * 1e-3) / 1e9, 1),
          "two_folds_GBps": round(32.0 * (n + n / 2 + n / 2 + n / 4) / (two * 1e-3) / 1e9, 1),
          "note": "the power table of the domain is built inside each call (zk_fri_ml_fold: two tables, zk_fri_ml_fold4: one)"}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20,24")
    ap.add_argument("--bn254-size", type=int, default=20)
    ap.add_argument("--fold-sizes", default="20,22,24")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--case", default=None, help="open:FIELD:D or fold:FIELD:L -- run this one case here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_ml_arity", "bench.jsonl"))
    a = ap.parse_args()
    if a.case:
        kind, field, size = a.case.split(":")
        (run_open if kind == "open" else run_fold)(int(field), int(size), a)
        return 0
    cases = [f"open:0:{int(x)}" for x in a.sizes.split(",") if x] + ([f"open:3:{a.bn254_size}"] if a.bn254_size else [])
    cases += [f"fold:0:{int(x)}" for x in a.fold_sizes.split(",") if x]
    for case in cases:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps),
               "--warmup", str(a.warmup), "--out", a.out]
        rc = subprocess.call(cmd)
        if rc != 0:                                          # a fault, an abort or a time limit: nothing more is started on the device
            print(f"case {case} ended with status {rc}; stopping", file=sys.stderr, flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
