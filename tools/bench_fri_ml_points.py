"""Multilinear opening of a FRI commitment at P = 2 points (zk_fri_ml_open_points; csrc/fri_ml.cuh fri_ml_round_w_kernel), b = 2, f = 6, Q = 64,
against what it replaces.  JSON lines (stdout, and appended to --out):
  kind = "open"    one case (field, d): wall_ms of ONE two-point opening with zk_fri_ml_last_stats' split, against TWO zk_fri_ml_open calls on
                   the same commitment in the same process (their walls and splits summed), `points_over_two_singles` = the ratio; on
                   BLS12-381 Fr also the two zk_kzg_open calls zk_gkr_prove_succinct makes at the same size (opening key precomputed).
                   Every timed opening is verified first (zk_fri_ml_verify_points, zk_fri_ml_verify, MultilinearKZG.verify).
  kind = "round"   zk_fri_ml_round (r given: T and W folded, three sums) on tables of 2^d entries against the single-point pass on the same
                   table -- MultilinearPolynomial.fold_half_sums has another shape, so the pass timed is the one inside an opening: what is
                   reported for it is ms_sumcheck / rounds of the single-point opening of the same run; the new pass is timed on its own,
                   device events around the call (its two output allocations inside), GB/s over its own traffic 12 x 32 x q bytes, q = 2^d / 4.
Cases: BLS12-381 Fr at --sizes, BN254 Fr once at --bn254-size.  Without --case the tool runs every case as a fresh child process of its own,
each under `timeout`, one after the other, and stops at the first one that fails (what `a && b && c` does): a case that faults or hangs
starts nothing after it.
    python3 tools/bench_fri_ml_points.py [--sizes 16,20,24] [--bn254-size 20] [--reps 5] [--warmup 2] [--step-timeout 240] [--out FILE]
    python3 tools/bench_fri_ml_points.py --case FIELD:D ...          one case in this process"""
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


def split(stats, warmup, prefix=""):
    return {prefix + key: round(statistics.median(s[key] for s in stats[warmup:]), 4) for key in KEYS}


def run_case(field, d, a):
    import numpy as np
    import torch
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    MP, lib = zk.MultilinearPolynomial, zk.lib()
    sync = lib.zk_device_synchronize
    b, f, Q = 2, 6, 64
    coset = zk.from_ints(field, [0x5EED])[0]
    table = MP.random(field, 1 << d, 0xB00 + 16 * d + field)
    c = zk.fri.commit(table, b, coset)
    pts = np.stack([zk.from_ints(field, [0x1234567 + 977 * i + 31337 * k for i in range(d)]) for k in range(2)])

    op = zk.fri.open_multilinear_points(c, pts, f, Q)
    if not zk.fri.verify_multilinear_points(c.root, pts, op):
        raise SystemExit(f"the two-point opening at d = {d} does not verify: nothing is timed")
    for k in range(2):
        if not zk.fri.verify_multilinear(c.root, pts[k], zk.fri.open_multilinear(c, pts[k], f, Q)):
            raise SystemExit(f"the single-point opening {k} at d = {d} does not verify: nothing is timed")
    pstats, sstats = [], [[], []]

    def run_points():
        zk.fri.open_multilinear_points(c, pts, f, Q)
        pstats.append(zk.fri.ml_last_stats())

    def run_singles():
        for k in range(2):
            zk.fri.open_multilinear(c, pts[k], f, Q)
            sstats[k].append(zk.fri.ml_last_stats())

    wall_p = timed(run_points, a.reps, a.warmup, sync)
    wall_s = timed(run_singles, a.reps, a.warmup, sync)
    sp, s0, s1 = split(pstats, a.warmup), split(sstats[0], a.warmup), split(sstats[1], a.warmup)
    row = {"kind": "open", "field": field, "d": d, "points": 2, "log_blowup": b, "log_final": f, "queries": Q, "verified": True,
           "points_wall_ms": round(wall_p, 4), **{"points_" + k: v for k, v in sp.items()}, "two_singles_wall_ms": round(wall_s, 4),
           **{"two_singles_" + k: round(s0[k] + s1[k], 4) for k in KEYS}, "points_over_two_singles": round(wall_p / wall_s, 4)}

    # the round pass on its own
    r = zk.from_ints(field, [0xD33B])[0]
    W = MP.random(field, 1 << d, 0xC00 + d)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e30
    for _ in range(a.reps + a.warmup):
        e0.record()
        out = zk.fri.ml_round(table, W, r)
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
        del out
    q = (1 << d) // 4
    rounds = d - f
    single_pass = s0["ms_sumcheck"] / rounds
    rrow = {"kind": "round", "field": field, "d": d, "ml_round_ms": round(best, 4), "ml_round_GBps": round(12 * 32.0 * q / (best * 1e-3) / 1e9, 1),
            "single_point_ms_sumcheck_per_round": round(single_pass, 4), "single_point_rounds": rounds,
            "note": "ml_round_ms: one pass over 2^d entries, output allocations inside; the single-point figure is the mean over the d - f passes "
                    "of one opening, whose tables halve every round (about 2 passes' worth of the first)"}
    del W

    if field == 0:                                           # the two openings of zk_gkr_prove_succinct at this size
        KZG = zk.MultilinearKZG
        taus = zk.from_ints(0, [0x1000003 * (i + 1) + 12345 for i in range(d)])
        setup = zk.TrustedSetup.initialize_setup(taus)
        setup.precompute_for_opens()
        cmt = KZG.commit_to_polynomial(table, setup)
        for k in range(2):
            if not KZG.verify(setup, cmt, pts[k], KZG.open_and_prove(table, setup, pts[k])):
                raise SystemExit(f"the KZG opening {k} at d = {d} does not verify: nothing is timed")
        wall_k = timed(lambda: [KZG.open_and_prove(table, setup, pts[k]) for k in range(2)], a.reps, a.warmup, sync)
        row.update({"two_kzg_opens_wall_ms": round(wall_k, 4), "points_over_two_kzg_opens": round(wall_p / wall_k, 4)})
        del setup
    emit(row, a.out)
    emit(rrow, a.out)
    c.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20,24")
    ap.add_argument("--bn254-size", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--case", default=None, help="FIELD:D -- run this one case here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_ml_points", "bench.jsonl"))
    a = ap.parse_args()
    if a.case:
        field, d = (int(x) for x in a.case.split(":"))
        run_case(field, d, a)
        return 0
    cases = [(0, int(x)) for x in a.sizes.split(",") if x] + ([(3, a.bn254_size)] if a.bn254_size else [])
    for field, d in cases:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--case", f"{field}:{d}", "--reps", str(a.reps),
               "--warmup", str(a.warmup), "--out", a.out]
        rc = subprocess.call(cmd)
        if rc != 0:                                          # a fault, an abort or a time limit: nothing more is started on the device
            print(f"case {field}:{d} ended with status {rc}; stopping", file=sys.stderr, flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
