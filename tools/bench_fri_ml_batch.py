"""Several FRI commitments opened together (zk_fri_ml_open_batch; csrc/fri_ml.cuh fri_ml_fold_batch_kernel) against the same work done table by
table: BLS12-381 Fr, b = 2, f = 6, Q = 64, k = 4.  JSON lines (stdout, and appended to --out):
  kind = "fold"    one codeword length N = 2^LOG: zk_fri_ml_fold_batch (r1 given: the fold by 4) on k codewords against
                   zk_mle_linear_combination followed by zk_fri_ml_fold4 on the same inputs, timed twice.  *_ms: the median host wall clock
                   of the whole call between two device synchronisations -- it includes the allocation of the outputs (N / 4 elements for
                   the fused call, N + N / 4 for the composition) and the power table each call builds.  *_dev_ms: the best time between
                   two device events around the call, as tools/bench_fri_ml_arity.py takes its folds: the kernels and whatever gap the host
                   leaves between them.  The bytes each moves by count ((k + 1/4) N against (k + 2 + 1/4) N elements of 32 bytes) and the
                   GB/s that count gives over the device time.  The two outputs are compared byte for byte first.
  kind = "open"    one case (d, schedule): in ONE process the batch opening of k commitments at P = 2 points and k single-table openings
                   (open_multilinear_points) of the same schedule on the same commitments and points: the median wall_ms of each with
                   zk_fri_ml_last_stats' split (the k single openings: summed), and path_bytes of the batch against k times the single form's.
                   Every timed opening is verified first.
Schedules: a1 (log_arity 1), a2 (log_arity 2), a2g (log_arity 2 on commitments with grouped leaves).  Without --case the tool runs every case
as a fresh child process of its own, each under `timeout`, one after the other, and stops at the first one that fails: a case that faults or
hangs starts nothing after it.
    python3 tools/bench_fri_ml_batch.py [--fold-sizes 22,24,26] [--sizes 20,22,24] [--schedules a1,a2,a2g] [--k 4] [--reps 5] [--warmup 2]
                                        [--step-timeout 300] [--out FILE]
    python3 tools/bench_fri_ml_batch.py --case fold:LOG | open:D:SCHEDULE ...          one case in this process"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_fri_ml_arity import KEYS, emit, setup, timed              # noqa: E402

FIELD, B, F, Q, P = 0, 2, 6, 64, 2
SCHEDULES = {"a1": (1, 0), "a2": (2, 0), "a2g": (2, 2)}       # (log_arity, log_group)


def run_fold(log_n, a):
    import numpy as np
    zk = setup()
    sync = zk.lib().zk_device_synchronize
    k, n = a.k, 1 << log_n
    tables = [zk.MultilinearPolynomial.random(FIELD, n, 0xF00 + 16 * log_n + j) for j in range(k)]
    coeffs = zk.from_ints(FIELD, [0xC0FFEE + 7919 * j for j in range(k)])
    r0, r1, coset = (zk.from_ints(FIELD, [v])[0] for v in (0x1234567, 0x7654321, 0x5EED))
    fused = lambda: zk.fri.ml_fold_batch(tables, coeffs, r0, r1, coset)
    composed = lambda: zk.fri.ml_fold4(zk.MultilinearPolynomial.linear_combination(tables, coeffs), r0, r1, coset)
    if not np.array_equal(fused().evaluated_values, composed().evaluated_values):
        raise SystemExit(f"the fused fold at 2^{log_n} differs from the composition: nothing is timed")
    import torch
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

    dev = {"composed": best_of(composed), "fused": best_of(fused)}
    walls = {"composed": [], "fused": []}
    for _ in range(3):                                       # interleaved rounds: a drift of the device shows in both
        for name, fn in (("composed", composed), ("fused", fused)):
            walls[name].append(timed(fn, a.reps, a.warmup, sync))
    row = {"kind": "fold", "field": FIELD, "log_len": log_n, "k": k}
    for name, elems in (("fused", (k + 0.25) * n), ("composed", (k + 2.25) * n)):
        ms = statistics.median(walls[name])
        row.update({name + "_ms": round(ms, 4), name + "_rounds_ms": [round(w, 4) for w in walls[name]], name + "_bytes": int(32 * elems),
                    name + "_dev_ms": round(dev[name], 4), name + "_dev_gbps": round(32 * elems / dev[name] / 1e6, 1)})
    row["fused_over_composed"] = round(row["fused_ms"] / row["composed_ms"], 4)
    row["fused_over_composed_dev"] = round(dev["fused"] / dev["composed"], 4)
    row["bytes_ratio"] = round((k + 0.25) / (k + 2.25), 4)
    emit(row, a.out)


def run_open(d, sched, a):
    import numpy as np
    zk = setup()
    sync = zk.lib().zk_device_synchronize
    arity, lg = SCHEDULES[sched]
    k = a.k
    coset = zk.from_ints(FIELD, [0x5EED])[0]
    cms = [zk.fri.commit(zk.MultilinearPolynomial.random(FIELD, 1 << d, 0xB00 + 16 * d + j), B, coset, log_group=lg) for j in range(k)]
    pts = np.stack([zk.from_ints(FIELD, [0x1234567 + 977 * i + 31337 * p for i in range(d)]) for p in range(P)])
    roots = [c.root for c in cms]
    op = zk.fri.open_multilinear_batch(cms, pts, F, Q, log_arity=arity)
    if not zk.fri.verify_multilinear_batch(roots, pts, op):
        raise SystemExit(f"the batch opening at d = {d} ({sched}) does not verify: nothing is timed")
    for c in cms:
        if not zk.fri.verify_multilinear_points(c.root, pts, zk.fri.open_multilinear_points(c, pts, F, Q, log_arity=arity)):
            raise SystemExit(f"a single opening at d = {d} ({sched}) does not verify: nothing is timed")
    stats = {"batch": [], "single": []}

    def batch():
        zk.fri.open_multilinear_batch(cms, pts, F, Q, log_arity=arity)
        stats["batch"].append(zk.fri.ml_last_stats())

    def single():
        tot = dict.fromkeys(KEYS, 0.0)
        for c in cms:
            zk.fri.open_multilinear_points(c, pts, F, Q, log_arity=arity)
            st = zk.fri.ml_last_stats()
            for key in KEYS:
                tot[key] += st[key]
        stats["single"].append(tot)

    wall = {"single": timed(single, a.reps, a.warmup, sync), "batch": timed(batch, a.reps, a.warmup, sync)}
    row = {"kind": "open", "field": FIELD, "d": d, "schedule": sched, "k": k, "points": P, "log_blowup": B, "log_final": F, "queries": Q, "verified": True}
    for name in ("batch", "single"):
        row[name + "_wall_ms"] = round(wall[name], 4)
        row.update({f"{name}_{key}": round(statistics.median(s[key] for s in stats[name][a.warmup:]), 4) for key in KEYS})
    one = zk.fri.ml_sizes(d, B, F, Q, log_arity=arity, grouped=lg == 2)[3]
    row.update({"batch_over_single": round(wall["batch"] / wall["single"], 4), "batch_path_bytes": zk.fri.ml_sizes(d, B, F, Q, arity, lg == 2, k=k)[3],
                "single_path_bytes": k * one})
    row["path_bytes_ratio"] = round(row["batch_path_bytes"] / row["single_path_bytes"], 4)
    emit(row, a.out)
    for c in cms:
        c.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fold-sizes", default="22,24,26")
    ap.add_argument("--sizes", default="20,22,24")
    ap.add_argument("--schedules", default="a1,a2,a2g")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--case", default=None, help="fold:LOG or open:D:SCHEDULE -- run this one case here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_ml_batch", "bench.jsonl"))
    a = ap.parse_args()
    if a.case:
        kind, *rest = a.case.split(":")
        if kind == "fold":
            run_fold(int(rest[0]), a)
        else:
            run_open(int(rest[0]), rest[1], a)
        return 0
    cases = [f"fold:{int(x)}" for x in a.fold_sizes.split(",") if x]
    cases += [f"open:{int(x)}:{s}" for x in a.sizes.split(",") if x for s in a.schedules.split(",") if s]
    for case in cases:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--case", case, "--k", str(a.k), "--reps", str(a.reps),
               "--warmup", str(a.warmup), "--out", a.out]
        rc = subprocess.call(cmd)
        if rc != 0:                                          # a fault, an abort or a time limit: nothing more is started on the device
            print(f"case {case} ended with status {rc}; stopping", file=sys.stderr, flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
