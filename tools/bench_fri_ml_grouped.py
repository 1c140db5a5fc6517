"""Multilinear opening of a FRI commitment with GROUPED leaves (zk_fri_ml_open_points_grouped; csrc/merkle.cuh merkle_leaf_group_kernel) against
the ungrouped openings of the same table at log_arity = 2 and 1, P = 2, b = 2, f = 6, Q = 64.  JSON lines (stdout, and appended to --out):
  kind = "open"    one case (field, d): in ONE process the arity-1 and arity-2 openings of zk_fri_commit's commitment and the grouped opening of
                   zk_fri_commit_grouped's, the same table, points and parameters: the median wall_ms of each with zk_fri_ml_last_stats' split,
                   the three path_bytes (zk_fri_ml_sizes*), the medians of zk_fri_commit and zk_fri_commit_grouped (device allocations inside),
                   and the ratios grouped / arity 2 of the walls and of the trees, folds and sumcheck columns.  Every timed opening is verified
                   first.
Cases: BLS12-381 Fr at --sizes, BN254 Fr once at --bn254-size.  Without --case the tool runs every case as a fresh child process of its own,
each under `timeout`, one after the other, and stops at the first one that fails: a case that faults or hangs starts nothing after it.
    python3 tools/bench_fri_ml_grouped.py [--sizes 16,20,24] [--bn254-size 20] [--reps 5] [--warmup 2] [--step-timeout 240] [--out FILE]
    python3 tools/bench_fri_ml_grouped.py --case open:FIELD:D ...          one case in this process"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_fri_ml_arity import emit, setup, split, timed              # noqa: E402


def run_open(field, d, a):
    import numpy as np
    zk = setup()
    sync = zk.lib().zk_device_synchronize
    b, f, Q = 2, 6, 64
    coset = zk.from_ints(field, [0x5EED])[0]
    table = zk.MultilinearPolynomial.random(field, 1 << d, 0xB00 + 16 * d + field)
    pts = np.stack([zk.from_ints(field, [0x1234567 + 977 * i + 31337 * k for i in range(d)]) for k in range(2)])
    commit_ms = {}
    for name, lg in (("commit", 0), ("commit_grouped", 2)):
        commit_ms[name] = timed(lambda: zk.fri.commit(table, b, coset, log_group=lg).free(), a.reps, 1, sync)
    plain, grouped = zk.fri.commit(table, b, coset), zk.fri.commit(table, b, coset, log_group=2)
    forms = {"arity1": (plain, 1), "arity2": (plain, 2), "grouped": (grouped, 2)}
    stats = {name: [] for name in forms}
    for name, (c, arity) in forms.items():
        op = zk.fri.open_multilinear_points(c, pts, f, Q, log_arity=arity)
        if op.grouped != (name == "grouped") or not zk.fri.verify_multilinear_points(c.root, pts, op):
            raise SystemExit(f"the {name} opening at d = {d} does not verify: nothing is timed")

    def run(name):
        c, arity = forms[name]
        zk.fri.open_multilinear_points(c, pts, f, Q, log_arity=arity)
        stats[name].append(zk.fri.ml_last_stats())

    wall = {name: timed(lambda: run(name), a.reps, a.warmup, sync) for name in ("grouped", "arity2", "arity1")}
    row = {"kind": "open", "field": field, "d": d, "points": 2, "log_blowup": b, "log_final": f, "queries": Q, "verified": True}
    for name in forms:
        row[name + "_wall_ms"] = round(wall[name], 4)
        row.update(split(stats[name], a.warmup, name + "_"))
        row[name + "_path_bytes"] = zk.fri.ml_sizes(d, b, f, Q, log_arity=forms[name][1], grouped=name == "grouped")[3]
    ratio = lambda key: round(row["grouped_" + key] / row["arity2_" + key], 4) if row["arity2_" + key] else None
    row.update({"commit_ms": round(commit_ms["commit"], 4), "commit_grouped_ms": round(commit_ms["commit_grouped"], 4),
                "grouped_over_arity2": ratio("wall_ms"), "trees_ratio": ratio("ms_trees"), "folds_ratio": ratio("ms_folds"),
                "sumcheck_ratio": ratio("ms_sumcheck"), "path_bytes_ratio": ratio("path_bytes")})
    emit(row, a.out)
    plain.free()
    grouped.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20,24")
    ap.add_argument("--bn254-size", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--case", default=None, help="open:FIELD:D -- run this one case here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_ml_grouped", "bench.jsonl"))
    a = ap.parse_args()
    if a.case:
        _, field, size = a.case.split(":")
        run_open(int(field), int(size), a)
        return 0
    cases = [f"open:0:{int(x)}" for x in a.sizes.split(",") if x] + ([f"open:3:{a.bn254_size}"] if a.bn254_size else [])
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
