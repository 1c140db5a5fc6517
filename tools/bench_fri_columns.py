"""Column commitments (zk_fri_commit_columns, zk_fri_ml_open_columns_pow; csrc/merkle_columns.cuh) against the same tables committed and opened
one tree each: BLS12-381 Fr, b = 2, f = 6, Q = 64.  JSON lines (stdout, and appended to --out):
  kind = "commit"  one case (d, k): in ONE process zk_fri_commit_columns of k tables alternates with k calls of zk_fri_commit_grouped(.., 2) on
                   the same tables, --reps times after --warmup: the median, min and max host wall clock of each between two device
                   synchronisations (allocations and frees of the commitment inside), every timed call's milliseconds, the median split of
                   zk_fri_columns_last_stats (the k transforms, the leaf launch, the node launches), and the permutation counts
                   (B(k) + 1) N / 4 against 2 k N / 4.  First a columns commitment is opened at 2 points with 8 queries and verified.
  kind = "open"    one case d: the opening of four column commitments of widths 12, 3, 1, 4 alternates with open_multilinear_batch_wide of
                   twenty grouped commitments of the same tables at the same point: median, min, max wall_ms of each with
                   zk_fri_ml_last_stats' split, and the proof's path bytes and whole bytes of each by zk_fri_ml_sizes_columns and
                   zk_fri_ml_sizes_batch_wide.  Both openings are verified first.
  kind = "leaf"    the tree alone at N = 2^LOG, k = 4: merkle.columns_root of four tables alternates with four merkle_root(t, log_group=2):
                   median, min, max wall_ms of the whole root-only call (leaf launch, node launches, one 32-byte download).  The leaf
                   kernels' own times come from a kernel trace of this case, taken in a run of its own.
Without --case the tool runs every case as a fresh child process of its own, each under `timeout`, one after the other, and stops at the
first one that fails: a case that faults or hangs starts nothing after it.
    python3 tools/bench_fri_columns.py [--sizes 20,24] [--ks 3,4,11] [--open-sizes 20,24] [--leaf-sizes 26] [--reps 5] [--warmup 2]
                                       [--step-timeout 300] [--out FILE]
    python3 tools/bench_fri_columns.py --case commit:D:K | open:D | leaf:LOG ...          one case in this process"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_fri_ml_arity import KEYS, emit, setup              # noqa: E402

FIELD, B, F, Q = 0, 2, 6, 64
WIDTHS = (12, 3, 1, 4)
COLUMN_KEYS = ("ms_extend", "ms_leaves", "ms_nodes", "ms_total")


def blocks(k):
    return (1 + 128 * k) // 136 + 1


def alternate(fns, reps, warmup, sync):
    """{name: [wall ms]}: the calls in turn, each between two device synchronisations; the warm-up rounds are dropped"""
    walls = {name: [] for name, _ in fns}
    for rep in range(warmup + reps):
        for name, fn in fns:
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if rep >= warmup:
                walls[name].append((time.perf_counter() - t0) * 1e3)
    return walls


def summary(prefix, walls):
    return {prefix + "_ms": round(statistics.median(walls), 4), prefix + "_min_ms": round(min(walls), 4), prefix + "_max_ms": round(max(walls), 4),
            prefix + "_all_ms": [round(w, 4) for w in walls]}


def points(zk, d, P):
    import numpy as np
    return np.stack([zk.from_ints(FIELD, [0x1234567 + 977 * i + 31337 * p for i in range(d)]) for p in range(P)])


def run_commit(d, k, a):
    zk = setup()
    sync = zk.lib().zk_device_synchronize
    coset = zk.from_ints(FIELD, [0x5EED])[0]
    tables = [zk.MultilinearPolynomial.random(FIELD, 1 << d, 0xC00 + 16 * d + j) for j in range(k)]
    with zk.fri.commit_columns(tables, B, coset) as cm:
        pts = points(zk, d, 2)
        if not zk.fri.verify_columns([cm.root], [k], pts, zk.fri.open_columns([cm], pts, F, 8)):
            raise SystemExit(f"the columns commitment at d = {d}, k = {k} does not open: nothing is timed")
        if k == 1 or d <= 20:                                 # column 0 alone is the grouped commitment of table 0
            with zk.fri.commit_columns(tables[:1], B, coset) as one, zk.fri.commit(tables[0], B, coset, log_group=2) as g:
                if one.root != g.root:
                    raise SystemExit("a one-column commitment differs from the grouped one: nothing is timed")
    stats = []

    def columns():
        zk.fri.commit_columns(tables, B, coset).free()
        stats.append(zk.fri.columns_last_stats())

    def grouped():
        for t in tables:
            zk.fri.commit(t, B, coset, log_group=2).free()

    walls = alternate((("grouped", grouped), ("columns", columns)), a.reps, a.warmup, sync)
    row = {"kind": "commit", "field": FIELD, "d": d, "k": k, "log_blowup": B, "verified": True}
    row.update(summary("columns", walls["columns"]))
    row.update(summary("grouped", walls["grouped"]))
    row.update({"columns_" + key: round(statistics.median(s[key] for s in stats[a.warmup:]), 4) for key in COLUMN_KEYS})
    quarter = (1 << (d + B)) // 4
    row.update({"columns_over_grouped": round(row["columns_ms"] / row["grouped_ms"], 4), "columns_permutations": (blocks(k) + 1) * quarter,
                "grouped_permutations": 2 * k * quarter, "permutation_ratio": round((blocks(k) + 1) / (2 * k), 4)})
    emit(row, a.out)


def run_open(d, a):
    zk = setup()
    sync = zk.lib().zk_device_synchronize
    coset = zk.from_ints(FIELD, [0x5EED])[0]
    K = sum(WIDTHS)
    tables = [zk.MultilinearPolynomial.random(FIELD, 1 << d, 0xD00 + 16 * d + j) for j in range(K)]
    cols, at = [], 0
    for w in WIDTHS:
        cols.append(zk.fri.commit_columns(tables[at:at + w], B, coset))
        at += w
    singles = [zk.fri.commit(t, B, coset, log_group=2) for t in tables]
    pts = points(zk, d, 1)
    if not zk.fri.verify_columns([c.root for c in cols], WIDTHS, pts, zk.fri.open_columns(cols, pts, F, Q)):
        raise SystemExit(f"the columns opening at d = {d} does not verify: nothing is timed")
    if not zk.fri.verify_multilinear_batch_wide([c.root for c in singles], pts, zk.fri.open_multilinear_batch_wide(singles, pts, F, Q, log_arity=2)):
        raise SystemExit(f"the wide opening at d = {d} does not verify: nothing is timed")
    stats = {"columns": [], "wide": []}

    def columns():
        zk.fri.open_columns(cols, pts, F, Q)
        stats["columns"].append(zk.fri.ml_last_stats())

    def wide():
        zk.fri.open_multilinear_batch_wide(singles, pts, F, Q, log_arity=2)
        stats["wide"].append(zk.fri.ml_last_stats())

    walls = alternate((("wide", wide), ("columns", columns)), a.reps, a.warmup, sync)
    row = {"kind": "open", "field": FIELD, "d": d, "widths": list(WIDTHS), "k": K, "points": 1, "log_blowup": B, "log_final": F, "queries": Q, "verified": True}
    sizes = {"columns": zk.fri.columns_sizes(WIDTHS, d, B, F, Q), "wide": zk.fri.ml_sizes_wide(d, B, F, Q, 2, True, k=K)}
    for name in ("columns", "wide"):
        row.update(summary(name, walls[name]))
        row.update({f"{name}_{key}": round(statistics.median(s[key] for s in stats[name][a.warmup:]), 4) for key in KEYS})
        nroots, nfinal, nvalues, path_bytes, nround = sizes[name]
        row.update({name + "_path_bytes": path_bytes, name + "_proof_bytes": 32 * (nroots + nfinal + nvalues + nround + K) + path_bytes})
    row.update({"columns_over_wide": round(row["columns_ms"] / row["wide_ms"], 4), "path_bytes_ratio": round(row["columns_path_bytes"] / row["wide_path_bytes"], 4),
                "proof_bytes_ratio": round(row["columns_proof_bytes"] / row["wide_proof_bytes"], 4)})
    emit(row, a.out)
    for c in cols + singles:
        c.free()


def run_leaf(log_n, a):
    zk = setup()
    sync = zk.lib().zk_device_synchronize
    k = 4
    tables = [zk.MultilinearPolynomial.random(FIELD, 1 << log_n, 0xE00 + 16 * log_n + j) for j in range(k)]
    if zk.merkle.columns_root(tables[:1]) != zk.merkle_root(tables[0], log_group=2):
        raise SystemExit("a one-column tree differs from the grouped one: nothing is timed")
    walls = alternate((("grouped", lambda: [zk.merkle_root(t, log_group=2) for t in tables]), ("columns", lambda: zk.merkle.columns_root(tables))), a.reps, a.warmup, sync)
    row = {"kind": "leaf", "field": FIELD, "log_len": log_n, "k": k, "verified": True}
    row.update(summary("columns", walls["columns"]))
    row.update(summary("grouped", walls["grouped"]))
    quarter = (1 << log_n) // 4
    row.update({"columns_over_grouped": round(row["columns_ms"] / row["grouped_ms"], 4), "columns_leaf_permutations": blocks(k) * quarter,
                "grouped_leaf_permutations": k * quarter, "node_permutations_each_tree": quarter - 1})
    emit(row, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--ks", default="3,4,11")
    ap.add_argument("--open-sizes", default="20,24")
    ap.add_argument("--leaf-sizes", default="26")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--case", default=None, help="commit:D:K, open:D or leaf:LOG -- run this one case here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_columns", "bench.jsonl"))
    a = ap.parse_args()
    if a.case:
        kind, *rest = a.case.split(":")
        if kind == "commit":
            run_commit(int(rest[0]), int(rest[1]), a)
        elif kind == "open":
            run_open(int(rest[0]), a)
        else:
            run_leaf(int(rest[0]), a)
        return 0
    cases = [f"commit:{int(x)}:{int(k)}" for x in a.sizes.split(",") if x for k in a.ks.split(",") if k]
    cases += [f"open:{int(x)}" for x in a.open_sizes.split(",") if x]
    cases += [f"leaf:{int(x)}" for x in a.leaf_sizes.split(",") if x]
    for case in cases:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps), "--warmup", str(a.warmup),
               "--out", a.out]
        rc = subprocess.call(cmd)
        if rc != 0:                                          # a fault, an abort or a time limit: nothing more is started on the device
            print(f"case {case} ended with status {rc}; stopping", file=sys.stderr, flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
