"""FRI polynomial commitment (csrc/fri_pcs.cuh, csrc/zkmle_fri_pcs.hip), BLS12-381 Fr, b = 2, f = 6, Q = 64.  JSON lines (stdout, and
appended to --out):
  kind = "commit"    zk_fri_commit at d: wall_ms (host clock around the call, which ends synchronised; the allocations of the codeword and
                     the tree are inside), median of --reps after --warmup
  kind = "open"      zk_fri_pcs_open of k = 1 and k = 4 commitments at d: wall_ms, zk_fri_pcs_last_stats' split (evaluations, quotient, FRI
                     proof, gather), zk_fri_last_stats' ms_trees of the FRI proof of the same quotient in the same process, the ratio
                     quotient / trees, and the quotient's achieved GB/s over its own traffic, (k + 1) x 32 x N bytes (+ 2 x 32 x N when the
                     prefix products go through memory, T = 16).  Every timed opening is verified (zk_fri_pcs_verify) first.
  kind = "quotient"  zk_fri_pcs_quotient alone at d and k with every T forced (ZK_FRI_PCS_BATCH): device-event ms and GB/s per T, and the T
                     the library picks by itself
    python3 tools/bench_fri_pcs.py [--sizes 16,20,24] [--reps 5] [--warmup 2] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G                                            # noqa: E402


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def wall_median(fn, reps, warmup, sync):
    for _ in range(warmup):
        fn()
    wall = []
    for _ in range(reps):
        sync(); t0 = time.perf_counter()
        fn()
        sync(); wall.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20,24")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_pcs", "bench_fri_pcs.jsonl"))
    a = ap.parse_args()
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    MP, lib = zk.MultilinearPolynomial, zk.lib()
    sync = lib.zk_device_synchronize
    field, b, f, Q = 0, 2, 6, 64
    cm, z, gamma = (zk.from_ints(field, [v])[0] for v in (0x5EED, 0xD33B, 0x6A33A))
    for d in [int(x) for x in a.sizes.split(",")]:
        n_dom = 1 << (d + b)
        polys = [MP.random(field, 1 << d, 0xA00 + 16 * d + j) for j in range(4)]
        held = []

        def commit_once():
            held.clear()                                                 # the previous commitment is freed inside the timed call, as a user would
            held.append(zk.fri.commit(polys[0], b, cm))

        emit({"kind": "commit", "d": d, "log_blowup": b, "wall_ms": round(wall_median(commit_once, a.reps, a.warmup, sync), 4)}, a.out)
        held.clear()
        cms = [zk.fri.commit(q, b, cm) for q in polys]
        for k in (1, 4):
            op = zk.fri.open_at(cms[:k], z, f, Q)
            if not zk.fri.verify_opening(field, [c.root for c in cms[:k]], z, op, d, b, f, Q, coset=cm):
                raise SystemExit(f"the opening at d = {d}, k = {k} does not verify: nothing is timed")
            stats = []

            def run():
                zk.fri.open_at(cms[:k], z, f, Q)
                stats.append((zk.fri.pcs_last_stats(), zk.fri.last_stats()))

            wall = wall_median(run, a.reps, a.warmup, sync)
            med = lambda which, key: statistics.median(s[which][key] for s in stats[a.warmup:])
            st = {key: round(med(0, key), 4) for key in ("ms_evals", "ms_quotient", "ms_fri", "ms_gather", "ms_total")}
            batch, trees = stats[-1][0]["batch"], med(1, "ms_trees")
            traffic = ((k + 1) + (2 if batch == 16 else 0)) * 32.0 * n_dom
            emit({"kind": "open", "d": d, "k": k, "log_blowup": b, "log_final": f, "queries": Q, "verified": True, "wall_ms": round(wall, 4), **st,
                  "batch": batch, "fri_ms_trees": round(trees, 4), "quotient_over_trees": round(st["ms_quotient"] / trees, 4),
                  "quotient_GBps": round(traffic / (st["ms_quotient"] * 1e-3) / 1e9, 1)}, a.out)
            ys = op.ys
            row = {"kind": "quotient", "d": d, "k": k}
            for T in (None, 1, 2, 4, 8, 16):
                if T is None:
                    os.environ.pop("ZK_FRI_PCS_BATCH", None)
                else:
                    os.environ["ZK_FRI_PCS_BATCH"] = str(T)
                ms = []
                for r in range(a.warmup + a.reps):
                    zk.fri.quotient(cms[:k], z, ys, gamma)
                    ms.append(zk.fri.pcs_last_stats()["ms_quotient"])
                m = statistics.median(ms[a.warmup:])
                if T is None:
                    row["picked"] = zk.fri.pcs_last_stats()["batch"]
                    row["picked_ms"] = round(m, 4)
                else:
                    row[f"T{T}_ms"] = round(m, 4)
                    row[f"T{T}_GBps"] = round(((k + 1) + (2 if T == 16 else 0)) * 32.0 * n_dom / (m * 1e-3) / 1e9, 1)
            os.environ.pop("ZK_FRI_PCS_BATCH", None)
            emit(row, a.out)
        for c in cms:
            c.free()
        del polys
        _lib.check(lib.zk_release_cached_memory())


if __name__ == "__main__":
    main()
