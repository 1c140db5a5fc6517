"""Multilinear opening of a FRI commitment (csrc/fri_ml.cuh, csrc/zkmle_fri_ml.hip), BLS12-381 Fr, b = 2, f = 6, Q = 64.  JSON lines
(stdout, and appended to --out):
  kind = "fold"   zk_fri_ml_fold against zk_fri_fold on the same codeword in the same run at --fold-sizes (log2 of the codeword length), with
                  and without a coset: device-event ms of the call (allocation of the output inside both), the ratio, and GB/s over the
                  fold's own traffic, 1.5 x 32 x len bytes
  kind = "open"   zk_fri_ml_open at d: wall_ms and zk_fri_ml_last_stats' split, against zk_fri_prove_codeword on the same codeword
                  (zk_fri_last_stats) and zk_fri_pcs_open with k = 1 (zk_fri_pcs_last_stats) in the same process.  Every timed opening is
                  verified (zk_fri_ml_verify) first.
    python3 tools/bench_fri_ml.py [--sizes 16,20,24] [--fold-sizes 20,22,24] [--reps 5] [--warmup 2] [--out FILE]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20,24")
    ap.add_argument("--fold-sizes", default="20,22,24")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_ml", "bench_fri_ml.jsonl"))
    a = ap.parse_args()
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    MP, lib = zk.MultilinearPolynomial, zk.lib()
    sync = lib.zk_device_synchronize
    field, b, f, Q = 0, 2, 6, 64
    cm, r = (zk.from_ints(field, [v])[0] for v in (0x5EED, 0xD33B))

    for loglen in [int(x) for x in a.fold_sizes.split(",") if x]:
        cw = MP.random(field, 1 << loglen, 0xF01D + loglen)
        for coset in (None, cm):
            ml = timed(lambda: zk.fri.ml_fold(cw, r, coset), a.reps, a.warmup, sync)
            mono = timed(lambda: zk.fri.fold(cw, r, coset), a.reps, a.warmup, sync)
            traffic = 1.5 * 32.0 * (1 << loglen)
            emit({"kind": "fold", "log_len": loglen, "coset": coset is not None, "ml_fold_ms": round(ml, 4), "fri_fold_ms": round(mono, 4),
                  "ml_over_fri": round(ml / mono, 4), "ml_fold_GBps": round(traffic / (ml * 1e-3) / 1e9, 1),
                  "fri_fold_GBps": round(traffic / (mono * 1e-3) / 1e9, 1)}, a.out)
        del cw
        _lib.check(lib.zk_release_cached_memory())

    for d in [int(x) for x in a.sizes.split(",") if x]:
        table = MP.random(field, 1 << d, 0xA00 + 16 * d)
        c = zk.fri.commit(table, b, cm)
        z = zk.from_ints(field, [0x1234567 + 977 * i for i in range(d)])
        op = zk.fri.open_multilinear(c, z, f, Q)
        if not zk.fri.verify_multilinear(c.root, z, op):
            raise SystemExit(f"the opening at d = {d} does not verify: nothing is timed")
        stats = []

        def run_ml():
            zk.fri.open_multilinear(c, z, f, Q)
            stats.append(zk.fri.ml_last_stats())

        wall = timed(run_ml, a.reps, a.warmup, sync)
        st = {key: round(statistics.median(s[key] for s in stats[a.warmup:]), 4) for key in ("ms_sumcheck", "ms_folds", "ms_trees", "ms_queries", "ms_total")}
        cw = c.codeword()
        fstats = []

        def run_fri():
            zk.fri.prove_codeword(cw, b, f, Q, cm)
            fstats.append(zk.fri.last_stats())

        fri_wall = timed(run_fri, a.reps, a.warmup, sync)
        fri = {"fri_" + key: round(statistics.median(s[key] for s in fstats[a.warmup:]), 4) for key in ("ms_trees", "ms_folds", "ms_queries", "ms_total")}
        del cw
        zp = zk.from_ints(field, [0xD33B])[0]
        pstats = []

        def run_pcs():
            zk.fri.open_at([c], zp, f, Q)
            pstats.append(zk.fri.pcs_last_stats())

        pcs_wall = timed(run_pcs, a.reps, a.warmup, sync)
        pcs = {"pcs_" + key: round(statistics.median(s[key] for s in pstats[a.warmup:]), 4) for key in ("ms_evals", "ms_quotient", "ms_fri", "ms_gather", "ms_total")}
        emit({"kind": "open", "d": d, "log_blowup": b, "log_final": f, "queries": Q, "verified": True, "wall_ms": round(wall, 4), **st,
              "fri_prove_codeword_wall_ms": round(fri_wall, 4), **fri, "pcs_open_k1_wall_ms": round(pcs_wall, 4), **pcs,
              "ml_over_fri_prove_codeword": round(wall / fri_wall, 4), "ml_over_pcs_open": round(wall / pcs_wall, 4)}, a.out)
        c.free()
        del table
        _lib.check(lib.zk_release_cached_memory())


if __name__ == "__main__":
    main()
