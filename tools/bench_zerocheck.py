"""Zerocheck of a product over three FRI commitments (zk_zerocheck_mul_prove; csrc/zerocheck.cuh zerocheck_mul_round_kernel) against the path that
existed before it, b = 2, f = 6, Q = 64, log_arity = 2 on grouped leaves.  JSON lines (stdout, and appended to --out):
  kind = "prove"   one case (field, d): A, B random, C = A o B on the device; the proof is verified (zk_zerocheck_mul_verify) before anything is
                   timed.  zk_zerocheck_last_stats' split of --reps proofs after --warmup: the medians of ms_eq, ms_rounds, ms_opening and of
                   the host wall clock, and min / max of ms_rounds.  The baseline in the same process: zk_sumcheck_gkr_rounds with nprod = 2,
                   nfac = 3 on (E, A, B), (E, -C, 1) with E a random table of the same length (its values do not change the work), timed by
                   the host clock between two device synchronisations, beside its own zk_sumcheck_last_stats ms_rounds; median, min, max.
                   `rounds_over_baseline` = median ms_rounds / median baseline wall; `not_slower` = the new median is at most the
                   baseline's median plus the larger of the two max - min spreads.
  kind = "round"   zk_zerocheck_mul_round (r given: the four tables folded, four sums) on tables of 2^d entries, device events around the call
                   (its four output allocations inside), best of the runs, GB/s over 24 x 32 x q bytes, q = 2^d / 4; beside zk_fri_ml_round
                   on two of the tables, timed the same way, GB/s over its 12 x 32 x q.
Cases: BLS12-381 Fr at --sizes, BN254 Fr once at --bn254-size.  Without --case the tool runs every case as a fresh child process of its own,
each under `timeout`, one after the other, and stops at the first one that fails: a case that faults or hangs starts nothing after it.
    python3 tools/bench_zerocheck.py [--sizes 20,24] [--bn254-size 20] [--round-size 24] [--reps 5] [--warmup 2] [--step-timeout 300] [--out FILE]
    python3 tools/bench_zerocheck.py --case FIELD:D ...          one case in this process"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
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


def three(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def run_case(field, d, a):
    import numpy as np
    import torch
    zk = G.import_package()
    from zkmle_amd import _lib
    from zkmle_amd import sumcheck as S
    _lib.check(zk.lib().zk_init(0))
    MP, lib = zk.MultilinearPolynomial, zk.lib()
    sync = lib.zk_device_synchronize
    b, f, Q, la, lg = 2, 6, 64, 2, 2
    n = 1 << d
    A, B = MP.random(field, n, 0xA00 + 16 * d + field), MP.random(field, n, 0xB00 + 16 * d + field)
    Cc = zk.ProductPolynomial([A, B]).multiply_polynomials_element_wise()
    coset = zk.from_ints(field, [0x5EED])[0]
    cms = [zk.fri.commit(t, b, coset, log_group=lg) for t in (A, B, Cc)]
    roots = [c.root for c in cms]

    pr = zk.zerocheck.prove_mul(*cms, f, Q, log_arity=la)
    if not zk.zerocheck.verify_mul(roots, pr):
        raise SystemExit(f"the zerocheck proof at d = {d} does not verify: nothing is timed")
    stats, wall = [], []
    for i in range(a.warmup + a.reps):
        sync(); t0 = time.perf_counter()
        zk.zerocheck.prove_mul(*cms, f, Q, log_arity=la)
        sync(); w = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            wall.append(w)
            stats.append(zk.zerocheck.last_stats())
    for c in cms:
        c.free()

    # the baseline: the six-table form on the rounds that existed before
    E = MP.random(field, n, 0xE00 + d)
    from zkmle_amd.mle import MODULI
    pm1 = zk.from_ints(field, [MODULI[field] - 1])[0]
    negC = Cc.scalar_mul(pm1)
    ones = A.scalar_mul(zk.from_ints(field, [0])[0]).sub_scalar(pm1)   # 0 - (p - 1) = 1 at every index
    six = [E, A, B, E, negC, ones]
    arr = (C.c_void_p * 6)(*[t._h for t in six])
    co, ch = np.zeros((d, 4, 4), np.uint64), np.zeros((d, 4), np.uint64)
    decl = S._decl()
    base_wall, base_rounds = [], []
    for i in range(a.warmup + a.reps):
        t = zk.Transcript()
        sync(); t0 = time.perf_counter()
        _lib.check(decl.zk_sumcheck_gkr_rounds(arr, 2, 3, t._h, _lib.p64(co), _lib.p64(ch), None))
        sync(); w = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            base_wall.append(w)
            base_rounds.append(S.last_stats()["ms_rounds"])
    new_r, base = three([s["ms_rounds"] for s in stats]), three(base_wall)
    spread = max(new_r["max"] - new_r["min"], base["max"] - base["min"])
    emit({"kind": "prove", "field": field, "d": d, "log_blowup": b, "log_final": f, "queries": Q, "log_arity": la, "log_group": lg, "verified": True,
          "reps": a.reps, "wall_ms": three(wall), "ms_eq": three([s["ms_eq"] for s in stats]), "ms_rounds": new_r,
          "ms_opening": three([s["ms_opening"] for s in stats]), "baseline_gkr_rounds_wall_ms": base, "baseline_gkr_rounds_own_ms_rounds": three(base_rounds),
          "rounds_over_baseline": round(new_r["median"] / base["median"], 4), "spread_ms": round(spread, 4),
          "not_slower": bool(new_r["median"] <= base["median"] + spread)}, a.out)

    if d == a.round_size:
        r = zk.from_ints(field, [0xD33B])[0]
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

        q = n // 4
        zc = best_of(lambda: zk.zerocheck.mul_round(A, B, Cc, E, r))
        ml = best_of(lambda: zk.fri.ml_round(A, E, r))
        emit({"kind": "round", "field": field, "d": d, "zerocheck_round_ms": round(zc, 4), "zerocheck_round_GBps": round(24 * 32.0 * q / (zc * 1e-3) / 1e9, 1),
              "ml_round_ms": round(ml, 4), "ml_round_GBps": round(12 * 32.0 * q / (ml * 1e-3) / 1e9, 1),
              "note": "one pass over 2^d entries each, output allocations inside (four tables of 2^d / 2 entries; two for zk_fri_ml_round)"}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--bn254-size", type=int, default=20)
    ap.add_argument("--round-size", type=int, default=24, help="the BLS12-381 Fr size at which the round pass is also timed on its own")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--case", default=None, help="FIELD:D -- run this one case here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zerocheck", "bench.jsonl"))
    a = ap.parse_args()
    if a.case:
        field, d = (int(x) for x in a.case.split(":"))
        if field != 0:
            a.round_size = -1
        run_case(field, d, a)
        return 0
    cases = [(0, int(x)) for x in a.sizes.split(",") if x] + ([(3, a.bn254_size)] if a.bn254_size else [])
    for field, d in cases:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--case", f"{field}:{d}", "--reps", str(a.reps),
               "--warmup", str(a.warmup), "--round-size", str(a.round_size), "--out", a.out]
        rc = subprocess.call(cmd)
        if rc != 0:                                          # a fault, an abort or a time limit: nothing more is started on the device
            print(f"case {field}:{d} ended with status {rc}; stopping", file=sys.stderr, flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
