"""Zerocheck of a Plonk gate over eight FRI commitments (zk_zerocheck_gate_prove; csrc/zerocheck.cuh zerocheck_gate_round_kernel), b = 2, f = 6,
Q = 64, log_arity = 2 on grouped leaves.  JSON lines (stdout, and appended to --out):
  kind = "prove"   one case (field, d): A, B, qM, qL, qR, qC random, qO = p - 1 everywhere and C = qM A B + qL A + qR B + qC on the device, a
                   satisfied circuit; the proof is verified (zk_zerocheck_gate_verify) before anything is timed.  zk_zerocheck_last_stats'
                   split of --reps proofs after --warmup: the medians of ms_eq, ms_rounds, ms_opening and of the host wall clock, with
                   min / max.  For information: there is no condition on it.
  kind = "round"   zk_zerocheck_gate_round (r given: the nine tables folded, five sums) on tables of 2^d entries against
                   zk_zerocheck_mul_round on four of them, in the same process and alternating, device events around each call (its output
                   allocations inside), --reps runs after --warmup: median, min, max in milliseconds, and GB/s of the median over
                   54 x 32 x q bytes (gate) and 24 x 32 x q (mul), q = 2^d / 4.  The gate pass makes 41 products for 54 accesses (42 bytes a
                   product), the mul pass 16 for 24 (48): `expected_ratio` = 42 / 48 of the mul pass's bytes per second.
                   `gate_over_mul` = the ratio of the two GB/s; `mul_spread_GBps` = the mul pass's GB/s at its fastest less at its slowest
                   run; `as_expected` = gate GB/s >= expected_ratio x mul GB/s - mul_spread_GBps.
Cases: BLS12-381 Fr at --sizes, BN254 Fr once at --bn254-size.  Without --case the tool runs every case as a fresh child process of its own,
each under `timeout`, one after the other, and stops at the first one that fails: a case that faults or hangs starts nothing after it.
    python3 tools/bench_zerocheck_gate.py [--sizes 20,24] [--bn254-size 20] [--round-size 24] [--reps 5] [--warmup 2] [--step-timeout 300] [--out FILE]
    python3 tools/bench_zerocheck_gate.py --case FIELD:D ...          one case in this process"""
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
    import torch
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    MP, lib = zk.MultilinearPolynomial, zk.lib()
    sync = lib.zk_device_synchronize
    b, f, Q, la, lg = 2, 6, 64, 2, 2
    n = 1 << d
    rand = lambda j: MP.random(field, n, 0xC00 + 256 * j + 16 * d + field)
    A, B, qM, qL, qR, qC = (rand(j) for j in range(6))
    mul = lambda *ts: zk.ProductPolynomial(list(ts)).multiply_polynomials_element_wise()
    one = zk.from_ints(field, [1])[0]
    qO = A.scalar_mul(zk.from_ints(field, [0])[0]).sub_scalar(one)    # 0 - 1 = p - 1 at every index
    add = MP.add_polynomials
    Cc = add(add(mul(qM, A, B), mul(qL, A)), add(mul(qR, B), qC))      # qO C = -C cancels the rest
    eight = [A, B, Cc, qM, qL, qR, qO, qC]
    coset = zk.from_ints(field, [0x5EED])[0]
    cms = [zk.fri.commit(t, b, coset, log_group=lg) for t in eight]
    roots = [c.root for c in cms]

    pr = zk.zerocheck.prove_gate(cms[:3], cms[3:], f, Q, log_arity=la)
    if not zk.zerocheck.verify_gate(roots, pr):
        raise SystemExit(f"the gate's zerocheck proof at d = {d} does not verify: nothing is timed")
    stats, wall = [], []
    for i in range(a.warmup + a.reps):
        sync(); t0 = time.perf_counter()
        zk.zerocheck.prove_gate(cms[:3], cms[3:], f, Q, log_arity=la)
        sync(); w = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            wall.append(w)
            stats.append(zk.zerocheck.last_stats())
    for c in cms:
        c.free()
    emit({"kind": "prove", "field": field, "d": d, "log_blowup": b, "log_final": f, "queries": Q, "log_arity": la, "log_group": lg, "verified": True,
          "reps": a.reps, "wall_ms": three(wall), "ms_eq": three([s["ms_eq"] for s in stats]), "ms_rounds": three([s["ms_rounds"] for s in stats]),
          "ms_opening": three([s["ms_opening"] for s in stats])}, a.out)

    if d == a.round_size:
        E = MP.random(field, n, 0xE00 + d)
        r = zk.from_ints(field, [0xD33B])[0]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed(fn):
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            del out
            return e0.elapsed_time(e1)

        gate_ms, mul_ms = [], []
        for i in range(a.warmup + a.reps):                   # alternating: both sides meet the same neighbours on the machine
            g = timed(lambda: zk.zerocheck.gate_round(eight + [E], r))
            m = timed(lambda: zk.zerocheck.mul_round(A, B, Cc, E, r))
            if i >= a.warmup:
                gate_ms.append(g)
                mul_ms.append(m)
        q = n // 4
        gbps = lambda accesses, ms: accesses * 32.0 * q / (ms * 1e-3) / 1e9
        gt, mt = three(gate_ms), three(mul_ms)
        gate_gbps, mul_gbps = gbps(54, gt["median"]), gbps(24, mt["median"])
        spread = gbps(24, mt["min"]) - gbps(24, mt["max"])
        expected = 42.0 / 48.0
        emit({"kind": "round", "field": field, "d": d, "reps": a.reps, "gate_round_ms": gt, "gate_round_GBps": round(gate_gbps, 1), "mul_round_ms": mt,
              "mul_round_GBps": round(mul_gbps, 1), "gate_over_mul": round(gate_gbps / mul_gbps, 4), "expected_ratio": round(expected, 4),
              "mul_spread_GBps": round(spread, 1), "as_expected": bool(gate_gbps >= expected * mul_gbps - spread),
              "note": "one pass over 2^d entries each, output allocations inside (nine tables of 2^d / 2 entries; four for zk_zerocheck_mul_round)"}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--bn254-size", type=int, default=20)
    ap.add_argument("--round-size", type=int, default=24, help="the BLS12-381 Fr size at which the round pass is also timed on its own")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--case", default=None, help="FIELD:D -- run this one case here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zerocheck_gate", "bench.jsonl"))
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
