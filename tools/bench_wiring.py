"""The permutation check over FRI commitments (zk_wiring_prove; csrc/wiring.cuh), b = 2, f = 6, Q = 64, log_arity = 2 on grouped leaves.
JSON lines (stdout, and appended to --out):
  kind = "prove"   one case (field, d): A random, B = A, C random; sigma swaps (A, x) with (B, x) for every x and fixes C: 2^d cycles of
                   length two, a satisfied wiring.  The proof is verified (zk_wiring_verify) before anything is timed.  zk_wiring_last_stats'
                   split of --reps proofs after --warmup: the medians of ms_fractions, ms_commit, ms_eq, ms_rounds, ms_opening and of the host
                   wall clock, with min / max; beside it `gate_*`: zk_zerocheck_gate_prove's split on a satisfied circuit of the same d
                   (tools/bench_zerocheck_gate.py's).  For information: there is no condition on it.
  kind = "round"   zk_wiring_round (r given: the ten tables folded, seven sums) on tables of 2^d entries against zk_zerocheck_gate_round on
                   nine of them, in the same process and alternating, device events around each call (its output allocations inside; the
                   wiring hook also copies the folded ten out of the pass's one block into the caller's tables), --reps runs after --warmup:
                   median, min, max in milliseconds.  The wiring pass makes c = 75 products for a = 60 accesses per lane, the gate pass 41
                   for 54: `bound_ratio` = max(c / 41, a / 54); `gate_spread_ms` = the gate pass's slowest less its fastest run;
                   `within_bound` = wiring median <= bound_ratio x gate median + gate_spread_ms.
Cases: BLS12-381 Fr at --sizes, BN254 Fr once at --bn254-size.  Without --case the tool runs every case as a fresh child process of its own,
each under `timeout`, one after the other, and stops at the first one that fails: a case that faults or hangs starts nothing after it.
    python3 tools/bench_wiring.py [--sizes 20,24] [--bn254-size 20] [--round-size 24] [--reps 5] [--warmup 2] [--step-timeout 400] [--out FILE]
    python3 tools/bench_wiring.py --case FIELD:D ...          one case in this process"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G                                            # noqa: E402

PRODUCTS, ACCESSES, GATE_PRODUCTS, GATE_ACCESSES = 75, 60, 41, 54


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def three(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def index_table(zk, field, first, n):
    """the table first, first + 1, .. as field elements on the device"""
    canon = np.zeros((n, 4), np.uint64)
    canon[:, 0] = np.arange(first, first + n, dtype=np.uint64)
    out = np.zeros_like(canon)
    assert zk.lib().zk_vec_from_canonical(field, canon.ctypes.data_as(zk._lib.u64p), n, out.ctypes.data_as(zk._lib.u64p)) == 0
    return zk.MultilinearPolynomial(field, out)


def run_case(field, d, a):
    import torch
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    MP, lib = zk.MultilinearPolynomial, zk.lib()
    sync = lib.zk_device_synchronize
    b, f, Q, la, lg = 2, 6, 64, 2, 2
    n = 1 << d
    rand = lambda j: MP.random(field, n, 0xD00 + 256 * j + 16 * d + field)
    A, Cc = rand(0), rand(1)
    B = A.clone()
    sig = [index_table(zk, field, n, n), index_table(zk, field, 0, n), index_table(zk, field, 2 * n, n)]
    coset = zk.from_ints(field, [0x5EED])[0]
    cms = [zk.fri.commit(t, b, coset, log_group=lg) for t in [A, B, Cc] + sig]
    roots = [c.root for c in cms]

    pr = zk.wiring.prove(cms[:3], cms[3:], f, Q, log_arity=la)
    if not zk.wiring.verify(roots, pr):
        raise SystemExit(f"the wiring proof at d = {d} does not verify: nothing is timed")
    stats, wall = [], []
    for i in range(a.warmup + a.reps):
        sync(); t0 = time.perf_counter()
        zk.wiring.prove(cms[:3], cms[3:], f, Q, log_arity=la)
        sync(); w = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            wall.append(w)
            stats.append(zk.wiring.last_stats())
    for c in cms:
        c.free()
    del cms, sig
    row = {"kind": "prove", "field": field, "d": d, "log_blowup": b, "log_final": f, "queries": Q, "log_arity": la, "log_group": lg, "verified": True, "reps": a.reps,
           "wall_ms": three(wall)}
    for name in ("ms_fractions", "ms_commit", "ms_eq", "ms_rounds", "ms_opening"):
        row[name] = three([s[name] for s in stats])

    # the gate's zerocheck on a satisfied circuit of the same d, beside it
    qM, qL, qR, qC = (rand(2 + j) for j in range(4))
    mul = lambda *ts: zk.ProductPolynomial(list(ts)).multiply_polynomials_element_wise()
    one = zk.from_ints(field, [1])[0]
    qO = A.scalar_mul(zk.from_ints(field, [0])[0]).sub_scalar(one)
    add = MP.add_polynomials
    Cg = add(add(mul(qM, A, B), mul(qL, A)), add(mul(qR, B), qC))
    eight = [A, B, Cg, qM, qL, qR, qO, qC]
    gcs = [zk.fri.commit(t, b, coset, log_group=lg) for t in eight]
    pg = zk.zerocheck.prove_gate(gcs[:3], gcs[3:], f, Q, log_arity=la)
    if not zk.zerocheck.verify_gate([c.root for c in gcs], pg):
        raise SystemExit(f"the gate's zerocheck proof at d = {d} does not verify: nothing is timed")
    gstats, gwall = [], []
    for i in range(a.warmup + a.reps):
        sync(); t0 = time.perf_counter()
        zk.zerocheck.prove_gate(gcs[:3], gcs[3:], f, Q, log_arity=la)
        sync(); w = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            gwall.append(w)
            gstats.append(zk.zerocheck.last_stats())
    for c in gcs:
        c.free()
    del gcs
    row.update({"gate_wall_ms": three(gwall), "gate_ms_eq": three([s["ms_eq"] for s in gstats]), "gate_ms_rounds": three([s["ms_rounds"] for s in gstats]),
                "gate_ms_opening": three([s["ms_opening"] for s in gstats])})
    emit(row, a.out)

    if d == a.round_size:
        E, H = MP.random(field, n, 0xE00 + d), [rand(8 + j) for j in range(3)]
        ten = [A, B, Cc, qM, qL, qR] + H + [E]               # any ten tables: the pass does the same work on every input
        el = [zk.from_ints(field, [v])[0] for v in (0xB37A, 0x6A33A, 0xA1FA, 0x33)]
        r = zk.from_ints(field, [0xD33B])[0]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed(fn):
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            del out
            return e0.elapsed_time(e1)

        w_ms, g_ms = [], []
        for i in range(a.warmup + a.reps):                   # alternating: both sides meet the same neighbours on the machine
            w = timed(lambda: zk.wiring.round(ten, *el, id_base=r, log_step=1, r=r))
            g = timed(lambda: zk.zerocheck.gate_round(eight + [E], r))
            if i >= a.warmup:
                w_ms.append(w)
                g_ms.append(g)
        wt, gt = three(w_ms), three(g_ms)
        bound = max(PRODUCTS / GATE_PRODUCTS, ACCESSES / GATE_ACCESSES)
        spread = gt["max"] - gt["min"]
        emit({"kind": "round", "field": field, "d": d, "reps": a.reps, "wiring_round_ms": wt, "gate_round_ms": gt, "products": PRODUCTS, "accesses": ACCESSES,
              "wiring_over_gate": round(wt["median"] / gt["median"], 4), "bound_ratio": round(bound, 4), "gate_spread_ms": round(spread, 4),
              "within_bound": bool(wt["median"] <= bound * gt["median"] + spread),
              "note": "one pass over 2^d entries each, output allocations inside; the wiring hook also copies the folded ten (10 x 2^d / 2 entries) out of "
                      "the pass's one block into the caller's tables, which the prover's rounds do not do"}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--bn254-size", type=int, default=20)
    ap.add_argument("--round-size", type=int, default=24, help="the BLS12-381 Fr size at which the round pass is also timed on its own")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--case", default=None, help="FIELD:D -- run this one case here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wiring", "bench.jsonl"))
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
