"""The lookup argument over FRI commitments (zk_lookup_prove; csrc/lookup.cuh), b = 2, f = 6, Q = 64, log_arity = 2 on grouped leaves.
JSON lines (stdout, and appended to --out):
  kind = "prove"   one case (field, d, table): `random`: T0, T1, T2 random, A, B, C their copies (row x looks up row x: every multiplicity is
                   1) and qK all ones; `all-equal`: the three columns constant, every witness row that one triple (M[0] = 2^d: the contended
                   case).  The proof is verified (zk_lookup_verify) before anything is timed.  zk_lookup_last_stats' split of --reps proofs
                   after --warmup: the medians of ms_multiplicities, ms_fractions, ms_commit (two commitments), ms_eq, ms_rounds, ms_opening
                   and of the host wall clock, with min / max.  For information.  On the random table, beside it and alternating in the same
                   process: zk_wiring_prove on commitments of the same shape (A, a copy of A, C and a sigma that swaps the first two wires row
                   by row), also verified first: `wiring_ms_rounds`, and
                       `rounds_within_margin` = lookup's median ms_rounds <= wiring's median ms_rounds + (wiring's max - min).
  kind = "round"   zk_lookup_round (r given: the ten tables folded, seven sums) on ten random tables of 2^d entries against zk_wiring_round on
                   the same ten, in the same process and alternating, device events around each call (output allocations and the copies of the
                   folded ten out of the pass's one block inside, for both), --reps runs after --warmup: median, min, max in milliseconds.
                   Both passes move 60 accesses of 32 bytes per lane; the lookup's makes 47 products, the wiring's 75.
                       `within_margin` = lookup's median <= wiring's median + (wiring's max - min).
Without --case the tool runs every case as a fresh child process of its own, each under `timeout`, one after the other, and stops at the first
one that fails: a case that faults or hangs starts nothing after it.
    python3 tools/bench_lookup.py [--sizes 20,24] [--round-size 24] [--reps 5] [--warmup 2] [--step-timeout 400] [--out FILE]
    python3 tools/bench_lookup.py --case D ...          one size in this process"""
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

FIELD = 0
PRODUCTS, WIRING_PRODUCTS, ACCESSES = 47, 75, 60


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


def run_case(d, a):
    import torch
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    field = FIELD
    MP, lib = zk.MultilinearPolynomial, zk.lib()
    sync = lib.zk_device_synchronize
    b, f, Q, la, lg = 2, 6, 64, 2, 2
    n = 1 << d
    rand = lambda j: MP.random(field, n, 0x10C + 256 * j + 16 * d + field)
    el = lambda v: zk.from_ints(field, [v])[0]
    const = lambda t, v: t.scalar_mul(el(0)).sub_scalar(el(-v))          # the table that holds v everywhere
    coset = el(0x5EED)
    commit = lambda t: zk.fri.commit(t, b, coset, log_group=lg)
    base = {"field": field, "d": d, "log_blowup": b, "log_final": f, "queries": Q, "log_arity": la, "log_group": lg, "verified": True, "reps": a.reps}
    names = ("ms_multiplicities", "ms_fractions", "ms_commit", "ms_eq", "ms_rounds", "ms_opening")

    T = [rand(j) for j in range(3)]
    qK = const(T[0], 1)
    cq = commit(qK)
    cT = [commit(t) for t in T]
    cW = [commit(t.clone()) for t in T]                       # A, B, C: row x holds table row x
    look = cW + [cq] + cT
    sig = [index_table(zk, field, n, n), index_table(zk, field, 0, n), index_table(zk, field, 2 * n, n)]
    cS = [commit(t) for t in sig]
    del sig
    wires = [cW[0], cT[0], cW[2]]                             # the second wire holds the first one's values: sigma swaps them row by row

    pr = zk.lookup.prove(look[:3], look[3], look[4:], f, Q, log_arity=la)
    if zk.lookup.last_stats()["misses"] or not zk.lookup.verify([c.root for c in look], pr):
        raise SystemExit(f"the lookup proof at d = {d} does not verify: nothing is timed")
    pw = zk.wiring.prove(wires, cS, f, Q, log_arity=la)
    if not zk.wiring.verify([c.root for c in wires + cS], pw):
        raise SystemExit(f"the wiring proof at d = {d} does not verify: nothing is timed")
    del pr, pw
    stats, wall, wstats = [], [], []
    for i in range(a.warmup + a.reps):                       # alternating: both provers meet the same neighbours on the machine
        sync(); t0 = time.perf_counter()
        zk.lookup.prove(look[:3], look[3], look[4:], f, Q, log_arity=la)
        sync(); w = (time.perf_counter() - t0) * 1e3
        st = zk.lookup.last_stats()
        zk.wiring.prove(wires, cS, f, Q, log_arity=la)
        ws = zk.wiring.last_stats()
        if i >= a.warmup:
            wall.append(w)
            stats.append(st)
            wstats.append(ws)
    row = dict(base, kind="prove", table="random", wall_ms=three(wall))
    for name in names:
        row[name] = three([s[name] for s in stats])
    wr = three([s["ms_rounds"] for s in wstats])
    margin = wr["max"] - wr["min"]
    row.update({"wiring_ms_rounds": wr, "wiring_spread_ms": round(margin, 4), "rounds_within_margin": bool(row["ms_rounds"]["median"] <= wr["median"] + margin)})
    emit(row, a.out)
    for c in cW + cT + cS:
        c.free()
    del cW, cT, cS, look, wires

    # the contended case: a table that is one row, every witness row hitting it
    cols = [const(T[0], 0xA11 + j) for j in range(3)]
    cT = [commit(t) for t in cols]
    cW = [commit(t.clone()) for t in cols]
    look = cW + [cq] + cT
    pr = zk.lookup.prove(look[:3], look[3], look[4:], f, Q, log_arity=la)
    if zk.lookup.last_stats()["misses"] or not zk.lookup.verify([c.root for c in look], pr):
        raise SystemExit(f"the lookup proof on the all-equal table at d = {d} does not verify: nothing is timed")
    del pr
    stats, wall = [], []
    for i in range(a.warmup + a.reps):
        sync(); t0 = time.perf_counter()
        zk.lookup.prove(look[:3], look[3], look[4:], f, Q, log_arity=la)
        sync(); w = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            wall.append(w)
            stats.append(zk.lookup.last_stats())
    row = dict(base, kind="prove", table="all-equal", wall_ms=three(wall))
    for name in names:
        row[name] = three([s[name] for s in stats])
    emit(row, a.out)
    for c in look:
        c.free()
    del cW, cT, look, cols

    if d == a.round_size:
        ten = T + [rand(3 + j) for j in range(7)]            # any ten tables: both passes do the same work on every input
        els = [el(v) for v in (0xB37A, 0x6A33A, 0xA1FA, 0x33)]
        r = el(0xD33B)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed(fn):
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            del out
            return e0.elapsed_time(e1)

        l_ms, w_ms = [], []
        for i in range(a.warmup + a.reps):
            lm = timed(lambda: zk.lookup.round(ten, els[0], els[1], els[3], r=r))
            wm = timed(lambda: zk.wiring.round(ten, *els, id_base=r, log_step=1, r=r))
            if i >= a.warmup:
                l_ms.append(lm)
                w_ms.append(wm)
        lt, wt = three(l_ms), three(w_ms)
        margin = wt["max"] - wt["min"]
        emit({"kind": "round", "field": field, "d": d, "reps": a.reps, "lookup_round_ms": lt, "wiring_round_ms": wt, "products": PRODUCTS,
              "wiring_products": WIRING_PRODUCTS, "accesses": ACCESSES, "lookup_over_wiring": round(lt["median"] / wt["median"], 4),
              "wiring_spread_ms": round(margin, 4), "within_margin": bool(lt["median"] <= wt["median"] + margin),
              "note": "one pass over 2^d entries each, output allocations inside; both hooks copy the folded ten (10 x 2^d / 2 entries) out of the pass's "
                      "one block into the caller's tables, which the provers' rounds do not do"}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--round-size", type=int, default=24, help="the size at which the round pass is also timed on its own")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--case", type=int, default=None, help="D -- run this one size here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup", "bench.jsonl"))
    a = ap.parse_args()
    if a.case is not None:
        run_case(a.case, a)
        return 0
    for d in [int(x) for x in a.sizes.split(",") if x]:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--case", str(d), "--reps", str(a.reps),
               "--warmup", str(a.warmup), "--round-size", str(a.round_size), "--out", a.out]
        rc = subprocess.call(cmd)
        if rc != 0:                                          # a fault, an abort or a time limit: nothing more is started on the device
            print(f"case {d} ended with status {rc}; stopping", file=sys.stderr, flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
