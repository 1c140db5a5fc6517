"""The Plonk proof with lookup rows on column commitments (zk_plonk_lookup_prove_columns; csrc/plonk_helpers.cuh) against the proof on fifteen
grouped commitments of the same tables (zk_plonk_lookup_prove at log_arity = 2, unchanged), b = 2, f = 6, Q = 64.  JSON lines (stdout, and
appended to --out):
  kind = "prove"    one case (field, d): tools/bench_plonk_lookup.py's circuit with the random table -- A random, B = A, qM, qL, qR, qC random,
                    qO = -1 and C = qM A B + qL A + qR B + qC; sigma swaps (A, x) with (B, x) and fixes C; 16 public values, all zero; qK = 1 on
                    every row; T0, T1, T2 copies of A, B, C.  The tables are committed twice: as a three-column and a twelve-column commitment,
                    and as fifteen grouped commitments.  Both proofs are verified before anything is timed.  Then, alternating in one process,
                    --reps runs after --warmup of
                        columns   zk_plonk_lookup_prove_columns     (zk_plonk_lookup_columns_last_stats)
                        fifteen   zk_plonk_lookup_prove             (zk_plonk_lookup_last_stats)
                    medians with min / max of ms_multiplicities, ms_fractions, ms_commit, ms_eq, ms_rounds, ms_opening and of the host wall
                    clock; `wall_ms_quiet` / `fifteen_wall_ms_quiet` are the wall clock over the runs whose ms_commit stayed below --slow-commit
                    ms on that side (commitments of 0.8 to 1.3 s occur on both sides at d = 24) with `quiet_runs` how many those were.  Four
                    expectations, each allowed the existing side's own min .. max spread and no more:
                        fractions_below   the new ms_fractions (median) is below the existing prover's MINIMUM; fractions_ratio beside the ratio
                                          of the product counts, 0.28
                        commit_within     one column of M plus four helper columns take at most the existing five commitments
                        opening_within    the columns opening takes at most the wide opening of twenty
                        wall_within       on the quiet runs
                    and the proofs' bytes on both sides (counted from the arrays).
  kind = "helpers"  the hook zk_plonk_lookup_helpers alone at 2^LOGN entries against the four existing hooks (three zk_wiring_fractions and
                    zk_lookup_fractions) on the same random tables, alternating; the outputs are compared byte for byte first.  Host wall clock
                    around each side with a device synchronisation: every hook allocates its output, as the other side's do.
Without --case the tool runs every case as a fresh child process of its own, each under `timeout`, one after the other, and stops at the first
one that fails: a case that faults or hangs starts nothing after it.
    python3 tools/bench_plonk_lookup_columns.py [--sizes 20,24] [--bn254-size 20] [--helpers-log 24] [--reps 5] [--warmup 2] [--step-timeout 400] [--out FILE]
    python3 tools/bench_plonk_lookup_columns.py --case prove:FIELD:D | helpers:FIELD:LOGN ...          one case in this process"""
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

NPUBLIC = 16
PRODUCTS_RATIO = 0.28                                                  # about 64 products a row against about 228 (csrc/plonk_helpers.cuh)


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def three(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)} if xs else None


def index_table(zk, field, first, n):
    """the table first, first + 1, .. as field elements on the device"""
    canon = np.zeros((n, 4), np.uint64)
    canon[:, 0] = np.arange(first, first + n, dtype=np.uint64)
    out = np.zeros_like(canon)
    assert zk.lib().zk_vec_from_canonical(field, canon.ctypes.data_as(zk._lib.u64p), n, out.ctypes.data_as(zk._lib.u64p)) == 0
    return zk.MultilinearPolynomial(field, out)


def circuit_tables(zk, field, d):
    """the fifteen device tables of a satisfied circuit whose every row is a lookup row"""
    MP = zk.MultilinearPolynomial
    n = 1 << d
    el = lambda v: zk.from_ints(field, [v])[0]
    rand = lambda j: MP.random(field, n, 0xF00 + 256 * j + 16 * d + field)
    qM, qL, qR = (rand(2 + j) for j in range(3))
    zero = qM.scalar_mul(el(0))
    mul = lambda *ts: zk.ProductPolynomial(list(ts)).multiply_polynomials_element_wise()
    add = MP.add_polynomials
    qO = zero.sub_scalar(el(1))
    A, qC = rand(0), rand(5)
    B = A.clone()
    Cc = add(add(mul(qM, A, B), mul(qL, A)), add(mul(qR, B), qC))
    qK = zero.sub_scalar(qO.evaluated_values[0])              # 0 - (-1) = 1 on every row
    sig = [index_table(zk, field, n, n), index_table(zk, field, 0, n), index_table(zk, field, 2 * n, n)]
    return [A, B, Cc, qM, qL, qR, qO, qC] + sig + [qK, A.clone(), B.clone(), Cc.clone()]


def run_prove(field, d, a):
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    sync = zk.lib().zk_device_synchronize
    b, f, Q, la, lg = 2, 6, 64, 2, 2
    coset = zk.from_ints(field, [0x5EED])[0]
    fifteen = circuit_tables(zk, field, d)
    wit, cir = zk.fri.commit_columns(fifteen[:3], b, coset), zk.fri.commit_columns(fifteen[3:], b, coset)
    cms = [zk.fri.commit(t, b, coset, log_group=lg) for t in fifteen]
    del fifteen
    roots = [c.root for c in cms]
    pub = np.zeros((NPUBLIC, 4), np.uint64)
    wires, sels, sigs, ksel, cols = cms[:3], cms[3:8], cms[8:11], cms[11], cms[12:]
    new = lambda: zk.plonk_lookup.prove_columns(wit, cir, pub, f, Q)
    old = lambda: zk.plonk_lookup.prove(wires, sels, sigs, ksel, cols, pub, f, Q, log_arity=la)

    pr = new()
    if not zk.plonk_lookup.verify_columns(wit.root, cir.root, pub, pr) or zk.plonk_lookup.columns_last_stats()["misses"]:
        raise SystemExit(f"the proof on column commitments at d = {d} does not verify: nothing is timed")
    po = old()
    if not zk.plonk_lookup.verify(roots, pub, po) or zk.plonk_lookup.last_stats()["misses"]:
        raise SystemExit(f"the proof on fifteen commitments at d = {d} does not verify: nothing is timed")
    nbytes = lambda q: sum(x.nbytes for x in (q.h_roots, q.round_polys, q.ys, q.opening.round_polys, q.opening.roots, q.opening.final_table, q.opening.query_values,
                                              q.opening.query_paths))
    row = {"kind": "prove", "field": field, "d": d, "log_blowup": b, "log_final": f, "queries": Q, "npublic": NPUBLIC, "verified": True, "reps": a.reps,
           "helpers_batch": zk.plonk_lookup.helpers_batch(), "proof_bytes": nbytes(pr), "fifteen_proof_bytes": nbytes(po), "path_bytes": int(pr.opening.query_paths.nbytes),
           "fifteen_path_bytes": int(po.opening.query_paths.nbytes)}
    del pr, po
    ns, nw, os_, ow = [], [], [], []
    for i in range(a.warmup + a.reps):                       # alternating: both sides meet the same neighbours on the machine
        sync(); t0 = time.perf_counter()
        new()
        sync(); w = (time.perf_counter() - t0) * 1e3
        st = zk.plonk_lookup.columns_last_stats()
        sync(); t0 = time.perf_counter()
        old()
        sync(); w2 = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            ns.append(st); nw.append(w); os_.append(zk.plonk_lookup.last_stats()); ow.append(w2)
    for c in cms + [wit, cir]:
        c.free()
    row.update(wall_ms=three(nw), fifteen_wall_ms=three(ow))
    for name in ("ms_multiplicities", "ms_fractions", "ms_commit", "ms_eq", "ms_rounds", "ms_opening"):
        row[name] = three([s[name] for s in ns])
        row["fifteen_" + name] = three([s[name] for s in os_])
    quiet_n = [w for w, s in zip(nw, ns) if s["ms_commit"] < a.slow_commit]
    quiet_o = [w for w, s in zip(ow, os_) if s["ms_commit"] < a.slow_commit]
    row.update(wall_ms_quiet=three(quiet_n), fifteen_wall_ms_quiet=three(quiet_o), quiet_runs=[len(quiet_n), len(quiet_o)], slow_commit_ms=a.slow_commit)
    within = lambda mine, theirs: bool(mine and theirs and mine["median"] <= theirs["median"] + (theirs["max"] - theirs["min"]))
    row.update(fractions_below=bool(row["ms_fractions"]["median"] < row["fifteen_ms_fractions"]["min"]),
               fractions_ratio=round(row["ms_fractions"]["median"] / row["fifteen_ms_fractions"]["median"], 4), products_ratio=PRODUCTS_RATIO,
               commit_within=within(row["ms_commit"], row["fifteen_ms_commit"]), opening_within=within(row["ms_opening"], row["fifteen_ms_opening"]),
               wall_within=within(row["wall_ms_quiet"], row["fifteen_wall_ms_quiet"]))
    emit(row, a.out)


def run_helpers(field, logn, a):
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    MP, sync = zk.MultilinearPolynomial, zk.lib().zk_device_synchronize
    n = 1 << logn
    rand = lambda j: MP.random(field, n, 0xA00 + 64 * j + logn + field)
    A, B, Cc, qK, T0, T1, T2, M = (rand(j) for j in range(8))
    S = [index_table(zk, field, n, n), index_table(zk, field, 0, n), index_table(zk, field, 2 * n, n)]
    beta, gamma = zk.from_ints(field, [0x1234567, 0x89ABCDE])
    eleven = [A, B, Cc] + S + [qK, T0, T1, T2, M]

    def four():
        hs = [zk.wiring.fractions(w, s, j * n, beta, gamma) for j, (w, s) in enumerate(zip((A, B, Cc), S))]
        return hs + [zk.lookup.fractions([A, B, Cc, qK, T0, T1, T2, M], beta, gamma)]

    new, old = zk.plonk_lookup.helpers(eleven, beta, gamma), four()
    same = all(np.array_equal(x.evaluated_values, y.evaluated_values) for x, y in zip(new, old))
    if not same:
        raise SystemExit(f"the hook's tables at 2^{logn} differ from the four existing hooks': nothing is timed")
    del new, old
    tn, to = [], []
    for i in range(a.warmup + a.reps):
        sync(); t0 = time.perf_counter()
        hs = zk.plonk_lookup.helpers(eleven, beta, gamma)
        sync(); w = (time.perf_counter() - t0) * 1e3
        del hs
        sync(); t0 = time.perf_counter()
        hs = four()
        sync(); w2 = (time.perf_counter() - t0) * 1e3
        del hs
        if i >= a.warmup:
            tn.append(w); to.append(w2)
    row = {"kind": "helpers", "field": field, "log_n": logn, "verified": True, "reps": a.reps, "helpers_batch": zk.plonk_lookup.helpers_batch(), "ms": three(tn),
           "four_hooks_ms": three(to), "products_ratio": PRODUCTS_RATIO}
    row.update(ratio=round(row["ms"]["median"] / row["four_hooks_ms"]["median"], 4), below=bool(row["ms"]["median"] < row["four_hooks_ms"]["min"]))
    emit(row, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--bn254-size", type=int, default=20)
    ap.add_argument("--helpers-log", type=int, default=24, help="the hook alone at 2^this entries on BLS12-381 Fr (0: not)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slow-commit", type=float, default=500.0, help="a run whose ms_commit reaches this is left out of the quiet wall clock")
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--case", default=None, help="prove:FIELD:D or helpers:FIELD:LOGN -- run this one case here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_lookup_columns", "bench.jsonl"))
    a = ap.parse_args()
    if a.case:
        kind, field, size = a.case.split(":")
        (run_prove if kind == "prove" else run_helpers)(int(field), int(size), a)
        return 0
    cases = ([("helpers", 0, a.helpers_log)] if a.helpers_log else []) + [("prove", 0, int(x)) for x in a.sizes.split(",") if x]
    cases += [("prove", 3, a.bn254_size)] if a.bn254_size else []
    for kind, field, size in cases:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--case", f"{kind}:{field}:{size}", "--reps", str(a.reps),
               "--warmup", str(a.warmup), "--slow-commit", str(a.slow_commit), "--out", a.out]
        rc = subprocess.call(cmd)
        if rc != 0:                                          # a fault, an abort or a time limit: nothing more is started on the device
            print(f"case {kind}:{field}:{size} ended with status {rc}; stopping", file=sys.stderr, flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
