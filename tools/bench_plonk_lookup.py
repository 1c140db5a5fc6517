"""The Plonk proof with lookup rows (zk_plonk_lookup_prove; csrc/plonk_lookup.cuh) against the pair of proofs it fuses, b = 2, f = 6, Q = 64,
log_arity = 2 on grouped leaves.  JSON lines (stdout, and appended to --out):
  kind = "prove"   one case (field, d, table): A random, B = A, qM, qL, qR, qC random, qO = -1 and C = qM A B + qL A + qR B + qC, so that every
                   row satisfies the gate; sigma swaps (A, x) with (B, x) for every x and fixes C: a satisfied wiring; 16 public values, all
                   zero; qK = 1 on EVERY row.  table = "random": T0, T1, T2 are copies of A, B, C (a random table, every row looked up once).
                   table = "equal": A = B = a and C = c constant, qC solved for them, and the table is that one row 2^d times (one slot of
                   the multiplicity count takes every addition).  zk_plonk_lookup_verify accepts the proof, and zk_plonk_verify and
                   zk_lookup_verify the pair's two on one transcript, before anything is timed.  Then, alternating in one process, --reps runs
                   after --warmup of
                       fused   zk_plonk_lookup_prove                                       (zk_plonk_lookup_last_stats)
                       pair    zk_plonk_prove then zk_lookup_prove on one transcript, the same fifteen commitments (their last-stats calls)
                   medians with min / max of ms_rounds, ms_opening, ms_commit, ms_fractions, ms_multiplicities (the pair's: the two added, run
                   by run) and of the host wall clock; the pair's two openings (k = 14 and k = 9) also each on its own, beside the fused
                   proof's wide one (k = 20).  Three expectations, each allowed the pair's own min .. max spread and no more:
                   `rounds_within` = fused rounds <= pair's rounds,  `opening_within`,  `wall_within`.
Cases: BLS12-381 Fr at --sizes with the random table, once at --equal-size with the all-equal table, BN254 Fr once at --bn254-size.  Without
--case the tool runs every case as a fresh child process of its own, each under `timeout`, one after the other, and stops at the first one
that fails: a case that faults or hangs starts nothing after it.
    python3 tools/bench_plonk_lookup.py [--sizes 20,24] [--equal-size 20] [--bn254-size 20] [--reps 5] [--warmup 2] [--step-timeout 400] [--out FILE]
    python3 tools/bench_plonk_lookup.py --case FIELD:D:TABLE ...          one case in this process"""
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


def run_case(field, d, table, a):
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    MP, lib = zk.MultilinearPolynomial, zk.lib()
    sync = lib.zk_device_synchronize
    b, f, Q, la, lg = 2, 6, 64, 2, 2
    n = 1 << d
    el = lambda v: zk.from_ints(field, [v])[0]
    rand = lambda j: MP.random(field, n, 0xF00 + 256 * j + 16 * d + field)
    qM, qL, qR = (rand(2 + j) for j in range(3))
    zero = qM.scalar_mul(el(0))
    mul = lambda *ts: zk.ProductPolynomial(list(ts)).multiply_polynomials_element_wise()
    add = MP.add_polynomials
    qO = zero.sub_scalar(el(1))
    if table == "random":
        A, qC = rand(0), rand(5)
        B = A.clone()
        Cc = add(add(mul(qM, A, B), mul(qL, A)), add(mul(qR, B), qC))
    else:                                                     # A = B = 3, C = 5: qC = 5 - (9 qM + 3 qL + 3 qR)
        p = int(zk.to_ints(field, qO.evaluated_values[:1])[0]) + 1
        A = zero.sub_scalar(el(p - 3))
        B, Cc = A.clone(), zero.sub_scalar(el(p - 5))
        qC = add(add(qM.scalar_mul(el(p - 9)), qL.scalar_mul(el(p - 3))), qR.scalar_mul(el(p - 3))).sub_scalar(el(p - 5))
    qK = zero.sub_scalar(qO.evaluated_values[0])              # 0 - (-1) = 1 on every row
    sig = [index_table(zk, field, n, n), index_table(zk, field, 0, n), index_table(zk, field, 2 * n, n)]
    coset = el(0x5EED)
    fifteen = [A, B, Cc, qM, qL, qR, qO, qC] + sig + [qK, A.clone(), B.clone(), Cc.clone()]
    cms = [zk.fri.commit(t, b, coset, log_group=lg) for t in fifteen]
    roots = [c.root for c in cms]
    pub = np.zeros((NPUBLIC, 4), np.uint64)
    wires, sels, sigs, ksel, cols = cms[:3], cms[3:8], cms[8:11], cms[11], cms[12:]

    def pair():
        t = zk.Transcript()
        pp = zk.plonk.prove(wires, sels, sigs, pub, f, Q, log_arity=la, transcript=t)
        ps = zk.plonk.last_stats()
        pl = zk.lookup.prove(wires, ksel, cols, f, Q, log_arity=la, transcript=t)
        return pp, pl, ps, zk.lookup.last_stats()

    pr = zk.plonk_lookup.prove(wires, sels, sigs, ksel, cols, pub, f, Q, log_arity=la)
    if not zk.plonk_lookup.verify(roots, pub, pr) or zk.plonk_lookup.last_stats()["misses"]:
        raise SystemExit(f"the fused proof at d = {d} ({table}) does not verify: nothing is timed")
    pp, pl, _, _ = pair()
    v = zk.Transcript()
    if not (zk.plonk.verify(roots[:11], pub, pp, transcript=v) and zk.lookup.verify(roots[:3] + roots[11:], pl, transcript=v)):
        raise SystemExit(f"the pair's proofs at d = {d} ({table}) do not verify: nothing is timed")
    nbytes = lambda q: sum(x.nbytes for x in (q.h_roots, q.round_polys, q.ys, q.opening.round_polys, q.opening.roots, q.opening.final_table, q.opening.query_values,
                                              q.opening.query_paths))
    proof_bytes, pair_bytes = nbytes(pr), nbytes(pp) + nbytes(pl)
    del pr, pp, pl
    fused, fwall, prs, pwall = [], [], [], []
    for i in range(a.warmup + a.reps):                       # alternating: both sides meet the same neighbours on the machine
        sync(); t0 = time.perf_counter()
        zk.plonk_lookup.prove(wires, sels, sigs, ksel, cols, pub, f, Q, log_arity=la)
        sync(); w = (time.perf_counter() - t0) * 1e3
        st = zk.plonk_lookup.last_stats()
        sync(); t0 = time.perf_counter()
        _, _, ps, ls = pair()
        sync(); w2 = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            fused.append(st); fwall.append(w); prs.append((ps, ls)); pwall.append(w2)
    for c in cms:
        c.free()
    row = {"kind": "prove", "field": field, "d": d, "table": table, "log_blowup": b, "log_final": f, "queries": Q, "log_arity": la, "log_group": lg, "npublic": NPUBLIC,
           "verified": True, "reps": a.reps, "proof_bytes": proof_bytes, "pair_proof_bytes": pair_bytes, "wall_ms": three(fwall), "pair_wall_ms": three(pwall)}
    for name in ("ms_multiplicities", "ms_fractions", "ms_commit", "ms_eq", "ms_rounds", "ms_opening"):
        row[name] = three([s[name] for s in fused])
        row["pair_" + name] = three([ps.get(name, 0.0) + ls[name] for ps, ls in prs])
    row["plonk_ms_rounds"], row["lookup_ms_rounds"] = three([ps["ms_rounds"] for ps, _ in prs]), three([ls["ms_rounds"] for _, ls in prs])
    row["plonk_ms_opening_k14"], row["lookup_ms_opening_k9"] = three([ps["ms_opening"] for ps, _ in prs]), three([ls["ms_opening"] for _, ls in prs])
    within = lambda mine, theirs: bool(mine["median"] <= theirs["median"] + (theirs["max"] - theirs["min"]))
    row.update(rounds_within=within(row["ms_rounds"], row["pair_ms_rounds"]), opening_within=within(row["ms_opening"], row["pair_ms_opening"]),
               wall_within=within(row["wall_ms"], row["pair_wall_ms"]))
    emit(row, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--equal-size", type=int, default=20, help="the BLS12-381 Fr size at which the all-equal table is also run (0: not)")
    ap.add_argument("--bn254-size", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--case", default=None, help="FIELD:D:TABLE -- run this one case here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_lookup", "bench.jsonl"))
    a = ap.parse_args()
    if a.case:
        field, d, table = a.case.split(":")
        run_case(int(field), int(d), table, a)
        return 0
    cases = [(0, int(x), "random") for x in a.sizes.split(",") if x] + ([(0, a.equal_size, "equal")] if a.equal_size else []) + ([(3, a.bn254_size, "random")] if a.bn254_size else [])
    for field, d, table in cases:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--case", f"{field}:{d}:{table}", "--reps", str(a.reps),
               "--warmup", str(a.warmup), "--out", a.out]
        rc = subprocess.call(cmd)
        if rc != 0:                                          # a fault, an abort or a time limit: nothing more is started on the device
            print(f"case {field}:{d}:{table} ended with status {rc}; stopping", file=sys.stderr, flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
