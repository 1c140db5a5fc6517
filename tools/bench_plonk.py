"""The Plonk proof over FRI commitments (zk_plonk_prove; csrc/plonk.cuh) against the pair it fuses, b = 2, f = 6, Q = 64, log_arity = 2 on grouped
leaves.  JSON lines (stdout, and appended to --out):
  kind = "prove"   one case (field, d): A random, B = A, qM, qL, qR, qC random, qO = -1 and C = qM A B + qL A + qR B + qC, so that every row
                   satisfies the gate; sigma swaps (A, x) with (B, x) for every x and fixes C: a satisfied wiring; 16 public values, all zero
                   (every row's gate is 0, so rows 0 .. 15 are public-input rows of the value 0).  zk_plonk_verify accepts the proof, and
                   zk_zerocheck_gate_verify and zk_wiring_verify the pair's two on one transcript, before anything is timed.  Then, alternating
                   in one process, --reps runs after --warmup of
                       fused   zk_plonk_prove                                              (zk_plonk_last_stats)
                       pair    zk_zerocheck_gate_prove then zk_wiring_prove on one transcript, the same eleven commitments (their last-stats calls)
                   medians with min / max of ms_rounds, ms_opening (the pair's: the two added, run by run) and of the host wall clock; the
                   fused proof's ms_fractions, ms_commit, ms_eq beside them.  Three expectations, each allowed the pair's own min .. max spread
                   and no more:  `rounds_within` = fused rounds <= pair's rounds,  `opening_within`,  `wall_within`.
  kind = "round"   zk_plonk_round (r given: the fifteen tables folded, seven sums) on tables of 2^d entries beside zk_wiring_round on ten and
                   zk_zerocheck_gate_round on nine of them, alternating, device events around each call (output allocations and the hooks'
                   device-to-device copies of the folded tables inside).  For information.
Cases: BLS12-381 Fr at --sizes, BN254 Fr once at --bn254-size.  Without --case the tool runs every case as a fresh child process of its own,
each under `timeout`, one after the other, and stops at the first one that fails: a case that faults or hangs starts nothing after it.
    python3 tools/bench_plonk.py [--sizes 20,24] [--bn254-size 20] [--round-size 24] [--reps 5] [--warmup 2] [--step-timeout 400] [--out FILE]
    python3 tools/bench_plonk.py --case FIELD:D ...          one case in this process"""
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


def run_case(field, d, a):
    import torch
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    MP, lib = zk.MultilinearPolynomial, zk.lib()
    sync = lib.zk_device_synchronize
    b, f, Q, la, lg = 2, 6, 64, 2, 2
    n = 1 << d
    rand = lambda j: MP.random(field, n, 0xF00 + 256 * j + 16 * d + field)
    A = rand(0)
    B = A.clone()
    qM, qL, qR, qC = (rand(2 + j) for j in range(4))
    mul = lambda *ts: zk.ProductPolynomial(list(ts)).multiply_polynomials_element_wise()
    one = zk.from_ints(field, [1])[0]
    qO = A.scalar_mul(zk.from_ints(field, [0])[0]).sub_scalar(one)
    add = MP.add_polynomials
    Cc = add(add(mul(qM, A, B), mul(qL, A)), add(mul(qR, B), qC))
    sig = [index_table(zk, field, n, n), index_table(zk, field, 0, n), index_table(zk, field, 2 * n, n)]
    coset = zk.from_ints(field, [0x5EED])[0]
    eleven = [A, B, Cc, qM, qL, qR, qO, qC] + sig
    cms = [zk.fri.commit(t, b, coset, log_group=lg) for t in eleven]
    roots = [c.root for c in cms]
    pub = np.zeros((NPUBLIC, 4), np.uint64)
    wires, sels, sigs = cms[:3], cms[3:8], cms[8:]

    def pair():
        t = zk.Transcript()
        pg = zk.zerocheck.prove_gate(wires, sels, f, Q, log_arity=la, transcript=t)
        gs = zk.zerocheck.last_stats()
        pw = zk.wiring.prove(wires, sigs, f, Q, log_arity=la, transcript=t)
        return pg, pw, gs, zk.wiring.last_stats()

    pr = zk.plonk.prove(wires, sels, sigs, pub, f, Q, log_arity=la)
    if not zk.plonk.verify(roots, pub, pr):
        raise SystemExit(f"the Plonk proof at d = {d} does not verify: nothing is timed")
    pg, pw, _, _ = pair()
    v = zk.Transcript()
    if not (zk.zerocheck.verify_gate(roots[:8], pg, transcript=v) and zk.wiring.verify(roots[:3] + roots[8:], pw, transcript=v)):
        raise SystemExit(f"the pair's proofs at d = {d} do not verify: nothing is timed")
    del pr, pg, pw
    fused, fwall, prs, pwall = [], [], [], []
    for i in range(a.warmup + a.reps):                       # alternating: both sides meet the same neighbours on the machine
        sync(); t0 = time.perf_counter()
        zk.plonk.prove(wires, sels, sigs, pub, f, Q, log_arity=la)
        sync(); w = (time.perf_counter() - t0) * 1e3
        st = zk.plonk.last_stats()
        sync(); t0 = time.perf_counter()
        _, _, gs, ws = pair()
        sync(); w2 = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            fused.append(st); fwall.append(w); prs.append((gs, ws)); pwall.append(w2)
    for c in cms:
        c.free()
    del cms, sig
    row = {"kind": "prove", "field": field, "d": d, "log_blowup": b, "log_final": f, "queries": Q, "log_arity": la, "log_group": lg, "npublic": NPUBLIC, "verified": True,
           "reps": a.reps, "wall_ms": three(fwall), "pair_wall_ms": three(pwall)}
    for name in ("ms_fractions", "ms_commit", "ms_eq", "ms_rounds", "ms_opening"):
        row[name] = three([s[name] for s in fused])
    row["pair_ms_rounds"] = three([g["ms_rounds"] + w["ms_rounds"] for g, w in prs])
    row["pair_ms_opening"] = three([g["ms_opening"] + w["ms_opening"] for g, w in prs])
    row["gate_ms_rounds"], row["wiring_ms_rounds"] = three([g["ms_rounds"] for g, _ in prs]), three([w["ms_rounds"] for _, w in prs])
    row["gate_ms_opening"], row["wiring_ms_opening"] = three([g["ms_opening"] for g, _ in prs]), three([w["ms_opening"] for _, w in prs])
    within = lambda mine, theirs: bool(mine["median"] <= theirs["median"] + (theirs["max"] - theirs["min"]))
    row.update(rounds_within=within(row["ms_rounds"], row["pair_ms_rounds"]), opening_within=within(row["ms_opening"], row["pair_ms_opening"]),
               wall_within=within(row["wall_ms"], row["pair_wall_ms"]))
    emit(row, a.out)

    if d == a.round_size:
        E, H = MP.random(field, n, 0xE00 + d), [rand(8 + j) for j in range(3)]
        fifteen = eleven + H + [E]                            # any fifteen tables: the pass does the same work on every input
        ten, nine = fifteen[:3] + fifteen[8:], fifteen[:8] + [E]
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

        p_ms, w_ms, g_ms = [], [], []
        for i in range(a.warmup + a.reps):
            p = timed(lambda: zk.plonk.round(fifteen, *el, id_base=r, log_step=1, r=r))
            w = timed(lambda: zk.wiring.round(ten, *el, id_base=r, log_step=1, r=r))
            g = timed(lambda: zk.zerocheck.gate_round(nine, r))
            if i >= a.warmup:
                p_ms.append(p); w_ms.append(w); g_ms.append(g)
        emit({"kind": "round", "field": field, "d": d, "reps": a.reps, "plonk_round_ms": three(p_ms), "wiring_round_ms": three(w_ms), "gate_round_ms": three(g_ms),
              "products": 110, "accesses": 96,
              "note": "one pass over 2^d entries each, output allocations inside; the plonk and the wiring hook also copy the folded tables (15 and 10 x 2^d / 2 "
                      "entries) out of the pass's one block into the caller's tables, which the provers' rounds do not do"}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--bn254-size", type=int, default=20)
    ap.add_argument("--round-size", type=int, default=24, help="the BLS12-381 Fr size at which the round pass is also timed on its own")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--case", default=None, help="FIELD:D -- run this one case here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk", "bench.jsonl"))
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
