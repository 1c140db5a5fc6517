"""The R1CS prover (zk_r1cs_prove) and its two sparse passes (zk_r1cs_matvec, zk_r1cs_bind_rows; csrc/r1cs.cuh) on a synthetic circuit.  JSON lines
(stdout, and appended to --out), one per case (field, d):
  instance   s = d - 1 rows.  The witness half is inputs (its first half) and outputs (its second).  Row r, with j = r mod 2^(d-3): A holds three
             entries at input columns an eighth of the witness half apart from a random start and one in the constant's column 2^(d-1) (the
             dense column of the public half); B three at input columns; C the output entry (r, 2^(d-2) + j, 1) and two input entries.  Rows r
             and r + 2^(d-2) are alike, so every output is defined once.  Random values, l = 3 public values (read by no row).
  z          satisfying, made with the library: z0 = (random inputs, zero outputs, x); the outputs are (A z0) o (B z0) - C z0 (the passes read
             no output column in A and B), by zk_r1cs_matvec, an element-wise product and a linear combination; w is committed (b = 2,
             grouped leaves) and one proof is verified before anything is timed.
  passes     zk_r1cs_last_stats after zk_r1cs_matvec / zk_r1cs_bind_rows: device events around the launches alone, --reps runs after --warmup;
             median, min, max in ms.  bytes = what the pass must move: per entry the value (32), the index (4) and the gathered operand (32),
             per item two offsets (8; the transpose reads three columns' offsets an item) and the list entry (4), per output one element (32).
             The transpose over the witness half (the prover's call) and over all columns (full = 1: the dense column on one workgroup).
  proof      zk_r1cs_prove at f = 6, Q = 64, log_arity 2: the wall clock between two device synchronisations and zk_r1cs_last_stats' split.
             zk_r1cs_create's time (host, once per circuit) is reported beside, not inside.
Without --case every case runs as a fresh child process under `timeout`, one after the other, and the tool stops at the first that fails.
    python3 tools/bench_r1cs.py [--sizes 16,20,22] [--fields 0,3] [--reps 7] [--warmup 2] [--step-timeout 280] [--out FILE]
    python3 tools/bench_r1cs.py --case FIELD:D ...          one case in this process"""
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


def synthetic(np, zk, field, d, seed):
    """-> [(rows, cols, vals)] for A, B, C"""
    s, half = d - 1, 1 << (d - 1)
    ins = half // 2
    rng = np.random.default_rng(seed)
    top = (1 << (zk.mle.MODULI[field].bit_length() - 1 - 192)) - 1        # the top word masked below the modulus's leading bit: a reduced element
    r = np.arange(1 << s, dtype=np.uint32)
    j = r % np.uint32(ins)
    one = zk.from_ints(field, [1])[0]

    def values(n):
        v = rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64)
        v[:, 3] &= np.uint64(top)
        return v

    def inputs(per):                                          # per input columns a row, the same for r and r + ins
        start = rng.integers(0, ins, ins, dtype=np.uint32)[j]
        cols = (np.repeat(start, per) + np.tile(np.arange(per, dtype=np.uint32) * np.uint32(ins // 4), 1 << s)) % np.uint32(ins)
        vals = values(ins * per).reshape(ins, per, 4)[j].reshape(-1, 4)
        return np.repeat(r, per), cols.astype(np.uint32), vals

    ra, ca, va = inputs(3)
    A = (np.concatenate([ra, r]), np.concatenate([ca, np.full(1 << s, half, np.uint32)]), np.concatenate([va, values(ins)[j]]))
    B = inputs(3)
    rc, cc, vc = inputs(2)
    Cm = (np.concatenate([rc, r]), np.concatenate([cc, (np.uint32(ins) + j).astype(np.uint32)]), np.concatenate([vc, np.tile(one, (1 << s, 1))]))
    return [A, B, Cm]


def run_case(field, d, a):
    import numpy as np
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    MP, sync = zk.MultilinearPolynomial, zk.lib().zk_device_synchronize
    s, half = d - 1, 1 << (d - 1)
    ins = half // 2
    mats = synthetic(np, zk, field, d, 0x51C5 + 16 * d + field)
    t0 = time.perf_counter()
    inst = zk.R1CS(field, s, d, *mats)
    create_s = time.perf_counter() - t0
    nnz = sum(m[0].shape[0] for m in mats)
    del mats
    # the satisfying z
    public = MP.random(field, 4, 0x4000 + d).evaluated_values[:3].copy()
    z0 = np.zeros((1 << d, 4), np.uint64)
    z0[:ins] = MP.random(field, ins, 0x2000 + d).evaluated_values
    z0[half] = zk.from_ints(field, [1])[0]
    z0[half + 1:half + 4] = public
    az, bz, cz = zk.r1cs.matvec(inst, MP.vector(field, z0))
    ab = zk.ProductPolynomial([az, bz]).multiply_polynomials_element_wise()
    coef = zk.from_ints(field, [1, -1])
    z0[ins:half] = MP.linear_combination([ab, cz], coef).evaluated_values[:ins]
    z = MP.vector(field, z0)
    az, bz, cz = zk.r1cs.matvec(inst, z)
    if not np.array_equal(zk.ProductPolynomial([az, bz]).multiply_polynomials_element_wise().evaluated_values, cz.evaluated_values):
        raise SystemExit(f"z does not satisfy the instance at d = {d}: nothing is timed")
    del az, bz, cz, ab
    b, f, Q, la = 2, 6, 64, 2
    cm = zk.fri.commit(MP(field, z0[:half]), b, zk.from_ints(field, [0x5EED])[0], log_group=2)
    pr = zk.r1cs.prove(inst, cm, public, f, Q, log_arity=la)
    if not zk.r1cs.verify(inst, cm.root, public, pr):
        raise SystemExit(f"the proof at d = {d} does not verify: nothing is timed")
    rx, rho = pr.challenges[::-1].copy(), pr.rho
    sh = inst.shape

    def timed(fn, key):
        ms = []
        for i in range(a.warmup + a.reps):
            out = fn()
            del out
            if i >= a.warmup:
                ms.append(zk.r1cs.last_stats()[key])
        return three(ms)

    mv = timed(lambda: zk.r1cs.matvec(inst, z), "ms_products")
    bh = timed(lambda: zk.r1cs.bind_rows(inst, rx, rho), "ms_bind")
    bf = timed(lambda: zk.r1cs.bind_rows(inst, rx, rho, full=True), "ms_bind")
    wall, stats = [], []
    for i in range(a.warmup + a.reps):
        sync(); t0 = time.perf_counter()
        zk.r1cs.prove(inst, cm, public, f, Q, log_arity=la)
        sync(); w = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            wall.append(w)
            stats.append(zk.r1cs.last_stats())
    cm.free()
    rows3, cols = 3 << s, 1 << d
    mv_bytes = nnz * 68 + rows3 * (12 + 32)
    nnz_half = nnz - (1 << s)                                   # the dense column lies in the public half
    bh_bytes = nnz_half * 68 + (cols // 2) * (3 * 8 + 4 + 32)
    bf_bytes = nnz * 68 + cols * (3 * 8 + 4 + 32)
    gbps = lambda by, t: round(by / (t["median"] * 1e-3) / 1e9, 1)
    row = {"kind": "r1cs", "field": field, "d": d, "s": s, "nnz": nnz, "block_rows": sh["block_rows"], "block_cols": sh["block_cols"], "create_s": round(create_s, 3),
           "reps": a.reps, "matvec_ms": mv, "matvec_bytes": mv_bytes, "matvec_GBps": gbps(mv_bytes, mv), "bind_half_ms": bh, "bind_half_bytes": bh_bytes,
           "bind_half_GBps": gbps(bh_bytes, bh), "bind_full_ms": bf, "bind_full_bytes": bf_bytes, "bind_full_GBps": gbps(bf_bytes, bf),
           "prove": {"log_blowup": b, "log_final": f, "queries": Q, "log_arity": la, "log_group": 2, "verified": True, "wall_ms": three(wall)}}
    for key in ("ms_products", "ms_eq", "ms_rounds", "ms_bind", "ms_opening", "ms_total"):
        row["prove"][key] = three([st[key] for st in stats])
    emit(row, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20,22")
    ap.add_argument("--fields", default="0,3")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=280)
    ap.add_argument("--case", default=None, help="FIELD:D -- run this one case here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1cs", "bench.jsonl"))
    a = ap.parse_args()
    if a.case:
        field, d = (int(x) for x in a.case.split(":"))
        run_case(field, d, a)
        return 0
    for field in (int(x) for x in a.fields.split(",") if x):
        for d in (int(x) for x in a.sizes.split(",") if x):
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--case", f"{field}:{d}", "--reps", str(a.reps),
                   "--warmup", str(a.warmup), "--out", a.out]
            rc = subprocess.call(cmd)
            if rc != 0:                                      # a fault, an abort or a time limit: nothing more is started on the device
                print(f"case {field}:{d} ended with status {rc}; stopping", file=sys.stderr, flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
