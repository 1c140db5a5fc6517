"""Batched multilinear-KZG opening (zk_kzg_batch_open: k polynomials at one point, one proof) against k single zk_kzg_open calls, with
the opening key's levels precomputed.  One JSON line per (log_n, k):
  batch_open_ms      one batched opening (best of --reps), evaluations + transcript + fused first level + levels 2..n + MSMs
  singles_ms         k zk_kzg_open calls of the same polynomials (best of --reps each, summed)
  lincomb_ms         zk_mle_linear_combination of the k tables (HIP events, best of --reps): the plain instantiation of the kernel
  fused_level_us     lincomb_kernel<Fr381, true> of the batched opening, from the rocprofv3 trace of a separate --profile-run of this
                     tool (--trace DIR); absent without one
  *_bytes, *_hbm_frac  bytes each kernel moves (k table reads + its writes) and that over the time, as a fraction of 8 TB/s
Every timed batched proof is checked by zk_kzg_batch_verify.
    python3 tools/bench_kzg_batch.py [--sizes 20,24] [--ks 1,4,8] [--reps 3] [--trace DIR]
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/bench_kzg_batch.py --profile-run [--sizes ..] [--ks ..]"""
import argparse
import csv
import glob
import json
import os
import sqlite3
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                     # noqa: E402
import __graft_entry__ as G                                            # noqa: E402

HBM_PEAK = 8.0e12
EL = 32                                                                # bytes per Fr element


def fused_times(d):
    """durations (us) of the fused first-level dispatches, in launch order"""
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)):
        rows += list(sqlite3.connect(f).execute("select name, start, end from kernels order by start"))
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        rows += [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: r[1])
    return [(e - s) / 1e3 for n, s, e in rows if "lincomb_kernel" in n and "true" in n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--ks", default="1,4,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--profile-run", action="store_true", help="one batched opening per case, nothing else timed (run under rocprofv3)")
    a = ap.parse_args()
    sizes, ks = [int(x) for x in a.sizes.split(",")], [int(x) for x in a.ks.split(",")]
    fused = fused_times(a.trace) if a.trace else None
    zk = G.import_package()
    from zkmle_amd import _lib
    import torch
    _lib.check(zk.lib().zk_init(0))
    MP, KZG = zk.MultilinearPolynomial, zk.MultilinearKZG
    sync = zk.lib().zk_device_synchronize
    case = 0
    for lg in sizes:
        n = 1 << lg
        taus = zk.from_ints(0, [0x1000003 * (i + 1) + 12345 for i in range(lg)])
        point = zk.from_ints(0, [0x2000003 * (i + 7) + 999 for i in range(lg)])
        setup = zk.TrustedSetup.initialize_setup(taus)
        setup.precompute_for_opens()
        polys = [MP.random(0, n, 0x5EED0100 + j) for j in range(max(ks))]
        commitments = np.stack([KZG.commit_to_polynomial(f, setup) for f in polys])
        out = MP.alloc(0, n)
        for k in ks:
            ps, cs = polys[:k], commitments[:k]
            if a.profile_run:
                proof = KZG.batch_open_and_prove(ps, setup, point, cs)
                assert KZG.batch_verify(setup, cs, point, proof), "the batched opening does not verify"
                print(json.dumps({"log_n": lg, "k": k, "profile_run": True}), flush=True)
                continue
            KZG.batch_open_and_prove(ps, setup, point, cs)                 # warm-up (scratch pool)
            ts = []
            for _ in range(a.reps):
                sync(); t0 = time.perf_counter()
                proof = KZG.batch_open_and_prove(ps, setup, point, cs)
                sync(); ts.append((time.perf_counter() - t0) * 1e3)
                assert KZG.batch_verify(setup, cs, point, proof), "the timed batched opening does not verify"
            singles = 0.0
            for f in ps:
                KZG.open_and_prove(f, setup, point)
                best = 1e30
                for _ in range(a.reps):
                    sync(); t0 = time.perf_counter()
                    KZG.open_and_prove(f, setup, point)
                    sync(); best = min(best, (time.perf_counter() - t0) * 1e3)
                singles += best
            coeffs = zk.from_ints(0, [pow(0x1234567, j, zk.mle.MODULI[0]) for j in range(k)])
            handles = (_lib.vp * k)(*[p._h.value for p in ps])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            lc = 1e30
            for _ in range(a.reps + 1):
                e0.record()
                _lib.check(zk.lib().zk_mle_linear_combination(handles, k, _lib.p64(coeffs), out._h, None))
                e1.record()
                e1.synchronize()
                lc = min(lc, e0.elapsed_time(e1))
            plain_bytes = (k + 1) * n * EL                                 # k tables read, one written
            fused_bytes = k * n * EL + n * EL                              # k tables read, two half tables (q, folded g - v) written
            row = {"log_n": lg, "k": k, "batch_open_ms": min(ts), "batch_open_ms_all": ts, "singles_ms": singles,
                   "speedup_vs_singles": singles / min(ts), "lincomb_ms": lc, "lincomb_bytes": plain_bytes,
                   "lincomb_hbm_frac": plain_bytes / (lc * 1e-3) / HBM_PEAK, "fused_level_bytes": fused_bytes,
                   "verified": True, "opening_key": "precomputed (zk_kzg_opening_key_precompute, levels >= 2^18)"}
            if fused is not None and case < len(fused):
                row["fused_level_us"] = fused[case]
                row["fused_level_hbm_frac"] = fused_bytes / (fused[case] * 1e-6) / HBM_PEAK
            case += 1
            print(json.dumps(row), flush=True)
        del setup, polys, out


if __name__ == "__main__":
    main()
