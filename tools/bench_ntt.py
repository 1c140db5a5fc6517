"""Number-theoretic transform (csrc/ntt.cuh): forward, inverse and coset forward of 2^16 .. 2^24 entries of BLS12-381 Fr, in place, against
the two floors measured in the same run.  JSON lines (stdout, and appended to --out):
  kind = "floors"  fold0_GBps: the streaming rate of the 2^24 fold (96 bytes per output entry); field_mul_per_s: the register-resident
                   Fr product rate of tools/microbench (fe_mul_u_chain_fr381)
  kind = "ntt"     per log_n and transform: wall_ms (host clock around the call and a device synchronise) and kernel_ms (device events
                   around the call's launches), medians of --reps runs after --warmup; passes, hbm_floor_ms = passes x 64 B x n at the
                   fold's rate, valu_floor_ms = ((n / 2) (log_n - passes) + twist and scale products) / product rate (a pass's first level
                   multiplies by 1 and is skipped), the binding floor and kernel_ms' share of it
    python3 tools/bench_ntt.py [--sizes 16,18,20,22,24] [--reps 20] [--warmup 5] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/bench_ntt.py --profile-run    (one forward, one coset inverse at the largest size)"""
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


def passes_of(log_n):
    return 1 if log_n <= 10 else 2 if log_n < 16 else 3 if log_n <= 24 else (log_n + 7) // 8


def timed(fn, reps, warmup, sync, torch):
    for _ in range(warmup):
        fn()
    wall, kern = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync(); t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        sync(); wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(e0.elapsed_time(e1))
    return statistics.median(wall), statistics.median(kern)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,18,20,22,24")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt", "bench_ntt.jsonl"))
    ap.add_argument("--profile-run", action="store_true", help="one forward and one coset inverse at the largest size, nothing timed")
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    import torch
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    MP = zk.MultilinearPolynomial
    sync = zk.lib().zk_device_synchronize
    field = 0
    cm = zk.from_ints(field, [0x5EED])[0]
    if a.profile_run:
        t = MP.random(field, 1 << max(sizes), 1)
        zk.ntt_inplace(t)
        zk.ntt_inplace(t, inverse=True, coset=cm)
        sync()
        return
    # the two floors, in this run
    big = MP.random(field, 1 << 24, 2)
    half = MP.alloc(field, 1 << 23)
    _, fold_ms = timed(lambda: _lib.check(zk.lib().zk_mle_fold(big._h, 0, _lib.p64(cm), half._h, None)), a.reps, a.warmup, sync, torch)
    fold_rate = 96.0 * (1 << 23) / (fold_ms * 1e-3)
    del big, half
    mul_rate = None
    mb = os.path.join(ROOT, "tools", "microbench")
    if os.path.exists(mb):
        for line in subprocess.run([mb], capture_output=True, text=True, timeout=300).stdout.splitlines():
            if '"fe_mul_u_chain_fr381"' in line:
                mul_rate = json.loads(line)["field_mul_per_s"]
    if mul_rate is None:
        raise SystemExit("tools/microbench did not report fe_mul_u_chain_fr381: build it with __graft_entry__.build()")
    emit({"kind": "floors", "fold0_ms_2p24": round(fold_ms, 4), "fold0_GBps": round(fold_rate / 1e9, 1), "field_mul_per_s": mul_rate}, a.out)
    for log_n in sizes:
        n = 1 << log_n
        t = MP.random(field, n, 3 + log_n)
        d = passes_of(log_n)
        for name, inverse, coset in (("forward", False, None), ("inverse", True, None), ("coset_forward", False, cm)):
            wall, kern = timed(lambda: zk.ntt_inplace(t, inverse, coset), a.reps, a.warmup, sync, torch)
            extra = (d - 1) * 2 + (2 if coset is not None else 0) + (1 if inverse else 0)          # twist: 2 per entry and pass boundary
            products = (n // 2) * (log_n - d) + extra * n
            hbm, valu = d * 64.0 * n / fold_rate * 1e3, products / mul_rate * 1e3
            emit({"kind": "ntt", "log_n": log_n, "transform": name, "passes": d, "wall_ms": round(wall, 4), "kernel_ms": round(kern, 4),
                  "field_products": products, "hbm_floor_ms": round(hbm, 4), "valu_floor_ms": round(valu, 4),
                  "binding": "valu" if valu > hbm else "hbm", "share_of_binding_floor": round(max(hbm, valu) / kern, 3)}, a.out)


if __name__ == "__main__":
    main()
