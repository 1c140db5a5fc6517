"""FRI low-degree prover (csrc/fri.cuh, csrc/zkmle_fri.hip), BLS12-381 Fr.  JSON lines (stdout, and appended to --out):
  kind = "fold"   zk_fri_fold against zk_mle_fold on a table of the same length in the same run: kernel_ms of each (device events around the
                  call, medians of --reps after --warmup; zk_fri_fold's includes building its power tables and allocating its output),
                  the ratio, and the achieved GB/s of both (96 bytes per output entry)
  kind = "proof"  zk_fri_prove at d, b = 2, f = 6, Q = 64: wall_ms (host clock around the call; it ends synchronised), zk_fri_last_stats'
                  split of it, and parts_ms = zk_uni_low_degree_extend + one zk_merkle_build per committed layer on the same tables, timed
                  in the same run: what existed before.  Every timed proof is verified (zk_fri_verify) first: "verified": true.
    python3 tools/bench_fri.py [--fold-sizes 20,22,24] [--proof-sizes 18,20,22] [--reps 10] [--warmup 3] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/bench_fri.py --profile-run    (one 2^24 fold of each kind, one d = 22 proof)"""
import argparse
import json
import os
import statistics
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
    ap.add_argument("--fold-sizes", default="20,22,24")
    ap.add_argument("--proof-sizes", default="18,20,22")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri", "bench_fri.jsonl"))
    ap.add_argument("--profile-run", action="store_true", help="one fold of each kind at 2^24 and one d = 22 proof, nothing timed")
    a = ap.parse_args()
    import torch
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    MP, lib = zk.MultilinearPolynomial, zk.lib()
    sync = lib.zk_device_synchronize
    field, b, f, Q = 0, 2, 6, 64
    cm, beta = zk.from_ints(field, [0x5EED])[0], zk.from_ints(field, [0xBE7A])[0]
    if a.profile_run:
        t, half = MP.random(field, 1 << 24, 1), MP.alloc(field, 1 << 23)
        _lib.check(lib.zk_mle_fold(t._h, 0, _lib.p64(beta), half._h, None))
        zk.fri.fold(t, beta, cm)
        del t, half
        assert zk.fri.verify(zk.fri.prove(MP.random(field, 1 << 22, 2), b, f, Q, cm))
        sync()
        return
    for log_n in [int(x) for x in a.fold_sizes.split(",")]:
        n = 1 << log_n
        t, half = MP.random(field, n, 3 + log_n), MP.alloc(field, n // 2)
        _, mle_ms = timed(lambda: _lib.check(lib.zk_mle_fold(t._h, 0, _lib.p64(beta), half._h, None)), a.reps, a.warmup, sync, torch)
        _, fri_ms = timed(lambda: zk.fri.fold(t, beta, cm), a.reps, a.warmup, sync, torch)
        gbps = lambda ms: round(96.0 * (n // 2) / (ms * 1e-3) / 1e9, 1)
        emit({"kind": "fold", "log_n": log_n, "mle_fold_ms": round(mle_ms, 4), "fri_fold_ms": round(fri_ms, 4), "ratio": round(fri_ms / mle_ms, 3),
              "mle_fold_GBps": gbps(mle_ms), "fri_fold_GBps": gbps(fri_ms)}, a.out)
        del t, half
    for d in [int(x) for x in a.proof_sizes.split(",")]:
        poly = MP.random(field, 1 << d, 0xF00 + d)
        proof = zk.fri.prove(poly, b, f, Q, cm)
        verified = zk.fri.verify(proof)
        if not verified:
            raise SystemExit(f"the proof at d = {d} does not verify: nothing is timed")
        stats = []

        def run():
            zk.fri.prove(poly, b, f, Q, cm)
            stats.append(zk.fri.last_stats())

        wall, _ = timed(run, a.reps, a.warmup, sync, torch)
        st = {k: round(statistics.median(s[k] for s in stats[a.warmup:]), 4) for k in ("ms_extend", "ms_trees", "ms_folds", "ms_queries", "ms_total")}
        # what existed before: the extension and one tree per committed layer, on tables of the layers' lengths
        ext_wall, _ = timed(lambda: zk.low_degree_extend(poly, b, cm), a.reps, a.warmup, sync, torch)
        trees = 0.0
        for l in range(d - f):
            layer = MP.random(field, (1 << (d + b)) >> l, 0x7EE + l)
            w, _ = timed(lambda: zk.MerkleTree.build(layer), max(3, a.reps // 2), 2, sync, torch)
            trees += w
            del layer
        emit({"kind": "proof", "d": d, "log_blowup": b, "log_final": f, "queries": Q, "verified": bool(verified), "wall_ms": round(wall, 4), **st,
              "parts_extend_ms": round(ext_wall, 4), "parts_trees_ms": round(trees, 4), "parts_ms": round(ext_wall + trees, 4),
              "added_ms": round(wall - ext_wall - trees, 4)}, a.out)


if __name__ == "__main__":
    main()
