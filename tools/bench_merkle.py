"""Keccak-256 Merkle commitment of a table (csrc/merkle.cuh) and the provers bound to it, against the host absorb they replace.
JSON lines (stdout, and appended to --out):
  kind = "root"      per log_n: root_only_ms / build_ms (wall, best of --reps, one synchronisation each; build includes the tree's
                     hipMalloc), permutations = 2 len - 1, perms_per_s of each; the two modes' roots are compared
  kind = "sumcheck"  per log_n: zk_sumcheck_basic_prove (wall, ms_absorb, ms_rounds) and prove_committed in the same run, and the ratio
  kind = "gkr"       the config-4 shaped sparse proof (depth 3, 2^log_gates gates per layer) in both bindings, each verified
    python3 tools/bench_merkle.py [--sizes 20,22,24] [--reps 3] [--gkr-log-gates 22] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/bench_merkle.py --profile-run    (one root, one build, one committed proof at
    2^24; summarise with tools/rocprof_summary.py DIR merkle_)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                     # noqa: E402
import __graft_entry__ as G                                            # noqa: E402


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def best_ms(fn, reps, sync):
    fn()                                                               # warm-up (scratch pool, code objects)
    ts = []
    for _ in range(reps):
        sync(); t0 = time.perf_counter()
        fn()
        sync(); ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,22,24")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gkr-log-gates", type=int, default=22)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle", "bench_merkle.jsonl"))
    ap.add_argument("--profile-run", action="store_true", help="one call of each kind at the largest size, nothing timed (run under rocprofv3)")
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    MP = zk.MultilinearPolynomial
    sync = zk.lib().zk_device_synchronize
    field = 0
    if a.profile_run:
        poly = MP.random(field, 1 << max(sizes), 0x3E4C1E)
        root = zk.merkle_root(poly)
        tree = zk.MerkleTree.build(poly)
        assert tree.root() == root
        proof = zk.Prover.init(field, poly).prove_committed()
        assert proof.root == root and zk.Verifier.init().verify_committed(proof)
        print(json.dumps({"log_n": max(sizes), "profile_run": True}), flush=True)
        return
    for lg in sizes:
        n = 1 << lg
        poly = MP.random(field, n, 0x3E4C1E + lg)
        perms = 2 * n - 1
        ms, all_ms = best_ms(lambda: zk.merkle_root(poly), a.reps, sync)
        emit({"kind": "root", "mode": "root_only", "log_n": lg, "root_only_ms": ms, "root_only_ms_all": all_ms, "permutations": perms,
              "perms_per_s": perms / (ms * 1e-3), "scratch_bytes": 32 * perms}, a.out)
        root = zk.merkle_root(poly)
        holder = []

        def build():
            holder.clear()
            holder.append(zk.MerkleTree.build(poly))
        ms, all_ms = best_ms(build, a.reps, sync)
        assert holder[0].root() == root
        holder.clear()
        emit({"kind": "root", "mode": "build", "log_n": lg, "build_ms": ms, "build_ms_all": all_ms, "permutations": perms,
              "perms_per_s": perms / (ms * 1e-3), "tree_bytes": 32 * perms}, a.out)
        # the two provers in the same run
        row = {"kind": "sumcheck", "log_n": lg}
        for name in ("prove", "prove_committed"):
            getattr(zk.Prover.init(field, poly), name)()               # warm-up
            best = None
            for _ in range(a.reps):
                prover = zk.Prover.init(field, poly)
                sync(); t0 = time.perf_counter()
                proof = getattr(prover, name)()
                wall = (time.perf_counter() - t0) * 1e3
                st = zk.sumcheck.last_stats()
                if best is None or wall < best[0]:
                    best = (wall, st["ms_absorb"], st["ms_rounds"])
            row[name + "_ms"], row[name + "_ms_absorb"], row[name + "_ms_rounds"] = best
        assert proof.root == root and zk.Verifier.init().verify_committed(proof)
        row["speedup"] = row["prove_ms"] / row["prove_committed_ms"]
        emit(row, a.out)
        del poly
    # config-4 shaped sparse GKR proof (tools/bench_gkr_sparse.py), output layer absorbed / bound by its root
    lg, depth = a.gkr_log_gates, 3
    n = 1 << lg
    rng = np.random.default_rng(0x5EED0004)
    rows = []
    for _ in range(depth):
        g = np.zeros((n, 4), np.uint64)
        g[:, 0] = rng.integers(0, n, n); g[:, 1] = rng.integers(0, n, n)
        g[:, 2] = np.arange(n); g[:, 3] = rng.integers(0, 2, n)
        rows.append(g)
    out_bits = [lg] * depth
    x = MP.random(field, n, 0x5EED0004).evaluated_values
    circuit = zk.gkr.SparseCircuit(rows, out_bits, n)
    row = {"kind": "gkr", "log_gates": lg, "depth": depth}
    for name, commit in (("absorbed", False), ("committed", True)):
        zk.gkr.sparse_prove(field, None, None, x, circuit=circuit, commit_output=commit)          # warm-up
        ts = []
        for _ in range(a.reps):
            sync(); t0 = time.perf_counter()
            proof = zk.gkr.sparse_prove(field, None, None, x, circuit=circuit, commit_output=commit)
            ts.append((time.perf_counter() - t0) * 1e3)
        row[name + "_prove_ms"], row[name + "_layers_ms"] = min(ts), sum(proof.ms_layers)
        row[name + "_verified"] = bool(zk.gkr.sparse_verify(field, rows, out_bits, proof, x, commit_output=commit))
    row["speedup"] = row["absorbed_prove_ms"] / row["committed_prove_ms"]
    emit(row, a.out)


if __name__ == "__main__":
    main()
