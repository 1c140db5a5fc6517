"""Proof-of-work grinding (zk_transcript_grind; csrc/grind.cuh fri_grind_kernel): the search's hash rate, and what a caller gets for it.
JSON lines (stdout, and appended to --out):
  kind = "rate"    one (bits, fill): SEEDS seeded transcripts whose open block holds `fill` bytes when the nonce goes in (40: one permutation a
                   candidate, 131: two), each searched once on the GPU.  A single search is geometric and says little, so the row sums them:
                   candidates (those up to and including each nonce: the lanes of the last launch hash somewhat more, so the rate is a lower
                   bound), HIP-event ms, hashes and permutations a second, and every nonce.
  kind = "host"    the one-core search (zk_host_transcript_grind) on the same transcripts at 18 bits: candidates a second, host clock.
  kind = "tree"    the Merkle tree of a table of 2^24 BLS12-381 Fr elements in the same run (zk_merkle_build: 2^24 leaf and 2^24 - 1 node
                   permutations, each with its loads and stores), best of --reps between two device events: permutations a second.  The leaf
                   kernel alone is not separated here; profiles/merkle/ has its share.
  kind = "trade"   one (d, k): k commitments with grouped leaves (b = 2, log_arity 2, f = 6, one point) opened with (Q, g) = (64, 0), (56, 16),
                   (54, 20), (52, 24), which are equal under the count b Q + g.  Proof bytes from zk_fri_ml_sizes_batch (+ 8 for the nonce where
                   g > 0); the opening's wall clock (median over --reps runs, each on a transcript with another prefix, so each run searches
                   another nonce) and the search's share of it (mean of zk_transcript_grind_last_stats' ms).  Every first opening is verified.
Without --case the tool runs every case as a fresh child process of its own, each under `timeout`, one after the other, and stops at the first
one that fails: a case that faults or hangs starts nothing after it.
    python3 tools/bench_fri_grind.py [--bits 20,24,28] [--fills 40,131] [--sizes 20,24] [--ks 1,4] [--reps 8] [--step-timeout 300] [--out FILE]
    python3 tools/bench_fri_grind.py --case rate:BITS:FILL | host:FILL | tree | trade:D:K ...       one case in this process"""
import argparse
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_fri_ml_arity import emit, setup              # noqa: E402

FIELD, B, F = 0, 2, 6
SEEDS = 8
TRADE = ((64, 0), (56, 16), (54, 20), (52, 24))


def transcript(zk, fill, seed):
    """a transcript whose open block holds `fill` bytes once the step's 8-byte tag is in, with two whole blocks absorbed before"""
    t = zk.Transcript()
    t.append(random.Random(104729 * seed + fill).randbytes((fill - 8) % 136 + 272))
    return t


def run_rate(bits, fill, a):
    zk = setup()
    transcript(zk, fill, 99).grind(12)                       # the first launch loads the code object
    cand, ms, nonces, launches = 0, 0.0, [], 0
    for seed in range(SEEDS):
        nonces.append(transcript(zk, fill, seed).grind(bits))
        st = zk.fri.grind_last_stats()
        cand, ms, launches = cand + st["candidates"], ms + st["ms"], launches + st["launches"]
    perms = 1 if fill <= 127 else 2
    emit({"kind": "rate", "bits": bits, "fill": fill, "permutations_per_candidate": perms, "searches": SEEDS, "candidates": cand, "launches": launches,
          "ms": round(ms, 3), "hashes_per_s": round(cand / ms * 1e3), "permutations_per_s": round(perms * cand / ms * 1e3), "nonces": nonces}, a.out)


def run_host(fill, a):
    zk = setup()
    bits, cand, t0 = 18, 0, time.perf_counter()
    for seed in range(4):
        cand += transcript(zk, fill, seed).grind_host(bits) + 1
    sec = time.perf_counter() - t0
    emit({"kind": "host", "bits": bits, "fill": fill, "searches": 4, "candidates": cand, "ms": round(sec * 1e3, 1), "hashes_per_s": round(cand / sec)}, a.out)


def run_tree(a):
    import ctypes as C

    import torch
    zk = setup()
    n = 1 << 24
    table = zk.MultilinearPolynomial.random(FIELD, n, 0xA11CE)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e30
    for _ in range(a.reps + 2):
        h = C.c_void_p()
        e0.record()
        rc = zk.lib().zk_merkle_build(table._h, C.byref(h))
        e1.record()
        e1.synchronize()
        if rc != 0:
            raise SystemExit(f"zk_merkle_build: status {rc}")
        best = min(best, e0.elapsed_time(e1))
        zk.lib().zk_merkle_free(h)
    emit({"kind": "tree", "field": FIELD, "log_len": 24, "permutations": 2 * n - 1, "best_ms": round(best, 3),
          "permutations_per_s": round((2 * n - 1) / best * 1e3)}, a.out)


def run_trade(d, k, a):
    import numpy as np
    zk = setup()
    sync = zk.lib().zk_device_synchronize
    coset = zk.from_ints(FIELD, [0x5EED])[0]
    cms = [zk.fri.commit(zk.MultilinearPolynomial.random(FIELD, 1 << d, 0xB00 + 16 * d + j), B, coset, log_group=2) for j in range(k)]
    pts = np.stack([zk.from_ints(FIELD, [0x1234567 + 977 * i for i in range(d)])])
    roots = [c.root for c in cms]

    def prefixed(rep):
        t = zk.Transcript()
        t.append(b"run %d" % rep)
        return t

    base_bytes = None
    for Q, g in TRADE:
        op = zk.fri.open_multilinear_batch(cms, pts, F, Q, log_arity=2, transcript=prefixed(0), grinding_bits=g)
        if not zk.fri.verify_multilinear_batch(roots, pts, op, transcript=prefixed(0)):
            raise SystemExit(f"the opening at d = {d}, k = {k}, (Q, g) = ({Q}, {g}) does not verify: nothing is timed")
        wall, grind_ms, cand = [], [], []
        for rep in range(1, a.reps + 1):
            t = prefixed(rep)
            sync()
            t0 = time.perf_counter()
            zk.fri.open_multilinear_batch(cms, pts, F, Q, log_arity=2, transcript=t, grinding_bits=g)
            sync()
            wall.append((time.perf_counter() - t0) * 1e3)
            st = zk.fri.grind_last_stats() if g else {"ms": 0.0, "candidates": 0}
            grind_ms.append(st["ms"])
            cand.append(st["candidates"])
        nroots, nfinal, nvalues, path_bytes, nround = zk.fri.ml_sizes(d, B, F, Q, log_arity=2, grouped=True, k=k)
        proof_bytes = 32 * (nroots + nfinal + nvalues + nround + k) + path_bytes + (8 if g else 0)   # + the k claims at the one point
        base_bytes = proof_bytes if base_bytes is None else base_bytes
        emit({"kind": "trade", "field": FIELD, "d": d, "k": k, "log_blowup": B, "log_final": F, "queries": Q, "grinding_bits": g, "count_bits": B * Q + g,
              "path_bytes": path_bytes, "proof_bytes": proof_bytes, "proof_bytes_over_g0": round(proof_bytes / base_bytes, 4), "verified": True,
              "wall_ms": round(statistics.median(wall), 3), "wall_ms_min": round(min(wall), 3), "wall_ms_max": round(max(wall), 3),
              "grind_ms_mean": round(statistics.mean(grind_ms), 3), "grind_ms_max": round(max(grind_ms), 3),
              "grind_candidates_mean": round(statistics.mean(cand)), "runs": a.reps}, a.out)
    for c in cms:
        c.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", default="20,24,28")
    ap.add_argument("--fills", default="40,131")
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--ks", default="1,4")
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--case", default=None, help="rate:BITS:FILL, host:FILL, tree or trade:D:K -- run this one case here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_grind", "bench.jsonl"))
    a = ap.parse_args()
    if a.case:
        kind, *rest = a.case.split(":")
        if kind == "rate":
            run_rate(int(rest[0]), int(rest[1]), a)
        elif kind == "host":
            run_host(int(rest[0]), a)
        elif kind == "tree":
            run_tree(a)
        else:
            run_trade(int(rest[0]), int(rest[1]), a)
        return 0
    fills = [int(x) for x in a.fills.split(",") if x]
    cases = [f"rate:{int(b)}:{f}" for b in a.bits.split(",") if b for f in fills] + [f"host:{f}" for f in fills] + ["tree"]
    cases += [f"trade:{int(d)}:{int(k)}" for d in a.sizes.split(",") if d for k in a.ks.split(",") if k]
    for case in cases:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps), "--out", a.out]
        rc = subprocess.call(cmd)
        if rc != 0:                                          # a fault, an abort or a time limit: nothing more is started on the device
            print(f"case {case} ended with status {rc}; stopping", file=sys.stderr, flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
