"""Child process of tests/test_gpu_foldk_edges.py: one pass of the weighted-sum fold through the zk_rounds_multi_* handle for every
(field, shape, table kind) named on the command line, compared with the integer model (tests/_foldk_shadow_model.py).  A child
process because folding 8 variables per pass needs ZK_BASIC_ROUNDS_PER_PASS=8, which is read once per process.
Prints one JSON line {case id: {...}}.   usage: _foldk_edge_worker.py SHAPE[,SHAPE...]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as G                                                          # noqa: E402
import _foldk_shadow_model as FM                                                     # noqa: E402

FIELDS = (0, 3)


def to_limbs(values):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), np.uint64).reshape(-1, 4).copy()


def to_ints(arr):
    return [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(arr, np.uint64).reshape(-1, 4)]


def main():
    names = sys.argv[1].split(",")
    zk = G.import_package()
    from zkmle_amd import _lib as L
    lib = zk.lib()
    L.check(lib.zk_init(0))
    vp, u64p = C.c_void_p, L.u64p
    lib.zk_rounds_new.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, vp, C.POINTER(vp)]
    lib.zk_rounds_free.argtypes = [vp]
    lib.zk_rounds_multi_max.argtypes = [vp]
    lib.zk_rounds_multi_max.restype = C.c_uint
    lib.zk_rounds_multi_evals.argtypes = [vp, vp, C.c_uint, vp]
    lib.zk_rounds_multi_absorb.argtypes = [vp, vp, C.c_uint]
    lib.zk_rounds_multi_fold_evals.argtypes = [vp, vp, vp, C.c_uint, C.c_uint, vp]
    lib.zk_rounds_multi_tail.argtypes = [vp, vp]
    lib.zk_rounds_collect.argtypes = [vp, vp, u64p, u64p, u64p, u64p]
    with open(os.path.join(ROOT, "tests", "golden", "foldk_hot_transcripts.json")) as f:
        hot = json.load(f)["fields"]
    MP = zk.MultilinearPolynomial
    out = {}
    for field in FIELDS:
        p = FM.MODULUS[field]
        limbs = MP.alloc(field, 1024)                                 # device scratch for the limb words (tests/test_gpu_sharded.py)
        lp = lib.zk_table_device_ptr(limbs._h)
        for name, K, logn, m_next, form in FM.SHAPES:
            if name not in names:
                continue
            n = 1 << (logn - K)
            for kind in FM.KINDS:
                nonce = hot.get(str(field), {}).get(name, {}).get(kind, {}).get("nonce", 0)
                table = FM.make_table(field, kind, 1 << logn)
                table_limbs = to_limbs(table)
                poly = MP(field, table_limbs)
                tr = zk.Transcript()
                tr.append(FM.nonce_bytes(nonce))
                r = vp()
                L.check(lib.zk_rounds_new(field, 0, 1, 1, logn, tr._h, C.byref(r)))
                res = {"multi_max": int(lib.zk_rounds_multi_max(r))}
                out["%d-%s-%s" % (field, name, kind)] = res
                if res["multi_max"] < K:
                    lib.zk_rounds_free(r)
                    continue
                L.check(lib.zk_rounds_multi_evals(r, poly._h, K, lp))
                L.check(lib.zk_rounds_multi_absorb(r, lp, K))
                t1 = MP.alloc(field, n)
                L.check(lib.zk_rounds_multi_fold_evals(r, poly._h, t1._h, K, m_next, lp if m_next else None))
                folded = to_ints(t1.evaluated_values)
                cur = t1
                if m_next:                                            # finish the proof: zk_rounds_collect wants every round done
                    L.check(lib.zk_rounds_multi_absorb(r, lp, m_next))
                    cur = MP.alloc(field, n >> m_next)
                    L.check(lib.zk_rounds_multi_fold_evals(r, t1._h, cur._h, m_next, 0, None))
                L.check(lib.zk_rounds_multi_tail(r, cur._h))
                ch = np.zeros((logn, 4), np.uint64)
                L.check(lib.zk_rounds_collect(r, tr._h, None, None, L.p64(ch), None))
                lib.zk_rounds_free(r)
                rs = [FM.real(field, c) for c in to_ints(ch)][:K]
                legacy = FM.parts(form, K)
                fixed = FM.parts(form, K, FM.chunk_terms(field, len(legacy[0])))
                want = FM.fold_exact(field, table, K, rs)
                wrong = [j for j in range(n) if folded[j] != want[j]]
                res.update({
                    "challenges_match_model": rs == FM.first_challenges(field, table, K, nonce),
                    "w_max_over_radix": max(FM.weight_sums(field, rs, legacy)) / FM.radix(field),
                    "hot_lanes_before_fix": len(FM.over_range_lanes(field, table, K, rs, legacy)),
                    "hot_lanes_after_fix": len(FM.over_range_lanes(field, table, K, rs, fixed)),
                    "len": len(folded), "mismatches": len(wrong), "noncanonical": sum(1 for v in folded if v >= p),
                    "first_wrong": [[j, hex(folded[j]), hex(want[j])] for j in wrong[:2]],
                    "input_unchanged": bool(np.array_equal(poly.evaluated_values, table_limbs)),
                })
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
