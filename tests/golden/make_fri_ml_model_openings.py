"""Writes tests/golden/fri_ml_model_openings.json: SHA-256 digests of the openings that the Python models of the multilinear FRI opening
family produce (tests/_fri_ml_{points,arity,grouped,batch}_model.py), so that a change of the models that changes an opening shows.  Only
the models' public names are used: open_points / open_batch, verify, GM.commit, PM.commit.

  grid      the 7 cases (field, d, b, f, P, coset) of tests/test_fri_ml_batch_cpu.py CASES at Q = 4: the several-point protocol, arity 2 and
            grouped leaves on each (every case has R >= 2), the batch at k in {1, 2, 5} under (1, ungrouped), (2, ungrouped), (2, grouped)
  digest    SHA-256 of the JSON of {"opening": the returned dict, "next": one challenge drawn from the caller's transcript afterwards}, with
            bytes as hex, tuples as lists, keys sorted and no spaces
  verify    the model verifier's answer on the opening, and on the opening with one claim changed

    python tests/golden/make_fri_ml_model_openings.py [OUT]      (the whole grid: under a minute of pure Python)"""
import functools
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if path not in sys.path:
        sys.path.insert(0, path)

import _fri_ml_arity_model as AM
import _fri_ml_batch_model as BM
import _fri_ml_grouped_model as GM
import _fri_ml_points_model as PT
import _fri_pcs_model as PM
import _ntt_model as NM
from oracle import pymodel as M

CASES = [(0, 3, 1, 1, 1, False), (3, 3, 2, 0, 2, True), (3, 4, 1, 2, 8, False), (0, 4, 2, 0, 2, True), (0, 6, 2, 3, 8, True), (3, 6, 1, 1, 1, True),
         (0, 6, 1, 0, 2, False)]
SCHEDULES = [(1, False), (2, False), (2, True)]              # (log_arity, grouped)
KS = (1, 2, 5)
Q = 4
PRIOR = b"what the caller had absorbed before"
OUT = os.path.join(HERE, "fri_ml_model_openings.json")


@functools.lru_cache(maxsize=None)
def commitment(field, d, b, with_coset, grouped, j, hasher):
    coeffs = NM.random_ints(field, 1 << d, 8100 + 13 * d + field + 101 * j)
    coset = random.Random(43 * d + b + field).randrange(2, NM.MODULUS[field]) if with_coset else 1
    return (GM if grouped else PM).commit(field, coeffs, b, coset, hasher)


def points_for(field, d, P):
    p, rng = NM.MODULUS[field], random.Random(103 * d + 7 * P + field)
    pts = [[rng.randrange(p) for _ in range(d)] for _ in range(P)]
    pts[0][d - 1] = p - 1
    return pts


def canonical(v):
    if isinstance(v, (bytes, bytearray)):
        return bytes(v).hex()
    if isinstance(v, dict):
        return {k: canonical(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [canonical(x) for x in v]
    assert isinstance(v, (bool, int, str)), type(v)
    return v


class Transcript(M.Transcript):
    """oracle/pymodel.py Transcript hashing with `hasher`"""

    def __init__(self, hasher):
        super().__init__()
        self.hasher = hasher

    def sample(self):
        d = self.hasher(bytes(self.buf))
        self.buf += d
        return d


def transcript(hasher):
    tr = Transcript(hasher)
    tr.append(PRIOR)
    return tr


def entry(protocol, case, k, run, verify, hasher):
    field, d, b, f, P, with_coset = case
    p, tr = NM.MODULUS[field], transcript(hasher)
    op = run(tr)
    text = json.dumps(canonical({"opening": op, "next": tr.challenge(p)}), sort_keys=True, separators=(",", ":"))
    if k is None:
        changed = dict(op, ys=[(op["ys"][0] + 1) % p] + op["ys"][1:])
    else:
        changed = dict(op, ys=op["ys"][:-1] + [op["ys"][-1][:-1] + [(op["ys"][-1][-1] + 1) % p]])
    return {"protocol": protocol, "case": [int(v) for v in case], "k": k, "digest": hashlib.sha256(text.encode()).hexdigest(),
            "verify": bool(verify(op, transcript(hasher), hasher)), "verify_changed": bool(verify(changed, transcript(hasher), hasher))}


def entries(max_d=None, hasher=M.keccak256):
    """the grid's entries in a fixed order; max_d: only the cases with d <= max_d; hasher: another implementation of Keccak-256, for the trees and the transcript"""
    out = []
    for case in CASES:
        field, d, b, f, P, with_coset = case
        if max_d is not None and d > max_d:
            continue
        pts = points_for(field, d, P)
        for (a, grouped), name, model in zip(SCHEDULES, ("points", "arity", "grouped"), (PT, AM, GM)):
            cm = commitment(field, d, b, with_coset, grouped, 0, hasher)
            out.append(entry(name, case, None, lambda tr: model.open_points(cm, pts, f, Q, tr, hasher=hasher), model.verify, hasher))
        for a, grouped in SCHEDULES:
            for k in KS:
                cms = [commitment(field, d, b, with_coset, grouped, j, hasher) for j in range(k)]
                out.append(entry("batch-a%d%s" % (a, "g" if grouped else ""), case, k, lambda tr: BM.open_batch(cms, pts, f, Q, a, tr, hasher), BM.verify, hasher))
    return out


def dump(rows):
    return "[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in rows) + "\n]\n"


if __name__ == "__main__":
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as fh:
        fh.write(dump(entries()))
