"""Writes tests/golden/zerocheck_family_model_proofs.json: SHA-256 digests of the proofs that the Python models of the zerocheck family
produce (tests/_zerocheck_model.py, _zerocheck_gate_model.py, _wiring_model.py, _plonk_model.py, _lookup_model.py, _plonk_lookup_model.py and
_plonk_lookup_columns_model.py), so that a change of the models that changes a proof, a verdict, a size or a C array shows.  Only the models'
public names are used: prove, verify, sizes, flat, pow_transcript, the instance generators and the commitment models.

  grid      per protocol the cases with d <= 4 of its own tests/test_*_cpu.py CASES (copied below), each under every schedule (log_arity,
            grouped) that runs there -- log_arity 2 where d - f >= 2; the column protocol has one schedule -- at Q = 4 on a caller's
            transcript that has absorbed PRIOR
  variants  the honest proof and each cheating prover (cheat=True, or "wiring" and "lookup") on a false instance: the model's own generator's,
            but for the product zerocheck, which has none (C[2^d - 1] is one more), and the missing lookup row of the two Plonk kinds with
            lookups (see `tables`); for the three protocols with public inputs all of these at l = 0 and at the case's own l; for the first
            case of each protocol with d - f >= 2 the honest proof through pow_transcript(d, f, 4) as well, under each schedule
  digest    SHA-256 of the JSON of {"proof": the returned dict, "next": one challenge drawn from the caller's transcript afterwards}, with
            bytes as hex, tuples as lists, keys sorted and no spaces
  verify    the model verifier's (ok, failed) on the proof, and on the proof with the last opened value one more
  sizes     the model's sizes(..) of the case
  flat      with the library (entries(zk=..)): SHA-256 over the arrays of flat(zk, proof) in name order, each as name, dtype, shape and bytes

entries() asserts that every honest proof verifies, that every changed one fails at check d or d + 1 and that every cheating one fails at a
check in 1 .. d.

    python tests/golden/make_zerocheck_family_model_proofs.py [OUT]      (the whole grid, 466 entries: about 20 seconds with the library's
                                                                          host Keccak, which __main__ uses after checking it against the
                                                                          model's; the library also converts the flat arrays)"""
import collections
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

import _fri_ml_grouped_model as GM
import _fri_pcs_model as PM
import _lookup_model as LM
import _ntt_model as NM
import _plonk_lookup_columns_model as KC
import _plonk_lookup_model as KL
import _plonk_model as KM
import _wiring_model as WM
import _zerocheck_gate_model as ZG
import _zerocheck_model as ZM
from oracle import pymodel as M

SCHEDULES = [(1, False), (2, False), (2, True)]              # (log_arity, grouped)
# (field, d, b, f, coset), then l, then looked, then the column test's bits: the CASES of the seven tests/test_*_cpu.py with d <= 4
PLAIN = [(0, 1, 1, 0, False), (3, 1, 2, 0, True), (0, 2, 2, 0, True), (3, 2, 1, 1, False), (3, 2, 1, 0, False), (0, 3, 1, 1, False), (3, 3, 2, 0, True),
         (3, 3, 1, 2, True), (0, 4, 2, 0, True), (3, 4, 1, 2, False), (0, 4, 1, 3, False)]
PLONK = [(0, 1, 1, 0, False, 0), (3, 1, 2, 0, True, 1), (3, 1, 1, 0, False, 2), (0, 2, 2, 0, True, 3), (3, 2, 1, 1, False, 4), (3, 2, 1, 0, False, 1),
         (0, 3, 1, 1, False, 8), (3, 3, 2, 0, True, 3), (3, 3, 1, 2, True, 0), (0, 4, 2, 0, True, 3), (3, 4, 1, 2, False, 16), (0, 4, 1, 3, False, 1)]
PLONK_LOOKUP = [(0, 1, 1, 0, False, 0, "all"), (3, 1, 2, 0, True, 1, "some"), (3, 1, 1, 0, False, 2, "none"), (0, 2, 2, 0, True, 3, "some"),
                (3, 2, 1, 1, False, 4, "all"), (3, 2, 1, 0, False, 1, "none"), (0, 3, 1, 1, False, 8, "some"), (3, 3, 2, 0, True, 3, "all"),
                (3, 3, 1, 2, True, 0, "none"), (0, 4, 2, 0, True, 3, "some"), (3, 4, 1, 2, False, 16, "all"), (0, 4, 1, 3, False, 1, "none")]
COLUMNS = [(0, 2, 1, 0, False, 0, "all", 0), (3, 2, 2, 0, True, 1, "some", 4), (0, 3, 1, 0, True, 3, "some", 0), (3, 3, 2, 1, False, 0, "none", 0),
           (0, 4, 2, 0, True, 3, "some", 4), (3, 4, 1, 1, False, 1, "all", 0), (3, 4, 1, 2, True, 0, "some", 0)]
# cheats: (the variant's name, prove's `cheat`, the false instance it runs on)
Kind = collections.namedtuple("Kind", "name model cases mul cheats")
ONE, TWO = (("cheat", True, "false"),), (("cheat-wiring", "wiring", "wiring"), ("cheat-lookup", "lookup", "lookup"))
KINDS = [Kind("zerocheck", ZM, tuple(PLAIN), 47, ONE), Kind("zerocheck_gate", ZG, tuple(PLAIN), 59, ONE), Kind("wiring", WM, tuple(PLAIN), 59, ONE),
         Kind("plonk", KM, tuple(PLONK), 67, ONE), Kind("lookup", LM, tuple(PLAIN), 59, ONE), Kind("plonk_lookup", KL, tuple(PLONK_LOOKUP), 71, TWO),
         Kind("plonk_lookup_columns", KC, tuple(COLUMNS), 73, TWO)]
Q = 4
POW_BITS = 4
PRIOR = b"what the caller had absorbed before"
OUT = os.path.join(HERE, "zerocheck_family_model_proofs.json")


def tables(name, field, d, l, looked, false):
    """-> (the given integer tables of one instance, its public values); false: None or the name of the part that is made false"""
    p, n = NM.MODULUS[field], 1 << d
    if name == "zerocheck":
        A, B = NM.random_ints(field, n, 9300 + 17 * d + field), NM.random_ints(field, n, 9400 + 19 * d + field)
        Cc = [a * b % p for a, b in zip(A, B)]
        if false:
            Cc[n - 1] = (Cc[n - 1] + 1) % p
        return [A, B, Cc], ()
    if name == "zerocheck_gate":
        return ZG.circuit(field, n, 9700 + 17 * d + field, n - 1 if false else None), ()
    if name == "wiring":
        ws, ss = WM.wiring(field, d, 4100 + 13 * d + field, bool(false))
        return ws + ss, ()
    if name == "plonk":
        return KM.circuit(field, d, 5100 + 13 * d + field + l, l, false_wiring=bool(false))
    if name == "lookup":
        tabs = LM.instance(field, d, 5100 + 13 * d + field)
        return (LM.falsified(tabs, n - 1, p, True) if false else tabs), ()
    seed = 6100 + 13 * d + field + l if name == "plonk_lookup" else 7300 + 17 * d + field + l
    tabs, pub = KL.circuit(field, d, seed, l, looked, false_wiring=false == "wiring")
    if false == "lookup":                                     # the last row is a lookup row and no table row holds its triple (the generator's own
        tabs[11][n - 1] = 1                                   # `miss` appends a table row, for which 2^d = 2 rows may have no room)
        triple = tuple(tabs[j][n - 1] for j in range(3))
        tabs[14] = [(v + 1) % p if (tabs[12][y], tabs[13][y], v) == triple else v for y, v in enumerate(tabs[14])]
        assert KL.satisfied(tabs, pub, p) == (True, True, False)
    return tabs, pub


@functools.lru_cache(maxsize=None)
def statement(kind, case, grouped, l, false, hasher):
    """-> (the model commitments, the public values)"""
    field, d, b, f, with_coset = case[:5]
    coset = random.Random(kind.mul * d + b + field).randrange(2, NM.MODULUS[field]) if with_coset else 1
    tabs, pub = tables(kind.name, field, d, l, case[6] if len(case) > 6 else None, false)
    if kind.model is KC:
        return KC.commitments(field, tabs, b, coset, hasher), tuple(pub)
    return tuple((GM if grouped else PM).commit(field, t, b, coset, hasher) for t in tabs), tuple(pub)


def canonical(v):
    if isinstance(v, (bytes, bytearray)):
        return bytes(v).hex()
    if isinstance(v, dict):
        return {k: canonical(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [canonical(x) for x in v]
    assert v is None or isinstance(v, (bool, int, str)), type(v)
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


def flat_digest(fl):
    h = hashlib.sha256()
    for name in sorted(fl):
        h.update(("%s %s %s " % (name, fl[name].dtype.str, list(fl[name].shape))).encode() + fl[name].tobytes())
    return h.hexdigest()


def entry(kind, case, sched, variant, l, cheat, false, pow_bits, hasher, zk):
    field, d, b, f = case[:4]
    a, grouped = sched
    model, p = kind.model, NM.MODULUS[field]
    has_pub, columns = len(case) > 5, kind.model is KC
    cms, pub = statement(kind, case, grouped, l, false, hasher)

    def transcript(nonce=None):
        if pow_bits:
            return model.pow_transcript(d, f, pow_bits, nonce, prefix=PRIOR)
        tr = Transcript(hasher)
        tr.append(PRIOR)
        return tr

    tr = transcript()
    args = ((list(pub),) if has_pub else ()) + ((f, Q) if columns else (f, Q, a))
    pr = model.prove(*(cms if columns else (list(cms),)), *args, tr, hasher, cheat=cheat)
    text = json.dumps(canonical({"proof": pr, "next": tr.challenge(p)}), sort_keys=True, separators=(",", ":"))
    op = pr["opening"]
    changed = dict(pr, opening=dict(op, ys=op["ys"][:-1] + [op["ys"][-1][:-1] + [(op["ys"][-1][-1] + 1) % p]]))
    nonce = pr["nonce"] if pow_bits else None
    verdict, verdict_changed = (list(model.verify(q, tr=transcript(nonce), hasher=hasher)) for q in (pr, changed))
    if cheat:
        assert verdict[0] is False and 1 <= verdict[1] <= d, (kind.name, case, sched, variant, verdict)
    else:
        assert verdict == [True, None], (kind.name, case, sched, variant, verdict)
    assert verdict_changed[0] is False and (cheat or verdict_changed[1] in (d, d + 1)), (kind.name, case, sched, variant, verdict_changed)
    out = {"protocol": kind.name, "case": [v if isinstance(v, str) else int(v) for v in case], "schedule": [a, bool(grouped)], "variant": variant,
           "digest": hashlib.sha256(text.encode()).hexdigest(), "verify": verdict, "verify_changed": verdict_changed,
           "sizes": list(model.sizes(d, b, f, Q) if columns else model.sizes(d, b, f, Q, a, grouped))}
    if zk is not None:
        out["flat"] = flat_digest(model.flat(zk, pr))
    return out


def entries(max_d=None, hasher=M.keccak256, zk=None):
    """the grid's entries in a fixed order; max_d: only the cases with d <= max_d; hasher: another implementation of Keccak-256, for the trees
    and the transcript; zk: the library's package, for the digests of the flat arrays"""
    out = []
    for kind in KINDS:
        pow_case = next(c for c in kind.cases if c[1] - c[3] >= 2)
        for case in kind.cases:
            d, f = case[1], case[3]
            if max_d is not None and d > max_d:
                continue
            scheds = [(2, True)] if kind.model is KC else [s for s in SCHEDULES if s[0] == 1 or d - f >= 2]
            assert scheds
            ls = [None] if len(case) <= 5 else sorted({0, case[5]})
            for sched in scheds:
                for l in ls:
                    pre = "" if l is None else "l%d-" % l
                    out.append(entry(kind, case, sched, pre + "honest", l, None, None, 0, hasher, zk))
                    for name, cheat, false in kind.cheats:
                        out.append(entry(kind, case, sched, pre + name, l, cheat, false, 0, hasher, zk))
                if case == pow_case:
                    out.append(entry(kind, case, sched, "pow%d" % POW_BITS, ls[-1], None, None, POW_BITS, hasher, zk))
    return out


def dump(rows):
    return "[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in rows) + "\n]\n"


if __name__ == "__main__":
    import __graft_entry__ as G
    import _fri_ml_columns_model as CM
    zk = G.import_package()
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as fh:
        fh.write(dump(entries(hasher=CM.check_host_keccak(zk), zk=zk)))
