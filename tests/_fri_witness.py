"""The committed operands of the FRI fold's last step that need the SECOND subtraction of fe_from_u_below_2p
(tests/golden/fri_fold_witnesses.json, found by tools/find_fold_witness.hip), as Python integers.  Helper of tests/test_fri_arith_cpu.py,
tests/test_gpu_fri_edges.py and, through tests/_fri_ml_edges.py, of tests/test_fri_ml_edges_cpu.py and tests/test_gpu_fri_ml_edges.py.

Everything in the file is in the stored (Montgomery) form x R mod p, R = 2^256; `real` leaves it."""
import json
import os

import _ntt_model as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 1 << 256


def limbs_to_int(limbs):
    return sum(int(w, 16) << (64 * k) for k, w in enumerate(limbs))


def int_to_limbs(v):
    return " ".join("%016x" % ((v >> (64 * k)) & (2 ** 64 - 1)) for k in range(4))


def real(field, stored):
    p = NM.MODULUS[field]
    return stored * pow(R, -1, p) % p


def stored(field, value):
    return value * R % NM.MODULUS[field]


def load(field, name="fri_fold_witnesses.json"):
    """-> (gamma, s, [t, ...]) of one field, stored-form integers.  name = "gkr_ufold_witnesses.json": the operands (r, a, [b, ...]) of
    ufold, the fold of the GKR round kernels (same tool, ufold mode)"""
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        d = json.load(f)["fields"][str(field)]
    return limbs_to_int(d["gamma"]), limbs_to_int(d["s"]), [limbs_to_int(w["t"]) for w in d["witnesses"]]
