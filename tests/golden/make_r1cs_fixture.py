"""Writes tests/golden/r1cs_proof.bin: one small valid Spartan proof (include/zkmle.h "R1CS satisfiability: Spartan over a FRI commitment") made by
the Python model of tests/_r1cs_model.py, with its instance, in the layout tools/r1cs_selftest.hip reads.  The library is used for the stored
(Montgomery) form of the elements and for its checked host Keccak only.

  statement   BN254 Fr, s = 4, d = 5, l = 2, log_blowup = 1, log_final = 1, Q = 3, log_arity = 2 on grouped leaves, a coset
  layout      little-endian: "R1FX"; the u32 field, s, d, l, log_blowup, log_final, Q, log_arity, log_group; the coset (4 u64, stored form);
              for A, B, C: a u64 entry count, the rows (u32 each), the columns (u32 each), the values (4 u64 each, stored form); then eleven
              arrays, each a u64 byte count and its bytes: the witness root, the public values, round_polys, va vb vc, c, the opening's
              round_polys, roots, final_table, challenges, query_values, query_paths

    python tests/golden/make_r1cs_fixture.py [OUT]"""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if path not in sys.path:
        sys.path.insert(0, path)

import _fri_ml_cases as FC
import _fri_ml_grouped_model as GM
import _r1cs_model as RM

FIELD, S, D, NPUB, B, F, Q, A = 3, 4, 5, 2, 1, 1, 3, 2
COSET = 0x5EED5EED5EED5EED5EED
OUT = os.path.join(HERE, "r1cs_proof.bin")


def hasher(zk):
    return FC.hasher(zk, True)


def model_case(zk):
    """(mats, public, the witness commitment, the proof)"""
    mats, w, public = RM.satisfied_instance(FIELD, S, D, NPUB, 515151)
    cm = GM.commit(FIELD, w, B, COSET, hasher(zk))
    return mats, public, cm, RM.prove(FIELD, S, D, mats, cm, public, F, Q, A, None, hasher(zk))


def fixture_bytes(zk):
    mats, public, cm, pr = model_case(zk)
    fl = RM.flat(zk, pr)
    op = fl["opening"]
    out = b"R1FX" + struct.pack("<9I", FIELD, S, D, NPUB, B, F, Q, A, 2) + zk.from_ints(FIELD, [COSET])[0].tobytes()
    for m in mats:
        out += struct.pack("<Q", len(m)) + np.array([e[0] for e in m], np.uint32).tobytes() + np.array([e[1] for e in m], np.uint32).tobytes()
        out += zk.from_ints(FIELD, [e[2] for e in m]).tobytes()
    arrays = (op["root"], zk.from_ints(FIELD, public).tobytes(), fl["polys"].tobytes(), fl["vs"].tobytes(), op["c"].tobytes(), op["polys"].tobytes(), op["roots"],
              op["final"].tobytes(), op["challenges"].tobytes(), op["values"].tobytes(), op["paths"])
    for data in arrays:
        out += struct.pack("<Q", len(data)) + bytes(data)
    return out


if __name__ == "__main__":
    import __graft_entry__ as G
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "wb") as fh:
        fh.write(fixture_bytes(G.import_package()))
