"""Writes tests/golden/wiring_proof.bin: one small valid proof of the permutation check over FRI commitments (include/zkmle.h "Wiring: a
permutation check over committed tables") made by the Python model of tests/_wiring_model.py, in the layout tools/wiring_selftest.hip reads.
The library is used for the stored (Montgomery) form of the elements and for its checked host Keccak only.

  statement   BN254 Fr, d = 4, log_blowup = 1, log_final = 1, Q = 2, log_arity = 2 on grouped leaves, a coset, 4 bits of proof of work
  wiring      _wiring_model.wiring: a random permutation of the 48 cells, one random value per cycle
  layout      little-endian: "ZWFX"; the u32 field, d, log_blowup, log_final, Q, log_arity, log_group, grinding_bits; the u64 nonce; the
              coset (4 u64, stored form); then nine arrays, each a u64 byte count and its bytes: the verifier's six roots, the helper roots,
              round_polys, ys, the opening's round_polys, roots, final_table, query_values, query_paths

    python tests/golden/make_wiring_fixture.py [OUT]"""
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if path not in sys.path:
        sys.path.insert(0, path)

import _fri_ml_cases as FC
import _fri_ml_grouped_model as GM
import _wiring_model as WM

FIELD, D, B, F, Q, A, G_BITS = 3, 4, 1, 1, 2, 2, 4
COSET = 0x5EED5EED5EED5EED5EED
OUT = os.path.join(HERE, "wiring_proof.bin")
ARRAYS = ("own_roots", "h_roots", "polys", "ys", "open_polys", "roots", "final", "values", "paths")


def hasher(zk):
    return FC.hasher(zk, True)


def model_proof(zk):
    ws, ss = WM.wiring(FIELD, D, 424209)
    cms = [GM.commit(FIELD, t, B, COSET, hasher(zk)) for t in ws + ss]
    return WM.prove(cms, F, Q, A, WM.pow_transcript(D, F, G_BITS), hasher(zk))


def fixture_bytes(zk):
    pr = model_proof(zk)
    fl = WM.flat(zk, pr)
    out = b"ZWFX" + struct.pack("<8IQ", FIELD, D, B, F, Q, A, 2, G_BITS, pr["nonce"]) + zk.from_ints(FIELD, [COSET])[0].tobytes()
    for name in ARRAYS:
        data = fl[name].tobytes()
        out += struct.pack("<Q", len(data)) + data
    return out


if __name__ == "__main__":
    import __graft_entry__ as G
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "wb") as fh:
        fh.write(fixture_bytes(G.import_package()))
