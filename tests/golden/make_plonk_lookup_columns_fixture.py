"""Writes tests/golden/plonk_lookup_columns_proof.bin: one small valid Plonk proof with lookup rows on column commitments (include/zkmle.h
"Plonk with lookups on column commitments") made by the Python model of tests/_plonk_lookup_columns_model.py, in the layout
tools/plonk_lookup_columns_selftest.hip reads.  The library is used for the stored (Montgomery) form of the elements and for its checked host
Keccak only.

  statement   BN254 Fr, d = 4, log_blowup = 1, log_final = 1, Q = 2, a coset, one public value, 4 bits of proof of work
  circuit     _plonk_lookup_model.circuit: a random wiring of the 48 cells, 1 public-input row, then additions, multiplications and random rows;
              about half the rows are lookup rows into a table of their own triples
  layout      little-endian: "ZLCX"; the u32 field, d, log_blowup, log_final, Q, grinding_bits; the u64 nonce; the coset (4 u64, stored form);
              then ten arrays, each a u64 byte count and its bytes: the verifier's two roots (witness, circuit), the public values, the helper
              roots (M, the helpers), round_polys, ys, the opening's round_polys, roots, final_table, query_values, query_paths

    python tests/golden/make_plonk_lookup_columns_fixture.py [OUT]"""
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if path not in sys.path:
        sys.path.insert(0, path)

import _fri_ml_columns_model as CM
import _plonk_lookup_columns_model as KC

FIELD, D, B, F, Q, G_BITS, L_PUBLIC = 3, 4, 1, 1, 2, 4, 1
COSET = 0x5EED5EED5EED5EED5EED
OUT = os.path.join(HERE, "plonk_lookup_columns_proof.bin")
ARRAYS = ("own_roots", "pub", "h_roots", "polys", "ys", "open_polys", "roots", "final", "values", "paths")


def hasher(zk):
    return CM.check_host_keccak(zk)


def model_proof(zk):
    tabs, pub = KC.circuit(FIELD, D, 434343, L_PUBLIC)
    wit, cir = KC.commitments(FIELD, tabs, B, COSET, hasher(zk))
    return KC.prove(wit, cir, pub, F, Q, KC.pow_transcript(D, F, G_BITS), hasher(zk))


def fixture_bytes(zk):
    pr = model_proof(zk)
    fl = KC.flat(zk, pr)
    out = b"ZLCX" + struct.pack("<6IQ", FIELD, D, B, F, Q, G_BITS, pr["nonce"]) + zk.from_ints(FIELD, [COSET])[0].tobytes()
    for name in ARRAYS:
        data = fl[name].tobytes()
        out += struct.pack("<Q", len(data)) + data
    return out


if __name__ == "__main__":
    import __graft_entry__ as G
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "wb") as fh:
        fh.write(fixture_bytes(G.import_package()))
