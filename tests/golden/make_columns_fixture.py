"""Writes tests/golden/columns_proof.bin: one small valid opening of column commitments (include/zkmle.h "Column commitments opened together")
made by the Python model of tests/_fri_ml_columns_model.py, in the layout tools/columns_selftest.hip reads.
The library is used for the stored (Montgomery) form of the elements and for its checked host Keccak only.

  statement   BN254 Fr, d = 4, log_blowup = 1, log_final = 1, Q = 2, three commitments of widths 3, 1 and 17 (a leaf whose message ends one byte
              into a block), two points, a coset, 4 bits of proof of work
  layout      little-endian: "ZCFX"; the u32 field, d, log_blowup, log_final, Q, grinding_bits, m, npoints; the u64 nonce; the coset (4 u64,
              stored form); the m u32 widths; then eight arrays, each a u64 byte count and its bytes: the verifier's m roots, the points, ys,
              round_polys, roots, final_table, query_values, query_paths

    python tests/golden/make_columns_fixture.py [OUT]"""
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if path not in sys.path:
        sys.path.insert(0, path)

import _fri_ml_cases as FC
import _fri_ml_columns_model as CM
import _ntt_model as NM

FIELD, D, B, F, Q, G_BITS, WIDTHS, P = 3, 4, 1, 1, 2, 4, (3, 1, 17), 2
COSET = 0x5EED5EED5EED5EED5EED
OUT = os.path.join(HERE, "columns_proof.bin")
ARRAYS = ("own_roots", "points", "ys", "polys", "roots", "final", "values", "paths")


def model_opening(zk):
    hasher = CM.check_host_keccak(zk)
    cms = [CM.commit(FIELD, [NM.random_ints(FIELD, 1 << D, 515100 + 101 * j + 7 * c) for c in range(w)], B, COSET, hasher) for j, w in enumerate(WIDTHS)]
    tr = CM.pow_transcript(D, F, G_BITS)
    op = CM.open_columns(cms, FC.points_for(FIELD, D, P, 515109), F, Q, tr, hasher)
    assert CM.verify(op, CM.pow_transcript(D, F, G_BITS, tr.nonce), hasher)
    return op, tr.nonce


def fixture_bytes(zk):
    op, nonce = model_opening(zk)
    fl = CM.flat(zk, op)
    out = b"ZCFX" + struct.pack("<8IQ", FIELD, D, B, F, Q, G_BITS, len(WIDTHS), P, nonce) + zk.from_ints(FIELD, [COSET])[0].tobytes()
    out += struct.pack("<%dI" % len(WIDTHS), *WIDTHS)
    for name in ARRAYS:
        data = fl[name].tobytes()
        out += struct.pack("<Q", len(data)) + data
    return out


if __name__ == "__main__":
    import __graft_entry__ as G
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "wb") as fh:
        fh.write(fixture_bytes(G.import_package()))
