"""Python model of the WIDE multilinear opening of several FRI commitments (helper of tests/test_fri_ml_wide_cpu.py, test_gpu_fri_ml_wide.py and
_plonk_lookup_model.py).  The definition is the one of include/zkmle.h "FRI commitments opened together, wide": the protocol of
tests/_fri_ml_batch_model.py byte for byte, for up to 32 commitments.  Nothing in that model's prover or verifier depends on the number of
commitments except one bound, its KMAX = 16, which it reads when it is called; the functions here run it under KMAX = 32 and put the bound back.

`pow_transcript(d, f, bits, nonce, prefix)`: the transcript of an opening of ONE point with the proof-of-work step, which stands in front of
the first index: sample number 1 (gamma) + R (the rounds).
Everything is Python integers; nothing here knows how the library works."""
import contextlib

import _fri_ml_batch_model as BM
import _fri_ml_family_model as FAM
import _grind_model as GR
from oracle import pymodel as M

KMAX = 32
steps, sizes, flat = BM.steps, BM.sizes, BM.flat


@contextlib.contextmanager
def _wide():
    old = FAM.KMAX
    FAM.KMAX = KMAX
    try:
        yield
    finally:
        FAM.KMAX = old


def open_batch(cms, points, f, Q, a=1, tr=None, hasher=M.keccak256):
    assert 1 <= len(cms) <= KMAX
    with _wide():
        return BM.open_batch(cms, points, f, Q, a, tr, hasher)


def verify(op, tr=None, hasher=M.keccak256):
    if not 1 <= op["k"] <= KMAX:
        return False
    with _wide():
        return BM.verify(op, tr, hasher) and getattr(tr, "pow_ok", None) is not False


def pow_transcript(d, f, bits, nonce=None, prefix=b""):
    tr = GR.PowTranscript(bits, 1 + (d - f), nonce)
    tr.append(prefix)
    return tr
