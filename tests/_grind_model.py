"""Python model of the proof-of-work step of the FRI transcripts (helper of tests/test_grind_cpu.py and test_gpu_grind.py).  The definition is
the one of include/zkmle.h "Proof-of-work grinding":

  1. append "GRND" and the bit count g as a big-endian u32 (8 bytes, one append)
  2. w = the smallest unsigned 64-bit integer (>= start) such that Keccak256(everything absorbed so far || w as 8 big-endian bytes) has its
     first g bits zero; bit i of the digest is bit 7 - i mod 8 of byte i div 8
  3. append w, sample the challenge: the digest of step 2, absorbed back

written with oracle/pymodel.py's Transcript (everything absorbed so far as one byte string) and its keccak256, a copy of the transcript per
candidate.  Nothing here comes from the library.  PowTranscript puts the step in front of a chosen sample of an existing model, which is how
the models of tests/_fri_model.py and tests/_fri_ml_batch_model.py are extended without being edited."""
import copy

from oracle import pymodel as M

MAX_BITS = 32


def tag(bits):
    return b"GRND" + int(bits).to_bytes(4, "big")


def be64(w):
    return int(w).to_bytes(8, "big")


def leading_zero(digest, bits):
    """the first `bits` bits of the 32-byte digest are zero"""
    return int.from_bytes(digest, "big") >> (256 - bits) == 0


def candidate_digest(tr, w):
    c = copy.deepcopy(tr)
    c.append(be64(w))
    return M.keccak256(c.buf)


def grind(tr, bits, start=0):
    """steps 1 - 3 on `tr` -> the nonce"""
    assert 1 <= bits <= MAX_BITS
    M.Transcript.append(tr, tag(bits))
    w = start
    while not leading_zero(candidate_digest(tr, w), bits):
        w += 1
    M.Transcript.append(tr, be64(w))
    assert leading_zero(M.Transcript.sample(tr), bits)
    return w


def check(tr, bits, w):
    """the verifier's step on `tr` -> whether the challenge has its first `bits` bits zero"""
    M.Transcript.append(tr, tag(bits))
    M.Transcript.append(tr, be64(w))
    return leading_zero(M.Transcript.sample(tr), bits)


class PowTranscript(M.Transcript):
    """A transcript that takes the step right before its sample number `at` (counted from 0): with nonce = None it searches (a prover's), else
    it checks the given nonce (a verifier's; `.pow_ok` holds the answer).  bits = 0: a plain transcript.  The FRI prover of tests/_fri_model.py
    draws R challenges before its first index, the batch opener of tests/_fri_ml_batch_model.py 1 + R."""

    def __init__(self, bits, at, nonce=None):
        super().__init__()
        self.bits, self.at, self.nonce, self.count, self.pow_ok = bits, at, nonce, 0, None

    def sample(self):
        if self.bits and self.count == self.at:
            if self.nonce is None:
                self.nonce = grind(self, self.bits)
                self.pow_ok = True
            else:
                self.pow_ok = check(self, self.bits, self.nonce)
        self.count += 1
        return super().sample()
