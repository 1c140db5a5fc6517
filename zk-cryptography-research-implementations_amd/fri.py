"""FRI low-degree proof of a coefficient table (extension: the reference's fri/ crate is empty; definition in include/zkmle.h).

  layer 0 = low_degree_extend(coeffs, log_blowup, coset); each layer is committed by its Merkle root and folded in half by the
  transcript's challenge; the last layer is sent as its m = 2^log_final low coefficients; Q queries open a pair of every committed layer.

`prove` / `prove_codeword` run on the GPU (there is no CPU path); `verify` is host code and needs no device.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .mle import MultilinearPolynomial, _elem, limbs


class _Stats(C.Structure):
    _fields_ = [("layers", C.c_uint32), ("queries", C.c_uint32), ("ms_extend", C.c_float), ("ms_trees", C.c_float),
                ("ms_folds", C.c_float), ("ms_queries", C.c_float), ("ms_total", C.c_float)]


def sizes(d, log_blowup, log_final, nqueries):
    """-> (nroots, nfinal, nvalues, path_bytes) of a proof over a coefficient table of 2^d entries"""
    out = [C.c_size_t(0) for _ in range(4)]
    L.check(L.lib().zk_fri_proof_sizes(d, log_blowup, log_final, nqueries, *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


class FriProof:
    """The flat proof: roots (R, 32) bytes, final_coeffs (m, limbs), query_values (Q, R, 2, limbs), query_paths (path_bytes,) bytes;
    betas (R, limbs) and query_indices (Q,) are what the prover's transcript gave (diagnostic: the verifier derives its own)."""

    def __init__(self, field, d, log_blowup, log_final, nqueries, coset=None):
        self.field, self.d, self.log_blowup, self.log_final, self.nqueries = field, d, log_blowup, log_final, nqueries
        self.coset = None if coset is None else _elem(field, coset).copy()
        nroots, nfinal, nvalues, path_bytes = self.sizes
        n = limbs(field)
        self.roots = np.zeros((nroots, 32), np.uint8)
        self.final_coeffs = np.zeros((nfinal, n), np.uint64)
        self.betas = np.zeros((nroots, n), np.uint64)
        self.query_indices = np.zeros(nqueries, np.uint64)
        self.query_values = np.zeros((nqueries, nroots, 2, n), np.uint64)
        self.query_paths = np.zeros(path_bytes, np.uint8)

    @property
    def sizes(self):
        return sizes(self.d, self.log_blowup, self.log_final, self.nqueries)

    def _coset(self):
        return None if self.coset is None else L.p64(self.coset)


def _handle(transcript):
    return None if transcript is None else transcript._h


def fold(codeword, beta, coset=None):
    """one fold of a codeword on {coset w_len^k}: a new table of half the length"""
    h = C.c_void_p()
    cs = None if coset is None else L.p64(_elem(codeword.field, coset))
    L.check(L.lib().zk_fri_fold(codeword._h, L.p64(_elem(codeword.field, beta)), cs, C.byref(h)))
    return MultilinearPolynomial(codeword.field, _handle=h)


def _run(fn, poly, d, log_blowup, log_final, nqueries, coset, transcript):
    pr = FriProof(poly.field, d, log_blowup, log_final, nqueries, coset)
    L.check(fn(poly._h, log_blowup, log_final, nqueries, pr._coset(), _handle(transcript), L.p8(pr.roots), L.p64(pr.final_coeffs),
               L.p64(pr.betas), L.p64(pr.query_indices), L.p64(pr.query_values), L.p8(pr.query_paths)))
    return pr


def prove(coeffs, log_blowup, log_final, nqueries, coset=None, transcript=None):
    """the proof that the coefficient table `coeffs` (2^d entries) has degree below 2^d"""
    return _run(L.lib().zk_fri_prove, coeffs, len(coeffs).bit_length() - 1, log_blowup, log_final, nqueries, coset, transcript)


def prove_codeword(codeword, log_blowup, log_final, nqueries, coset=None, transcript=None):
    """the same from the 2^(d + log_blowup) evaluations; a codeword that is not of low degree gets a proof that does not verify"""
    d = len(codeword).bit_length() - 1 - log_blowup
    if d < 1:
        raise L.ZkError(L.ZK_E_ARG, "the codeword is no longer than its blow-up")
    return _run(L.lib().zk_fri_prove_codeword, codeword, d, log_blowup, log_final, nqueries, coset, transcript)


def verify(proof, transcript=None):
    """host only"""
    ok = C.c_int(0)
    vals, paths = np.ascontiguousarray(proof.query_values, np.uint64), np.ascontiguousarray(proof.query_paths, np.uint8)
    roots, fin = np.ascontiguousarray(proof.roots, np.uint8), np.ascontiguousarray(proof.final_coeffs, np.uint64)
    L.check(L.lib().zk_fri_verify(proof.field, proof.d, proof.log_blowup, proof.log_final, proof.nqueries, proof._coset(),
                                  _handle(transcript), L.p8(roots), L.p64(fin), L.p64(vals), L.p8(paths), C.byref(ok)))
    return bool(ok.value)


def last_stats():
    """milliseconds of the calling thread's last proof: the extension, the trees, the folds, the query gather"""
    st = _Stats()
    L.check(L.lib().zk_fri_last_stats(C.byref(st)))
    return {name: getattr(st, name) for name, _ in _Stats._fields_}
