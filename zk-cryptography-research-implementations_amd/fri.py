"""FRI low-degree proof of a coefficient table (extension: the reference's fri/ crate is empty; definition in include/zkmle.h).

  layer 0 = low_degree_extend(coeffs, log_blowup, coset); each layer is committed by its Merkle root and folded in half by the
  transcript's challenge; the last layer is sent as its m = 2^log_final low coefficients; Q queries open a pair of every committed layer.

`prove` / `prove_codeword` run on the GPU (there is no CPU path); `verify` is host code and needs no device.

The evaluation opening on top of it (include/zkmle.h "FRI polynomial commitment"): `commit` keeps the coefficients, the codeword and its tree
in HBM; `open_at` proves f_j(z) = y_j for k commitments at one point with one proof (the DEEP quotient, proved low-degree, every query tied
back to the roots); `verify_opening` is host code and needs nothing but the roots.

The same commitment opened as a MULTILINEAR polynomial (include/zkmle.h "FRI commitment opened as a multilinear polynomial"): the committed
table read as evaluations over the cube, `open_multilinear` proves y = evaluate(table, z) by a sumcheck interleaved with Lagrange-form folds of
the codeword; `verify_multilinear` is host code and needs nothing but the root.  `open_multilinear_points` opens ONE commitment at up to
eight points with one proof (include/zkmle.h "FRI commitment opened at several points"): the layers and trees are built once.  With
`log_arity=2` it commits every second folded layer only (include/zkmle.h "FRI commitment opened with a fold arity"): a third of the leaves hashed.
On a commitment made with `commit(.., log_group=2)` every tree has one leaf per fold coset (include/zkmle.h "FRI commitment opened with grouped
leaves"): a quarter of that again, and one path per step instead of four, so the proof shrinks.
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

    def __init__(self, field, d, log_blowup, log_final, nqueries, coset=None, grinding_bits=0):
        self.field, self.d, self.log_blowup, self.log_final, self.nqueries = field, d, log_blowup, log_final, nqueries
        self.grinding_bits, self.pow_nonce = grinding_bits, 0      # the proof-of-work step in front of the indices, and its nonce
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


def prove(coeffs, log_blowup, log_final, nqueries, coset=None, transcript=None, grinding_bits=0):
    """the proof that the coefficient table `coeffs` (2^d entries) has degree below 2^d.  grinding_bits = g > 0: a proof-of-work nonce with g
    leading zero bits is found on the GPU before the indices are drawn (include/zkmle.h "Proof-of-work grinding"); the proof carries g and it"""
    pr = FriProof(coeffs.field, len(coeffs).bit_length() - 1, log_blowup, log_final, nqueries, coset, grinding_bits)
    nonce = C.c_uint64(0)
    L.check(L.lib().zk_fri_prove_pow(coeffs._h, log_blowup, log_final, nqueries, pr._coset(), _handle(transcript), L.p8(pr.roots),
                                     L.p64(pr.final_coeffs), L.p64(pr.betas), L.p64(pr.query_indices), L.p64(pr.query_values),
                                     L.p8(pr.query_paths), grinding_bits, C.byref(nonce)))
    pr.pow_nonce = int(nonce.value)
    return pr


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
    L.check(L.lib().zk_fri_verify_pow(proof.field, proof.d, proof.log_blowup, proof.log_final, proof.nqueries, proof._coset(),
                                      _handle(transcript), L.p8(roots), L.p64(fin), L.p64(vals), L.p8(paths),
                                      getattr(proof, "grinding_bits", 0), getattr(proof, "pow_nonce", 0), C.byref(ok)))
    return bool(ok.value)


class _GrindStats(C.Structure):
    _fields_ = [("candidates", C.c_uint64), ("launches", C.c_uint32), ("ms", C.c_float)]


def grind_last_stats():
    """the calling thread's last GPU nonce search (Transcript.grind, or a prover's): the candidates up to and including the nonce, the launches,
    and the milliseconds of the launches with their result reads"""
    st = _GrindStats()
    L.check(L.lib().zk_transcript_grind_last_stats(C.byref(st)))
    return {name: getattr(st, name) for name, _ in _GrindStats._fields_}


def last_stats():
    """milliseconds of the calling thread's last proof: the extension, the trees, the folds, the query gather"""
    st = _Stats()
    L.check(L.lib().zk_fri_last_stats(C.byref(st)))
    return {name: getattr(st, name) for name, _ in _Stats._fields_}


# ---- the evaluation opening ------------------------------------------------------------------------------------------------------------
class _PcsStats(C.Structure):
    _fields_ = [("polys", C.c_uint32), ("batch", C.c_uint32), ("ms_evals", C.c_float), ("ms_quotient", C.c_float), ("ms_fri", C.c_float),
                ("ms_gather", C.c_float), ("ms_total", C.c_float)]


def pcs_sizes(k, d, log_blowup, log_final, nqueries):
    """-> sizes(..) + (nopened, opened_path_bytes) of an opening of k polynomials of 2^d coefficients"""
    out = [C.c_size_t(0) for _ in range(6)]
    L.check(L.lib().zk_fri_pcs_sizes(k, d, log_blowup, log_final, nqueries, *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


class FriCommitment:
    """The prover's side of a commitment: a device copy of the coefficients, the codeword and every level of its Merkle tree.  `root` is all a
    verifier needs.  Use as a context manager, or call free()."""

    def __init__(self, field, d, log_blowup, coset, handle):
        self.field, self.d, self.log_blowup, self._h = field, d, log_blowup, handle
        self.log_group = int(L.lib().zk_fri_commitment_log_group(handle))
        self.coset = None if coset is None else _elem(field, coset).copy()
        root = np.zeros(32, np.uint8)
        L.check(L.lib().zk_fri_commitment_root(handle, L.p8(root)))
        self.root = root.tobytes()

    def codeword(self):
        """a copy of the N evaluations f(c w^i) as a table of its own"""
        h, out = C.c_void_p(), C.c_void_p()
        L.check(L.lib().zk_fri_commitment_codeword(self._h, C.byref(h)))
        L.check(L.lib().zk_table_clone(h, C.byref(out)))
        return MultilinearPolynomial(self.field, _handle=out)

    def free(self):
        if self._h is not None:
            L.lib().zk_fri_commitment_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:      # noqa: BLE001  (interpreter shutdown)
            pass


def commit(coeffs, log_blowup, coset=None, log_group=0):
    """the commitment to the coefficient table `coeffs` (2^d entries): its root is root_0 of `prove` on the same input.  log_group = 2: the
    tree's leaves are the cosets of the first fold by 4 (a quarter of the hashes); only open_multilinear_points(.., log_arity=2) opens it"""
    h = C.c_void_p()
    cs = None if coset is None else L.p64(_elem(coeffs.field, coset))
    if log_group == 0:
        L.check(L.lib().zk_fri_commit(coeffs._h, log_blowup, cs, C.byref(h)))
    else:
        L.check(L.lib().zk_fri_commit_grouped(coeffs._h, log_blowup, cs, log_group, C.byref(h)))
    return FriCommitment(coeffs.field, len(coeffs).bit_length() - 1, log_blowup, coset, h)


class FriOpening:
    """ys (k, limbs); proof: the FriProof of the quotient; opened_values (Q, 2, k, limbs); opened_paths (Q 2 k L 32,) bytes"""

    def __init__(self, field, k, d, log_blowup, log_final, nqueries, coset=None):
        self.field, self.k = field, k
        self.proof = FriProof(field, d, log_blowup, log_final, nqueries, coset)
        n = limbs(field)
        self.ys = np.zeros((k, n), np.uint64)
        self.opened_values = np.zeros((nqueries, 2, k, n), np.uint64)
        self.opened_paths = np.zeros(nqueries * 2 * k * (d + log_blowup) * 32, np.uint8)


def _handles(commitments):
    arr = (C.c_void_p * len(commitments))(*[c._h for c in commitments])
    return arr


def quotient(commitments, z, ys, gamma):
    """the DEEP quotient codeword (sum_j gamma^j (f_j[i] - ys[j])) / (c w^i - z): a new table of N entries"""
    c0 = commitments[0]
    h = C.c_void_p()
    ys = np.ascontiguousarray(ys, np.uint64)
    L.check(L.lib().zk_fri_pcs_quotient(_handles(commitments), len(commitments), L.p64(_elem(c0.field, z)), L.p64(ys),
                                        L.p64(_elem(c0.field, gamma)), C.byref(h)))
    return MultilinearPolynomial(c0.field, _handle=h)


def open_at(commitments, z, log_final, nqueries, transcript=None):
    """one proof that f_j(z) = ys[j] for every commitment (same field, size, blow-up and coset); z outside the evaluation domain"""
    c0 = commitments[0]
    op = FriOpening(c0.field, len(commitments), c0.d, c0.log_blowup, log_final, nqueries, c0.coset)
    pr = op.proof
    L.check(L.lib().zk_fri_pcs_open(_handles(commitments), len(commitments), L.p64(_elem(c0.field, z)), log_final, nqueries, _handle(transcript),
                                    L.p64(op.ys), L.p8(pr.roots), L.p64(pr.final_coeffs), L.p64(pr.betas), L.p64(pr.query_indices),
                                    L.p64(pr.query_values), L.p8(pr.query_paths), L.p64(op.opened_values), L.p8(op.opened_paths)))
    return op


def verify_opening(field, roots, z, opening, d, log_blowup, log_final, nqueries, coset=None, transcript=None):
    """host only: `roots` = the k commitment roots (32 bytes each) in the prover's order"""
    ok = C.c_int(0)
    pr = opening.proof
    rf = np.frombuffer(b"".join(bytes(r) for r in roots), np.uint8).copy()
    arrs = [np.ascontiguousarray(a, t) for a, t in ((opening.ys, np.uint64), (pr.roots, np.uint8), (pr.final_coeffs, np.uint64),
                                                    (pr.query_values, np.uint64), (pr.query_paths, np.uint8),
                                                    (opening.opened_values, np.uint64), (opening.opened_paths, np.uint8))]
    ys, fr, fin, vals, paths, ov, opaths = arrs
    cs = None if coset is None else L.p64(_elem(field, coset))
    L.check(L.lib().zk_fri_pcs_verify(field, len(roots), L.p8(rf), d, log_blowup, log_final, nqueries, cs, L.p64(_elem(field, z)), L.p64(ys),
                                      _handle(transcript), L.p8(fr), L.p64(fin), L.p64(vals), L.p8(paths), L.p64(ov), L.p8(opaths), C.byref(ok)))
    return bool(ok.value)


def pcs_last_stats():
    """milliseconds of the calling thread's last open_at: the evaluations, the quotient, the FRI proof, the opening gather"""
    st = _PcsStats()
    L.check(L.lib().zk_fri_pcs_last_stats(C.byref(st)))
    return {name: getattr(st, name) for name, _ in _PcsStats._fields_}


# ---- the multilinear opening ------------------------------------------------------------------------------------------------------------
class _MlStats(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("queries", C.c_uint32), ("ms_sumcheck", C.c_float), ("ms_folds", C.c_float), ("ms_trees", C.c_float),
                ("ms_queries", C.c_float), ("ms_total", C.c_float)]


def ml_sizes(d, log_blowup, log_final, nqueries, log_arity=1, grouped=False, k=None):
    """-> sizes(..) + (nround,): the 3 R elements of round polynomials of a multilinear opening of a table of 2^d entries; log_arity = 2: the
    counts of the opening folded by 4 (nroots = ceil(R / 2), four values and paths per fold-4 step); grouped (log_arity = 2 only): one path
    of L - l - log_sides digests per step; k: the counts of k commitments opened together (open_multilinear_batch)"""
    out = [C.c_size_t(0) for _ in range(5)]
    if grouped and log_arity != 2:
        raise ValueError("grouped leaves need log_arity=2")
    L.check(L.lib().zk_fri_ml_sizes_batch(1 if k is None else k, d, log_blowup, log_final, nqueries, log_arity, 2 if grouped else 0,
                                          *[C.byref(o) for o in out]))      # at k = 1 the single-table counts
    return tuple(int(o.value) for o in out)


def ml_fold(codeword, r, coset=None):
    """one Lagrange-form fold of a codeword on {coset w_len^k}: (1 - r) f_even + r f_odd on the squared domain, a new table of half the length"""
    h = C.c_void_p()
    cs = None if coset is None else L.p64(_elem(codeword.field, coset))
    L.check(L.lib().zk_fri_ml_fold(codeword._h, L.p64(_elem(codeword.field, r)), cs, C.byref(h)))
    return MultilinearPolynomial(codeword.field, _handle=h)


def ml_fold4(codeword, r0, r1, coset=None):
    """two Lagrange-form folds in one pass: ml_fold(ml_fold(codeword, r0, coset), r1, coset^2) byte for byte, a new table of a quarter the length"""
    h = C.c_void_p()
    cs = None if coset is None else L.p64(_elem(codeword.field, coset))
    L.check(L.lib().zk_fri_ml_fold4(codeword._h, L.p64(_elem(codeword.field, r0)), L.p64(_elem(codeword.field, r1)), cs, C.byref(h)))
    return MultilinearPolynomial(codeword.field, _handle=h)


class FriMlOpening:
    """y (limbs,); round_polys (R, 3, limbs); roots (R, 32) bytes, roots[0] = the commitment's; final_table (m, limbs); query_values
    (Q, R, 2, limbs); query_paths (path_bytes,) bytes; challenges (R, limbs) and query_indices (Q,) are what the prover's transcript gave
    (diagnostic: the verifier derives its own)."""

    def __init__(self, field, d, log_blowup, log_final, nqueries, coset=None, log_arity=1, grouped=False):
        self.field, self.d, self.log_blowup, self.log_final, self.nqueries = field, d, log_blowup, log_final, nqueries
        self.coset = None if coset is None else _elem(field, coset).copy()
        nroots, nfinal, nvalues, path_bytes, nround = ml_sizes(d, log_blowup, log_final, nqueries, log_arity, grouped)
        n = limbs(field)
        self.y = np.zeros(n, np.uint64)
        self.round_polys = np.zeros((nround // 3, 3, n), np.uint64)
        self.roots = np.zeros((nroots, 32), np.uint8)
        self.final_table = np.zeros((nfinal, n), np.uint64)
        self.challenges = np.zeros((nround // 3, n), np.uint64)
        self.query_indices = np.zeros(nqueries, np.uint64)
        # log_arity = 2: per query the steps' values one after the other, four per fold-4 step and two for a final fold-2 step
        self.query_values = np.zeros((nqueries, nroots, 2, n) if log_arity == 1 else (nqueries, nvalues // nqueries, n), np.uint64)
        self.query_paths = np.zeros(path_bytes, np.uint8)

    def _coset(self):
        return None if self.coset is None else L.p64(self.coset)


def _point(field, z):
    z = np.ascontiguousarray(z, np.uint64)
    if z.ndim != 2 or z.shape[1] != limbs(field):
        raise L.ZkError(L.ZK_E_ARG, "the point is a (d, limbs) array of elements")
    return z


def open_multilinear(commitment, z, log_final, nqueries, transcript=None):
    """the proof that the committed table, read as evaluations over the cube, has the multilinear extension value `.y` at z (d elements, variable 0
    the most significant index bit, as MultilinearPolynomial.evaluate)"""
    z = _point(commitment.field, z)
    if z.shape[0] != commitment.d:
        raise L.ZkError(L.ZK_E_ARG, "the point needs one element per variable")
    op = FriMlOpening(commitment.field, commitment.d, commitment.log_blowup, log_final, nqueries, commitment.coset)
    L.check(L.lib().zk_fri_ml_open(commitment._h, L.p64(z), log_final, nqueries, _handle(transcript), L.p64(op.y), L.p64(op.round_polys), L.p8(op.roots),
                                   L.p64(op.final_table), L.p64(op.challenges), L.p64(op.query_indices), L.p64(op.query_values), L.p8(op.query_paths)))
    return op


def _points(field, d, points):
    pts = np.ascontiguousarray(points, np.uint64)
    if pts.ndim != 3 or pts.shape[1] != d or pts.shape[2] != limbs(field):
        raise L.ZkError(L.ZK_E_ARG, "the points are a (P, d, limbs) array of elements")
    return pts


def _verifier_inputs(op, roots, claims, points=None, k=None, arity=None):
    """what the verifiers of the multilinear openings marshal alike -> (the roots' bytes, the points, the claims, the proof's arrays in the C
    ABI's order), checked: 32 bytes per root (k: as many roots as a batch has commitments), the points' shape, one claim per point (and
    commitment), and with arity = (log_arity, grouped) that the arrays hold the proof of that arity, whose counts may not be the opening's own"""
    rf = np.frombuffer(b"".join(bytes(r) for r in roots), np.uint8).copy()
    if rf.shape[0] != 32 * len(roots) or len(roots) != (1 if k is None else k):
        raise L.ZkError(L.ZK_E_ARG, "a Merkle root is 32 bytes" if k is None else "one 32-byte Merkle root per commitment")
    pts = None if points is None else _points(op.field, op.d, points)
    ys, rp, fin, vals = (np.ascontiguousarray(a, np.uint64) for a in (claims, op.round_polys, op.final_table, op.query_values))
    if pts is not None and ys.shape != (() if k is None else (k,)) + (pts.shape[0], limbs(op.field)):
        raise L.ZkError(L.ZK_E_ARG, "one claim per point" if k is None else "one claim per commitment and point")
    rts, paths = np.ascontiguousarray(op.roots, np.uint8), np.ascontiguousarray(op.query_paths, np.uint8)
    if arity is not None:
        nroots, nfinal, nvalues, path_bytes, nround = ml_sizes(op.d, op.log_blowup, op.log_final, op.nqueries, *arity)
        n = limbs(op.field)
        if rts.size < 32 * nroots or fin.size < nfinal * n or vals.size < nvalues * n or paths.size < path_bytes or rp.size < nround * n:
            raise L.ZkError(L.ZK_E_ARG, "the opening's arrays are shorter than this arity's proof")
    return L.p8(rf), pts, ys, (L.p64(rp), L.p8(rts), L.p64(fin), L.p64(vals), L.p8(paths))


def _prover_outputs(op):
    """the outputs of a several-point prover in the C ABI's order"""
    return (L.p64(op.ys), L.p64(op.gamma), L.p64(op.round_polys), L.p8(op.roots), L.p64(op.final_table), L.p64(op.challenges),
            L.p64(op.query_indices), L.p64(op.query_values), L.p8(op.query_paths))


def verify_multilinear(root, z, opening, transcript=None):
    """host only: `root` = the commitment's 32 bytes; the claim checked is evaluate(table, z) = opening.y"""
    op, ok = opening, C.c_int(0)
    rf, _, y, proof = _verifier_inputs(op, [root], op.y)
    z = _point(op.field, z)
    if z.shape[0] != op.d:
        raise L.ZkError(L.ZK_E_ARG, "the point needs one element per variable")
    L.check(L.lib().zk_fri_ml_verify(op.field, rf, op.d, op.log_blowup, op.log_final, op.nqueries, op._coset(), L.p64(z), L.p64(y), _handle(transcript),
                                     *proof, C.byref(ok)))
    return bool(ok.value)


# ---- the multilinear opening at several points ------------------------------------------------------------------------------------------
class FriMlPointsOpening(FriMlOpening):
    """FriMlOpening with ys (P, limbs) in place of y, and gamma (limbs,), the batching challenge the prover's transcript gave (diagnostic).
    log_arity = 2: roots (ceil(R / 2), 32), query_values (Q, 4 floor(R / 2) + 2 (R mod 2), limbs).  grouped: the opening of a commitment with
    grouped leaves, one path per step."""

    def __init__(self, field, npoints, d, log_blowup, log_final, nqueries, coset=None, log_arity=1, grouped=False):
        super().__init__(field, d, log_blowup, log_final, nqueries, coset, log_arity, grouped)
        del self.y
        self.npoints, self.log_arity, self.grouped = npoints, log_arity, grouped
        self.ys = np.zeros((npoints, limbs(field)), np.uint64)
        self.gamma = np.zeros(limbs(field), np.uint64)


def ml_round(T, W, r=None):
    """one round pass of the several-point opening on its own.  r = None: -> g3 (3, limbs) = g(0), g(1), g(2) of (T, W), nothing folded.
    Otherwise -> (T', W', g3): both tables folded by r in their last variable, g3 of the folded pair."""
    g3 = np.zeros((3, limbs(T.field)), np.uint64)
    if r is None:
        L.check(L.lib().zk_fri_ml_round(T._h, W._h, None, None, None, L.p64(g3)))
        return g3
    to, wo = C.c_void_p(), C.c_void_p()
    L.check(L.lib().zk_fri_ml_round(T._h, W._h, L.p64(_elem(T.field, r)), C.byref(to), C.byref(wo), L.p64(g3)))
    return MultilinearPolynomial(T.field, _handle=to), MultilinearPolynomial(T.field, _handle=wo), g3


def open_multilinear_points(commitment, points, log_final, nqueries, transcript=None, log_arity=1):
    """one proof that the committed table's multilinear extension has the values `.ys` at the P <= 8 points (P, d, limbs); log_arity = 2 folds
    by 4 and commits every second layer.  A commitment with grouped leaves (commit(.., log_group=2)) takes the grouped protocol, which
    exists for log_arity = 2 only"""
    grouped = getattr(commitment, "log_group", 0) != 0
    if grouped and log_arity != 2:
        raise ValueError("a commitment with grouped leaves is opened with log_arity=2")
    pts = _points(commitment.field, commitment.d, points)
    op = FriMlPointsOpening(commitment.field, pts.shape[0], commitment.d, commitment.log_blowup, log_final, nqueries, commitment.coset, log_arity, grouped)
    first = (commitment._h, L.p64(pts), pts.shape[0], log_final, nqueries)
    if grouped:
        L.check(L.lib().zk_fri_ml_open_points_grouped(*first, _handle(transcript), *_prover_outputs(op)))
    elif log_arity == 1:
        L.check(L.lib().zk_fri_ml_open_points(*first, _handle(transcript), *_prover_outputs(op)))
    else:
        L.check(L.lib().zk_fri_ml_open_points_arity(*first, log_arity, _handle(transcript), *_prover_outputs(op)))
    return op


def verify_multilinear_points(root, points, opening, transcript=None, log_arity=None):
    """host only: `root` = the commitment's 32 bytes; the claims checked are evaluate(table, points[p]) = opening.ys[p].  log_arity: the
    opening's own unless given; an opening with `.grouped` set is checked by the grouped protocol's verifier"""
    op, ok = opening, C.c_int(0)
    log_arity = getattr(op, "log_arity", 1) if log_arity is None else log_arity
    grouped = bool(getattr(op, "grouped", False))
    if grouped and log_arity != 2:
        raise ValueError("an opening with grouped leaves has log_arity=2")
    rf, pts, ys, proof = _verifier_inputs(op, [root], op.ys, points, arity=None if log_arity == 1 else (log_arity, grouped))
    first = (op.field, rf, op.d, op.log_blowup, op.log_final, op.nqueries)
    rest = (op._coset(), L.p64(pts), pts.shape[0], L.p64(ys), _handle(transcript), *proof, C.byref(ok))
    if grouped:
        L.check(L.lib().zk_fri_ml_verify_points_grouped(*first, *rest))
    elif log_arity == 1:
        L.check(L.lib().zk_fri_ml_verify_points(*first, *rest))
    else:
        L.check(L.lib().zk_fri_ml_verify_points_arity(*first, log_arity, *rest))
    return bool(ok.value)


# ---- several commitments opened together --------------------------------------------------------------------------------------------------
def ml_fold_batch(codewords, coeffs, r0, r1=None, coset=None):
    """the first step's fold of k codewords opened together: ml_fold4(sum_j coeffs[j] codewords[j], r0, r1, coset) -- r1 = None:
    ml_fold(.., r0, coset) -- byte for byte, in one pass that never stores the sum.  coeffs: (k, limbs)"""
    field = codewords[0].field
    h = C.c_void_p()
    cf = np.ascontiguousarray(coeffs, np.uint64)
    if cf.shape != (len(codewords), limbs(field)):
        raise L.ZkError(L.ZK_E_ARG, "one coefficient per codeword")
    hs = (C.c_void_p * len(codewords))(*[c._h for c in codewords])
    cs = None if coset is None else L.p64(_elem(field, coset))
    p1 = None if r1 is None else L.p64(_elem(field, r1))
    L.check(L.lib().zk_fri_ml_fold_batch(hs, len(codewords), L.p64(cf), L.p64(_elem(field, r0)), p1, cs, C.byref(h)))
    return MultilinearPolynomial(field, _handle=h)


class FriMlBatchOpening(FriMlPointsOpening):
    """The opening of k commitments at the same P points: ys (k, P, limbs) table-major; roots (k + nroots - 1, 32), the k commitments' first;
    query_values (Q, per, limbs) and query_paths with step 0's answers once per commitment, j-major, in front of the later steps'."""

    def __init__(self, field, k, npoints, d, log_blowup, log_final, nqueries, coset=None, log_arity=1, grouped=False, grinding_bits=0):
        super().__init__(field, npoints, d, log_blowup, log_final, nqueries, coset, log_arity, grouped)
        self.k = k
        self.grinding_bits, self.pow_nonce = grinding_bits, 0      # the proof-of-work step in front of the indices, and its nonce
        nroots, _, nvalues, path_bytes, _ = ml_sizes(d, log_blowup, log_final, nqueries, log_arity, grouped, k=k)
        n = limbs(field)
        self.ys = np.zeros((k, npoints, n), np.uint64)
        self.roots = np.zeros((nroots, 32), np.uint8)
        self.query_values = np.zeros((nqueries, nvalues // nqueries, n), np.uint64)
        self.query_paths = np.zeros(path_bytes, np.uint8)


def open_multilinear_batch(commitments, points, log_final, nqueries, log_arity=1, transcript=None, grinding_bits=0):
    """one proof that each of the k <= 16 committed tables has the values `.ys[j]` at the same P <= 8 points (P, d, limbs).  The commitments
    share field, size, blow-up, coset and leaf grouping; grouped ones (commit(.., log_group=2)) need log_arity=2.  grinding_bits = g > 0: a
    proof-of-work nonce with g leading zero bits is found on the GPU before the indices are drawn; the opening carries g and it"""
    c0 = commitments[0]
    grouped = getattr(c0, "log_group", 0) != 0
    if grouped and log_arity != 2:
        raise ValueError("commitments with grouped leaves are opened with log_arity=2")
    pts = _points(c0.field, c0.d, points)
    op = FriMlBatchOpening(c0.field, len(commitments), pts.shape[0], c0.d, c0.log_blowup, log_final, nqueries, c0.coset, log_arity, grouped,
                           grinding_bits)
    nonce = C.c_uint64(0)
    L.check(L.lib().zk_fri_ml_open_batch_pow(_handles(commitments), len(commitments), L.p64(pts), pts.shape[0], log_final, nqueries, log_arity,
                                             _handle(transcript), *_prover_outputs(op), grinding_bits, C.byref(nonce)))
    op.pow_nonce = int(nonce.value)
    return op


def verify_multilinear_batch(roots, points, opening, transcript=None):
    """host only: `roots` = the k commitment roots (32 bytes each) in the prover's order; the claims checked are
    evaluate(table_j, points[p]) = opening.ys[j, p]"""
    op, ok = opening, C.c_int(0)
    rf, pts, ys, proof = _verifier_inputs(op, roots, op.ys, points, k=op.k)
    L.check(L.lib().zk_fri_ml_verify_batch_pow(op.field, rf, op.k, op.d, op.log_blowup, op.log_final, op.nqueries, op.log_arity, 2 if op.grouped else 0,
                                               op._coset(), L.p64(pts), pts.shape[0], L.p64(ys), _handle(transcript), *proof,
                                               getattr(op, "grinding_bits", 0), getattr(op, "pow_nonce", 0), C.byref(ok)))
    return bool(ok.value)


# ---- the opening against a weight table ---------------------------------------------------------------------------------------------------
class FriMlWeightedOpening(FriMlOpening):
    """The opening of sum_x T[x] W[x] = c against a caller's weight table: FriMlOpening with c (limbs,) in place of y; challenges (R, limbs) are
    part of the proof here (the verifier compares them with its own); query_values (Q, per, limbs); grinding_bits and pow_nonce as a batch's."""

    def __init__(self, field, d, log_blowup, log_final, nqueries, coset=None, log_arity=1, grouped=False, grinding_bits=0):
        super().__init__(field, d, log_blowup, log_final, nqueries, coset, log_arity, grouped)
        del self.y
        self.log_arity, self.grouped, self.grinding_bits, self.pow_nonce = log_arity, grouped, grinding_bits, 0
        self.c = np.zeros(limbs(field), np.uint64)
        self.query_values = self.query_values.reshape(nqueries, -1, limbs(field))


def ml_sizes_weighted(d, log_blowup, log_final, nqueries, log_arity=1, grouped=False):
    """-> (nroots, nfinal, nvalues, path_bytes, nround) of an opening against a weight table: ml_sizes' counts of one table"""
    out = [C.c_size_t(0) for _ in range(5)]
    L.check(L.lib().zk_fri_ml_sizes_weighted(d, log_blowup, log_final, nqueries, log_arity, 2 if grouped else 0, *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def open_weighted(commitment, weights, log_final, nqueries, log_arity=1, transcript=None, grinding_bits=0):
    """the proof that the committed table T and the device table `weights` (2^d entries, not modified) have the inner product `.c`.  The weight
    table does NOT enter the transcript: the caller has bound it (or what it is computed from) to `transcript` already.  A commitment with
    grouped leaves needs log_arity=2."""
    grouped = getattr(commitment, "log_group", 0) != 0
    if grouped and log_arity != 2:
        raise ValueError("a commitment with grouped leaves is opened with log_arity=2")
    op = FriMlWeightedOpening(commitment.field, commitment.d, commitment.log_blowup, log_final, nqueries, commitment.coset, log_arity, grouped, grinding_bits)
    nonce = C.c_uint64(0)
    L.check(L.lib().zk_fri_ml_open_weighted(commitment._h, weights._h, log_final, nqueries, log_arity, grinding_bits, _handle(transcript), L.p64(op.c),
                                            L.p64(op.round_polys), L.p8(op.roots), L.p64(op.final_table), L.p64(op.challenges), L.p64(op.query_indices),
                                            L.p64(op.query_values), L.p8(op.query_paths), C.byref(nonce)))
    op.pow_nonce = int(nonce.value)
    return op


def verify_weighted(root, w_final, opening, transcript=None):
    """host only: `root` = the commitment's 32 bytes; w_final (2^log_final, limbs) = the caller's weight table folded over its last variable by
    opening.challenges, one after the other.  The verifier refuses an opening whose carried challenges are not the transcript's."""
    op, ok = opening, C.c_int(0)
    rf, _, c, proof = _verifier_inputs(op, [root], op.c)
    wf, ch = np.ascontiguousarray(w_final, np.uint64), np.ascontiguousarray(op.challenges, np.uint64)
    if wf.shape != (1 << op.log_final, limbs(op.field)) or ch.shape != (op.d - op.log_final, limbs(op.field)):
        raise L.ZkError(L.ZK_E_ARG, "w_final has 2^log_final elements and the opening one challenge per round")
    L.check(L.lib().zk_fri_ml_verify_weighted(op.field, rf, op.d, op.log_blowup, op.log_final, op.nqueries, op.log_arity, 2 if op.grouped else 0, op._coset(),
                                              L.p64(c), L.p64(ch), L.p64(wf), _handle(transcript), *proof, op.grinding_bits, op.pow_nonce, C.byref(ok)))
    return bool(ok.value)


# ---- several commitments opened together, wide: up to 32 ----------------------------------------------------------------------------------
# The narrow functions above keep their cap of 16.  These are the same protocol byte for byte, for k <= 32.
def ml_sizes_wide(d, log_blowup, log_final, nqueries, log_arity=1, grouped=False, k=1):
    """ml_sizes(.., k=k) for k <= 32"""
    out = [C.c_size_t(0) for _ in range(5)]
    if grouped and log_arity != 2:
        raise ValueError("grouped leaves need log_arity=2")
    L.check(L.lib().zk_fri_ml_sizes_batch_wide(k, d, log_blowup, log_final, nqueries, log_arity, 2 if grouped else 0, *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def ml_fold_batch_wide(codewords, coeffs, r0, r1=None, coset=None):
    """ml_fold_batch for k <= 32 codewords"""
    field = codewords[0].field
    h = C.c_void_p()
    cf = np.ascontiguousarray(coeffs, np.uint64)
    if cf.shape != (len(codewords), limbs(field)):
        raise L.ZkError(L.ZK_E_ARG, "one coefficient per codeword")
    hs = (C.c_void_p * len(codewords))(*[c._h for c in codewords])
    cs = None if coset is None else L.p64(_elem(field, coset))
    p1 = None if r1 is None else L.p64(_elem(field, r1))
    L.check(L.lib().zk_fri_ml_fold_batch_wide(hs, len(codewords), L.p64(cf), L.p64(_elem(field, r0)), p1, cs, C.byref(h)))
    return MultilinearPolynomial(field, _handle=h)


class FriMlWideOpening(FriMlBatchOpening):
    """FriMlBatchOpening for k <= 32: the same arrays, sized by ml_sizes_wide"""

    def __init__(self, field, k, npoints, d, log_blowup, log_final, nqueries, coset=None, log_arity=1, grouped=False, grinding_bits=0):
        FriMlPointsOpening.__init__(self, field, npoints, d, log_blowup, log_final, nqueries, coset, log_arity, grouped)
        self.k = k
        self.grinding_bits, self.pow_nonce = grinding_bits, 0
        nroots, _, nvalues, path_bytes, _ = ml_sizes_wide(d, log_blowup, log_final, nqueries, log_arity, grouped, k=k)
        n = limbs(field)
        self.ys = np.zeros((k, npoints, n), np.uint64)
        self.roots = np.zeros((nroots, 32), np.uint8)
        self.query_values = np.zeros((nqueries, nvalues // nqueries, n), np.uint64)
        self.query_paths = np.zeros(path_bytes, np.uint8)


def open_multilinear_batch_wide(commitments, points, log_final, nqueries, log_arity=1, transcript=None, grinding_bits=0):
    """open_multilinear_batch for k <= 32 commitments: the same proof bytes for k <= 16"""
    c0 = commitments[0]
    grouped = getattr(c0, "log_group", 0) != 0
    if grouped and log_arity != 2:
        raise ValueError("commitments with grouped leaves are opened with log_arity=2")
    if not 1 <= len(commitments) <= 32:
        raise L.ZkError(L.ZK_E_ARG, "1 to 32 commitments")
    pts = _points(c0.field, c0.d, points)
    op = FriMlWideOpening(c0.field, len(commitments), pts.shape[0], c0.d, c0.log_blowup, log_final, nqueries, c0.coset, log_arity, grouped, grinding_bits)
    nonce = C.c_uint64(0)
    L.check(L.lib().zk_fri_ml_open_batch_wide_pow(_handles(commitments), len(commitments), L.p64(pts), pts.shape[0], log_final, nqueries, log_arity,
                                                  _handle(transcript), *_prover_outputs(op), grinding_bits, C.byref(nonce)))
    op.pow_nonce = int(nonce.value)
    return op


def verify_multilinear_batch_wide(roots, points, opening, transcript=None):
    """host only: verify_multilinear_batch for k <= 32"""
    op, ok = opening, C.c_int(0)
    rf, pts, ys, proof = _verifier_inputs(op, roots, op.ys, points, k=op.k)
    L.check(L.lib().zk_fri_ml_verify_batch_wide_pow(op.field, rf, op.k, op.d, op.log_blowup, op.log_final, op.nqueries, op.log_arity,
                                                    2 if op.grouped else 0, op._coset(), L.p64(pts), pts.shape[0], L.p64(ys), _handle(transcript), *proof,
                                                    getattr(op, "grinding_bits", 0), getattr(op, "pow_nonce", 0), C.byref(ok)))
    return bool(ok.value)


def ml_last_stats():
    """milliseconds of the calling thread's last open_multilinear / open_multilinear_points: the sumcheck's passes, the codeword folds, the trees, the query gather"""
    st = _MlStats()
    L.check(L.lib().zk_fri_ml_last_stats(C.byref(st)))
    return {name: getattr(st, name) for name, _ in _MlStats._fields_}


# ---- column commitments: several tables under one tree, opened together --------------------------------------------------------------------
class _ColumnsStats(C.Structure):
    _fields_ = [("columns", C.c_uint32), ("ms_extend", C.c_float), ("ms_leaves", C.c_float), ("ms_nodes", C.c_float), ("ms_total", C.c_float)]


class FriColumns:
    """The prover's side of a commitment to k tables under ONE Merkle tree (include/zkmle.h "Column commitments opened together"): device
    copies of the tables, their codewords and every level of the one tree.  `root` is all a verifier needs.  Use as a context manager, or
    call free()."""

    def __init__(self, field, d, log_blowup, coset, handle):
        self.field, self.d, self.log_blowup, self._h = field, d, log_blowup, handle
        self.k = int(L.lib().zk_fri_columns_count(handle))
        self.coset = None if coset is None else _elem(field, coset).copy()
        root = np.zeros(32, np.uint8)
        L.check(L.lib().zk_fri_columns_root(handle, L.p8(root)))
        self.root = root.tobytes()

    def _copy(self, fn, j):
        h, out = C.c_void_p(), C.c_void_p()
        L.check(fn(self._h, j, C.byref(h)))
        L.check(L.lib().zk_table_clone(h, C.byref(out)))
        return MultilinearPolynomial(self.field, _handle=out)

    def codeword(self, j):
        """a copy of column j's N evaluations f_j(c w^i) as a table of its own"""
        return self._copy(L.lib().zk_fri_columns_codeword, j)

    def table(self, j):
        """a copy of column j's committed table"""
        return self._copy(L.lib().zk_fri_columns_table, j)

    def free(self):
        if self._h is not None:
            L.lib().zk_fri_columns_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:      # noqa: BLE001  (interpreter shutdown)
            pass


def commit_columns(tables, log_blowup, coset=None):
    """ONE commitment to the k <= 32 tables (one field, 2^d entries each): leaf j of its tree holds the first fold's coset of every column, so
    one path answers all of them.  k = 1 has the root of commit(.., log_group=2)"""
    if not 1 <= len(tables) <= 32:
        raise L.ZkError(L.ZK_E_ARG, "1 to 32 tables")
    t0, h = tables[0], C.c_void_p()
    cs = None if coset is None else L.p64(_elem(t0.field, coset))
    L.check(L.lib().zk_fri_commit_columns((C.c_void_p * len(tables))(*[t._h for t in tables]), len(tables), log_blowup, cs, C.byref(h)))
    return FriColumns(t0.field, len(t0).bit_length() - 1, log_blowup, coset, h)


def columns_last_stats():
    """milliseconds of the calling thread's last commit_columns: the k transforms, the leaf launch, the node launches"""
    st = _ColumnsStats()
    L.check(L.lib().zk_fri_columns_last_stats(C.byref(st)))
    return {name: getattr(st, name) for name, _ in _ColumnsStats._fields_}


def _widths(widths):
    return (C.c_uint32 * len(widths))(*[int(w) for w in widths])


def columns_sizes(widths, d, log_blowup, log_final, nqueries):
    """(nroots, nfinal, nvalues, path_bytes, nround) of an opening of column commitments of these widths"""
    out = [C.c_size_t(0) for _ in range(5)]
    L.check(L.lib().zk_fri_ml_sizes_columns(_widths(widths), len(widths), d, log_blowup, log_final, nqueries, *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


class FriColumnsOpening(FriMlPointsOpening):
    """The opening of m column commitments of `widths` (K columns together) at the same P points: ys (K, P, limbs) in global column order;
    roots (m + nroots - 1, 32), the m commitments' first; query_values (Q, per, limbs) with step 0's 4 K values column-major in front of the
    later steps'; query_paths with step 0's m paths in front of the later steps'."""

    def __init__(self, field, widths, npoints, d, log_blowup, log_final, nqueries, coset=None, grinding_bits=0):
        super().__init__(field, npoints, d, log_blowup, log_final, nqueries, coset, 2, True)
        self.widths, self.k = [int(w) for w in widths], int(sum(widths))
        self.grinding_bits, self.pow_nonce = grinding_bits, 0
        nroots, _, nvalues, path_bytes, _ = columns_sizes(widths, d, log_blowup, log_final, nqueries)
        n = limbs(field)
        self.ys = np.zeros((self.k, npoints, n), np.uint64)
        self.roots = np.zeros((nroots, 32), np.uint8)
        self.query_values = np.zeros((nqueries, nvalues // nqueries, n), np.uint64)
        self.query_paths = np.zeros(path_bytes, np.uint8)


def open_columns(commitments, points, log_final, nqueries, transcript=None, grinding_bits=0):
    """one proof that every column of the m column commitments (together at most 32 columns; one field, size, blow-up and coset) has the values
    `.ys[c]` at the same P <= 8 points (P, d, limbs): each query's step 0 carries one path per COMMITMENT"""
    c0 = commitments[0]
    pts = _points(c0.field, c0.d, points)
    op = FriColumnsOpening(c0.field, [c.k for c in commitments], pts.shape[0], c0.d, c0.log_blowup, log_final, nqueries, c0.coset, grinding_bits)
    nonce = C.c_uint64(0)
    L.check(L.lib().zk_fri_ml_open_columns_pow(_handles(commitments), len(commitments), L.p64(pts), pts.shape[0], log_final, nqueries, grinding_bits,
                                               _handle(transcript), *_prover_outputs(op), C.byref(nonce)))
    op.pow_nonce = int(nonce.value)
    return op


def verify_columns(roots, widths, points, opening, transcript=None):
    """host only: `roots` = the m commitment roots (32 bytes each) and `widths` their column counts, in the prover's order; the claims checked
    are evaluate(column_c, points[p]) = opening.ys[c, p]"""
    op, ok = opening, C.c_int(0)
    rf, _, ys, proof = _verifier_inputs(op, roots, op.ys, k=len(widths))      # one 32-byte root per width
    pts = _points(op.field, op.d, points)
    if ys.shape != (int(sum(widths)), pts.shape[0], limbs(op.field)):
        raise L.ZkError(L.ZK_E_ARG, "one claim per column and point")
    L.check(L.lib().zk_fri_ml_verify_columns_pow(op.field, rf, _widths(widths), len(widths), op.d, op.log_blowup, op.log_final, op.nqueries,
                                                 getattr(op, "grinding_bits", 0), op._coset(), L.p64(pts), pts.shape[0], L.p64(ys), _handle(transcript),
                                                 *proof, getattr(op, "pow_nonce", 0), C.byref(ok)))
    return bool(ok.value)
