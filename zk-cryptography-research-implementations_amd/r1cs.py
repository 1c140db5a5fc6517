"""R1CS instances (extension; the protocol and bytes are in include/zkmle.h "R1CS instance: sparse matrices times a table").

  R1CS(field, s, d, A, B, C)   three sparse matrices of 2^s rows and 2^d columns, each a (rows, cols, vals) triple: two integer sequences
                               and a (nnz, limbs) array of Montgomery elements (zk.from_ints), in any order.  .digest, .shape
  matvec(inst, z)              (A z, B z, C z) for a table z of 2^d entries: three new tables of 2^s
  bind_rows(inst, rx, rho)     M[y] = sum_x eq(rx, x) (A + rho B + rho^2 C)[x, y] over the witness columns y < 2^(d-1), or with full=True
                               over all 2^d
  prove(inst, cmW, public, ..) the Spartan proof that (A z) o (B z) = C z for z = (w || 1, public.., 0 ..), w the table cmW commits to -> R1CSProof
  verify(inst, root, public, proof)   host only
  public_terms(inst, public, rx, rho, open_challenges)   host only: (c_pub, w_final) of the verifier
  sizes(..), last_stats()

Creating an instance and reading its digest need no GPU; the two passes run HIP kernels and raise without one."""
import ctypes as C

import numpy as np

from . import _lib as L
from .mle import MultilinearPolynomial, _elem, limbs

ROW_SPLIT = 32      # ZK_R1CS_ROW_SPLIT: rows and columns of more entries go one to a workgroup


class _Stats(C.Structure):
    _fields_ = [("ms_products", C.c_float), ("ms_eq", C.c_float), ("ms_rounds", C.c_float), ("ms_bind", C.c_float), ("ms_opening", C.c_float),
                ("ms_total", C.c_float)]


def last_stats():
    """the calling thread's last prove (products, E_0, rounds, row binding, opening, total); matvec sets ms_products, bind_rows ms_eq and ms_bind"""
    st = _Stats()
    L.check(L.lib().zk_r1cs_last_stats(C.byref(st)))
    return {n: getattr(st, n) for n, _ in _Stats._fields_}


class R1CS:
    def __init__(self, field, log_rows, log_cols, A, B, C_):
        self.field = field
        keep, rp, cp, vp_, nnz = [], [], [], [], []
        for rows, cols, vals in (A, B, C_):
            r = np.ascontiguousarray(rows, np.uint32).reshape(-1)
            c = np.ascontiguousarray(cols, np.uint32).reshape(-1)
            v = np.ascontiguousarray(vals, np.uint64).reshape(-1, limbs(field))
            if not (r.shape[0] == c.shape[0] == v.shape[0]):
                raise L.ZkError(L.ZK_E_ARG, "rows, cols and vals of a matrix have one length")
            keep += [r, c, v]
            rp.append(r.ctypes.data_as(C.POINTER(C.c_uint32)))
            cp.append(c.ctypes.data_as(C.POINTER(C.c_uint32)))
            vp_.append(L.p64(v))
            nnz.append(r.shape[0])
        h = C.c_void_p()
        L.check(L.lib().zk_r1cs_create(field, log_rows, log_cols, (C.POINTER(C.c_uint32) * 3)(*rp), (C.POINTER(C.c_uint32) * 3)(*cp),
                                       (L.u64p * 3)(*vp_), (C.c_size_t * 3)(*nnz), C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                L.lib().zk_r1cs_free(self._h)
            except Exception:
                pass
            self._h = None

    @property
    def digest(self):
        out = np.zeros(32, np.uint8)
        L.check(L.lib().zk_r1cs_digest(self._h, L.p8(out)))
        return out.tobytes()

    @property
    def shape(self):
        """{"field", "log_rows", "log_cols", "nnz": (a, b, c), "block_rows", "block_cols"}: the last two count the rows (of all three matrices)
        and the columns that go one to a workgroup"""
        f, s, d = C.c_int(), C.c_uint32(), C.c_uint32()
        nnz, blk = np.zeros(3, np.uint64), np.zeros(2, np.uint64)
        L.check(L.lib().zk_r1cs_shape(self._h, C.byref(f), C.byref(s), C.byref(d), L.p64(nnz), L.p64(blk)))
        return {"field": f.value, "log_rows": s.value, "log_cols": d.value, "nnz": tuple(int(x) for x in nnz), "block_rows": int(blk[0]),
                "block_cols": int(blk[1])}


def matvec(inst, z):
    out = (C.c_void_p * 3)()
    L.check(L.lib().zk_r1cs_matvec(inst._h, z._h, out))
    return tuple(MultilinearPolynomial(inst.field, _handle=C.c_void_p(h)) for h in out)


def bind_rows(inst, rx, rho, full=False):
    rx = np.ascontiguousarray(rx, np.uint64).reshape(-1, limbs(inst.field))
    if rx.shape[0] != inst.shape["log_rows"]:
        raise L.ZkError(L.ZK_E_ARG, "rx has one element per row variable")
    h = C.c_void_p()
    L.check(L.lib().zk_r1cs_bind_rows(inst._h, L.p64(rx), L.p64(_elem(inst.field, rho)), 1 if full else 0, C.byref(h)))
    return MultilinearPolynomial(inst.field, _handle=h)


def sizes(log_rows, log_cols, log_blowup, log_final, nqueries, log_arity=1, grouped=False):
    """-> (nzc_round, nroots, nfinal, nvalues, path_bytes, nround): 4 s round-polynomial elements, then the weighted opening's counts at d - 1"""
    out = [C.c_size_t(0) for _ in range(6)]
    L.check(L.lib().zk_r1cs_sizes(log_rows, log_cols, log_blowup, log_final, nqueries, log_arity, 2 if grouped else 0, *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


class R1CSProof:
    """round_polys (s, 4, limbs), vs (3, limbs) = va, vb, vc, and `opening`, a fri.FriMlWeightedOpening of the witness (its c is the second
    sumcheck's claim); tau (s, limbs), challenges (s, limbs) and rho are what the prover's transcript gave (diagnostic)"""

    def __init__(self, field, log_rows, opening):
        n = limbs(field)
        self.field, self.log_rows, self.opening = field, log_rows, opening
        self.tau, self.challenges = np.zeros((log_rows, n), np.uint64), np.zeros((log_rows, n), np.uint64)
        self.round_polys = np.zeros((log_rows, 4, n), np.uint64)
        self.vs, self.rho = np.zeros((3, n), np.uint64), np.zeros(n, np.uint64)


def _public(field, public):
    pub = np.ascontiguousarray(public if public is not None and len(public) else np.zeros((0, limbs(field))), np.uint64).reshape(-1, limbs(field))
    return pub, (L.p64(pub) if pub.shape[0] else None)


def prove(inst, commitment, public, log_final, nqueries, log_arity=1, transcript=None, grinding_bits=0):
    from . import fri
    grouped = getattr(commitment, "log_group", 0) != 0
    if grouped and log_arity != 2:
        raise ValueError("a commitment with grouped leaves is opened with log_arity=2")
    pub, pp = _public(inst.field, public)
    op = fri.FriMlWeightedOpening(commitment.field, commitment.d, commitment.log_blowup, log_final, nqueries, commitment.coset, log_arity, grouped, grinding_bits)
    pr = R1CSProof(inst.field, inst.shape["log_rows"], op)
    nonce = C.c_uint64(0)
    L.check(L.lib().zk_r1cs_prove(inst._h, commitment._h, pp, pub.shape[0], log_final, nqueries, log_arity, grinding_bits, fri._handle(transcript), L.p64(pr.tau),
                                  L.p64(pr.round_polys), L.p64(pr.challenges), L.p64(pr.vs), L.p64(pr.rho), L.p64(op.c), L.p64(op.round_polys), L.p8(op.roots),
                                  L.p64(op.final_table), L.p64(op.challenges), L.p64(op.query_indices), L.p64(op.query_values), L.p8(op.query_paths),
                                  C.byref(nonce)))
    op.pow_nonce = int(nonce.value)
    return pr


def verify(inst, root, public, proof, transcript=None):
    """host only: `root` = the witness commitment's 32 bytes"""
    from . import fri
    op, ok = proof.opening, C.c_int(0)
    pub, pp = _public(inst.field, public)
    rf = np.frombuffer(bytes(root), np.uint8).copy()
    if rf.shape[0] != 32:
        raise L.ZkError(L.ZK_E_ARG, "a Merkle root is 32 bytes")
    arrs = [np.ascontiguousarray(a, np.uint64) for a in (proof.round_polys, proof.vs, op.c, op.round_polys, op.final_table, op.challenges, op.query_values)]
    rts, paths = np.ascontiguousarray(op.roots, np.uint8), np.ascontiguousarray(op.query_paths, np.uint8)
    L.check(L.lib().zk_r1cs_verify(inst._h, L.p8(rf), pp, pub.shape[0], op.log_blowup, op.log_final, op.nqueries, op.log_arity, 2 if op.grouped else 0, op._coset(),
                                   fri._handle(transcript), L.p64(arrs[0]), L.p64(arrs[1]), L.p64(arrs[2]), L.p64(arrs[3]), L.p8(rts), L.p64(arrs[4]), L.p64(arrs[5]),
                                   L.p64(arrs[6]), L.p8(paths), op.grinding_bits, op.pow_nonce, C.byref(ok)))
    return bool(ok.value)


def public_terms(inst, public, rx, rho, open_challenges):
    """host only -> (c_pub (limbs,), w_final (2^(d - 1 - R), limbs)) for R = len(open_challenges)"""
    n = limbs(inst.field)
    pub, pp = _public(inst.field, public)
    rx = np.ascontiguousarray(rx, np.uint64).reshape(-1, n)
    ch = np.ascontiguousarray(open_challenges, np.uint64).reshape(-1, n)
    sh = inst.shape
    if rx.shape[0] != sh["log_rows"] or ch.shape[0] > sh["log_cols"] - 1:
        raise L.ZkError(L.ZK_E_ARG, "rx has one element per row variable and the opening at most d - 1 challenges")
    c_pub, wf = np.zeros(n, np.uint64), np.zeros((1 << (sh["log_cols"] - 1 - ch.shape[0]), n), np.uint64)
    L.check(L.lib().zk_r1cs_public_terms(inst._h, pp, pub.shape[0], L.p64(rx), L.p64(_elem(inst.field, rho)), L.p64(ch) if ch.shape[0] else None, ch.shape[0],
                                         L.p64(c_pub), L.p64(wf)))
    return c_pub, wf
