"""What the wrappers of the zerocheck-family provers share (zerocheck.py, wiring.py, plonk.py, lookup.py, plonk_lookup.py): one proof class, one
marshalling of a prover call and of a verifier call, `sizes`, a round pass on its own, `last_stats`.  The C entries differ in their leading
arguments (the commitments, the public inputs) and in a few counts; everything behind those is laid out alike (include/zkmle.h)."""
import ctypes as C

import numpy as np

from . import _lib as L
from . import fri
from .mle import MultilinearPolynomial, _elem, limbs

_COUNT = {2: "two", 3: "three", 5: "five"}


def sizes_of(fn, nout, d, log_blowup, log_final, nqueries, log_arity=None, grouped=False):
    """the `nout` counts of a sizes entry; log_arity None: an entry without a schedule (column commitments)"""
    out = [C.c_size_t(0) for _ in range(nout)]
    if grouped and log_arity != 2:
        raise ValueError("grouped leaves need log_arity=2")
    sched = () if log_arity is None else (log_arity, 2 if grouped else 0)
    L.check(fn(d, log_blowup, log_final, nqueries, *sched, *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def round_pass(fn, tables, scalars, log_step, r, nodes):
    """one round pass on its own: fn(tables, *scalars, [log_step,] r, outs, g).  r = None: -> g (nodes, limbs), nothing folded.  Otherwise ->
    (the tables folded by r in their last variable, g of the folded ones).  log_step None: an entry without one"""
    field, n = tables[0].field, len(tables)
    g = np.zeros((nodes, limbs(field)), np.uint64)
    ins = (C.c_void_p * n)(*[t._h for t in tables])
    lead = [L.p64(_elem(field, v)) for v in scalars] + ([] if log_step is None else [log_step])
    if r is None:
        L.check(fn(ins, *lead, None, None, L.p64(g)))
        return g
    outs = (C.c_void_p * n)()
    L.check(fn(ins, *lead, L.p64(_elem(field, r)), outs, L.p64(g)))
    return tuple(MultilinearPolynomial(field, _handle=C.c_void_p(h)) for h in outs), g


def _public_args(public):
    """public() -> (the public values' array, its pointer) -> (the array, which the caller keeps alive over the call; the C arguments)"""
    if public is None:
        return None, ()
    pub, pp = public()
    return pub, (pp, pub.shape[0])


class Proof:
    """round_polys (d, NODES, limbs), challenges (d, limbs), the opening of the K tables, and with HELPER_ROOTS helper commitments h_roots
    (HELPER_ROOTS, 32) and drawn (DRAWN + d, limbs) = the DRAWN challenges ahead of tau, then tau; without helpers (DRAWN None) tau (d, limbs)"""

    K = NODES = None
    HELPER_ROOTS, DRAWN = 0, None
    OPENING = fri.FriMlBatchOpening

    def __init__(self, field, d, log_blowup, log_final, nqueries, coset=None, log_arity=1, grouped=False, grinding_bits=0):
        self._allocate(field, d, self.OPENING(field, self.K, 1, d, log_blowup, log_final, nqueries, coset, log_arity, grouped, grinding_bits))

    def _allocate(self, field, d, opening):
        n = limbs(field)
        self.field, self.d = field, d
        if self.DRAWN is None:
            self.tau = np.zeros((d, n), np.uint64)
        else:
            self.h_roots = np.zeros((self.HELPER_ROOTS, 32), np.uint8)
            self.drawn = np.zeros((self.DRAWN + d, n), np.uint64)
        self.round_polys = np.zeros((d, self.NODES, n), np.uint64)
        self.challenges = np.zeros((d, n), np.uint64)
        self.opening = opening

    @property
    def ys(self):
        return self.opening.ys[:, 0]

    @property
    def point(self):
        """(1, d, limbs): where the tables are opened"""
        return np.ascontiguousarray(self.challenges[::-1])[None]


def prove_with(cls, call, c0, log_final, nqueries, log_arity, transcript, grinding_bits, public=None):
    """-> the cls that call(*rest) filled: the C prover behind its commitments.  c0: a commitment, for the shape; log_arity None: a prover of
    column commitments, which has no schedule; public() -> (the public values' array, its pointer), which then lead `rest`"""
    sched = ()
    if log_arity is not None:
        grouped = getattr(c0, "log_group", 0) != 0
        if grouped and log_arity != 2:
            raise ValueError("commitments with grouped leaves are opened with log_arity=2")
        sched = (log_arity, grouped)
    pub, pub_args = _public_args(public)
    pr = cls(c0.field, c0.d, c0.log_blowup, log_final, nqueries, c0.coset, *sched, grinding_bits)
    op, nonce = pr.opening, C.c_uint64(0)
    own = (L.p64(pr.tau),) if cls.DRAWN is None else (L.p8(pr.h_roots), L.p64(pr.drawn))
    L.check(call(*pub_args, log_final, nqueries, *sched[:1], grinding_bits, fri._handle(transcript), *own,
                 L.p64(pr.round_polys), L.p64(pr.challenges), *fri._prover_outputs(op), C.byref(nonce)))
    op.pow_nonce = int(nonce.value)
    return pr


def verify_with(fn, proof, own_roots, transcript, public=None):
    """host only: the C verifier `fn` on the proof and the verifier's own roots; public() as for prove_with"""
    op, ok = proof.opening, C.c_int(0)
    columns = isinstance(op, fri.FriColumnsOpening)
    every, helper = list(own_roots), ()
    if proof.DRAWN is not None:
        hr = np.ascontiguousarray(proof.h_roots, np.uint8)
        if hr.shape != (proof.HELPER_ROOTS, 32):
            raise L.ZkError(L.ZK_E_ARG, _COUNT[proof.HELPER_ROOTS] + " 32-byte helper roots")
        # the opening's roots and claims are those of all the commitments; only the first are the verifier's own
        every, helper = every + [hr[j].tobytes() for j in range(proof.HELPER_ROOTS)], (L.p8(hr),)
    pub, pub_args = _public_args(public)
    rf, _, ys, arrays = fri._verifier_inputs(op, every, op.ys, k=len(op.widths) if columns else proof.K)
    rp = np.ascontiguousarray(proof.round_polys, np.uint64)
    if columns:                                              # one pointer per root, and no schedule
        own = np.frombuffer(b"".join(bytes(r) for r in own_roots), np.uint8).copy()
        roots, sched = (L.p8(own[:32]), L.p8(own[32:])), ()
    else:
        roots, sched = (rf,), (op.log_arity, 2 if op.grouped else 0)
    L.check(fn(op.field, *roots, *pub_args, op.d, op.log_blowup, op.log_final, op.nqueries, *sched, op._coset(),
               fri._handle(transcript), *helper, L.p64(rp), L.p64(ys), *arrays, getattr(op, "grinding_bits", 0), getattr(op, "pow_nonce", 0), C.byref(ok)))
    return bool(ok.value)


def stats_of(fn, Stats):
    st = Stats()
    L.check(fn(C.byref(st)))
    return {name: getattr(st, name) for name, _ in Stats._fields_}
