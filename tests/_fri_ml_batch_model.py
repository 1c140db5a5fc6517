"""Python model of the multilinear opening of SEVERAL FRI commitments with one proof (helper of tests/test_fri_ml_batch_cpu.py and
test_gpu_fri_ml_batch.py).  The definition is the one of include/zkmle.h "FRI commitments opened together"; the prover, the verifier, `sizes`
and `flat` are those of tests/_fri_ml_family_model.py under its protocols batch(a, grouped):

  schedules    (log_arity 1, ungrouped), (2, ungrouped), (2, grouped): the steps of the single-table protocols
  transcript   FRI's header, "BTCH" a grouped k (16 bytes), the k roots, P, the points, the k P claims table-major, ONE gamma, then the rounds,
               the later roots, T_R and the indices as in the single-table protocol of the schedule
  combination  alpha = gamma^P;  claim_0 = sum_j alpha^j sum_p gamma^p y_{j,p};  T = sum_j alpha^j T_j;  f_0 = sum_j alpha^j f_j
  answers      step 0: per commitment its own values and its own path(s); steps s >= 1 as in the single-table protocol
  roots        the k commitments' first, then the later layers'

Everything is Python integers; nothing here knows how the library works."""
import _fri_ml_family_model as FAM
from oracle import pymodel as M

KMAX = FAM.KMAX
steps = FAM.steps                                            # steps(L, R, a): [(l, sides)] of an opening with R rounds at log_arity a
sizes = FAM.sizes                                            # sizes(k, d, b, f, Q, a=1, grouped=False)


def open_batch(cms, points, f, Q, a=1, tr=None, hasher=M.keccak256):
    """-> the opening as a dict; `cms`: k commitments of tests/_fri_pcs_model.py (ungrouped) or of _fri_ml_grouped_model.py (all grouped), points
    a list of P lists of d ints; `tr` is advanced"""
    return FAM.open_family(FAM.batch(a, cms[0].get("log_group", 0) == 2), cms, points, f, Q, tr, hasher)


def verify(op, tr=None, hasher=M.keccak256):
    return FAM.verify_family(FAM.batch(op["a"], op["grouped"]), op, tr, hasher)


def flat(zk, op):
    """own_roots (k, 32), points (P, d, 4), ys (k, P, 4), gamma (4,), polys (R, 3, 4), roots (k + steps - 1, 32), final (m, 4), challenges
    (R, 4), indices (Q,), values (Q, per, 4), paths (bytes)"""
    return FAM.flat(FAM.batch(op["a"], op["grouped"]), zk, op)
