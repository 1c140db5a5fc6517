"""zk-cryptography-research-implementations_amd -- MI355X-native multilinear prover path.

Python host binding (ctypes) of libzkmle_amd.so, mirroring the reference's Rust items for the
path: `MultilinearPolynomial::{new, evaluate, partial_evaluate, ...}`
(polynomials/src/multilinear/evaluation_form.rs).  Tables live in HBM behind `zk_table` handles;
every operation runs hand-written HIP kernels through the C ABI of include/zkmle.h.

There is NO CPU fallback: if the shared library is missing, or no HIP device is usable, the
operations raise.  (The directory name contains '-', so import it with
`__graft_entry__.import_package()`, which registers it as `zkmle_amd`.)
"""
from . import _lib
from ._lib import FR381, FQ381, BN254_FQ, BN254_FR, ZkError, ReferencePanic, lib, library_path  # noqa: F401
from .mle import MultilinearPolynomial, from_ints, to_ints, limbs  # noqa: F401
from . import sumcheck  # noqa: F401
from .sumcheck import Transcript, ProductPolynomial, SumPolynomial, Prover, Verifier  # noqa: F401
from . import merkle  # noqa: F401
from .merkle import MerkleTree, merkle_root  # noqa: F401
from . import ntt  # noqa: F401  (the module, like merkle and kzg: the transform itself is zk.ntt.ntt)
from .ntt import two_adicity, root_of_unity, ntt_inplace, low_degree_extend, poly_mul, evaluate_at  # noqa: F401
from . import fri  # noqa: F401  (the module: zk.fri.prove, zk.fri.verify, ...)
from .fri import FriProof, FriCommitment, FriOpening, FriMlOpening, FriMlWeightedOpening  # noqa: F401
from . import zerocheck  # noqa: F401  (the module: zk.zerocheck.prove_mul, zk.zerocheck.verify_mul, ...)
from . import wiring  # noqa: F401  (the module: zk.wiring.prove, zk.wiring.verify, ...)
from .wiring import WiringProof  # noqa: F401
from . import plonk  # noqa: F401  (the module: zk.plonk.prove, zk.plonk.verify, ...)
from .plonk import PlonkProof  # noqa: F401
from . import lookup  # noqa: F401  (the module: zk.lookup.prove, zk.lookup.verify, ...)
from .lookup import LookupProof  # noqa: F401
from . import plonk_lookup  # noqa: F401  (the module: zk.plonk_lookup.prove, zk.plonk_lookup.verify, ...)
from .plonk_lookup import PlonkLookupProof  # noqa: F401
from .plonk_lookup import PlonkLookupColumnsProof  # noqa: F401
from . import r1cs  # noqa: F401  (the module: zk.r1cs.matvec, zk.r1cs.bind_rows, ...)
from .r1cs import R1CS, R1CSProof  # noqa: F401
from . import gkr  # noqa: F401
from .gkr import Circuit, Gate, Layer, Operator  # noqa: F401
from . import kzg  # noqa: F401
from .kzg import G1Bases, TrustedSetup, MultilinearKZG, MultilinearKZGProof, MultilinearKZGBatchProof  # noqa: F401
from . import sharded  # noqa: F401

__all__ = ["MultilinearPolynomial", "FR381", "FQ381", "BN254_FQ", "BN254_FR", "ZkError", "ReferencePanic",
           "from_ints", "to_ints", "limbs", "lib", "library_path", "MerkleTree", "merkle_root",
           "ntt", "two_adicity", "root_of_unity", "ntt_inplace", "low_degree_extend", "poly_mul", "evaluate_at", "fri", "FriProof",
           "FriCommitment", "FriOpening", "FriMlOpening"]
