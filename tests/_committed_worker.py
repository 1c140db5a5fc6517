"""Child process of tests/test_gpu_sumcheck_committed.py: the committed basic sumcheck of one 2^logn table under the environment it was
started with (ZK_HOST_TRANSCRIPT, ZK_FOLD_SPLIT2 are read once per process).  Prints one JSON line {"digest": sha256 of root || claimed
sum || round messages || challenges, "verified": bool}."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G                                                          # noqa: E402


def proof_digest(proof, challenges):
    h = hashlib.sha256()
    h.update(bytes(proof.root))
    h.update(proof.initial_claimed_sum.tobytes())
    h.update(proof.round_univariate_polynomials.tobytes())
    h.update(challenges.tobytes())
    return h.hexdigest()


def main():
    field, logn, seed = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    zk = G.import_package()
    from zkmle_amd import _lib
    _lib.check(zk.lib().zk_init(0))
    poly = zk.MultilinearPolynomial.random(field, 1 << logn, seed)
    prover = zk.Prover.init(field, poly)
    proof = prover.prove_committed()
    print(json.dumps({"digest": proof_digest(proof, prover.challenges), "verified": zk.Verifier.init().verify_committed(proof)}))


if __name__ == "__main__":
    main()
