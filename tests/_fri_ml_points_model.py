"""Python model of the multilinear opening of a FRI commitment at SEVERAL points (helper of tests/test_fri_ml_points_cpu.py and
test_gpu_fri_ml_points.py).  The definition is the one of include/zkmle.h "FRI commitment opened at several points"; the prover, the verifier
and `flat` are those of tests/_fri_ml_family_model.py under its protocol POINTS:

  claims       y_p = the multilinear extension of T at z^p, p < P
  transcript   FRI's header, root_0, P (4 bytes), the points point-major, y_0 .. y_{P-1}, gamma, (g_l, r_l, root_{l+1})*, T_R, Q indices
  weights      W_0[x] = sum_p gamma^p eq(x, z^p);  W_{l+1} = mle_fold_last(W_l, r_l), as T_{l+1} from T_l
  round l      g_l(X) = sum_x' (W_l[2x'] + X (W_l[2x'+1] - W_l[2x'])) (T_l[2x'] + X (T_l[2x'+1] - T_l[2x'])), sent at X = 0, 1, 2
  verifier     claim_0 = sum_p gamma^p y_p; the sumcheck's checks; sum_j T_R[j] W_R[j] = the last claim with W_R from the points alone; FRI's
               query checks with the Lagrange fold

Everything is Python integers; nothing here knows how the library works.  `open_points(.., false_y=(p, v))` opens with claim p replaced by v:
round 0's polynomial is shifted so that g_0(0) + g_0(1) equals the false claim_0 and everything else is run honestly.

The second half is the transcript SCHEDULE of the succinct sparse GKR proof (zk_gkr_sparse_prove_succinct): oracle/pymodel.py gkr_prove_wide
opens a transcript of its own and cannot start from one that holds the root, so the oracle here is a replay -- every challenge re-derived
from the proof's elements in the order the header pins, root first."""
import functools

import _fri_ml_family_model as FAM
import _fri_ml_model as ML
import _fri_model as FM
import _ntt_model as NM
from oracle import pymodel as M

be32 = FM.be32
weights, round_g3 = FAM.weights, FAM.round_g3
verify = functools.partial(FAM.verify_family, FAM.POINTS)
flat = functools.partial(FAM.flat, FAM.POINTS)              # (tests/_fri_ml_model.py flat with points (P, d, 4), ys (P, 4) and gamma (4,) in place of z and y)


def round_polys(field, table, points, gamma, rs):
    """the round polynomials of the weight-table form on GIVEN challenges rs -> (polys, T_R)"""
    p = NM.MODULUS[field]
    T, W, polys = list(table), weights(points, gamma, p), []
    for r in rs:
        polys.append(round_g3(T, W, p))
        T, W = ML.mle_fold_last(field, T, r), ML.mle_fold_last(field, W, r)
    return polys, T


def open_points(cm, points, f, Q, tr=None, false_y=None, hasher=M.keccak256):
    """-> the opening as a dict; `cm` is a tests/_fri_pcs_model.py commitment, points a list of P lists of d ints; `tr` is advanced"""
    return FAM.open_family(FAM.POINTS, [cm], points, f, Q, tr, hasher, false_y)


# ---- the transcript schedule of the succinct sparse GKR proof ---------------------------------------------------------------------------
def gkr_succinct_replay(p, root, circuit_output, out_bits0, layer_claims, layer_coeffs, wb, wc):
    """Every challenge of zk_gkr_sparse_prove_succinct's GKR part, re-derived from the proof's integers: the commitment's root is absorbed FIRST,
    then gkr_protocol.rs' appends unchanged (oracle/pymodel.py gkr_prove_wide's order): the output layer's bytes, out_bits0 output challenges,
    per layer its claim and its rounds' little-endian coefficients with a challenge after each, and between layers wb, alpha, wc, beta.
    layer_coeffs[l]: the layer's round polynomials (coefficient lists).  -> dict(output_challenges, challenges (per layer), alpha, beta)"""
    t = M.Transcript()
    t.append(root)
    t.append(b"".join(be32(v) for v in circuit_output))
    out = {"output_challenges": [t.challenge(p) for _ in range(out_bits0)], "challenges": [], "alpha": [], "beta": []}
    nl = len(layer_coeffs)
    for l in range(nl):
        t.append(be32(layer_claims[l]))
        chal = []
        for co in layer_coeffs[l]:
            t.append(b"".join(M.le32(c) for c in co))
            chal.append(t.challenge(p))
        out["challenges"].append(chal)
        if l + 1 < nl:
            t.append(be32(wb[l]))
            out["alpha"].append(t.challenge(p))
            t.append(be32(wc[l]))
            out["beta"].append(t.challenge(p))
    return out
