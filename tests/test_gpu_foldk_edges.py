"""GPU: the weighted-sum fold of K variables (csrc/mle_kernels.cuh foldk_seg_sums_kernel, foldk_seg_sums_split2_kernel,
foldk_split_kernel) at operands where the lazily reduced sum leaves the range its one conditional subtraction finishes.

One raw_mont_reduce + u_reduce_once is in range for any canonical inputs only up to floor(2^261 / p) terms: 70 on BLS12-381 Fr, 169 on
BN254 Fr.  Before the fix the forms below summed 256 or 128 terms per reduction and stored elements at or above p for near-p tables
and challenge tuples whose weights (residues) sum past 2^261; the segment sums stayed congruent, so proofs on random tables never
noticed.  Each case drives the public zk_rounds_multi_* sequence (one rank, as tests/test_gpu_sharded.py), steers the challenges by a
nonce appended to the transcript before zk_rounds_new (tests/golden/foldk_hot_transcripts.json, found on the CPU by
make_foldk_hot_transcripts.py), reads the challenges back with zk_rounds_collect, and compares the downloaded folded table with the
exact integer fold -- byte for byte, every element below p, the input unchanged.  W and the lanes the model puts at or above 2 p are
recomputed from the challenges the library returned and asserted first, so a stale fixture fails instead of passing empty.

Shapes (fold_pass in csrc/zkmle_sumcheck.hip, launch_foldk in csrc/fold_multi.h; kBlock = 256):

  shape        input  K  m_next  output  kernel                                          terms per reduction before -> after (Fr381)
  unsplit_k8   2^14   8  1       2^6     foldk_seg_sums_kernel<8>  (segments of 32 < 128)  256 -> 4 x 64
  unsplit_k7   2^15   7  2       2^8     foldk_seg_sums_kernel<7>  (segments of 64 < 128)  128 -> 2 x 64
  split2_k8    2^17   8  1       2^9     foldk_seg_sums_split2_kernel<8>                   128 -> 2 x 64 per lane
  split2_k7    2^16   7  1       2^9     foldk_seg_sums_split2_kernel<7>  (default path)    64
  split2_k6    2^15   6  1       2^9     foldk_seg_sums_split2_kernel<6>                    32
  unsplit_k5   2^11   5  1       2^6     foldk_seg_sums_kernel<5>                           32
  split8_k8    2^14   8  0       2^6     foldk_split_kernel<8>  (no sums, output <= 2^13)   32 per lane

(m_next = 0 with an output of at most 2^13 entries always takes foldk_split_kernel, so the one-lane form is reached with segment sums
over segments shorter than half a workgroup.)  K = 8 needs ZK_BASIC_ROUNDS_PER_PASS=8, read once per process: the cases run in two
child processes (tests/_foldk_edge_worker.py), one per setting, started once for the module, both with ZK_HOST_TRANSCRIPT=1 set
explicitly: a handle that offers fewer than K rounds per pass is a failure, never a skip.

Conditions on BLS12-381 Fr in the three forms above the bound (tests/_foldk_shadow_model.py lanes_required): W > 2^261 in one part for
every kind; at least 8 outputs the model puts at or above 2 p for every non-uniform kind at 256 terms and for the near tables at 128
terms.  The other kinds cannot get there at 128 terms: a constant c folds to c, its lanes hold c + k p and reach 2 p only for
W > 141.3 p, and a third of a mix table is zero, which leaves its lanes the weight of some 85 terms.  BN254 Fr: no tuple with W > 169 p can be found (256 terms
sit at 128 p +- 5 p), so the same shapes assert only equality and canonicity."""
import json
import os
import subprocess
import sys

import pytest

import _foldk_shadow_model as FM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RESULTS = {}


def results(k8):
    if k8 not in _RESULTS:
        names = ",".join(s[0] for s in FM.SHAPES if (s[1] == 8) == k8)
        e = dict(os.environ)
        e["ZK_HOST_TRANSCRIPT"] = "1"                      # the multi-round passes exist with the host-assisted transcript step only
        if k8:
            e["ZK_BASIC_ROUNDS_PER_PASS"] = "8"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_foldk_edge_worker.py"), names], capture_output=True, text=True,
                           env=e, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        _RESULTS[k8] = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return _RESULTS[k8]


@pytest.mark.parametrize("kind", FM.KINDS)
@pytest.mark.parametrize("shape", [s[0] for s in FM.SHAPES])
@pytest.mark.parametrize("field", [0, 3])
def test_folded_table_is_exact_and_canonical(field, shape, kind):
    K = [s[1] for s in FM.SHAPES if s[0] == shape][0]
    res = results(K == 8)["%d-%s-%s" % (field, shape, kind)]
    assert res["multi_max"] >= K, res
    assert res["challenges_match_model"]
    if field == 0 and shape in FM.HOT:
        assert res["w_max_over_radix"] > 1.0, res
        assert res["hot_lanes_before_fix"] >= FM.lanes_required(shape, kind), res
    assert res["hot_lanes_after_fix"] == 0, res
    assert res["len"] == 1 << ([s[2] for s in FM.SHAPES if s[0] == shape][0] - K)
    assert res["noncanonical"] == 0, res
    assert res["mismatches"] == 0, res
    assert res["input_unchanged"]
