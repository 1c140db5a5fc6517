"""Generator of tests/golden/gkr_ufold_witnesses.json: builds tools/find_fold_witness.hip (a host program, CPU only), runs its ufold
mode for the two scalar fields and writes what it prints as JSON.  A hit is reproducible from (field, seed, trial) alone, and a round
is 2^28 trials whatever the thread count, so the file does not depend on the machine.

    python tests/golden/make_gkr_ufold_witnesses.py        (a few seconds on 8 threads)"""
import json
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SEED, WANT, MAX_ROUNDS, THREADS = 20261019, 3, 64, 8
BUILD = "hipcc --offload-arch=gfx950 -O2 -std=c++17 -pthread tools/find_fold_witness.hip -o find_fold_witness"
ABOUT = ("Stored-form (Montgomery) operands of ufold (csrc/ufield.cuh: a + r (b - a), the fold of the GKR round kernels in "
         "csrc/sumcheck_kernels.cuh) whose value before the reduction is >= 2 p: fe_from_u_below_2p takes its second subtraction, and the "
         "un-reduced value feeds the lazy products of the next round's evaluations. gamma = the challenge r, s = a = p - 1 as stored limbs, "
         "t = b. Found by tools/find_fold_witness.hip in its ufold mode; an element is four 64-bit hexadecimal limbs, least significant first.")


def main():
    out = {"about": ABOUT, "build": BUILD, "fields": {}}
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "find_fold_witness")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O2", "-std=c++17", "-pthread",
                               os.path.join(ROOT, "tools", "find_fold_witness.hip"), "-o", exe])
        for field in (0, 3):
            args = [str(field), str(SEED), str(WANT), str(MAX_ROUNDS), str(THREADS), "ufold"]
            lines = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.splitlines()
            head = lines[0].split()            # field <id> <name> mode ufold seed <seed> trials <n> hits <h>
            assert head[0] == "field" and head[4] == "ufold" and lines[1].startswith("gamma") and lines[2].startswith("s ")
            out["fields"][str(field)] = {
                "name": head[2], "command": "find_fold_witness " + " ".join(args), "seed": int(head[6]), "trials": int(head[8]),
                "gamma": lines[1].split()[1:], "s": lines[2].split()[1:],
                "witnesses": [{"trial": int(w[1]), "t": w[3:7]} for w in (l.split() for l in lines[3:])],
            }
    with open(os.path.join(HERE, "gkr_ufold_witnesses.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
