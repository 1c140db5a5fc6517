"""Generator of tests/golden/foldk_hot_transcripts.json: for every shape of tests/_foldk_shadow_model.py SHAPES whose form sums more than
floor(2^261 / p) = 70 terms per reduction on BLS12-381 Fr, and every table kind, a nonce that -- appended to the transcript before
zk_rounds_new -- makes the first K challenges a tuple whose weights sum to more than 2^261 in one part (W >= 73 p), with at least
lanes_required(shape, kind) outputs the integer model puts at or above 2 p, one of which at least it stores at or above p (where
that count is 0: W alone).  CPU only, Python transcript model.

    python tests/golden/make_foldk_hot_transcripts.py        (about a minute)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import _foldk_shadow_model as FM                                                       # noqa: E402

FIELD = 0
W_MIN = 73


def search(table, K, form, need_lanes):
    p = FM.MODULUS[FIELD]
    n = len(table) >> K
    S = [FM.real(FIELD, sum(table[s * n:(s + 1) * n]) % p) for s in range(1 << K)]
    pl = FM.parts(form, K)
    for nonce in range(100000):
        rs = FM.challenges_from_sums(FIELD, S, nonce)
        if max(FM.weight_sums(FIELD, rs, pl)) < W_MIN * p:
            continue
        lanes = len(FM.over_range_lanes(FIELD, table, K, rs, pl))
        if lanes < need_lanes:
            continue
        # the lanes whose STORED element the model of the old form leaves at or above p (with two lanes per output the closing
        # fe_add takes one half's extra p away again unless the two reduced halves sum past p)
        wrong = sum(1 for v in FM.kernel_result(FIELD, table, K, rs, pl) if v >= p) if need_lanes else 0
        if wrong >= (1 if need_lanes else 0):
            return nonce, lanes, wrong
    raise SystemExit("no nonce found")


def main():
    out = {"comment": "nonces found by make_foldk_hot_transcripts.py; lanes = outputs the model puts at or above 2 p before the fix, stored_at_or_above_p = those it then stores non-canonical",
           "fields": {str(FIELD): {}}}
    for name, K, logn, _m_next, form in FM.SHAPES:
        if name not in FM.HOT:
            continue
        out["fields"][str(FIELD)][name] = {}
        for kind in FM.KINDS:
            table = FM.make_table(FIELD, kind, 1 << logn)
            nonce, lanes, wrong = search(table, K, form, FM.lanes_required(name, kind))
            out["fields"][str(FIELD)][name][kind] = {"nonce": nonce, "lanes": lanes, "stored_at_or_above_p": wrong}
            print(name, kind, nonce, lanes, wrong, flush=True)
    with open(os.path.join(HERE, "foldk_hot_transcripts.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
