"""The integer shadow of the MSM pipeline (tests/_msm_shadow_model.py) and the scenarios built on it (tests/_msm_cases.py), without a GPU:
  * the model computes sum s_i m_i mod r on random small inputs at every form of the pipeline -- which licenses trusting its tally;
  * the scenarios, taken together, send equal, opposite, one-infinite and both-infinite operands through EVERY stage at every form
    (one lane / quad, bit sums / tail), and waves of three or more classes through every quad stage;
  * the signed digits of the edge scalars.
tests/test_gpu_msm_group_law.py runs the same scenarios on the GPU; nothing it asserts depends on the model."""
import functools
import random

import pytest

import _msm_cases as MC
import _msm_shadow_model as SM

R = SM.R


@pytest.mark.parametrize("c,pre", [(2, False), (4, False), (5, False), (6, False), (9, False), (13, False), (16, False), (18, False),
                                   (9, True), (13, True), (18, True)])
def test_model_computes_the_msm(c, pre):
    rng = random.Random(1000 * c + pre)
    for it in range(200 if c <= 6 else 100):                 # (a run at the wide windows costs ~0.1 s: their short arrays are walked entry by entry)
        n = rng.randrange(1, 24)
        m = [rng.randrange(-8, 9) for _ in range(n)]
        s = [rng.choice((rng.randrange(R), rng.randrange(R), rng.randrange(1 << (2 * c)), R - 1 - rng.randrange(3))) for _ in range(n)]
        got, _ = SM.shadow(m, s, c, pre, force_tail=bool(it & 1) and c >= 6)
        assert got == SM.expected(m, s), (c, pre, it, m, s)
    assert SM.shadow([1, 1], [5, R - 5], c, pre)[0] is None                  # infinity is None, not 0


def test_model_window_rule():
    assert [SM.pick_window(n) for n in (1, 5, 255, 256, 4096, (1 << 14) - 1, 1 << 14, 1 << 18, 1 << 19)] == [4, 4, 4, 5, 9, 10, 13, 13, 16]


@functools.lru_cache(maxsize=None)
def union_tally(c, pre):
    total, per_case = SM.Tally(), {}
    for case in MC.scenarios(c, pre):
        assert len(case.m) == len(case.s) <= 1 << 12
        assert all(abs(x) <= 64 or (pre and case.name == "precomputed_copies") for x in case.m), case.name
        assert all(0 <= x < R for x in case.s)
        got, t = SM.shadow(case.m, case.s, c, pre)
        assert got == SM.expected(case.m, case.s), case.name
        per_case[case.name] = t
        total.merge(t)
    return total, per_case


STAGES = {   # what runs at this window, by the launch rule of csrc/msm_reduce.hip (work <= 2^13: a quad per addition)
    (4, False): {"bucket_sum", "regroup", "combine", "reduce_level/quad", "window_sums", "host_horner"},
    (9, False): {"bucket_sum", "regroup", "combine", "plain_level/quad", "bit_sums/quad", "bit_combine/quad", "host_two_stage", "host_horner"},
    (13, False): {"bucket_sum", "regroup", "combine", "plain_level/lane", "plain_level/quad", "bit_sums/quad", "bit_combine/quad", "host_two_stage",
                  "host_horner"},
    (13, True): {"bucket_sum", "regroup", "combine", "plain_level/quad", "bit_sums/quad", "bit_combine/quad", "host_two_stage"},
    (18, False): {"bucket_sum", "regroup", "combine", "plain_level/lane", "plain_level/quad", "reduce_level/lane", "reduce_level/quad", "tail/quad",
                  "host_two_stage", "host_horner"},
}


@pytest.mark.parametrize("c,pre", sorted(STAGES))
def test_scenarios_reach_every_stage_and_class(c, pre):
    """no cell is exempt: every stage x {equal, opposite, one infinite, both infinite} has traffic, every quad stage a wave of >= 3 classes,
    and every stage that doubles also doubles infinity"""
    total, _ = union_tally(c, pre)
    adds, mixed = total.adds, total.mixed_waves()
    assert set(adds) == STAGES[(c, pre)], total.table()
    empty = [(st, cls) for st in sorted(adds) for cls in SM.NONGENERIC if adds[st][cls] == 0]
    empty += [(st, "mixed wave") for st in sorted(adds) if st.endswith("/quad") and mixed[st] == 0]
    empty += [(st, "doubling of infinity") for st in sorted(total.dbls) if total.dbl_inf[st] == 0]
    assert not empty, "%s\n%s" % (empty, total.table())


def test_named_scenarios_do_what_they_say():
    for c in (4, 9):
        _, per = union_tally(c, False)
        post = [st for st in per["uniform"].adds if st.split("/")[0] in ("plain_level", "reduce_level", "bit_sums", "tail")]
        for st in post:                                      # uniform: every addition of every level and bit tree that has two operands is P + P
            row = per["uniform"].adds[st]
            assert row["equal"] > 0 and row["opposite"] == 0, (c, st, row)
        assert per["uniform"].adds["plain_level/quad" if c == 9 else "reduce_level/quad"]["equal"] > 0      # the equal-points branch of g1u_add_quad
        top = max(int(n.rsplit("bit", 1)[1]) for n in per if n.startswith("cancel_bases_bit"))
        for name in ("cancel_bases_bit%d" % top, "cancel_digits_bit%d" % top):                              # cancelling halves
            row = per[name].adds["plain_level/quad" if c == 9 else "reduce_level/quad"]
            assert row["opposite"] > 0 and row["inf_inf"] > 0, (c, name, row)
        assert per["accumulation_heavy"].adds["regroup"]["equal"] > 0 and per["accumulation"].adds["regroup"] == {}
        assert per["accumulation"].adds["combine"]["opposite"] > 0 and per["accumulation"].adds["bucket_sum"]["opposite"] > 0
        assert sum(per["checkerboard%d" % v].mixed_waves()["plain_level/quad" if c == 9 else "reduce_level/quad"] for v in range(3)) > 0
    for name in ("vanish_s_and_r_minus_s", "vanish_neg_base"):
        assert SM.shadow(*[getattr(dict((k.name, k) for k in MC.scenarios(9))[name], f) for f in ("m", "s")], 9)[0] is None


def test_random_inputs_never_reach_the_exceptional_paths_after_the_buckets():
    """what the suite had before: random scalars on distinct bases -- no equal or opposite operands anywhere behind the bucket sums"""
    rng = random.Random(7)
    n = 256
    m, s = [rng.randrange(1, R) for _ in range(n)], [rng.randrange(R) for _ in range(n)]
    for c in (4, 9):
        _, t = SM.shadow(m, s, c)
        for st, row in t.adds.items():
            if st != "bucket_sum":
                assert row["equal"] == 0 and row["opposite"] == 0, (c, st, row)


@pytest.mark.parametrize("c", [2, 4, 5, 9, 13, 16, 17, 20, 24])
def test_digit_edges(c):
    nwin, half = SM.nwindows(c), 1 << (c - 1)
    edges = MC.edge_scalars(c)
    assert len(edges) >= 10
    seen = set()
    for s in edges:
        d = SM.signed_digits(s, c)
        assert len(d) == nwin and SM.from_digits(d, c) == s
        assert all(-half <= x < half for x in d[:-1]) and d[-1] >= 0, (c, hex(s), d)
        seen.update(x for x in d[:-1] if abs(x) in (half - 1, half))
        seen.add(("top", d[-1]))
    assert {-half, half - 1, -(half - 1) if c > 2 else -half} <= seen         # the magnitude 2^(c-1) occurs, and only as a negative digit
    assert half not in seen
    if c == 2:
        assert ("top", half) in seen                         # ... except in the top window, by a carry
    d = SM.signed_digits((1 << 254) - 1, c)                  # carries through every window: -1, 0, 0, ..., then the top digit takes the carry
    assert d[0] == -1 and all(x == 0 for x in d[1:254 // c]) and d[-1] > 0
