// round_schedule.h -- how many rounds each transcript exchange of a sumcheck covers.  In the host-assisted mode the proving thread
// queues one request per exchange before a tail or pass kernel runs (zkmle_sumcheck.hip DeviceRounds) and the kernel decides for
// itself when to post: both walk these functions, so they cannot disagree.  Pure functions of lengths; the switches that feed them
// (ZK_TAIL_TWO_ROUNDS, ZK_BASIC_ROUNDS_PER_PASS) are read by the callers and passed in.
#pragma once
#include <stddef.h>

#include "fields.cuh"

namespace zk {

// the one-workgroup tail (dev_transcript.cuh sumcheck_tail_kernel, basic_multi.cuh basic_tail_kernel) takes tables of <= kTailLen entries
constexpr int kTailBlock = 512;
constexpr size_t kTailLen = 4 * (size_t)kTailBlock;
// basic tail: rounds per exchange at most (its sums and challenges live in LDS)
constexpr int kTailMultiMax = 6;

// Sumcheck tail: the rounds the next exchange covers on tables of `cl` entries -- 0 once fewer than 4 are left (the last fold needs no
// exchange), 2 while the (product, quad) pairs number at most `two_rounds` (host-assisted step, two-factor products; 0 = never), else 1.
// An exchange of k rounds leaves cl >> k entries.  A tail entered with two challenges pending (pending2, after a two-round exchange of
// split2_round_kernel) first folds by the first of them without an exchange: its schedule starts at len / 2 entries and round + 1.
ZK_HD constexpr bool tail_takes_two(size_t cl, int nprod, int two_rounds) {
    return two_rounds && cl >= 8 && (size_t)nprod * (cl / 8) <= (size_t)two_rounds;
}
ZK_HD constexpr int tail_step(size_t cl, int nprod, int two_rounds) { return tail_takes_two(cl, nprod, two_rounds) ? 2 : cl >= 4 ? 1 : 0; }

// Basic-sumcheck tail: the rounds the next exchange covers on a table of 2 <= cl <= kTailLen entries
ZK_HD constexpr unsigned basic_tail_step(size_t cl) {
    const unsigned lg = 31u - (unsigned)__builtin_clz((unsigned)cl);
    return lg < (unsigned)kTailMultiMax ? lg : (unsigned)kTailMultiMax;
}

// Basic sumcheck, grid-wide passes: the rounds of the next pass over a table of `global_len` > kTailLen entries, at most kmax.  Never
// past the length the tail takes over at, and the rounds left are spread evenly over the passes they need (13 rounds = 7 + 6 rather
// than 8 + 5: the host's share of an exchange grows with 2^m, and the fold of 8 variables reads 256 streams per lane -- r3 sweep at
// 2^24 / 2^20, ms per proof: m <= 4 0.338 / 0.123, 5 0.346 / 0.120, 6 0.330 / 0.121, 7 0.332 / 0.137 (7 + 2), 8 0.348 / 0.191)
constexpr int rounds_per_pass(size_t global_len, int kmax) {
    const int left = __builtin_clzll((unsigned long long)kTailLen) - __builtin_clzll((unsigned long long)global_len);   // log2 global_len - log2 kTailLen
    const int passes = (left + kmax - 1) / kmax;
    return (left + passes - 1) / passes;
}

}  // namespace zk
