// grind_host.h -- the proof-of-work step of the FRI transcripts (include/zkmle.h "Proof-of-work grinding") on the host: the tag, the test of
// a digest's leading bits, the verifier's step, and the search on one core.  The search is the definition spelled out with the transcript's
// own Keccak256, cloned per candidate: the GPU search (grind.cuh, zkmle_grind.hip) must return what it returns.  Depends on transcript.h alone,
// so a stand-alone host program can compile it (tools/grind_selftest.hip).
#pragma once
#include "transcript.h"

namespace zk {

constexpr uint32_t kGrindMaxBits = 32;                       // ZK_FRI_GRIND_MAX_BITS

inline void grind_put_be64(uint8_t out[8], uint64_t v) {
    for (int k = 0; k < 8; k++) out[k] = (uint8_t)(v >> (56 - 8 * k));
}
// bit i of a digest is bit 7 - i mod 8 of byte i div 8: the first `bits` <= 32 of them are zero
inline bool grind_leading_zero(const uint8_t dg[32], uint32_t bits) {
    const uint32_t head = ((uint32_t)dg[0] << 24) | ((uint32_t)dg[1] << 16) | ((uint32_t)dg[2] << 8) | (uint32_t)dg[3];
    return bits == 0 || (head >> (32 - bits)) == 0;
}
// step 1: "GRND", then the bit count as a big-endian u32, in one append
inline void grind_tag(Transcript &tr, uint32_t bits) {
    uint8_t tag[8] = {'G', 'R', 'N', 'D'};
    for (int k = 0; k < 4; k++) tag[4 + k] = (uint8_t)(bits >> (24 - 8 * k));
    tr.append(tag, sizeof tag);
}
// step 2's test of one candidate: the digest of (everything absorbed so far || w), on a clone
inline bool grind_candidate(const Keccak256 &h, uint64_t w, uint32_t bits) {
    Keccak256 c = h;
    uint8_t wb[8], dg[32];
    grind_put_be64(wb, w);
    c.update(wb, 8);
    c.finalize_copy(dg);
    return grind_leading_zero(dg, bits);
}
// step 3: append w, sample the challenge (the digest of step 2, absorbed back as always).  -> the challenge has its leading bits zero
inline bool grind_finish(Transcript &tr, uint32_t bits, uint64_t w) {
    uint8_t wb[8], dg[32];
    grind_put_be64(wb, w);
    tr.append(wb, 8);
    tr.sample_random_challenge(dg);
    return grind_leading_zero(dg, bits);
}
// the verifier's step: the tag, w, the challenge; the transcript ends where the prover's did whatever the answer
inline bool grind_check(Transcript &tr, uint32_t bits, uint64_t w) {
    grind_tag(tr, bits);
    return grind_finish(tr, bits, w);
}
// the hard cap of a search: 2^(bits + 6) candidates, which an honest search exceeds with probability e^-64
inline uint64_t grind_cap(uint32_t bits) { return (uint64_t)1 << (bits + 6); }

// steps 1-3 on one core: the smallest w >= start among the first max_tries candidates (0: grind_cap).  false: none of them, and then the
// transcript is as it was
inline bool grind_search_host(Transcript &tr, uint32_t bits, uint64_t start, uint64_t max_tries, uint64_t *nonce) {
    Transcript tagged = tr;
    grind_tag(tagged, bits);
    if (max_tries == 0) max_tries = grind_cap(bits);
    const Keccak256 &h = tagged.sponge();
    for (uint64_t i = 0; i < max_tries; i++) {
        const uint64_t w = start + i;
        if (w < start || w == ~(uint64_t)0) break;           // 2^64 - 1 is the device search's "no hit" and is not a candidate
        if (!grind_candidate(h, w, bits)) continue;
        (void)grind_finish(tagged, bits, w);
        tr = tagged;
        *nonce = w;
        return true;
    }
    return false;
}

}  // namespace zk
