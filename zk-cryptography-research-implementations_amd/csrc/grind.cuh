// grind.cuh -- the nonce search of the proof-of-work step (include/zkmle.h "Proof-of-work grinding"): one candidate per LANE per iteration
// on the one-sponge-per-lane permutation of keccak_lane.cuh (the Merkle kernels').
//
// The transcript's sponge arrives as 25 lanes and the fill of its open block (Keccak256::export_state), by value in the kernel's argument
// block: every lane of every wave reads the same 26 words, so they live in scalar registers and a candidate starts as 25 copies.  The host
// has already XORed in whatever of the pad does not depend on the nonce.  The nonce w enters as its 8 big-endian bytes at byte `fill` of
// the rate: as the little-endian word v = bswap(w) shifted to that byte, into lane fill / 8 and, when fill is no multiple of 8, the lane
// after it.  Which lanes is uniform but not constant, so the XOR is a select per lane of the rate, not an indexed store into the state
// (that would move the state to scratch memory).
//   TWO = false  fill <= 127: nonce and pad (0x01 at fill + 8, 0x80 at 135) share the open block: one permutation
//   TWO = true   fill = 128 .. 135: 136 - fill bytes of the nonce end the open block, which is permuted; the other fill - 128 bytes and the
//                pad make the next block (fill = 128: the pad alone): two permutations
// Only word 0 of the last state is read (ZK_FRI_GRIND_MAX_BITS = 32 leading bits lie in its low half), so the compiler drops what of the
// last round feeds the other lanes.
//
// A launch covers [base, base + count) and always ends: a lane walks its candidates upwards with the grid's stride, hashes each, and on a
// hit lowers *best (all ones before the first hit) by atomicMin.  A lane whose candidate is already above *best stops: every later one of
// its candidates is larger still.  No lane waits for another or for the host; the smallest hit of the range is in *best when the kernel ends.
#pragma once
#include "keccak_lane.cuh"

namespace zk {

constexpr int kGrindBlock = 256;
constexpr unsigned kGrindMaxBlocks = 2048;                   // 256 CUs x 8 workgroups; the rest of a range by the grid's stride

struct GrindSponge {
    uint64_t a[25];                                          // the sponge after the tag, with the nonce-independent pad bytes of its block
    uint32_t fill;                                           // bytes in the open block, 0 .. 135
};

template <bool TWO> __global__ void __launch_bounds__(kGrindBlock) fri_grind_kernel(GrindSponge sp, uint64_t base, uint64_t count, uint32_t bits,
                                                                                      unsigned long long *__restrict__ best) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    // TWO: the nonce starts in the rate's last word (lane 16) at byte fill - 128; else in lane q at byte fill mod 8
    const unsigned q = TWO ? 16u : sp.fill >> 3, s = 8u * (sp.fill & 7u);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        const uint64_t w = base + i;
        if (w > __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        const uint64_t v = __builtin_bswap64(w), lo = v << s, hi = s ? v >> (64 - s) : 0;
        uint64_t a[25];
#pragma unroll
        for (int j = 0; j < 25; j++) a[j] = sp.a[j];
        if constexpr (TWO) {
            a[16] ^= lo;
            keccak_f1600_lane(a);
            a[0] ^= hi ^ ((uint64_t)0x01 << s);               // the nonce's last fill - 128 bytes, then the pad
            a[16] ^= (uint64_t)0x80 << 56;
        } else {
            switch (q) {                                     // a uniform branch to two XORs into named registers
#define ZK_GRIND_AT(Q) case Q: a[Q] ^= lo; a[Q + 1] ^= hi; break;
                ZK_GRIND_AT(0) ZK_GRIND_AT(1) ZK_GRIND_AT(2) ZK_GRIND_AT(3) ZK_GRIND_AT(4) ZK_GRIND_AT(5) ZK_GRIND_AT(6) ZK_GRIND_AT(7)
                ZK_GRIND_AT(8) ZK_GRIND_AT(9) ZK_GRIND_AT(10) ZK_GRIND_AT(11) ZK_GRIND_AT(12) ZK_GRIND_AT(13) ZK_GRIND_AT(14) ZK_GRIND_AT(15)
#undef ZK_GRIND_AT
            }
        }
        keccak_f1600_lane(a);
        // digest bytes 0 .. 7 are word 0 read little-endian: its big-endian reading has digest bit 0 on top
        if ((__builtin_bswap64(a[0]) >> (64 - bits)) == 0) atomicMin(best, (unsigned long long)w);
    }
}

}  // namespace zk
