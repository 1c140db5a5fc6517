// merkle_columns.cuh -- level 0 of a Merkle tree over k COLUMNS (include/zkmle.h "Merkle commitment of several columns"; 32-byte elements
// only): k tables of one length under one tree whose leaf j holds the fold coset of every column.  With part = len >> 2, j < part,
//   leaf_j = Keccak256(0x00 || for c < k: for s < 4: bytes(f_c[j + s part]))
// 1 + 128 k bytes: the quad leaf of merkle_leaf_group_kernel<F, 2> once per column behind ONE tag, so k = 1 is that leaf byte for byte.  The
// nodes above are merkle.cuh's over `part` leaves.
//
// The message is longer than the rate from k = 2 on, so the lane runs a sponge: B(k) = floor((1 + 128 k) / 136) + 1 permutations.  It walks
// the 16 k big-endian words of the message one at a time; the tag byte shifts every word by 8 bits (merkle_block), so the top byte of each
// word is carried into the next.  Where a word lands in the rate depends on k and the word's number alone, which are the same for every lane
// of the wave: the word is XORed into the state through a uniform 17-way branch, the state stays in registers and nothing is indexed
// dynamically.  (1 + 128 k) mod 136 is odd and never 135, so the first pad byte always follows the carry byte inside one word and never
// meets the rate's last byte; at k = 17 that word is alone in the last block.  ONE permutation site serves every block, the last included.
#pragma once
#include "merkle.cuh"

namespace zk {

constexpr int kMerkleColumnsMax = 32;

struct MerkleColumnsArgs {
    const void *t[kMerkleColumnsMax];                        // the columns, `len` elements each
    int k;
};

// a[pos] ^= m with pos wave-uniform, pos < 17
__device__ __forceinline__ void merkle_absorb_word(uint64_t (&a)[25], int pos, uint64_t m) {
    switch (pos) {
#define ZK_ABSORB_AT(P) case P: a[P] ^= m; break;
        ZK_ABSORB_AT(0) ZK_ABSORB_AT(1) ZK_ABSORB_AT(2) ZK_ABSORB_AT(3) ZK_ABSORB_AT(4) ZK_ABSORB_AT(5) ZK_ABSORB_AT(6) ZK_ABSORB_AT(7) ZK_ABSORB_AT(8)
        ZK_ABSORB_AT(9) ZK_ABSORB_AT(10) ZK_ABSORB_AT(11) ZK_ABSORB_AT(12) ZK_ABSORB_AT(13) ZK_ABSORB_AT(14) ZK_ABSORB_AT(15)
#undef ZK_ABSORB_AT
        default: a[16] ^= m; break;
    }
}

// one lane per leaf j < part, which reads f_c[j + s part] for c < k, s < 4: across a wave each of the 4 k strided streams is coalesced
template <class F> __global__ void __launch_bounds__(kMerkleBlock) merkle_leaf_columns_kernel(const MerkleColumnsArgs args, size_t part, uint64_t *__restrict__ out) {
    static_assert(F::N == 8, "32-byte elements");
    const int nwords = 16 * args.k;                           // of the message behind the tag; word i is word i & 3 of element i >> 2
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < part; j += stride) {
        uint64_t a[25];
#pragma unroll
        for (int t = 0; t < 25; t++) a[t] = 0;
        uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, carry = 0x00;   // the element's four words; the tag, then the last word's top byte
        int pos = 0;
        for (int i = 0; i <= nwords; i++) {
            const bool last = i == nwords;
            uint64_t m = carry | ((uint64_t)0x01 << 8);       // the word behind the message: its last byte and the pad's first
            if (!last) {
                const int w = i & 3;
                if (w == 0) {
                    uint64_t s[4];
                    merkle_be_words<F>(s, fe_load<F>(args.t[i >> 4], j + (size_t)((i >> 2) & 3) * part));
                    s0 = s[0]; s1 = s[1]; s2 = s[2]; s3 = s[3];
                }
                const uint64_t x = w == 0 ? s0 : w == 1 ? s1 : w == 2 ? s2 : s3;
                m = carry | (x << 8);
                carry = x >> 56;
            }
            merkle_absorb_word(a, pos, m);
            if (last) a[16] ^= (uint64_t)0x80 << 56;
            if (++pos == 17 || last) {
                keccak_f1600_lane(a);
                pos = 0;
            }
        }
        digest_store(out, j, merkle_digest_of(a));
    }
}

}  // namespace zk
