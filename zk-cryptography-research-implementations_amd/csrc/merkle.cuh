// merkle.cuh -- Keccak-256 Merkle commitment of a table: one hash per LANE (include/zkmle.h "Merkle commitment").
//
//   leaf_i = Keccak256(0x00 || bytes(e_i))        bytes = convert_to_bytes of one element: canonical big-endian, 32 or 48 bytes
//   node   = Keccak256(0x01 || left || right)      node j of level l + 1 hashes nodes 2j, 2j + 1 of level l; level 0 = the leaves
//   root   = the single node of level log2(len); a one-entry table's root is leaf_0
//
// GROUPED leaves (include/zkmle.h "Merkle commitment with grouped leaves"; 32-byte elements only): with part = len >> LG, LG = 1 or 2,
//   leaf_j = Keccak256(0x00 || bytes(e_j) || bytes(e_{j+part}) || .. )    the 2^LG entries a FRI fold of arity 2^LG reads together, j < part
// and the nodes above are the same over `part` leaves.  The pair leaf (LG = 1, 65 bytes) has a NODE's length but a LEAF's tag: the tag byte
// alone tells it from a node.  The quad leaf is 129 bytes, 131 with the pad's two bytes: still inside the 136-byte rate.
//
// Keccak-256 is the transcript's (transcript.h): rate 136, original pad 0x01 .. 0x80.  Every input is 33, 49, 65 or 129 bytes: one block, one
// permutation per hash.  The permutation (keccak_lane.cuh) keeps the 25 lanes of ONE sponge in the VGPRs of ONE GPU lane, all 24 rounds unrolled
// (round constants and rotation counts become immediates): 64 independent hashes per wave, no LDS, no cross-lane traffic.  The
// wave-per-sponge permutation of dev_transcript.cuh is the other shape -- one sequential sponge, as fast as it can go -- and stays.
//
// A digest is kept as 4 u64 words = its 32 bytes read little-endian, which is also how the state's lanes 0 .. 3 hold it.
#pragma once
#include "fields.cuh"
#include "keccak_lane.cuh"
#include "ufield.cuh"

namespace zk {

constexpr int kMerkleBlock = 256;          // 4 waves; the hash kernels are pure VALU work
constexpr size_t kMerkleFinish = 512;      // a level of at most this many nodes is finished by ONE workgroup (merkle_finish_kernel)

struct Digest {
    uint64_t w[4];
};

// The padded block of a message of 1 + 8 NW bytes: the tag byte, then the NW words of `s` as they lie in memory (NW = 4 or 6: a leaf's
// big-endian element; NW = 8: two digests or a pair leaf; NW = 16: a quad leaf, whose pad starts in the rate's last word).  Everything after
// the pad is zero but the rate's last byte.
template <int NW> __device__ __forceinline__ void merkle_block(uint64_t (&a)[25], uint64_t tag, const uint64_t (&s)[NW]) {
    static_assert(NW <= 16, "the message and its first pad byte must fit the rate of 17 words");
    a[0] = tag | (s[0] << 8);
#pragma unroll
    for (int j = 1; j < NW; j++) a[j] = (s[j - 1] >> 56) | (s[j] << 8);
    a[NW] = (s[NW - 1] >> 56) | ((uint64_t)0x01 << 8);
#pragma unroll
    for (int j = NW + 1; j < 25; j++) a[j] = 0;
    a[16] ^= (uint64_t)0x80 << 56;
}

// element (Montgomery) -> canonical big-endian bytes, as OP_TO_CANONICAL_BE (mle_kernels.cuh) does: F::N / 2 words at s
template <class F> __device__ __forceinline__ void merkle_be_words(uint64_t *s, const Fe<F> &x) {
    const Fe<F> c = fe_to_canonical<F>(x);                                          // into_bigint()
#pragma unroll
    for (int t = 0; t < F::N / 2; t++)                                              // to_bytes_be(): word t = bytes 8 t .. 8 t + 7
        s[t] = (uint64_t)__builtin_bswap32(c.l[F::N - 1 - 2 * t]) | ((uint64_t)__builtin_bswap32(c.l[F::N - 2 - 2 * t]) << 32);
}
// ... into the leaf's block
template <class F> __device__ __forceinline__ void merkle_leaf_block(uint64_t (&a)[25], const Fe<F> &x) {
    constexpr int NW = F::N / 2;
    uint64_t s[NW];
    merkle_be_words<F>(s, x);
    merkle_block<NW>(a, 0x00, s);
}
__device__ __forceinline__ void merkle_node_block(uint64_t (&a)[25], const Digest &l, const Digest &r) {
    const uint64_t s[8] = {l.w[0], l.w[1], l.w[2], l.w[3], r.w[0], r.w[1], r.w[2], r.w[3]};
    merkle_block<8>(a, 0x01, s);
}
__device__ __forceinline__ Digest merkle_digest_of(const uint64_t (&a)[25]) { return Digest{{a[0], a[1], a[2], a[3]}}; }

__device__ __forceinline__ Digest digest_load(const uint64_t *base, size_t idx) {
    const uint4 *p = reinterpret_cast<const uint4 *>(base) + 2 * idx;
    const uint4 u = p[0], v = p[1];
    return Digest{{(uint64_t)u.x | ((uint64_t)u.y << 32), (uint64_t)u.z | ((uint64_t)u.w << 32), (uint64_t)v.x | ((uint64_t)v.y << 32),
                   (uint64_t)v.z | ((uint64_t)v.w << 32)}};
}
__device__ __forceinline__ void digest_store(uint64_t *base, size_t idx, const Digest &d) {
    uint4 *p = reinterpret_cast<uint4 *>(base) + 2 * idx;
    p[0] = make_uint4((uint32_t)d.w[0], (uint32_t)(d.w[0] >> 32), (uint32_t)d.w[1], (uint32_t)(d.w[1] >> 32));
    p[1] = make_uint4((uint32_t)d.w[2], (uint32_t)(d.w[2] >> 32), (uint32_t)d.w[3], (uint32_t)(d.w[3] >> 32));
}

// level 0: one lane per leaf
template <class F> __global__ void __launch_bounds__(kMerkleBlock) merkle_leaf_kernel(const void *__restrict__ table, size_t len, uint64_t *__restrict__ out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += stride) {
        uint64_t a[25];
        merkle_leaf_block<F>(a, fe_load<F>(table, i));
        keccak_f1600_lane(a);
        digest_store(out, i, merkle_digest_of(a));
    }
}

// level 0 with grouped leaves: one lane per leaf j < part = len >> LG, which reads e[j + s part], s < 2^LG -- across a wave each of the 2^LG
// strided streams is coalesced -- and hashes them as ONE block: the permutation a single-element leaf costs
template <class F, int LG> __global__ void __launch_bounds__(kMerkleBlock) merkle_leaf_group_kernel(const void *__restrict__ table, size_t part,
                                                                                                   uint64_t *__restrict__ out) {
    static_assert(F::N == 8 && (LG == 1 || LG == 2), "32-byte elements, two or four to a leaf");
    constexpr int G = 1 << LG;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < part; j += stride) {
        uint64_t s[4 * G], a[25];
#pragma unroll
        for (int g = 0; g < G; g++) merkle_be_words<F>(s + 4 * g, fe_load<F>(table, j + (size_t)g * part));
        merkle_block<4 * G>(a, 0x00, s);
        keccak_f1600_lane(a);
        digest_store(out, j, merkle_digest_of(a));
    }
}

// one level up: one lane per node; out[j] = H(0x01 || in[2j] || in[2j + 1]), n = nodes written
__global__ void __launch_bounds__(kMerkleBlock) merkle_node_kernel(const uint64_t *__restrict__ in, size_t n, uint64_t *__restrict__ out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
        uint64_t a[25];
        merkle_node_block(a, digest_load(in, 2 * j), digest_load(in, 2 * j + 1));
        keccak_f1600_lane(a);
        digest_store(out, j, merkle_digest_of(a));
    }
}

// The top of the tree in one workgroup: `lv` holds n <= kMerkleFinish digests (n a power of two, >= 2); the levels above are written right
// behind it, n / 2 then n / 4 ... then the root at lv[2 n - 2].  One permutation site, run by half as many lanes each time: these are the
// levels whose dense launches would each cost a launch for less than one wave's worth of work per CU.
__global__ void __launch_bounds__(kMerkleBlock) merkle_finish_kernel(uint64_t *lv, unsigned n) {
    uint64_t *in = lv;
    for (unsigned m = n / 2; m >= 1; m /= 2) {
        uint64_t *out = in + (size_t)8 * m;                                        // behind the 2 m digests of this level
        for (unsigned j = threadIdx.x; j < m; j += blockDim.x) {
            uint64_t a[25];
            merkle_node_block(a, digest_load(in, 2 * j), digest_load(in, 2 * j + 1));
            keccak_f1600_lane(a);
            digest_store(out, j, merkle_digest_of(a));
        }
        __threadfence_block();
        __syncthreads();
        in = out;
    }
}

// every requested path with one launch: lane (q, l) copies the sibling of index[q]'s ancestor at level l.  `tree` = all levels, level l at
// digest offset 2 len - (2 len >> l)
__global__ void merkle_open_kernel(const uint64_t *__restrict__ tree, size_t len, unsigned depth, const uint64_t *__restrict__ indices, size_t nidx,
                                   uint64_t *__restrict__ paths) {
    const size_t total = nidx * depth, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const size_t q = t / depth;
        const unsigned l = (unsigned)(t % depth);
        const size_t off = 2 * len - ((2 * len) >> l), sib = (indices[q] >> l) ^ 1;
        digest_store(paths, t, digest_load(tree, off + sib));
    }
}

}  // namespace zk
