// keccak_lane.cuh -- Keccak-f[1600] with the 25 lanes of ONE sponge in the VGPRs of ONE GPU lane, all 24 rounds unrolled (round constants and
// rotation counts become immediates): 64 independent permutations per wave, no LDS, no cross-lane traffic.  Shared by the Merkle kernels
// (merkle.cuh) and the proof-of-work search (grind.cuh); a header of its own because merkle.cuh also defines kernels that are no templates
// and so belong to one translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zk {

__device__ __forceinline__ uint64_t mk_rotl(uint64_t x, unsigned s) { return s ? (x << s) | (x >> (64 - s)) : x; }

// Keccak-f[1600], state a[x + 5 y]
__device__ __forceinline__ void keccak_f1600_lane(uint64_t (&a)[25]) {
    constexpr uint64_t rc[24] = {
        0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
        0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
        0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
        0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    constexpr unsigned rho[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
#pragma unroll
    for (int round = 0; round < 24; round++) {
        uint64_t c[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; x++) {
            const uint64_t d = c[(x + 4) % 5] ^ mk_rotl(c[(x + 1) % 5], 1);
#pragma unroll
            for (int y = 0; y < 5; y++) a[x + 5 * y] ^= d;
        }
#pragma unroll
        for (int x = 0; x < 5; x++)
#pragma unroll
            for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = mk_rotl(a[x + 5 * y], rho[x + 5 * y]);
#pragma unroll
        for (int y = 0; y < 5; y++)
#pragma unroll
            for (int x = 0; x < 5; x++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        a[0] ^= rc[round];
    }
}

}  // namespace zk
