// ntt.cuh -- radix-2 number-theoretic transform over the scalar fields, several butterfly levels per pass, held in LDS.
//
// n = 2^log_n is cut into D digits, n = n_0 n_1 .. n_{D-1} (digit 0 the most significant of the input index, the least significant of
// the output index).  Pass d < D - 1 transforms digit d at its place: a workgroup's tile is n_d points S_d = n_{d+1} .. n_{D-1} apart by C
// adjacent columns (C >= 4: every global access is a whole 128-byte line), and the transformed entry (k_d, lo) leaves multiplied by the
// twist w_n^(T_d k_d lo), T_d = n_0 .. n_{d-1}.  The last pass transforms the contiguous digit of C rows whose k_0 are adjacent and
// stores entry k of row (k_0 .. k_{D-2}) at k_0 + n_0 k_1 + .. + T_{D-1} k: the digit reversal that brings the output into natural
// order, again in 128-byte pieces.  D = 1 (a table that fits one workgroup's LDS) is the last pass alone.
//
// Inside a tile: decimation in time on canonical stored-form elements.  The twiddles w_P^j, j < P / 2, sit in LDS as the 29-bit limbs of
// their stored form, so that a butterfly's product is one umul_std scan with no conversion of the multiplier (ufield.cuh).  The twist
// and the coset powers base^e, e < n, are read from two small tables, base^lo (4096 entries, 29-bit limbs) and base^(4096 hi) (stored
// form): one extra product per element instead of a table of n entries.
#pragma once
#include "ufield.cuh"

namespace zk {

constexpr int kNttBlock = 256;
constexpr unsigned kNttTileLog = 10;        // elements of a tile: 32 KiB of LDS for the four-limb fields
constexpr unsigned kNttDigitMax = 8;        // levels of a pass of a transform that takes several
constexpr unsigned kNttLoBits = 12;         // base^e = lo[e mod 2^12] * hi[e >> 12]
constexpr unsigned kNttMaxDigits = 12;

// p - 1 = 2^S t, t odd; G generates the multiplicative group (unused where S = 1: w_2 = -1)
template <class F> struct NttField;
template <> struct NttField<Fr381> { static constexpr unsigned S = 32, G = 7; };
template <> struct NttField<Fq381> { static constexpr unsigned S = 1, G = 0; };
template <> struct NttField<Bn254Fq> { static constexpr unsigned S = 1, G = 0; };
template <> struct NttField<Bn254Fr> { static constexpr unsigned S = 28, G = 5; };

// out[j] = pre * base^j, j < count: 29-bit limbs of the stored form (UFORM: a multiplier of umul_std) or the stored form itself
template <class F, bool UFORM> __global__ void __launch_bounds__(kNttBlock) ntt_pow_table_kernel(Fe<F> base, Fe<F> pre, uint32_t count, void *__restrict__ out) {
    for (uint32_t j = blockIdx.x * kNttBlock + threadIdx.x; j < count; j += gridDim.x * kNttBlock) {
        Fe<F> acc = pre, b = base;
        for (uint32_t e = j; e; e >>= 1) {
            if (e & 1) acc = fe_mul<F>(acc, b);
            b = fe_sqr<F>(b);
        }
        if (UFORM) reinterpret_cast<Ufe<F> *>(out)[j] = u_from_limbs32<F>(acc);
        else fe_store<F>(out, j, acc);
    }
}

struct NttPassArgs {
    const void *src;
    void *dst;
    uint64_t src_len;                 // entries of src that exist: the others read as zero (low-degree extension) and are never loaded
    const void *tw;                   // Ufe[2^(tw_log - 1)]: w_{2^tw_log}^j
    const void *twist_lo, *twist_hi;  // w_n^e; twist_hi null when n <= 2^12
    const void *scale_lo, *scale_hi;  // the factor of entry i: of the loaded entry (scale_mode 1: c^i) or of the stored one (2: n^-1 c^-i)
    uint32_t scale_mode, scale_mask;  // scale_mask 0: the same factor scale_lo[0] for every entry
    uint32_t log_n, log_p, log_c, log_s, log_t, tw_log;
    uint32_t log_k0;                  // last pass: log2 n_0, the digit the columns run over (0 when D = 1)
    uint32_t ndig;
    uint8_t dig_log[kNttMaxDigits], t_log[kNttMaxDigits];   // log2 n_d and log2 T_d
};

template <class F> __device__ __forceinline__ Ufe<F> ntt_pow2t(const void *lo, const void *hi, uint64_t e) {
    const Ufe<F> l = reinterpret_cast<const Ufe<F> *>(lo)[e & ((1u << kNttLoBits) - 1)];
    if (!hi) return l;
    return umul_std<F>(l, fe_load<F>(hi, e >> kNttLoBits));      // below 2 p: a valid multiplier
}

template <class F> __device__ __forceinline__ uint32_t ntt_brev(uint32_t v, uint32_t bits) { return bits ? __brev(v) >> (32 - bits) : 0u; }

// One pass over one tile.  LDS: the tile as [point][column] (columns adjacent), then the P / 2 twiddles, one word after the other.
template <class F, bool LAST> __global__ void __launch_bounds__(kNttBlock) ntt_pass_kernel(NttPassArgs a) {
    extern __shared__ uint4 ntt_smem[];
    constexpr int L = UParams<F>::L;
    const uint32_t tid = threadIdx.x, log_p = a.log_p, log_c = a.log_c;
    const uint32_t P = 1u << log_p, C = 1u << log_c, elems = P << log_c;
    Fe<F> *tile = reinterpret_cast<Fe<F> *>(ntt_smem);
    uint32_t *twl = reinterpret_cast<uint32_t *>(tile + elems);
    const uint64_t w = blockIdx.x;

    for (uint32_t j = tid; j < P / 2; j += kNttBlock) {
        const Ufe<F> t = reinterpret_cast<const Ufe<F> *>(a.tw)[(size_t)j << (a.tw_log - log_p)];
#pragma unroll
        for (int k = 0; k < L; k++) twl[j * L + k] = t.l[k];
    }

    // ---- load: point p of the transform goes to row brev(p) ----
    uint64_t base, lo0 = 0, out_base = 0;
    if (!LAST) {
        const uint32_t lg = a.log_s - log_c;
        lo0 = (w & (((uint64_t)1 << lg) - 1)) << log_c;
        base = ((w >> lg) << (log_p + a.log_s)) + lo0;
        for (uint32_t idx = tid; idx < elems; idx += kNttBlock) {        // in LDS order: the reversal is on the global side, a line per row either way
            const uint32_t c = idx & (C - 1), p = ntt_brev<F>(idx >> log_c, log_p);
            const uint64_t addr = base + ((uint64_t)p << a.log_s) + c;
            Fe<F> x = addr < a.src_len ? fe_load<F>(a.src, addr) : fe_zero<F>();
            if (a.scale_mode == 1) x = fe_mul_u_pre<F>(ntt_pow2t<F>(a.scale_lo, a.scale_hi, addr & a.scale_mask), x);
            tile[idx] = x;
        }
    } else {
        const uint32_t lg = a.log_k0 - log_c, log_r0 = a.log_n - a.log_k0 - log_p;
        const uint64_t g = w & (((uint64_t)1 << lg) - 1);
        uint64_t rest = w >> lg;
        base = rest << log_p;
        out_base = g << log_c;
        for (uint32_t d = a.ndig - 1; d-- > 1;) {                        // digits D - 2 .. 1 of the row, the last one lowest
            out_base += (rest & (((uint64_t)1 << a.dig_log[d]) - 1)) << a.t_log[d];
            rest >>= a.dig_log[d];
        }
        for (uint32_t idx = tid; idx < elems; idx += kNttBlock) {        // along the rows: contiguous in memory
            const uint32_t p = idx & (P - 1), c = idx >> log_p;
            const uint64_t addr = ((((g << log_c) + c) << log_r0) << log_p) + base + p;
            Fe<F> x = addr < a.src_len ? fe_load<F>(a.src, addr) : fe_zero<F>();
            if (a.scale_mode == 1) x = fe_mul_u_pre<F>(ntt_pow2t<F>(a.scale_lo, a.scale_hi, addr & a.scale_mask), x);
            tile[(ntt_brev<F>(p, log_p) << log_c) + c] = x;
        }
    }
    __syncthreads();

    // ---- log_p levels of butterflies (a, b) -> (a + w b, a - w b); level 0's twiddle is 1 ----
    for (uint32_t lev = 0; lev < log_p; lev++) {
        const uint32_t h = 1u << lev;
        for (uint32_t j = tid; j < elems / 2; j += kNttBlock) {
            const uint32_t c = j & (C - 1), q = j >> log_c, r = q & (h - 1);
            const uint32_t i0 = ((((q >> lev) << (lev + 1)) + r) << log_c) + c, i1 = i0 + (h << log_c);
            const Fe<F> x = tile[i0];
            Fe<F> y = tile[i1];
            if (lev) {
                Ufe<F> t;
                const uint32_t *tp = twl + (r << (log_p - 1 - lev)) * L;
#pragma unroll
                for (int k = 0; k < L; k++) t.l[k] = tp[k];
                y = fe_mul_u_pre<F>(t, y);
            }
            tile[i0] = fe_add<F>(x, y);
            tile[i1] = fe_sub<F>(x, y);
        }
        __syncthreads();
    }

    // ---- store ----
    for (uint32_t idx = tid; idx < elems; idx += kNttBlock) {
        const uint32_t c = idx & (C - 1), k = idx >> log_c;
        Fe<F> x = tile[idx];
        if (!LAST) {
            if (a.twist_lo) x = fe_mul_u_pre<F>(ntt_pow2t<F>(a.twist_lo, a.twist_hi, ((uint64_t)k * (lo0 + c)) << a.log_t), x);
            fe_store<F>(a.dst, base + ((uint64_t)k << a.log_s) + c, x);
        } else {
            const uint64_t addr = out_base + c + ((uint64_t)k << a.log_t);
            if (a.scale_mode == 2) x = fe_mul_u_pre<F>(ntt_pow2t<F>(a.scale_lo, a.scale_hi, addr & a.scale_mask), x);
            fe_store<F>(a.dst, addr, x);
        }
    }
}

}  // namespace zk
