// lookup_driver.cuh -- what the drivers of the lookup argument (zkmle_lookup.hip) and of the Plonk proof with lookup rows (zkmle_plonk_lookup.hip)
// share: the multiplicity count, the launch of the helper table's two kernels, and the commitment of a helper table with the shape of a given
// one.  Library-internal; included by .hip files only.
#pragma once
#include "fri_host.h"
#include "lookup.cuh"

namespace zk {
namespace host {

constexpr int kLookupMaxLog = 31;                                  // the counts and the slots are 32 bits

inline unsigned lookup_blocks_for(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// the hash table of the table's rows: cap = 2 n slots and the status block, both of the pool
struct LookupSlots {
    DevBuf slots, status;
    size_t cap = 0;
};

// the set-up and the insert pass, what multiplicities_into and zk_lookup_hash_slots both run: the slots all ones, the status zero, then a lane per
// row of T0, T1, T2 (n <= 2^31 entries each).  Launches only.
template <class F> int lookup_insert_rows(const void *T0, const void *T1, const void *T2, size_t n, LookupSlots &h) {
    h.cap = 2 * n;
    ZK_TRY(h.slots.alloc(h.cap * 4));
    ZK_TRY(h.status.alloc(sizeof(LookupStatus)));
    ZK_HIP(hipMemsetAsync(h.slots.p, 0xFF, h.cap * 4, cur_stream()));
    ZK_HIP(hipMemsetAsync(h.status.p, 0, sizeof(LookupStatus), cur_stream()));
    lookup_insert_kernel<F><<<lookup_blocks_for(n), kBlock, 0, cur_stream()>>>(T0, T1, T2, n, (uint32_t *)h.slots.p, h.cap, (LookupStatus *)h.status.p);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

// the status block after the last launch that writes it (a synchronisation): the error word as a status
inline int lookup_status(const LookupSlots &h, LookupStatus &st) {
    ZK_HIP(zk::memcpy_on_stream(&st, h.status.p, sizeof st, hipMemcpyDeviceToHost));
    if (st.error) {
        set_last_error("lookup multiplicities: a probe of the hash table ran through its whole capacity");
        return ZK_E_HIP;
    }
    return ZK_OK;
}

// M (n elements, device) and the miss count from the seven tables A, B, C, qK, T0, T1, T2 of n <= 2^31 entries.  One synchronisation.
template <class F> int multiplicities_into(const void *const *in, size_t n, void *M, uint64_t *misses) {
    LookupSlots h;
    DevBuf counts;
    ZK_TRY(counts.alloc(n * 4));
    ZK_HIP(hipMemsetAsync(counts.p, 0, n * 4, cur_stream()));
    ZK_TRY(lookup_insert_rows<F>(in[4], in[5], in[6], n, h));
    lookup_count_kernel<F><<<lookup_blocks_for(n), kBlock, 0, cur_stream()>>>(in[0], in[1], in[2], in[3], in[4], in[5], in[6], n, (const uint32_t *)h.slots.p, h.cap,
                                                                      (uint32_t *)counts.p, (LookupStatus *)h.status.p);
    ZK_HIP(hipGetLastError());
    lookup_finish_kernel<F><<<lookup_blocks_for(n), kBlock, 0, cur_stream()>>>((const uint32_t *)counts.p, n, M);
    ZK_HIP(hipGetLastError());
    LookupStatus st{};
    ZK_TRY(lookup_status(h, st));
    *misses = st.misses;
    return ZK_OK;
}

// the slots as the insert pass leaves them (2 n words, host) from the three tables T0, T1, T2; nothing is written on an error.  A test hook: two synchronisations.
template <class F> int hash_slots_into(const void *const *T, size_t n, uint32_t *slots) {
    LookupSlots h;
    ZK_TRY(lookup_insert_rows<F>(T[0], T[1], T[2], n, h));
    LookupStatus st{};
    ZK_TRY(lookup_status(h, st));
    ZK_HIP(zk::memcpy_on_stream(slots, h.slots.p, h.cap * 4, hipMemcpyDeviceToHost));
    return ZK_OK;
}

// H (n elements, device) from the eight tables A, B, C, qK, T0, T1, T2, M.  Launches only; the two columns of denominators go back to the pool
// when the call returns (stream-ordered: what reuses them runs after the kernels that read them)
template <class F> int launch_fractions_lookup(const void *const *in, size_t n, void *H, const Fe<F> &beta, const Fe<F> &gamma) {
    constexpr size_t ESZ = sizeof(Fe<F>);
    DevBuf den;
    ZK_TRY(den.alloc(2 * n * ESZ));
    void *DW = den.p, *DT = (char *)den.p + n * ESZ;
    lookup_denominators_kernel<F><<<lookup_blocks_for(n), kBlock, 0, cur_stream()>>>(in[0], in[1], in[2], in[4], in[5], in[6], DW, DT, n, beta, gamma, fe_mul<F>(gamma, gamma));
    ZK_HIP(hipGetLastError());
    const size_t per = (size_t)kLookupBatch * kPcsBlock;
    lookup_fractions_kernel<F><<<(unsigned)((n + per - 1) / per), kPcsBlock, 0, cur_stream()>>>(DW, DT, in[3], in[7], H, n);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

inline int commit_like(const zk_fri_commitment *c0, const zk_table *t, zk_fri_commitment **out) {
    const uint64_t *coset = c0->has_coset ? c0->coset : nullptr;
    return c0->log_group ? zk_fri_commit_grouped(t, c0->b, coset, c0->log_group, out) : zk_fri_commit(t, c0->b, coset, out);
}

}  // namespace host
}  // namespace zk
