// host_util.h -- small host-side pieces that several translation units had a copy each of: RAII holders of pool memory and events, loaders and
// range checks of field elements in the C ABI's limb layout.  Library-internal; included by .hip files only.
#pragma once
#include <string.h>

#include <vector>

#include "context.h"
#include "fields.cuh"

namespace zk {
namespace host {

struct DevBuf {   // RAII block of the caching pool
    void *p = nullptr;
    ~DevBuf() { pool_free(p); }
    int alloc(size_t bytes) { return pool_alloc(bytes, &p); }
};
struct TableHolder {   // tables of the pool, freed with the proof
    std::vector<zk_table *> v;
    ~TableHolder() { for (zk_table *t : v) zk_table_free(t); }
    int alloc(int field, size_t len, zk_table **out) {
        ZK_TRY(table_alloc_pooled(field, len, out));
        v.push_back(*out);
        return ZK_OK;
    }
};
// HIP events along the calling thread's stream; elapsed times are read after the proof's last synchronisation
struct Events {
    std::vector<hipEvent_t> ev;
    ~Events() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    int mark(size_t *id) {
        hipEvent_t e;
        ZK_HIP(hipEventCreate(&e));
        ev.push_back(e);
        ZK_HIP(hipEventRecord(e, cur_stream()));
        *id = ev.size() - 1;
        return ZK_OK;
    }
    float ms(size_t a, size_t b) const {
        float v = 0.f;
        return hipEventElapsedTime(&v, ev[a], ev[b]) == hipSuccess ? v : 0.f;
    }
    float since(size_t a) const { return ms(a, ev.size() - 1); }   // up to the latest mark
};

template <class F> Fe<F> load_host(const uint64_t *src) {
    Fe<F> e;
    memcpy(e.l, src, sizeof(uint32_t) * F::N);
    return e;
}
template <class F> void store_host(uint64_t *dst, const Fe<F> &e) { memcpy(dst, e.l, sizeof(uint32_t) * F::N); }
template <class F> Fe<F> fe_pow(Fe<F> b, uint64_t e) {
    Fe<F> acc = fe_one<F>();
    for (; e; e >>= 1) {
        if (e & 1) acc = fe_mul<F>(acc, b);
        b = fe_sqr<F>(b);
    }
    return acc;
}
template <class F> bool is_reduced(const uint64_t *el) {
    const Fe<F> x = load_host<F>(el);
    for (int i = F::N - 1; i >= 0; i--)
        if (x.l[i] != F::p(i)) return x.l[i] < F::p(i);
    return false;
}
inline bool all_reduced(int field, const uint64_t *els, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!(field == ZK_FR381 ? is_reduced<Fr381>(els + i * 4) : is_reduced<Bn254Fr>(els + i * 4))) return false;
    return true;
}
inline bool is_zero_element(int field, const uint64_t *x) {
    uint64_t v = 0;
    for (int k = 0; k < field_limbs64(field); k++) v |= x[k];
    return v == 0;
}
inline void put_be32(uint8_t *out, uint32_t v) {
    for (int k = 0; k < 4; k++) out[k] = (uint8_t)(v >> (24 - 8 * k));
}

}  // namespace host
}  // namespace zk
