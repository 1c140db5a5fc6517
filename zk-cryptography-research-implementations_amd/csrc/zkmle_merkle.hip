// zkmle_merkle.hip -- C ABI of the Keccak-256 Merkle commitment of a table (merkle.cuh): the root alone (what the committed provers bind
// their transcript to), the whole tree resident in HBM with batched openings, and the host-side path check.  Extension: the reference
// leaves `merkle_tree/` empty; the bytes are defined in include/zkmle.h.
#include <string.h>

#include <vector>

#include "host_util.h"
#include "merkle_columns.cuh"
#include "transcript.h"

using namespace zk;
using host::DevBuf;

struct zk_merkle_tree {
    int field;
    size_t len;             // the LEAVES: the table's length, or that >> log_group of a tree with grouped leaves
    unsigned depth;
    uint64_t *levels;       // 2 len - 1 digests: level l at digest offset 2 len - (2 len >> l), the root last
};

namespace {

inline unsigned merkle_grid(size_t work) {
    size_t b = (work + kMerkleBlock - 1) / kMerkleBlock;
    return (unsigned)(b < 1 ? 1 : b > ((size_t)1 << 20) ? (size_t)1 << 20 : b);
}

// `lv` holds n digests (a power of two); the levels above are written right behind it, the root at lv[2 n - 2]
int hash_up(uint64_t *lv, size_t n) {
    while (n > kMerkleFinish) {
        merkle_node_kernel<<<merkle_grid(n / 2), kMerkleBlock, 0, cur_stream()>>>(lv, n / 2, lv + 4 * n);
        ZK_HIP(hipGetLastError());
        lv += 4 * n;
        n /= 2;
    }
    if (n >= 2) {
        merkle_finish_kernel<<<1, kMerkleBlock, 0, cur_stream()>>>(lv, (unsigned)n);
        ZK_HIP(hipGetLastError());
    }
    return ZK_OK;
}

template <class F> int launch_leaves(const zk_table *t, uint64_t *out) {
    merkle_leaf_kernel<F><<<merkle_grid(t->len), kMerkleBlock, 0, cur_stream()>>>(t->dptr, t->len, out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}
// the len >> lg grouped leaves (lg = 1 or 2) of a table of 32-byte elements
template <class F> int launch_leaves_grouped(const zk_table *t, unsigned lg, uint64_t *out) {
    if constexpr (F::N == 8) {
        const size_t part = t->len >> lg;
        if (lg == 1) merkle_leaf_group_kernel<F, 1><<<merkle_grid(part), kMerkleBlock, 0, cur_stream()>>>(t->dptr, part, out);
        else merkle_leaf_group_kernel<F, 2><<<merkle_grid(part), kMerkleBlock, 0, cur_stream()>>>(t->dptr, part, out);
        ZK_HIP(hipGetLastError());
        return ZK_OK;
    } else {
        return ZK_E_ARG;
    }
}
// the statuses of a grouped tree of `t` that need no device
int grouped_check(const zk_table *t, uint32_t lg) {
    if (!t || lg > 2 || field_limbs64(t->field) != 4 || t->len < ((size_t)1 << lg)) return ZK_E_ARG;
    return is_pow2(t->len) ? ZK_OK : ZK_E_NOT_POW2;
}
// Root-only mode: build mode on ONE scratch block of the caching pool, 2 len - 1 digests (64 B x len; cached by the calling thread's pool
// after the call like every per-call scratch).  Nothing but the root leaves the device.
template <class F> int root_only(const zk_table *t, uint8_t root32[32]) {
    const size_t n = t->len;
    DevBuf buf;
    ZK_TRY(buf.alloc((2 * n - 1) * 32));
    uint64_t *lv = (uint64_t *)buf.p;
    ZK_TRY(launch_leaves<F>(t, lv));
    ZK_TRY(hash_up(lv, n));
    ZK_HIP(zk::memcpy_on_stream(root32, lv + 4 * (2 * n - 2), 32, hipMemcpyDeviceToHost));   // the call's one synchronisation
    return ZK_OK;
}

int root_only_grouped(const zk_table *t, unsigned lg, uint8_t root32[32]) {
    const size_t n = t->len >> lg;
    DevBuf buf;
    ZK_TRY(buf.alloc((2 * n - 1) * 32));
    ZK_TRY(merkle_levels_grouped_device(t, lg, (uint64_t *)buf.p));
    ZK_HIP(zk::memcpy_on_stream(root32, (uint64_t *)buf.p + 4 * (2 * n - 2), 32, hipMemcpyDeviceToHost));   // the call's one synchronisation
    return ZK_OK;
}

// leaf and node hashes on the host (zk_merkle_verify; Keccak256 of transcript.h, pinned by the reference KATs)
template <class F> void host_leaf(const uint64_t *element, uint8_t out[32]) {
    uint8_t msg[1 + 4 * F::N];
    Fe<F> e;
    memcpy(e.l, element, 4 * F::N);
    msg[0] = 0x00;
    host_to_bytes_be<F>(e, msg + 1);
    Keccak256 h;
    h.update(msg, sizeof msg);
    h.finalize_copy(out);
}
// the grouped leaf of 2^lg elements of 32 bytes; false: one of them is not reduced
template <class F> bool host_leaf_grouped(const uint64_t *elements, unsigned lg, uint8_t out[32]) {
    if constexpr (F::N == 8) {
        uint8_t msg[1 + 4 * 32];
        msg[0] = 0x00;
        for (size_t g = 0; g < (size_t)1 << lg; g++) {
            if (!host::is_reduced<F>(elements + 4 * g)) return false;
            host_to_bytes_be<F>(host::load_host<F>(elements + 4 * g), msg + 1 + 32 * g);
        }
        Keccak256 h;
        h.update(msg, 1 + ((size_t)32 << lg));
        h.finalize_copy(out);
        return true;
    } else {
        return false;
    }
}
// ---- several columns under one tree (merkle_columns.cuh) ---------------------------------------------------------------------------
// the leaf launch's grid: a block per 256 leaves, at most 2^14 blocks (64 a CU), the stride loop takes the rest.  ZK_MERKLE_COLUMNS_BLOCKS
// (read once, here only) lowers the cap, so that a test can put a small tree on the loop's second trip
inline unsigned merkle_columns_grid(size_t part) {
    static const size_t cap = [] {
        const char *e = getenv("ZK_MERKLE_COLUMNS_BLOCKS");
        const long v = e ? atol(e) : 0;
        return (size_t)(v >= 1 && v < (1 << 14) ? v : 1 << 14);
    }();
    const size_t b = (part + kMerkleBlock - 1) / kMerkleBlock;
    return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}
template <class F> int launch_leaves_columns(const zk_table *const *tables, uint32_t k, uint64_t *out) {
    MerkleColumnsArgs a{};
    for (uint32_t c = 0; c < k; c++) a.t[c] = tables[c]->dptr;
    a.k = (int)k;
    const size_t part = tables[0]->len >> 2;
    merkle_leaf_columns_kernel<F><<<merkle_columns_grid(part), kMerkleBlock, 0, cur_stream()>>>(a, part, out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}
int root_only_columns(const zk_table *const *tables, uint32_t k, uint8_t root32[32]) {
    const size_t n = tables[0]->len >> 2;
    DevBuf buf;
    ZK_TRY(buf.alloc((2 * n - 1) * 32));
    ZK_TRY(merkle_levels_columns_device(tables, k, (uint64_t *)buf.p));
    ZK_HIP(zk::memcpy_on_stream(root32, (uint64_t *)buf.p + 4 * (2 * n - 2), 32, hipMemcpyDeviceToHost));   // the call's one synchronisation
    return ZK_OK;
}
// the leaf over k columns: `elements` = 4 k of them in the leaf's order; false: one of them is not reduced
template <class F> bool host_leaf_columns(const uint64_t *elements, uint32_t k, uint8_t out[32]) {
    if constexpr (F::N == 8) {
        std::vector<uint8_t> msg(1 + (size_t)128 * k);
        msg[0] = 0x00;
        for (size_t g = 0; g < (size_t)4 * k; g++) {
            if (!host::is_reduced<F>(elements + 4 * g)) return false;
            host_to_bytes_be<F>(host::load_host<F>(elements + 4 * g), msg.data() + 1 + 32 * g);
        }
        Keccak256 h;
        h.update(msg.data(), msg.size());
        h.finalize_copy(out);
        return true;
    } else {
        return false;
    }
}

void host_node(const uint8_t *l, const uint8_t *r, uint8_t out[32]) {
    uint8_t msg[65];
    msg[0] = 0x01;
    memcpy(msg + 1, l, 32);
    memcpy(msg + 33, r, 32);
    Keccak256 h;
    h.update(msg, sizeof msg);
    h.finalize_copy(out);
}

}  // namespace

namespace zk {
int merkle_root_device(const zk_table *t, uint8_t root32[32]) {
    if (!t || !root32 || field_limbs64(t->field) < 0) return ZK_E_ARG;
    if (!is_pow2(t->len)) return ZK_E_NOT_POW2;
    ZK_TRY(require_device());
    ZK_DISPATCH_FIELD(t->field, return root_only<F>(t, root32));
    return ZK_OK;
}
int merkle_levels_device(const zk_table *t, uint64_t *levels) {
    ZK_DISPATCH_FIELD(t->field, ZK_TRY(launch_leaves<F>(t, levels)));
    return hash_up(levels, t->len);
}
int merkle_levels_grouped_device(const zk_table *t, unsigned log_group, uint64_t *levels) {
    if (log_group == 0) return merkle_levels_device(t, levels);
    ZK_DISPATCH_FIELD(t->field, ZK_TRY(launch_leaves_grouped<F>(t, log_group, levels)));
    return hash_up(levels, t->len >> log_group);
}
// the statuses of a tree over the k columns `tables` that need no device
int merkle_columns_check(const zk_table *const *tables, uint32_t k, size_t min_len) {
    if (!tables || k < 1 || k > (uint32_t)kMerkleColumnsMax || !tables[0]) return ZK_E_ARG;
    const int field = tables[0]->field;
    if (field != ZK_FR381 && field != ZK_BN254_FR) return ZK_E_ARG;
    for (uint32_t c = 1; c < k; c++)
        if (!tables[c] || tables[c]->field != field) return ZK_E_ARG;
    for (uint32_t c = 0; c < k; c++)
        if (tables[c]->len < min_len) return ZK_E_ARG;
    for (uint32_t c = 1; c < k; c++)
        if (tables[c]->len != tables[0]->len) return ZK_E_LEN_MISMATCH;
    return is_pow2(tables[0]->len) ? ZK_OK : ZK_E_NOT_POW2;
}
int merkle_leaves_columns_device(const zk_table *const *tables, uint32_t k, uint64_t *levels) {
    if (tables[0]->field == ZK_FR381) return launch_leaves_columns<Fr381>(tables, k, levels);
    return launch_leaves_columns<Bn254Fr>(tables, k, levels);
}
int merkle_nodes_device(uint64_t *levels, size_t leaves) { return hash_up(levels, leaves); }
int merkle_levels_columns_device(const zk_table *const *tables, uint32_t k, uint64_t *levels) {
    ZK_TRY(merkle_leaves_columns_device(tables, k, levels));
    return hash_up(levels, tables[0]->len >> 2);
}
}  // namespace zk

extern "C" {

int zk_mle_merkle_root(const zk_table *t, uint8_t root32[32]) { return merkle_root_device(t, root32); }

int zk_merkle_build(const zk_table *t, zk_merkle_tree **out) {
    if (!t || !out || field_limbs64(t->field) < 0) return ZK_E_ARG;
    if (!is_pow2(t->len)) return ZK_E_NOT_POW2;
    ZK_TRY(require_device());
    void *d = nullptr;
    ZK_HIP(hipMalloc(&d, (2 * t->len - 1) * 32));
    zk_merkle_tree *m = new zk_merkle_tree{t->field, t->len, ilog2(t->len), (uint64_t *)d};
    int rc = ZK_OK;
    ZK_DISPATCH_FIELD(t->field, rc = launch_leaves<F>(t, m->levels));
    if (rc == ZK_OK) rc = hash_up(m->levels, m->len);
    if (rc == ZK_OK && hipStreamSynchronize(cur_stream()) != hipSuccess) { set_last_error("zk_merkle_build: the hash kernels failed"); rc = ZK_E_HIP; }
    if (rc != ZK_OK) { zk_merkle_free(m); return rc; }
    *out = m;
    return ZK_OK;
}
int zk_mle_merkle_root_grouped(const zk_table *t, uint32_t log_group, uint8_t root32[32]) {
    if (!root32) return ZK_E_ARG;
    if (log_group == 0) return merkle_root_device(t, root32);
    ZK_TRY(grouped_check(t, log_group));
    ZK_TRY(require_device());
    return root_only_grouped(t, log_group, root32);
}
int zk_merkle_build_grouped(const zk_table *t, uint32_t log_group, zk_merkle_tree **out) {
    if (!out) return ZK_E_ARG;
    if (log_group == 0) return zk_merkle_build(t, out);
    ZK_TRY(grouped_check(t, log_group));
    ZK_TRY(require_device());
    const size_t n = t->len >> log_group;
    void *d = nullptr;
    ZK_HIP(hipMalloc(&d, (2 * n - 1) * 32));
    zk_merkle_tree *m = new zk_merkle_tree{t->field, n, ilog2(n), (uint64_t *)d};
    int rc = merkle_levels_grouped_device(t, log_group, m->levels);
    if (rc == ZK_OK && hipStreamSynchronize(cur_stream()) != hipSuccess) { set_last_error("zk_merkle_build_grouped: the hash kernels failed"); rc = ZK_E_HIP; }
    if (rc != ZK_OK) { zk_merkle_free(m); return rc; }
    *out = m;
    return ZK_OK;
}
int zk_mle_merkle_root_columns(const zk_table *const *tables, uint32_t k, uint8_t root32[32]) {
    if (!root32) return ZK_E_ARG;
    ZK_TRY(merkle_columns_check(tables, k));
    ZK_TRY(require_device());
    return root_only_columns(tables, k, root32);
}
int zk_merkle_build_columns(const zk_table *const *tables, uint32_t k, zk_merkle_tree **out) {
    if (!out) return ZK_E_ARG;
    ZK_TRY(merkle_columns_check(tables, k));
    ZK_TRY(require_device());
    const size_t n = tables[0]->len >> 2;
    void *d = nullptr;
    ZK_HIP(hipMalloc(&d, (2 * n - 1) * 32));
    zk_merkle_tree *m = new zk_merkle_tree{tables[0]->field, n, ilog2(n), (uint64_t *)d};
    int rc = merkle_levels_columns_device(tables, k, m->levels);
    if (rc == ZK_OK && hipStreamSynchronize(cur_stream()) != hipSuccess) { set_last_error("zk_merkle_build_columns: the hash kernels failed"); rc = ZK_E_HIP; }
    if (rc != ZK_OK) { zk_merkle_free(m); return rc; }
    *out = m;
    return ZK_OK;
}
int zk_merkle_free(zk_merkle_tree *m) {
    if (!m) return ZK_OK;
    if (m->levels) (void)hipFree(m->levels);
    delete m;
    return ZK_OK;
}
size_t zk_merkle_depth(const zk_merkle_tree *m) { return m ? m->depth : 0; }
int zk_merkle_root(const zk_merkle_tree *m, uint8_t root32[32]) {
    if (!m || !root32) return ZK_E_ARG;
    ZK_HIP(zk::memcpy_on_stream(root32, m->levels + 4 * (2 * m->len - 2), 32, hipMemcpyDeviceToHost));
    return ZK_OK;
}
int zk_merkle_open(const zk_merkle_tree *m, const size_t *indices, size_t nidx, uint8_t *paths) {
    if (!m || (!indices && nidx) || (!paths && nidx && m->depth)) return ZK_E_ARG;
    for (size_t q = 0; q < nidx; q++)
        if (indices[q] >= m->len) return ZK_E_RANGE;
    if (nidx == 0 || m->depth == 0) return ZK_OK;
    static_assert(sizeof(size_t) == 8, "indices travel as 64-bit words");
    DevBuf idx, out;
    ZK_TRY(idx.alloc(nidx * 8));
    ZK_TRY(out.alloc(nidx * m->depth * 32));
    ZK_HIP(hipMemcpyAsync(idx.p, indices, nidx * 8, hipMemcpyHostToDevice, cur_stream()));
    merkle_open_kernel<<<merkle_grid(nidx * m->depth), kMerkleBlock, 0, cur_stream()>>>(m->levels, m->len, m->depth, (const uint64_t *)idx.p, nidx,
                                                                                     (uint64_t *)out.p);
    ZK_HIP(hipGetLastError());
    ZK_HIP(zk::memcpy_on_stream(paths, out.p, nidx * m->depth * 32, hipMemcpyDeviceToHost));   // one download
    return ZK_OK;
}

int zk_merkle_verify(int field, const uint8_t root32[32], size_t depth, size_t index, const uint64_t *element, const uint8_t *path, int *ok) {
    if (!root32 || !element || (!path && depth) || !ok || field_limbs64(field) < 0) return ZK_E_ARG;
    if (depth >= 64 || (index >> depth) != 0) return ZK_E_RANGE;
    uint8_t cur[32];
    ZK_DISPATCH_FIELD(field, host_leaf<F>(element, cur));
    for (size_t l = 0; l < depth; l++) {                       // the leaf's sibling first
        const uint8_t *sib = path + 32 * l;
        uint8_t nx[32];
        if ((index >> l) & 1) host_node(sib, cur, nx); else host_node(cur, sib, nx);
        memcpy(cur, nx, 32);
    }
    *ok = memcmp(cur, root32, 32) == 0 ? 1 : 0;
    return ZK_OK;
}

int zk_merkle_verify_grouped(int field, const uint8_t root32[32], size_t depth, size_t index, uint32_t log_group, const uint64_t *elements,
                             const uint8_t *path, int *ok) {
    if (!root32 || !elements || (!path && depth) || !ok || log_group > 2 || field_limbs64(field) != 4) return ZK_E_ARG;
    if (depth >= 64 || (index >> depth) != 0) return ZK_E_RANGE;
    uint8_t cur[32];
    bool reduced = false;
    ZK_DISPATCH_FIELD(field, reduced = host_leaf_grouped<F>(elements, log_group, cur));
    *ok = 0;
    if (!reduced) return ZK_OK;
    for (size_t l = 0; l < depth; l++) {                       // the leaf's sibling first
        const uint8_t *sib = path + 32 * l;
        uint8_t nx[32];
        if ((index >> l) & 1) host_node(sib, cur, nx); else host_node(cur, sib, nx);
        memcpy(cur, nx, 32);
    }
    *ok = memcmp(cur, root32, 32) == 0 ? 1 : 0;
    return ZK_OK;
}

int zk_merkle_verify_columns(int field, const uint8_t root32[32], size_t depth, size_t index, uint32_t k, const uint64_t *elements, const uint8_t *path,
                             int *ok) {
    if (!root32 || !elements || (!path && depth) || !ok || k < 1 || k > (uint32_t)kMerkleColumnsMax || (field != ZK_FR381 && field != ZK_BN254_FR)) return ZK_E_ARG;
    if (depth >= 64 || (index >> depth) != 0) return ZK_E_RANGE;
    uint8_t cur[32];
    const bool reduced = field == ZK_FR381 ? host_leaf_columns<Fr381>(elements, k, cur) : host_leaf_columns<Bn254Fr>(elements, k, cur);
    *ok = 0;
    if (!reduced) return ZK_OK;
    for (size_t l = 0; l < depth; l++) {                       // the leaf's sibling first
        const uint8_t *sib = path + 32 * l;
        uint8_t nx[32];
        if ((index >> l) & 1) host_node(sib, cur, nx); else host_node(cur, sib, nx);
        memcpy(cur, nx, 32);
    }
    *ok = memcmp(cur, root32, 32) == 0 ? 1 : 0;
    return ZK_OK;
}

}  // extern "C"
