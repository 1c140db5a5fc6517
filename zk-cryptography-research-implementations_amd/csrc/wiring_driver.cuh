// wiring_driver.cuh -- what the drivers of the wiring's sumcheck (zkmle_wiring.hip) and of the Plonk proof (zkmle_plonk.hip) share: the room for a
// pass's seven sums, the holder of the three helper commitments, and the launch of the helper tables' kernel.  Library-internal; included by .hip
// files only.
#pragma once
#include "fri_host.h"
#include "wiring.cuh"
#include "wiring_host.h"

namespace zk {
namespace host {

// room for the workgroups' partial sums and the seven sums behind them
struct SumsBuf {
    DevBuf buf;
    void *sums = nullptr;
    int alloc(size_t esz) {
        const size_t cap = (size_t)reduce_block_cap();
        ZK_TRY(buf.alloc((kWiringSums * cap + kWiringSums) * esz));
        sums = (char *)buf.p + kWiringSums * cap * esz;
        return ZK_OK;
    }
};

// the prover's helper commitments: freed with the call
struct CommitHolder {
    zk_fri_commitment *cm[kWiringWires] = {};
    ~CommitHolder() { for (zk_fri_commitment *c : cm) zk_fri_commitment_free(c); }
};

// H (n entries, device) of one wire with id[x] = first + x.  Launches only.
template <class F> int launch_fractions(const void *W, const void *S, void *H, size_t n, uint64_t first, const Fe<F> &beta, const Fe<F> &gamma) {
    const size_t per = (size_t)kWiringBatch * kPcsBlock;
    const Fe<F> gfirst = fe_mul<F>(gamma, fe_from_u64<F>(first)), g256 = fe_mul<F>(gamma, fe_from_u64<F>((uint64_t)kPcsBlock));
    wiring_fractions_kernel<F><<<(unsigned)((n + per - 1) / per), kPcsBlock, 0, cur_stream()>>>(W, S, H, n, beta, gamma, gfirst, g256);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

}  // namespace host
}  // namespace zk
