// zkmle_grind.hip -- the proof-of-work step of the FRI transcripts (include/zkmle.h "Proof-of-work grinding"): the driver of the GPU nonce
// search (grind.cuh) and the C ABI of the step on its own.  The host search and the verifier's step are grind_host.h's.
#include "grind.cuh"
#include "grind_host.h"
#include "host_util.h"

using namespace zk;
using namespace zk::host;

namespace {

thread_local zk_grind_stats g_grind_stats{};

int bits_check(uint32_t bits) { return bits >= 1 && bits <= ZK_FRI_GRIND_MAX_BITS ? ZK_OK : ZK_E_ARG; }
// 2^22 candidates a launch (a millisecond or so of hashing), a quarter of the expected search where that is more
unsigned default_log_batch(uint32_t bits) { return bits <= 24 ? 22 : bits - 2; }

}  // namespace

namespace zk {

// Ranges of 2^log_batch candidates in ascending order, one launch and one read of the result word each: the first range with a hit holds
// the smallest w >= start.  The hard cap is checked between launches, so a kernel that never reports a hit ends the loop too.  2^64 - 1 is
// the word's "no hit yet" and is not searched.
int transcript_grind(Transcript &tr, uint32_t bits, uint64_t start, uint32_t log_batch, uint64_t *nonce) {
    if (!nonce || (log_batch != 0 && (log_batch < 8 || log_batch > 30))) return ZK_E_ARG;
    ZK_TRY(bits_check(bits));
    ZK_TRY(require_device());
    Transcript tagged = tr;
    grind_tag(tagged, bits);
    GrindSponge sp;
    tagged.sponge().export_state(sp.a, &sp.fill);
    const bool two = sp.fill >= 128;
    if (!two) {                                              // the pad of a block that also holds the whole nonce
        sp.a[(sp.fill + 8) / 8] ^= (uint64_t)0x01 << (8 * ((sp.fill + 8) % 8));
        sp.a[16] ^= (uint64_t)0x80 << 56;
    }
    constexpr uint64_t kNone = ~(uint64_t)0;
    const uint64_t batch = (uint64_t)1 << (log_batch ? log_batch : default_log_batch(bits)), cap = grind_cap(bits);
    DevBuf best;
    ZK_TRY(best.alloc(8));
    ZK_HIP(hipMemsetAsync(best.p, 0xFF, 8, cur_stream()));
    Events ev;
    size_t e0, e1;
    ZK_TRY(ev.mark(&e0));
    zk_grind_stats st{};
    uint64_t covered = 0, found = kNone;
    while (covered < cap && start + covered >= start && start + covered != kNone) {
        const uint64_t base = start + covered, room = kNone - base, count = batch < room ? batch : room;
        const uint64_t want = (count + kGrindBlock - 1) / kGrindBlock;
        const unsigned blocks = (unsigned)(want < kGrindMaxBlocks ? want : kGrindMaxBlocks);
        if (two) fri_grind_kernel<true><<<blocks, kGrindBlock, 0, cur_stream()>>>(sp, base, count, bits, (unsigned long long *)best.p);
        else fri_grind_kernel<false><<<blocks, kGrindBlock, 0, cur_stream()>>>(sp, base, count, bits, (unsigned long long *)best.p);
        ZK_HIP(hipGetLastError());
        ZK_HIP(zk::memcpy_on_stream(&found, best.p, 8, hipMemcpyDeviceToHost));
        st.launches++;
        covered += count;
        if (found != kNone || count < batch) break;
    }
    ZK_TRY(ev.mark(&e1));
    ZK_HIP(hipEventSynchronize(ev.ev[e1]));
    st.ms = ev.ms(e0, e1);
    if (found != kNone && found - start >= cap) found = kNone;   // a launch reaches past the cap where the batch is the larger: the host search's answer
    st.candidates = found != kNone ? found - start + 1 : covered;
    g_grind_stats = st;
    if (found == kNone) return ZK_E_RANGE;
    if (found < start || !grind_finish(tagged, bits, found)) {   // one hash on the host: a nonce the kernel made up goes no further
        set_last_error("zk_transcript_grind: the device's nonce fails the host's check");
        return ZK_E_HIP;
    }
    tr = tagged;
    *nonce = found;
    return ZK_OK;
}

}  // namespace zk

extern "C" {

int zk_transcript_grind(zk_transcript *t, uint32_t bits, uint64_t start, uint32_t log_batch, uint64_t *nonce) {
    if (!t) return ZK_E_ARG;
    return transcript_grind(t->t, bits, start, log_batch, nonce);
}

int zk_host_transcript_grind(zk_transcript *t, uint32_t bits, uint64_t start, uint64_t max_tries, uint64_t *nonce) {
    if (!t || !nonce) return ZK_E_ARG;
    ZK_TRY(bits_check(bits));
    return grind_search_host(t->t, bits, start, max_tries, nonce) ? ZK_OK : ZK_E_RANGE;
}

int zk_transcript_grind_check(zk_transcript *t, uint32_t bits, uint64_t nonce, int *ok) {
    if (!t || !ok) return ZK_E_ARG;
    ZK_TRY(bits_check(bits));
    *ok = grind_check(t->t, bits, nonce) ? 1 : 0;
    return ZK_OK;
}

int zk_transcript_grind_last_stats(zk_grind_stats *out) {
    if (!out) return ZK_E_ARG;
    *out = g_grind_stats;
    return ZK_OK;
}

}  // extern "C"
