// adsb_score_rx.hip -- device-side scoring of a pass whose buffers belong to several receivers, each with an ICAO filter
// of its own (adsb_set_receiver_scoring; adsb_device.h: RxScoreDev has the argument).  Kernels of their own behind the
// records kernel of such a pass, on the score stream: the scans, the match, the records kernel and the plain k_score /
// k_emit (adsb_aux.hip) are what they always were.
//   k_rx_adders   every trial that can add (clean DF11 IID 0 / DF17) into the first-adder table keyed (receiver, value)
//   k_score_rx    adsb_score_dev.h's score_body with RxFilter: "is (r, v) in the keyed set, or did an earlier trial of
//                 r's add v"
//   k_emit_rx     adsb_score_dev.h's emit_body with RxCommit: additions leave as (value, receiver) pairs and go into the
//                 keyed set; both first-adder tables (the plain one the records kernel filled, and the keyed one) are left
//                 empty; the set an icao_flush retired is cleared; an insertion that ran out of probes makes the summary
//                 say scored = 0
//   k_rx_set_fill / k_rx_set_lookup   the keyed set rebuilt from the host's filters; the self-test of its two functions
// Like k_score / k_emit they run beside the next pass's persistent scan: issue priority raised, the messages staged and
// stored as consecutive 8-byte system-scope words, agent-scope accesses and no fence anywhere.
#include <algorithm>

#include "../../include/adsb_hip.h"
#include "adsb_dev_common.h"
#include "adsb_scan_geometry.h"
#include "adsb_tail_dev.h"
#include "adsb_fix_dev.h"
#include "adsb_score_dev.h"

namespace adsb {

namespace {

__device__ __forceinline__ unsigned long long rx_key(uint32_t r, uint32_t v) { return (unsigned long long)r << 24 | v; }

// the receiver of trial i's buffer (pos = buffer << 24 | j; a buffer index past the map would be the records kernel's
// fault: it reads the last entry, never past the array)
__device__ __forceinline__ uint32_t rx_of(const ScanParams &p, const RxScoreDev &x, unsigned long long pos)
{
    return x.rx_map[min((uint32_t)(pos >> 24), p.n_chunks - 1u)];
}

// ---- the keyed exact set: insert and lookup, both at most probe_max slots from the key's home ----
__device__ __forceinline__ bool rx_set_insert(unsigned long long *set, uint32_t lg, uint32_t probe_max, unsigned long long key)
{
    const uint32_t mask = (1u << lg) - 1u;
    uint32_t h = rx_set_home(key, lg);
    for (uint32_t t = 0; t < probe_max; t++) {
        const unsigned long long cur = atomicCAS(&set[h], ~0ull, key);
        if (cur == ~0ull || cur == key) return true;   // claimed an empty slot, or the key was there
        h = (h + 1u) & mask;
    }
    return false;
}

// (nothing is ever deleted and an insertion never goes further than probe_max slots: neither does the lookup)
__device__ __forceinline__ bool rx_set_has(const unsigned long long *set, uint32_t lg, uint32_t probe_max, unsigned long long key)
{
    const uint32_t mask = (1u << lg) - 1u;
    uint32_t h = rx_set_home(key, lg);
    for (uint32_t t = 0; t < probe_max; t++) {
        const unsigned long long cur = __hip_atomic_load(&set[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == key) return true;
        if (cur == ~0ull) return false;
        h = (h + 1u) & mask;
    }
    return false;
}

// ---- the keyed first-adder table: key << 24 | index, atomic-min per key (14 + 24 + 24 bits: never ~0) ----
// the slot the key sits in, or 0xFFFFFFFF: out of probes
__device__ __forceinline__ uint32_t rx_first_insert(const RxScoreDev &x, unsigned long long key, uint32_t idx)
{
    const unsigned long long mine = key << 24 | idx;
    const uint32_t mask = (1u << x.first_lg) - 1u;
    uint32_t h = rx_set_home(key, x.first_lg);
    for (uint32_t t = 0; t < kRxProbeMax; t++) {
        const unsigned long long cur = atomicCAS(&x.first[h], ~0ull, mine);
        if (cur == ~0ull) return h;
        if ((cur >> 24) == key) {
            atomicMin(&x.first[h], mine);
            return h;
        }
        h = (h + 1u) & mask;
    }
    return 0xFFFFFFFFu;
}

// index of the first adder of the key in this pass, or 0xFFFFFFFF
__device__ __forceinline__ uint32_t rx_first(const RxScoreDev &x, unsigned long long key)
{
    const uint32_t mask = (1u << x.first_lg) - 1u;
    uint32_t h = rx_set_home(key, x.first_lg);
    for (uint32_t t = 0; t < kRxProbeMax; t++) {
        const unsigned long long cur = __hip_atomic_load(&x.first[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == ~0ull) return 0xFFFFFFFFu;
        if ((cur >> 24) == key) return (uint32_t)cur & 0xFFFFFFu;
        h = (h + 1u) & mask;
    }
    return 0xFFFFFFFFu;
}

// "v is in receiver r's filter when trial i is scored" (src/icao_filter.rs:65-97; address 0 always is)
struct RxFilter {
    const RxScoreDev &x;
    uint32_t r;
    __device__ __forceinline__ bool operator()(uint32_t v, uint32_t i) const
    {
        if (v == 0) return true;
        const unsigned long long key = rx_key(r, v);
        if (rx_set_has(x.set, x.set_lg, x.probe_max, key)) return true;
        return rx_first(x, key) < i;
    }
};

// k_rx_adders: one thread per hit.  The records kernel has classified every trial (ScoreDev::si) and filled the plain
// first-adder table, which a receivers pass does not consult; the keyed one is filled here, before any trial is scored.
__global__ __launch_bounds__(256) void k_rx_adders(ScanParams p, RxScoreDev x)
{
    TAIL_PRIO();
    const ScoreDev &sd = p.score;
    const uint32_t n = sd.state->n;
    bool failed = false;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t w = sd.si[i], v = w & 0xFFFFFFu, kind = w >> 24;
        uint32_t slot = 0xFFFFFFFFu;
        if (kind == kSkDf11Iid0 || kind == kSkDf17) {
            slot = rx_first_insert(x, rx_key(rx_of(p, x, sd.pos[i]), v), i);
            failed = failed || slot == 0xFFFFFFFFu;
        }
        x.rx_slot[i] = slot;
    }
    if (failed) atomicOr(&sd.state->reserved, 1u);
}

// What k_emit_rx does with an addition (adsb_score_dev.h: emit_body): its receiver goes out beside the value, and the pair
// into the keyed set, which can run out of probes; the keyed first-adder table is left empty like the plain one.
struct RxCommit {
    const ScanParams &p;
    const RxScoreDev &x;
    // (every k_score_rx that read the retired set is ahead of this kernel on the stream)
    __device__ __forceinline__ void clear_retired(uint32_t k0, uint32_t step) const
    {
        if (!x.set_retired) return;
        uint4 *w = (uint4 *)x.set_retired;
        const uint32_t quads = 1u << (x.retired_lg - 1u);   // two 8-byte slots per 16 bytes
        for (uint32_t k = k0; k < quads; k += step)
            w[k] = make_uint4(~0u, ~0u, ~0u, ~0u);
    }
    __device__ __forceinline__ bool commit(uint32_t at, uint32_t i, uint32_t v, bool keep) const
    {
        const uint32_t rcv = rx_of(p, x, p.score.pos[i]);
        host_store32(x.out_add_rx + at, rcv);
        return !keep || rx_set_insert(x.set, x.set_lg, x.probe_max, rx_key(rcv, v));
    }
    __device__ __forceinline__ void forget(uint32_t i) const
    {
        const uint32_t rs = x.rx_slot[i];
        if (rs != 0xFFFFFFFFu) x.first[rs] = ~0ull;
    }
    // (k_rx_adders' insertions and this kernel's)
    __device__ __forceinline__ uint32_t out_of_probes() const { return atomicOr(&p.score.state->reserved, 0u) ? 1u : 0u; }
    __device__ __forceinline__ void reset_state() const { p.score.state->reserved = 0; }
};

// k_score_rx, k_emit_rx: the shared bodies (adsb_score_dev.h) with the filter of the trial's own receiver
__global__ __launch_bounds__(256) void k_score_rx(ScanParams p, RxScoreDev x)
{
    TAIL_PRIO();
    score_body(p, [&](uint64_t pos) { return RxFilter{x, rx_of(p, x, pos)}; }, blockDim.x);
}

__global__ __launch_bounds__(256) void k_emit_rx(ScanParams p, RxScoreDev x)
{
    TAIL_PRIO();
    emit_body(p, RxCommit{p, x}, blockDim.x);
}

__global__ __launch_bounds__(256) void k_rx_set_fill(const unsigned long long *__restrict__ keys, uint32_t n, unsigned long long *set,
                                                     uint32_t lg, uint32_t probe_max, uint32_t *failed)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !rx_set_insert(set, lg, probe_max, keys[i])) atomicAdd(failed, 1u);
}

__global__ __launch_bounds__(256) void k_rx_set_lookup(const unsigned long long *__restrict__ queries, uint32_t n,
                                                       const unsigned long long *set, uint32_t lg, uint32_t probe_max,
                                                       uint32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rx_set_has(set, lg, probe_max, queries[i]) ? 1u : 0u;
}

inline int hip_ok(hipError_t e) { return e == hipSuccess ? 0 : (int)e; }
inline void hip_clear() { (void)hipGetLastError(); }

}  // namespace

int launch_score_rx(const ScanParams &p, const RxScoreDev &x, void *stream)
{
    hip_clear();
    if (!p.score.si || !x.set || !x.first || !x.rx_map || p.n_chunks == 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rx_adders, dim3(kScoreBlocks), dim3(256), 0, (hipStream_t)stream, p, x);
    hipLaunchKernelGGL(k_score_rx, dim3(kScoreBlocks), dim3(256), 0, (hipStream_t)stream, p, x);
    hipLaunchKernelGGL(k_emit_rx, dim3(kScoreBlocks), dim3(256), 0, (hipStream_t)stream, p, x);
    return hip_ok(hipGetLastError());
}

int launch_rx_set_fill(const unsigned long long *d_keys, uint32_t n, unsigned long long *set, uint32_t set_lg, uint32_t probe_max,
                       uint32_t *d_failed, void *stream)
{
    hip_clear();
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_rx_set_fill, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_keys, n, set, set_lg, probe_max, d_failed);
    return hip_ok(hipGetLastError());
}

int launch_rx_set_lookup(const unsigned long long *d_queries, uint32_t n, const unsigned long long *set, uint32_t set_lg,
                         uint32_t probe_max, uint32_t *d_out, void *stream)
{
    hip_clear();
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_rx_set_lookup, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_queries, n, set, set_lg, probe_max, d_out);
    return hip_ok(hipGetLastError());
}

}  // namespace adsb
