// adsb_score_rx.hip -- device-side scoring of a pass whose buffers belong to several receivers, each with an ICAO filter
// of its own (adsb_set_receiver_scoring; adsb_device.h: RxScoreDev has the argument).  Kernels of their own behind the
// records kernel of such a pass, on the score stream: the scans, the match, the records kernel and the plain k_score /
// k_emit (adsb_aux.hip) are what they always were.
//   k_rx_adders   every trial that can add (clean DF11 IID 0 / DF17) into the first-adder table keyed (receiver, value)
//   k_score_rx    k_score with "is (r, v) in the keyed set, or did an earlier trial of r's add v"
//   k_emit_rx     k_emit: additions leave as (value, receiver) pairs and go into the keyed set; both first-adder tables
//                 (the plain one the records kernel filled, and the keyed one) are left empty; the set an icao_flush
//                 retired is cleared; an insertion that ran out of probes makes the summary say scored = 0
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

// k_score_rx: k_score (adsb_aux.hip) with the filter of the trial's own receiver -- the same best-of-five grouping by
// position, the same flag layout, the same repair bits.  The trials of one position are trials of one buffer: one receiver.
__global__ __launch_bounds__(256) void k_score_rx(ScanParams p, RxScoreDev x)
{
    TAIL_PRIO();
    const ScoreDev &sd = p.score;
    const uint32_t n = sd.state->n;
    const uint32_t per = (n + gridDim.x - 1) / gridDim.x;
    const uint32_t first = blockIdx.x * per, last = min(n, first + per);
    uint32_t emits = 0, addc = 0;
    for (uint32_t i = first + threadIdx.x; i < last; i += blockDim.x) {
        const uint64_t pos = sd.pos[i];
        const RxFilter in_filter{x, rx_of(p, x, pos)};
        uint32_t g0 = i;
        while (g0 > 0 && i - g0 < 8 && sd.pos[g0 - 1] == pos) g0--;
        int best = -2, mine = -2;
        uint32_t win = 0xFFFFFFFFu, my_add = 0, my_fix = kFixNoRepair;
        for (uint32_t k = g0; k < n && k < g0 + 16 && sd.pos[k] == pos; k++) {
            uint32_t a, fx = kFixNoRepair;
            const int s = score_trial(sd, k, &a, p.tables, p.fix, &fx, in_filter);
            if (k == i) {
                mine = s;
                my_add = a;
                my_fix = fx;
            }
            if (s > best) {
                best = s;
                win = k;
            }
        }
        const bool emit = win == i && best >= 0;
        // (ScoreDev::flag: a repaired trial's bits ride along above the score, as k_score packs them)
        const uint32_t fa = my_fix & 0x7Fu, fb = (my_fix >> 8) & 0x7Fu;
        sd.flag[i] = (emit ? 1u : 0u) | (my_add ? 2u : 0u) | ((uint32_t)(mine + 3) << 8) | (fa >> 6) << 2 | (fa & 63u) << 19 | fb << 25;
        emits += emit;
        addc += my_add != 0;
    }
    __shared__ uint32_t tot[2];
    if (threadIdx.x < 2) tot[threadIdx.x] = 0;
    __syncthreads();
    if (emits) atomicAdd(&tot[0], emits);
    if (addc) atomicAdd(&tot[1], addc);
    __syncthreads();
    if (threadIdx.x < 2) sd.blk[2 * blockIdx.x + threadIdx.x] = tot[threadIdx.x];
}

// k_emit_rx: the messages and the additions in order (block b writes behind what blocks < b write), the additions
// committed to the keyed set, both first-adder tables left empty, the summary last.
__global__ __launch_bounds__(256) void k_emit_rx(ScanParams p, RxScoreDev x)
{
    TAIL_PRIO();
    const ScoreDev &sd = p.score;
    const uint32_t n = sd.state->n;
    const uint32_t per = (n + gridDim.x - 1) / gridDim.x;
    const uint32_t first = blockIdx.x * per, last = min(n, first + per);
    static_assert(kScoreBlocks == 256, "the block-offset reduction below takes one earlier block per thread");
    __shared__ uint32_t base[2], scan[2][256];
    __shared__ unsigned long long stage[5 * 256];  // this round's messages, 40 bytes each
    __shared__ uint32_t wtot[2][4];
    {
        // what the blocks before this one write: all threads fetch, one reduction (kScoreBlocks == blockDim)
        const uint32_t k = threadIdx.x;
        scan[0][k] = k < blockIdx.x ? sd.blk[2 * k] : 0u;
        scan[1][k] = k < blockIdx.x ? sd.blk[2 * k + 1] : 0u;
        __syncthreads();
        for (uint32_t off = 128; off > 0; off >>= 1) {
            if (k < off) {
                scan[0][k] += scan[0][k + off];
                scan[1][k] += scan[1][k + off];
            }
            __syncthreads();
        }
        if (k < 2) base[k] = scan[k][0];
        __syncthreads();
    }
    // an icao_flush preceded this pass: it scores against the other (empty) set; the one the passes before it used is
    // emptied here, for the flush after this one (every k_score_rx that read it is ahead of this kernel on the stream)
    if (x.set_retired) {
        uint4 *w = (uint4 *)x.set_retired;
        const uint32_t quads = 1u << (x.retired_lg - 1u);   // two 8-byte slots per 16 bytes
        for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < quads; k += gridDim.x * blockDim.x)
            w[k] = make_uint4(~0u, ~0u, ~0u, ~0u);
    }
    adsb_msg *out = (adsb_msg *)sd.out_msgs;
    unsigned long long my_sum = 0;
    bool no_room = false;
    for (uint32_t i0 = first; i0 < last; i0 += blockDim.x) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t f = i < last ? sd.flag[i] : 0u;
        {
            // inclusive scan of the two flags over the block: ballots inside a wave, four wave totals
            const uint32_t ln = threadIdx.x & 63u, wv = threadIdx.x >> 6;
            const unsigned long long m0 = __ballot(f & 1u), m1 = __ballot((f >> 1) & 1u);
            const unsigned long long below = ln == 63u ? ~0ull : ((1ull << (ln + 1u)) - 1ull);
            const uint32_t i0 = (uint32_t)__popcll(m0 & below), i1 = (uint32_t)__popcll(m1 & below);
            if (ln == 0) {
                wtot[0][wv] = (uint32_t)__popcll(m0);
                wtot[1][wv] = (uint32_t)__popcll(m1);
            }
            __syncthreads();
            uint32_t b0w = 0, b1w = 0;
            for (uint32_t k = 0; k < wv; k++) {
                b0w += wtot[0][k];
                b1w += wtot[1][k];
            }
            scan[0][threadIdx.x] = b0w + i0;
            scan[1][threadIdx.x] = b1w + i1;
            __syncthreads();
        }
        if (i < last) {
            const TrialRecord r = sd.rec[i];
            const uint32_t w = sd.si[i], v = w & 0xFFFFFFu, kind = w >> 24;
            if (f & 1u) {
                adsb_msg m;
                for (int k = 0; k < 14; k++) m.msg[k] = r.msg[k];
                m.score = (int32_t)((f >> 8) & 0x7FFu) - 3;
                // a repaired message carries the corrected bytes (k_emit: the bits k_score_rx found are in the flag; the
                // record in memory stays as sliced, for a host that cannot use this result)
                if (m.score == ADSB_SCORE_FIXED_1BIT || m.score == ADSB_SCORE_FIXED_2BIT) {
                    const uint32_t fb = f >> 25, fa = m.score == ADSB_SCORE_FIXED_2BIT ? ((f >> 19) & 63u) | ((f >> 2) & 1u) << 6 : kFixNoBit;
                    unsigned long long lo = 0, hi = 0;   // message bits 0..63, 64..111 (MSB first) to flip
                    for (uint32_t k = 0; k < 2; k++) {
                        const uint32_t bit = k ? fa : fb;
                        if (bit < 64u) lo |= 1ull << (63u - bit);
                        else if (bit < 112u) hi |= 1ull << (127u - bit);
                    }
#pragma unroll
                    for (int k = 0; k < 8; k++) m.msg[k] ^= (uint8_t)(lo >> (56 - 8 * k));
#pragma unroll
                    for (int k = 0; k < 6; k++) m.msg[8 + k] ^= (uint8_t)(hi >> (56 - 8 * k));
                }
                m.len = (r.msg[0] & 0x80) ? ADSB_MODES_LONG_MSG_BYTES : ADSB_MODES_SHORT_MSG_BYTES;
                m.try_phase = (uint8_t)(r.j_tp >> 24);
                m.j = r.j_tp & 0xFFFFFFu;
                m.chunk = r.chunk;
                // demod_2400.rs:191-198: the same three divisions, in this order
                const double signal_power = (double)(r.power & ((1ull << 40) - 1)) / 65535.0 / 65535.0;
                m.signal_level = signal_power / 33.0;
                // staged: the block's messages of this round leave as consecutive 8-byte words from consecutive lanes
                const unsigned long long *mw = (const unsigned long long *)&m;
                unsigned long long *sw = stage + 5u * (scan[0][threadIdx.x] - 1u);
#pragma unroll
                for (int k = 0; k < 5; k++) sw[k] = mw[k];
            }
            if (f & 2u) {
                const uint32_t val = kind == kSkDf18 ? (v | (1u << 25)) : v;
                const uint32_t rcv = rx_of(p, x, sd.pos[i]);
                const uint32_t at = base[1] + scan[1][threadIdx.x] - 1u;
                host_store32(sd.out_adds + at, val);
                host_store32(x.out_add_rx + at, rcv);
                // visible to later passes only (this pass's k_score_rx has finished)
                if (kind != kSkDf18 && !rx_set_insert(x.set, x.set_lg, x.probe_max, rx_key(rcv, v))) no_room = true;
            }
            // leave both first-adder tables empty for the next pass, of either kind: every adder resets the slot its key
            // sits in (remembered at insertion; probes only happen in the score kernels, which have finished)
            const uint32_t hs = sd.slot[i];
            if (hs != 0xFFFFFFFFu) sd.hash[hs] = ~0ull;
            const uint32_t rs = x.rx_slot[i];
            if (rs != 0xFFFFFFFFu) x.first[rs] = ~0ull;
        }
        __syncthreads();
        {
            const uint32_t words = 5u * scan[0][255];
            unsigned long long *ow = (unsigned long long *)(out + base[0]);
            for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) {
                const unsigned long long v = stage[w];
                __hip_atomic_store(ow + w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                my_sum += v;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            base[0] += scan[0][255];
            base[1] += scan[1][255];
        }
        __syncthreads();
    }
    if (no_room) atomicOr(&sd.state->reserved, 1u);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) my_sum += __shfl_down(my_sum, off);
    if ((threadIdx.x & 63) == 0 && my_sum) atomicAdd(&sd.state->msg_sum, my_sum);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __shared__ bool is_last;
    __syncthreads();
    if (threadIdx.x == 0) is_last = atomicAdd(&sd.state->blocks_done, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!is_last) return;
    // the last block: totals and summary, then the state back to empty
    __shared__ uint32_t tot[2][4];
    {
        uint32_t nm = threadIdx.x < gridDim.x ? sd.blk[2 * threadIdx.x] : 0u;   // kScoreBlocks == blockDim.x
        uint32_t na = threadIdx.x < gridDim.x ? sd.blk[2 * threadIdx.x + 1] : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            nm += __shfl_down(nm, off);
            na += __shfl_down(na, off);
        }
        if ((threadIdx.x & 63) == 0) {
            tot[0][threadIdx.x >> 6] = nm;
            tot[1][threadIdx.x >> 6] = na;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t nm = tot[0][0] + tot[0][1] + tot[0][2] + tot[0][3];
        const uint32_t na = tot[1][0] + tot[1][1] + tot[1][2] + tot[1][3];
        const unsigned long long ms = atomicAdd(&sd.state->msg_sum, 0ull);
        // (k_rx_adders' insertions and this kernel's: whoever ran out of probes said so before its block counted in)
        const uint32_t out_of_probes = atomicOr(&sd.state->reserved, 0u) ? 1u : 0u;
        uint32_t *sm = (uint32_t *)sd.summary;
        const uint32_t vals[8] = {nm, na, (uint32_t)ms, (uint32_t)(ms >> 32), out_of_probes ? 0u : sd.state->scored, out_of_probes, 0u, sd.seq};
#pragma unroll
        for (int k = 0; k < 8; k++) host_store32(sm + k, vals[k]);
        sd.state->n = 0;
        sd.state->scored = 0;
        sd.state->blocks_done = 0;
        sd.state->reserved = 0;
        sd.state->msg_sum = 0;
    }
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
