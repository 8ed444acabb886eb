// adsb_aux.hip -- the small kernels around the scan: to_mag alone, the address/parity
// match, the record builder and the magnitude self-test digest.
#include <algorithm>

#include "../../include/adsb_hip.h"
#include "adsb_dev_common.h"
#include "adsb_scan_geometry.h"
#include "adsb_tail_dev.h"
#include "adsb_fix_dev.h"
#include "adsb_score_dev.h"

namespace adsb {

namespace {

// ---------------------------------------------------------------------------
// to_mag alone (adsb_to_mag).  data[0..326) = 0, data[326+k] = mag(iq[k]), rest 0
// (src/lib.rs:36-50, src/utils.rs:43-58).
// ---------------------------------------------------------------------------

// Eight outputs per thread: one 16-byte store (the output may be pinned host memory, written over the link:
// 2-byte stores would be 128 bytes per wave-instruction there); the eight samples behind them through a
// buffer resource over the n input samples (a dword each, 4-byte aligned: the 326-sample lead-in shifts the
// output by 6 of 8; out of range -- lead-in, tail -- reads as zero IQ, whose magnitude is zero).
__global__ __launch_bounds__(256) void k_to_mag(const uint32_t *__restrict__ iq, uint32_t n,
                                                uint16_t *__restrict__ data)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t i0 = 8u * t;                       // first output of this thread
    if (i0 >= (uint32_t)kMagDataLen) return;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)iq, 0, (int)(n * 4u), 0x00020000);
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        int off = ((int)i0 + i - kLead) * 4;          // negative in the lead-in: out of range, zero
        asm volatile("" : "+v"(off));                 // (not folded into the immediate: adsb_tail_dev.h, records)
        w[i] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0);
    }
    uint32_t pk[4];
#pragma unroll
    for (int i = 0; i < 4; i++) pk[i] = mag2(w[2 * i], w[2 * i + 1]);
    if (i0 + 8u <= (uint32_t)kMagDataLen) {
        *(uint4 *)(data + i0) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    } else {  // the last, partial group (131398 = 8 * 16424 + 6)
        for (uint32_t i = 0; i0 + i < (uint32_t)kMagDataLen; i++) data[i0 + i] = (uint16_t)(pk[i >> 1] >> (16 * (i & 1)));
    }
}

// The same from CU8 input (adsb_to_mag_u8): a 2-byte sample each through a resource over the n input samples,
// widened through the table and masked by position -- T[0] is not zero, so the lead-in and tail must not be
// left to the range check's zero bytes.
__global__ __launch_bounds__(256) void k_to_mag_u8(const uint8_t *__restrict__ iq, uint32_t n, const uint16_t *__restrict__ tab,
                                                   uint16_t *__restrict__ data)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t i0 = 8u * t;
    if (i0 >= (uint32_t)kMagDataLen) return;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)iq, 0, (int)(n * 2u), 0x00020000);
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = load_u8_sample(rsrc, (int)i0 + i - kLead, (int)n, tab);
    uint32_t pk[4];
#pragma unroll
    for (int i = 0; i < 4; i++) pk[i] = mag2(w[2 * i], w[2 * i + 1]);
    if (i0 + 8u <= (uint32_t)kMagDataLen) {
        *(uint4 *)(data + i0) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    } else {
        for (uint32_t i = 0; i0 + i < (uint32_t)kMagDataLen; i++) data[i0 + i] = (uint16_t)(pk[i >> 1] >> (16 * (i & 1)));
    }
}

// CU8 samples [first, first + count) widened into CS16 dwords: the overflow fallback's staging (the reference-shaped
// kernel reads CS16 only)
__global__ __launch_bounds__(256) void k_widen_u8(const uint8_t *__restrict__ src, unsigned long long first, uint32_t count,
                                                  const uint16_t *__restrict__ tab, uint32_t *__restrict__ dst)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint8_t *b = src + 2ull * (first + i);
    dst[i] = widen_u8_pair(tab, (uint32_t)b[0] | (uint32_t)b[1] << 8);
}

// ---------------------------------------------------------------------------
// reset: one launch per pass instead of a string of memsets.  Zeroes the counters and,
// after an icao_flush, the 2 MiB address bitmap; address 0 always tests true
// (src/icao_filter.rs:71-80: an empty slot equals 0), so bit 0 starts set.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_reset(Counters *ctr, uint32_t *bitmap, uint32_t lg)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    constexpr uint32_t kCtrDwords = sizeof(Counters) / 4;
    if (i < kCtrDwords) ((uint32_t *)ctr)[i] = 0;
    if (bitmap) bitmap_clear(bitmap, lg, i, gridDim.x * blockDim.x);
}

// ---------------------------------------------------------------------------
// match.  An address/parity trial can only score >= 0 if its CRC residual is in
// the filter when it is scored (mode_s/mod.rs:71,115,130); the bitmap now holds
// every address the filter can contain at any point of this call (plus 0, which
// icao_filter_test always accepts, icao_filter.rs:71-80).  Entries from the fast
// scan carry H' = x^51*H: the residual itself for 56-bit trials, x^56*H' for 112-bit
// ones (adsb_tables.h).
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_match(ScanParams p)
{
    if (p.order_cnt) TAIL_PRIO();  // dense streams only: elsewhere the scan is what bounds the step
    // the x^56 multiplier table (3 KB) and the bitmap's 4096-bit summary in LDS: an entry costs
    // one coalesced 8-byte load and LDS lookups; only the few per cent of residuals whose low 12
    // bits are taken by some address go on to the 2 MiB bitmap
    __shared__ uint32_t stab[3 * 256];
    __shared__ uint32_t coarse[kCoarseWords];
    for (int i = threadIdx.x; i < 3 * 256; i += blockDim.x) stab[i] = p.tables[kTabX56 * 256 + i];
    if (threadIdx.x < kCoarseWords) coarse[threadIdx.x] = p.bitmap[bitmap_words(p.bitmap_lg) + threadIdx.x];
    __syncthreads();
    const uint32_t seg_cap = p.seg_cap;
    // work units: pairs of wave segments of the fast scan's list (a few hundred entries per
    // segment), then the dap list of the simple kernel, which all the blocks past the segments
    // share.  Four entries per thread per trip -- two from each segment of the pair -- so that
    // their list loads, then their bitmap loads, are in flight together (the chain entry ->
    // residual -> bitmap word is all latency) and the usual pair is a single trip.
    const bool is_dap = blockIdx.x >= (uint32_t)kApWaveSegs / 2;
    uint32_t n[2];
    const uint64_t *ap[2];
    uint32_t first = 0, stride = 2 * blockDim.x;
    if (is_dap) {  // both halves walk the same list, interleaved
        n[0] = n[1] = min(p.ctr->n_dap, p.dap_cap);
        ap[0] = ap[1] = p.dap;
        first = (blockIdx.x - kApWaveSegs / 2) * 4 * blockDim.x;
        stride = (gridDim.x - kApWaveSegs / 2) * 4 * blockDim.x;
    } else {
        for (int h = 0; h < 2; h++) {
            const uint32_t sg = 2 * blockIdx.x + h;
            n[h] = min(p.ctr->seg_ap[sg], seg_cap);
            ap[h] = p.ap + (uint64_t)sg * seg_cap;
        }
    }
    const uint32_t nmax = max(n[0], n[1]);
    for (uint32_t i0 = first + threadIdx.x; i0 < nmax; i0 += stride) {
        uint64_t e[4];
        uint32_t c[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            // segment pair: k = 0,1 from the first, 2,3 from the second; dap: four consecutive strides
            const int h = is_dap ? 0 : k >> 1;
            const uint32_t i = i0 + (is_dap ? (uint32_t)k : (uint32_t)(k & 1)) * blockDim.x;
            e[k] = i < n[h] ? ap[h][i] : ~0ull;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t code = entry_code(e[k]);
            c[k] = entry_value(e[k]);
            if (code >= 5 && code < 10) c[k] = gf_apply(stab, c[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (e[k] == ~0ull || !((coarse[(c[k] & 4095u) >> 5] >> (c[k] & 31)) & 1u)) continue;
            const uint32_t at = bitmap_index(c[k], p.bitmap_lg);
            if ((p.bitmap[at >> 5] >> (at & 31)) & 1u) {  // rare: one atomic each
                const uint32_t idx = atomicAdd(&p.ctr->n_hits, 1u);
                if (p.order_cnt) {  // dense stream: into the buffer's bucket, its tile's part of it (adsb_device.h: order_tmp)
                    const uint32_t ch = (uint32_t)entry_chunk(e[k]), tl = entry_j(e[k]) / (uint32_t)fastgeo::kTile;
                    const uint32_t at = atomicAdd(&p.order_cnt[ch * fastgeo::kTilesPerChunk + tl], 1u);
                    if (at < kTileBucket) {
                        const size_t place = (size_t)ch * kOrderBucket + tl * kTileBucket + at;
                        p.order_tmp[place] = e[k];
                        // (an address/parity hit: no fields from the scan, the record builder slices it)
                        if (p.hit_fields) p.hit_fields[place * kHitFieldWords + 5] = 0u;
                    } else {
                        atomicOr(&p.ctr->overflow, 1u);
                    }
                } else if (idx < p.hits_cap) {
                    p.hits[idx] = e[k];
                    if (p.hit_fields) p.hit_fields[(size_t)idx * kHitFieldWords + 5] = 0u;
                } else {
                    atomicOr(&p.ctr->overflow, 1u);
                }
            }
        }
    }
}

// The match of a sparse stream's three-launch pass in a large context (no order_cnt, fast scan: the dap list is empty).
// What k_match pays per block before it looks at its pair's ~2.5 entries per thread is a dependent chain -- table loads,
// barrier, fill counts, entries, bitmap -- in a kernel that is all latency.  Here the fill counts come first, a block
// whose segments are empty leaves at once (small passes use a fraction of the segments), and the first trip's entries are
// in flight before the tables are staged, so the barrier waits for the longer of the two, not for both in turn.
// K segment pairs per block, consecutive ones: the next pair's entries are loaded before this pair's are looked at, and
// the staging is shared by K times as many entries -- measured, K = 2 and 4 are slower alone (9.0 and 12.2 us against 7.1)
// and beside a scan (31 us against 27): many short blocks beat few long ones here too.  The kernel asks for no issue
// priority: with it, it and the records kernel run in 16 us each beside a scan and the step gets 3 % longer.
// (ADSB_MATCH_PAIRS: K, 0 = k_match for these passes too; the A/B is in profiles/README.md: tail_rate.jsonl.)
#ifndef ADSB_MATCH_PAIRS
#define ADSB_MATCH_PAIRS 1
#endif
template <int K>
__global__ __launch_bounds__(256) void k_match_sparse(ScanParams p, uint32_t n_pairs)
{
    __shared__ uint32_t stab[3 * 256];
    __shared__ uint32_t coarse[kCoarseWords];
    const uint32_t seg_cap = p.seg_cap, tid = threadIdx.x;
    const uint32_t pair0 = blockIdx.x * (uint32_t)K;
    uint32_t n[K][2], any = 0;
#pragma unroll
    for (int q = 0; q < K; q++)
#pragma unroll
        for (int h = 0; h < 2; h++) {
            n[q][h] = pair0 + q < n_pairs ? min(p.ctr->seg_ap[2 * (pair0 + q) + h], seg_cap) : 0u;
            any |= n[q][h];
        }
    if (!any) return;  // (uniform: every thread read the same counts)
    // entries [base, base + 512) of both segments of pair q: k = 0,1 from the first, 2,3 from the second
    auto fetch = [&](const uint32_t (&cnt)[2], uint32_t pair, uint32_t base, uint64_t (&e)[4]) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t i = base + tid + (uint32_t)(k & 1) * 256u;
            e[k] = i < cnt[k >> 1] ? p.ap[(uint64_t)(2 * pair + (k >> 1)) * seg_cap + i] : ~0ull;
        }
    };
    auto look = [&](const uint64_t (&e)[4]) {
        uint32_t c[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t code = entry_code(e[k]);
            c[k] = entry_value(e[k]);
            if (code >= 5 && code < 10) c[k] = gf_apply(stab, c[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (e[k] == ~0ull || !((coarse[(c[k] & 4095u) >> 5] >> (c[k] & 31)) & 1u)) continue;
            const uint32_t at = bitmap_index(c[k], p.bitmap_lg);
            if ((p.bitmap[at >> 5] >> (at & 31)) & 1u) {  // rare: one atomic each
                const uint32_t idx = atomicAdd(&p.ctr->n_hits, 1u);
                if (idx < p.hits_cap) {
                    p.hits[idx] = e[k];
                    if (p.hit_fields) p.hit_fields[(size_t)idx * kHitFieldWords + 5] = 0u;
                } else {
                    atomicOr(&p.ctr->overflow, 1u);
                }
            }
        }
    };
    uint64_t e[4];
    fetch(n[0], pair0, 0u, e);
    for (uint32_t i = tid; i < 3 * 256; i += 256) stab[i] = p.tables[kTabX56 * 256 + i];
    if (tid < kCoarseWords) coarse[tid] = p.bitmap[bitmap_words(p.bitmap_lg) + tid];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < K; q++) {
        uint64_t nx[4];
        if (q + 1 < K) fetch(n[q + 1 < K ? q + 1 : q], pair0 + q + 1, 0u, nx);
        look(e);
        const uint32_t nmax = max(n[q][0], n[q][1]);
        for (uint32_t base = 512u; base < nmax; base += 512u) {  // (rare: the usual pair is a single trip)
            uint64_t f[4];
            fetch(n[q], pair0 + q, base, f);
            look(f);
        }
        if (q + 1 < K)
#pragma unroll
            for (int k = 0; k < 4; k++) e[k] = nx[k];
    }
}

// ---------------------------------------------------------------------------
// order.  The hit list is filled in whatever order workgroups finish; the host replay needs
// (buffer, j, try_phase) order (demodulate2400 walks j upwards and tries phases 4..8 at each,
// src/demod_2400.rs:121,158).  Sorting it here is a counting sort by buffer followed by a rank
// sort inside each buffer's handful of hits: a busy airspace leaves tens of hits per buffer, and
// keys are unique (a trial is either self-validating or address/parity, never both).
//   producers       whoever finds a hit puts it into its buffer's bucket (order_tmp, order_cnt)
//   k_order_prefix  one workgroup: exclusive prefix of the counts (order_base)
//   k_records       takes whole buckets: a workgroup sorts a buffer's bucket in LDS (rank sort) and
//                   writes its records at the bucket's place; the count goes back to zero, which
//                   is how the next pass must find it.  (The sorted hit list itself is never stored.)
// A pass whose lists overflowed is redone by the host anyway: its counts are only zeroed.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(1024) void k_order_prefix(ScanParams p)
{
    TAIL_PRIO();
    __shared__ uint32_t part[1024];
    __shared__ uint32_t carry;
    const uint32_t tid = threadIdx.x;
    constexpr uint32_t T = fastgeo::kTilesPerChunk;
    if (p.ctr->overflow) {  // (uniform) nothing will be ordered: leave the counts clean
        for (uint32_t c = tid; c < p.n_chunks * T; c += 1024) p.order_cnt[c] = 0;
        return;
    }
    if (tid == 0) carry = 0;
    __syncthreads();
    for (uint32_t c0 = 0; c0 <= p.n_chunks; c0 += 1024) {
        const uint32_t c = c0 + tid;
        uint32_t v = 0;   // the buffer's hits = its tiles' counts (adsb_device.h: kTileBucket)
        if (c < p.n_chunks)
#pragma unroll
            for (uint32_t t = 0; t < T; t++) v += min(p.order_cnt[c * T + t], kTileBucket);
        part[tid] = v;
        __syncthreads();
        for (uint32_t off = 1; off < 1024; off <<= 1) {
            const uint32_t add = tid >= off ? part[tid - off] : 0u;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        if (c <= p.n_chunks) p.order_base[c] = carry + part[tid] - v;
        __syncthreads();
        if (tid == 1023) carry += part[1023];
        __syncthreads();
    }
}


// ---------------------------------------------------------------------------
// device-side scoring (adsb_device.h: ScoreDev) of a pass with one filter.  The kernels' bodies are
// adsb_score_dev.h's; here is what a plain pass hands them: its filter (the exact bitmap, and the first
// index at which an address is added -- an open-addressing table of (value << 32 | index), atomic-min
// per key) and what k_emit does with an addition.
// ---------------------------------------------------------------------------

// index of the first adder of v in this pass, or 0xFFFFFFFF
__device__ __forceinline__ uint32_t score_hash_first(const ScoreDev &sd, uint32_t v)
{
    uint32_t h = score_hash_slot(v) & sd.hash_mask;
    for (;;) {
        const unsigned long long cur = __hip_atomic_load(&sd.hash[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == ~0ull) return 0xFFFFFFFFu;
        if ((uint32_t)(cur >> 32) == v) return (uint32_t)cur;
        h = (h + 1u) & sd.hash_mask;
    }
}

// "v is in the filter when trial i is scored" (src/icao_filter.rs:65-97; address 0 always is)
__device__ __forceinline__ bool score_in_filter(const ScoreDev &sd, uint32_t v, uint32_t i)
{
    if (v == 0) return true;
    if ((sd.exact[v >> 5] >> (v & 31)) & 1u) return true;
    if (sd.earlier && ((sd.earlier[v >> 5] >> (v & 31)) & 1u)) return true;
    return score_hash_first(sd, v) < i;
}

// the one filter of a plain pass, as the shared scoring of a trial asks for it (adsb_score_dev.h: score_trial)
struct PlainFilter {
    const ScoreDev &sd;
    __device__ __forceinline__ bool operator()(uint32_t v, uint32_t i) const { return score_in_filter(sd, v, i); }
};


// What k_emit does with an addition of a plain pass (adsb_score_dev.h: emit_body): into the exact bitmap.  An insertion
// there cannot fail, and there is no table or state of the policy's own: those hooks are empty and fold away.
struct PlainCommit {
    const ScoreDev &sd;
    __device__ __forceinline__ void clear_retired(uint32_t k0, uint32_t step) const
    {
        if (!sd.exact_retired) return;
        uint4 *w = (uint4 *)sd.exact_retired;
        for (uint32_t k = k0; k < kBitmapAllocWords / 4; k += step)
            w[k] = make_uint4(0u, 0u, 0u, 0u);
    }
    __device__ __forceinline__ bool commit(uint32_t, uint32_t, uint32_t v, bool keep) const
    {
        if (keep) atomicOr(&sd.exact[v >> 5], 1u << (v & 31));
        return true;
    }
    __device__ __forceinline__ void forget(uint32_t) const {}
    __device__ __forceinline__ uint32_t out_of_probes() const { return 0u; }
    __device__ __forceinline__ void reset_state() const {}
};

// k_score, k_emit: the shared bodies (adsb_score_dev.h) with the one filter of a plain pass
__global__ __launch_bounds__(256) void k_score(ScanParams p)
{
    TAIL_PRIO();
    score_body(p, [&](uint64_t) { return PlainFilter{p.score}; }, blockDim.x);
}

__global__ __launch_bounds__(256) void k_emit(ScanParams p)
{
    TAIL_PRIO();
    emit_body(p, PlainCommit{p.score}, blockDim.x);
}


// ---------------------------------------------------------------------------
// records (adsb_tail_dev.h: records_block).  One wave per hit: lanes are message bits.  The 291-sample
// window behind j is rebuilt from IQ (rare path: a handful of hits per chunk, so magnitudes are not
// kept in HBM), the 112 bits of the trial phase are sliced (demod_2400.rs:158-182) and the 33-sample
// power summed (:191-196).
// ---------------------------------------------------------------------------
template <bool FROM_MAG, bool BUCKETS, bool U8 = false>
__global__ __launch_bounds__(256) void k_records(ScanParams p, TrialRecord *rec)
{
    if (p.order_cnt) TAIL_PRIO();  // dense streams only: elsewhere the scan is what bounds the step
    // (dynamic LDS, only asked for by device-ordered launches: with 8 KB more a block of a sparse
    // stream's launch held up the next scan's workgroups on its CU -- sparse step +3.6 %)
    extern __shared__ uint64_t sorted[];
    records_block<FROM_MAG, BUCKETS, false, U8>(p, rec, blockIdx.x, gridDim.x, sorted, true);
}

// carry-over mode: the last kCarrySamples samples of the stream so far
__global__ __launch_bounds__(kCarrySamples) void k_update_carry(const uint32_t *__restrict__ prev,
                                                               const uint32_t *__restrict__ src, long long n,
                                                               uint32_t *__restrict__ next)
{
    const long long i = threadIdx.x, idx = n - kCarrySamples + i;
    next[i] = idx >= 0 ? src[idx] : prev[i + n];
}

// ... from CU8 input: the carry stays CS16, widened, so that a stream may alternate the two formats
__global__ __launch_bounds__(kCarrySamples) void k_update_carry_u8(const uint32_t *__restrict__ prev,
                                                                  const uint8_t *__restrict__ src, long long n,
                                                                  const uint16_t *__restrict__ tab, uint32_t *__restrict__ next)
{
    const long long i = threadIdx.x, idx = n - kCarrySamples + i;
    next[i] = idx >= 0 ? widen_u8_pair(tab, (uint32_t)src[2 * idx] | (uint32_t)src[2 * idx + 1] << 8) : prev[i + n];
}

// first phase of a shard that listed its fresh addresses as it scanned (ScanParams::fresh): only the summary is
// left to write.  Same ten words, same order as the records kernel's (seq last); rec_sum_lo carries the sum of the
// listed addresses, n_dap their count.
__global__ __launch_bounds__(64) void k_shard_summary(ScanParams p)
{
    if (threadIdx.x != 0) return;
    uint32_t *sm = (uint32_t *)p.summary;
    const uint32_t vals[9] = {p.ctr->n_hits, p.ctr->overflow, p.ctr->fresh_sum, p.ctr->n_fresh, 0u, 0u, 0u, p.seq, 0u};
    host_store32(sm + 9, summary_check(vals));
    host_store32(sm + 8, 0u);
#pragma unroll
    for (int k = 0; k < 8; k++) host_store32(sm + k, vals[k]);
}

// addresses learned elsewhere (other shards of the same capture) join the superset
__global__ __launch_bounds__(256) void k_set_addresses(const uint32_t *__restrict__ addrs, uint32_t n,
                                                       uint32_t *bitmap, uint32_t lg)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) bitmap_set(bitmap, lg, addrs[i] & 0xFFFFFFu);
}

// ---------------------------------------------------------------------------
// self-test: digest of the magnitude tail over consecutive f32 bit patterns of
// X = im^2 + rn(re^2) (an integer-valued float in [0, 2^31]).  Lets a test sweep every
// representable X against the CPU pipeline, which proves the folded constant and
// the device sqrt exactly.  out[0] += sum of outputs, out[1] ^= order-free hash.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mag_digest(uint32_t first_bits, uint32_t count,
                                                    unsigned long long *out)
{
    unsigned long long sum = 0, h = 0;
    // pairs (i, i + half) so that both lanes of the packed pipeline are exercised
    const uint32_t half = (count + 1) / 2;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < half; i += gridDim.x * blockDim.x) {
        const uint32_t b0 = first_bits + i, b1 = first_bits + i + half;
        const f32x2 x = {__uint_as_float(b0), __uint_as_float(i + half < count ? b1 : 0u)};
        const uint32_t pk = mag_tail2(x);
        const uint32_t u0 = pk & 0xFFFFu, u1 = pk >> 16;
        sum += u0;
        h ^= ((unsigned long long)u0 + 1ull) * (2ull * b0 + 1ull);
        if (i + half < count) {
            sum += u1;
            h ^= ((unsigned long long)u1 + 1ull) * (2ull * b1 + 1ull);
        }
    }
    atomicAdd(&out[0], sum);
    atomicXor(&out[1], h);
}

// self-test: the lookup k_score / k_emit repair with, over a list of residuals (adsb_selftest_fix_lookup)
__global__ __launch_bounds__(256) void k_fix_lookup(const uint32_t *__restrict__ tables, const uint32_t *__restrict__ residuals,
                                                    uint32_t n, uint32_t mode, uint32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = fix_lookup(tables, residuals[i], mode);
}

inline int hip_ok(hipError_t e) { return e == hipSuccess ? 0 : (int)e; }
// hipGetLastError is sticky across unrelated calls (the caller's too): start every launch clean
inline void hip_clear() { (void)hipGetLastError(); }

}  // namespace

int launch_to_mag(const void *d_iq, uint32_t n, uint16_t *d_data, void *stream, const uint16_t *u8_table)
{
    hip_clear();
    const int blocks = ((kMagDataLen + 7) / 8 + 255) / 256;
    if (u8_table) {
        hipLaunchKernelGGL(k_to_mag_u8, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)d_iq, n, u8_table, d_data);
        return hip_ok(hipGetLastError());
    }
    hipLaunchKernelGGL(k_to_mag, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       (const uint32_t *)d_iq, n, d_data);
    return hip_ok(hipGetLastError());
}

int launch_widen_u8(const void *d_src, uint64_t first, uint32_t count, const uint16_t *u8_table, uint32_t *dst, void *stream)
{
    hip_clear();
    if (count == 0) return 0;
    hipLaunchKernelGGL(k_widen_u8, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)d_src,
                       (unsigned long long)first, count, u8_table, dst);
    return hip_ok(hipGetLastError());
}

int launch_reset(Counters *ctr, uint32_t *bitmap, uint32_t bitmap_lg, void *stream)
{
    hip_clear();
    const uint32_t ctr_blocks = (uint32_t)((sizeof(Counters) / 4 + 255) / 256);
    const uint32_t blocks = bitmap ? std::max(ctr_blocks, std::min(512u, bitmap_alloc_words(bitmap_lg) / 4 / 256 + 1u)) : ctr_blocks;
    hipLaunchKernelGGL(k_reset, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ctr, bitmap, bitmap_lg);
    return hip_ok(hipGetLastError());
}

int launch_match(const ScanParams &p, void *stream, bool sparse_fast)
{
    hip_clear();
    if (sparse_fast && ADSB_MATCH_PAIRS && !p.order_cnt) {
        // the segments this pass's scan can have filled: four per workgroup of its grid (adsb_scan_fast.hip: launch_scan)
        const uint32_t tiles = p.n_chunks * (uint32_t)fastgeo::kTilesPerChunk;
        const uint32_t n_pairs = 2u * std::min(tiles, (uint32_t)scan_resident_blocks());
        constexpr uint32_t K = ADSB_MATCH_PAIRS ? ADSB_MATCH_PAIRS : 1;
        static_assert(K <= 8, "the fill counts of a block's pairs are held in registers");
        if (n_pairs == 0) return 0;
        hipLaunchKernelGGL((k_match_sparse<(int)K>), dim3((n_pairs + K - 1) / K), dim3(256), 0, (hipStream_t)stream, p, n_pairs);
        return hip_ok(hipGetLastError());
    }
    // one block per two wave segments of the fast scan's AP list, 64 for the dap list; the fill
    // counts live on the device
    const uint32_t blocks = kApWaveSegs / 2 + 64;  // 64 blocks share the dap list
    hipLaunchKernelGGL(k_match, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    return hip_ok(hipGetLastError());
}

// Blocks of the records kernel behind a sparse stream's match (no order_cnt): a few hundred hits, whatever the pass's
// size.  (ADSB_REC_SPARSE_BLOCKS: 0 = a block per buffer there too.)
#ifndef ADSB_REC_SPARSE_BLOCKS
#define ADSB_REC_SPARSE_BLOCKS 72
#endif

int launch_records(const ScanParams &p, SrcFormat fmt, TrialRecord *d_rec, void *stream, bool sparse_fast)
{
    hip_clear();
    // Contiguous runs of hits per block (the count lives on the device); on sparse input most
    // blocks find nothing and leave at once.  Measured on dense input (17 000 hits per pass, beside
    // a scan): the kernel's duration does not depend on the block count between one per CU and
    // one per buffer (the scan's four workgroups leave a SIMD 96 registers per lane, one wave of
    // this kernel, whatever the grid), and four or eight blocks per buffer are two and four
    // times slower (more rounds of the fixed per-block latencies).  What it does depend on is the
    // instruction count per hit: see the hit loop.
    // (every block ends with one atomic on the same counter, ~90 of them a microsecond on this chip: a pass of
    // 4096 buffers with a block per buffer spent 126 us in a kernel that writes a few hundred records --
    // profiles/r5_multi_overhead.txt; beyond 1024 blocks the runs per block simply get longer)
    uint32_t blocks = p.n_chunks + 8u;
    if (blocks > 1024) blocks = 1024;
    // A sparse stream's pass (host-ordered, CS16): its hit list is bounded by hits_cap and holds a few hundred entries in
    // practice, so a block per buffer is 500 blocks that find nothing and still take their turn at the one counter behind
    // the last-block ticket.  A small fixed grid instead, whatever the pass's size: the runs per block get longer (at 2000
    // hits: 28, less than one batch), the retired bitmap's clear is 7 x 16 bytes per thread instead of one.  Alone the
    // kernel takes 11.3 us instead of 15.0, beside a scan 43 instead of 52; 32, 144 and 256 blocks measured no better.
    if (sparse_fast && ADSB_REC_SPARSE_BLOCKS && !p.order_cnt && fmt == SrcFormat::kCs16) blocks = ADSB_REC_SPARSE_BLOCKS;
    if (fmt == SrcFormat::kCu8) {
        if (!p.u8_table) return (int)hipErrorInvalidValue;
        if (p.order_cnt)
            hipLaunchKernelGGL((k_records<false, true, true>), dim3(blocks), dim3(256), kOrderBucket * (sizeof(uint64_t) + sizeof(uint16_t)),
                               (hipStream_t)stream, p, d_rec);
        else
            hipLaunchKernelGGL((k_records<false, false, true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, d_rec);
    } else if (fmt == SrcFormat::kMag)  // (one caller-supplied buffer: never device-ordered)
        hipLaunchKernelGGL((k_records<true, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, d_rec);
    else if (p.order_cnt)  // device-ordered: dynamic LDS for the bucket being sorted
        hipLaunchKernelGGL((k_records<false, true>), dim3(blocks), dim3(256), kOrderBucket * (sizeof(uint64_t) + sizeof(uint16_t)),
                           (hipStream_t)stream, p, d_rec);
    else
        hipLaunchKernelGGL((k_records<false, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, d_rec);
    return hip_ok(hipGetLastError());
}

int launch_order_hits(const ScanParams &p, void *stream)
{
    hip_clear();
    if (!p.order_cnt || !p.order_base || !p.order_tmp) return 0;
    hipLaunchKernelGGL(k_order_prefix, dim3(1), dim3(1024), 0, (hipStream_t)stream, p);
    return hip_ok(hipGetLastError());
}

int launch_score(const ScanParams &p, void *stream)
{
    hip_clear();
    if (!p.score.si) return 0;
    hipLaunchKernelGGL(k_score, dim3(kScoreBlocks), dim3(256), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(k_emit, dim3(kScoreBlocks), dim3(256), 0, (hipStream_t)stream, p);
    return hip_ok(hipGetLastError());
}

int launch_set_addresses(const uint32_t *d_addrs, uint32_t n, uint32_t *bitmap, uint32_t bitmap_lg, void *stream)
{
    hip_clear();
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_set_addresses, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_addrs, n,
                       bitmap, bitmap_lg);
    return hip_ok(hipGetLastError());
}

int launch_shard_summary(const ScanParams &p, void *stream)
{
    hip_clear();
    hipLaunchKernelGGL(k_shard_summary, dim3(1), dim3(64), 0, (hipStream_t)stream, p);
    return hip_ok(hipGetLastError());
}

int launch_update_carry(const uint32_t *prev, const void *d_src, uint64_t n_samples, uint32_t *next, void *stream,
                        const uint16_t *u8_table)
{
    hip_clear();
    if (u8_table) {
        hipLaunchKernelGGL(k_update_carry_u8, dim3(1), dim3(kCarrySamples), 0, (hipStream_t)stream, prev,
                           (const uint8_t *)d_src, (long long)n_samples, u8_table, next);
        return hip_ok(hipGetLastError());
    }
    hipLaunchKernelGGL(k_update_carry, dim3(1), dim3(kCarrySamples), 0, (hipStream_t)stream, prev,
                       (const uint32_t *)d_src, (long long)n_samples, next);
    return hip_ok(hipGetLastError());
}

int launch_fix_lookup(const uint32_t *tables, const uint32_t *d_residuals, uint32_t n, uint32_t mode, uint32_t *d_out, void *stream)
{
    hip_clear();
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_fix_lookup, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, tables, d_residuals, n, mode, d_out);
    return hip_ok(hipGetLastError());
}

int launch_mag_digest(uint32_t first_bits, uint32_t count, unsigned long long *d_out, void *stream)
{
    hip_clear();
    hipLaunchKernelGGL(k_mag_digest, dim3(1024), dim3(256), 0, (hipStream_t)stream, first_bits, count,
                       d_out);
    return hip_ok(hipGetLastError());
}

}  // namespace adsb
