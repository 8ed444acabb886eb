// adsb_seam.hip -- receiver seams (adsb_set_receiver_carry): carry-over for a pass that holds many receivers' buffers.
//
// In the reference a trial at position j reads data[j .. j+290] and nothing else (src/demod_2400.rs:127-196), so what
// a buffer's lead-in holds decides the trials at j < 326 and no others.  The pass's own scan keeps its zero lead-in
// and is right from j = 326 on; the kernels here try the first 326 positions of every buffer against the lead-in the
// buffer's own receiver left:
//
//   k_rx_lead          per buffer, the 328 samples in front of it: the receiver's carry, or the end of the receiver's
//                      previous buffer in the same pass
//   k_rx_carry_update  per receiver, the end of its last buffer of the pass becomes its carry (a launch of its own: no
//                      workgroup reads a carry that another one writes)
//   k_seam_scan        reference-shaped, one workgroup per buffer: magnitudes of lead-in ++ the buffer's first samples,
//                      the gates, five trial phases, DF class and CRC residual.  Self-validating trials are finished
//                      records and teach the pass's address superset; address/parity trials go to the seam list
//   k_seam_match       behind the pass's last kernel: the seam list against the superset, the hits as records, then the
//                      count and the checksum for the host
//
// Records go straight into mapped host memory; the host drops the pass's own records with j < 326 and replays these in
// their place (adsb_collect.cpp).
#include "adsb_dev_common.h"
#include "adsb_fix_dev.h"

namespace adsb {

namespace {

constexpr int kSeamRowPad = kCarrySamples - kLead;   // a lead-in row holds offsets -328 .. -1: data[d] is row[d + 2]
constexpr int kSeamMags = 624;                       // data[0 .. 325 + kReach], rounded up
static_assert(kSeamMags >= kLead + kReach + 1, "every sample a seam trial touches");

__device__ __forceinline__ void seam_store64(unsigned long long *p, unsigned long long v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // written through: mapped host memory
}
__device__ __forceinline__ void seam_store32(uint32_t *p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// sample s of the pass's input as a CS16 dword (CU8 widened through the table); s < n_samples
__device__ __forceinline__ uint32_t seam_sample(const SeamParams &q, uint64_t s)
{
    if (q.u8_table) return widen_u8_pair(q.u8_table, (uint32_t)((const uint16_t *)q.src)[s]);
    return ((const uint32_t *)q.src)[s];
}

// a finished record into the block in mapped host memory, its words into the checksum
__device__ __forceinline__ void seam_emit(const SeamParams &q, const TrialRecord &r)
{
    const uint32_t at = atomicAdd(&q.ctr->n_rec, 1u);
    if (at >= q.rec_cap) {
        atomicOr(&q.ctr->overflow, 1u);
        return;
    }
    unsigned long long w[4];
    __builtin_memcpy(w, &r, sizeof r);
    unsigned long long *dst = (unsigned long long *)(q.rec + at);
#pragma unroll
    for (int k = 0; k < 4; k++) seam_store64(dst + k, w[k]);
    atomicAdd(&q.ctr->rec_sum, w[0] + w[1] + w[2] + w[3]);
    // scored on the device (adsb_seam_score.hip): the same record into the mirror the merge reads, behind this pass's
    // k_seam_match on another stream -- a kernel boundary and an event, like ScoreDev::rec
    if (q.rec_dev) q.rec_dev[at] = r;
}

__device__ __forceinline__ bool seam_bitmap_test(const uint32_t *bitmap, uint32_t lg, uint32_t a)
{
    const uint32_t at = bitmap_index(a, lg);
    return (__hip_atomic_load(&bitmap[at >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (at & 31)) & 1u;
}

__global__ __launch_bounds__(128) void k_rx_lead(SeamParams q)
{
    const uint32_t b = blockIdx.x;
    if (b >= q.n_chunks) return;
    const SeamDesc d = q.desc[b];
    uint32_t *row = q.lead + (size_t)b * kCarrySamples;
    for (int i = threadIdx.x; i < kCarrySamples; i += blockDim.x) {
        uint32_t w = 0;
        if (d.prev < 0) {
            if (d.rx < q.n_receivers) w = q.carry[(size_t)d.rx * kCarrySamples + i];
        } else if ((uint32_t)d.prev < b) {
            // (a buffer with a successor in the pass is a whole one: only a pass's last buffer may be short)
            const uint64_t s = (uint64_t)d.prev * kChunkSamples + (uint64_t)(kChunkSamples - kCarrySamples + i);
            if (s < q.n_samples) w = seam_sample(q, s);
        }
        row[i] = w;
    }
}

// carry[i] = sample (len - 328 + i) of lead-in ++ buffer: k_update_carry's rule, per receiver
__global__ __launch_bounds__(128) void k_rx_carry_update(SeamParams q)
{
    const uint32_t b = blockIdx.x;
    if (b >= q.n_chunks) return;
    const SeamDesc d = q.desc[b];
    if (!d.last || d.rx >= q.n_receivers) return;
    const int len = chunk_len(q.n_samples, b);
    const uint32_t *row = q.lead + (size_t)b * kCarrySamples;
    uint32_t *carry = q.carry + (size_t)d.rx * kCarrySamples;
    for (int i = threadIdx.x; i < kCarrySamples; i += blockDim.x) {
        const int k = len - kCarrySamples + i;
        carry[i] = k >= 0 ? seam_sample(q, (uint64_t)b * kChunkSamples + (uint64_t)k) : row[kCarrySamples + k];
    }
}

__global__ __launch_bounds__(256) void k_seam_scan(SeamParams q)
{
    __shared__ uint16_t smag[kSeamMags];
    __shared__ uint32_t scrc[256];
    __shared__ uint16_t scand[kLead];
    __shared__ uint32_t sncand;

    if (blockIdx.x >= q.n_scan) return;
    const uint32_t chunk = q.first_chunk + blockIdx.x;
    if (chunk >= q.n_chunks) return;
    const int len = chunk_len(q.n_samples, chunk);
    const int jn = min(kLead, len);
    scrc[threadIdx.x] = crc_table_entry(threadIdx.x);
    if (threadIdx.x == 0) sncand = 0;
    // data[0 .. kSeamMags) of the buffer's MagnitudeBuffer: the lead-in, then the buffer, then zeros
    const uint32_t *row = q.lead + (size_t)chunk * kCarrySamples;
    for (int d = threadIdx.x; d < kSeamMags; d += blockDim.x) {
        uint32_t w = 0;
        if (d < kLead) w = row[d + kSeamRowPad];
        else if (d - kLead < len) w = seam_sample(q, (uint64_t)chunk * kChunkSamples + (uint64_t)(d - kLead));
        smag[d] = (uint16_t)mag_of_dword(w);
    }
    __syncthreads();

    // --- preamble / SNR / quiet gates for every seam position (demod_2400.rs:121-146)
    for (int j = threadIdx.x; j < jn; j += blockDim.x)
        if (preamble_gates(smag + j)) scand[atomicAdd(&sncand, 1u)] = (uint16_t)j;
    __syncthreads();
    const int ntrial = (int)sncand * 5;

    // --- five trial phases per candidate (demod_2400.rs:158-184): slice, DF, CRC.  A trial is sliced by kSliceLanes
    // neighbouring lanes, 112 / kSliceLanes bits each, and the words are OR-ed together across them: one thread walking
    // all 112 bits through LDS was this kernel's whole duration (~90 us a launch, the scan's own order of magnitude)
    constexpr int kSliceLanes = 8, kBitsPerLane = 112 / kSliceLanes;
    static_assert(kBitsPerLane * kSliceLanes == 112 && 64 % kSliceLanes == 0, "whole trials per wave");
    const int sub = threadIdx.x % kSliceLanes;
    const int per_round = blockDim.x / kSliceLanes;
    for (int t0 = 0; t0 < ntrial; t0 += per_round) {     // (uniform: every lane takes part in the shuffles)
        const int t = t0 + (int)threadIdx.x / kSliceLanes;
        const bool live = t < ntrial;
        const int j = live ? scand[t / 5] : 0, tp = 4 + t % 5;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (live) {
            int pos = 5 * 19 + tp + 12 * kBitsPerLane * sub;
            for (int n = kBitsPerLane * sub; n < kBitsPerLane * (sub + 1); n++, pos += 12) {
                const int sidx = pos / 5, ph = pos - 5 * sidx;
                if (slice_value_any(smag + j + sidx, ph) > 0) w[n >> 5] |= 0x80000000u >> (n & 31);
            }
        }
#pragma unroll
        for (int off = 1; off < kSliceLanes; off <<= 1)
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] |= __shfl_xor(w[k], off);
        if (!live || sub != 0) continue;
        if ((w[0] | w[1] | w[2] | w[3]) == 0) continue;   // mode_s/mod.rs:51
        const uint32_t df = w[0] >> 27;                   // :41
        const uint32_t addr = w[0] & 0xFFFFFFu;           // message bits 8..31
        bool is_hit = false, is_ap = false;
        uint32_t c = 0;
        if (df == 11) {                                   // :73-90
            c = modes_checksum(w, 7, scrc);
            is_hit = (c & 0xFFFF80u) == 0;
            if (is_hit && (c & 0x7Fu) == 0) bitmap_set(q.bitmap, q.bitmap_lg, addr);   // the replay adds it
        } else if (df == 17 || df == 18) {                // :91-109
            c = modes_checksum(w, 14, scrc);
            if (c == 0) {
                is_hit = true;
                // DF18 adds addr | 1 << 25, which no 24-bit test can match
                if (df == 17) bitmap_set(q.bitmap, q.bitmap_lg, addr);
            } else if (q.fix) {                           // (a repaired trial adds nothing)
                is_hit = fix_lookup(q.tables, c, q.fix) != kFixNoRepair;
            }
        } else if (df == 0 || df == 4 || df == 5) {       // :56-72
            is_ap = true;
            c = modes_checksum(w, 7, scrc);
        } else if (df == 16 || df == 20 || df == 21 || df >= 24) {   // :110-135
            is_ap = true;
            c = modes_checksum(w, 14, scrc);
        }
        if (!is_hit && !is_ap) continue;
        TrialRecord r;
        unsigned long long pw = 0;
        for (int k = 0; k < 33; k++) {                    // demod_2400.rs:191-196
            const unsigned long long m = smag[j + 19 + k];
            pw += m * m;
        }
        r.power = pw | ((unsigned long long)c << 40);
        r.chunk = chunk;
        r.j_tp = (uint32_t)j | ((uint32_t)tp << 24);
#pragma unroll
        for (int k = 0; k < 14; k++) r.msg[k] = (uint8_t)msg_byte(w, k);
        r.pad = 1;                                        // `power` carries the residual
        if (is_hit || q.emit_all) {
            seam_emit(q, r);
        } else {
            const uint32_t at = atomicAdd(&q.ctr->n_list, 1u);
            if (at < q.list_cap) q.list[at] = r;
            else atomicOr(&q.ctr->overflow, 2u);
        }
    }
}

// one workgroup: the seam list is a few entries per buffer
__global__ __launch_bounds__(256) void k_seam_match(SeamParams q)
{
    const uint32_t n = min(__hip_atomic_load(&q.ctr->n_list, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), q.list_cap);
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const TrialRecord r = q.list[i];
        if (seam_bitmap_test(q.bitmap, q.bitmap_lg, (uint32_t)(r.power >> 40) & 0xFFFFFFu)) seam_emit(q, r);
    }
    __threadfence_system();   // this thread's records have left
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint32_t n_rec = __hip_atomic_load(&q.ctr->n_rec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t ovf = __hip_atomic_load(&q.ctr->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long rs = __hip_atomic_load(&q.ctr->rec_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t n_list = __hip_atomic_load(&q.ctr->n_list, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t vals[6] = {min(n_rec, q.rec_cap), ovf, (uint32_t)rs, (uint32_t)(rs >> 32), n_list, 0u};
    uint32_t *sm = (uint32_t *)q.summary;
    seam_store32(sm + 6, seam_summary_check(vals, q.seq));
#pragma unroll
    for (int k = 0; k < 6; k++) seam_store32(sm + k, vals[k]);
    __threadfence_system();
    // the counters back to zero, BEFORE the summary's sequence word goes out: the host may reuse the slot as soon as it
    // has seen that word, and the slot's next k_seam_scan (scan stream 0) need not be in stream order behind this kernel
    // (a three-launch pass's match runs on the tail stream)
    if (q.note) {   // ... and what the device-side merge needs of them first
        q.note[0] = vals[0];
        q.note[1] = ovf;
    }
    q.ctr->n_list = q.ctr->n_rec = q.ctr->overflow = q.ctr->reserved = 0;
    q.ctr->rec_sum = 0;
    __threadfence();
    seam_store32(sm + 7, q.seq);   // last
}

inline int hip_ok(hipError_t e) { return e == hipSuccess ? 0 : (int)e; }
inline void hip_clear() { (void)hipGetLastError(); }

bool seam_params_ok(const SeamParams &q)
{
    return q.src && q.n_chunks && q.n_samples > (uint64_t)(q.n_chunks - 1) * kChunkSamples &&
           q.n_samples <= (uint64_t)q.n_chunks * kChunkSamples && q.lead && q.ctr && q.summary && q.rec && q.bitmap && q.tables;
}

}  // namespace

int launch_seam_lead(const SeamParams &q, void *stream)
{
    hip_clear();
    if (!seam_params_ok(q) || !q.desc || !q.carry || !q.n_receivers) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rx_lead, dim3(q.n_chunks), dim3(128), 0, (hipStream_t)stream, q);
    hipLaunchKernelGGL(k_rx_carry_update, dim3(q.n_chunks), dim3(128), 0, (hipStream_t)stream, q);
    return hip_ok(hipGetLastError());
}

int launch_seam_scan(const SeamParams &q, void *stream)
{
    hip_clear();
    if (!seam_params_ok(q) || !q.n_scan || q.first_chunk + q.n_scan > q.n_chunks || (!q.emit_all && !q.list))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_seam_scan, dim3(q.n_scan), dim3(256), 0, (hipStream_t)stream, q);
    return hip_ok(hipGetLastError());
}

int launch_seam_match(const SeamParams &q, void *stream)
{
    hip_clear();
    if (!seam_params_ok(q)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_seam_match, dim3(1), dim3(256), 0, (hipStream_t)stream, q);
    return hip_ok(hipGetLastError());
}

}  // namespace adsb
