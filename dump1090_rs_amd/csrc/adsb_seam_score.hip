// adsb_seam_score.hip -- receiver seams scored on the device (adsb_set_receiver_carry_scoring): the device-side merge.
//
// A receivers pass with a seam step that is scored on the device has two sources of trials: the records kernel's ordered
// arrays (ScoreDev::rec, si, pos, slot; ScoreState::n of them, in (buffer, j, try_phase) order), whose hits at j < kLead
// tried a zero lead-in and do not count, and the seam step's records (adsb_seam.hip), which tried those positions against
// the receiver's own lead-in.  The kernels here, on the score stream in front of k_rx_adders, write the pass the keyed
// kernels (adsb_score_rx.hip, unchanged) are to score into a second set of arrays: every seam record and every own hit
// with j >= kLead, in (buffer, j, try_phase) order.  adsb_seam_score_dev.h has the index arithmetic; no sort is needed.
//
//   k_seam_mark     one thread per own hit and per seam record: the first own hit of every buffer (the hits are ordered:
//                   a buffer's run starts where the buffer index changes), the own hits a buffer drops, a presence bit
//                   per seam record; and the plain first-adder table emptied -- a receivers pass never consults it, and
//                   the merged arrays name no slot of it
//   k_seam_prefix   one workgroup: per buffer the seam records present, the exclusive sums of dropped and present over
//                   the buffers, where each buffer's seam records land and what its kept own hits move by; the merged
//                   count into ScoreState::n -- or, after a seam overflow or with more merged hits than the arrays hold,
//                   ScoreState::scored = 0 and n = 0: the keyed kernels then do nothing, their summary says so and the
//                   host replays; the merge's own summary for the host
//   k_seam_place    one thread per own hit and per seam record: each into its place; a seam record classified as the
//                   records kernel classifies a hit.  Its last workgroup leaves the presence rows and the drop counts zero
// The first set of arrays stays as it was: a host that refuses the result fetches ScoreDev::rec as it always did.
// Like the other tail kernels they run beside the next pass's scan: issue priority raised, agent-scope accesses, no fence.
#include "adsb_dev_common.h"
#include "adsb_scan_geometry.h"
#include "adsb_tail_dev.h"
#include "adsb_seam_score_dev.h"

namespace adsb {

namespace {

static_assert(kSeamLead == (uint32_t)kLead, "the seam positions");
static_assert((uint32_t)kSeamSkOther == kSkOther && (uint32_t)kSeamSkApShort == kSkApShort && (uint32_t)kSeamSkApLong == kSkApLong &&
                  (uint32_t)kSeamSkDf11Iid0 == kSkDf11Iid0 && (uint32_t)kSeamSkDf11 == kSkDf11 && (uint32_t)kSeamSkDf17 == kSkDf17 &&
                  (uint32_t)kSeamSkDf18 == kSkDf18 && (uint32_t)kSeamSkNone == kSkNone,
              "adsb_seam_score_dev.h restates ScoreKind");

constexpr int kMergeBlocks = kScoreBlocks, kMergeThreads = 256;

// seam records the merge has in hand: none after an overflow (the pass is not scored then)
__device__ __forceinline__ uint32_t seam_count(const SeamMergeParams &m) { return m.note[1] ? 0u : min(m.note[0], m.seam_cap); }

__global__ __launch_bounds__(kMergeThreads) void k_seam_mark(ScanParams p, SeamMergeParams m)
{
    TAIL_PRIO();
    const ScoreDev &sd = p.score;
    const uint32_t n = min(sd.state->n, sd.cap), nb = p.n_chunks;
    const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x, gn = gridDim.x * blockDim.x;
    bool bad = false;
    if (n == 0)
        for (uint32_t b = gi; b <= nb; b += gn) m.own_start[b] = 0;
    for (uint32_t i = gi; i < n; i += gn) {
        const unsigned long long pos = sd.pos[i];
        const uint32_t b = (uint32_t)min(pos >> 24, (unsigned long long)nb), j = (uint32_t)pos & 0xFFFFFFu;
        const uint32_t hs = sd.slot[i];
        if (hs <= sd.hash_mask) sd.hash[hs] = ~0ull;   // (0xFFFFFFFF: no adder)
        if (b >= nb) bad = true;
        else if (j < kSeamLead) atomicAdd(&m.drop[b], 1u);
        // buffers (the one before, b] start here; the last hit closes every buffer behind its own
        const uint32_t from = i ? (uint32_t)min(sd.pos[i - 1] >> 24, (unsigned long long)nb) + 1u : 0u;
        for (uint32_t k = from; k <= min(b, nb); k++) m.own_start[k] = i;
        if (i == n - 1)
            for (uint32_t k = b + 1; k <= nb; k++) m.own_start[k] = n;
        if (i && from > b + 1u) bad = true;            // (not in buffer order: the records kernel's fault)
    }
    const uint32_t ns = seam_count(m);
    for (uint32_t s = gi; s < ns; s += gn) {
        const uint32_t b = m.seam_rec[s].chunk, key = seam_key(m.seam_rec[s].j_tp);
        if (b >= nb || key >= kSeamKeys) {
            bad = true;
            continue;
        }
        const uint32_t bit = 1u << (key & 31u);
        if (atomicOr(&m.present[(size_t)b * kSeamKeyStride + (key >> 5)], bit) & bit) bad = true;   // (a key twice)
    }
    if (bad) atomicOr(&m.st->bad, 1u);
}

__global__ __launch_bounds__(kMergeThreads) void k_seam_prefix(ScanParams p, SeamMergeParams m)
{
    TAIL_PRIO();
    __shared__ uint32_t sc[2][kMergeThreads];
    __shared__ uint32_t carry[2];
    const ScoreDev &sd = p.score;
    const uint32_t nb = p.n_chunks, t = threadIdx.x;
    if (t < 2) carry[t] = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < nb; b0 += kMergeThreads) {
        const uint32_t b = b0 + t;
        const uint32_t s = b < nb ? seam_row_count(m.present + (size_t)b * kSeamKeyStride) : 0u;
        const uint32_t d = b < nb ? m.drop[b] : 0u;
        sc[0][t] = d, sc[1][t] = s;
        __syncthreads();
        for (uint32_t off = 1; off < kMergeThreads; off <<= 1) {   // inclusive scans of both
            const uint32_t vd = t >= off ? sc[0][t - off] : 0u, vs = t >= off ? sc[1][t - off] : 0u;
            __syncthreads();
            sc[0][t] += vd, sc[1][t] += vs;
            __syncthreads();
        }
        const uint32_t d_upto = carry[0] + sc[0][t], s_upto = carry[1] + sc[1][t];
        if (b < nb) {
            m.seam_base[b] = seam_base_of(m.own_start[b], d_upto - d, s_upto - s);
            m.own_shift[b] = seam_own_shift(d_upto, s_upto);
        }
        __syncthreads();
        if (t == kMergeThreads - 1) carry[0] = d_upto, carry[1] = s_upto;
        __syncthreads();
    }
    if (t != 0) return;
    const uint32_t n_own = min(sd.state->n, sd.cap), scored = sd.state->scored;
    const uint32_t ovf = m.note[1], ns = seam_count(m);
    const uint32_t d_total = carry[0], s_total = carry[1];
    const uint32_t bad = __hip_atomic_load(&m.st->bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool go = scored && !bad && s_total == ns && seam_merge_fits(n_own, d_total, s_total, sd.cap, ovf);
    m.st->n_own = n_own;
    m.st->n_seam = ns;
    m.st->go = go ? 1u : 0u;
    m.st->bad = 0;
    m.note[0] = m.note[1] = 0;
    if (go) {
        sd.state->n = seam_merged_count(n_own, d_total, s_total);
    } else {
        sd.state->n = 0;
        sd.state->scored = 0;
    }
    uint32_t *sm = (uint32_t *)m.summary;
    const uint32_t vals[8] = {scored ? 1u : 0u, go ? s_total : 0u, go ? d_total : 0u, scored && !go ? 1u : 0u, 0u, 0u, 0u, m.seq};
#pragma unroll
    for (int k = 0; k < 8; k++) host_store32(sm + k, vals[k]);   // seq last
}

__global__ __launch_bounds__(kMergeThreads) void k_seam_place(ScanParams p, SeamMergeParams m)
{
    TAIL_PRIO();
    const ScoreDev &sd = p.score, &md = m.merged;
    const uint32_t nb = p.n_chunks;
    const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x, gn = gridDim.x * blockDim.x;
    if (m.st->go) {
        const uint32_t n = m.st->n_own, ns = m.st->n_seam;
        for (uint32_t i = gi; i < n; i += gn) {
            const unsigned long long pos = sd.pos[i];
            const uint32_t b = (uint32_t)(pos >> 24), j = (uint32_t)pos & 0xFFFFFFu;
            if (j < kSeamLead || b >= nb) continue;
            const uint32_t at = seam_own_dst(i, m.own_shift[b]);
            if (at >= md.cap) continue;                // (cannot be: the prefix step counted)
            const uint4 *src = (const uint4 *)(sd.rec + i);
            uint4 *dst = (uint4 *)(md.rec + at);
            dst[0] = src[0], dst[1] = src[1];
            md.si[at] = sd.si[i];
            md.pos[at] = pos;
            md.slot[at] = 0xFFFFFFFFu;
        }
        for (uint32_t s = gi; s < ns; s += gn) {
            const TrialRecord r = m.seam_rec[s];
            const uint32_t b = r.chunk, key = seam_key(r.j_tp);
            if (b >= nb || key >= kSeamKeys) continue;   // (k_seam_mark has said so: go would be 0)
            const uint32_t at = seam_rec_dst(m.seam_base[b], m.present + (size_t)b * kSeamKeyStride, key);
            if (at >= md.cap) continue;
            md.rec[at] = r;
            md.si[at] = seam_classify(r);
            md.pos[at] = seam_pos(r);
            md.slot[at] = 0xFFFFFFFFu;
        }
    }
    // the last workgroup to finish leaves the presence rows and the drop counts zero for the slot's next pass (everybody's
    // reads of them have returned: their results went into the stores above)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __shared__ bool is_last;
    __syncthreads();
    if (threadIdx.x == 0) is_last = atomicAdd(&m.st->ticket, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!is_last) return;
    for (uint32_t k = threadIdx.x; k < nb * kSeamKeyStride; k += blockDim.x) m.present[k] = 0;
    for (uint32_t b = threadIdx.x; b < nb; b += blockDim.x) m.drop[b] = 0;
    if (threadIdx.x == 0) m.st->ticket = 0;
}

inline int hip_ok(hipError_t e) { return e == hipSuccess ? 0 : (int)e; }
inline void hip_clear() { (void)hipGetLastError(); }

}  // namespace

int launch_seam_merge(const ScanParams &p, const SeamMergeParams &m, void *stream)
{
    hip_clear();
    const ScoreDev &sd = p.score, &md = m.merged;
    if (!sd.si || !sd.rec || !sd.pos || !sd.slot || !sd.hash || !sd.state || p.n_chunks == 0) return (int)hipErrorInvalidValue;
    if (!md.si || !md.rec || !md.pos || !md.slot || !md.flag || md.cap != sd.cap || md.state != sd.state) return (int)hipErrorInvalidValue;
    if (!m.seam_rec || !m.seam_cap || !m.note || !m.present || !m.own_start || !m.drop || !m.seam_base || !m.own_shift || !m.st || !m.summary)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_seam_mark, dim3(kMergeBlocks), dim3(kMergeThreads), 0, (hipStream_t)stream, p, m);
    hipLaunchKernelGGL(k_seam_prefix, dim3(1), dim3(kMergeThreads), 0, (hipStream_t)stream, p, m);
    hipLaunchKernelGGL(k_seam_place, dim3(kMergeBlocks), dim3(kMergeThreads), 0, (hipStream_t)stream, p, m);
    return hip_ok(hipGetLastError());
}

}  // namespace adsb
