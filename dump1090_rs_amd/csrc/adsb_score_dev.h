// adsb_score_dev.h -- everything the scoring kernels of a plain pass (adsb_aux.hip: k_score / k_emit, one filter) and of a
// receivers pass (adsb_score_rx.hip: k_score_rx / k_emit_rx, one filter per receiver) share, which is all but their filters:
//   score_trial / score_repair   the score of one trial, src/mode_s/mod.rs:56-135
//   flag_pack, flag_*            the one place that knows the layout of ScoreDev::flag
//   score_body                   a whole k_score: best of the trials of a position, the flags, the per-block totals
//   emit_message                 the adsb_msg of an emitted record, repaired where its flag says so
//   emit_body                    a whole k_emit: messages and additions out in order, the tables left empty, the summary
// The kernels themselves are thin wrappers that hand in what differs.  To the score: "is value v in the filter when trial
// i is scored", a functor `in_filter(v, i)`, made per position.  To the emit: a commit policy of five hooks (emit_body).
// And to both the block size, `block`: blockDim.x read in here, in a device function, compiles to a load per lane where
// the kernel's own read is one scalar load.
#pragma once
#include "../../include/adsb_hip.h"
#include "adsb_device.h"
#include "adsb_tail_dev.h"
#include "adsb_fix_dev.h"

namespace adsb {

// A trial the record builder left unclassified (kSkOther) in a pass that repairs (ScanParams::fix, include/adsb_hip.h:
// adsb_set_error_correction): a DF17/18 whose residual c -- bits 40..63 of its record's `power` -- names one flipped bit,
// or (mode 3) two, scores 1200 / 1100 when the REPAIRED address is in the filter at that moment (DF18 too, with the
// plain address), else -1; it adds nothing and is no adder in the hash.  `damaged`: the address field as sliced.
// Everything else stays -2.  Only such trials come here: the common kinds never see the lookup.
// *repair: the bits found, a | b << 8 (k_emit flips them; it gets them through ScoreDev::flag and looks nothing up).
template <class InFilter>
__device__ __forceinline__ int score_repair(const ScoreDev &sd, uint32_t i, uint32_t damaged, const uint32_t *tables, uint32_t fix,
                                            uint32_t *repair, const InFilter &in_filter)
{
    const TrialRecord &r = sd.rec[i];
    const uint32_t df = (uint32_t)r.msg[0] >> 3;
    if (df != 17u && df != 18u) return -2;
    const uint32_t ab = fix_lookup(tables, (uint32_t)(r.power >> 40), fix);
    if (ab == kFixNoRepair) return -2;
    *repair = ab;
    const uint32_t a = ab & 0xFFu, b = ab >> 8;
    const uint32_t addr = damaged ^ fix_addr_mask(a) ^ fix_addr_mask(b);
    if (!in_filter(addr, i)) return -1;
    return a == kFixNoBit ? ADSB_SCORE_FIXED_1BIT : ADSB_SCORE_FIXED_2BIT;
}

// src/mode_s/mod.rs:56-135 for trial i; *adds: the value this trial hands to icao_filter_add (or 0)
template <class InFilter>
__device__ __forceinline__ int score_trial(const ScoreDev &sd, uint32_t i, uint32_t *adds, const uint32_t *tables, uint32_t fix,
                                           uint32_t *repair, const InFilter &in_filter)
{
    const uint32_t w = sd.si[i], v = w & 0xFFFFFFu, kind = w >> 24;
    *adds = 0;
    switch (kind) {
    case kSkApShort: return in_filter(v, i) ? 1000 : -1;
    case kSkApLong: return in_filter(v, i) ? 1000 : -2;
    case kSkDf11: return in_filter(v, i) ? 1000 : -1;
    case kSkDf11Iid0:
        if (in_filter(v, i)) return 1600;
        *adds = v;
        return 750;
    case kSkDf17:
        if (in_filter(v, i)) return 1800;
        *adds = v;
        return 1400;
    case kSkDf18:
        if (in_filter(v, i)) return 1800;
        *adds = v | (1u << 25);                       // ICAO_FILTER_ADSB_NT, src/icao_filter.rs:6
        return 1400;
    case kSkNone: return -3;                          // the reference's None: never taken
    case kSkOther: return fix ? score_repair(sd, i, v, tables, fix, repair, in_filter) : -2;
    default: return -2;
    }
}

// ---- ScoreDev::flag, one word per trial from the score kernel to the emit kernel ----
//   bit 0        this trial is the one its (buffer, j) emits
//   bit 1        it adds its address to the filter
//   bits 8..18   its score + 3
// and for a repaired trial (score_repair: a | b << 8) the bits found ride along: b in bits 25..31; a in bits 19..24 and
// bit 2 -- kFixNoBit & 127 for a single bit, which the score tells apart.  (Zero there for every other trial: never read.)
__device__ __forceinline__ uint32_t flag_pack(bool emit, bool adds, int score, uint32_t repair)
{
    const uint32_t fa = repair & 0x7Fu, fb = (repair >> 8) & 0x7Fu;
    return (emit ? 1u : 0u) | (adds ? 2u : 0u) | ((uint32_t)(score + 3) << 8) | (fa >> 6) << 2 | (fa & 63u) << 19 | fb << 25;
}
__device__ __forceinline__ uint32_t flag_emit(uint32_t f) { return f & 1u; }
__device__ __forceinline__ uint32_t flag_adds(uint32_t f) { return (f >> 1) & 1u; }
__device__ __forceinline__ int32_t flag_score(uint32_t f) { return (int32_t)((f >> 8) & 0x7FFu) - 3; }
__device__ __forceinline__ uint32_t flag_fix_a(uint32_t f) { return ((f >> 19) & 63u) | ((f >> 2) & 1u) << 6; }
__device__ __forceinline__ uint32_t flag_fix_b(uint32_t f) { return f >> 25; }

// k_score / k_score_rx: one thread per hit.  Its own score, whether it is the one its (buffer, j) emits
// (src/demod_2400.rs:149-207: strictly greater wins, from -2; emitted when >= 0) and what it adds.
// filter_at(pos): the in_filter functor for the trials at position pos (one position is one buffer: one receiver).
template <class FilterAt>
__device__ __forceinline__ void score_body(const ScanParams &p, const FilterAt &filter_at, uint32_t block)
{
    const ScoreDev &sd = p.score;
    const uint32_t n = sd.state->n;
    const uint32_t per = (n + gridDim.x - 1) / gridDim.x;
    const uint32_t first = blockIdx.x * per, last = min(n, first + per);
    uint32_t emits = 0, addc = 0;
    for (uint32_t i = first + threadIdx.x; i < last; i += block) {
        const uint64_t pos = sd.pos[i];
        const auto in_filter = filter_at(pos);
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
        sd.flag[i] = flag_pack(emit, my_add != 0, mine, my_fix);
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

// The message of record r, emitted with flag f.  A repaired one carries the corrected bytes (the two repair scores occur
// nowhere else; the bits the score kernel found are in the flag); the record in memory stays as sliced, with its
// residual: a host that cannot use this result repairs it itself.
__device__ __forceinline__ void emit_message(adsb_msg &m, const TrialRecord &r, uint32_t f)
{
    for (int k = 0; k < 14; k++) m.msg[k] = r.msg[k];
    m.score = flag_score(f);
    if (m.score == ADSB_SCORE_FIXED_1BIT || m.score == ADSB_SCORE_FIXED_2BIT) {
        const uint32_t fb = flag_fix_b(f), fa = m.score == ADSB_SCORE_FIXED_2BIT ? flag_fix_a(f) : kFixNoBit;
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
}

// k_emit / k_emit_rx: the messages and the additions in order (block b writes behind what blocks < b write), the
// additions committed to the filter the next pass scores against, the first-adder tables left empty, the summary last.
// What "the filter" is comes in as the commit policy `c`, five hooks and nothing else:
//   c.clear_retired()            an icao_flush preceded this pass: it scores against the other (empty) filter; the one
//                                the passes before it used is emptied here, for the flush after this one
//   c.commit(at, i, v, keep)     trial i's addition is the at-th of the pass: anything that goes out beside sd.out_adds,
//                                and (keep: all but DF18's) v into the filter, visible to later passes only.  False: no room
//   c.forget(i)                  trial i's slot in a first-adder table of the policy's own, back to empty
//   c.out_of_probes()            the last block's look at whether any insertion of the pass had no room (the summary then
//                                says scored = 0, and so)
//   c.reset_state()              the last block: the policy's own word of sd.state back to zero
template <class Commit>
__device__ __forceinline__ void emit_body(const ScanParams &p, const Commit &c, uint32_t block)
{
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
    c.clear_retired(blockIdx.x * block + threadIdx.x, gridDim.x * block);
    adsb_msg *out = (adsb_msg *)sd.out_msgs;
    unsigned long long my_sum = 0;
    bool no_room = false;
    for (uint32_t i0 = first; i0 < last; i0 += block) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t f = i < last ? sd.flag[i] : 0u;
        {
            // inclusive scan of the two flags over the block: ballots inside a wave, four wave totals
            const uint32_t ln = threadIdx.x & 63u, wv = threadIdx.x >> 6;
            const unsigned long long m0 = __ballot(flag_emit(f)), m1 = __ballot(flag_adds(f));
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
            if (flag_emit(f)) {
                adsb_msg m;
                emit_message(m, r, f);
                // staged: the block's messages of this round are contiguous in the output, so they leave as consecutive
                // 8-byte words from consecutive lanes (separate 8-byte writes to host memory from one lane each cost
                // ~30 ns apiece)
                const unsigned long long *mw = (const unsigned long long *)&m;
                unsigned long long *sw = stage + 5u * (scan[0][threadIdx.x] - 1u);
#pragma unroll
                for (int k = 0; k < 5; k++) sw[k] = mw[k];
            }
            if (flag_adds(f)) {
                const uint32_t val = kind == kSkDf18 ? (v | (1u << 25)) : v;
                const uint32_t at = base[1] + scan[1][threadIdx.x] - 1u;
                host_store32(sd.out_adds + at, val);
                if (!c.commit(at, i, v, kind != kSkDf18)) no_room = true;
            }
            // leave the first-adder tables empty for the next pass, of either kind: every adder resets the slot its key
            // sits in (remembered at insertion; probes only happen in the score kernels, which have finished)
            const uint32_t hs = sd.slot[i];
            if (hs != 0xFFFFFFFFu) sd.hash[hs] = ~0ull;
            c.forget(i);
        }
        __syncthreads();
        {
            const uint32_t words = 5u * scan[0][255];
            unsigned long long *ow = (unsigned long long *)(out + base[0]);
            for (uint32_t w = threadIdx.x; w < words; w += block) {
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
        uint32_t nm = threadIdx.x < gridDim.x ? sd.blk[2 * threadIdx.x] : 0u;   // kScoreBlocks == block
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
        // (whoever ran out of probes said so before its block counted in)
        const uint32_t out_of_probes = c.out_of_probes();
        uint32_t *sm = (uint32_t *)sd.summary;
        const uint32_t vals[8] = {nm, na, (uint32_t)ms, (uint32_t)(ms >> 32), out_of_probes ? 0u : sd.state->scored, out_of_probes, 0u, sd.seq};
#pragma unroll
        for (int k = 0; k < 8; k++) host_store32(sm + k, vals[k]);
        sd.state->n = 0;
        sd.state->scored = 0;
        sd.state->blocks_done = 0;
        c.reset_state();
        sd.state->msg_sum = 0;
    }
}

}  // namespace adsb
