// adsb_seam_score_dev.h -- what the device-side seam merge (adsb_seam_score.hip: receiver seams scored on the device,
// adsb_set_receiver_carry_scoring) computes per record, stated once for the device and for the host: where a record of
// the merged pass lands, and how a seam record is classified for the keyed score kernels.  No HIP in here: plain g++
// builds it under the sanitizers (tests/seam_score_index_san.cpp).
//
// The merged pass holds, in (buffer, j, try_phase) order, every seam record of the pass and every own hit with
// j >= kSeamLead.  A seam record has j < kSeamLead, so within its buffer it sorts in front of every kept own hit, and the
// own hits a buffer drops are the first of its run.  With D(b) the own hits dropped and S(b) the seam records in buffers
// <= b (D(-1) = S(-1) = 0):
//   own hit i of buffer b (j >= kSeamLead)                  lands at i - D(b) + S(b)
//   the k-th seam record of buffer b in (j, try_phase) order  lands at ownstart(b) - D(b-1) + S(b-1) + k
// and k needs no sort: a buffer's seam records have distinct keys 5 j + try_phase - 4 < kSeamKeys, so k is the number of
// keys present below the record's own -- a popcount in the buffer's presence bitmap.
#pragma once
#include <stdint.h>

#include "adsb_record.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ADSB_SEAM_HD __host__ __device__
#else
#define ADSB_SEAM_HD
#endif

namespace adsb {

constexpr uint32_t kSeamLead = 326;                      // kLead (adsb_device.h), restated: no HIP in this header
constexpr uint32_t kSeamKeys = 5u * kSeamLead;           // 1630
constexpr uint32_t kSeamKeyWords = (kSeamKeys + 31u) / 32u;   // 51 words of presence bits per buffer ...
constexpr uint32_t kSeamKeyStride = 52;                  // ... in rows of 52 (8-byte aligned)

// the key of a seam record inside its buffer, or kSeamKeys: not a seam position (j >= kSeamLead, try_phase outside 4..8)
ADSB_SEAM_HD inline uint32_t seam_key(uint32_t j_tp)
{
    const uint32_t j = j_tp & 0xFFFFFFu, tp = j_tp >> 24;
    return j < kSeamLead && tp >= 4u && tp <= 8u ? 5u * j + tp - 4u : kSeamKeys;
}

ADSB_SEAM_HD inline uint32_t seam_popc(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(x);
#else
    return (uint32_t)__builtin_popcount(x);
#endif
}

// keys present below `key` in one buffer's row of the presence bitmap (key < kSeamKeys)
ADSB_SEAM_HD inline uint32_t seam_rank(const uint32_t *row, uint32_t key)
{
    uint32_t k = 0;
    for (uint32_t w = 0; w < (key >> 5); w++) k += seam_popc(row[w]);
    return k + seam_popc(row[key >> 5] & ((1u << (key & 31u)) - 1u));
}

// keys present in the row
ADSB_SEAM_HD inline uint32_t seam_row_count(const uint32_t *row)
{
    uint32_t k = 0;
    for (uint32_t w = 0; w < kSeamKeyWords; w++) k += seam_popc(row[w]);
    return k;
}

// What the prefix step leaves per buffer b, from ownstart(b), D and S as exclusive (before b) and inclusive sums:
//   seam_base(b)  where the buffer's first seam record lands
//   own_shift(b)  what is added to the index of a kept own hit of the buffer (two's complement: D may exceed S)
ADSB_SEAM_HD inline uint32_t seam_base_of(uint32_t ownstart, uint32_t d_before, uint32_t s_before) { return ownstart - d_before + s_before; }
ADSB_SEAM_HD inline uint32_t seam_own_shift(uint32_t d_upto, uint32_t s_upto) { return s_upto - d_upto; }
ADSB_SEAM_HD inline uint32_t seam_own_dst(uint32_t i, uint32_t own_shift) { return i + own_shift; }
ADSB_SEAM_HD inline uint32_t seam_rec_dst(uint32_t seam_base, const uint32_t *row, uint32_t key) { return seam_base + seam_rank(row, key); }
// the merged count, and whether the pass is scored at all: every seam record in hand, and room in the score arrays
ADSB_SEAM_HD inline uint32_t seam_merged_count(uint32_t n_own, uint32_t d_total, uint32_t s_total) { return n_own - d_total + s_total; }
ADSB_SEAM_HD inline bool seam_merge_fits(uint32_t n_own, uint32_t d_total, uint32_t s_total, uint32_t cap, uint32_t seam_overflow)
{
    return !seam_overflow && d_total <= n_own && (uint64_t)n_own - d_total + s_total <= cap;
}

// How the records kernel classifies a hit for the score kernels (adsb_tail_dev.h, records_block: ScoreDev::si = value |
// kind << 24), restated for a seam record, whose residual is bits 40..63 of `power` (k_seam_scan: pad = 1).  The kinds
// are ScoreKind's (adsb_device.h; adsb_seam_score.hip asserts they are).
enum SeamKind : uint32_t { kSeamSkOther = 0, kSeamSkApShort, kSeamSkApLong, kSeamSkDf11Iid0, kSeamSkDf11, kSeamSkDf17, kSeamSkDf18, kSeamSkNone };
ADSB_SEAM_HD inline uint32_t seam_classify(const uint8_t msg[14], uint32_t residual)
{
    uint32_t any = 0;
    for (int k = 0; k < 14; k++) any |= msg[k];
    const uint32_t df = (uint32_t)msg[0] >> 3;
    const bool lng = (msg[0] & 0x80u) != 0;
    const bool ap = ((0xFF310031u >> df) & 1u) != 0;    // DF 0, 4, 5, 16, 20, 21, 24..31: address/parity
    const uint32_t addr = (uint32_t)msg[1] << 16 | (uint32_t)msg[2] << 8 | msg[3];
    const bool d11 = df == 11u, d17 = df == 17u, d18 = df == 18u;
    const bool clean11 = d11 && (residual & 0xFFFF80u) == 0, iid0 = (residual & 0x7Fu) == 0;
    const bool clean17 = (d17 || d18) && residual == 0;
    uint32_t kind = kSeamSkOther;
    if (!any) kind = kSeamSkNone;
    else if (ap) kind = lng ? kSeamSkApLong : kSeamSkApShort;
    else if (clean11) kind = iid0 ? kSeamSkDf11Iid0 : kSeamSkDf11;
    else if (clean17) kind = d17 ? kSeamSkDf17 : kSeamSkDf18;
    return ((ap ? residual : addr) & 0xFFFFFFu) | kind << 24;
}
ADSB_SEAM_HD inline uint32_t seam_classify(const TrialRecord &r) { return seam_classify(r.msg, (uint32_t)(r.power >> 40) & 0xFFFFFFu); }
ADSB_SEAM_HD inline uint64_t seam_pos(const TrialRecord &r) { return (uint64_t)r.chunk << 24 | (r.j_tp & 0xFFFFFFu); }

}  // namespace adsb
