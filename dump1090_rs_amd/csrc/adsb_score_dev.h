// adsb_score_dev.h -- what the two scoring kernels (adsb_aux.hip: k_score, one filter; adsb_score_rx.hip: k_score_rx,
// one filter per receiver) share: the score of one trial, src/mode_s/mod.rs:56-135.  The only thing that differs between
// them is the question "is value v in the filter when trial i is scored", which each hands in as `in_filter(v, i)`.
#pragma once
#include "../../include/adsb_hip.h"
#include "adsb_device.h"
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

}  // namespace adsb
