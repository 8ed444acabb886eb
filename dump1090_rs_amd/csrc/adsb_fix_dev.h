// adsb_fix_dev.h -- device code that finds the repair of a DF17/18 trial from its CRC residual (adsb_set_error_correction),
// shared by the scoring kernels (adsb_aux.hip: k_score / k_emit, the lookup self-test) and the reference-shaped scan
// (adsb_scan_simple.hip).  The tables are the ones every context uploads behind the GF(2) tables (adsb_device.h:
// kTabFixOff, kTabFix2Off; adsb_tables.h: build_fix_table, build_fix2_table), keyed by H' = x^-56 * residual.
#pragma once
#include "adsb_device.h"

namespace adsb {
namespace {

constexpr uint32_t kFixNoBit = 0xFFu;                          // "none" in either half of a repair
constexpr uint32_t kFixNoRepair = kFixNoBit | kFixNoBit << 8;

// a residual in the domain the tables are keyed in: H' = x^-56 * c in GF(2)[x]/g (56 steps of adsb_tables.h: gf_divx)
__device__ __forceinline__ uint32_t fix_key_of_residual(uint32_t c)
{
#pragma unroll
    for (int e = 0; e < 56; e++) c = (c & 1u) ? ((c ^ kCrcPoly) >> 1) | 0x800000u : c >> 1;
    return c;
}

// the single bit b in 5..111 whose key h is (one multiply, one load, one compare), else kFixNoBit; h != 0
__device__ __forceinline__ uint32_t fix1_probe(const uint32_t *tables, uint32_t h)
{
    const uint32_t *t = tables + kTabFixOff;
    const uint32_t e = t[(h * t[kFixSlots]) >> (32 - kFixLg)];
    return (e & 0xFFFFFFu) == h ? e >> 24 : kFixNoBit;
}

// the pair a < b in 5..111 whose key h is, as a | b << 8, else kFixNoRepair: the key's two buckets, two entries each --
// two independent 16-byte loads and four compares, no loop; h != 0 (an empty entry is {0, 0})
__device__ __forceinline__ uint32_t fix2_probe(const uint32_t *tables, uint32_t h)
{
    const uint32_t *t = tables + kTabFix2Off;
    const uint4 *bk = (const uint4 *)(t + 4);
    const uint4 q0 = bk[(h * t[0]) >> (32 - kFix2Lg)], q1 = bk[(h * t[1]) >> (32 - kFix2Lg)];
    uint32_t ab = kFixNoRepair;
    ab = (q0.x & 0xFFFFFFu) == h ? (q0.x >> 24) | (q0.y >> 24) << 8 : ab;
    ab = (q0.z & 0xFFFFFFu) == h ? (q0.z >> 24) | (q0.w >> 24) << 8 : ab;
    ab = (q1.x & 0xFFFFFFu) == h ? (q1.x >> 24) | (q1.y >> 24) << 8 : ab;
    ab = (q1.z & 0xFFFFFFu) == h ? (q1.z >> 24) | (q1.w >> 24) << 8 : ab;
    return ab;
}

// The repair the header defines for residual c under `mode` (ScanParams::fix), as a | b << 8:
//   c == syn(b), b in 5..111                          -> kFixNoBit | b << 8   (modes 1 and 3)
//   else c == syn(a) ^ syn(b), 5 <= a < b <= 111      -> a | b << 8           (mode 3 only)
//   else (c == 0 and mode 0 included)                 -> kFixNoRepair
__device__ __forceinline__ uint32_t fix_lookup(const uint32_t *tables, uint32_t c, uint32_t mode)
{
    c &= 0xFFFFFFu;
    if (c == 0u || !(mode & 1u)) return kFixNoRepair;
    const uint32_t h = fix_key_of_residual(c);
    const uint32_t b = fix1_probe(tables, h);
    if (b != kFixNoBit) return kFixNoBit | b << 8;
    return mode == 3u ? fix2_probe(tables, h) : kFixNoRepair;
}

// what flipping message bit k (or kFixNoBit) does to the address field, message bits 8..31
__device__ __forceinline__ uint32_t fix_addr_mask(uint32_t k) { return (k >= 8u && k < 32u) ? 1u << (31u - k) : 0u; }

}  // namespace
}  // namespace adsb
