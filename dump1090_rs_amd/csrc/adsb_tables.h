// adsb_tables.h -- GF(2) lookup tables for the Mode-S CRC-24 as the scan kernel computes it.
//
// The reference computes  residual = crc24(first n-3 bytes) XOR last 3 bytes
// (src/crc.rs:263-282), which is M(x) mod g(x) for the whole `bits`-bit message
// M(x) = sum_n bit_n * x^(bits-1-n), g(x) = x^24 + 0xFFF409.
//
// The scan kernel never assembles the message: it pulls, for each of the five bit
// classes r = n mod 5, one field f_r whose bit k is message bit n = 5k + r (those bits
// are 12 samples apart, which is how the sign planes are laid out).  With
// y = x^-5 mod g:
//     M(x) = sum_r x^(bits-1-r) * F(f_r),      F(f) = sum_k f[k] * y^k
//          = x^(bits-5) * H,                   H = sum_r x^(4-r) * F(f_r)   (Horner in x)
// The tables hold F' = x^51 * F (three 256-entry lookups, one per byte of the field), so
// H' = x^51 * H is the residual itself for 56-bit messages (DF11's test and the short
// address/parity trials need nothing more) and x^56 * H' for 112-bit ones; that constant
// multiplier is three more lookups, applied only in the match kernel.  A clean DF17/18 is
// simply H' == 0 (x is invertible mod g).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace adsb {

constexpr uint32_t kCrcPoly = 0xFFF409u;  // src/crc.rs: g(x) minus the x^24 term

// multiply by x in GF(2)[x]/g
inline uint32_t gf_mulx(uint32_t a)
{
    const uint32_t hi = a & 0x800000u;
    a = (a << 1) & 0xFFFFFFu;
    return hi ? a ^ kCrcPoly : a;
}
// multiply by x^-1 (g has constant term 1, so x is invertible)
inline uint32_t gf_divx(uint32_t a)
{
    return (a & 1u) ? ((a ^ kCrcPoly) >> 1) | 0x800000u : a >> 1;
}

// tables[t][v]: t = kTabF+b:   x^51 * sum of y^(8b+i) over set bits i of v
//               t = kTabX56+b: (v << 8b) * x^56
inline std::vector<uint32_t> build_gf_tables()
{
    std::vector<uint32_t> t(6 * 256, 0);
    // powers of y = x^-5
    uint32_t ypow[24];
    uint32_t p = 1;
    for (int e = 0; e < 51; e++) p = gf_mulx(p);  // x^51 folded into F
    for (int k = 0; k < 24; k++) {
        ypow[k] = p;
        for (int s = 0; s < 5; s++) p = gf_divx(p);
    }
    // x^56 * x^i for i = 0..23
    uint32_t x56[24];
    p = 1;
    for (int e = 0; e < 56; e++) p = gf_mulx(p);
    for (int i = 0; i < 24; i++, p = gf_mulx(p)) x56[i] = p;
    for (int b = 0; b < 3; b++)
        for (uint32_t v = 0; v < 256; v++) {
            uint32_t f = 0, a = 0;
            for (int i = 0; i < 8; i++)
                if (v & (1u << i)) {
                    f ^= ypow[8 * b + i];
                    a ^= x56[8 * b + i];
                }
            t[(0 + b) * 256 + v] = f;
            t[(3 + b) * 256 + v] = a;
        }
    return t;
}

// Reduction of x^24..x^27: R16[v] = sum of x^(24+i) over set bits i of v (16 entries).
inline std::vector<uint32_t> build_r16()
{
    uint32_t xp[4];
    uint32_t p = 1;
    for (int e = 0; e < 24; e++) p = gf_mulx(p);
    for (int i = 0; i < 4; i++, p = gf_mulx(p)) xp[i] = p;
    std::vector<uint32_t> r(16, 0);
    for (uint32_t v = 0; v < 16; v++)
        for (int i = 0; i < 4; i++)
            if (v & (1u << i)) r[v] ^= xp[i];
    return r;
}

// Per-bit residual constants for the records kernel: the residual of a message is the XOR of
// x^(bits-1-n) mod g over its set bits n (src/crc.rs:263-282 is M(x) mod g, see above).
// [0..112): x^(111-n) for 112-bit messages; [112..168): x^(55-n) for 56-bit ones.
inline std::vector<uint32_t> build_bit_residuals()
{
    std::vector<uint32_t> t(168, 0);
    uint32_t p = 1;
    for (int e = 0; e < 112; e++, p = gf_mulx(p)) {
        t[111 - e] = p;
        if (e < 56) t[112 + 55 - e] = p;
    }
    return t;
}

// Single-bit repair of DF17/18 (adsb_set_error_correction, ADSB_FIX_1BIT) on the device.  The scan knows a 112-bit
// trial's residual only as H' = x^-56 * residual (see the top of this file), so the table of the repairable
// syndromes is keyed in that domain: bit b (5..111) flipped leaves residual x^(111-b), i.e. H' = x^(55-b).
// A collision-free multiplicative hash, slot = (H' * mult) >> (32 - kFixLg), entry = H' | b << 24 (0: empty; H' of
// a repairable trial is never 0).  `mult` is the first odd number of a fixed xorshift sequence under which the 107
// keys land in distinct slots: deterministic, and re-derived wherever it is needed.
constexpr int kFixLg = 9, kFixSlots = 1 << kFixLg, kFixFirstBit = 5;

inline uint32_t fix_key(int b)   // H' of the 112-bit message with only bit b set
{
    uint32_t p = 1;
    for (int e = 0; e < 111 - b; e++) p = gf_mulx(p);
    for (int e = 0; e < 56; e++) p = gf_divx(p);
    return p;
}

inline uint32_t fix_slot(uint32_t key, uint32_t mult) { return (key * mult) >> (32 - kFixLg); }

// the table (kFixSlots u32) and its multiplier
inline std::vector<uint32_t> build_fix_table(uint32_t *mult_out)
{
    uint32_t key[112];
    for (int b = kFixFirstBit; b < 112; b++) key[b] = fix_key(b);
    uint32_t x = 0x9E3779B9u;
    std::vector<uint32_t> t(kFixSlots);
    for (;;) {
        x ^= x << 13;
        x ^= x >> 17;
        x ^= x << 5;
        const uint32_t mult = x | 1u;
        std::fill(t.begin(), t.end(), 0u);
        bool ok = true;
        for (int b = kFixFirstBit; b < 112 && ok; b++) {
            const uint32_t k = key[b], at = fix_slot(k, mult);
            ok = t[at] == 0;
            t[at] = k | (uint32_t)b << 24;
        }
        if (ok) {
            if (mult_out) *mult_out = mult;
            return t;
        }
    }
}

// Two-bit repair of DF17/18 (ADSB_FIX_2BIT) on the device: the 5671 pairs 5 <= a < b <= 111, keyed in the same
// domain, H'(a) ^ H'(b) = x^(55-a) + x^(55-b) (distinct, non-zero, and never a single bit's key: tests/test_fix2_cpu.py).
// Too many for LDS at the scan's occupancy, so the table lives in global memory (128 KB, which stays in L2) as a
// two-choice cuckoo hash: kFix2Buckets buckets of two 8-byte entries, one 16-byte load each; a key sits in bucket
// (key * mult_i) >> (32 - kFix2Lg) for i = 0 or 1.  A lookup is therefore exactly two independent 16-byte loads and
// four compares -- the probe bound kFix2Probes, no loop.  Entry = {key | a << 24, residual | b << 24}, the residual
// being syn(a) ^ syn(b) = x^(111-a) + x^(111-b), the value a repaired hit carries; {0, 0}: empty (no key is 0).
// Words: mult_0, mult_1, 0, 0 (16-byte alignment), then the buckets.  Deterministic: the multipliers are the first
// pair of a fixed xorshift sequence under which the insertions (in (a, b) order, evicting by a fixed rule) settle.
constexpr int kFix2Lg = 13, kFix2Buckets = 1 << kFix2Lg, kFix2Ways = 2, kFix2Probes = 2 * kFix2Ways, kFix2Pairs = 5671;
constexpr int kFix2Words = 4 + 4 * kFix2Buckets;

inline uint32_t fix2_bucket(uint32_t key, uint32_t mult) { return (key * mult) >> (32 - kFix2Lg); }

inline std::vector<uint32_t> build_fix2_table()
{
    std::vector<uint64_t> items;   // (key | a << 24) | (residual | b << 24) << 32
    items.reserve(kFix2Pairs);
    {
        uint32_t key[112], res[112];
        const std::vector<uint32_t> bits = build_bit_residuals();
        for (int b = kFixFirstBit; b < 112; b++) key[b] = fix_key(b), res[b] = bits[b];
        for (int a = kFixFirstBit; a < 112; a++)
            for (int b = a + 1; b < 112; b++)
                items.push_back((uint64_t)((key[a] ^ key[b]) | (uint32_t)a << 24) |
                                (uint64_t)((res[a] ^ res[b]) | (uint32_t)b << 24) << 32);
    }
    uint32_t x = 0x9E3779B9u;
    const auto next = [&x] {
        x ^= x << 13;
        x ^= x >> 17;
        x ^= x << 5;
        return x | 1u;
    };
    std::vector<uint64_t> slot((size_t)kFix2Buckets * kFix2Ways);
    for (;;) {
        const uint32_t m0 = next(), m1 = next();
        std::fill(slot.begin(), slot.end(), 0ull);
        bool ok = true;
        for (size_t i = 0; i < items.size() && ok; i++) {
            uint64_t cur = items[i];
            uint32_t at = fix2_bucket((uint32_t)cur & 0xFFFFFFu, m0);
            for (int kick = 0;; kick++) {
                int w = 0;
                while (w < kFix2Ways && slot[(size_t)at * kFix2Ways + w]) w++;
                if (w < kFix2Ways) {
                    slot[(size_t)at * kFix2Ways + w] = cur;
                    break;
                }
                if (kick == 500) {
                    ok = false;
                    break;
                }
                // full: the entry in way (kick % ways) moves to its other bucket
                std::swap(cur, slot[(size_t)at * kFix2Ways + kick % kFix2Ways]);
                const uint32_t k = (uint32_t)cur & 0xFFFFFFu, b0 = fix2_bucket(k, m0);
                at = b0 == at ? fix2_bucket(k, m1) : b0;
            }
        }
        if (!ok) continue;
        std::vector<uint32_t> t(kFix2Words, 0u);
        t[0] = m0;
        t[1] = m1;
        for (size_t s = 0; s < slot.size(); s++) {
            t[4 + 2 * s] = (uint32_t)slot[s];
            t[4 + 2 * s + 1] = (uint32_t)(slot[s] >> 32);
        }
        return t;
    }
}

// Field addressing of the fast scan's trial phase.  Message bit n = 5k + r of trial phase
// tp = 4 + tpi at a preamble whose LDS slot is 12*qs + rs sits in sign plane
// (ph, res), bit qs + carry + k, with
//     P = tp + 12r,  a = P / 5,  ph = P % 5,  res' = rs + 19 + a,  carry = res' / 12,  res = res' % 12
// (reference src/demod_2400.rs:158-182 in closed form).  Entry [tpi][r][rs] =
// byte offset of plane row (ph*12 + res) | carry << 16; plane rows are plane_bytes long.
inline std::vector<uint32_t> build_field_table(uint32_t plane_bytes)
{
    std::vector<uint32_t> t(5 * 5 * 12, 0);
    for (int tpi = 0; tpi < 5; tpi++)
        for (int r = 0; r < 5; r++)
            for (int rs = 0; rs < 12; rs++) {
                const int P = 4 + tpi + 12 * r, a = P / 5, ph = P % 5;
                const int rp = rs + 19 + a, carry = rp / 12, res = rp % 12;
                t[(tpi * 5 + r) * 12 + rs] = (uint32_t)((ph * 12 + res) * plane_bytes) | ((uint32_t)carry << 16);
            }
    return t;
}

}  // namespace adsb
