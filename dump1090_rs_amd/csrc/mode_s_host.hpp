// mode_s_host.hpp -- the sequential tail of the hot path, kept on the host.
//
// The ICAO address filter is the one piece of state in demodulate2400 that makes
// trial N depend on trial N-1 (scoring reads AND writes it: reference
// src/mode_s/mod.rs:71,80-84,97-104,115,130), so the device hands back the few
// trials that can matter and this file replays them in the reference's order.
// Semantics follow src/icao_filter.rs, src/crc.rs and src/mode_s/mod.rs; the state
// is per-context instead of process-global.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <vector>

namespace adsb {

// src/icao_filter.rs.  Table B of the reference is never written (only flushed),
// so probing it succeeds exactly for address 0 (an empty slot equals 0).
class IcaoFilter {
  public:
    static constexpr uint32_t kSize = 4096;           // :5
    static constexpr uint32_t kAdsbNt = 1u << 25;     // :6

    IcaoFilter() { flush(); }
    void flush() { table_.fill(0); }                  // :11-17

    static uint32_t hash(uint32_t addr)               // :19-43
    {
        uint64_t h = 0;
        const uint64_t a = addr;
        const uint64_t bytes[3] = {a & 0xff, (a >> 8) & 0xff, (a >> 16) & 0xff};
        for (uint64_t b : bytes) {
            h += b;
            h += h << 10;
            h ^= h >> 6;
        }
        h += h << 3;
        h ^= h >> 11;
        h += h << 15;
        return static_cast<uint32_t>(h) & (kSize - 1);
    }

    void add(uint32_t addr) { add(addr, hash(addr)); }  // :46-62
    // `start` = hash(addr), when the caller already has it (the device computes it per record)
    void add(uint32_t addr, uint32_t start)
    {
        uint32_t h = start;
        do {
            if (table_[h] == addr) return;
            if (table_[h] == 0) {
                table_[h] = addr;
                inserts_++;
                return;
            }
            h = (h + 1) & (kSize - 1);
        } while (h != start);
        // full: the reference prints "icao24 hash table full" and inserts nothing
    }

    bool test(uint32_t addr) const { return test(addr, hash(addr)); }  // :65-97
    bool test(uint32_t addr, uint32_t start) const
    {
        uint32_t h = start;
        while (table_[h] != 0 && table_[h] != addr) {
            h = (h + 1) & (kSize - 1);
            if (h == start) break;
        }
        return table_[h] == addr || addr == 0 /* table B */;
    }

    const std::array<uint32_t, kSize> &table() const { return table_; }
    // how many values add() has newly put into the table so far (never reset: callers compare)
    uint64_t inserts() const { return inserts_; }
    void load(const uint32_t *t) { std::memcpy(table_.data(), t, sizeof(uint32_t) * kSize); }
    void store(uint32_t *t) const { std::memcpy(t, table_.data(), sizeof(uint32_t) * kSize); }

  private:
    std::array<uint32_t, kSize> table_;
    uint64_t inserts_ = 0;
};

// src/crc.rs: Mode-S CRC-24, generator 0xFFF409.
struct Crc24 {
    uint32_t t[256];
    Crc24()
    {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i << 16;
            for (int k = 0; k < 8; k++) c = (c & 0x800000u) ? ((c << 1) ^ 0xFFF409u) : (c << 1);
            t[i] = c & 0xFFFFFFu;
        }
        set_fix(0);
    }
    // :263-282; residual = syndrome of the first n-3 bytes XOR the last three
    uint32_t residual(const uint8_t *m, int nbytes) const
    {
        uint32_t rem = 0;
        for (int i = 0; i < nbytes - 3; i++)
            rem = ((rem << 8) ^ t[m[i] ^ ((rem >> 16) & 0xff)]) & 0xFFFFFFu;
        return rem ^ (uint32_t(m[nbytes - 3]) << 16 | uint32_t(m[nbytes - 2]) << 8 | m[nbytes - 1]);
    }

    // Error correction of DF17/18 (adsb_set_error_correction): off (0, the reference), 1 (ADSB_FIX_1BIT) or 3
    // (ADSB_FIX_2BIT).  The one scoring option there is; it rides along with the table because every replay is handed both.
    int fix = 0;
    // syn112[b]: the residual of the 112-bit message with only bit b set (bit 0 = MSB of byte 0)
    uint32_t syn112[112];
    void set_fix(int mode)
    {
        fix = mode;
        uint8_t e[14];
        for (int b = 0; b < 112; b++) {
            std::memset(e, 0, sizeof e);
            e[b >> 3] = uint8_t(0x80u >> (b & 7));
            syn112[b] = residual(e, 14);
        }
        // ADSB_FIX_2BIT: syn(a) ^ syn(b) << 16 | a << 8 | b for 5 <= a < b <= 111, sorted (the 5671 values are distinct,
        // non-zero and none is a single bit's: tests/test_fix2_cpu.py), built once here
        pairs.clear();
        if (mode == 3) {
            pairs.reserve(5671);
            for (int a = 5; a < 112; a++)
                for (int b = a + 1; b < 112; b++)
                    pairs.push_back(uint64_t(syn112[a] ^ syn112[b]) << 16 | uint64_t(a) << 8 | uint64_t(b));
            std::sort(pairs.begin(), pairs.end());
        }
    }
    std::vector<uint64_t> pairs;
    // the bit in 5..111 whose syndrome `c` is (they are distinct: tests/test_fix_cpu.py), else -1; bits 0..4 are the DF
    int fix_bit(uint32_t c) const
    {
        for (int b = 5; b < 112; b++)
            if (syn112[b] == c) return b;
        return -1;
    }
    // the bits a < b in 5..111 whose syndromes XOR to `c` (mode 3 only), as a << 8 | b; else -1
    int fix_pair(uint32_t c) const
    {
        const auto it = std::lower_bound(pairs.begin(), pairs.end(), uint64_t(c) << 16);
        return it != pairs.end() && (*it >> 16) == c ? int(*it & 0xFFFFu) : -1;
    }
};

struct Score {
    bool some;    // false == the reference's None
    int len;      // 7 | 14
    int32_t value;
    int fix_bit = -1;   // >= 0: a DF17/18 repaired by flipping this message bit (ADSB_FIX_1BIT, scored 1200 or -1)
    int fix_bit2 = -1;  // >= 0: ... and this one too (ADSB_FIX_2BIT, scored 1100 or -1)
};

// a repaired message's bytes: the bits a Score flipped, flipped back
inline void apply_fix(const Score &s, uint8_t msg[14])
{
    if (s.fix_bit >= 0) msg[s.fix_bit >> 3] ^= (uint8_t)(0x80u >> (s.fix_bit & 7));
    if (s.fix_bit2 >= 0) msg[s.fix_bit2 >> 3] ^= (uint8_t)(0x80u >> (s.fix_bit2 & 7));
}

// src/mode_s/mod.rs:34-139 on a 14-byte trial message whose CRC residual (over its own length:
// 14 bytes for DF >= 16, else 7) is already known.
// `hash`: icao_hash of the value this message's DF asks the filter about (the residual for the
// address/parity DFs, the address for DF11/17/18) when the device supplied it, else -1.
// `Filter`: IcaoFilter, or a stand-in with the same test(addr, start) / add(addr, start) (the position-aware view of
// the parallel replay, adsb_replay_host.cpp).
// `fixer`: the Crc24 whose `fix` mode applies (null: none) -- the one branch it changes is DF17/18 with a non-zero residual.
template <class Filter>
inline Score score_modes_message(Filter &filter, uint32_t residual, const uint8_t msg[14], int hash = -1,
                                 const Crc24 *fixer = nullptr)
{
    const uint32_t df = msg[0] >> 3;                            // :41
    const int len = (df & 0x10) ? 14 : 7;                       // :42-46
    uint64_t w0, w1;                                            // :51-53 all 14 bytes zero -> None
    std::memcpy(&w0, msg, 8);
    std::memcpy(&w1, msg + 6, 8);
    if ((w0 | w1) == 0) return {false, len, 0};

    const uint32_t addr = uint32_t(msg[1]) << 16 | uint32_t(msg[2]) << 8 | msg[3];
    int32_t v = -2;
    switch (df) {
    case 0: case 4: case 5:                                     // :56-72
        v = filter.test(residual, hash >= 0 ? (uint32_t)hash : IcaoFilter::hash(residual)) ? 1000 : -1;
        break;
    case 11: {                                                  // :73-90
        const uint32_t c = residual;
        const uint32_t h = hash >= 0 ? (uint32_t)hash : IcaoFilter::hash(addr);
        const bool known = filter.test(addr, h);
        if ((c & 0xFFFF80u) != 0) {
            v = -2;
        } else if ((c & 0x7f) == 0) {
            if (known) {
                v = 1600;
            } else {
                filter.add(addr, h);
                v = 750;
            }
        } else {
            v = known ? 1000 : -1;
        }
        break;
    }
    case 17: case 18: {                                         // :91-109
        const uint32_t c = residual;
        const uint32_t h = hash >= 0 ? (uint32_t)hash : IcaoFilter::hash(addr);  // the hash takes 24 bits
        if (c != 0) {
            v = -2;
            // ADSB_FIX_1BIT: a residual that is the syndrome of one bit in 5..111 is that bit flipped.  The repaired
            // address is tested (DF18 too, with the plain address) and never added; `hash` is the damaged
            // address's, so it is not used.
            const int b = fixer && (fixer->fix & 1) ? fixer->fix_bit(c) : -1;
            if (b >= 0) {
                const uint32_t fixed = (b >= 8 && b < 32) ? addr ^ (1u << (31 - b)) : addr;
                return {true, len, filter.test(fixed, IcaoFilter::hash(fixed)) ? 1200 : -1, b};
            }
            // ADSB_FIX_2BIT: ... else a residual that is syn(a) ^ syn(b), 5 <= a < b <= 111, is those two bits
            // flipped (no residual names both a single bit and a pair), tested the same way, scored 1100
            const int ab = b < 0 && fixer && fixer->fix == 3 ? fixer->fix_pair(c) : -1;
            if (ab >= 0) {
                uint32_t fixed = addr;
                for (const int k : {ab >> 8, ab & 0xFF})
                    if (k >= 8 && k < 32) fixed ^= 1u << (31 - k);
                return {true, len, filter.test(fixed, IcaoFilter::hash(fixed)) ? 1100 : -1, ab >> 8, ab & 0xFF};
            }
        } else if (filter.test(addr, h)) {
            v = 1800;
        } else {
            filter.add(df == 17 ? addr : (addr | IcaoFilter::kAdsbNt), h);
            v = 1400;
        }
        break;
    }
    case 16: case 20: case 21:                                  // :110-120
    case 24: case 25: case 26: case 27: case 28: case 29: case 30: case 31:  // :121-135
        v = filter.test(residual, hash >= 0 ? (uint32_t)hash : IcaoFilter::hash(residual)) ? 1000 : -2;
        break;
    default:
        v = -2;                                                 // :136
    }
    return {true, len, v};
}

// ... computing the residual here (src/crc.rs:263-282)
template <class Filter>
inline Score score_modes_message(Filter &filter, const Crc24 &crc, const uint8_t msg[14])
{
    return score_modes_message(filter, crc.residual(msg, (msg[0] & 0x80) ? 14 : 7), msg, -1, &crc);
}

}  // namespace adsb
