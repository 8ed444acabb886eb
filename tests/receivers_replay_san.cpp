// Sanitizer driver for the per-receiver replay (csrc/adsb_replay_host.h: ReceiverReplay over a ReplayPool), a program of
// its own: tests/test_receivers_cpu.py builds it once with -fsanitize=address,undefined and once with -fsanitize=thread and
// runs it directly.  Seeded random captures of trial records for a handful of receivers (a few aircraft they share; DF17 /
// DF18 / DF11 with clean and with broken CRCs, damaged DF17s for the repair modes, address/parity replies, duplicates, records
// out of order) are replayed twice -- one walk over the records, and the receivers dealt to the threads of ONE pool --
// with filters that carry over from capture to capture, single receivers flushed now and then, and one receiver that is fed
// new aircraft until its 4096-slot table is full and on past that: the same messages, the same tables, and no report from
// the sanitizer.  The ABI entry (adsb_replay_records_rx) takes a capture now and then, with pools of its own.
#include <cstdio>
#include <cstring>
#include <random>

#include "../dump1090_rs_amd/csrc/adsb_replay_host.h"

using namespace adsb;
using namespace adsb::host;

static void crc_fix(const Crc24 &crc, uint8_t *m, int nbytes, uint32_t xor_with)
{
    m[nbytes - 3] = m[nbytes - 2] = m[nbytes - 1] = 0;
    const uint32_t c = crc.residual(m, nbytes) ^ xor_with;
    m[nbytes - 3] = (uint8_t)(c >> 16), m[nbytes - 2] = (uint8_t)(c >> 8), m[nbytes - 1] = (uint8_t)c;
}

int main(int argc, char **argv)
{
    const int captures = argc > 1 ? std::atoi(argv[1]) : 120;
    std::mt19937_64 rng(20261018);
    constexpr uint32_t kReceivers = 9, kFiller = 8;   // receiver 8 hears a new aircraft in almost every frame
    constexpr uint32_t kBuffers = 24;
    std::vector<uint32_t> aircraft;
    for (int k = 0; k < 40; k++) aircraft.push_back((uint32_t)(rng() % 0xFFFFFEu) + 1);
    static const uint32_t dfs[] = {0, 4, 5, 11, 11, 16, 17, 17, 17, 18, 20, 21, 24, 1};
    std::vector<IcaoFilter> serial(kReceivers), pooled(kReceivers);
    std::vector<IcaoFilter *> serial_of, pooled_of;
    for (uint32_t r = 0; r < kReceivers; r++) serial_of.push_back(&serial[r]), pooled_of.push_back(&pooled[r]);
    ReplayPool pool(5, {}, 0);
    ReceiverReplay one_walk, dealt;
    size_t total_msgs = 0, went_pooled = 0, gained_n = 0, full_n = 0;
    uint32_t next_new = 0x100000;
    for (int cap = 0; cap < captures; cap++) {
        Crc24 crc;
        const int mode = cap % 3 == 0 ? 0 : (cap % 3 == 1 ? 1 : 3);
        crc.set_fix(mode);
        if (rng() % 5 == 0) {   // adsb_icao_flush_receiver
            const uint32_t r = (uint32_t)(rng() % kReceivers);
            serial[r].flush(), pooled[r].flush();
        }
        if (rng() % 40 == 0)   // adsb_icao_flush
            for (uint32_t r = 0; r < kReceivers; r++) serial[r].flush(), pooled[r].flush();
        // the map: mostly all receivers, now and then one or two only
        uint32_t map[kBuffers];
        const uint32_t present = rng() % 6 == 0 ? 1 + (uint32_t)(rng() % 2) : kReceivers;
        const uint32_t base = (uint32_t)(rng() % kReceivers);
        for (uint32_t b = 0; b < kBuffers; b++) map[b] = (base + (uint32_t)(rng() % present)) % kReceivers;
        std::vector<TrialRecord> rec;
        const size_t n = rng() % 6000;
        for (size_t i = 0; i < n; i++) {
            TrialRecord r{};
            r.chunk = (uint32_t)(rng() % kBuffers);
            const bool filler = map[r.chunk] == kFiller && rng() % 4 != 0;
            const uint32_t df = filler ? 17u : dfs[rng() % (sizeof(dfs) / sizeof(dfs[0]))];
            for (auto &b : r.msg) b = (uint8_t)rng();
            r.msg[0] = (uint8_t)(df << 3 | (rng() & 7));
            const int nbytes = df >= 16 ? 14 : 7;
            const uint32_t a = filler ? next_new++ : aircraft[rng() % aircraft.size()];
            if ((df == 11 || df == 17 || df == 18) && (filler || rng() % 10 < 8)) {
                r.msg[1] = (uint8_t)(a >> 16), r.msg[2] = (uint8_t)(a >> 8), r.msg[3] = (uint8_t)a;
                crc_fix(crc, r.msg, nbytes, df == 11 && rng() % 4 == 0 ? (uint32_t)(rng() % 127 + 1) : 0u);
                if ((df == 17 || df == 18) && rng() % 5 == 0) {   // one or two bits damaged: a repair under modes 1 / 3
                    for (int flips = 1 + (int)(rng() % 2); flips > 0; flips--) {
                        const int bit = 5 + (int)(rng() % 107);
                        r.msg[bit >> 3] ^= (uint8_t)(0x80u >> (bit & 7));
                    }
                }
            } else if (rng() % 10 < 5) {
                crc_fix(crc, r.msg, nbytes, a);   // an address/parity frame for one of the aircraft
            }
            r.j_tp = (uint32_t)(rng() % 131072) | (uint32_t)(4 + rng() % 5) << 24;
            r.power = rng() & ((1ull << 38) - 1);
            if (rng() & 1) {   // as the device hands them over: residual and hash along
                const uint32_t c = crc.residual(r.msg, (r.msg[0] & 0x80) ? 14 : 7);
                const bool ap = ((0xFF310031u >> df) & 1u) != 0;
                const uint32_t addr = uint32_t(r.msg[1]) << 16 | uint32_t(r.msg[2]) << 8 | r.msg[3];
                r.power |= (uint64_t)c << 40;
                r.pad = (uint16_t)(3u | IcaoFilter::hash(ap ? c : addr) << 4);
            }
            rec.push_back(r);
            if (rng() % 9 == 0) rec.push_back(r);   // twice
        }
        if (rng() & 1) {   // in replay order, as a large pass hands them over
            std::vector<TrialRecord> sorted;
            if (sort_records(rec.data(), rec.size(), sorted)) rec.swap(sorted);
        }
        std::vector<adsb_msg> want, got;
        bool gained_a = false, gained_b = false, was_pooled = false;
        uint64_t sorts_a = 0, sorts_b = 0;
        if (!one_walk.run(serial_of.data(), map, kBuffers, crc, rec.data(), rec.size(), 0, want, nullptr, &sorts_a, &gained_a)) return 3;
        if (cap % 10 == 9) {
            // through the ABI: tables in, tables out, a pool of its own
            std::vector<uint32_t> tables((size_t)kReceivers * IcaoFilter::kSize);
            for (uint32_t r = 0; r < kReceivers; r++) pooled[r].store(tables.data() + (size_t)r * IcaoFilter::kSize);
            size_t n_out = 0;
            got.resize(rec.size() + 1);
            const int rc = adsb_replay_records_rx(tables.data(), kReceivers, map, kBuffers, reinterpret_cast<adsb_trial *>(rec.data()),
                                                  rec.size(), mode, 2 + (int)(rng() % 6), got.data(), got.size(), &n_out);
            if (rc != ADSB_OK) return 4;
            got.resize(n_out);
            for (uint32_t r = 0; r < kReceivers; r++) pooled[r].load(tables.data() + (size_t)r * IcaoFilter::kSize);
            gained_b = gained_a, sorts_b = sorts_a;
        } else {
            if (!dealt.run(pooled_of.data(), map, kBuffers, crc, rec.data(), rec.size(), 0, got, &pool, &sorts_b, &gained_b, &was_pooled)) return 3;
            if (present == kReceivers && rec.size() > 200 && !was_pooled) return 5;   // (several receivers present: the pool's)
        }
        went_pooled += was_pooled;
        gained_n += gained_a;
        bool same = want.size() == got.size() && (want.empty() || std::memcmp(want.data(), got.data(), want.size() * sizeof(adsb_msg)) == 0) &&
                    gained_a == gained_b && sorts_a == sorts_b;
        for (uint32_t r = 0; r < kReceivers && same; r++) same = serial[r].table() == pooled[r].table();
        if (!same) {
            std::printf("capture %d: the dealt replay differs from the one walk (%zu messages against %zu)\n", cap, got.size(), want.size());
            return 1;
        }
        total_msgs += want.size();
        size_t held = 0;
        for (uint32_t v : serial[kFiller].table()) held += v != 0;
        full_n += held == IcaoFilter::kSize;   // (replayed with its table full: add() gives up, test() walks all of it)
        // a record whose buffer lies outside the map is refused before anything is replayed
        if (!rec.empty() && cap % 17 == 0) {
            std::vector<adsb_msg> none;
            const auto before = serial[map[0]].table();
            if (one_walk.run(serial_of.data(), map, rec[0].chunk, crc, rec.data(), rec.size(), 0, none, &pool) || !none.empty() ||
                before != serial[map[0]].table())
                return 6;
        }
    }
    std::printf("receiver replay ok: %d captures, %zu messages, %zu dealt to the pool, %zu gained an address, receiver %u ended %zu with a full table\n",
                captures, total_msgs, went_pooled, gained_n, kFiller, full_n);
    return went_pooled * 2 > (size_t)captures && total_msgs > 1000 && full_n > 2 ? 0 : 2;
}
