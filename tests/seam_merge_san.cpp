// Sanitizer driver for the host code of receiver seams (csrc/adsb_replay_host.h: seam_prev_map, merge_seam_records), a
// program of its own: tests/test_receiver_seams_cpu.py builds it with -fsanitize=address,undefined and runs it directly.
// Seeded random maps and record sets: the previous-buffer map against a quadratic restatement (and its scratch left all
// -1), the merge against a restatement written the other way round, for whole passes and for the one-buffer windows of
// the overflow fallback, and the merged records through the per-receiver replay.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../dump1090_rs_amd/csrc/adsb_replay_host.h"

using namespace adsb;
using namespace adsb::host;

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 400;
    std::mt19937_64 rng(20261021);
    std::vector<int32_t> latest;
    size_t merged_total = 0, dropped_total = 0, chained = 0, messages = 0, sorted_total = 0;
    for (int round = 0; round < rounds; round++) {
        const uint32_t n_receivers = 1 + (uint32_t)(rng() % (round % 7 == 0 ? 16384 : 9));
        const size_t n_buffers = (size_t)(rng() % 70);
        std::vector<uint32_t> map(n_buffers), last(n_buffers, 7u);
        std::vector<int32_t> prev(n_buffers, 7);
        for (auto &m : map) m = (uint32_t)(rng() % std::min<uint32_t>(n_receivers, 1 + (uint32_t)(rng() % 12)));
        if (!seam_prev_map(map.data(), n_buffers, n_receivers, latest, prev.data(), last.data())) return 3;
        for (size_t b = 0; b < n_buffers; b++) {
            int32_t want_prev = -1;
            uint32_t want_last = 1;
            for (size_t k = 0; k < b; k++)
                if (map[k] == map[b]) want_prev = (int32_t)k;
            for (size_t k = b + 1; k < n_buffers; k++)
                if (map[k] == map[b]) want_last = 0;
            if (prev[b] != want_prev || last[b] != want_last) {
                std::printf("round %d: buffer %zu has prev %d / last %u, not %d / %u\n", round, b, prev[b], last[b], want_prev, want_last);
                return 1;
            }
            chained += want_prev >= 0;
        }
        for (int32_t v : latest)
            if (v != -1) return 4;   // (the scratch is left as it was found)
        if (n_buffers) {   // an entry outside the receivers: refused, nothing written
            std::vector<uint32_t> bad(map);
            bad[rng() % n_buffers] = n_receivers + (uint32_t)(rng() % 3);
            std::vector<int32_t> p2(n_buffers, 7);
            std::vector<uint32_t> l2(n_buffers, 7u);
            if (seam_prev_map(bad.data(), n_buffers, n_receivers, latest, p2.data(), l2.data())) return 5;
            for (size_t b = 0; b < n_buffers; b++)
                if (p2[b] != 7 || l2[b] != 7u) return 5;
        }
        // the merge: a pass's records (chunk relative to `first`) and the seam's records of the whole pass
        const uint64_t first = n_buffers ? rng() % n_buffers : 0, window = std::min<uint64_t>(round % 3 == 0 ? 1 : n_buffers, n_buffers - first);
        std::vector<TrialRecord> pass(rng() % 300), seam(rng() % 200), out(3), want;
        for (auto &r : pass) {
            std::memset(&r, 0, sizeof r);
            r.chunk = (uint32_t)(window ? rng() % window : 0);
            r.j_tp = (uint32_t)(rng() % 4 == 0 ? rng() % 326 : 326 + rng() % 130746) | (uint32_t)(4 + rng() % 5) << 24;
            for (auto &b : r.msg) b = (uint8_t)rng();
            r.power = rng() & ((1ull << 38) - 1);
        }
        const auto key = [](const TrialRecord &r) { return (uint64_t)r.chunk << 32 | (uint64_t)(r.j_tp & 0xFFFFFFu) << 8 | (r.j_tp >> 24); };
        const auto before = [&](const TrialRecord &a, const TrialRecord &b) { return key(a) < key(b); };
        const bool in_order = round % 2 == 0;   // as a dense pass hands its records over
        if (in_order) std::stable_sort(pass.begin(), pass.end(), before);
        for (auto &r : seam) {
            std::memset(&r, 0, sizeof r);
            r.chunk = (uint32_t)(rng() % (n_buffers + 1));
            r.j_tp = (uint32_t)(rng() % 326) | (uint32_t)(4 + rng() % 5) << 24;
            for (auto &b : r.msg) b = (uint8_t)rng();
            r.power = rng() & ((1ull << 38) - 1);
        }
        uint64_t dropped = 0, taken = 0, want_dropped = 0, want_taken = 0;
        merge_seam_records(pass.data(), pass.size(), seam.data(), seam.size(), first, window, 326, out, &dropped, &taken);
        for (const auto &r : pass)
            if ((r.j_tp & 0xFFFFFFu) >= 326) want.push_back(r);
            else want_dropped++;
        for (auto r : seam)
            if (r.chunk >= first && r.chunk < first + window) {
                r.chunk -= (uint32_t)first;
                want.push_back(r);
                want_taken++;
            }
        // the same records, in (chunk, j, try_phase) order where the pass's came in order, else the seam's behind the pass's
        const bool pass_sorted = std::is_sorted(want.begin(), want.begin() + (long)(want.size() - want_taken), before);
        if (in_order && !pass_sorted) return 7;
        if (pass_sorted && want_taken) {
            if (!std::is_sorted(out.begin(), out.end(), before)) return 8;
            const auto bytes = [](const TrialRecord &a, const TrialRecord &b) { return std::memcmp(&a, &b, sizeof a) < 0; };
            std::sort(out.begin(), out.end(), bytes);
            std::sort(want.begin(), want.end(), bytes);
            sorted_total++;
        }
        if (out.size() != want.size() || dropped != want_dropped || taken != want_taken ||
            (!want.empty() && std::memcmp(out.data(), want.data(), want.size() * sizeof(TrialRecord)) != 0)) {
            std::printf("round %d: the merge differs (%zu records against %zu)\n", round, out.size(), want.size());
            return 2;
        }
        merged_total += out.size(), dropped_total += dropped;
        // ... and through the replay, buffer by buffer against the receivers' filters (every chunk is inside the window)
        if (window && n_receivers <= 64) {
            std::vector<IcaoFilter> filters(n_receivers);
            std::vector<IcaoFilter *> of;
            for (auto &f : filters) of.push_back(&f);
            Crc24 crc;
            ReceiverReplay replay;
            std::vector<adsb_msg> msgs;
            if (!replay.run(of.data(), map.data(), map.size(), crc, out.data(), out.size(), first, msgs, nullptr)) return 6;
            messages += msgs.size();
        }
    }
    std::printf("seam merge ok: %d rounds, %zu records merged, %zu dropped, %zu buffers with a previous one, %zu messages\n", rounds,
                merged_total, dropped_total, chained, messages);
    return merged_total > 1000 && dropped_total > 1000 && chained > 1000 && sorted_total > 50 ? 0 : 2;
}
