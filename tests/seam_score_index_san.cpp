// Sanitizer driver for the index arithmetic and the classification of the device-side seam merge
// (csrc/adsb_seam_score_dev.h, the header adsb_seam_score.hip's kernels are written with), a program of its own:
// tests/test_receiver_seams_scored_cpu.py builds it with -fsanitize=address,undefined and runs it directly.
// Seeded random passes -- 1-40 buffers, 0-30 own hits per buffer in (buffer, j, try_phase) order with some at j < 326,
// 0-12 seam records per buffer in any order, empty buffers, buffers with seam records only, the largest key 1629 -- go
// through the three steps the kernels take (mark, prefix, place), every array access checked by the sanitizer, and what
// comes out must be merge_seam_records' list (csrc/adsb_replay_host.cpp), record for record.  The rule for a pass that
// does not fit and the classification restatement are pinned against values written out by hand.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "../dump1090_rs_amd/csrc/adsb_replay_host.h"
#include "../dump1090_rs_amd/csrc/adsb_seam_score_dev.h"

using namespace adsb;
using namespace adsb::host;

namespace {

struct Merged {
    std::vector<TrialRecord> rec;
    std::vector<uint32_t> si;
    std::vector<uint64_t> pos;
    uint32_t n = 0, dropped = 0, taken = 0;
    bool fits = false;
};

// the kernels' three steps, on the host
Merged device_merge(const std::vector<TrialRecord> &own, const std::vector<TrialRecord> &seam, uint32_t nb, uint32_t cap)
{
    const uint32_t n = (uint32_t)own.size();
    std::vector<uint32_t> present((size_t)nb * kSeamKeyStride, 0u), own_start(nb + 1, 0xDEADu), drop(nb, 0u), base(nb), shift(nb);
    // mark
    if (n == 0) std::fill(own_start.begin(), own_start.end(), 0u);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t b = own[i].chunk, j = own[i].j_tp & 0xFFFFFFu;
        if (j < kSeamLead) drop[b]++;
        const uint32_t from = i ? own[i - 1].chunk + 1u : 0u;
        for (uint32_t k = from; k <= b; k++) own_start[k] = i;
        if (i == n - 1)
            for (uint32_t k = b + 1; k <= nb; k++) own_start[k] = n;
    }
    for (const TrialRecord &r : seam) {
        const uint32_t key = seam_key(r.j_tp);
        if (key >= kSeamKeys || r.chunk >= nb) std::abort();
        present[(size_t)r.chunk * kSeamKeyStride + (key >> 5)] |= 1u << (key & 31u);
    }
    // prefix
    uint32_t d_upto = 0, s_upto = 0;
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t s = seam_row_count(&present[(size_t)b * kSeamKeyStride]), d = drop[b];
        base[b] = seam_base_of(own_start[b], d_upto, s_upto);
        d_upto += d, s_upto += s;
        shift[b] = seam_own_shift(d_upto, s_upto);
    }
    Merged m;
    m.dropped = d_upto, m.taken = s_upto;
    m.fits = s_upto == seam.size() && seam_merge_fits(n, d_upto, s_upto, cap, 0);
    if (!m.fits) return m;
    m.n = seam_merged_count(n, d_upto, s_upto);
    // place: into arrays of exactly the merged count, every slot written exactly once
    m.rec.resize(m.n), m.si.assign(m.n, 0xFFFFFFFFu), m.pos.resize(m.n);
    std::vector<uint8_t> written(m.n, 0);
    for (uint32_t i = 0; i < n; i++) {
        if ((own[i].j_tp & 0xFFFFFFu) < kSeamLead) continue;
        const uint32_t at = seam_own_dst(i, shift[own[i].chunk]);
        m.rec.at(at) = own[i], m.pos.at(at) = seam_pos(own[i]), m.si.at(at) = 0u, written.at(at)++;
    }
    for (const TrialRecord &r : seam) {
        const uint32_t at = seam_rec_dst(base[r.chunk], &present[(size_t)r.chunk * kSeamKeyStride], seam_key(r.j_tp));
        m.rec.at(at) = r, m.pos.at(at) = seam_pos(r), m.si.at(at) = seam_classify(r), written.at(at)++;
    }
    for (uint8_t w : written)
        if (w != 1) std::abort();
    return m;
}

struct ClassCase {
    uint8_t msg[14];
    uint32_t residual, kind, value;
};

int check_classification()
{
    // (DF in the top five bits of byte 0, the address in bytes 1..3)
    const ClassCase cases[] = {
        {{0x8D, 0x4B, 0x1A, 0x2C, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, 0x000000, 5, 0x4B1A2C},   // DF17 clean: kSkDf17
        {{0x8D, 0x4B, 0x1A, 0x2C, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, 0x000400, 0, 0x4B1A2C},   // DF17 with a residual: kSkOther (a repair's)
        {{0x90, 0x4B, 0x1A, 0x2C, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, 0x000000, 6, 0x4B1A2C},   // DF18 clean: kSkDf18
        {{0x92, 0x4B, 0x1A, 0x2C, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, 0xFFF409, 0, 0x4B1A2C},   // DF18 with a residual: kSkOther
        {{0x5D, 0x3C, 0x65, 0x89, 1, 2, 3, 0, 0, 0, 0, 0, 0, 0}, 0x000000, 3, 0x3C6589},    // DF11 clean, IID 0: kSkDf11Iid0
        {{0x5D, 0x3C, 0x65, 0x89, 1, 2, 3, 0, 0, 0, 0, 0, 0, 0}, 0x00007F, 4, 0x3C6589},    // DF11 clean, IID 127: kSkDf11
        {{0x5D, 0x3C, 0x65, 0x89, 1, 2, 3, 0, 0, 0, 0, 0, 0, 0}, 0x000080, 0, 0x3C6589},    // DF11 not clean: kSkOther
        {{0x00, 0x11, 0x22, 0x33, 1, 2, 3, 9, 9, 9, 9, 9, 9, 9}, 0xA1B2C3, 1, 0xA1B2C3},    // DF0: kSkApShort, the residual
        {{0x20, 0x11, 0x22, 0x33, 1, 2, 3, 0, 0, 0, 0, 0, 0, 0}, 0x4B1A2C, 1, 0x4B1A2C},    // DF4
        {{0x28, 0x11, 0x22, 0x33, 1, 2, 3, 0, 0, 0, 0, 0, 0, 0}, 0x000000, 1, 0x000000},    // DF5, address 0
        {{0x80, 0x11, 0x22, 0x33, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, 0x06A0AF, 2, 0x06A0AF},   // DF16: kSkApLong
        {{0xA0, 0x11, 0x22, 0x33, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, 0x06A0AF, 2, 0x06A0AF},   // DF20
        {{0xA8, 0x11, 0x22, 0x33, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, 0xFFFFFF, 2, 0xFFFFFF},   // DF21
        {{0xC0, 0x11, 0x22, 0x33, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, 0x123456, 2, 0x123456},   // DF24
        {{0xFF, 0x11, 0x22, 0x33, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, 0x123456, 2, 0x123456},   // DF31
        {{0x98, 0x4B, 0x1A, 0x2C, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, 0x000000, 0, 0x4B1A2C},   // DF19: kSkOther, whatever the residual
        {{0x08, 0x4B, 0x1A, 0x2C, 1, 2, 3, 0, 0, 0, 0, 0, 0, 0}, 0x000000, 0, 0x4B1A2C},    // DF1: kSkOther
        {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, 0x000000, 7, 0x000000},                // all zero: kSkNone
        {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, 0x000001, 1, 0x000001},                // DF0 with one bit: a trial again
    };
    std::set<uint32_t> kinds;
    for (const ClassCase &c : cases) {
        const uint32_t w = seam_classify(c.msg, c.residual);
        if (w != (c.value | c.kind << 24)) {
            std::printf("classification: DF %u residual %06x -> %08x, not kind %u value %06x\n", c.msg[0] >> 3, c.residual, w, c.kind, c.value);
            return 1;
        }
        kinds.insert(c.kind);
        // ... and from a record as k_seam_scan writes it: the residual above the 40 bits of the power
        TrialRecord r;
        std::memset(&r, 0, sizeof r);
        std::memcpy(r.msg, c.msg, 14);
        r.power = (uint64_t)c.residual << 40 | 0x3FFFFFFFFFull;
        r.pad = 1;
        if (seam_classify(r) != w) return 1;
    }
    return kinds.size() == 8 ? 0 : 1;   // every ScoreKind
}

int check_limits()
{
    // the largest key, the keys that are none, and the rule for a pass that does not fit
    if (seam_key(325u | 8u << 24) != 1629u || kSeamKeys != 1630u || kSeamKeyWords != 51u || kSeamKeyStride < kSeamKeyWords) return 1;
    if (seam_key(0u | 4u << 24) != 0u || seam_key(326u | 4u << 24) != kSeamKeys || seam_key(5u | 3u << 24) != kSeamKeys ||
        seam_key(5u | 9u << 24) != kSeamKeys)
        return 1;
    if (!seam_merge_fits(100, 10, 10, 100, 0) || seam_merge_fits(100, 10, 11, 100, 0) || seam_merge_fits(100, 10, 10, 100, 1) ||
        seam_merge_fits(100, 10, 10, 100, 2) || !seam_merge_fits(0, 0, 100, 100, 0) || seam_merge_fits(0, 0, 101, 100, 0) ||
        seam_merge_fits(5, 6, 0, 100, 0) || !seam_merge_fits(0xFFFFFFFFu, 0, 0, 0xFFFFFFFFu, 0) || seam_merge_fits(0xFFFFFFFFu, 0, 1, 0xFFFFFFFFu, 0))
        return 1;
    return seam_merged_count(100, 10, 7) == 97u ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 600;
    if (check_classification()) return 10;
    if (check_limits()) return 11;
    std::mt19937_64 rng(20261021);
    size_t merged_total = 0, dropped_total = 0, seam_total = 0, empty_buffers = 0, seam_only = 0, max_key = 0, too_many = 0;
    for (int round = 0; round < rounds; round++) {
        const uint32_t nb = 1 + (uint32_t)(rng() % 40);
        std::vector<TrialRecord> own, seam;
        for (uint32_t b = 0; b < nb; b++) {
            const uint32_t shape = (uint32_t)(rng() % 6);   // 0: an empty buffer, 1: seam records only
            const uint32_t n_own = shape <= 1 ? 0 : (uint32_t)(rng() % 31), n_seam = shape == 0 ? 0 : (uint32_t)(rng() % 13);
            empty_buffers += shape == 0 || (n_own == 0 && n_seam == 0), seam_only += n_own == 0 && n_seam > 0;
            std::vector<uint32_t> keys;   // (j, try_phase) of the own hits: any, repeats allowed across try_phase only
            std::set<uint32_t> used;
            while (keys.size() < n_own) {
                const uint32_t j = rng() % 3 == 0 ? (uint32_t)(rng() % 326) : 326u + (uint32_t)(rng() % 130746);
                const uint32_t k = j << 3 | (uint32_t)(rng() % 5);
                if (used.insert(k).second) keys.push_back(k);
            }
            std::sort(keys.begin(), keys.end());
            for (uint32_t k : keys) {
                TrialRecord r;
                std::memset(&r, 0, sizeof r);
                r.chunk = b, r.j_tp = (k >> 3) | (4u + (k & 7u)) << 24;
                for (auto &x : r.msg) x = (uint8_t)rng();
                r.power = rng() & ((1ull << 38) - 1);
                r.pad = 3;
                own.push_back(r);
            }
            used.clear();
            if (n_seam && rng() % 4 == 0) used.insert(1629u);   // the largest key
            while (used.size() < n_seam) used.insert((uint32_t)(rng() % kSeamKeys));
            std::vector<uint32_t> sk(used.begin(), used.end());
            std::shuffle(sk.begin(), sk.end(), rng);            // the seam's records come in any order
            for (uint32_t k : sk) {
                TrialRecord r;
                std::memset(&r, 0, sizeof r);
                r.chunk = b, r.j_tp = (k / 5u) | (4u + k % 5u) << 24;
                for (auto &x : r.msg) x = (uint8_t)rng();
                r.power = (rng() & ((1ull << 38) - 1)) | (rng() & 0xFFFFFFull) << 40;
                r.pad = 1;
                seam.push_back(r);
                max_key += k == 1629u;
            }
        }
        std::shuffle(seam.begin(), seam.end(), rng);            // ... and across buffers too
        std::vector<TrialRecord> want;
        uint64_t dropped = 0, taken = 0;
        merge_seam_records(own.data(), own.size(), seam.data(), seam.size(), 0, nb, 326, want, &dropped, &taken);
        const Merged m = device_merge(own, seam, nb, (uint32_t)want.size());
        if (!m.fits || m.n != want.size() || m.dropped != dropped || m.taken != taken ||
            (m.n && std::memcmp(m.rec.data(), want.data(), want.size() * sizeof(TrialRecord)) != 0)) {
            std::printf("round %d: the placement differs (%u records against %zu)\n", round, m.n, want.size());
            return 2;
        }
        for (uint32_t i = 0; i < m.n; i++) {
            const bool is_seam = want[i].pad == 1;
            if (m.pos[i] != ((uint64_t)want[i].chunk << 24 | (want[i].j_tp & 0xFFFFFFu)) || (is_seam && m.si[i] != seam_classify(want[i])) ||
                (is_seam != ((want[i].j_tp & 0xFFFFFFu) < 326u)))
                return 3;
        }
        // one hit more than the score arrays hold: the pass is not scored (nothing is placed)
        if (!want.empty()) {
            const Merged over = device_merge(own, seam, nb, (uint32_t)want.size() - 1);
            if (over.fits || over.n != 0 || !over.rec.empty()) return 4;
            too_many++;
        }
        merged_total += m.n, dropped_total += dropped, seam_total += taken;
    }
    std::printf("seam score index ok: %d rounds, %zu records placed, %zu dropped, %zu seam records, %zu empty buffers, %zu buffers with seam "
                "records only, %zu times the largest key, %zu passes that did not fit\n",
                rounds, merged_total, dropped_total, seam_total, empty_buffers, seam_only, max_key, too_many);
    return merged_total > 10000 && dropped_total > 1000 && seam_total > 1000 && empty_buffers > 100 && seam_only > 100 && max_key > 50 && too_many > 100
               ? 0 : 5;
}
