/* fix_restatement.c -- the CPU restatement of ADSB_FIX_1BIT (include/adsb_hip.h, "Error correction") that the tests
 * of single-bit repair compare the library with.  Test infrastructure, not part of the library: tests/test_fix_cpu.py
 * and tests/test_gpu_fix.py compile it with gcc against oracle/liboracle.so.
 *
 * Everything but the one new branch is the oracle's: orc_all_trials gives the five unscored trials of every gated j
 * with their power, orc_score_modes_message scores them, and this file keeps the reference's best-of-5 (strict >
 * from -2, emitted when >= 0; src/demod_2400.rs:149-207) and signal level.  Only a DF17/18 trial with a non-zero
 * residual is restated: in mode 1 a residual equal to the syndrome of one bit b in 5..111 is that bit flipped; the
 * repaired address is tested (never added) and scores 1200, else -1. */
#include <stdlib.h>
#include <string.h>

#include "dump1090_oracle.h"

static uint32_t syn[112];

static void init_syndromes(void)
{
    for (int b = 0; b < 112; b++) {
        uint8_t e[14] = {0};
        e[b >> 3] = (uint8_t)(0x80u >> (b & 7));
        syn[b] = orc_modes_checksum(e, 112);
    }
}

int fix_syndrome_table(uint32_t *out112)
{
    init_syndromes();
    memcpy(out112, syn, sizeof syn);
    return 0;
}

/* one trial, scored as the library does in `mode`; returns 0 for None; *fixbit = the repaired bit or -1 */
static int score_trial(orc_filter *f, const uint8_t *msg, int mode, int *len, int32_t *score, int *fixbit)
{
    *fixbit = -1;
    const uint32_t df = msg[0] >> 3;
    if (mode == 1 && (df == 17 || df == 18)) {
        const uint32_t c = orc_modes_checksum(msg, 112);
        if (c != 0) {
            *len = 14;
            *score = -2;
            for (int b = 5; b < 112; b++)
                if (syn[b] == c) {
                    uint8_t m2[14];
                    memcpy(m2, msg, 14);
                    m2[b >> 3] ^= (uint8_t)(0x80u >> (b & 7));
                    const uint32_t addr = (uint32_t)orc_getbits(m2, 9, 32);
                    *score = orc_icao_filter_test(f, addr) ? 1200 : -1;
                    *fixbit = b;
                    break;
                }
            return 1;
        }
    }
    return orc_score_modes_message(f, msg, 14, len, score);
}

/* demodulate2400 of one magnitude buffer in `mode` (the reference's when mode == 0) */
static size_t demod_buffer(orc_filter *f, const orc_magbuf *mb, uint64_t chunk, int mode, orc_msg *out, size_t cap,
                           orc_trial *tr, size_t tr_cap)
{
    const size_t n = orc_all_trials(mb, chunk, tr, tr_cap);
    size_t found = 0;
    for (size_t i = 0; i < n; i += 5) {
        int best = -1, best_len = 7, best_fix = -1;
        int32_t best_score = -2;
        for (size_t k = i; k < i + 5 && k < n; k++) {
            int len = 0, fixbit = -1;
            int32_t score = 0;
            if (!score_trial(f, tr[k].msg, mode, &len, &score, &fixbit)) continue;
            if (score > best_score) {
                best = (int)k;
                best_score = score;
                best_len = len;
                best_fix = fixbit;
            }
        }
        if (best < 0 || best_score < 0) continue;
        if (found < cap) {
            orc_msg *m = &out[found];
            memset(m, 0, sizeof *m);
            memcpy(m->msg, tr[best].msg, 14);
            if (best_fix >= 0) m->msg[best_fix >> 3] ^= (uint8_t)(0x80u >> (best_fix & 7));
            m->len = (uint8_t)best_len;
            m->try_phase = (uint8_t)(tr[best].j_tp >> 24);
            m->score = best_score;
            m->j = tr[best].j_tp & 0xFFFFFFu;
            m->chunk = chunk;
            const double signal_power = (double)tr[best].power / 65535.0 / 65535.0;
            m->signal_level = signal_power / 33.0;
        }
        found++;
    }
    return found;
}

/* orc_demod_iq (carry == NULL) or orc_demod_iq_carry (carry: the stream's last 326 IQ samples, updated) in `mode` */
size_t fix_demod_iq(orc_filter *f, const int16_t *iq_re_im, size_t n_samples, int mode, int16_t *carry, orc_msg *out,
                    size_t cap)
{
    init_syndromes();
    orc_magbuf *mb = (orc_magbuf *)malloc(sizeof(orc_magbuf));
    const size_t tr_cap = 5 * (size_t)ORC_MODES_MAG_BUF_SAMPLES;
    orc_trial *tr = (orc_trial *)malloc(tr_cap * sizeof(orc_trial));
    if (!mb || !tr) {
        free(mb);
        free(tr);
        return 0;
    }
    size_t found = 0;
    uint64_t chunk = 0;
    for (size_t off = 0; off < n_samples; off += ORC_MODES_MAG_BUF_SAMPLES, chunk++) {
        size_t n = n_samples - off;
        if (n > ORC_MODES_MAG_BUF_SAMPLES) n = ORC_MODES_MAG_BUF_SAMPLES;
        orc_to_mag(iq_re_im + 2 * off, n, mb);
        if (carry)
            for (size_t d = 1; d <= ORC_TRAILING_SAMPLES; d++) {
                const int16_t *s = off >= d ? iq_re_im + 2 * (off - d) : carry + 2 * (ORC_TRAILING_SAMPLES - (d - off));
                mb->data[ORC_TRAILING_SAMPLES - d] = orc_mag_sample(s[0], s[1]);
            }
        const size_t room = found < cap ? cap - found : 0;
        found += demod_buffer(f, mb, chunk, mode, out + (found < cap ? found : cap), room, tr, tr_cap);
    }
    if (carry) {
        if (n_samples >= ORC_TRAILING_SAMPLES) {
            memcpy(carry, iq_re_im + 2 * (n_samples - ORC_TRAILING_SAMPLES), 2 * ORC_TRAILING_SAMPLES * sizeof(int16_t));
        } else if (n_samples) {
            memmove(carry, carry + 2 * n_samples, 2 * (ORC_TRAILING_SAMPLES - n_samples) * sizeof(int16_t));
            memcpy(carry + 2 * (ORC_TRAILING_SAMPLES - n_samples), iq_re_im, 2 * n_samples * sizeof(int16_t));
        }
    }
    free(tr);
    free(mb);
    return found;
}

/* one caller-supplied magnitude buffer (adsb_demodulate2400) in `mode` */
size_t fix_demodulate2400(orc_filter *f, const orc_magbuf *mb, int mode, orc_msg *out, size_t cap)
{
    init_syndromes();
    const size_t tr_cap = 5 * (size_t)ORC_MODES_MAG_BUF_SAMPLES;
    orc_trial *tr = (orc_trial *)malloc(tr_cap * sizeof(orc_trial));
    if (!tr) return 0;
    const size_t found = demod_buffer(f, mb, 0, mode, out, cap, tr, tr_cap);
    free(tr);
    return found;
}
