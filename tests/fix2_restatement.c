/* fix2_restatement.c -- the CPU restatement of ADSB_FIX_2BIT (include/adsb_hip.h, "Error correction") that the tests
 * of two-bit repair compare the library with.  Test infrastructure, not part of the library: tests/fix2_support.py
 * compiles it with gcc against oracle/liboracle.so.
 *
 * As tests/fix_restatement.c: everything but one branch is the oracle's (orc_all_trials, orc_score_modes_message, the
 * reference's best-of-5 and signal level).  Only a DF17/18 trial with a non-zero residual c is restated.  Mode 1: c
 * equal to the syndrome of one bit b in 5..111 is that bit flipped (1200 if the repaired address is known, else -1).
 * Mode 3: the same, and otherwise c equal to syn(a) ^ syn(b), 5 <= a < b <= 111, is those two bits flipped (1100 if
 * the repaired address is known, else -1) -- found by a plain walk over the pairs.  A repaired trial adds nothing. */
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

/* the 5671 pair syndromes, in (a, b) order */
int fix2_pair_syndromes(uint32_t *out5671)
{
    init_syndromes();
    size_t k = 0;
    for (int a = 5; a < 112; a++)
        for (int b = a + 1; b < 112; b++) out5671[k++] = syn[a] ^ syn[b];
    return (int)k;
}

static void flip(uint8_t *m, int b) { m[b >> 3] ^= (uint8_t)(0x80u >> (b & 7)); }

/* one trial, scored as the library does in `mode`; returns 0 for None; fix[0], fix[1] = the repaired bits or -1 */
static int score_trial(orc_filter *f, const uint8_t *msg, int mode, int *len, int32_t *score, int fix[2])
{
    fix[0] = fix[1] = -1;
    const uint32_t df = msg[0] >> 3;
    if ((mode == 1 || mode == 3) && (df == 17 || df == 18)) {
        const uint32_t c = orc_modes_checksum(msg, 112);
        if (c != 0) {
            *len = 14;
            *score = -2;
            for (int b = 5; b < 112 && fix[0] < 0; b++)
                if (syn[b] == c) fix[0] = b;
            for (int a = 5; mode == 3 && fix[0] < 0 && a < 112; a++)
                for (int b = a + 1; b < 112; b++)
                    if ((syn[a] ^ syn[b]) == c) {
                        fix[0] = a;
                        fix[1] = b;
                        break;
                    }
            if (fix[0] >= 0) {
                uint8_t m2[14];
                memcpy(m2, msg, 14);
                flip(m2, fix[0]);
                if (fix[1] >= 0) flip(m2, fix[1]);
                const uint32_t addr = (uint32_t)orc_getbits(m2, 9, 32);
                *score = orc_icao_filter_test(f, addr) ? (fix[1] >= 0 ? 1100 : 1200) : -1;
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
        int best = -1, best_len = 7, best_fix[2] = {-1, -1};
        int32_t best_score = -2;
        for (size_t k = i; k < i + 5 && k < n; k++) {
            int len = 0, fix[2];
            int32_t score = 0;
            if (!score_trial(f, tr[k].msg, mode, &len, &score, fix)) continue;
            if (score > best_score) {
                best = (int)k;
                best_score = score;
                best_len = len;
                best_fix[0] = fix[0];
                best_fix[1] = fix[1];
            }
        }
        if (best < 0 || best_score < 0) continue;
        if (found < cap) {
            orc_msg *m = &out[found];
            memset(m, 0, sizeof *m);
            memcpy(m->msg, tr[best].msg, 14);
            if (best_fix[0] >= 0) flip(m->msg, best_fix[0]);
            if (best_fix[1] >= 0) flip(m->msg, best_fix[1]);
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
size_t fix2_demod_iq(orc_filter *f, const int16_t *iq_re_im, size_t n_samples, int mode, int16_t *carry, orc_msg *out,
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
size_t fix2_demodulate2400(orc_filter *f, const orc_magbuf *mb, int mode, orc_msg *out, size_t cap)
{
    init_syndromes();
    const size_t tr_cap = 5 * (size_t)ORC_MODES_MAG_BUF_SAMPLES;
    orc_trial *tr = (orc_trial *)malloc(tr_cap * sizeof(orc_trial));
    if (!tr) return 0;
    const size_t found = demod_buffer(f, mb, 0, mode, out, cap, tr, tr_cap);
    free(tr);
    return found;
}
