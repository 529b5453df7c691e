// jpeg2png_amd — the table estimator's host half: a quantisation table from the histogram j2p_samples_histogram makes.  Pure C,
// integer arithmetic only, no device and no library: the rule of include/jpeg2png_amd.h ("Estimated tables"), which
// tests/estimate_cases.py restates.  j2p_quant_estimate (compute_host.c) is this function.
#pragma once
#include <stdint.h>
#include <string.h>

#include "jpeg2png_amd.h"

#define J2P_EST_BINS 1024
#define J2P_EST_QMIN 4                  /* the smallest step the search tries: below it "within 1 of a multiple" says nothing */
#define J2P_EST_SMALL_DIVISOR 4         /* steps 3 and 2: at most nz / 4 of the values of 2 and more are no exact multiple */
#define J2P_EST_QMAX 255
#define J2P_EST_SLACK_PERCENT 5         /* of the values of 2 and more may lie further than 1 from a multiple */
#define J2P_EST_MIN_VALUES 12           /* values of 2 and more that a determined entry needs */

// Annex K's tables in natural order and the IJG scaling of jpeg_set_quality(quality, TRUE): what quality_tables makes
static const uint8_t j2p_est_base[2][64] = {
        {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
        {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99},
};

static inline int j2p_est_ijg(int chroma, int quality, int j)
{
        const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
        const int v = (j2p_est_base[chroma ? 1 : 0][j] * scale + 50) / 100;
        return v < 1 ? 1 : (v > 255 ? 255 : v);
}

// distance of m to the nearest multiple of q
static inline int j2p_est_distance(int m, int q)
{
        const int r = m % q;
        return r < q - r ? r : q - r;
}

// the largest q of 255..4 that leaves at most 5 % of the values of `lo` and more further than 1 from its multiples, or 0
static inline int j2p_est_search(const uint32_t h[J2P_EST_BINS], int lo, int mmax)
{
        uint64_t n = 0;
        for(int m = lo; m <= mmax; m++) { n += h[m]; }
        const uint64_t allowed = J2P_EST_SLACK_PERCENT * n / 100;
        for(int q = J2P_EST_QMAX; q >= J2P_EST_QMIN; q--) {
                uint64_t off = 0;
                for(int m = lo; m <= mmax && off <= allowed; m++) {
                        if(h[m] && j2p_est_distance(m, q) > 1) { off += h[m]; }
                }
                if(off <= allowed) { return q; }
        }
        return 0;
}

// one frequency's step from its 1024 counts, or 0 when the rule names none; *nz: its values of 2 and more
static inline int j2p_est_step(const uint32_t h[J2P_EST_BINS], uint64_t *nz)
{
        uint64_t n = 0;
        int mmax = 0;
        for(int m = 2; m < J2P_EST_BINS; m++) {
                n += h[m];
                if(h[m]) { mmax = m; }
        }
        *nz = n;
        const int qmax = j2p_est_search(h, 2, mmax);
        if(!qmax) {
                // a large step whose zeros' noise reaches 2 and 3 (the values of 4 and more have a step): not named
                if(j2p_est_search(h, 4, mmax)) { return 0; }
                // no step of 4 or more: 3 or 2 when all but a quarter of the values are its exact multiples, otherwise 1
                int s = 1;
                for(int q = 3; q >= 2 && s == 1; q--) {
                        uint64_t off = 0;
                        for(int m = 2; m <= mmax; m++) {
                                if(m % q) { off += h[m]; }
                        }
                        if(off <= n / J2P_EST_SMALL_DIVISOR) { s = q; }
                }
                // ... and only where the counts repeat with that period: half the values or more lie where the histogram and
                // itself moved by s overlap.  Clusters around the multiples of a large step do not
                uint64_t overlap = 0;
                for(int m = 2; m + s <= mmax; m++) { overlap += h[m] < h[m + s] ? h[m] : h[m + s]; }
                return 2 * overlap >= n ? s : 0;
        }
        int best = 0;
        uint64_t best_cost = 0;
        for(int q = qmax; q >= J2P_EST_QMIN && q > qmax - 3; q--) {
                uint64_t cost = 0;
                for(int m = 2; m <= mmax; m++) {
                        const int d = j2p_est_distance(m, q);
                        cost += (uint64_t)h[m] * (uint64_t)(d >= 2 ? 4 : d);          /* min(d, 2)^2 */
                }
                if(!best || cost < best_cost) { best = q, best_cost = cost; }         /* ties: the larger q */
        }
        return best;
}

static inline int j2p_quant_estimate_rule(const uint32_t hist[64][J2P_EST_BINS], int chroma, j2p_quant_estimate_result *out)
{
        if(!hist || !out) { return -1; }
        memset(out, 0, sizeof(*out));
        int step[64], ndet = 0;
        for(int j = 0; j < 64; j++) {
                uint64_t nz = 0;
                step[j] = j2p_est_step(hist[j], &nz);
                out->determined[j] = step[j] && nz >= J2P_EST_MIN_VALUES ? 1 : 0;
                ndet += out->determined[j];
        }
        // the IJG quality whose table lies nearest the determined entries; ties: the higher quality; nothing determined: 100
        int quality = 100;
        if(ndet) {
                long best = -1;
                for(int q = 100; q >= 1; q--) {
                        long sum = 0;
                        for(int j = 0; j < 64; j++) {
                                if(out->determined[j]) {
                                        const int d = j2p_est_ijg(chroma, q, j) - step[j];
                                        sum += d < 0 ? -d : d;
                                }
                        }
                        if(best < 0 || sum < best) { best = sum, quality = q; }
                }
        }
        out->quality = quality;
        for(int j = 0; j < 64; j++) {
                int v = step[j];
                if(!out->determined[j]) {
                        // the box of a coefficient taken as 0 must hold the largest magnitude seen
                        int mmax = 0;
                        for(int m = 0; m < J2P_EST_BINS; m++) { if(hist[j][m]) { mmax = m; } }
                        const int floor_ = 2 * (mmax - 1);
                        v = j2p_est_ijg(chroma, quality, j);
                        if(floor_ > v) { v = floor_; }
                }
                out->table[j] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
        return 0;
}
