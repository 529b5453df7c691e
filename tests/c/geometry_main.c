/* What the functions of j2p_geometry.h return, for tests/test_geometry_cpu.py.  Every argument is one case, a word and
 * numbers separated by blanks; every case prints one line of numbers:
 *   "canvas w h w_samp h_samp [w h w_samp h_samp ...]"  ->  W H align min_band_rows
 *   "cuts units nband align"                            ->  edge[0] ... edge[nband-1], or "refused"
 *   "schedule W H band_rows nchannel"                   ->  strips rpw zone_d zone_b zone_c
 *   "window ch hs H row0 row1 band_local"               ->  covers crow0 crows frow0 frows
 * Includes nothing of the library but that header. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "j2p_geometry.h"

#define MAX_NUMBERS 16

int main(int argc, char **argv)
{
        for(int i = 1; i < argc; i++) {
                char word[16] = "";
                unsigned v[MAX_NUMBERS] = {0}, n = 0;
                int used = 0;
                if(sscanf(argv[i], "%15s%n", word, &used) != 1) { fprintf(stderr, "case %d: empty\n", i); return 2; }
                for(char *p = argv[i] + used, *end = p; n < MAX_NUMBERS; p = end, n++) {
                        const unsigned long x = strtoul(p, &end, 10);
                        if(end == p) { break; }
                        v[n] = (unsigned)x;
                }
                if(strcmp(word, "canvas") == 0 && n >= 4 && n % 4 == 0) {
                        j2p_canvas cv = J2P_CANVAS_NONE;
                        for(unsigned k = 0; k < n; k += 4) { j2p_canvas_add(&cv, v[k], v[k + 1], v[k + 2], v[k + 3]); }
                        printf("%u %u %u %u\n", cv.W, cv.H, cv.align, j2p_min_band_rows(cv.align));
                } else if(strcmp(word, "cuts") == 0 && n == 3 && v[1] <= 65536) {
                        unsigned *edge = malloc((v[1] ? v[1] : 1) * sizeof(unsigned));
                        if(!edge) { return 2; }
                        const int cut = j2p_near_equal_cuts(v[0], v[1], v[2], edge);
                        if(!cut) { printf("refused\n"); }
                        for(unsigned b = 0; cut && b < v[1]; b++) { printf("%u%c", edge[b], b + 1 < v[1] ? ' ' : '\n'); }
                        free(edge);
                } else if(strcmp(word, "schedule") == 0 && n == 4) {
                        const j2p_strip_schedule p = j2p_strip_schedule_of(v[0], v[1], v[2], v[3]);
                        printf("%u %u %u %u %u\n", p.strips, p.rpw, p.zone_d, p.zone_b, p.zone_c);
                } else if(strcmp(word, "window") == 0 && n == 6) {
                        j2p_row_window w = {0, 0, 0, 0};
                        const int covers = j2p_row_window_of(v[0], v[1], v[2], v[3], v[4], (int)v[5], &w);
                        printf("%d %u %u %u %u\n", covers, w.crow0, w.crows, w.frow0, w.frows);
                } else {
                        fprintf(stderr, "case %d: cannot read \"%s\"\n", i, argv[i]);
                        return 2;
                }
        }
        return 0;
}
