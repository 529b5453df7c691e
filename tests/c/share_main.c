/* The rule by which a channel keeps its gradient and its prob state in one buffer, and what a solver then counts as live
 * (j2p_geometry.h), for tests/test_share_state_cpu.py.  Every argument is one case, a word and numbers separated by
 * blanks; every case prints one line of numbers:
 *   "shares cw ch ws hs W H row0 row1 prob_on wide"            ->  shared crow0 crows
 *        (the channel's row window is the solver's own: j2p_row_window_of, arrays of the whole canvas)
 *   "live rows W limit [cw crows d_bytes shared] ..."          ->  working_set g planes d level
 *        (one group of four numbers per channel; level: j2p_nt_level against `limit` bytes of cache)
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
                unsigned long long v[MAX_NUMBERS] = {0};
                unsigned n = 0;
                int used = 0;
                if(sscanf(argv[i], "%15s%n", word, &used) != 1) { fprintf(stderr, "case %d: empty\n", i); return 2; }
                for(char *p = argv[i] + used, *end = p; n < MAX_NUMBERS; p = end, n++) {
                        const unsigned long long x = strtoull(p, &end, 10);
                        if(end == p) { break; }
                        v[n] = x;
                }
                if(strcmp(word, "shares") == 0 && n == 10 && v[0] && v[1] && v[2] && v[3]) {
                        j2p_row_window w = {0, 0, 0, 0};
                        (void)j2p_row_window_of((unsigned)v[1], (unsigned)v[3], (unsigned)v[5], (unsigned)v[6], (unsigned)v[7], 0, &w);
                        const int shared = j2p_shares_state((unsigned)v[0], (unsigned)v[2], (unsigned)v[3], w.crow0, (unsigned)v[4], (unsigned)v[6],
                                                            (int)v[8], (int)v[9]);
                        printf("%d %u %u\n", shared, w.crow0, w.crows);
                } else if(strcmp(word, "live") == 0 && n >= 7 && (n - 3) % 4 == 0) {
                        j2p_live_bytes l = {0, 0, 0, 0};
                        const size_t rows = (size_t)v[0], W = (size_t)v[1];
                        for(unsigned k = 3; k < n; k += 4) {
                                const size_t cells = (size_t)(v[k + 1] ? v[k + 1] : 1) * (size_t)v[k];
                                j2p_live_bytes_add(&l, (rows + 2 * J2P_HALO_ROWS) * W, rows * W, cells, (size_t)v[k + 2], (int)v[k + 3]);
                        }
                        printf("%zu %zu %zu %zu %d\n", l.working_set, l.g, l.planes, l.d, j2p_nt_level(&l, (size_t)v[2]));
                } else {
                        fprintf(stderr, "case %d: cannot read \"%s\"\n", i, argv[i]);
                        return 2;
                }
        }
        return 0;
}
