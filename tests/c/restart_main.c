/* Stand-alone driver of jpeg2png_amd/csrc/j2p_restart.h, the restart plan of a JPEG file the library writes, for
 * tests/test_restart_cpu.py: no device, no library — the header alone, so that it can be built with the address and
 * undefined-behaviour sanitizers.
 * stdin: one file per line — width height ncomp sub_w sub_h progressive N R.
 * stdout: per line "refused" for arguments j2p_restart_error refuses, or nscans and the markers of the whole file, then per scan
 * units units_per_row interval intervals dri. */
#include <stdio.h>

#include "j2p_restart.h"

int main(void)
{
        unsigned w, h, ncomp, sub_w, sub_h, progressive, n, r;
        while(scanf("%u %u %u %u %u %u %u %u", &w, &h, &ncomp, &sub_w, &sub_h, &progressive, &n, &r) == 8) {
                if(j2p_restart_error(n, r)) {
                        printf("refused\n");
                        continue;
                }
                const j2p_restart_plan p = j2p_restart_plan_of(w, h, ncomp, sub_w, sub_h, (int)progressive, n, r);
                printf("%u %llu", p.nscans, j2p_restart_markers(&p));
                for(unsigned s = 0; s < p.nscans; s++) {
                        const j2p_restart_scan *k = &p.scan[s];
                        printf(" %u %u %u %u %u", k->units, k->units_per_row, k->interval, k->intervals, k->dri);
                }
                printf("\n");
        }
        return 0;
}
