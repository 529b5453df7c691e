/* What j2p_huff_build (jpeg2png_amd/csrc/j2p_huffman.h) returns, for tests/test_huffman_cpu.py.  stdin: cases of 256 counts
 * each, numbers separated by blanks or line ends.  Every case prints one line: "refused <code>", or
 *   longest nvals BITS[1] ... BITS[16] HUFFVAL[0] ... HUFFVAL[nvals - 1]
 * Includes nothing of the library but that header. */
#include <inttypes.h>
#include <stdio.h>

#include "j2p_huffman.h"

int main(void)
{
        for(;;) {
                uint64_t count[256];
                int n = 0;
                while(n < 256 && scanf("%" SCNu64, &count[n]) == 1) { n++; }
                if(n == 0) { return 0; }
                if(n != 256) {
                        fprintf(stderr, "huffman_main: a case of %d counts\n", n);
                        return 2;
                }
                j2p_huff_table t;
                const int rc = j2p_huff_build(count, &t);
                if(rc != J2P_HUFF_OK) {
                        printf("refused %d\n", rc);
                        continue;
                }
                printf("%u %u", t.longest, t.nvals);
                for(int i = 0; i < 16; i++) { printf(" %u", t.bits[i]); }
                for(unsigned i = 0; i < t.nvals; i++) { printf(" %u", t.vals[i]); }
                printf("\n");
        }
}
