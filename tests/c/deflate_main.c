/* What the host's part of the PNG coder (jpeg2png_amd/csrc/j2p_deflate.h) makes, for tests/test_png_cpu.py.  stdin: records,
 * numbers separated by blanks or line ends, each beginning with its kind:
 *   0 final count[0] ... count[285]      a block's tables; prints
 *                                        longest hlit hclen dist_length header_bits bytes literals matches, the 286 lengths, the 19
 *                                        lengths of the code-length code, the 286 table entries and the header's bytes
 *   1 n byte[0] ... byte[n - 1]          prints the bytes' CRC-32
 *   2 m, then m times: n s1 s2           prints the Adler-32 of m blocks of n bytes with the sums s1 and s2
 * Includes nothing of the library but that header. */
#include <inttypes.h>
#include <stdio.h>

#include "j2p_deflate.h"

static int number(uint64_t *v)
{
        return scanf("%" SCNu64, v) == 1;
}

int main(void)
{
        uint64_t kind;
        while(number(&kind)) {
                if(kind == 0) {
                        uint64_t final, v;
                        uint32_t count[J2P_DEFLATE_SYMBOLS];
                        if(!number(&final)) { return 2; }
                        for(int s = 0; s < J2P_DEFLATE_SYMBOLS; s++) {
                                if(!number(&v)) { return 2; }
                                count[s] = (uint32_t)v;
                        }
                        static j2p_deflate_block b;
                        j2p_deflate_block_make(count, (int)final, &b);
                        printf("%u %u %u %u %u %" PRIu64 " %" PRIu64 " %" PRIu64, b.longest, b.hlit, b.hclen, b.dist_length, b.header_bits, b.bytes,
                               b.literals, b.matches);
                        for(int s = 0; s < J2P_DEFLATE_SYMBOLS; s++) { printf(" %u", b.lengths[s]); }
                        for(int s = 0; s < 19; s++) { printf(" %u", b.cl_lengths[s]); }
                        for(int s = 0; s < J2P_DEFLATE_SYMBOLS; s++) { printf(" %" PRIu32, b.code[s]); }
                        for(unsigned i = 0; i < (b.header_bits + 7) / 8; i++) { printf(" %u", b.header[i]); }
                        printf("\n");
                } else if(kind == 1) {
                        uint64_t n, v;
                        if(!number(&n)) { return 2; }
                        uint8_t *data = malloc(n ? n : 1);
                        if(!data) { return 2; }
                        for(uint64_t i = 0; i < n; i++) {
                                if(!number(&v)) { return 2; }
                                data[i] = (uint8_t)v;
                        }
                        printf("%" PRIu32 "\n", j2p_crc32(data, n));
                        free(data);
                } else if(kind == 2) {
                        uint64_t m, n, s1, s2;
                        uint32_t a = 1, b = 0;
                        if(!number(&m)) { return 2; }
                        for(uint64_t i = 0; i < m; i++) {
                                if(!number(&n) || !number(&s1) || !number(&s2)) { return 2; }
                                j2p_deflate_adler_add(&a, &b, n, (uint32_t)s1, (uint32_t)s2);
                        }
                        printf("%" PRIu32 "\n", (b << 16) | a);
                } else {
                        fprintf(stderr, "deflate_main: record kind %" PRIu64 "\n", kind);
                        return 2;
                }
        }
        return 0;
}
