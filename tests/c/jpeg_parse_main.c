/* Test program: the library's JPEG marker parser (jpeg2png_amd/csrc/j2p_jpeg_parse.c, pure C, compiled into this program) fed
 * every prefix of each file named on the command line, and each file with every single byte set to FF and to 00.  Every input
 * lives in a heap block of exactly its size, so that a read past its end is one past an allocation.  Built with
 * -fsanitize=address,undefined by tests/test_decode_cpu.py; exits 0 when the parser returned one of its codes every time.
 * usage: jpeg_parse_main a.jpg b.jpg ... */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "j2p_internal.h"

void j2p_set_last_error(const char *msg) { (void)msg; }

static unsigned long long calls, accepted;

static int feed(const uint8_t *bytes, size_t size)
{
        uint8_t *exact = malloc(size ? size : 1);
        if(!exact) { return 1; }
        memcpy(exact, bytes, size);
        j2p_jpeg_parsed parsed;
        const int rc = j2p_jpeg_parse_full(exact, size, &parsed);
        free(exact);
        calls++;
        if(rc == J2P_OK) {
                accepted++;
                if(parsed.info.scan_begin > parsed.info.scan_end || parsed.info.scan_end > size || parsed.info.blocks_per_mcu > 10) { return 1; }
        }
        return rc == J2P_OK || rc == J2P_EFORMAT || rc == J2P_ENOTSUP ? 0 : 1;
}

int main(int argc, char **argv)
{
        for(int a = 1; a < argc; a++) {
                FILE *in = fopen(argv[a], "rb");
                if(!in) {
                        perror(argv[a]);
                        return 2;
                }
                fseek(in, 0, SEEK_END);
                const long size = ftell(in);
                fseek(in, 0, SEEK_SET);
                uint8_t *file = malloc((size_t)size + 1), *work = malloc((size_t)size + 1);
                if(!file || !work || fread(file, 1, (size_t)size, in) != (size_t)size) { return 2; }
                fclose(in);
                if(feed(file, (size_t)size)) { return 1; }
                if(accepted == 0) {
                        fprintf(stderr, "%s: the whole file was refused\n", argv[a]);
                        return 1;
                }
                for(long n = 0; n < size; n++) {
                        if(feed(file, (size_t)n)) { return 1; }
                }
                for(long i = 0; i < size; i++) {
                        for(int v = 0; v < 2; v++) {
                                memcpy(work, file, (size_t)size);
                                work[i] = v ? 0x00 : 0xff;
                                if(feed(work, (size_t)size)) { return 1; }
                        }
                }
                free(file);
                free(work);
        }
        printf("%llu calls, %llu accepted\n", calls, accepted);
        return 0;
}
