/* Test program: the library's scans parser (j2p_jpeg_parse_scans_full of jpeg2png_amd/csrc/j2p_jpeg_parse.c, pure C, compiled into
 * this program) fed every prefix of each file named on the command line, and each file with every single byte set to FF and to 00,
 * as tests/c/jpeg_parse_main.c feeds the baseline parser.  Every input lives in a heap block of exactly its size.  Built with
 * -fsanitize=address,undefined by tests/test_scan_decode_cpu.py; exits 0 when the parser returned one of its codes every time and
 * what it accepted is consistent.
 * usage: jpeg_scans_main a.jpg b.jpg ... */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "j2p_internal.h"

void j2p_set_last_error(const char *msg) { (void)msg; }

static unsigned long long calls, accepted;
static j2p_scans_parsed *parsed;

static int feed(const uint8_t *bytes, size_t size)
{
        uint8_t *exact = malloc(size ? size : 1);
        if(!exact) { return 1; }
        memcpy(exact, bytes, size);
        const int rc = j2p_jpeg_parse_scans_full(exact, size, parsed);
        free(exact);
        calls++;
        if(rc == J2P_OK) {
                accepted++;
                const j2p_jpeg_scans *s = &parsed->scans;
                if(s->nscans == 0 || s->nscans > J2P_DECODE_SCANS_MAX || parsed->ntables > J2P_SCAN_TABLES_MAX) { return 1; }
                if(parsed->base.info.scan_begin != s->scan[0].begin || parsed->base.info.scan_end != s->scan[s->nscans - 1].end) { return 1; }
                for(unsigned i = 0; i < s->nscans; i++) {
                        const j2p_jpeg_scan *q = &s->scan[i];
                        if(q->begin > q->end || q->end > size || q->ncomp == 0 || q->ncomp > 3 || q->se > 63 || q->ss > q->se || q->intervals == 0) { return 1; }
                        if(i && q->begin < s->scan[i - 1].end) { return 1; }
                        if(s->progressive) {
                                if(q->ss && parsed->ac_table[i] >= parsed->ntables) { return 1; }
                                for(unsigned c = 0; c < q->ncomp; c++) {
                                        if(q->comp[c] >= parsed->base.info.ncomp) { return 1; }
                                        if(q->ss == 0 && q->ah == 0 && parsed->dc_table[i][c] >= parsed->ntables) { return 1; }
                                }
                        }
                }
        }
        return rc == J2P_OK || rc == J2P_EFORMAT || rc == J2P_ENOTSUP ? 0 : 1;
}

int main(int argc, char **argv)
{
        parsed = malloc(sizeof(*parsed));
        if(!parsed) { return 2; }
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
                const unsigned long long before = accepted;
                if(feed(file, (size_t)size)) { return 1; }
                if(accepted == before) {
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
        free(parsed);
        printf("%llu calls, %llu accepted\n", calls, accepted);
        return 0;
}
