/* Test program: the library's EXIF Orientation reader (j2p_jpeg_orientation in jpeg2png_amd/csrc/j2p_jpeg_parse.c, pure C, compiled
 * into this program) fed every prefix of each file named on the command line, and each file with every single byte set to FF, to
 * 00 and to its complement.  Every input lives in a heap block of exactly its size, so that a read past its end is one past an
 * allocation.  Built with -fsanitize=address,undefined by tests/test_upright_cpu.py; exits 0 when the reader returned J2P_OK and a
 * value in 1..8 every time, and for the whole file the value its name ends with (name_<value>.jpg).
 * usage: orientation_main a_6.jpg b_1.jpg ... */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "j2p_internal.h"

void j2p_set_last_error(const char *msg) { (void)msg; }

static unsigned long long calls, oriented;

static int feed(const uint8_t *bytes, size_t size, unsigned *value)
{
        uint8_t *exact = malloc(size ? size : 1);
        if(!exact) { return 1; }
        memcpy(exact, bytes, size);
        unsigned o = 99;
        const int rc = j2p_jpeg_orientation(exact, size, &o);
        free(exact);
        calls++;
        if(o != 1) { oriented++; }
        if(value) { *value = o; }
        return rc == J2P_OK && o >= 1 && o <= 8 ? 0 : 1;
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
                const char *underscore = strrchr(argv[a], '_');
                unsigned whole = 0;
                if(feed(file, (size_t)size, &whole)) { return 1; }
                if(!underscore || whole != (unsigned)atoi(underscore + 1)) {
                        fprintf(stderr, "%s: the whole file reads as %u\n", argv[a], whole);
                        return 1;
                }
                for(long n = 0; n < size; n++) {
                        if(feed(file, (size_t)n, NULL)) { return 1; }
                }
                for(long i = 0; i < size; i++) {
                        for(int v = 0; v < 3; v++) {
                                memcpy(work, file, (size_t)size);
                                work[i] = v == 0 ? 0xff : (v == 1 ? 0x00 : (uint8_t)~file[i]);
                                if(feed(work, (size_t)size, NULL)) { return 1; }
                        }
                }
                free(file);
                free(work);
        }
        printf("%llu calls, %llu oriented\n", calls, oriented);
        return 0;
}
