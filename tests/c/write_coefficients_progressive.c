/* Test helper: tests/c/write_coefficients_optimized.c plus the one call jpeg_simple_progression() — the progressive JPEG file
 * libjpeg writes from given quantised coefficients: jpeg_set_defaults, jpeg_set_colorspace, jpeg_set_quality(Q, TRUE),
 * optimize_coding (which progressive mode forces anyway), jpeg_simple_progression, jpeg_write_coefficients — ten scans for three
 * components, six for one, every Huffman-coded scan with tables of its own, no restart markers (include/jpeg2png_amd.h: "The
 * progressive JPEG file").  What the restatement in tests/progressive_cases.py is compared with.
 * stdin, plain binary: uint32 width, height, ncomp (1 or 3), quality, sub_w, sub_h, then per component its
 * int16 data[blocks_h][blocks_w][64] (natural order; component 0: ceil(width / 8) x ceil(height / 8) blocks, the others
 * ceil(that / sub_w) x ceil(that / sub_h)).  stdout: the file.
 * With -t, the milliseconds jpeg_finish_compress took — the entropy coding of every block and the writing of the file — go to
 * stderr as one number (tools/entropy_probe.py: what the host pays per image).
 * usage: write_coefficients_progressive [-t] < coefficients.bin > picture.jpg */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <jpeglib.h>

static void need(void *p, size_t bytes)
{
        if(fread(p, 1, bytes, stdin) != bytes) {
                fprintf(stderr, "write_coefficients: short input\n");
                exit(1);
        }
}

int main(int argc, char **argv)
{
        const int timed = argc > 1 && strcmp(argv[1], "-t") == 0;
        uint32_t head[6];
        need(head, sizeof(head));
        const unsigned w = head[0], h = head[1], ncomp = head[2];
        unsigned sub_w = head[4], sub_h = head[5];
        if((ncomp != 1 && ncomp != 3) || w == 0 || h == 0 || sub_w < 1 || sub_w > 2 || sub_h < 1 || sub_h > 2) {
                fprintf(stderr, "write_coefficients: bad header\n");
                return 2;
        }
        if(ncomp == 1) { sub_w = sub_h = 1; }
        struct jpeg_compress_struct c;
        struct jpeg_error_mgr err;
        c.err = jpeg_std_error(&err);
        jpeg_create_compress(&c);
        jpeg_stdio_dest(&c, stdout);
        c.image_width = w;
        c.image_height = h;
        c.input_components = (int)ncomp;
        c.in_color_space = ncomp == 1 ? JCS_GRAYSCALE : JCS_YCbCr;
        jpeg_set_defaults(&c);
        jpeg_set_colorspace(&c, ncomp == 1 ? JCS_GRAYSCALE : JCS_YCbCr);
        jpeg_set_quality(&c, (int)head[3], TRUE);
        c.optimize_coding = TRUE;
        jpeg_simple_progression(&c);
        for(unsigned i = 0; i < ncomp; i++) {
                c.comp_info[i].h_samp_factor = i == 0 ? (int)sub_w : 1;
                c.comp_info[i].v_samp_factor = i == 0 ? (int)sub_h : 1;
        }
#if JPEG_LIB_VERSION >= 70
        c.min_DCT_h_scaled_size = 8;
        c.min_DCT_v_scaled_size = 8;
        c.jpeg_width = w;
        c.jpeg_height = h;
#endif
        const unsigned bw = (w + 7) / 8, bh = (h + 7) / 8;
        jvirt_barray_ptr arrays[3] = {NULL, NULL, NULL};
        unsigned cbw[3], cbh[3];
        for(unsigned i = 0; i < ncomp; i++) {
                const unsigned hs = (unsigned)c.comp_info[i].h_samp_factor, vs = (unsigned)c.comp_info[i].v_samp_factor;
                cbw[i] = i == 0 ? bw : (bw + sub_w - 1) / sub_w;
                cbh[i] = i == 0 ? bh : (bh + sub_h - 1) / sub_h;
                c.comp_info[i].width_in_blocks = cbw[i];
                c.comp_info[i].height_in_blocks = cbh[i];
                /* (zeroed, and rounded up to the sampling factors: libjpeg reads the rows and columns that complete an MCU) */
                arrays[i] = c.mem->request_virt_barray((j_common_ptr)&c, JPOOL_IMAGE, TRUE, (cbw[i] + hs - 1) / hs * hs,
                                                       (cbh[i] + vs - 1) / vs * vs, (JDIMENSION)vs);
        }
        jpeg_write_coefficients(&c, arrays);
        for(unsigned i = 0; i < ncomp; i++) {
                for(unsigned by = 0; by < cbh[i]; by++) {
                        JBLOCKARRAY row = c.mem->access_virt_barray((j_common_ptr)&c, arrays[i], by, 1, TRUE);
                        need(row[0][0], sizeof(JCOEF) * 64 * cbw[i]);
                }
        }
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        jpeg_finish_compress(&c);
        fflush(stdout);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if(timed) { fprintf(stderr, "%.3f\n", (double)(t1.tv_sec - t0.tv_sec) * 1e3 + (double)(t1.tv_nsec - t0.tv_nsec) / 1e6); }
        jpeg_destroy_compress(&c);
        return 0;
}
