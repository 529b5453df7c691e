/* Test helper: tests/c/write_coefficients.c, _optimized.c and _progressive.c as one program that also sets libjpeg's restart
 * interval — the JPEG file libjpeg writes from given quantised coefficients: jpeg_set_defaults, jpeg_set_colorspace,
 * jpeg_set_quality(Q, TRUE), then by `coder` nothing more (0), optimize_coding = TRUE (1) or that and jpeg_simple_progression() (2),
 * then restart_interval = N or restart_in_rows = R, then jpeg_write_coefficients (include/jpeg2png_amd.h: "Restart intervals").  What
 * the restatement in tests/restart_cases.py is compared with.
 * stdin, plain binary: uint32 width, height, ncomp (1 or 3), quality, sub_w, sub_h, coder, N, R, then per component its
 * int16 data[blocks_h][blocks_w][64] (natural order; component 0: ceil(width / 8) x ceil(height / 8) blocks, the others
 * ceil(that / sub_w) x ceil(that / sub_h)).  stdout: the file.
 * usage: write_coefficients_restart < coefficients.bin > picture.jpg */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <jpeglib.h>

static void need(void *p, size_t bytes)
{
        if(fread(p, 1, bytes, stdin) != bytes) {
                fprintf(stderr, "write_coefficients: short input\n");
                exit(1);
        }
}

int main(void)
{
        uint32_t head[9];
        need(head, sizeof(head));
        const unsigned w = head[0], h = head[1], ncomp = head[2];
        unsigned sub_w = head[4], sub_h = head[5];
        if((ncomp != 1 && ncomp != 3) || w == 0 || h == 0 || sub_w < 1 || sub_w > 2 || sub_h < 1 || sub_h > 2 || head[6] > 2) {
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
        if(head[6] >= 1) { c.optimize_coding = TRUE; }
        if(head[6] == 2) { jpeg_simple_progression(&c); }
        c.restart_interval = head[7];
        c.restart_in_rows = (int)head[8];
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
        jpeg_finish_compress(&c);
        fflush(stdout);
        jpeg_destroy_compress(&c);
        return 0;
}
