/* Test helper: component 0 of a one- or three-component JPEG — the only component of a greyscale file, Y of a colour
 * one — as libjpeg delivers it (the contract of the reference's jpeg.c:22-80), written to stdout in a plain binary form:
 *   uint32 w, h (image size), uint32 num_components, then uint32 w, h, w_samp, h_samp (coefficient plane and sampling
 *   factors), uint16 quant[64] (natural order), int16 data[h/8][w/8][64]
 * usage: read_component picture.jpg > component.bin */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <jpeglib.h>

static void put_u32(uint32_t v) { fwrite(&v, sizeof(v), 1, stdout); }

int main(int argc, char **argv)
{
        if(argc != 2) {
                fprintf(stderr, "usage: read_component picture.jpg\n");
                return 2;
        }
        FILE *in = fopen(argv[1], "rb");
        if(!in) {
                perror(argv[1]);
                return 1;
        }
        struct jpeg_decompress_struct d;
        struct jpeg_error_mgr err;
        d.err = jpeg_std_error(&err);
        jpeg_create_decompress(&d);
        jpeg_stdio_src(&d, in);
        jpeg_read_header(&d, TRUE);
        jvirt_barray_ptr *arrays = jpeg_read_coefficients(&d);
        if(d.num_components != 1 && d.num_components != 3) {
                fprintf(stderr, "need a one- or three-component JPEG\n");
                return 1;
        }
        put_u32(d.image_width);
        put_u32(d.image_height);
        put_u32((uint32_t)d.num_components);
        jpeg_component_info *ci = &d.comp_info[0];
        put_u32(ci->width_in_blocks * 8);
        put_u32(ci->height_in_blocks * 8);
        put_u32((uint32_t)(d.max_h_samp_factor / ci->h_samp_factor));
        put_u32((uint32_t)(d.max_v_samp_factor / ci->v_samp_factor));
        uint16_t q[64];
        const JQUANT_TBL *tbl = d.quant_tbl_ptrs[ci->quant_tbl_no];
        for(int i = 0; i < 64; i++) { q[i] = tbl->quantval[i]; }
        fwrite(q, sizeof(q), 1, stdout);
        for(JDIMENSION by = 0; by < ci->height_in_blocks; by++) {
                JBLOCKARRAY row = d.mem->access_virt_barray((j_common_ptr)&d, arrays[0], by, 1, FALSE);
                fwrite(row[0][0], sizeof(JCOEF) * 64, ci->width_in_blocks, stdout);
        }
        jpeg_destroy_decompress(&d);
        fclose(in);
        return 0;
}
