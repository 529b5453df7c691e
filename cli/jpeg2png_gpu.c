/*
 * jpeg2png_gpu — command-line driver with the reference's flags and behaviour
 * (jpeg2png.c:177-357, decode_file :120-172) on top of libjpeg2png_amd.so.
 *
 * What stays on the host: option parsing, reading the quantised DCT coefficients with
 * libjpeg (the contract of jpeg.c:22-80), writing the PNG with libpng (png.c:20-78).
 * What moves to the GPU: decode_coefficients + unbox (jpeg.c:83-92, box.c:5), the whole
 * solver, the luma fix-up and the YCbCr->RGB conversion (jpeg2png.c:156-159, png.c:37-62),
 * so that only int16 coefficients go up and only RGB bytes come down (with -j: only int16 coefficients, which
 * libjpeg Huffman-codes into a JPEG file; with -P: only the PNG file, and libpng is not used).
 *
 * Differences from the reference, on purpose:
 *   -t threads   = number of input files in flight (host threads reading / writing files; each file's GPU work
 *                  is a job of the library's batch engine, j2p_batch_*), instead of an OpenMP thread count;
 *                  default: the number of online cores, as OpenMP's default is (jpeg2png.c:246-257, :330)
 *   J2P_DEVICE / J2P_DEVICES environment: GPU index, or a comma list.  Files are spread over the listed GPUs; with
 *                  fewer files than GPUs the GPUs are shared out among the files and every image is row-tiled
 *                  over its share (one band per GPU; the library uses fewer bands, or one GPU, for images too
 *                  small to pay for the cross-band schedule: at least 2 Mpixel per band) — same pixels either way
 *   -g, --greyscale = a greyscale PNG: the reference's compute(1, ...) on component 0 alone, as `-s` solves it
 *                  (jpeg2png.c:147-152), written with Cb = Cr = 0 (png.c:37-45); one- and three-component JPEGs
 *   -j, --jpeg Q = a baseline JFIF file of libjpeg quality Q (1..100) instead of a PNG, 4:4:4 unless -S (one component with -g):
 *                  the GPU turns the solved float planes straight into quantised coefficients (j2p_planes_to_coefficients)
 *                  and the host only entropy-codes them (jpeg_write_coefficients) — no RGB, no 8-bit samples in between
 *   -S, --chroma-subsampling 444|422|420|440 = with -j: the chroma components of the file at half the resolution across, across
 *                  and down, or down; every chroma sample is the mean of the solved values it covers (the mean the solver's
 *                  projection constrains, compute.c:351-359), taken in float on the GPU (j2p_planes_to_coefficients_sub)
 *   -O, --optimize = with -j: Huffman tables made for the image instead of the standard's (libjpeg's optimize_coding; with -e the
 *                  GPU counts the symbols, J2P_JPEG_OPTIMIZE in j2p_jpeg_options.flags) — the same coefficients in a smaller
 *                  file, and the same file either way
 *   -r, --progressive = with -j: the progressive file of libjpeg's jpeg_simple_progression() — ten scans (six with -g), every one with
 *                  Huffman tables of its own (include/jpeg2png_amd.h, "The progressive JPEG file"); with -e the GPU codes every scan
 *                  (j2p_batch_submit_jpeg_opt or j2p_batch_submit_file_jpeg_opt, j2p_jpeg_options.progressive), without it
 *                  libjpeg does — the same file either way.  -O changes nothing about it
 *   -R, --restart N | NB = with -j: restart markers every N MCU rows, or with a B behind the number every N MCUs, as cjpeg -restart
 *                  spells them (libjpeg's restart_in_rows / restart_interval; include/jpeg2png_amd.h, "Restart intervals"); with -e the
 *                  GPU writes the intervals (the same two calls, j2p_jpeg_options.restart_*), without it libjpeg does — the same
 *                  file either way
 *   -D, --decode-any-on-gpu = -d, and a progressive input's scans are all decoded on the GPU as well (j2p_batch_next_file_scans;
 *                  include/jpeg2png_amd.h, "Reading a progressive JPEG file"); a file that decoder still refuses goes to libjpeg after
 *                  the one line -d prints
 *   -P, --png-on-gpu = the PNG is filtered and deflated on the GPU (j2p_batch_submit_png; include/jpeg2png_amd.h, "The PNG file") and
 *                  written as it comes down: no libpng, and no samples on the bus.  The same pixels as without it, in another (usually
 *                  somewhat larger) file; with -1, -g, -z, -s and -d; not with -j, not for row-tiled images
 * Messages and exit codes follow the reference ("jpeg2png: <message>", EXIT_FAILURE).
 */
#define _POSIX_C_SOURCE 200809L
#include <getopt.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <jpeglib.h>
#include <png.h>

#include "jpeg2png_amd.h"

#define VERSION_STRING "1.01-gfx950"
#define BAR_WIDTH 70u

/* ---- progress bar (same look as progressbar.c:16-29, 56-66) and die() (utils.c:11-40) ---- */

static pthread_mutex_t ui_lock = PTHREAD_MUTEX_INITIALIZER;
static bool bar_on = false;
static unsigned bar_cur = 0, bar_max = 1;

static void bar_draw(void)
{
        unsigned fill = BAR_WIDTH * bar_cur / bar_max;
        printf("\r[");
        for(unsigned i = 0; i < BAR_WIDTH; i++) { putchar(i < fill ? '#' : ' '); }
        printf("] %3u%%", 100 * bar_cur / bar_max);
        fflush(stdout);
}

static void bar_clear(void)
{
        printf("\r%*s\r", (int)(BAR_WIDTH + 7), "");
        fflush(stdout);
}

static void bar_add(unsigned n)
{
        pthread_mutex_lock(&ui_lock);
        if(bar_on) {
                unsigned of = BAR_WIDTH * bar_cur / bar_max, op = 100 * bar_cur / bar_max;
                bar_cur += n;
                if(of != BAR_WIDTH * bar_cur / bar_max || op != 100 * bar_cur / bar_max) { bar_draw(); }
        }
        pthread_mutex_unlock(&ui_lock);
}

static void die_va(bool with_errno, const char *fmt, va_list l)
{
        pthread_mutex_lock(&ui_lock);
        if(bar_on) { bar_clear(); bar_on = false; }
        fprintf(stderr, "jpeg2png: ");
        vfprintf(stderr, fmt, l);
        if(with_errno) { fprintf(stderr, ": "); perror(NULL); } else { fprintf(stderr, "\n"); }
        exit(EXIT_FAILURE);
}

static void die(const char *fmt, ...)
{
        va_list l;
        va_start(l, fmt);
        die_va(false, fmt, l);
}

static void die_perror(const char *fmt, ...)
{
        va_list l;
        va_start(l, fmt);
        die_va(true, fmt, l);
}

/* ---- JPEG coefficients in (what jpeg.c:22-80 delivers) ---- */

struct component {
        unsigned w, h, w_samp, h_samp;
        int16_t *data;
        uint16_t quant[64];
};

struct jpeg_in {
        unsigned w, h;
        unsigned n;             /* components read: 3, or 1 with -g (component 0 only) */
        struct component c[3];
        uint8_t *file;          /* -d: the file's bytes, for the library to decode; c[].data are then NULL */
        size_t file_size;
};

/* libjpeg's output_message hook: warnings (a truncated file, extraneous bytes ...) are printed and the
 * decode carries on, exactly like die_output_message of jpeg.c:14-19 — which, despite its name, returns.
 * Like die_message_start (utils.c:10-16) it takes the progress bar down for good.  Fatal errors keep
 * libjpeg's default error_exit: output_message, then exit(EXIT_FAILURE). */
static void jpeg_message(j_common_ptr info)
{
        char buf[JMSG_LENGTH_MAX];
        (*info->err->format_message)(info, buf);
        pthread_mutex_lock(&ui_lock);
        if(bar_on) { bar_clear(); bar_on = false; }
        fprintf(stderr, "jpeg2png: libjpeg error: %s\n", buf);
        pthread_mutex_unlock(&ui_lock);
}

/* zoom: the integer zoom factor (-z) the sampling factors are multiplied by later on, for the memory guard;
 * grey (-g): one- and three-component files are accepted and only component 0 is read */
static void read_coefficients(FILE *in, struct jpeg_in *jp, unsigned zoom, bool grey)
{
        struct jpeg_decompress_struct d;
        struct jpeg_error_mgr err;
        d.err = jpeg_std_error(&err);
        err.output_message = jpeg_message;
        jpeg_create_decompress(&d);
        jpeg_stdio_src(&d, in);
        jpeg_read_header(&d, TRUE);
        jp->w = d.image_width;
        jp->h = d.image_height;
        if(!grey && d.num_components != 3) { die("only 3 component jpegs are supported"); }
        if(grey && d.num_components != 1 && d.num_components != 3) { die("only 1 and 3 component jpegs are supported with -g"); }
        jp->n = grey ? 1 : 3;
        for(unsigned c = 0; c < jp->n; c++) {
                int t = d.comp_info[c].quant_tbl_no;
                if(t < 0 || t >= NUM_QUANT_TBLS) { die("weird jpeg: invalid quant_tbl_no"); }
                JQUANT_TBL *tbl = d.quant_tbl_ptrs[t];
                if(!tbl) { die("weird jpeg: no quant table pointer"); }
                for(int j = 0; j < 64; j++) {
                        if(tbl->quantval[j] == 0) { die("invalid quantization table"); }
                        jp->c[c].quant[j] = tbl->quantval[j];
                }
        }
        jvirt_barray_ptr *arrays = jpeg_read_coefficients(&d);
        for(unsigned c = 0; c < jp->n; c++) {
                jpeg_component_info *ci = &d.comp_info[c];
                struct component *k = &jp->c[c];
                k->w = ci->width_in_blocks * 8;
                k->h = ci->height_in_blocks * 8;
                k->w_samp = d.max_h_samp_factor / ci->h_samp_factor;
                k->h_samp = d.max_v_samp_factor / ci->v_samp_factor;
                if(k->h / 8 != (jp->h / k->h_samp + 7) / 8) { die("jpeg invalid coef h size"); }
                if(k->w / 8 != (jp->w / k->w_samp + 7) / 8) { die("jpeg invalid coef w size"); }
                if(SIZE_MAX / k->h / k->w / (k->h_samp * zoom) / (k->w_samp * zoom) < 6) { die("jpeg is too big to fit in memory"); }
                k->data = malloc(sizeof(int16_t) * (size_t)k->w * k->h);
                if(!k->data) { die("could not allocate memory for coefs"); }
                int16_t *dst = k->data;
                for(unsigned by = 0; by < ci->height_in_blocks; by++) {
                        JBLOCKARRAY row = d.mem->access_virt_barray((j_common_ptr)&d, arrays[c], by, 1, FALSE);
                        memcpy(dst, row[0][0], sizeof(int16_t) * 64 * ci->width_in_blocks);
                        dst += 64 * ci->width_in_blocks;
                }
        }
        jpeg_destroy_decompress(&d);
}

/* -d: no libjpeg on the way in — the file's bytes go to the library, which reads the marker segments on the host (j2p_jpeg_parse, here,
 * for the sizes) and Huffman-decodes the scan on the GPU that runs the job (j2p_batch_submit_file): jp gets the geometry and the tables,
 * no coefficients, and keeps the bytes.  false, after one line on stderr: the file is valid but of a kind that decoder does not read
 * (progressive, several scans, ...: J2P_ENOTSUP) and the caller goes on through libjpeg.  A damaged file dies with the library's message,
 * here or when its job is waited for. */
static bool read_file_for_gpu(const char *infile, FILE *in, struct jpeg_in *jp, unsigned zoom, bool grey, bool any)
{
        if(fseek(in, 0, SEEK_END) != 0) { die_perror("could not read input file `%s`", infile); }
        const long size = ftell(in);
        if(size < 0 || fseek(in, 0, SEEK_SET) != 0) { die_perror("could not read input file `%s`", infile); }
        uint8_t *file = malloc((size_t)size + 1);
        if(!file) { die("could not allocate memory for the file"); }
        if(fread(file, 1, (size_t)size, in) != (size_t)size) { die_perror("could not read input file `%s`", infile); }
        j2p_jpeg_info info;
        int rc;
        if(any) {               /* -D: progressive files too (j2p_jpeg_parse_scans) */
                j2p_jpeg_scans *scans = malloc(sizeof(*scans));
                if(!scans) { die("could not allocate memory for the file"); }
                rc = j2p_jpeg_parse_scans(file, (size_t)size, &info, scans);
                free(scans);
        } else {
                rc = j2p_jpeg_parse(file, (size_t)size, &info);
        }
        if(rc == J2P_ENOTSUP) {
                pthread_mutex_lock(&ui_lock);
                if(bar_on) { bar_clear(); bar_on = false; }
                fprintf(stderr, "jpeg2png: `%s`: %s; decoding with libjpeg\n", infile, j2p_last_error());
                pthread_mutex_unlock(&ui_lock);
                free(file);
                rewind(in);
                return false;
        }
        if(rc != J2P_OK) { die("`%s`: %s", infile, j2p_last_error()); }
        if(!grey && info.ncomp != 3) { die("only 3 component jpegs are supported"); }
        jp->w = info.width;
        jp->h = info.height;
        jp->n = grey ? 1 : 3;
        for(unsigned c = 0; c < jp->n; c++) {
                const j2p_jpeg_component *ci = &info.comp[c];
                struct component *k = &jp->c[c];
                for(int j = 0; j < 64; j++) {
                        if(ci->quant[j] == 0) { die("invalid quantization table"); }
                }
                k->w = ci->blocks_w * 8;
                k->h = ci->blocks_h * 8;
                k->w_samp = ci->w_samp;
                k->h_samp = ci->h_samp;
                if(SIZE_MAX / k->h / k->w / (k->h_samp * zoom) / (k->w_samp * zoom) < 6) { die("jpeg is too big to fit in memory"); }
                memcpy(k->quant, ci->quant, sizeof(k->quant));
                k->data = NULL;
        }
        jp->file = file;
        jp->file_size = (size_t)size;
        return true;
}

/* -a: the EXIF Orientation tag of the input, read from its bytes by the library (j2p_jpeg_orientation: 1 where the file has none
 * that counts); leaves `in` rewound */
static unsigned read_orientation(const char *infile, FILE *in)
{
        if(fseek(in, 0, SEEK_END) != 0) { die_perror("could not read input file `%s`", infile); }
        const long size = ftell(in);
        if(size < 0 || fseek(in, 0, SEEK_SET) != 0) { die_perror("could not read input file `%s`", infile); }
        uint8_t *file = malloc((size_t)size + 1);
        if(!file) { die("could not allocate memory for the file"); }
        if(fread(file, 1, (size_t)size, in) != (size_t)size) { die_perror("could not read input file `%s`", infile); }
        unsigned orientation = 1;
        if(j2p_jpeg_orientation(file, (size_t)size, &orientation) != J2P_OK) { die("`%s`: %s", infile, j2p_last_error()); }
        free(file);
        rewind(in);
        return orientation;
}

/* ---- PNG out (the file side of png.c:20-78; pixels arrive already converted) ---- */

static void png_fatal(png_structp png, png_const_charp msg)
{
        (void)png;
        die("%s", msg);
}

/* channels: 3 (RGB) or 1 (greyscale, -g) */
static void write_png(FILE *out, unsigned w, unsigned h, unsigned bits, unsigned channels, uint8_t *pixels)
{
        png_structp png = png_create_write_struct(PNG_LIBPNG_VER_STRING, NULL, png_fatal, NULL);
        if(!png) { die("could not initialize PNG write struct"); }
        png_infop info = png_create_info_struct(png);
        if(!info) { die("could not initialize PNG info struct"); }
        png_init_io(png, out);
        png_set_IHDR(png, info, w, h, (int)bits, channels == 1 ? PNG_COLOR_TYPE_GRAY : PNG_COLOR_TYPE_RGB, PNG_INTERLACE_NONE,
                     PNG_COMPRESSION_TYPE_BASE, PNG_FILTER_TYPE_BASE);
        png_write_info(png, info);
        png_bytep *rows = malloc(sizeof(*rows) * h);
        if(!rows) { die("allocation failure"); }
        size_t stride = (size_t)w * channels * (bits / 8);
        for(unsigned y = 0; y < h; y++) { rows[y] = pixels + y * stride; }
        png_write_image(png, rows);
        free(rows);
        png_write_end(png, info);
        png_destroy_write_struct(&png, &info);
}

/* ---- JPEG out (-j): the quantised coefficients arrive from the GPU; libjpeg only entropy-codes them ---- */

/* libjpeg's own tables for `quality` (jpeg_set_defaults, jpeg_set_colorspace, jpeg_set_quality(Q, TRUE)), natural order:
 * table 0 for component 0, table 1 for the chroma components */
static void setup_jpeg_out(struct jpeg_compress_struct *c, unsigned w, unsigned h, unsigned ncomp, int quality, unsigned sub_w, unsigned sub_h)
{
        c->image_width = w;
        c->image_height = h;
        c->input_components = (int)ncomp;
        c->in_color_space = ncomp == 1 ? JCS_GRAYSCALE : JCS_YCbCr;
        jpeg_set_defaults(c);
        jpeg_set_colorspace(c, ncomp == 1 ? JCS_GRAYSCALE : JCS_YCbCr);
        jpeg_set_quality(c, quality, TRUE);
        /* chroma at 1 / sub_w x 1 / sub_h: component 0 carries the factors, the others 1 (4:4:4: all 1) */
        for(unsigned i = 0; i < ncomp; i++) {
                c->comp_info[i].h_samp_factor = i == 0 ? (int)sub_w : 1;
                c->comp_info[i].v_samp_factor = i == 0 ? (int)sub_h : 1;
        }
}

static void jpeg_out_tables(unsigned ncomp, int quality, uint16_t quant[3][64])
{
        struct jpeg_compress_struct c;
        struct jpeg_error_mgr err;
        c.err = jpeg_std_error(&err);
        err.output_message = jpeg_message;
        jpeg_create_compress(&c);
        setup_jpeg_out(&c, 8, 8, ncomp, quality, 1, 1);
        for(unsigned i = 0; i < ncomp; i++) {
                JQUANT_TBL *tbl = c.quant_tbl_ptrs[c.comp_info[i].quant_tbl_no];
                if(!tbl) { die("libjpeg gave no quantization table"); }
                for(int j = 0; j < 64; j++) { quant[i][j] = tbl->quantval[j]; }
        }
        jpeg_destroy_compress(&c);
}

/* coef[i]: component i's bh * bw blocks of 64 int16, block-major, natural order (JBLOCK rows); component 0 has
 * ceil(w / 8) x ceil(h / 8) blocks, the chroma components ceil(that / sub_w) x ceil(that / sub_h).  Only these real blocks are
 * filled: the dummy blocks that complete a partial MCU are libjpeg's own (jctrans.c), but it reaches them through arrays
 * whose sizes are rounded up to the component's sampling factors and that can hold v_samp_factor rows at a time */
static void write_jpeg(FILE *out, unsigned w, unsigned h, unsigned ncomp, int quality, unsigned sub_w, unsigned sub_h, bool optimize,
                       bool progressive, unsigned restart_interval, unsigned restart_in_rows, int16_t *const coef[3])
{
        struct jpeg_compress_struct c;
        struct jpeg_error_mgr err;
        c.err = jpeg_std_error(&err);
        err.output_message = jpeg_message;
        jpeg_create_compress(&c);
        jpeg_stdio_dest(&c, out);
        if(ncomp == 1) { sub_w = sub_h = 1; }
        setup_jpeg_out(&c, w, h, ncomp, quality, sub_w, sub_h);
        if(optimize) { c.optimize_coding = TRUE; }
        if(progressive) { jpeg_simple_progression(&c); }
        c.restart_interval = restart_interval;
        c.restart_in_rows = (int)restart_in_rows;
        const unsigned bw = (w + 7) / 8, bh = (h + 7) / 8;
#if JPEG_LIB_VERSION >= 70
        /* IJG 7+: jpeg_write_coefficients expects what jpeg_calc_jpeg_dimensions / initial_setup would have left */
        c.min_DCT_h_scaled_size = 8;
        c.min_DCT_v_scaled_size = 8;
        c.jpeg_width = w;
        c.jpeg_height = h;
#endif
        jvirt_barray_ptr arrays[3] = {NULL, NULL, NULL};
        unsigned cbw[3], cbh[3];
        for(unsigned i = 0; i < ncomp; i++) {
                const unsigned hs = (unsigned)c.comp_info[i].h_samp_factor, vs = (unsigned)c.comp_info[i].v_samp_factor;
                cbw[i] = i == 0 ? bw : (bw + sub_w - 1) / sub_w;
                cbh[i] = i == 0 ? bh : (bh + sub_h - 1) / sub_h;
                c.comp_info[i].width_in_blocks = cbw[i];
                c.comp_info[i].height_in_blocks = cbh[i];
                /* (pre-zeroed: the transcoder reads the padding row of an odd block-row count, which nothing here writes) */
                arrays[i] = c.mem->request_virt_barray((j_common_ptr)&c, JPOOL_IMAGE, TRUE, (cbw[i] + hs - 1) / hs * hs,
                                                       (cbh[i] + vs - 1) / vs * vs, (JDIMENSION)vs);
        }
        jpeg_write_coefficients(&c, arrays);
        for(unsigned i = 0; i < ncomp; i++) {
                for(unsigned by = 0; by < cbh[i]; by++) {
                        JBLOCKARRAY row = c.mem->access_virt_barray((j_common_ptr)&c, arrays[i], by, 1, TRUE);
                        memcpy(row[0][0], coef[i] + (size_t)by * cbw[i] * 64, sizeof(int16_t) * 64 * cbw[i]);
                }
        }
        jpeg_finish_compress(&c);
        jpeg_destroy_compress(&c);
}

/* ---- one file: decode_file (jpeg2png.c:120-172) ---- */

struct options {
        unsigned iterations[3];
        float weights[3], pweights[3];
        unsigned png_bits;
        int jpeg_quality;       /* -j: 1..100 = write a JPEG of that libjpeg quality instead of a PNG; 0 = PNG */
        bool decode_any_on_gpu; /* -D: -d, and progressive files are decoded on the GPU too (j2p_batch_next_file_scans) */
        bool decode_on_gpu;     /* -d: the input's scan is Huffman-decoded on the GPU (j2p_entropy_decode); libjpeg only for files that decoder does not read */
        bool encode_on_gpu;     /* -e: with -j, the file is entropy-coded on the GPU (j2p_batch_submit_jpeg_opt, _file_jpeg_opt) and written as it comes down */
        bool png_on_gpu;        /* -P: the PNG is coded on the GPU (j2p_batch_submit_png) and written as it comes down */
        bool auto_orient;       /* -a: the input's EXIF Orientation is applied: every output is the upright image, and carries no tag */
        bool progressive;       /* -r: with -j, the progressive file (jpeg_simple_progression; with -e j2p_jpeg_options.progressive) */
        unsigned restart_interval, restart_in_rows;     /* -R NB, -R N: with -j, restart intervals of N MCUs or N MCU rows */
        bool optimize;          /* -O: with -j, Huffman tables made for the image (optimize_coding; with -e J2P_JPEG_OPTIMIZE) */
        unsigned sub_w, sub_h;  /* -S: the chroma components of that JPEG at 1 / sub_w x 1 / sub_h of the resolution (1 or 2) */
        bool joint, quiet;
        bool grey;              /* -g: component 0 alone, one-channel job, greyscale PNG */
        unsigned zoom;          /* -z: integer zoom factor 1..4 (every sampling factor times zoom, output zoom times the size) */
        bool tile;              /* fewer files than GPUs: every image row-tiled over its share of them */
        unsigned nfiles;
        FILE *csv;
        int ndev, devs[16];
};

static pthread_mutex_t csv_lock = PTHREAD_MUTEX_INITIALIZER;
/* the library's batch engine, created when the first file has been read (a file that cannot be read fails on its
 * own message, with or without a GPU) */
static j2p_batch *batch = NULL;
static pthread_once_t batch_once = PTHREAD_ONCE_INIT;
static unsigned batch_ndev = 1, batch_slots = 1;
static int batch_devs[16];
static int batch_rc = J2P_OK;
static char batch_err[512];

static void batch_start(void)
{
        batch_rc = j2p_batch_create(&batch, batch_ndev, batch_devs, batch_slots);
        if(batch_rc != J2P_OK) { snprintf(batch_err, sizeof(batch_err), "%s", j2p_last_error()); }
}

static void gpu_check(int rc)
{
        if(rc != J2P_OK) { die("%s", j2p_last_error()); }
}

/* callbacks of a batch job (called on the library's worker thread): CSV rows (logger.c:20-28) and progress ticks */
struct job_ctx {
        const struct options *o;
        const char *name;
};

static void job_rows(void *user, unsigned channel, unsigned first, unsigned n, const j2p_log_row *rows)
{
        struct job_ctx *ctx = user;
        pthread_mutex_lock(&csv_lock);                                 /* critical(write_log), logger.c:22 */
        for(unsigned i = 0; i < n; i++) {
                if(fprintf(ctx->o->csv, "%s,%u,%u,%f,%f,%f,%f\n", ctx->name, channel, first + i, rows[i].objective,
                           rows[i].prob_dist, rows[i].tv, rows[i].tv2) < 0) {
                        die_perror("could not write to csv log");
                }
        }
        pthread_mutex_unlock(&csv_lock);
}

static void job_progress(void *user, unsigned n)
{
        (void)user;
        bar_add(n);
}

/* decode_file (jpeg2png.c:120-172): the coefficients go to the library's batch engine, which decodes, solves
 * (one joint compute(3, ...) or three compute(1, ...), jpeg2png.c:141-152) and converts on a GPU slot of its own
 * while this thread's neighbours read their JPEGs and deflate their PNGs */
static void decode_file(const char *infile, const char *outfile, const struct options *o, unsigned index)
{
        FILE *in = fopen(infile, "rb");
        if(!in) { die_perror("could not open input file `%s`", infile); }
        struct jpeg_in jp;
        memset(&jp, 0, sizeof(jp));
        const unsigned orientation = o->auto_orient ? read_orientation(infile, in) : 1;
        if(!o->decode_on_gpu || !read_file_for_gpu(infile, in, &jp, o->zoom, o->grey, o->decode_any_on_gpu)) {
                read_coefficients(in, &jp, o->zoom, o->grey);
        }
        fclose(in);
        /* zooming by z = the same solve with every component's sampling factors times z (compute.c:407-416): the
         * canvas, and the image written, are z times as wide and as high.  The library's canvas height limit is
         * 65536 rows; refused here, before any GPU work */
        const unsigned zoom = o->zoom;
        {
                unsigned long long cw = 0, chh = 0;
                for(unsigned c = 0; c < jp.n; c++) {
                        const unsigned long long w = (unsigned long long)jp.c[c].w * jp.c[c].w_samp * zoom;
                        const unsigned long long h = (unsigned long long)jp.c[c].h * jp.c[c].h_samp * zoom;
                        if(w > cw) { cw = w; }
                        if(h > chh) { chh = h; }
                }
                if(cw > 65536 || chh > 65536) {
                        die("zoomed canvas of `%s` is %llux%llu pixels: at most 65536 per side", infile, cw, chh);
                }
        }

        struct job_ctx ctx = {o, infile};
        j2p_job job;
        memset(&job, 0, sizeof(job));
        /* -g: component 0 as one compute(1, ...) with entry 0 of the lists, as the first call of `-s` makes it
         * (jpeg2png.c:147-152); separate, so that its CSV rows are channel 0's, as that run writes them */
        job.nchannel = jp.n;
        for(unsigned c = 0; c < jp.n; c++) {
                job.planes[c].w = jp.c[c].w;
                job.planes[c].h = jp.c[c].h;
                job.planes[c].w_samp = jp.c[c].w_samp * zoom;
                job.planes[c].h_samp = jp.c[c].h_samp * zoom;
                job.planes[c].data = jp.c[c].data;
                job.planes[c].fdata = NULL;                             /* decoded on the device */
                job.planes[c].quant_table = jp.c[c].quant;
                job.weight[c] = o->weights[c];
                job.pweight[c] = o->pweights[c];
                job.iterations[c] = o->iterations[c];
        }
        job.separate = o->grey || !o->joint;
        job.tile = o->tile && !jp.file;        /* (a row-tiled job takes no file) */
        {
                /* (tests row-tile small images: the pixel gate of the library can be lowered from outside the program) */
                const char *gate = getenv("J2P_TILE_MIN_BAND_PIXELS");
                if(gate && *gate) {
                        const unsigned long long v = strtoull(gate, NULL, 10);
                        job.tile_min_band_pixels = v ? (size_t)v : (size_t)-1;
                }
        }
        if(o->tile && o->nfiles > 1) {
                /* several files, still fewer than GPUs: file i gets GPUs [i n / f, (i + 1) n / f) of the list */
                job.tile_first = index * (unsigned)o->ndev / o->nfiles;
                job.tile_count = (index + 1) * (unsigned)o->ndev / o->nfiles - job.tile_first;
        }
        job.out_w = jp.w * zoom;
        job.out_h = jp.h * zoom;
        if(orientation >= 5) {
                /* -a: the job's solvers are oriented (ORIENT_NEXT below) and every output form is that of the upright image, here
                 * a turned one (a file without the tag, or with tag 1, is the job it always was) */
                job.out_w = jp.h * zoom;
                job.out_h = jp.w * zoom;
        }
        uint8_t *pixels = NULL;
        uint16_t out_quant[3][64];
        int16_t *out_coef[3] = {NULL, NULL, NULL};
        if(o->jpeg_quality) {
                /* -j: int16 coefficients of a JPEG come down instead of samples (-S: fewer for the chroma components) */
                jpeg_out_tables(jp.n, o->jpeg_quality, out_quant);
                job.out_blocks_w = (job.out_w + 7) / 8;
                job.out_blocks_h = (job.out_h + 7) / 8;
                for(unsigned c = 0; c < jp.n; c++) {
                        job.out_sub_w[c] = c == 0 ? 1 : o->sub_w;
                        job.out_sub_h[c] = c == 0 ? 1 : o->sub_h;
                        const size_t bw = (job.out_blocks_w + job.out_sub_w[c] - 1) / job.out_sub_w[c];
                        const size_t bh = (job.out_blocks_h + job.out_sub_h[c] - 1) / job.out_sub_h[c];
                        out_coef[c] = malloc(sizeof(int16_t) * 64 * bw * bh);
                        if(!out_coef[c]) { die("could not allocate image data"); }
                        job.out_quant[c] = out_quant[c];
                        job.out_coef[c] = out_coef[c];
                }
        } else if(!o->png_on_gpu) {
                job.out_bits = o->png_bits;
                size_t bytes = (size_t)job.out_w * job.out_h * jp.n * (o->png_bits / 8);
                pixels = malloc(bytes);
                if(!pixels) { die("could not allocate image data"); }
                job.out_rgb = pixels;
        }
        job.on_rows = o->csv ? job_rows : NULL;
        job.on_progress = o->quiet ? NULL : job_progress;
        job.user = &ctx;
        int ticket = 0;
        pthread_once(&batch_once, batch_start);
        if(batch_rc != J2P_OK) { die("%s", batch_err); }
        /* (the orientation travels next to the job: set for this thread's next submit, before every one of them below) */
#define ORIENT_NEXT() do { \
                gpu_check(orientation > 1 ? j2p_batch_next_orientation(batch, orientation, jp.w * zoom, jp.h * zoom) : J2P_OK); \
                gpu_check(jp.file && o->decode_any_on_gpu ? j2p_batch_next_file_scans(batch, 1) : J2P_OK); /* (-D: what the submit below accepts) */ \
        } while(0)
        uint8_t *file = NULL;
        size_t file_bytes = 0;
        if(o->jpeg_quality && o->encode_on_gpu) {
                /* -e: the same tables, but the coefficients stay on the GPU and the finished file comes down.  Room for a quarter
                 * of a byte per sample at first; a file that needs more says how much, and the job runs again */
                j2p_jpeg spec = {job.out_w, job.out_h, jp.n == 1 ? 1 : o->sub_w, jp.n == 1 ? 1 : o->sub_h, {NULL, NULL, NULL}};
                for(unsigned c = 0; c < jp.n; c++) {
                        spec.quant[c] = out_quant[c];
                        job.out_quant[c] = NULL;
                        job.out_coef[c] = NULL;
                }
                job.out_blocks_w = job.out_blocks_h = 0;
                job.tile = 0;           /* (a row-tiled job has no file output) */
                /* -O, -r and -R as the one record that describes the file */
                const j2p_jpeg_options options = {o->optimize ? J2P_JPEG_OPTIMIZE : 0u, o->progressive ? 1u : 0u, o->restart_interval, o->restart_in_rows};
                size_t capacity = 4096 + (size_t)job.out_w * job.out_h * jp.n / 4;
                for(int attempt = 0;; attempt++) {
                        file = malloc(capacity);
                        if(!file) { die("could not allocate image data"); }
                        ORIENT_NEXT();
                        if(jp.file) {
                                gpu_check(j2p_batch_submit_file_jpeg_opt(batch, &job, jp.file, jp.file_size, &spec, file, capacity, &file_bytes, &options, &ticket));
                        } else {
                                gpu_check(j2p_batch_submit_jpeg_opt(batch, &job, NULL, &spec, file, capacity, &file_bytes, &options, &ticket));
                        }
                        const int rc = j2p_batch_wait(batch, ticket);
                        if(rc != J2P_ESPACE || attempt) {
                                gpu_check(rc);
                                break;
                        }
                        free(file);
                        capacity = file_bytes;
                }
        } else if(o->png_on_gpu) {
                /* -P: the samples stay on the GPU and the finished file comes down.  Room for three quarters of a byte per byte of
                 * samples at first; a file that needs more says how much, and the job runs again */
                const j2p_png spec = {job.out_w, job.out_h, o->png_bits, J2P_PNG_FILTER_ADAPTIVE, 0, 0};
                job.out_bits = 0;
                job.out_rgb = NULL;
                job.tile = 0;           /* (a row-tiled job has no file output) */
                size_t capacity = 4096 + (size_t)job.out_w * job.out_h * jp.n * (o->png_bits / 8) / 4 * 3;
                for(int attempt = 0;; attempt++) {
                        file = malloc(capacity);
                        if(!file) { die("could not allocate image data"); }
                        ORIENT_NEXT();
                        if(jp.file) { gpu_check(j2p_batch_submit_file_png(batch, &job, jp.file, jp.file_size, &spec, file, capacity, &file_bytes, &ticket)); }
                        else { gpu_check(j2p_batch_submit_png(batch, &job, NULL, &spec, file, capacity, &file_bytes, &ticket)); }
                        const int rc = j2p_batch_wait(batch, ticket);
                        if(rc != J2P_ESPACE || attempt) {
                                gpu_check(rc);
                                break;
                        }
                        free(file);
                        capacity = file_bytes;
                }
        } else {
                ORIENT_NEXT();
                if(jp.file) { gpu_check(j2p_batch_submit_file(batch, &job, jp.file, jp.file_size, 0, NULL, &ticket)); }
                else { gpu_check(j2p_batch_submit(batch, &job, &ticket)); }
                gpu_check(j2p_batch_wait(batch, ticket));
        }
#undef ORIENT_NEXT
        for(unsigned c = 0; c < jp.n; c++) { free(jp.c[c].data); }
        free(jp.file);
        FILE *out = fopen(outfile, "wb");
        if(!out) { die_perror("could not open output file `%s`", outfile); }
        if(file) {
                if(fwrite(file, 1, file_bytes, out) != file_bytes) { die_perror("could not write output file `%s`", outfile); }
        } else if(o->jpeg_quality) { write_jpeg(out, job.out_w, job.out_h, jp.n, o->jpeg_quality, o->sub_w, o->sub_h, o->optimize, o->progressive, o->restart_interval, o->restart_in_rows, out_coef); }
        else { write_png(out, job.out_w, job.out_h, o->png_bits, jp.n, pixels); }
        fclose(out);
        free(pixels);
        free(file);
        for(unsigned c = 0; c < 3; c++) { free(out_coef[c]); }
}

/* ---- file-level parallelism (jpeg2png.c:330: omp parallel for over files) ---- */

struct work {
        unsigned nin, next;
        char **in, **out;
        const struct options *o;
        pthread_mutex_t lock;
};

static void *worker(void *arg)
{
        struct work *w = arg;
        for(;;) {
                pthread_mutex_lock(&w->lock);
                unsigned i = w->next++;
                pthread_mutex_unlock(&w->lock);
                if(i >= w->nin) { break; }
                decode_file(w->in[i], w->out[i], w->o, i);
        }
        return NULL;
}

static void usage(void)
{
        printf("usage: jpeg2png_gpu picture.jpg ... [-o picture.png] ... [flags...]\n\n"
               "  -o, --output FILE            output file (overwritten); zero times or once per input\n"
               "                               default: input name with the extension .png\n"
               "  -f, --force                  overwrite default-named outputs too\n"
               "  -w, --second-order-weight W[,Wcb,Wcr]\n"
               "                               TGV weight, 0 = plain total variation (default 0.3; chroma 0\n"
               "                               with -s); three values need -s\n"
               "  -p, --probability-weight P[,Pcb,Pcr]\n"
               "                               DCT-coefficient distance weight (default 0.001)\n"
               "  -i, --iterations N[,Ncb,Ncr] optimisation steps (default 50); three values need -s\n"
               "  -s, --separate-components    optimise Y, Cb, Cr independently (three GPU streams)\n"
               "  -t, --threads N              input files processed concurrently (default: online cores)\n"
               "  -1, --16-bits-png            16-bit PNG\n"
               "  -z, --zoom N                 upscale N times (1..4) while removing the artifacts (default 1)\n"
               "  -g, --greyscale              greyscale PNG; also reads 1-component JPEGs.  The grey is component 0\n"
               "                               (Y) solved alone, as -s solves it, with the first -w/-p/-i value; not\n"
               "                               the luma of the default joint solve\n"
               "  -j, --jpeg Q                 write a baseline JPEG of quality Q (1..100; 4:4:4 unless -S, one component with -g)\n"
               "                               straight from the solved planes instead of a PNG; needs -o for every input\n"
               "  -S, --chroma-subsampling 444|422|420|440\n"
               "                               with -j: chroma at half the resolution across (422), across and down (420)\n"
               "                               or down (440), every sample the mean of the solved values it covers\n"
               "  -d, --decode-on-gpu          the GPU Huffman-decodes the input too (baseline files; others are read by libjpeg\n"
               "                               after one line saying so): no libjpeg between the file's bytes and the solver;\n"
               "                               such an image is not row-tiled\n"
               "  -D, --decode-any-on-gpu      -d, and the GPU decodes every scan of a progressive file too; what it still does\n"
               "                               not read goes to libjpeg after that one line\n"
               "  -e, --encode-on-gpu          with -j: the GPU also entropy-codes the file (default Huffman tables, the bytes\n"
               "                               libjpeg would write) and only the file comes down; not for row-tiled images\n"
               "  -O, --optimize               with -j: Huffman tables made for the image, a smaller file of the same\n"
               "                               coefficients (with -e the GPU counts the symbols; the same bytes either way)\n"
               "  -r, --progressive            with -j: a progressive JPEG (libjpeg's simple progression: ten scans, six with -g,\n"
               "                               each with Huffman tables of its own); with -e the GPU codes every scan; the\n"
               "                               same bytes either way\n"
               "  -R, --restart N | NB         with -j: restart markers every N MCU rows, or (NB) every N MCUs, 1..65535; with -e\n"
               "                               the GPU writes them; the same bytes either way\n"
               "  -P, --png-on-gpu             the GPU also filters and deflates the PNG and only the file comes down: the same\n"
               "                               pixels in another, usually somewhat larger file; not with -j, not for row-tiled images\n"
               "  -a, --auto-orient            apply the input's EXIF Orientation: every output is the upright image (turned and\n"
               "                               mirrored on the GPU; the files written carry no tag); not for row-tiled images\n"
               "  -c, --csv-log FILE           per-iteration objective log\n"
               "  -q, --quiet                  no progress bar\n"
               "  -h, --help    -V, --version\n"
               "environment: J2P_DEVICE=n or J2P_DEVICES=a,b,... selects the GPU(s); fewer files than GPUs:\n"
               "             large images are row-tiled over their share of them\n");
        exit(EXIT_FAILURE);
}

int main(int argc, char **argv)
{
        static const struct option longopts[] = {
                {"help", no_argument, NULL, 'h'}, {"version", no_argument, NULL, 'V'}, {"output", required_argument, NULL, 'o'},
                {"force", no_argument, NULL, 'f'}, {"csv-log", required_argument, NULL, 'c'},
                {"threads", required_argument, NULL, 't'}, {"quiet", no_argument, NULL, 'q'},
                {"separate-components", no_argument, NULL, 's'}, {"16-bits-png", no_argument, NULL, '1'},
                {"iterations", required_argument, NULL, 'i'}, {"probability-weight", required_argument, NULL, 'p'},
                {"second-order-weight", required_argument, NULL, 'w'}, {"zoom", required_argument, NULL, 'z'},
                {"greyscale", no_argument, NULL, 'g'}, {"jpeg", required_argument, NULL, 'j'},
                {"chroma-subsampling", required_argument, NULL, 'S'}, {"encode-on-gpu", no_argument, NULL, 'e'},
                {"decode-on-gpu", no_argument, NULL, 'd'}, {"decode-any-on-gpu", no_argument, NULL, 'D'}, {"optimize", no_argument, NULL, 'O'},
                {"progressive", no_argument, NULL, 'r'}, {"restart", required_argument, NULL, 'R'},
                {"png-on-gpu", no_argument, NULL, 'P'}, {"auto-orient", no_argument, NULL, 'a'}, {NULL, 0, NULL, 0}};
        struct options o = {.iterations = {50, 50, 50}, .weights = {0.3f, 0.f, 0.f}, .pweights = {0.001f, 0.001f, 0.001f},
                            .png_bits = 8, .jpeg_quality = 0, .encode_on_gpu = false, .png_on_gpu = false, .optimize = false, .sub_w = 1, .sub_h = 1, .joint = true, .quiet = false, .grey = false, .zoom = 1, .tile = false, .csv = NULL, .ndev = 1, .devs = {0}};
        const char *w_arg = NULL, *p_arg = NULL, *i_arg = NULL, *t_arg = NULL, *c_arg = NULL, *z_arg = NULL, *j_arg = NULL, *S_arg = NULL, *R_arg = NULL;
        char **outs = calloc((size_t)argc, sizeof(*outs));
        unsigned nout = 0;
        bool force = false, help = false, version = false;
        int ch;
        while((ch = getopt_long(argc, argv, "h?Vo:fc:t:qs1i:p:w:z:gj:S:edDOParR:", longopts, NULL)) != -1) {
                switch(ch) {
                case 'V': version = true; break;
                case 'o': outs[nout++] = optarg; break;
                case 'f': force = true; break;
                case 'c': c_arg = optarg; break;
                case 't': t_arg = optarg; break;
                case 'q': o.quiet = true; break;
                case 's': o.joint = false; break;
                case '1': o.png_bits = 16; break;
                case 'i': i_arg = optarg; break;
                case 'p': p_arg = optarg; break;
                case 'w': w_arg = optarg; break;
                case 'z': z_arg = optarg; break;
                case 'g': o.grey = true; break;
                case 'j': j_arg = optarg; break;
                case 'S': S_arg = optarg; break;
                case 'e': o.encode_on_gpu = true; break;
                case 'd': o.decode_on_gpu = true; break;
                case 'D': o.decode_on_gpu = o.decode_any_on_gpu = true; break;
                case 'O': o.optimize = true; break;
                case 'r': o.progressive = true; break;
                case 'R': R_arg = optarg; break;
                case 'P': o.png_on_gpu = true; break;
                case 'a': o.auto_orient = true; break;
                default: help = true; break;
                }
        }
        if(version) {
                printf("jpeg2png_gpu version " VERSION_STRING " (%s)\n", j2p_version());
                exit(EXIT_FAILURE);                                     /* sic: jpeg2png.c:195-198 */
        }
        unsigned nin = (unsigned)(argc - optind);
        if(nin == 0 || help) { usage(); }
        char **ins = argv + optind;

        if(w_arg) {
                int n = sscanf(w_arg, "%f,%f,%f", &o.weights[0], &o.weights[1], &o.weights[2]);
                if(n == 3) { if(o.joint) { die("different weights are only possible when using separated components"); } }
                else if(n != 1) { die("invalid weight"); }
        }
        if(p_arg) {
                int n = sscanf(p_arg, "%f,%f,%f", &o.pweights[0], &o.pweights[1], &o.pweights[2]);
                if(n == 1) { o.pweights[1] = o.pweights[2] = o.pweights[0]; }
                else if(n != 3) { die("invalid probability weight"); }
        }
        if(i_arg) {
                int n = sscanf(i_arg, "%u,%u,%u", &o.iterations[0], &o.iterations[1], &o.iterations[2]);
                if(n == 3) { if(o.joint) { die("different iteration counts are only possible when using separated components"); } }
                else if(n == 1) { o.iterations[1] = o.iterations[2] = o.iterations[0]; }
                else { die("invalid number of iterations"); }
        }
        if(z_arg) {
                char *end = NULL;
                const unsigned long z = strtoul(z_arg, &end, 10);
                if(end == z_arg || *end != '\0' || z_arg[0] == '-' || z < 1 || z > 4) { die("invalid zoom factor"); }
                o.zoom = (unsigned)z;
        }
        if(j_arg) {
                char *end = NULL;
                const unsigned long q = strtoul(j_arg, &end, 10);
                if(end == j_arg || *end != '\0' || j_arg[0] == '-' || q < 1 || q > 100) { die("invalid jpeg quality"); }
                o.jpeg_quality = (int)q;
                if(o.png_bits == 16) { die("16-bit output is only possible for PNG"); }
                /* the default name would replace .jpg by .jpg: the input itself */
                if(nout == 0) { die("-j needs an output file name (-o) for every input"); }
        }
        if(S_arg) {
                static const struct { const char *name; unsigned w, h; } subs[] = {{"444", 1, 1}, {"422", 2, 1}, {"420", 2, 2}, {"440", 1, 2}};
                unsigned k = 0;
                while(k < 4 && strcmp(S_arg, subs[k].name) != 0) { k++; }
                if(k == 4) { die("invalid chroma subsampling"); }
                if(!j_arg) { die("-S needs JPEG output (-j)"); }
                if(o.grey && k != 0) { die("chroma subsampling needs a colour output"); }
                o.sub_w = subs[k].w;
                o.sub_h = subs[k].h;
        }
        if(o.encode_on_gpu && !j_arg) { die("-e needs JPEG output (-j)"); }
        if(o.optimize && !j_arg) { die("-O needs JPEG output (-j)"); }
        if(o.progressive && !j_arg) { die("-r needs JPEG output (-j)"); }
        if(R_arg) {
                char *end = NULL;
                const unsigned long n = strtoul(R_arg, &end, 10);
                const bool blocks = end != R_arg && (*end == 'B' || *end == 'b') && end[1] == '\0';
                if(end == R_arg || (*end != '\0' && !blocks) || R_arg[0] == '-' || n < 1 || n > 65535) { die("invalid restart interval"); }
                if(!j_arg) { die("-R needs JPEG output (-j)"); }
                o.restart_interval = blocks ? (unsigned)n : 0;
                o.restart_in_rows = blocks ? 0 : (unsigned)n;
        }
        if(o.png_on_gpu && j_arg) { die("-P writes a PNG: not with JPEG output (-j)"); }
        /* the reference leaves the thread count to OpenMP, i.e. one per online core (jpeg2png.c:246-257) */
        long cores = sysconf(_SC_NPROCESSORS_ONLN);
        unsigned threads = cores > 0 ? (unsigned)cores : 1u;
        if(t_arg) {
                if(sscanf(t_arg, "%u", &threads) != 1 || threads == 0) { die("invalid number of threads"); }
        }
        if(c_arg) {
                o.csv = fopen(c_arg, "wb");
                if(!o.csv) { die_perror("could not open csv log `%s`", c_arg); }
                if(fprintf(o.csv, "filename,channel,iteration,objective,prob_dist,tv,tv2\n") < 0) {
                        die_perror("could not write to csv log");
                }
        }
        const char *devs = getenv("J2P_DEVICES");
        if(!devs) { devs = getenv("J2P_DEVICE"); }
        if(devs && *devs) {
                o.ndev = 0;
                char *copy = strdup(devs), *save = NULL;
                for(char *tok = strtok_r(copy, ",", &save); tok && o.ndev < 16; tok = strtok_r(NULL, ",", &save)) {
                        o.devs[o.ndev++] = atoi(tok);
                }
                free(copy);
                if(o.ndev == 0) { o.ndev = 1; o.devs[0] = 0; }
        }

        /* (fewer files than GPUs: the images would be row-tiled over them, and a row-tiled job has no upright output) */
        if(o.auto_orient && o.ndev > 1 && nin < (unsigned)o.ndev) { die("-a is not supported for row-tiled images (fewer files than GPUs)"); }
        if(!(nout == 0 || nout == nin)) { die("must give output file names for all input files or none"); }
        char **outfiles = malloc(sizeof(*outfiles) * nin);
        if(!outfiles) { die("could not allocate outfiles"); }
        for(unsigned i = 0; i < nin; i++) {
                if(nout) { outfiles[i] = outs[i]; continue; }
                const char *infile = ins[i];
                FILE *in = fopen(infile, "rb");
                if(!in) { die("could not open input file `%s`", infile); }
                fclose(in);
                size_t l = strlen(infile), e = l;                       /* jpeg2png.c:291-301 */
                if(l >= 5 && memcmp(".jpeg", infile + l - 5, 5) == 0) { e = l - 5; }
                else if(l >= 4 && memcmp(".jpg", infile + l - 4, 4) == 0) { e = l - 4; }
                char *outfile = malloc(e + 5);
                if(!outfile) { die("could not allocate outfile"); }
                memcpy(outfile, infile, e);
                memcpy(outfile + e, ".png", 5);
                if(!force) {
                        FILE *exists = fopen(outfile, "rb");
                        if(exists) { die("not overwriting output file `%s`", outfile); }
                }
                FILE *probe = fopen(outfile, "wb");
                if(!probe) { die("could not open output file `%s`", outfile); }
                fclose(probe);
                remove(outfile);
                outfiles[i] = outfile;
        }

        if(!o.quiet) {
                pthread_mutex_lock(&ui_lock);
                bar_max = o.joint || o.grey ? nin * o.iterations[0] : nin * (o.iterations[0] + o.iterations[1] + o.iterations[2]);
                if(bar_max == 0) { bar_max = 1; }
                bar_cur = 0;
                bar_on = true;
                bar_draw();
                pthread_mutex_unlock(&ui_lock);
        }

        struct work w = {.nin = nin, .next = 0, .in = ins, .out = outfiles, .o = &o};
        pthread_mutex_init(&w.lock, NULL);
        if(threads > nin) { threads = nin; }
        /* as many GPU slots as files in flight, spread over the devices of J2P_DEVICES; with fewer files than GPUs
         * the GPUs are shared out among the files and the library tiles every image over its share (decode_file ->
         * compute of one large image, jpeg2png.c:141-152) when the image is large enough for that to pay */
        o.tile = o.ndev > 1 && nin < (unsigned)o.ndev;
        o.nfiles = nin;
        batch_ndev = (unsigned)o.ndev;
        memcpy(batch_devs, o.devs, sizeof(batch_devs));
        batch_slots = (threads + batch_ndev - 1) / batch_ndev;
        if(batch_slots > 16) { batch_slots = 16; }
        pthread_t *tid = malloc(sizeof(*tid) * threads);
        for(unsigned t = 1; t < threads; t++) { pthread_create(&tid[t], NULL, worker, &w); }
        worker(&w);
        for(unsigned t = 1; t < threads; t++) { pthread_join(tid[t], NULL); }
        free(tid);
        if(batch) { j2p_batch_destroy(batch); }

        if(!nout) { for(unsigned i = 0; i < nin; i++) { free(outfiles[i]); } }
        free(outfiles);
        free(outs);
        if(!o.quiet) {
                pthread_mutex_lock(&ui_lock);
                bar_clear();
                bar_on = false;
                pthread_mutex_unlock(&ui_lock);
        }
        if(o.csv) { fclose(o.csv); }
        return 0;
}
