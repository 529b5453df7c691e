// jpeg2png_amd — declarations shared by the translation units of libjpeg2png_amd.so; not part of the C-ABI.
#pragma once
#include <stdlib.h>
#include "jpeg2png_amd.h"

// ---- the part compute_host.c (C11) shares with the HIP translation units ----
#ifdef __cplusplus
extern "C" {
#endif

// sets the calling thread's j2p_last_error() text (j2p_solver.hip)
void j2p_set_last_error(const char *msg);
// true when J2P_TILED_EXCHANGE / J2P_TILED_WAIT name an exchange: one that cannot be had is then an error, not a reason to
// solve on one GPU (j2p_tiled.hip)
int j2p_tiled_exchange_forced(void);
// the device whose plain device memory p points into (hipPointerGetAttributes); J2P_EINVAL without an error text for host,
// managed and unknown memory (j2p_output.hip) — what tensor output checks its destination with
int j2p_device_of_pointer(const void *p, int *device);
// what kind of memory p points into (hipPointerGetAttributes), for sample input, which takes two kinds: plain device memory
// (*device: whose), host memory (pageable or pinned), or anything else — managed memory above all, which is refused
#define J2P_MEMORY_HOST 0
#define J2P_MEMORY_DEVICE 1
#define J2P_MEMORY_OTHER 2
int j2p_memory_of_pointer(const void *p, int *device);

// bytes of one tensor element of a J2P_DTYPE_* code (u8 1, f32 4, the 16-bit kinds 2)
static inline unsigned j2p_tensor_element_bytes(int dtype) { return dtype == J2P_DTYPE_U8 ? 1 : (dtype == J2P_DTYPE_F32 ? 4 : 2); }

// what is wrong with a j2p_resize for a w x h image, or NULL: what j2p_planes_to_tensor_resized and j2p_batch_submit_resized
// both refuse with J2P_EINVAL
static inline const char *j2p_resize_error(const j2p_resize *r, unsigned w, unsigned h)
{
        if(!r) { return "resize is NULL"; }
        if(r->box_w == 0 || r->box_h == 0) { return "resize: empty box"; }
        if(r->box_x >= w || r->box_w > w - r->box_x || r->box_y >= h || r->box_h > h - r->box_y) { return "resize: the box leaves the image"; }
        if(r->out_w == 0 || r->out_h == 0) { return "resize: empty output"; }
        if(r->out_w > r->box_w || r->out_h > r->box_h) { return "resize: the output is larger than the box (enlarging is what zooming is for)"; }
        return NULL;
}

// the same for a j2p_resample (j2p_planes_to_tensor_resampled, j2p_batch_submit_resampled): the output may be larger than the box
static inline const char *j2p_resample_error(const j2p_resample *r, unsigned w, unsigned h)
{
        if(!r) { return "resample is NULL"; }
        if(r->filter != J2P_FILTER_TRIANGLE && r->filter != J2P_FILTER_CUBIC) { return "resample: unknown filter"; }
        if(r->box_w == 0 || r->box_h == 0) { return "resample: empty box"; }
        if(r->box_x >= w || r->box_w > w - r->box_x || r->box_y >= h || r->box_h > h - r->box_y) { return "resample: the box leaves the image"; }
        if(r->out_w == 0 || r->out_h == 0) { return "resample: empty output"; }
        if(r->out_w > J2P_RESAMPLE_MAX_OUT || r->out_h > J2P_RESAMPLE_MAX_OUT) { return "resample: the output is larger than 65536"; }
        return NULL;
}

// the same for a j2p_jpeg of ncomp components (j2p_planes_to_jpeg, j2p_entropy_encode, j2p_batch_submit_jpeg)
static inline const char *j2p_jpeg_error(const j2p_jpeg *spec, unsigned ncomp)
{
        if(!spec) { return "jpeg: spec is NULL"; }
        if(ncomp != 1 && ncomp != 3) { return "jpeg: three components or one"; }
        if(spec->width == 0 || spec->height == 0 || spec->width > 65535 || spec->height > 65535) { return "jpeg: width and height must be 1..65535"; }
        if(ncomp == 3 && (spec->sub_w < 1 || spec->sub_w > 2 || spec->sub_h < 1 || spec->sub_h > 2)) { return "jpeg: sampling factors must be 1 or 2"; }
        for(unsigned c = 0; c < ncomp; c++) {
                if(!spec->quant[c]) { return "jpeg: a quantisation table is NULL"; }
                for(int j = 0; j < 64; j++) {
                        if(spec->quant[c][j] == 0) { return "jpeg: a quantisation step is zero"; }
                        if(spec->quant[c][j] > 255) { return "jpeg: a quantisation step is above 255 (the file is 8-bit baseline)"; }
                }
        }
        for(int j = 0; ncomp == 3 && j < 64; j++) {
                if(spec->quant[2][j] != spec->quant[1][j]) { return "jpeg: quant[2] differs from quant[1] (the file has two table slots)"; }
        }
        return NULL;
}

// the same for a j2p_png of `channels` samples per pixel (j2p_planes_to_png, j2p_png_encode, j2p_batch_submit_png)
static inline const char *j2p_png_error(const j2p_png *spec, unsigned channels)
{
        if(!spec) { return "png: spec is NULL"; }
        if(channels != 1 && channels != 3) { return "png: three samples per pixel (RGB) or one (greyscale)"; }
        if(spec->width == 0 || spec->height == 0 || spec->width > J2P_PNG_SIDE_MAX || spec->height > J2P_PNG_SIDE_MAX) {
                return "png: width and height must be 1..16777216";
        }
        if(spec->bits != 8 && spec->bits != 16) { return "png: bits must be 8 or 16"; }
        if(spec->filter < J2P_PNG_FILTER_ADAPTIVE || spec->filter > 4) { return "png: filter must be 0..4, or J2P_PNG_FILTER_ADAPTIVE"; }
        if(spec->block_bytes && (spec->block_bytes < J2P_PNG_SIZE_MIN || spec->block_bytes > J2P_PNG_SIZE_MAX)) {
                return "png: block_bytes must be 0 (the default) or 16..16777216";
        }
        if(spec->idat_bytes && (spec->idat_bytes < J2P_PNG_SIZE_MIN || spec->idat_bytes > J2P_PNG_SIZE_MAX)) {
                return "png: idat_bytes must be 0 (the default) or 16..16777216";
        }
        return NULL;
}

// ---- reading a JPEG file (j2p_jpeg_parse.c, pure C; the decode kernels of j2p_decode_kernels.hip.h) ----
// One Huffman table in the form the kernels look symbols up in (the choice and what it costs: DESIGN.md section 21): an 8-bit
// first level for the codes of up to 8 bits — look[the next 8 bits] = (length << 8) | symbol, 0 when the code is longer —
// and per length 9..16 the canonical decode of T.81 F.2.2.3: the next `length` bits are a code of that length when they are
// <= maxcode[length] (-1: no code of that length), and its symbol is vals[bits + valoff[length]].
typedef struct j2p_huff_decode {
        uint16_t look[256];
        int32_t maxcode[17], valoff[17];
        uint8_t vals[256];
        uint32_t defined;
} j2p_huff_decode;
// everything j2p_jpeg_parse_full reads: what the caller sees (info) and what only the decoder needs
typedef struct j2p_jpeg_parsed {
        j2p_jpeg_info info;
        uint16_t quant[4][64];          // by slot, natural order
        unsigned quant_defined;         // bit per slot
        j2p_huff_decode dc[4], ac[4];   // by slot
} j2p_jpeg_parsed;
// the marker segments of `file`: J2P_OK, J2P_EFORMAT or J2P_ENOTSUP (include/jpeg2png_amd.h); touches no device
int j2p_jpeg_parse_full(const uint8_t *file, size_t size, j2p_jpeg_parsed *out);
// everything j2p_jpeg_parse_scans_full reads ("Reading a progressive JPEG file").  base: the frame, the quantisation tables and, for a
// sequential file (scans.progressive == 0), the whole baseline parse.  pool: every Huffman table the file defines, in file order;
// a scan's tables are the ones in force at its SOS: dc_table[s][c] for component c of a DC first scan, ac_table[s] for an AC scan.
typedef struct j2p_scans_parsed {
        j2p_jpeg_parsed base;
        j2p_jpeg_scans scans;
        unsigned ntables;
        uint16_t dc_table[J2P_DECODE_SCANS_MAX][3], ac_table[J2P_DECODE_SCANS_MAX];
        j2p_huff_decode pool[J2P_SCAN_TABLES_MAX];
} j2p_scans_parsed;
int j2p_jpeg_parse_scans_full(const uint8_t *file, size_t size, j2p_scans_parsed *out);

// Iterations per device round trip WHEN SOMEBODY IS WATCHING (a progress bar, log rows: compute.c:428,449-452 tick once per
// iteration, in real time).  A host sync per iteration would cost a small image most of its speed and a fixed chunk moves
// the bar of the default `-i 50` twice; so chunks follow the clock: one iteration each at first, then a sixth of the
// iterations done so far (every chunk ~1/6 of the time elapsed: the bar of `-i 50` moves ~24 times, 4096^2 `-i 500` syncs
// ~36 times = under 1 % of its 60 ms), never more than ~J2P_CHUNK_MS worth or J2P_CHUNK_MAX (the callers' row buffers),
// never more than are left.  elapsed_ms: since the loop began, for the `done` iterations so far.
#define J2P_CHUNK_MAX 256u
#define J2P_CHUNK_MS 50.0
static inline unsigned j2p_next_chunk(unsigned done, unsigned left, double elapsed_ms)
{
        unsigned chunk = done / 6;
        if(done) {
                const double per_it = elapsed_ms / (double)done;
                const double most = per_it > 0. ? J2P_CHUNK_MS / per_it : (double)J2P_CHUNK_MAX;
                if((double)chunk > most) { chunk = (unsigned)most; }
        }
        if(chunk > J2P_CHUNK_MAX) { chunk = J2P_CHUNK_MAX; }
        if(chunk < 1) { chunk = 1; }
        return left < chunk ? left : chunk;
}

// The most tile rows whose sums ONE in-kernel tree turns into ||g||: the tree at the end of a folding k_gradient launch and
// the one k_project's wavefronts run (j2p_kernels.hip.h size their arrays by it), hence also where the solver's norm plan
// (j2p_solver.hip: norm_plan) and the row tiling's exchange picker (j2p_tiled.hip) fall back to a k_norm_finish launch or
// to the copy exchange.  Canvas height <= 16384 at 16-row tile rows.
#define J2P_NORM_TREE_ROWS 1024u

#ifdef __cplusplus
}  // extern "C"

#include <hip/hip_runtime_api.h>     // hipStream_t, hipError_t: every C++ unit of the library is a HIP unit
#include <functional>
#include <memory>

// Environment knobs of the EXPERIMENTS build (-DJ2P_EXPERIMENTS: jpeg2png_amd/libjpeg2png_amd_exp.so, built by
// buildlib.build_experiments() for the schedule-equivalence tests and the timing tools): the switches that move choices
// AMONG the release kernels (rows per strip, item shares, launch direction, where the norm is finished, ...) and the
// split phases.  Its device code is the release build's.  The release library carries neither the switches nor the split
// phases and reads only J2P_DEVICE, J2P_DEVICES, J2P_TILED_EXCHANGE, J2P_TILED_WAIT, J2P_TILED_VERIFY, J2P_RCCL_LIBRARY,
// J2P_POOL_MIB, J2P_COMPUTE_TIMING and J2P_PHASE_ORDER (the value of J2P_OPT_PHASE_ORDER for every solver created: the
// benchmark can then be run in either launch order as it stands).
static inline const char *j2p_exp_env(const char *name)
{
#ifdef J2P_EXPERIMENTS
        return getenv(name);
#else
        (void)name;
        return nullptr;
#endif
}

// error text of the calling thread (what j2p_last_error() returns); returns `code`
int j2p_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// ---- what the output stage (j2p_output.hip) sees of a solver; defined in j2p_solver.hip ----
// The solver's place and state as far as converting its planes needs them.  A copy: valid until the solver is next used.
struct j2p_solver_view {
        int device;
        hipStream_t stream;
        unsigned nch;
        unsigned W, H;                  // the canvas
        unsigned row0, rows;            // the canvas rows this solver holds: [row0, row0 + rows)
        bool whole;                     // ... which are all of them (not a band)
        bool mid_iteration;             // between the two phases of an iteration: the planes are not an iterate
        unsigned orientation;           // j2p_solver_set_orientation: 1 = none, otherwise of a source image of orient_w x orient_h
        unsigned orient_w, orient_h;
};
j2p_solver_view j2p_solver_view_of(const j2p_solver *s);         // s is not NULL
// the device address of canvas row y (one of the solver's own) of channel c in the current iterate; the rows after it follow
// at a stride of W floats.  Hides the halo as j2p_solver_plane_ptr does.
int j2p_solver_row(const j2p_solver *s, unsigned c, unsigned y, const float **row);
// at least `bytes` bytes of device memory that belong to the solver until it is destroyed, for what the output stage queues on
// the solver's stream: taken from the pool once and grown on demand (growing waits for the stream, since what is queued may
// still read the old block; a call that fits allocates nothing and waits for nothing).  One block: every call returns the same
// memory, and stream order is what makes the next call's writes safe.
int j2p_solver_scratch(j2p_solver *s, size_t bytes, void **out);
// the size of that block now (0: none yet): a request beyond it gets ANOTHER block, and what the old one held is lost
size_t j2p_solver_scratch_bytes(const j2p_solver *s);
// the same kind of block, a second one, for the upright planes of the calls this solver is the first plane of (j2p_output.hip,
// "upright planes"): live
// together with the scratch, which the forms that run on the upright planes use as before
int j2p_solver_upright(j2p_solver *s, size_t bytes, float **out);

// ---- the JPEG codec (j2p_codec.hip) ----
// offsets of the parts of one block of device memory, in the order asked for, each aligned to 256 bytes
struct j2p_carve {
        size_t total = 0;
        size_t operator()(size_t bytes)
        {
                const size_t at = total;
                total += ((bytes ? bytes : 1) + 255) / 256 * 256;
                return at;
        }
};
// bytes of a component's coefficient grid of bw x bh blocks
static inline size_t j2p_grid_bytes(unsigned bw, unsigned bh) { return (size_t)bw * bh * 64 * sizeof(int16_t); }

// the block grids of the file j2p_encode_options writes from a spec that j2p_jpeg_error accepted: component c's grid has
// bw[c] x bh[c] blocks; sub_w x sub_h of component 0's make an MCU (1 x 1 for one component)
struct j2p_scan_grids {
        unsigned sub_w, sub_h, bw[3], bh[3];
};
j2p_scan_grids j2p_scan_grids_of(const j2p_jpeg &spec, unsigned ncomp);
// The coder: the file of `spec` that `options` describe (include/jpeg2png_amd.h: "Restart intervals" has the record), on the host,
// from coefficients the caller leaves in device memory, on `stream`, which has been waited for on return.  memory(bytes, &p, &moved):
// one block of device memory of at least that size which stays the same block while it is large enough and is ANOTHER block (moved),
// contents lost, once it has to grow (j2p_solver_scratch); fill(stream, coef): queues what leaves component c's coefficients
// (j2p_scan_grids_of) at coef[c].  Both may be called up to three times, by the coder's j2p_coder_block (j2p_coder_block.h).
// J2P_ESPACE: *size is what the file needs.  options has passed j2p_jpeg_options_error.  The record chooses the coder in
// j2p_codec.hip — the progressive one for options.progressive, else the baseline one with options.flags — and its restart plan
// (j2p_restart.h); with all of it 0 the launches and the bytes are the baseline file's as they ever were.  stats,
// progressive_stats, restart_stats: may be NULL; the one of the other coder is left alone.  With J2P_JPEG_OPTIMIZE, with stats or
// in a progressive file the symbols are counted on the device and the stream is waited for once more on the way.
int j2p_encode_options(hipStream_t stream, const j2p_jpeg &spec, unsigned ncomp, const j2p_jpeg_options &options,
                       const std::function<int(size_t, void **, bool *)> &memory, const std::function<void(hipStream_t, int16_t *const[3])> &fill,
                       uint8_t *out_host, size_t capacity, size_t *size, j2p_encode_stats *stats = nullptr,
                       j2p_progressive_stats *progressive_stats = nullptr, j2p_restart_stats *restart_stats = nullptr);
// what is wrong with the record of a call that writes a JPEG file, or NULL
const char *j2p_jpeg_options_error(const j2p_jpeg_options *options);

// The PNG coder: the file of `spec` on the host from `channels` (1 or 3) interleaved samples per pixel that the caller leaves in
// device memory, on `stream`, which has been waited for on return (twice on the way: the blocks' counts come down for the host's
// tables).  memory: as for j2p_encode_options; fill(stream, samples): queues what leaves the width * height * channels * bits / 8 bytes
// of samples (16 bits: big-endian) at `samples`.  Both may be called twice.  J2P_ESPACE: *size is what the file needs, known before
// anything is packed.  spec has passed j2p_png_error.  stats may be NULL.
int j2p_png_write(hipStream_t stream, const j2p_png &spec, unsigned channels, const std::function<int(size_t, void **, bool *)> &memory,
                  const std::function<void(hipStream_t, uint8_t *)> &fill, uint8_t *out_host, size_t capacity, size_t *size,
                  j2p_png_stats *stats = nullptr);

// A JPEG file opened for decoding: its marker segments parsed on the host (from a temporary copy for a file in device memory),
// and where the caller's bytes are, which the decode reads in place.
struct j2p_jpeg_file {
        std::unique_ptr<j2p_jpeg_parsed> parsed;
        std::unique_ptr<j2p_scans_parsed> scans;        // j2p_jpeg_open_scans: every scan; info() is then scans->base.info
        const j2p_jpeg_info &info() const { return scans ? scans->base.info : parsed->info; }
        const uint8_t *scan = nullptr;  // the caller's bytes from info.scan_begin on
        bool on_device = false;         // ... which are plain device memory
        int device = -1;                // ... of this device (-1: host memory)
};
// J2P_EINVAL (NULL or empty; managed or unknown memory), J2P_ENOMEM, J2P_EDEVICE (the copy), or what j2p_jpeg_parse_full says
int j2p_jpeg_open(const uint8_t *file, size_t size, j2p_jpeg_file *opened);
// ... through the scans parser: scans is set, and parsed too for a sequential file (then j2p_decode_file decodes it)
int j2p_jpeg_open_scans(const uint8_t *file, size_t size, j2p_jpeg_file *opened);
// parsed's scan, whose bytes begin at `data` (host memory, or device memory of `device` read in place), decoded into the device
// grids coef[c] (blocks_w * blocks_h * 64 int16) on `stream`; waits for the stream.  S: bits per subsequence, 0 the default.
// The calling thread's device is `device`.  J2P_EFORMAT: the grids hold nothing of use.
int j2p_decode_file(int device, hipStream_t stream, const j2p_jpeg_parsed *parsed, const uint8_t *data, bool data_on_device, unsigned S,
                    int16_t *const coef[3], j2p_decode_stats *stats);
struct j2p_jpeg_file;
// an opened file's decode, whichever way it was opened (scans_stats: what a file opened by j2p_jpeg_open_scans fills; both may be NULL)
int j2p_decode_opened(int device, hipStream_t stream, const j2p_jpeg_file &file, unsigned S, int16_t *const coef[3], j2p_decode_stats *stats,
                      j2p_scans_stats *scans_stats);
// every scan of a progressive file (p->scans.progressive), whose bytes from info.scan_begin on are `data`: j2p_decode_file's contract
int j2p_decode_scans_file(int device, hipStream_t stream, const j2p_scans_parsed *p, const uint8_t *data, bool data_on_device, unsigned S,
                          int16_t *const coef[3], j2p_scans_stats *stats);
// The component grids of an opened file in one pooled block of `device` (the calling thread's), each at a 256-byte step, on a
// stream of their own: construction decodes (j2p_decode_file), `rc` is what came of it, and only after J2P_OK do the grids hold
// anything.  Destruction waits for the stream, destroys it and gives the block back.
struct j2p_decoded_grids {
        int rc = J2P_OK;
        int16_t *coef[3] = {nullptr, nullptr, nullptr};
        size_t at[3] = {0, 0, 0};       // coef[c] is the block + at[c]
        void *block = nullptr;
        size_t bytes = 0;               // the block's first bytes, which hold the grids
        j2p_decoded_grids(int device, const j2p_jpeg_file &file, unsigned S, j2p_decode_stats *stats, j2p_scans_stats *scans_stats = nullptr);
        ~j2p_decoded_grids();
        j2p_decoded_grids(const j2p_decoded_grids &) = delete;
        j2p_decoded_grids &operator=(const j2p_decoded_grids &) = delete;

private:
        int device_;
        hipStream_t stream_ = nullptr;
        size_t block_bytes_ = 0;
        int decode(const j2p_jpeg_file &file, unsigned S, j2p_decode_stats *stats, j2p_scans_stats *scans_stats);
};

// a whole-canvas solver whose coefficients a decode has left in device memory of `device` (decoded[c]: channel c's grid,
// planes[c].w / 8 x planes[c].h / 8 blocks; planes carry no arrays), copied into the resident buffers on the solver's own stream;
// the grids may go away when it returns (j2p_solver.hip; what a batch job with a file makes its solvers with)
int j2p_solver_create_from_decoded(j2p_solver **out, int device, unsigned nchannel, const j2p_plane planes[], const int16_t *const decoded[],
                                   float weight, const float pweight[], unsigned iterations);

// ---- j2p_pool.hip ----
// the device-memory pool, for a solver's arena and for buffers that live as long as one call: at least `bytes` bytes on
// `device`, *got the size to give back with
hipError_t j2p_pool_take(int device, size_t bytes, void **out, size_t *got);
void j2p_pool_give(int device, void *ptr, size_t bytes);
// hipMalloc that returns the pool's cached blocks to the device and tries once more when memory is short
hipError_t j2p_dev_malloc(void **out, size_t bytes);
// What is live on each device, for the non-temporal policy (j2p_solver.hip: nt_policy): the Infinity Cache is shared by
// every solver iterating on the GPU — the images of a batch, the components of `-s`, the bands of a tiled run that
// share a device — so the policy looks at the sum of their working sets, not at one solver's.
struct LiveBytes {
        size_t working_set = 0, g = 0, planes = 0, d = 0;
};
void j2p_live_add(int device, const LiveBytes &b, int sign);    // sign > 0: b joins the device's total, otherwise leaves it
LiveBytes j2p_live_on(int device);

// log rows from per-iteration sums like j2p_log_rows_from_sums(), but continuing a run: carried[] holds the prob
// distance per channel of the state entering the first of the n iterations and is updated (all 0 at iteration 0);
// !carried_valid: that distance is unknown (the previous iterations ran without logging) and the first row
// reports NaN for prob_dist and objective, as j2p_solver_run does
void j2p_rows_from_sums_carry(unsigned nch, float weight, const float *pweight, unsigned n, const double *sums,
                              double *carried, bool carried_valid, j2p_log_row *rows);


// test hook behind j2p_debug_fail_run_after(): true when THIS run call is the one that has to fail
bool j2p_injected_failure();
// ... (negative argument) true when the LAST band of this threaded run has to fail halfway through its iterations
bool j2p_injected_band_failure();
#endif  // __cplusplus
