// jpeg2png_amd — image batches over streams and GPUs (BASELINE.json configs[4]; the file loop jpeg2png.c:330-337
// and decode_file's compute calls, jpeg2png.c:141-152).
//
// A j2p_batch owns `slots_per_device` worker threads per GPU.  A job is one image — what decode_file() does
// between read_jpeg() and write_png(): one joint compute(3, ...) or three separate compute(1, ...) calls, then the
// planes handed back as floats or, converted on the device (png.c:37-62), as RGB samples (greyscale ones for a
// one-channel job), as quantised coefficients, or left on the device as a tensor (a job that only workers of the tensor's
// GPU take).  Every worker drives its jobs on streams of its own, so while one slot's image is being solved
// the next slot's coefficients go up and a third one's pixels come down: H2D / solve / D2H overlap without any of
// them knowing about the others.  Device memory comes from the library's pool (one arena per solver, recycled
// between jobs): after the first few images a job performs no hipMalloc / hipFree — the device-wide synchronisation
// inside hipFree is what used to serialise concurrent compute() calls.
#include <hip/hip_runtime.h>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <optional>
#include <thread>
#include <vector>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jpeg2png_amd.h"
#include "j2p_internal.h"
#include "j2p_geometry.h"

namespace {

// The optional parts of a job.  j2p_job may not grow, so they arrive next to it: every entry point fills in the ones it carries,
// and classify() turns the job and its request into the one record, Job, that everything downstream reads.
struct Request {
        const j2p_resize *resize = nullptr;
        const j2p_resample *resample = nullptr;
        unsigned nout = 0;
        const j2p_output *outs = nullptr;
        const j2p_samples *samples = nullptr;
        const uint8_t *file = nullptr;
        size_t file_size = 0;
        const j2p_jpeg *jpeg = nullptr;     // the file the job delivers, with where it goes:
        uint8_t *jpeg_out = nullptr;
        size_t jpeg_capacity = 0, *jpeg_size = nullptr;
        j2p_jpeg_options jpeg_options = {0, 0, 0, 0};   // ... and which file it is: the caller's record as it came, for validate_jpeg
        unsigned orientation = 0, orient_w = 0, orient_h = 0;    // j2p_batch_next_orientation: what the calling thread set for this submit
        bool file_scans = false;                                 // j2p_batch_next_file_scans: the file goes through the scans parser
        const j2p_png *png = nullptr;       // the PNG file the job delivers, with where it goes:
        uint8_t *png_out = nullptr;
        size_t png_capacity = 0, *png_size = nullptr;
        bool estimate = false;              // j2p_batch_submit_samples_estimated: the tables are read off the samples ...
        j2p_quant_estimate_result *estimates = nullptr;     // ... and reported here (or nowhere)
        Request &estimated(j2p_quant_estimate_result *e) { estimate = true, estimates = e; return *this; }
        Request &resized(const j2p_resize *r) { resize = r; return *this; }
        Request &resampled(const j2p_resample *r) { resample = r; return *this; }
        // (no outputs, or an array that is not there, is the job's own output)
        Request &outputs(unsigned n, const j2p_output *o) { if(n && o) { nout = n, outs = o; } return *this; }
        Request &from_samples(const j2p_samples *m) { samples = m; return *this; }
        Request &from_file(const uint8_t *f, size_t size) { file = f, file_size = size; return *this; }
        Request &jpeg_to(const j2p_jpeg *spec, uint8_t *out, size_t capacity, size_t *size, const j2p_jpeg_options &options)
        {
                jpeg = spec, jpeg_out = out, jpeg_capacity = capacity, jpeg_size = size, jpeg_options = options;
                return *this;
        }
        Request &png_to(const j2p_png *spec, uint8_t *out, size_t capacity, size_t *size)
        {
                png = spec, png_out = out, png_capacity = capacity, png_size = size;
                return *this;
        }
};

// what a job's solvers are made from: planes[].data / fdata, Job::samples, or Job::file
enum class In { planes, samples, file };
// what becomes of the solve: the job's own out_* fields (samples, coefficients or out_tensor's rows, and out_planes), out_tensor
// filled through Job::resize or Job::resample, Job::outputs, Job::jpeg or Job::png.  out_planes come down after every form without
// out_bits.
enum class Out { own, resized, resampled, outputs, jpeg, png };

// where the file of an Out::jpeg job goes; spec.quant[] point into tables[] (so a JpegOut stays where it was set)
struct JpegOut {
        j2p_jpeg spec = {0, 0, 0, 0, {nullptr, nullptr, nullptr}};
        uint16_t tables[3][64];
        uint8_t *out = nullptr;
        size_t capacity = 0, *size = nullptr;
        j2p_jpeg_options options = {0, 0, 0, 0};
        // from a request that validate_jpeg has passed: the tables travel with the job
        void set(const Request &q, unsigned nchannel)
        {
                spec = *q.jpeg;
                options = q.jpeg_options;
                out = q.jpeg_out, capacity = q.jpeg_capacity, size = q.jpeg_size;
                for(unsigned c = 0; c < nchannel; c++) {
                        memcpy(tables[c], q.jpeg->quant[c], sizeof(tables[c]));
                        spec.quant[c] = tables[c];
                }
        }
};

// where the file of an Out::png job goes
struct PngOut {
        j2p_png spec = {0, 0, 0, 0, 0, 0};
        uint8_t *out = nullptr;
        size_t capacity = 0, *size = nullptr;
};

struct Job {
        j2p_job desc;                       // (of a file job: with the sizes it left zero filled in from the file)
        In in = In::planes;
        Out out = Out::own;
        std::vector<j2p_samples> samples;   // In::samples: [channel]
        bool estimate = false;              // In::samples: the worker estimates the tables (planes[].quant_table is not read) ...
        j2p_quant_estimate_result *estimates = nullptr;     // ... and reports them here, [channel], when the caller wants them
        j2p_jpeg_file file;                 // In::file: opened at submit; the worker decodes the solvers' coefficients from the caller's
                                            // bytes, which stay valid until j2p_batch_wait
        j2p_resize resize = {0, 0, 0, 0, 0, 0};          // Out::resized
        j2p_resample resample = {0, 0, 0, 0, 0, 0, 0};   // Out::resampled
        std::vector<j2p_output> outputs;    // Out::outputs: never empty
        JpegOut jpeg;                       // Out::jpeg
        PngOut png;                         // Out::png
        unsigned orientation = 0, orient_w = 0, orient_h = 0;   // j2p_batch_next_orientation, settled at submit: 0 / 1 none, 2..8 of that source size
        int ticket = 0;
        int device = -1;                    // tensors, device samples, a file in device memory: their GPU, the only one whose workers may take the job
        int rc = J2P_OK;
        bool finished = false;
        char err[256] = "";
};

}  // namespace

struct j2p_batch {
        std::vector<int> devices;           // as given to j2p_batch_create
        std::vector<int> worker_device;
        std::vector<std::thread> workers;
        std::mutex lock;
        std::condition_variable work, finished;
        std::deque<Job *> queue;            // (the batch owns a job from here until j2p_batch_wait has collected it)
        std::map<int, Job *> jobs;          // every job not yet collected by j2p_batch_wait
        int next_ticket = 1;
        bool quit = false;
};

namespace {

#define JOB_TRY(expr)                                                                              \
        do {                                                                                       \
                const int rc_ = (expr);                                                            \
                if(rc_ != J2P_OK) { return rc_; }                                                  \
        } while(0)

// j2p_job::out_sub_w / out_sub_h: 0 means 1, so that zero-initialised jobs are 4:4:4
unsigned out_sub(unsigned v) { return v ? v : 1u; }

// what leaving the image on the device as tensors needs, whether in out_tensor or in outputs
int validate_tensor_form(const j2p_job &d)
{
        if(d.nchannel != 1 && d.nchannel != 3) { return j2p_fail(J2P_EINVAL, "job: tensor output needs three channels (RGB) or one (greyscale)"); }
        if(d.out_w == 0 || d.out_h == 0) { return j2p_fail(J2P_EINVAL, "job: tensor output needs out_w and out_h"); }
        if(d.tile) { return j2p_fail(J2P_EINVAL, "job: tensor output of a row-tiled job is not supported"); }
        return J2P_OK;
}

// The job's own fields: what the worker checks before it touches anything — so a job without tensors learns of it from
// j2p_batch_wait — and what classify() checks at submit for a job with them.
int validate_job(const j2p_job &d)
{
        if(d.nchannel == 0 || d.nchannel > J2P_MAX_CHANNELS) { return j2p_fail(J2P_EINVAL, "job: nchannel must be 1..3"); }
        if(d.out_bits != 0 && d.out_bits != 8 && d.out_bits != 16) { return j2p_fail(J2P_EINVAL, "job: out_bits must be 0, 8 or 16"); }
        if(d.out_bits && (!d.out_rgb || d.nchannel == 2)) {
                return j2p_fail(J2P_EINVAL, "job: sample output needs out_rgb and three channels (RGB) or one (greyscale)");
        }
        if(d.out_bits && (d.out_w == 0 || d.out_h == 0)) { return j2p_fail(J2P_EINVAL, "job: sample output of an empty image"); }
        if(d.out_coef[0]) {
                // coefficient output (JPEG): instead of samples, for every channel
                if(d.out_bits) { return j2p_fail(J2P_EINVAL, "job: coefficient output (out_coef) needs out_bits 0"); }
                if(d.out_blocks_w == 0 || d.out_blocks_h == 0) { return j2p_fail(J2P_EINVAL, "job: coefficient output needs out_blocks_w and out_blocks_h"); }
                for(unsigned c = 0; c < d.nchannel; c++) {
                        if(!d.out_coef[c] || !d.out_quant[c]) { return j2p_fail(J2P_EINVAL, "job: coefficient output needs out_coef and out_quant for channel %u", c); }
                        for(int j = 0; j < 64; j++) {
                                if(d.out_quant[c][j] == 0) { return j2p_fail(J2P_EINVAL, "job: channel %u: output quantisation table entry %d is zero", c, j); }
                        }
                        if(d.out_sub_w[c] > 2 || d.out_sub_h[c] > 2) {
                                return j2p_fail(J2P_EINVAL, "job: channel %u: output sampling factors %ux%u (1 and 2 are supported)", c, d.out_sub_w[c], d.out_sub_h[c]);
                        }
                }
        }
        if(d.out_tensor.data) {
                // tensor output: the image left in device memory, instead of samples and coefficients
                if(d.out_bits || d.out_coef[0]) { return j2p_fail(J2P_EINVAL, "job: tensor output (out_tensor) needs out_bits 0 and no out_coef"); }
                JOB_TRY(validate_tensor_form(d));
        }
        return J2P_OK;
}

// pixels per channel a band must at least have: the cross-band schedule costs every band ~35 us per iteration
// whatever its size (profiles/r03_band_alone.jsonl: 276 vs 245 us for a 2048-row band of a 16384-wide plane), which
// is more than a whole 1080p iteration takes on one GPU
size_t tile_min_band_pixels(const j2p_job &d)
{
        return d.tile_min_band_pixels ? (d.tile_min_band_pixels == (size_t)-1 ? 0 : d.tile_min_band_pixels) : (size_t)2 << 20;
}

// Output channel c of a job is channel 0 of its own solve (`-s`, jpeg2png.c:147-152: one compute(1, ...) per component,
// each with its own weight and iteration count) or channel c of the one joint solve (jpeg2png.c:144: compute(3, ...) with
// the first weight and iteration count).  The only place that knows.
struct Where {
        unsigned solve, channel;
};
Where where(const j2p_job &d, unsigned c) { return d.separate ? Where{c, 0} : Where{0, c}; }
unsigned solves(const j2p_job &d) { return d.separate ? d.nchannel : 1; }

// The k-th solve of a job: one j2p_solver that holds the canvas on one GPU (a single band), or one j2p_tiled with a band
// per GPU.  Never a one-band j2p_tiled: a whole-canvas solver and a band solver pick different norm paths.
struct Engine {
        j2p_solver *s = nullptr;
        j2p_tiled *t = nullptr;
        int run(unsigned n, j2p_log_row *rows) const { return t ? j2p_tiled_run(t, n, rows) : j2p_solver_run(s, n, rows); }
        int sync() const { return t ? j2p_tiled_sync(t) : j2p_solver_sync(s); }
        int download(unsigned c, float *out) const { return t ? j2p_tiled_download(t, c, out) : j2p_solver_download(s, c, out); }
        unsigned nband() const
        {
                unsigned n = 1;
                if(t) { (void)j2p_tiled_canvas(t, nullptr, nullptr, &n); }
                return n;
        }
        // band b's solver and the canvas rows it holds
        int band(unsigned b, j2p_solver **bs, unsigned *row_begin, unsigned *row_end) const
        {
                if(t) { return j2p_tiled_band(t, b, nullptr, row_begin, row_end, bs); }
                *bs = s;
                return j2p_solver_band(s, row_begin, row_end);
        }
};

// the engines of one job, destroyed with it
struct Engines {
        Engine e[J2P_MAX_CHANNELS];
        ~Engines()
        {
                for(Engine &k : e) {
                        if(k.t) { j2p_tiled_destroy(k.t); }
                        if(k.s) { j2p_solver_destroy(k.s); }
                }
        }
};

// Band b of a job's engines as delivery sees it: channel c's plane there and the canvas rows [row0[c], row1[c]) it holds.  The
// solves of a job share their cuts (multiples of 16 rows: of a block row of either sampling) and differ only in where the last
// band ends; the last band takes all that the output has left — the block row that overhangs the canvas too — and the rows
// forms refuse what is not there.
struct Band {
        j2p_plane_ref ref[J2P_MAX_CHANNELS];
        unsigned row0[J2P_MAX_CHANNELS], row1[J2P_MAX_CHANNELS];
        bool last;
        // the band's image rows [*y0, *y1); false: none (a band below the image, canvas padding only)
        bool image_rows(const j2p_job &d, unsigned *y0, unsigned *y1) const
        {
                *y0 = row0[0];
                *y1 = !last && row1[0] < d.out_h ? row1[0] : d.out_h;
                return *y0 < *y1;
        }
};

// ---- the output forms: what one band delivers.  Only the three rows forms are ever row-tiled; for the others the one band is the
// whole canvas.  A form that fills tensors ends with a sync (synced): the ticket says complete, for any stream. ----

int synced(int rc, const Band &band) { return rc != J2P_OK ? rc : j2p_solver_sync(band.ref[0].solver); }

// an oriented job (never row-tiled: its one band is the whole canvas) delivers through the whole-canvas forms, which see the
// upright planes; the rows forms take no oriented solver
bool oriented(const Job &j) { return j.orientation > 1; }

int deliver_samples(const Job &j, const j2p_job &d, const Band &band)
{
        if(oriented(j)) {
                return d.nchannel == 1 ? j2p_planes_to_grey(band.ref, d.out_w, d.out_h, d.out_bits, d.out_rgb)
                                       : j2p_planes_to_rgb(band.ref, d.out_w, d.out_h, d.out_bits, d.out_rgb);
        }
        unsigned y0, y1;
        if(!band.image_rows(d, &y0, &y1)) { return J2P_OK; }
        const size_t row_bytes = (size_t)d.out_w * (d.nchannel == 1 ? 1 : 3) * (d.out_bits / 8);
        uint8_t *out = d.out_rgb + (size_t)y0 * row_bytes;
        if(d.nchannel == 1) { return j2p_planes_rows_to_grey(band.ref, d.out_w, y0, y1, d.out_bits, out); }   // greyscale: one sample per pixel
        return j2p_planes_rows_to_rgb(band.ref, d.out_w, y0, y1, d.out_bits, out);
}

int deliver_tensor_rows(const Job &j, const j2p_job &d, const Band &band)
{
        if(oriented(j)) { return synced(j2p_planes_to_tensor(band.ref, d.nchannel, d.out_w, d.out_h, &d.out_tensor), band); }
        unsigned y0, y1;
        if(!band.image_rows(d, &y0, &y1)) { return J2P_OK; }
        j2p_tensor rows = d.out_tensor;                  // the band's first row of it
        const size_t row_bytes = (size_t)(d.out_tensor.stride_y > 0 ? d.out_tensor.stride_y : 0) * j2p_tensor_element_bytes(d.out_tensor.dtype);
        rows.data = static_cast<char *>(d.out_tensor.data) + (size_t)y0 * row_bytes;
        return synced(j2p_planes_rows_to_tensor(band.ref, d.nchannel, d.out_w, y0, y1, &rows), band);
}

int deliver_coefficients(const Job &j, const j2p_job &d, const Band &band)
{
        for(unsigned c = 0; d.out_coef[0] && c < d.nchannel; c++) {
                const unsigned sx = out_sub(d.out_sub_w[c]), sy = out_sub(d.out_sub_h[c]);
                const unsigned bw = (d.out_blocks_w + sx - 1) / sx, bh = (d.out_blocks_h + sy - 1) / sy;
                if(oriented(j)) {
                        JOB_TRY(j2p_planes_to_coefficients_sub(&band.ref[c], sx, sy, bw, bh, d.out_quant[c], d.out_coef[c]));
                        continue;
                }
                const unsigned r0 = band.row0[c] / (8 * sy), r1 = !band.last && band.row1[c] / (8 * sy) < bh ? band.row1[c] / (8 * sy) : bh;
                if(r0 >= r1) { continue; }                       // band below the image (canvas padding only)
                JOB_TRY(j2p_planes_rows_to_coefficients_sub(&band.ref[c], sx, sy, bw, r0, r1, d.out_quant[c], d.out_coef[c] + (size_t)r0 * bw * 64));
        }
        return J2P_OK;
}

int deliver_resized(const Job &j, const j2p_job &d, const Band &band)
{
        return synced(j2p_planes_to_tensor_resized(band.ref, d.nchannel, d.out_w, d.out_h, &j.resize, &d.out_tensor), band);
}

int deliver_resampled(const Job &j, const j2p_job &d, const Band &band)
{
        return synced(j2p_planes_to_tensor_resampled(band.ref, d.nchannel, d.out_w, d.out_h, &j.resample, &d.out_tensor), band);
}

int deliver_outputs(const Job &j, const j2p_job &d, const Band &band)
{
        return synced(j2p_planes_to_tensors_resampled(band.ref, d.nchannel, d.out_w, d.out_h, (unsigned)j.outputs.size(), j.outputs.data()), band);
}

int deliver_jpeg(const Job &j, const j2p_job &d, const Band &band)
{
        return j2p_planes_to_jpeg_opt(band.ref, d.nchannel, &j.jpeg.spec, j.jpeg.out, j.jpeg.capacity, j.jpeg.size, &j.jpeg.options);
}

int deliver_png(const Job &j, const j2p_job &d, const Band &band)
{
        return j2p_planes_to_png(band.ref, d.nchannel, &j.png.spec, j.png.out, j.png.capacity, j.png.size);
}

int deliver(const Job &j, const Band &band)
{
        const j2p_job &d = j.desc;
        switch(j.out) {
        // (validate_job lets at most one of the three be asked for; none: out_planes only)
        case Out::own: return d.out_bits ? deliver_samples(j, d, band) : d.out_tensor.data ? deliver_tensor_rows(j, d, band) : deliver_coefficients(j, d, band);
        case Out::resized: return deliver_resized(j, d, band);
        case Out::resampled: return deliver_resampled(j, d, band);
        case Out::outputs: return deliver_outputs(j, d, band);
        case Out::jpeg: return deliver_jpeg(j, d, band);
        case Out::png: return deliver_png(j, d, band);
        }
        return J2P_OK;
}

// What a job does once its engines exist: the iterations (compute.c:427-453), then its output form, band by band.
// Chunked when the caller watches (j2p_next_chunk), so that its bar and CSV keep moving.  `overlap`: the chunk of every
// solve is issued before any of them is settled (sync, progress, done) — how the three solves of `-s` overlap on one GPU,
// unless log rows make every run synchronous anyway.  Row-tiled jobs settle each solve right after issuing it.
int solve_and_deliver(const Job &j, const Engine *e, bool overlap)
{
        const j2p_job &d = j.desc;
        const unsigned nsolve = solves(d);
        if(!d.on_rows && !d.on_progress) {
                for(unsigned k = 0; k < nsolve; k++) { JOB_TRY(e[k].run(d.iterations[k], nullptr)); }
        } else {
                j2p_log_row rows[J2P_CHUNK_MAX];
                unsigned done[J2P_MAX_CHANNELS] = {0, 0, 0};
                const auto t_loop = std::chrono::steady_clock::now();
                for(;;) {
                        unsigned step[J2P_MAX_CHANNELS] = {0, 0, 0};
                        const auto settle = [&](unsigned k) {
                                if(!d.on_rows) { JOB_TRY(e[k].sync()); }
                                if(d.on_progress) { d.on_progress(d.user, step[k]); }
                                done[k] += step[k];
                                return (int)J2P_OK;
                        };
                        bool any = false;
                        for(unsigned k = 0; k < nsolve; k++) {
                                const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_loop).count();
                                step[k] = j2p_next_chunk(done[k], d.iterations[k] - done[k], ms);
                                if(!step[k]) { continue; }
                                any = true;
                                JOB_TRY(e[k].run(step[k], d.on_rows ? rows : nullptr));
                                if(d.on_rows) { d.on_rows(d.user, d.separate ? k : 3u, done[k], step[k], rows); }   // channel 3 = joint, jpeg2png.c:143
                                if(!overlap) { JOB_TRY(settle(k)); }
                        }
                        if(!any) { break; }
                        for(unsigned k = 0; overlap && k < nsolve; k++) {
                                if(step[k]) { JOB_TRY(settle(k)); }
                        }
                }
        }
        // every band delivers its own rows from its own GPU
        const unsigned nband = e[0].nband();
        for(unsigned b = 0; b < nband; b++) {
                Band band;
                band.last = b + 1 == nband;
                for(unsigned c = 0; c < d.nchannel; c++) {
                        const Where at = where(d, c);
                        band.ref[c].channel = at.channel;
                        JOB_TRY(e[at.solve].band(b, &band.ref[c].solver, &band.row0[c], &band.row1[c]));
                }
                JOB_TRY(deliver(j, band));
        }
        for(unsigned c = 0; !d.out_bits && c < d.nchannel; c++) {
                if(d.out_planes[c]) { JOB_TRY(e[where(d, c).solve].download(where(d, c).channel, d.out_planes[c])); }
        }
        return J2P_OK;
}

// One image over several of the batch's devices (j2p_job::tile; classify() lets only In::planes jobs with Out::own ask for it):
// every solve of the job becomes a j2p_tiled with band b on devices[b]; the solves of `-s` share their cuts so that band b of the
// three components meets on one GPU for the colour conversion.  Returns J2P_OK with *handled = false when the image should be
// solved on one GPU after all: too small for two bands (rows, or pixels per band), or the devices cannot be tiled over (the
// create phase failed: no peer access and no RCCL, or no room for the band arenas) — the caller then takes the single-solver path.
// Failures after the iterations have started stay failures.
int run_job_tiled(const Job &j, const std::vector<int> &devices, bool *handled)
{
        const j2p_job &d = j.desc;
        *handled = false;
        const unsigned nsolve = solves(d);
        // the canvas of every solve; the alignment is the one all the job's channels share
        j2p_canvas all = J2P_CANVAS_NONE, cv[J2P_MAX_CHANNELS] = {J2P_CANVAS_NONE, J2P_CANVAS_NONE, J2P_CANVAS_NONE};
        for(unsigned c = 0; c < d.nchannel; c++) {
                const j2p_plane &p = d.planes[c];
                if(p.h_samp == 0 || p.h == 0 || p.w_samp == 0 || p.w == 0) { return j2p_fail(J2P_EINVAL, "job: channel %u: empty plane", c); }
                j2p_canvas_add(&all, p.w, p.h, p.w_samp, p.h_samp);
                j2p_canvas_add(&cv[where(d, c).solve], p.w, p.h, p.w_samp, p.h_samp);
        }
        const unsigned align = all.align;
        unsigned hmin = ~0u;
        size_t pixels_min = ~(size_t)0;
        for(unsigned k = 0; k < nsolve; k++) {
                if(cv[k].H < hmin) { hmin = cv[k].H; }
                if((size_t)cv[k].W * cv[k].H < pixels_min) { pixels_min = (size_t)cv[k].W * cv[k].H; }
        }
        unsigned nband = hmin / j2p_min_band_rows(align);
        if(tile_min_band_pixels(d) && pixels_min / tile_min_band_pixels(d) < nband) { nband = (unsigned)(pixels_min / tile_min_band_pixels(d)); }
        if(nband > devices.size()) { nband = (unsigned)devices.size(); }
        if(nband > 32) { nband = 32; }
        if(nband < 2) { return J2P_OK; }
        // near-equal bands of the shortest canvas in units of the alignment; the last band ends where each canvas ends
        unsigned cuts[33];
        (void)j2p_near_equal_cuts(hmin / align, nband, align, cuts);      // whole units (at least nband); the remainder goes to the last band
        Engines eng;
        for(unsigned k = 0; k < nsolve; k++) {
                cuts[nband] = cv[k].H;
                const int rc = j2p_tiled_create(&eng.e[k].t, nband, devices.data(), cuts, d.separate ? 1 : d.nchannel, &d.planes[k], d.weight[k],
                                                &d.pweight[k], d.iterations[k]);
                if((rc == J2P_EDEVICE || rc == J2P_ENOMEM) && !j2p_tiled_exchange_forced()) {
                        // these GPUs cannot be tiled over (no peer access and no RCCL, no exchange that verifies on them, or
                        // no room for the band arenas): the image is solved on one of them, as it would have been without
                        // `tile`.  Nothing has run yet.  (An exchange NAMED through J2P_TILED_EXCHANGE / J2P_TILED_WAIT that
                        // cannot be had is an error: the caller asked for that one.)
                        fprintf(stderr, "jpeg2png_amd: not row-tiling this image over %u GPUs (%s); solving it on one\n", nband, j2p_last_error());
                        return J2P_OK;
                }
                if(rc != J2P_OK) { return rc; }
        }
        *handled = true;
        return solve_and_deliver(j, eng.e, false);
}

// The engines of a job on one GPU, made from its input kind.  A file's scan is decoded ONCE, on this GPU, into pooled grids
// (j2p_decoded_grids: all components, whichever of them the job solves), from which every solver of the job copies its channels
// on the device; the grids go when the solvers exist.
int create_engines(const Job &j, int device, Engines &eng)
{
        const j2p_job &d = j.desc;
        const j2p_band whole = {0, 0};
        // estimated tables: the two steps of Solver.from_samples(quant="estimate"), a histogram launch per channel and the rule
        j2p_plane sampled[J2P_MAX_CHANNELS];
        uint16_t tables[J2P_MAX_CHANNELS][64];
        for(unsigned c = 0; j.in == In::samples && c < d.nchannel; c++) {
                sampled[c] = d.planes[c];
                if(!j.estimate) { continue; }
                std::vector<uint32_t> hist(64 * 1024);
                unsigned long long blocks = 0, excluded = 0;
                j2p_quant_estimate_result r;
                JOB_TRY(j2p_samples_histogram(device, nullptr, &j.samples[c], hist.data(), &blocks, &excluded));
                JOB_TRY(j2p_quant_estimate(reinterpret_cast<const uint32_t (*)[1024]>(hist.data()), c != 0, &r));
                memcpy(tables[c], r.table, sizeof(tables[c]));
                sampled[c].quant_table = tables[c];
                if(j.estimates) { j.estimates[c] = r; }
        }
        std::optional<j2p_decoded_grids> grids;
        if(j.in == In::file) {
                grids.emplace(device, j.file, 0u, nullptr);
                JOB_TRY(grids->rc);
        }
        for(unsigned k = 0; k < solves(d); k++) {
                const unsigned nch = d.separate ? 1 : d.nchannel;
                j2p_solver **s = &eng.e[k].s;
                switch(j.in) {
                case In::planes: JOB_TRY(j2p_solver_create(s, device, nullptr, nch, &d.planes[k], d.weight[k], &d.pweight[k], d.iterations[k], whole, 0)); break;
                case In::samples:
                        JOB_TRY(j2p_solver_create_from_samples(s, device, nullptr, nch, &sampled[k], &j.samples[k], d.weight[k], &d.pweight[k], d.iterations[k]));
                        break;
                case In::file:
                        JOB_TRY(j2p_solver_create_from_decoded(s, device, nch, &d.planes[k], &grids->coef[k], d.weight[k], &d.pweight[k], d.iterations[k]));
                        break;
                }
                if(oriented(j)) { JOB_TRY(j2p_solver_set_orientation(*s, j.orientation, j.orient_w, j.orient_h)); }
        }
        return J2P_OK;
}

int run_job(const Job &j, int device)
{
        Engines eng;
        JOB_TRY(create_engines(j, device, eng));
        return solve_and_deliver(j, eng.e, true);
}

void worker_main(j2p_batch *b, int device)
{
        (void)hipSetDevice(device);
        for(;;) {
                Job *job = nullptr;
                {
                        std::unique_lock<std::mutex> g(b->lock);
                        // the first queued job this worker may run: any job, except that a pinned one is for its GPU's workers
                        const auto mine = [&] {
                                auto it = b->queue.begin();
                                while(it != b->queue.end() && (*it)->device >= 0 && (*it)->device != device) { ++it; }
                                return it;
                        };
                        b->work.wait(g, [&] { return b->quit || mine() != b->queue.end(); });
                        const auto it = mine();
                        if(it == b->queue.end()) { return; }      // quit, and nothing left for this worker to do
                        job = *it;
                        b->queue.erase(it);
                }
                int rc = validate_job(job->desc);
                bool tiled = false;
                int single = device;
                if(rc == J2P_OK && job->desc.tile) {
                        // the job's share of the batch's devices, in the order given (a tiled job puts one band on each)
                        const size_t first = job->desc.tile_first, nall = b->devices.size();
                        const size_t count = job->desc.tile_count ? job->desc.tile_count : nall;
                        if(first >= nall || count > nall - first) { rc = j2p_fail(J2P_EINVAL, "job: tile devices [%zu, %zu) of %zu", first, first + count, nall); }
                        else {
                                const std::vector<int> share(b->devices.begin() + (ptrdiff_t)first, b->devices.begin() + (ptrdiff_t)(first + count));
                                if(job->desc.tile_count) { single = share[0]; }     // untiled after all: on a GPU of its share
                                if(share.size() > 1) { rc = run_job_tiled(*job, share, &tiled); }
                        }
                }
                if(rc == J2P_OK && !tiled) {
                        if(single != device) { (void)hipSetDevice(single); }
                        rc = run_job(*job, single);
                        if(single != device) { (void)hipSetDevice(device); }
                }
                {
                        std::lock_guard<std::mutex> g(b->lock);
                        job->rc = rc;
                        if(rc != J2P_OK) { strncpy(job->err, j2p_last_error(), sizeof(job->err) - 1); }
                        job->finished = true;
                }
                b->finished.notify_all();
        }
}

// ---- submit: the job and its request become the record, or are refused.  The first failing check decides the message, so the
// order below is part of the interface: file, JPEG, PNG, samples, outputs, resample, resize, then the pins. ----

// a file job: the marker segments are read here, on the caller's thread and before any device is asked for work — what they
// show is refused at submit (J2P_EFORMAT, J2P_ENOTSUP); the plane sizes the job left zero are filled in from the file (the
// image's: settle_orientation)
int open_file(const Request &q, Job &j)
{
        j2p_job &d = j.desc;
        if(d.tile) { return j2p_fail(J2P_EINVAL, "job: file input of a row-tiled job is not supported"); }
        JOB_TRY(q.file_scans ? j2p_jpeg_open_scans(q.file, q.file_size, &j.file) : j2p_jpeg_open(q.file, q.file_size, &j.file));
        const j2p_jpeg_info &info = j.file.info();
        if(d.nchannel == 0) { d.nchannel = info.ncomp; }
        // (one channel of a three-component file: component 0 alone, the greyscale solve)
        if(d.nchannel != info.ncomp && d.nchannel != 1) {
                return j2p_fail(J2P_EINVAL, "job: %u channels for a file of %u components (all of them, or 1 for component 0 alone)", d.nchannel, info.ncomp);
        }
        for(unsigned c = 0; c < d.nchannel; c++) {
                j2p_plane &p = d.planes[c];
                const j2p_jpeg_component &k = info.comp[c];
                if(p.data || p.fdata) { return j2p_fail(J2P_EINVAL, "job: channel %u: a job with a file takes no data / fdata (both must be NULL)", c); }
                if((p.w && p.w != k.blocks_w * 8) || (p.h && p.h != k.blocks_h * 8)) {
                        return j2p_fail(J2P_EINVAL, "job: channel %u: the plane is %ux%u, the file's component %ux%u", c, p.w, p.h, k.blocks_w * 8, k.blocks_h * 8);
                }
                p.w = k.blocks_w * 8;
                p.h = k.blocks_h * 8;
                // (sampling factors left zero are the file's; a caller who zooms gives the file's times the zoom)
                if(!p.w_samp) { p.w_samp = k.w_samp; }
                if(!p.h_samp) { p.h_samp = k.h_samp; }
                p.quant_table = k.quant;           // (the file's table: lives in the job's parse)
        }
        return J2P_OK;
}

// The orientation that arrived next to the job (Job::orientation), settled at submit: the tag read from the file's bytes (J2P_ORIENTATION_EXIF; of a file in device memory,
// from a copy of what precedes its scan), the source size a file job left zero taken from the file, and then the image size a
// file job left zero: the upright one.
int settle_orientation(const Request &q, Job &j)
{
        j2p_job &d = j.desc;
        if(j.orientation) {
                if(d.tile) { return j2p_fail(J2P_EINVAL, "job: upright output of a row-tiled job is not supported"); }
                if(j.orientation == J2P_ORIENTATION_EXIF) {
                        if(!q.file) { return j2p_fail(J2P_EINVAL, "job: J2P_ORIENTATION_EXIF needs a job with a file"); }
                        if(j.file.on_device) {
                                std::vector<uint8_t> head(j.file.info().scan_begin < q.file_size ? j.file.info().scan_begin : q.file_size);
                                if(hipMemcpy(head.data(), q.file, head.size(), hipMemcpyDeviceToHost) != hipSuccess) {
                                        return j2p_fail(J2P_EDEVICE, "job: the file's head could not be copied from device memory");
                                }
                                JOB_TRY(j2p_jpeg_orientation(head.data(), head.size(), &j.orientation));
                        } else {
                                JOB_TRY(j2p_jpeg_orientation(q.file, q.file_size, &j.orientation));
                        }
                }
                if(j.orientation > 8) { return j2p_fail(J2P_EINVAL, "job: orientation %u (0: none, 1..8, J2P_ORIENTATION_EXIF)", j.orientation); }
                if(q.file) {
                        if(!j.orient_w) { j.orient_w = j.file.info().width; }
                        if(!j.orient_h) { j.orient_h = j.file.info().height; }
                }
                if(j.orient_w == 0 || j.orient_h == 0) { return j2p_fail(J2P_EINVAL, "job: an orientation needs the source image's size (orient_w, orient_h)"); }
        }
        if(q.file) {
                const j2p_jpeg_info &info = j.file.info();
                const bool transposed = j.orientation >= 5;
                if(!d.out_w) { d.out_w = j.orientation > 1 ? (transposed ? j.orient_h : j.orient_w) : info.width; }
                if(!d.out_h) { d.out_h = j.orientation > 1 ? (transposed ? j.orient_w : j.orient_h) : info.height; }
        }
        return J2P_OK;
}

int validate_jpeg(const j2p_job &d, const Request &q)
{
        if(d.out_bits || d.out_coef[0] || d.out_tensor.data) {
                return j2p_fail(J2P_EINVAL, "job: a JPEG job needs out_bits 0, no out_coef and out_tensor.data NULL");
        }
        if(d.tile) { return j2p_fail(J2P_EINVAL, "job: JPEG output of a row-tiled job is not supported"); }
        if(const char *why = j2p_jpeg_error(q.jpeg, d.nchannel)) { return j2p_fail(J2P_EINVAL, "job: %s", why); }
        if(const char *why = j2p_jpeg_options_error(&q.jpeg_options)) { return j2p_fail(J2P_EINVAL, "job: %s", why); }
        if(q.jpeg->width != d.out_w || q.jpeg->height != d.out_h) {
                return j2p_fail(J2P_EINVAL, "job: the JPEG is %ux%u, the job's image (out_w x out_h) %ux%u", q.jpeg->width, q.jpeg->height, d.out_w, d.out_h);
        }
        if(!q.jpeg_size || (!q.jpeg_out && q.jpeg_capacity)) { return j2p_fail(J2P_EINVAL, "job: JPEG output needs out and size"); }
        return J2P_OK;
}

int validate_png(const j2p_job &d, const Request &q)
{
        if(d.out_bits || d.out_coef[0] || d.out_tensor.data) {
                return j2p_fail(J2P_EINVAL, "job: a PNG job needs out_bits 0, no out_coef and out_tensor.data NULL");
        }
        if(d.tile) { return j2p_fail(J2P_EINVAL, "job: PNG output of a row-tiled job is not supported"); }
        if(const char *why = j2p_png_error(q.png, d.nchannel)) { return j2p_fail(J2P_EINVAL, "job: %s", why); }
        if(q.png->width != d.out_w || q.png->height != d.out_h) {
                return j2p_fail(J2P_EINVAL, "job: the PNG is %ux%u, the job's image (out_w x out_h) %ux%u", q.png->width, q.png->height, d.out_w, d.out_h);
        }
        if(!q.png_size || (!q.png_out && q.png_capacity)) { return j2p_fail(J2P_EINVAL, "job: PNG output needs out and size"); }
        return J2P_OK;
}

// *device: the GPU that holds the device samples, or -1 (host samples only)
int validate_samples(const j2p_job &d, const j2p_samples *samples, int *device)
{
        if(d.nchannel == 0 || d.nchannel > J2P_MAX_CHANNELS) { return j2p_fail(J2P_EINVAL, "job: nchannel must be 1..3"); }
        if(d.tile) { return j2p_fail(J2P_EINVAL, "job: sample input of a row-tiled job is not supported"); }
        *device = -1;
        for(unsigned c = 0; c < d.nchannel; c++) {
                const j2p_plane &p = d.planes[c];
                const j2p_samples &m = samples[c];
                if(p.data || p.fdata) { return j2p_fail(J2P_EINVAL, "job: channel %u: a job with samples takes no data / fdata (both must be NULL)", c); }
                if(!m.data) { return j2p_fail(J2P_EINVAL, "job: channel %u: samples: data is NULL", c); }
                if(m.w == 0 || m.h == 0 || m.w > p.w || m.h > p.h) {
                        return j2p_fail(J2P_EINVAL, "job: channel %u: samples: %ux%u samples for a coefficient plane of %ux%u", c, m.w, m.h, p.w, p.h);
                }
                if(m.stride_y < 1 || m.stride_x < 1) { return j2p_fail(J2P_EINVAL, "job: channel %u: samples: strides must be at least 1", c); }
                int dev = -1;
                const int kind = j2p_memory_of_pointer(m.data, &dev);
                if(kind == J2P_MEMORY_OTHER) { return j2p_fail(J2P_EINVAL, "job: channel %u: samples: data is neither host nor plain device memory (managed memory is refused)", c); }
                if(kind == J2P_MEMORY_DEVICE) {
                        if(*device >= 0 && dev != *device) { return j2p_fail(J2P_EINVAL, "job: channel %u: samples live on device %d, others on device %d", c, dev, *device); }
                        *device = dev;
                }
        }
        return J2P_OK;
}

// *device: the one GPU that holds every tensor
int validate_outputs(const j2p_job &d, unsigned n, const j2p_output *outs, int *device)
{
        if(n > J2P_MAX_OUTPUTS) { return j2p_fail(J2P_EINVAL, "job: %u outputs (at most %d)", n, J2P_MAX_OUTPUTS); }
        if(d.out_tensor.data || d.out_bits || d.out_coef[0]) {
                return j2p_fail(J2P_EINVAL, "job: a job with outputs needs out_tensor.data NULL, out_bits 0 and no out_coef");
        }
        JOB_TRY(validate_tensor_form(d));
        for(unsigned i = 0; i < n; i++) {
                if(const char *why = j2p_resample_error(&outs[i].r, d.out_w, d.out_h)) { return j2p_fail(J2P_EINVAL, "job: output %u: %s", i, why); }
                int dev = -1;
                if(j2p_device_of_pointer(outs[i].t.data, &dev) != J2P_OK) {
                        return j2p_fail(J2P_EINVAL, "job: output %u: the tensor's data is not device memory (managed and host memory are refused)", i);
                }
                if(i && dev != *device) { return j2p_fail(J2P_EINVAL, "job: output %u lives on device %d, output 0 on device %d", i, dev, *device); }
                *device = dev;
        }
        return J2P_OK;
}

// The job runs on `device` only, where its tensor(s), device samples or file are (what: "the tensor lives", ...): that must be one of
// the batch's GPUs, and the one an earlier pin chose.
int pin(const j2p_batch &b, Job &j, int device, const char *what)
{
        if(j.device >= 0 && j.device != device) { return j2p_fail(J2P_EINVAL, "job: %s on device %d, the output tensor on device %d", what, device, j.device); }
        bool owned = false;
        for(int dev : b.devices) { owned = owned || dev == device; }
        if(!owned) { return j2p_fail(J2P_EINVAL, "job: %s on device %d, which this batch does not drive", what, device); }
        j.device = device;
        return J2P_OK;
}

// j = the record of `given` and what its entry point sent along: the input kind and the output kind with their payloads, and the pin
int classify(const j2p_batch &b, const j2p_job &given, const Request &q, Job &j)
{
        j.desc = given;
        j.orientation = q.orientation, j.orient_w = q.orient_w, j.orient_h = q.orient_h;
        const j2p_job &d = j.desc;
        int samples_device = -1, tensor_device = -1;
        if(q.file) {
                j.in = In::file;
                JOB_TRY(open_file(q, j));
        }
        JOB_TRY(settle_orientation(q, j));
        if(q.jpeg) {
                j.out = Out::jpeg;
                JOB_TRY(validate_jpeg(d, q));
                j.jpeg.set(q, d.nchannel);
        }
        if(q.png) {
                j.out = Out::png;
                JOB_TRY(validate_png(d, q));
                j.png.spec = *q.png;
                j.png.out = q.png_out, j.png.capacity = q.png_capacity, j.png.size = q.png_size;
        }
        if(q.estimate && !q.samples) { return j2p_fail(J2P_EINVAL, "job: estimated tables need samples"); }
        if(q.samples) {
                j.in = In::samples;
                JOB_TRY(validate_samples(d, q.samples, &samples_device));
                j.samples.assign(q.samples, q.samples + d.nchannel);
        }
        if(q.estimate) {
                // no table at all, or one in every plane (ignored): a job with some cannot mean either
                unsigned have = 0;
                for(unsigned c = 0; c < d.nchannel; c++) { have += d.planes[c].quant_table ? 1u : 0u; }
                if(have && have != d.nchannel) { return j2p_fail(J2P_EINVAL, "job: estimated tables, but %u of %u planes carry a quant_table", have, d.nchannel); }
                j.estimate = true;
                j.estimates = q.estimates;
        }
        if(q.nout) {
                j.out = Out::outputs;
                JOB_TRY(validate_outputs(d, q.nout, q.outs, &tensor_device));
                j.outputs.assign(q.outs, q.outs + q.nout);
        }
        if(q.resample) {
                j.out = Out::resampled;
                if(!d.out_tensor.data) { return j2p_fail(J2P_EINVAL, "job: a resampled job needs tensor output (out_tensor)"); }
                if(const char *why = j2p_resample_error(q.resample, d.out_w, d.out_h)) { return j2p_fail(J2P_EINVAL, "job: %s", why); }
                j.resample = *q.resample;
        }
        if(q.resize) {
                j.out = Out::resized;
                if(!d.out_tensor.data) { return j2p_fail(J2P_EINVAL, "job: a resized job needs tensor output (out_tensor)"); }
                if(const char *why = j2p_resize_error(q.resize, d.out_w, d.out_h)) { return j2p_fail(J2P_EINVAL, "job: %s", why); }
                j.resize = *q.resize;
        }
        if(d.out_tensor.data || j.out == Out::outputs) {
                // a job with tensors: what can be refused is refused here, and the job is pinned to the GPU that holds them
                JOB_TRY(validate_job(d));
                if(j.out != Out::outputs && j2p_device_of_pointer(d.out_tensor.data, &tensor_device) != J2P_OK) {
                        return j2p_fail(J2P_EINVAL, "job: out_tensor.data is not device memory (managed and host memory are refused)");
                }
                JOB_TRY(pin(b, j, tensor_device, "the tensor lives"));
        }
        // device samples, and a file in device memory, pin the job as tensors do
        if(samples_device >= 0) { JOB_TRY(pin(b, j, samples_device, "the samples live")); }
        if(j.file.device >= 0) { JOB_TRY(pin(b, j, j.file.device, "the file lives")); }
        return J2P_OK;
}

// what j2p_batch_next_orientation left for the calling thread's next submit
thread_local struct {
        const j2p_batch *batch = nullptr;
        unsigned orientation = 0, orient_w = 0, orient_h = 0;
} next_orientation;
// what j2p_batch_next_file_scans left for it
thread_local struct {
        const j2p_batch *batch = nullptr;
} next_file_scans;

int submit(j2p_batch *b, const j2p_job *job, const Request &entry, int *ticket)
{
        // (consumed by this submit, whatever becomes of it)
        Request q = entry;
        if(next_orientation.batch && next_orientation.batch == b) {
                q.orientation = next_orientation.orientation, q.orient_w = next_orientation.orient_w, q.orient_h = next_orientation.orient_h;
        }
        next_orientation.batch = nullptr;
        q.file_scans = next_file_scans.batch && next_file_scans.batch == b;
        next_file_scans.batch = nullptr;
        if(!b || !job || !ticket) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        std::unique_ptr<Job> j(new(std::nothrow) Job());
        if(!j) { return j2p_fail(J2P_ENOMEM, "host allocation failed"); }
        JOB_TRY(classify(*b, *job, q, *j));
        const bool pinned = j->device >= 0;
        {
                std::lock_guard<std::mutex> g(b->lock);
                if(b->quit) { return j2p_fail(J2P_ESTATE, "batch is shutting down"); }
                *ticket = j->ticket = b->next_ticket++;
                b->jobs[j->ticket] = j.get();
                b->queue.push_back(j.release());
        }
        // (a pinned job may not be for the worker notify_one would wake)
        if(pinned) { b->work.notify_all(); } else { b->work.notify_one(); }
        return J2P_OK;
}

}  // namespace

extern "C" {

int j2p_batch_create(j2p_batch **out, unsigned ndev, const int devices[], unsigned slots_per_device)
{
        if(!out || !devices) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        *out = nullptr;
        if(ndev == 0 || ndev > 64 || slots_per_device == 0 || slots_per_device > 16) {
                return j2p_fail(J2P_EINVAL, "batch: 1..64 devices, 1..16 slots per device");
        }
        int have = 0;
        if(hipGetDeviceCount(&have) != hipSuccess || have <= 0) {
                return j2p_fail(J2P_EDEVICE, "no HIP device available: the jpeg2png_amd solver has no CPU fallback");
        }
        for(unsigned i = 0; i < ndev; i++) {
                if(devices[i] < 0 || devices[i] >= have) { return j2p_fail(J2P_EINVAL, "device %d out of range (0..%d)", devices[i], have - 1); }
        }
        j2p_batch *b = new(std::nothrow) j2p_batch();
        if(!b) { return j2p_fail(J2P_ENOMEM, "host allocation failed"); }
        b->devices.assign(devices, devices + ndev);
        // slot-major order: the first ndev workers sit on different GPUs, so few images spread out first
        for(unsigned k = 0; k < slots_per_device; k++) {
                for(unsigned i = 0; i < ndev; i++) { b->worker_device.push_back(devices[i]); }
        }
        for(int dev : b->worker_device) { b->workers.emplace_back(worker_main, b, dev); }
        *out = b;
        return J2P_OK;
}

void j2p_batch_destroy(j2p_batch *b)
{
        if(!b) { return; }
        {
                std::lock_guard<std::mutex> g(b->lock);
                b->quit = true;
        }
        b->work.notify_all();
        for(std::thread &t : b->workers) { t.join(); }          // queued jobs are finished first
        for(auto &kv : b->jobs) { delete kv.second; }
        delete b;
        j2p_pool_trim();        // the arenas the images recycled go back to the device with the batch
}

int j2p_batch_submit(j2p_batch *b, const j2p_job *job, int *ticket)
{
        return submit(b, job, Request(), ticket);
}

int j2p_batch_submit_resized(j2p_batch *b, const j2p_job *job, const j2p_resize *r, int *ticket)
{
        return submit(b, job, Request().resized(r), ticket);
}

int j2p_batch_submit_resampled(j2p_batch *b, const j2p_job *job, const j2p_resample *r, int *ticket)
{
        return submit(b, job, Request().resampled(r), ticket);
}

int j2p_batch_submit_outputs(j2p_batch *b, const j2p_job *job, unsigned n, const j2p_output outs[], int *ticket)
{
        return submit(b, job, Request().outputs(n, outs), ticket);
}

int j2p_batch_submit_samples(j2p_batch *b, const j2p_job *job, const j2p_samples samples[], unsigned n, const j2p_output outs[], int *ticket)
{
        return submit(b, job, Request().from_samples(samples).outputs(n, outs), ticket);
}

int j2p_batch_submit_samples_estimated(j2p_batch *b, const j2p_job *job, const j2p_samples samples[], unsigned n, const j2p_output outs[],
                                       j2p_quant_estimate_result estimates[], int *ticket)
{
        return submit(b, job, Request().from_samples(samples).outputs(n, outs).estimated(estimates), ticket);
}

// A JPEG job from samples (or, with none, from the job's coefficients), and one from a file: the record says which file is
// written, and the older entry points are these two with their records.
int j2p_batch_submit_jpeg_opt(j2p_batch *b, const j2p_job *job, const j2p_samples samples[], const j2p_jpeg *spec, uint8_t *out, size_t capacity,
                              size_t *size, const j2p_jpeg_options *options, int *ticket)
{
        if(!spec) { return j2p_fail(J2P_EINVAL, "job: jpeg: spec is NULL"); }
        if(!options) { return j2p_fail(J2P_EINVAL, "job: jpeg: options is NULL"); }
        return submit(b, job, Request().from_samples(samples).jpeg_to(spec, out, capacity, size, *options), ticket);
}

int j2p_batch_submit_file_jpeg_opt(j2p_batch *b, const j2p_job *job, const uint8_t *file, size_t size, const j2p_jpeg *spec, uint8_t *out,
                                   size_t capacity, size_t *out_size, const j2p_jpeg_options *options, int *ticket)
{
        if(!file || size == 0) { return j2p_fail(J2P_EINVAL, "job: file is NULL or empty"); }
        if(!spec) { return j2p_fail(J2P_EINVAL, "job: jpeg: spec is NULL"); }
        if(!options) { return j2p_fail(J2P_EINVAL, "job: jpeg: options is NULL"); }
        return submit(b, job, Request().from_file(file, size).jpeg_to(spec, out, capacity, out_size, *options), ticket);
}

int j2p_batch_submit_jpeg_ex(j2p_batch *b, const j2p_job *job, const j2p_samples samples[], const j2p_jpeg *spec, uint8_t *out, size_t capacity,
                             size_t *size, unsigned flags, int *ticket)
{
        const j2p_jpeg_options options = {flags, 0, 0, 0};
        return j2p_batch_submit_jpeg_opt(b, job, samples, spec, out, capacity, size, &options, ticket);
}

int j2p_batch_submit_jpeg_progressive(j2p_batch *b, const j2p_job *job, const j2p_samples samples[], const j2p_jpeg *spec, uint8_t *out,
                                      size_t capacity, size_t *size, int *ticket)
{
        const j2p_jpeg_options options = {0, 1, 0, 0};
        return j2p_batch_submit_jpeg_opt(b, job, samples, spec, out, capacity, size, &options, ticket);
}

int j2p_batch_submit_jpeg(j2p_batch *b, const j2p_job *job, const j2p_samples samples[], const j2p_jpeg *spec, uint8_t *out, size_t capacity,
                          size_t *size, int *ticket)
{
        const j2p_jpeg_options options = {0, 0, 0, 0};
        return j2p_batch_submit_jpeg_opt(b, job, samples, spec, out, capacity, size, &options, ticket);
}

int j2p_batch_submit_file_jpeg_ex(j2p_batch *b, const j2p_job *job, const uint8_t *file, size_t size, const j2p_jpeg *spec, uint8_t *out,
                                  size_t capacity, size_t *out_size, unsigned flags, int *ticket)
{
        const j2p_jpeg_options options = {flags, 0, 0, 0};
        return j2p_batch_submit_file_jpeg_opt(b, job, file, size, spec, out, capacity, out_size, &options, ticket);
}

int j2p_batch_submit_file_jpeg_progressive(j2p_batch *b, const j2p_job *job, const uint8_t *file, size_t size, const j2p_jpeg *spec, uint8_t *out,
                                           size_t capacity, size_t *out_size, int *ticket)
{
        const j2p_jpeg_options options = {0, 1, 0, 0};
        return j2p_batch_submit_file_jpeg_opt(b, job, file, size, spec, out, capacity, out_size, &options, ticket);
}

int j2p_batch_submit_file_jpeg(j2p_batch *b, const j2p_job *job, const uint8_t *file, size_t size, const j2p_jpeg *spec, uint8_t *out,
                               size_t capacity, size_t *out_size, int *ticket)
{
        const j2p_jpeg_options options = {0, 0, 0, 0};
        return j2p_batch_submit_file_jpeg_opt(b, job, file, size, spec, out, capacity, out_size, &options, ticket);
}

int j2p_batch_submit_file(j2p_batch *b, const j2p_job *job, const uint8_t *file, size_t size, unsigned n, const j2p_output outs[], int *ticket)
{
        if(!file || size == 0) { return j2p_fail(J2P_EINVAL, "job: file is NULL or empty"); }
        return submit(b, job, Request().from_file(file, size).outputs(n, outs), ticket);
}

int j2p_batch_submit_png(j2p_batch *b, const j2p_job *job, const j2p_samples samples[], const j2p_png *spec, uint8_t *out, size_t capacity, size_t *size,
                         int *ticket)
{
        if(!spec) { return j2p_fail(J2P_EINVAL, "job: png: spec is NULL"); }
        return submit(b, job, Request().from_samples(samples).png_to(spec, out, capacity, size), ticket);
}

int j2p_batch_submit_file_png(j2p_batch *b, const j2p_job *job, const uint8_t *file, size_t size, const j2p_png *spec, uint8_t *out, size_t capacity,
                              size_t *out_size, int *ticket)
{
        if(!file || size == 0) { return j2p_fail(J2P_EINVAL, "job: file is NULL or empty"); }
        if(!spec) { return j2p_fail(J2P_EINVAL, "job: png: spec is NULL"); }
        return submit(b, job, Request().from_file(file, size).png_to(spec, out, capacity, out_size), ticket);
}

void j2p_debug_job_layout(size_t *size, size_t *out_tensor_offset)
{
        if(size) { *size = sizeof(j2p_job); }
        if(out_tensor_offset) { *out_tensor_offset = offsetof(j2p_job, out_tensor); }
}

int j2p_batch_next_orientation(j2p_batch *b, unsigned orientation, unsigned orient_w, unsigned orient_h)
{
        if(!b) { return j2p_fail(J2P_EINVAL, "batch is NULL"); }
        next_orientation.batch = orientation ? b : nullptr;
        next_orientation.orientation = orientation;
        next_orientation.orient_w = orient_w;
        next_orientation.orient_h = orient_h;
        return J2P_OK;
}

int j2p_batch_next_file_scans(j2p_batch *b, unsigned accept)
{
        if(!b) { return j2p_fail(J2P_EINVAL, "batch is NULL"); }
        next_file_scans.batch = accept ? b : nullptr;
        return J2P_OK;
}

int j2p_batch_wait(j2p_batch *b, int ticket)
{
        if(!b) { return j2p_fail(J2P_EINVAL, "batch is NULL"); }
        Job *j = nullptr;
        {
                std::unique_lock<std::mutex> g(b->lock);
                auto it = b->jobs.find(ticket);
                if(it == b->jobs.end()) { return j2p_fail(J2P_EINVAL, "unknown ticket %d", ticket); }
                j = it->second;
                b->finished.wait(g, [&] { return j->finished; });
                b->jobs.erase(it);
        }
        const int rc = j->rc;
        if(rc != J2P_OK) { j2p_fail(rc, "%s", j->err); }
        delete j;
        return rc;
}

}  // extern "C"
