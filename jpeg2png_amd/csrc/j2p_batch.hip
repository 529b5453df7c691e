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
#include <thread>
#include <vector>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jpeg2png_amd.h"
#include "j2p_internal.h"
#include "j2p_geometry.h"

namespace {

// where the file of a j2p_batch_submit_jpeg job goes; spec.quant[] point into tables[]
struct JpegOut {
        bool on = false;
        j2p_jpeg spec = {0, 0, 0, 0, {nullptr, nullptr, nullptr}};
        uint16_t tables[3][64];
        uint8_t *out = nullptr;
        size_t capacity = 0, *size = nullptr;
};

struct Job {
        j2p_job desc;
        j2p_resize resize = {0, 0, 0, 0, 0, 0};   // j2p_batch_submit_resized: the tensor receives the image resized
        bool resized = false;
        j2p_resample resample = {0, 0, 0, 0, 0, 0, 0};   // j2p_batch_submit_resampled: ... resampled with a filter
        bool resampled = false;
        std::vector<j2p_output> outputs;    // j2p_batch_submit_outputs: these tensors are filled from the one solve, not out_tensor
        std::vector<j2p_samples> samples;   // j2p_batch_submit_samples: [channel] the solvers are made from these, not from planes[].data
        JpegOut jpeg;                       // j2p_batch_submit_jpeg: the job delivers the file
        j2p_jpeg_file file;                 // j2p_batch_submit_file: opened at submit; the worker decodes the solvers' coefficients from
                                            // the caller's bytes, which stay valid until j2p_batch_wait
        int ticket = 0;
        int device = -1;                    // tensor output, device samples: their device, the only one whose workers may take the job
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
        std::deque<Job *> queue;
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

// what both paths of a job check before they touch anything
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
                if(d.nchannel == 2) { return j2p_fail(J2P_EINVAL, "job: tensor output needs three channels (RGB) or one (greyscale)"); }
                if(d.out_w == 0 || d.out_h == 0) { return j2p_fail(J2P_EINVAL, "job: tensor output needs out_w and out_h"); }
                if(d.tile) { return j2p_fail(J2P_EINVAL, "job: tensor output of a row-tiled job is not supported"); }
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

// What a job does once its engines exist: the iterations (compute.c:427-453), then the samples, coefficients or planes.
// Chunked when the caller watches (j2p_next_chunk), so that its bar and CSV keep moving.  `overlap`: the chunk of every
// solve is issued before any of them is settled (sync, progress, done) — how the three solves of `-s` overlap on one GPU,
// unless log rows make every run synchronous anyway.  Row-tiled jobs settle each solve right after issuing it.
// resize / resample (tensor jobs on one GPU only, at most one of the two): the tensor receives the image resized.
// outputs (never empty when given; a job on one GPU without out_tensor): those tensors are filled from the solve.
// jpeg (a job on one GPU with no other output but out_planes): the file is made from the solve.
int solve_and_deliver(const j2p_job &d, const Engine *e, bool overlap, const j2p_resize *resize, const j2p_resample *resample,
                      const std::vector<j2p_output> *outputs, const JpegOut *jpeg)
{
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
        // Every band delivers its own rows from its own GPU.  The solves of a job share their cuts (multiples of 16 rows: of a
        // block row of either sampling) and differ only in where the last band ends; the last band takes all that the output
        // has left — the block row that overhangs the canvas too — and the rows forms refuse what is not there.
        const unsigned nband = e[0].nband();
        for(unsigned b = 0; b < nband; b++) {
                j2p_plane_ref ref[J2P_MAX_CHANNELS];
                unsigned row0[J2P_MAX_CHANNELS], row1[J2P_MAX_CHANNELS];
                for(unsigned c = 0; c < d.nchannel; c++) {
                        const Where at = where(d, c);
                        ref[c].channel = at.channel;
                        JOB_TRY(e[at.solve].band(b, &ref[c].solver, &row0[c], &row1[c]));
                }
                if(outputs) {
                        // (never row-tiled: this one band is the whole canvas)
                        JOB_TRY(j2p_planes_to_tensors_resampled(ref, d.nchannel, d.out_w, d.out_h, (unsigned)outputs->size(), outputs->data()));
                        JOB_TRY(j2p_solver_sync(ref[0].solver));         // the ticket says: every tensor complete, for any stream
                        continue;
                }
                if(jpeg) {
                        // (never row-tiled: this one band is the whole canvas)
                        JOB_TRY(j2p_planes_to_jpeg(ref, d.nchannel, &jpeg->spec, jpeg->out, jpeg->capacity, jpeg->size));
                        continue;
                }
                if(d.out_bits || d.out_tensor.data) {
                        const unsigned y0 = row0[0], y1 = b + 1 < nband && row1[0] < d.out_h ? row1[0] : d.out_h;   // the band's image rows
                        if(y0 >= y1) { continue; }                       // band below the image (canvas padding only)
                        if(d.out_bits) {
                                const size_t row_bytes = (size_t)d.out_w * (d.nchannel == 1 ? 1 : 3) * (d.out_bits / 8);
                                uint8_t *out = d.out_rgb + (size_t)y0 * row_bytes;
                                if(d.nchannel == 1) { JOB_TRY(j2p_planes_rows_to_grey(ref, d.out_w, y0, y1, d.out_bits, out)); }   // greyscale: one sample per pixel
                                else { JOB_TRY(j2p_planes_rows_to_rgb(ref, d.out_w, y0, y1, d.out_bits, out)); }
                                continue;
                        }
                        if(resize) {
                                // (never row-tiled: this one band is the whole canvas)
                                JOB_TRY(j2p_planes_to_tensor_resized(ref, d.nchannel, d.out_w, d.out_h, resize, &d.out_tensor));
                                JOB_TRY(j2p_solver_sync(ref[0].solver));
                                continue;
                        }
                        if(resample) {
                                JOB_TRY(j2p_planes_to_tensor_resampled(ref, d.nchannel, d.out_w, d.out_h, resample, &d.out_tensor));
                                JOB_TRY(j2p_solver_sync(ref[0].solver));
                                continue;
                        }
                        j2p_tensor rows = d.out_tensor;                  // the band's first row of it
                        const size_t row_bytes = (size_t)(d.out_tensor.stride_y > 0 ? d.out_tensor.stride_y : 0) * j2p_tensor_element_bytes(d.out_tensor.dtype);
                        rows.data = static_cast<char *>(d.out_tensor.data) + (size_t)y0 * row_bytes;
                        JOB_TRY(j2p_planes_rows_to_tensor(ref, d.nchannel, d.out_w, y0, y1, &rows));
                        JOB_TRY(j2p_solver_sync(ref[0].solver));         // the ticket says: complete, for any stream
                        continue;
                }
                for(unsigned c = 0; d.out_coef[0] && c < d.nchannel; c++) {
                        const unsigned sx = out_sub(d.out_sub_w[c]), sy = out_sub(d.out_sub_h[c]);
                        const unsigned bw = (d.out_blocks_w + sx - 1) / sx, bh = (d.out_blocks_h + sy - 1) / sy;
                        const unsigned r0 = row0[c] / (8 * sy), r1 = b + 1 < nband && row1[c] / (8 * sy) < bh ? row1[c] / (8 * sy) : bh;
                        if(r0 >= r1) { continue; }                       // band below the image (canvas padding only)
                        JOB_TRY(j2p_planes_rows_to_coefficients_sub(&ref[c], sx, sy, bw, r0, r1, d.out_quant[c], d.out_coef[c] + (size_t)r0 * bw * 64));
                }
        }
        for(unsigned c = 0; !d.out_bits && c < d.nchannel; c++) {
                if(d.out_planes[c]) { JOB_TRY(e[where(d, c).solve].download(where(d, c).channel, d.out_planes[c])); }
        }
        return J2P_OK;
}

// One image over several of the batch's devices (j2p_job::tile): every solve of the job becomes a j2p_tiled with band
// b on devices[b]; the solves of `-s` share their cuts so that band b of the three components meets on one GPU for
// the colour conversion.  Returns J2P_OK with *handled = false when the image should be solved on one GPU after all:
// too small for two bands (rows, or pixels per band), or the devices cannot be tiled over (the create phase failed:
// no peer access and no RCCL, or no room for the band arenas) — the caller then takes the single-solver path.
// Failures after the iterations have started stay failures.
int run_job_tiled(const j2p_job &d, const std::vector<int> &devices, bool *handled)
{
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
        return solve_and_deliver(d, eng.e, false, nullptr, nullptr, nullptr, nullptr);
}

// a file job's engines: the file's scan decoded ONCE on the worker's GPU into pooled grids (j2p_decoded_grids: all components,
// whichever of them the job solves), from which every solver of the job copies its channels on the device
int create_from_file(const j2p_job &d, int device, const j2p_jpeg_file &file, Engines &eng)
{
        const j2p_decoded_grids grids(device, file, 0, nullptr);
        int rc = grids.rc;
        for(unsigned k = 0; rc == J2P_OK && k < solves(d); k++) {
                const unsigned nch = d.separate ? 1 : d.nchannel;
                rc = j2p_solver_create_from_decoded(&eng.e[k].s, device, nch, &d.planes[k], &grids.coef[k], d.weight[k], &d.pweight[k], d.iterations[k]);
        }
        return rc;
}

// (samples: NULL, or [channel] what the solvers are made from instead of planes[].data; file: NULL, or the file they are made from)
int run_job(const j2p_job &d, int device, const j2p_resize *resize, const j2p_resample *resample, const std::vector<j2p_output> *outputs,
            const j2p_samples *samples, const JpegOut *jpeg, const j2p_jpeg_file *file)
{
        const j2p_band whole = {0, 0};
        Engines eng;
        if(file) {
                JOB_TRY(create_from_file(d, device, *file, eng));
                return solve_and_deliver(d, eng.e, true, resize, resample, outputs, jpeg);
        }
        for(unsigned k = 0; k < solves(d); k++) {
                const unsigned nch = d.separate ? 1 : d.nchannel;
                if(samples) {
                        JOB_TRY(j2p_solver_create_from_samples(&eng.e[k].s, device, nullptr, nch, &d.planes[k], &samples[k], d.weight[k], &d.pweight[k],
                                                               d.iterations[k]));
                        continue;
                }
                JOB_TRY(j2p_solver_create(&eng.e[k].s, device, nullptr, nch, &d.planes[k], d.weight[k], &d.pweight[k], d.iterations[k], whole, 0));
        }
        return solve_and_deliver(d, eng.e, true, resize, resample, outputs, jpeg);
}

void worker_main(j2p_batch *b, int device)
{
        (void)hipSetDevice(device);
        for(;;) {
                Job *job = nullptr;
                {
                        std::unique_lock<std::mutex> g(b->lock);
                        // the first queued job this worker may run: any job, except that one with a tensor is pinned to its GPU
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
                                if(share.size() > 1) { rc = run_job_tiled(job->desc, share, &tiled); }
                        }
                }
                if(rc == J2P_OK && !tiled) {
                        if(single != device) { (void)hipSetDevice(single); }
                        rc = run_job(job->desc, single, job->resized ? &job->resize : nullptr, job->resampled ? &job->resample : nullptr,
                                     job->outputs.empty() ? nullptr : &job->outputs, job->samples.empty() ? nullptr : job->samples.data(),
                                     job->jpeg.on ? &job->jpeg : nullptr, job->file.parsed ? &job->file : nullptr);
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

// what j2p_batch_submit_outputs refuses at submit; *device: the one GPU that holds every tensor
int validate_outputs(const j2p_job &d, unsigned n, const j2p_output *outs, int *device)
{
        if(n > J2P_MAX_OUTPUTS) { return j2p_fail(J2P_EINVAL, "job: %u outputs (at most %d)", n, J2P_MAX_OUTPUTS); }
        if(d.out_tensor.data || d.out_bits || d.out_coef[0]) {
                return j2p_fail(J2P_EINVAL, "job: a job with outputs needs out_tensor.data NULL, out_bits 0 and no out_coef");
        }
        if(d.nchannel != 1 && d.nchannel != 3) { return j2p_fail(J2P_EINVAL, "job: tensor output needs three channels (RGB) or one (greyscale)"); }
        if(d.out_w == 0 || d.out_h == 0) { return j2p_fail(J2P_EINVAL, "job: tensor output needs out_w and out_h"); }
        if(d.tile) { return j2p_fail(J2P_EINVAL, "job: tensor output of a row-tiled job is not supported"); }
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

// what j2p_batch_submit_samples refuses at submit; *device: the GPU that holds the device samples, or -1 (host samples only)
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

// j2p_batch_submit, and — r != NULL — j2p_batch_submit_resized, — f != NULL — j2p_batch_submit_resampled, — nout != 0 —
// j2p_batch_submit_outputs (never two of them); samples != NULL: j2p_batch_submit_samples (with nout or without; never with r or f);
// jpeg != NULL: j2p_batch_submit_jpeg (with samples or without, and nothing else); file != NULL: j2p_batch_submit_file and
// j2p_batch_submit_file_jpeg (never with samples; with nout or with jpeg)
int submit(j2p_batch *b, const j2p_job *job, const j2p_resize *r, const j2p_resample *f, unsigned nout, const j2p_output *outs,
           const j2p_samples *samples, const JpegOut *jpeg, int *ticket, const uint8_t *file = nullptr, size_t file_size = 0)
{
        if(!b || !job || !ticket) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        // a file job: the marker segments are read here, on the caller's thread and before any device is asked for work — what they
        // show is refused at submit (J2P_EFORMAT, J2P_ENOTSUP); the sizes the job left zero are filled in from the file
        j2p_jpeg_file file_in;
        j2p_job filled;
        int file_device = -1;
        if(file) {
                if(job->tile) { return j2p_fail(J2P_EINVAL, "job: file input of a row-tiled job is not supported"); }
                if(const int rc = j2p_jpeg_open(file, file_size, &file_in); rc != J2P_OK) { return rc; }
                file_device = file_in.device;
                const j2p_jpeg_info &info = file_in.parsed->info;
                filled = *job;
                if(filled.nchannel == 0) { filled.nchannel = info.ncomp; }
                // (one channel of a three-component file: component 0 alone, the greyscale solve)
                if(filled.nchannel != info.ncomp && filled.nchannel != 1) {
                        return j2p_fail(J2P_EINVAL, "job: %u channels for a file of %u components (all of them, or 1 for component 0 alone)", filled.nchannel, info.ncomp);
                }
                for(unsigned c = 0; c < filled.nchannel; c++) {
                        j2p_plane &p = filled.planes[c];
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
                if(!filled.out_w) { filled.out_w = info.width; }
                if(!filled.out_h) { filled.out_h = info.height; }
                job = &filled;
        }
        if(jpeg) {
                if(job->out_bits || job->out_coef[0] || job->out_tensor.data) {
                        return j2p_fail(J2P_EINVAL, "job: a JPEG job needs out_bits 0, no out_coef and out_tensor.data NULL");
                }
                if(job->tile) { return j2p_fail(J2P_EINVAL, "job: JPEG output of a row-tiled job is not supported"); }
                if(const char *why = j2p_jpeg_error(&jpeg->spec, job->nchannel)) { return j2p_fail(J2P_EINVAL, "job: %s", why); }
                if(jpeg->spec.width != job->out_w || jpeg->spec.height != job->out_h) {
                        return j2p_fail(J2P_EINVAL, "job: the JPEG is %ux%u, the job's image (out_w x out_h) %ux%u", jpeg->spec.width, jpeg->spec.height,
                                        job->out_w, job->out_h);
                }
                if(!jpeg->size || (!jpeg->out && jpeg->capacity)) { return j2p_fail(J2P_EINVAL, "job: JPEG output needs out and size"); }
        }
        int samples_device = -1;
        if(samples) {
                if(const int rc = validate_samples(*job, samples, &samples_device); rc != J2P_OK) { return rc; }
        }
        int outputs_device = -1;
        if(nout) {
                if(const int rc = validate_outputs(*job, nout, outs, &outputs_device); rc != J2P_OK) { return rc; }
        }
        if(f) {
                if(!job->out_tensor.data) { return j2p_fail(J2P_EINVAL, "job: a resampled job needs tensor output (out_tensor)"); }
                if(const char *why = j2p_resample_error(f, job->out_w, job->out_h)) { return j2p_fail(J2P_EINVAL, "job: %s", why); }
        }
        if(r) {
                if(!job->out_tensor.data) { return j2p_fail(J2P_EINVAL, "job: a resized job needs tensor output (out_tensor)"); }
                if(const char *why = j2p_resize_error(r, job->out_w, job->out_h)) { return j2p_fail(J2P_EINVAL, "job: %s", why); }
        }
        Job *j = new(std::nothrow) Job();
        if(!j) { return j2p_fail(J2P_ENOMEM, "host allocation failed"); }
        j->desc = *job;
        if(r) {
                j->resize = *r;
                j->resized = true;
        }
        if(f) {
                j->resample = *f;
                j->resampled = true;
        }
        if(nout) { j->outputs.assign(outs, outs + nout); }
        if(samples) { j->samples.assign(samples, samples + job->nchannel); }
        if(file) { j->file = std::move(file_in); }
        if(jpeg) {
                // the tables travel with the job
                j->jpeg = *jpeg;
                j->jpeg.on = true;
                for(unsigned c = 0; c < job->nchannel; c++) {
                        memcpy(j->jpeg.tables[c], jpeg->spec.quant[c], sizeof(j->jpeg.tables[c]));
                        j->jpeg.spec.quant[c] = j->jpeg.tables[c];
                }
        }
        if(job->out_tensor.data || nout) {
                // what can be refused is refused here, and the job is pinned to the GPU that holds its tensor(s)
                int rc = validate_job(j->desc);
                if(nout) { j->device = outputs_device; }
                else if(rc == J2P_OK && j2p_device_of_pointer(job->out_tensor.data, &j->device) != J2P_OK) {
                        rc = j2p_fail(J2P_EINVAL, "job: out_tensor.data is not device memory (managed and host memory are refused)");
                }
                bool owned = false;
                for(int dev : b->devices) { owned = owned || dev == j->device; }
                if(rc == J2P_OK && !owned) { rc = j2p_fail(J2P_EINVAL, "job: the tensor lives on device %d, which this batch does not drive", j->device); }
                if(rc != J2P_OK) { delete j; return rc; }
        }
        if(samples_device >= 0) {
                // device samples pin the job as tensors do: to their GPU, which must be the tensors' and one of the batch's
                int rc = J2P_OK;
                bool owned = false;
                for(int dev : b->devices) { owned = owned || dev == samples_device; }
                if(j->device >= 0 && j->device != samples_device) {
                        rc = j2p_fail(J2P_EINVAL, "job: the samples live on device %d, the output tensor on device %d", samples_device, j->device);
                }
                else if(!owned) { rc = j2p_fail(J2P_EINVAL, "job: the samples live on device %d, which this batch does not drive", samples_device); }
                if(rc != J2P_OK) { delete j; return rc; }
                j->device = samples_device;
        }
        if(file_device >= 0) {
                // a file in device memory pins the job as device samples do
                int rc = J2P_OK;
                bool owned = false;
                for(int dev : b->devices) { owned = owned || dev == file_device; }
                if(j->device >= 0 && j->device != file_device) {
                        rc = j2p_fail(J2P_EINVAL, "job: the file lives on device %d, the output tensor on device %d", file_device, j->device);
                }
                else if(!owned) { rc = j2p_fail(J2P_EINVAL, "job: the file lives on device %d, which this batch does not drive", file_device); }
                if(rc != J2P_OK) { delete j; return rc; }
                j->device = file_device;
        }
        const bool pinned = j->device >= 0;
        {
                std::lock_guard<std::mutex> g(b->lock);
                if(b->quit) { delete j; return j2p_fail(J2P_ESTATE, "batch is shutting down"); }
                j->ticket = b->next_ticket++;
                b->jobs[j->ticket] = j;
                b->queue.push_back(j);
                *ticket = j->ticket;
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
        return submit(b, job, nullptr, nullptr, 0, nullptr, nullptr, nullptr, ticket);
}

int j2p_batch_submit_resized(j2p_batch *b, const j2p_job *job, const j2p_resize *r, int *ticket)
{
        return submit(b, job, r, nullptr, 0, nullptr, nullptr, nullptr, ticket);
}

int j2p_batch_submit_resampled(j2p_batch *b, const j2p_job *job, const j2p_resample *r, int *ticket)
{
        return submit(b, job, nullptr, r, 0, nullptr, nullptr, nullptr, ticket);
}

int j2p_batch_submit_outputs(j2p_batch *b, const j2p_job *job, unsigned n, const j2p_output outs[], int *ticket)
{
        const bool none = n == 0 || !outs;
        return submit(b, job, nullptr, nullptr, none ? 0 : n, none ? nullptr : outs, nullptr, nullptr, ticket);
}

int j2p_batch_submit_samples(j2p_batch *b, const j2p_job *job, const j2p_samples samples[], unsigned n, const j2p_output outs[], int *ticket)
{
        const bool none = n == 0 || !outs;
        return submit(b, job, nullptr, nullptr, none ? 0 : n, none ? nullptr : outs, samples, nullptr, ticket);
}

int j2p_batch_submit_jpeg(j2p_batch *b, const j2p_job *job, const j2p_samples samples[], const j2p_jpeg *spec, uint8_t *out, size_t capacity,
                          size_t *size, int *ticket)
{
        if(!spec) { return j2p_fail(J2P_EINVAL, "job: jpeg: spec is NULL"); }
        JpegOut jpeg;
        jpeg.spec = *spec;
        jpeg.out = out;
        jpeg.capacity = capacity;
        jpeg.size = size;
        return submit(b, job, nullptr, nullptr, 0, nullptr, samples, &jpeg, ticket);
}

int j2p_batch_submit_file(j2p_batch *b, const j2p_job *job, const uint8_t *file, size_t size, unsigned n, const j2p_output outs[], int *ticket)
{
        if(!file || size == 0) { return j2p_fail(J2P_EINVAL, "job: file is NULL or empty"); }
        const bool none = n == 0 || !outs;
        return submit(b, job, nullptr, nullptr, none ? 0 : n, none ? nullptr : outs, nullptr, nullptr, ticket, file, size);
}

int j2p_batch_submit_file_jpeg(j2p_batch *b, const j2p_job *job, const uint8_t *file, size_t size, const j2p_jpeg *spec, uint8_t *out,
                               size_t capacity, size_t *out_size, int *ticket)
{
        if(!file || size == 0) { return j2p_fail(J2P_EINVAL, "job: file is NULL or empty"); }
        if(!spec) { return j2p_fail(J2P_EINVAL, "job: jpeg: spec is NULL"); }
        JpegOut jpeg;
        jpeg.spec = *spec;
        jpeg.out = out;
        jpeg.capacity = capacity;
        jpeg.size = out_size;
        return submit(b, job, nullptr, nullptr, 0, nullptr, nullptr, &jpeg, ticket, file, size);
}

void j2p_debug_job_layout(size_t *size, size_t *out_tensor_offset)
{
        if(size) { *size = sizeof(j2p_job); }
        if(out_tensor_offset) { *out_tensor_offset = offsetof(j2p_job, out_tensor); }
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
