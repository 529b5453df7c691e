/*
 * jpeg2png_amd — MI355X (gfx950) implementation of jpeg2png's deblocking solver.
 *
 * C-ABI of libjpeg2png_amd.so.  Plain pointers and sizes only; every function
 * except j2p_last_error()/j2p_version() returns 0 on success and a negative
 * J2P_E* code on failure (message via j2p_last_error()); nothing here ever
 * calls exit().  Citations are into the reference tree (victorvde/jpeg2png).
 *
 * Two layers:
 *
 *  1. Drop-in layer (declared in jpeg2png_amd_compute.h, C host code):
 *       void compute(unsigned nchannel, struct coef coefs[], struct logger *log,
 *                    struct progressbar *pb, float weight, float pweight[],
 *                    unsigned iterations);
 *     same symbol, signature, ownership and callback behaviour as
 *     compute.h:8 / compute.c:407-465, linked in place of compute.o.
 *
 *  2. Shim layer (this file): what that host code — or any other FFI (ctypes,
 *     cgo, JNI) — binds.  A `j2p_solver` owns the device-resident working set of
 *     ONE compute() call (the reference's `struct aux`, compute.c:21-34, for all
 *     channels) on one GPU.  A solver may hold just a horizontal BAND of rows of
 *     a taller plane (row tiling over several GPUs); the caller then exchanges
 *     the band-edge rows and the per-row-of-tiles gradient norms between the two
 *     phase calls of every iteration.
 */
#ifndef JPEG2PNG_AMD_H
#define JPEG2PNG_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define J2P_OK          0
#define J2P_EINVAL     -1   /* bad argument / precondition of compute() violated   */
#define J2P_ENOMEM     -2   /* host or device allocation failed                    */
#define J2P_EDEVICE    -3   /* HIP runtime error, no usable gfx950 device          */
#define J2P_ESTATE     -4   /* call sequence error                                 */

#define J2P_MAX_CHANNELS 3  /* ASSUME(nchannel <= 3), compute.c:118                */
#define J2P_HALO_ROWS    2  /* TGV2 gradient reach in rows, compute.c:137-143,165-183 */
#define J2P_TILE_ROWS   16  /* rows per gradient tile = granularity of the norm partials */

/* One colour component as compute() receives it — the fields of `struct coef`
 * (jpeg2png.h:7-20) that the solver reads.  All pointers are HOST pointers. */
typedef struct j2p_plane {
        unsigned w, h;              /* coefficient-plane size; multiples of 8 (box.c:6-7)   */
        unsigned w_samp, h_samp;    /* max_samp / comp_samp (jpeg.c:57-58), >= 1            */
        const int16_t *data;        /* quantised DCT coefficients, block-major
                                       [h/8][w/8][64], natural order (jpeg.c:68-77)         */
        const float *fdata;         /* decoded plane, row-major w*h (jpeg.c:83-92 +
                                       jpeg2png.c:131-139); may be NULL: the library then
                                       decodes `data` itself on the device                  */
        const uint16_t *quant_table;/* 64 entries, natural order, all non-zero (jpeg.c:41-46) */
} j2p_plane;

/* Zooming (upscaling while deblocking) by an integer s: multiply w_samp and h_samp of EVERY plane by s, and (j2p_job)
 * set out_w / out_h to s times the image size.  The canvas is then s times as wide and as high (compute.c:407-416), x_0
 * the replicated planes (compute.c:295-309), and the result the smoothest image whose means over each coefficient's
 * s*w_samp x s*h_samp footprint re-encode to the given coefficients (compute.c:334-404) — the reference's compute() on
 * the same factors, bit for bit.  Limits: s in 1..4 (what the command-line driver and the Python binding accept; the
 * wide-footprint projection path covers footprints 3, 4, 6 and 8 columns wide, others take the generic one), and the
 * canvas height at most 65536 rows, as for any input. */

/* Row band of the canvas this solver owns, in canvas rows.  {0,0} = whole canvas.
 * row_begin/row_end must be multiples of lcm(8*h_samp) over channels and of
 * J2P_TILE_ROWS so that no DCT block and no gradient tile straddles two GPUs. */
typedef struct j2p_band {
        unsigned row_begin, row_end;
} j2p_band;

typedef struct j2p_solver j2p_solver;

/* per-iteration log row = arguments of logger_log() (logger.c:20, compute.c:271-272) */
typedef struct j2p_log_row {
        double objective, prob_dist, tv, tv2;
} j2p_log_row;

const char *j2p_version(void);
const char *j2p_last_error(void);            /* thread-local */
int j2p_device_count(int *count);

/* aux_init (compute.c:278-310) on the device: uploads the planes (for a band:
 * only the coefficient rows the band covers; `planes` always describes the
 * WHOLE image, host arrays may be band-local when bit 0 of band_local_arrays is set;
 * bit 1, J2P_BAND_EVEN_IF_WHOLE: a band covering every row is still driven with the
 * phase calls and exchanges like any other band — one-band runs of the row tiling),
 * allocates x_k, x_{k-1}, gradient, prob state, and sets x_k = x_{k-1} =
 * replicate-upsample(fdata).  `iterations` fixes the step size
 * radius/sqrtf(1+iterations) (compute.c:443).  `stream` is a hipStream_t
 * (NULL = the solver creates its own). */
int j2p_solver_create(j2p_solver **out, int device, void *stream,
                      unsigned nchannel, const j2p_plane planes[],
                      float weight, const float pweight[], unsigned iterations,
                      j2p_band band, int band_local_arrays);
void j2p_solver_destroy(j2p_solver *s);
#define J2P_BAND_LOCAL_ARRAYS  1
#define J2P_BAND_EVEN_IF_WHOLE 2

/* Device memory of destroyed solvers is cached per process and handed to the next solver on the same device
 * (hipMalloc / hipFree cost milliseconds and hipFree stalls every stream of the device, which matters when the
 * host calls compute() from several threads, jpeg2png.c:147,330).  Bounded PER DEVICE: 16 blocks and 8 GiB
 * (environment J2P_POOL_MIB = another limit in MiB, 0 = cache nothing); any device allocation of the library
 * that runs out of memory drops the cache and retries.  j2p_pool_trim() releases the cache; j2p_batch_destroy()
 * and j2p_tiled_destroy() call it. */
void j2p_pool_trim(void);
/* diagnostics: blocks the CALLING thread has taken from the cache or the device so far (a solver's arena, its scratch, a
 * coder's block — each request that was not met by the block already held counts once).  A call whose block had to grow k
 * times took 1 + k; a call that found its block large enough took none. */
unsigned long long j2p_pool_thread_takes(void);

/* diagnostics: schedule switches that change speed, never results (A/B timing and the parity tests of both
 * schedules).  Only between iterations. */
#define J2P_OPT_NORM_FOLD     1   /* 1 (default for band solvers, for whole canvases up to 2.5 Mpixel and for whole canvases from
                                     32 Mpixel on): level 1 of the ||g|| reduction runs inside the gradient kernel (its
                                     last-arriving wavefronts); 0: separate reduction kernel — same bits */
/* (2 is not an option any more: the all-channels-in-one-wavefront gradient kernel it selected is deleted) */
#define J2P_OPT_NORM_IN_PROJECT 4 /* 1 (needs NORM_FOLD): the gradient kernel leaves per-tile-row sums and every wavefront of
                                     the projection kernel runs the final tree itself: no reduction launch in between */
#define J2P_OPT_NT_GRADIENT 5     /* 0..3: which streams are accessed non-temporally (1: the gradient plane, 2: + the prob
                                     state, 3: + the coefficients); negative = default: by the working sets of ALL
                                     solvers live on the device against its Infinity Cache (256 MiB), re-evaluated at
                                     create and reset (environment J2P_NT_SCOPE=solver: this solver's own only) */
#define J2P_OPT_MIXED_PROJECT 6   /* 1 (default): canvases up to 1 Mpixel project all channels in ONE launch whatever their
                                     sampling; 0: one launch per sampling class, as large canvases do */
#define J2P_OPT_NARROW_COEFFICIENTS 7 /* 1 (default): a channel whose quantised coefficients all lie in [-127, 127] (found at create)
                                     keeps them resident as one byte each and the projection reads those: 21 instead of
                                     22 bytes per pixel; 0: the int16 form (jpeg2png.h:14) for every channel — same floats, same bits */
#define J2P_OPT_WIDE_FOOTPRINT 8  /* 1 (default): a channel whose footprint is 3, 4, 6 or 8 canvas columns wide (any rows: zoomed
                                     channels, see "Zooming" at j2p_plane) is projected by the wide-footprint path wherever its strip
                                     lies inside canvas and coverage — except in the one-launch projection of small canvases with
                                     several samplings (J2P_OPT_MIXED_PROJECT); 0: the generic path for those channels — same bits */
#define J2P_OPT_PHASE_ORDER 9     /* J2P_PHASE_ORDER(gradient, project): the order in which every XCD walks its run of each phase
                                     launch's work; negative = default: the policy of j2p_geometry.h (j2p_phase_order_of).
                                     The environment variable J2P_PHASE_ORDER, read at create, takes the same values — same bits */
#define J2P_ORDER_FORWARD 0         /* every XCD walks its contiguous run of the canvas top-down */
#define J2P_ORDER_REVERSE 1         /* every XCD walks its OWN run bottom-up: with the other phase forward each phase starts
                                       on the rows the XCD's L2 touched last in the phase before (serpentine) */
#define J2P_PHASE_ORDER(gradient, project) ((gradient) | ((project) << 1))
int j2p_solver_debug_option(j2p_solver *s, int option, int value);
/* the orders the solver's next iteration takes: J2P_ORDER_* of the gradient and of the projection phase */
int j2p_solver_phase_order(const j2p_solver *s, unsigned *gradient, unsigned *project);
/* bytes per quantised coefficient the projection kernel reads for channel c: 1 or 2 (J2P_OPT_NARROW_COEFFICIENTS) */
int j2p_solver_coefficient_bytes(const j2p_solver *s, unsigned c, unsigned *bytes);
/* *shared = 1 when channel c keeps its gradient and its prob state in ONE buffer (a channel sampled 1x1 whose coefficient
 * raster has the canvas's pitch, with the prob term on: the two are never live at the same pixel at the same time), else 0 */
int j2p_solver_shares_state(const j2p_solver *s, unsigned c, int *shared);
/* bytes of device memory the solver carved its planes, state and reduction buffers from */
int j2p_solver_arena_bytes(const j2p_solver *s, size_t *bytes);
/* bytes of the one block the output stage keeps for this solver (tensor taps, the JPEG coder's stages): 0 before the first call that
 * needs it; it only grows, and a call that finds it large enough allocates nothing */
int j2p_solver_output_scratch_bytes(const j2p_solver *s, size_t *bytes);
/* *on = 1 when the interior strips of channel c take the wide-footprint projection path in an unlogged run (J2P_OPT_WIDE_FOOTPRINT,
 * J2P_OPT_MIXED_PROJECT), else 0 */
int j2p_solver_wide_footprint(const j2p_solver *s, unsigned c, unsigned *on);

/* The checked build (the analogue of the reference's DEBUG=1, whose pixel indexer p() asserts every access,
 * utils.h:68-81): compiled with -DJ2P_DEBUG, every global load and store of the two phase kernels is compared
 * with the byte range it is meant to stay in; violations are counted on the device.  j2p_debug_build() tells
 * which build this is; j2p_solver_debug_violations() returns the count, the code of the first offending site
 * (1xx = gradient phase, 2xx = projection phase, see j2p_kernels.hip.h) and its offset; J2P_ESTATE in a release
 * build, where the checks are compiled out. */
int j2p_debug_build(void);
/* Test hook (no device needed): the map from k_gradient's workgroups to (strip, rows) — j2p_kernels.hip.h: grad_item —
 * evaluated on the host for a W x rows plane with `rows_per_tile`-row tile rows, one wavefront per strip
 * (channel_wavefronts 1) or per strip and channel (2, 3), the given shares (1/256 of every XCD's run) of double / half /
 * quarter tile-row items, every XCD's run top-down (`reverse` 0) or bottom-up (J2P_ORDER_REVERSE).  items: up to max_items records of five unsigned {strip,
 * first row, rows, tile row, kind (0 whole, 1 half, 2 quarter, 3 double)} in dispatch order (workgroup, then wavefront);
 * *n_items: how many the launch has; *workgroups: its grid. */
int j2p_debug_grad_items(unsigned W, unsigned rows, unsigned rows_per_tile, unsigned channel_wavefronts, unsigned zone_d, unsigned zone_b,
                         unsigned zone_c, int reverse, unsigned *items, unsigned max_items, unsigned *n_items, unsigned *workgroups);
/* ... and with item_workgroup[i] = the workgroup of item i (it runs on XCD workgroup % 8) */
int j2p_debug_grad_items_workgroups(unsigned W, unsigned rows, unsigned rows_per_tile, unsigned channel_wavefronts, unsigned zone_d, unsigned zone_b,
                                    unsigned zone_c, int reverse, unsigned *items, unsigned *item_workgroup, unsigned max_items, unsigned *n_items,
                                    unsigned *workgroups);
/* Test hook (no device needed): the map from a projection launch's workgroups to strips — j2p_kernels.hip.h: project_item —
 * evaluated on the host for a launch over `nby` block rows of `strips_x` strips (by = by_offset + i * by_mul for i < nby: the
 * whole phase is 0, 1, block rows; the split phases take the first and last, or all but those), walked in `order`
 * (J2P_ORDER_FORWARD or J2P_ORDER_REVERSE).  items: up to max_items records of four unsigned {workgroup, wavefront,
 * block row, strip in the row} of the ACTIVE wavefronts in dispatch order; *n_items: how many; *workgroups: the grid. */
int j2p_debug_project_items(unsigned strips_x, unsigned nby, unsigned by_offset, unsigned by_mul, int order, unsigned *items,
                            unsigned max_items, unsigned *n_items, unsigned *workgroups);
/* Test hook (no device needed): the phase-order policy (j2p_geometry.h: j2p_phase_order_of) for a solver of W x rows canvas rows
 * whose iteration touches `working_set` bytes, `planes` of them the two iterates, whole canvas (band 0) or band (1) */
int j2p_debug_phase_order(size_t working_set, size_t planes, unsigned W, unsigned rows, int band, unsigned *gradient, unsigned *project);
/* Test hook (no device needed): the solver's norm plan — who reduces ||g|| between the two phase kernels of ONE iteration
 * (DESIGN.md section 4 has the table) — for a whole-canvas (whole 1) or band (0) solver with J2P_OPT_NORM_FOLD `fold`,
 * J2P_OPT_NORM_IN_PROJECT `norm_in_project` (0, 1, 2), bands finishing ||g|| inside k_project (`band_nip`, the default) or
 * not, `tile_rows` tile rows in the canvas, the phase the reduction would ride on issued in parts (`split`: the gradient
 * phase of a whole canvas, the projection phase of a band) and the CSV sums wanted (`log`).
 * *level1, who forms the per-tile-row sums: */
#define J2P_NORM_L1_NONE 0      /* nobody: k_norm_whole reads the strips' partials itself */
#define J2P_NORM_L1_TICKETS 1   /* the gradient launch: the last wavefront to arrive at a tile row sums it */
#define J2P_NORM_L1_ROWSUMS 2   /* a k_rowsums launch behind the gradient phase */
/* *level2, who runs the tree over them and writes ||g||: */
#define J2P_NORM_L2_GRADIENT 0       /* the gradient launch: its last wavefront */
#define J2P_NORM_L2_NORM_WHOLE 1     /* a k_norm_whole launch */
#define J2P_NORM_L2_NORM_FINISH 2    /* a k_norm_finish launch */
#define J2P_NORM_L2_PROJECT_WAVES 3  /* every wavefront of k_project (NIP 1) */
#define J2P_NORM_L2_PROJECT_FIRST 4  /* the first wavefront of every workgroup of k_project (NIP 2) */
#define J2P_NORM_L2_EXTERNAL 5       /* the caller, between the phases (j2p_solver_norm_from_bands / _norm_external): never
                                        planned, only what those calls turn a plan into */
/* *launches: kernel launches of such an iteration, 2 + the reduction launches of the plan (k_rowsums, k_norm_whole,
 * k_norm_finish). */
int j2p_debug_norm_plan(int whole, int fold, int norm_in_project, int band_nip, unsigned tile_rows, int split, int log,
                        int *level1, int *level2, unsigned *launches);
int j2p_solver_debug_violations(j2p_solver *s, unsigned long long *count, unsigned *site, unsigned long long *offset);

/* Timing tool (builds with -DJ2P_TRACE only, tools/wave_trace.py; J2P_ESTATE otherwise): while on, every wavefront
 * of the two phase kernels appends {start, first data, end (10 ns ticks), id} — four 64-bit words — to a device
 * buffer; a call with host_out copies up to max_records records out and empties the buffer. */
int j2p_solver_trace(j2p_solver *s, int on, unsigned long long *host_out, unsigned max_records, unsigned *n);

/* canvas geometry (compute.c:410-416) and band bookkeeping */
int j2p_solver_canvas(const j2p_solver *s, unsigned *W, unsigned *H);
int j2p_solver_band(const j2p_solver *s, unsigned *row_begin, unsigned *row_end);

/* kernel launches per iteration of an unlogged run of whole phases: 2 = gradient and projection with ||g|| reduced inside
 * them, + the reduction launches the solver's norm plan issues in between (k_rowsums, k_norm_whole, k_norm_finish; see
 * j2p_debug_norm_plan).  Read from the plan, so also right where the tile-row limit bites: a whole canvas or a band of a
 * canvas with more than 1024 tile rows takes k_norm_finish (3; reported as 2 before), and a band with folding off takes
 * k_rowsums as well (3 or 4; k_rowsums went uncounted before). */
int j2p_solver_launches_per_iteration(const j2p_solver *s, unsigned *n);

/* back to iteration 0 from the inputs that are already resident in HBM */
int j2p_solver_reset(j2p_solver *s);

/* The whole iteration loop (compute.c:427-453) for a solver that owns the whole
 * canvas.  Runs `n` further iterations asynchronously on the solver's stream;
 * if `rows` is non-NULL it receives n log rows (this synchronises at the end). */
int j2p_solver_run(j2p_solver *s, unsigned n, j2p_log_row *rows);

/* The same loop split at its two device-wide dependencies, for row-tiled runs.
 *   phase_gradient : FISTA point (compute.c:430-440) + prob/TV/TGV2 gradient
 *                    (compute.c:239-261) for the band; leaves one double per
 *                    channel per row-of-tiles (sum of g*g) in the partials buffer.
 *   [caller all-gathers the partials of all bands into norm_partials_all]
 *   phase_project  : norm (compute.c:200-207, fixed summation order over the
 *                    GLOBAL partial array => GPU-count invariant), step
 *                    (:209-216), projection (:334-404), next prob state.
 *   [caller sends the band's first/last J2P_HALO_ROWS rows of the new iterate
 *    to the neighbouring bands' halo rows]
 */
int j2p_solver_phase_gradient(j2p_solver *s);
int j2p_solver_phase_project(j2p_solver *s);

/* phase_gradient in two parts, to hide the halo exchange behind compute: the INTERIOR part
 * (every 16-row segment except the band's first and last) reads no halo row and can be issued
 * straight after phase_project; the EDGES part needs the neighbours' rows and may go to another
 * stream (NULL = the solver's).  Once the solver's stream has been made to wait for the EDGES
 * part, j2p_solver_phase_rowsums() finishes the phase (partials_local is valid after it). */
/* (Both split forms measured slower than whole phases wherever tried — DESIGN.md section 10 — and answer only in the
 * experiments build, -DJ2P_EXPERIMENTS: j2p_experiments_build() == 1; the release library returns J2P_ESTATE.) */
int j2p_experiments_build(void);
#define J2P_GRADIENT_INTERIOR 1
#define J2P_GRADIENT_EDGES    2
int j2p_solver_phase_gradient_part(j2p_solver *s, int part, void *stream);
int j2p_solver_phase_rowsums(j2p_solver *s);

/* phase_project in two parts, for the same purpose: the BOUNDARY part computes the norm and projects the
 * band's first and last block row of every channel — the rows send_top / send_bottom point into — so the
 * halo exchange can start while the INTERIOR part (everything else; ends the iteration) is still running. */
#define J2P_PROJECT_BOUNDARY 1
#define J2P_PROJECT_INTERIOR 2
int j2p_solver_phase_project_part(j2p_solver *s, int part);

/* Device addresses the caller needs for the exchanges (all on the solver's device).
 *   partials_local : nchannel * local_tile_rows doubles written by phase_gradient
 *   partials_all   : nchannel * global_tile_rows doubles read by phase_project;
 *                    for a whole-canvas solver both are the same buffer. Layout
 *                    [tile_row][channel], so the bands of consecutive GPUs concatenate.
 *   halo addresses : for channel c, the rows of the CURRENT iterate x_k:
 *                    send_top  = first J2P_HALO_ROWS own rows, recv_top = the halo
 *                    rows above them (same for bottom); each J2P_HALO_ROWS*W floats.
 *   log_local      : NULL unless j2p_solver_set_logging() is on; then 2 + J2P_MAX_CHANNELS doubles:
 *                    the band's tv and tv2 sums (valid after the gradient phase) and its prob distance
 *                    per channel for the state the projection phase leaves. */
typedef struct j2p_exchange {
        double *partials_local;  unsigned local_tile_rows;
        double *partials_all;    unsigned global_tile_rows; unsigned first_tile_row;
        float *send_top[J2P_MAX_CHANNELS], *recv_top[J2P_MAX_CHANNELS];
        float *send_bottom[J2P_MAX_CHANNELS], *recv_bottom[J2P_MAX_CHANNELS];
        size_t halo_floats;
        double *log_local;
} j2p_exchange;
int j2p_solver_exchange_info(j2p_solver *s, j2p_exchange *info);

/* Test hook, read-only: where the gradient phase leaves the STRIP partials partials_local is summed from — part_g2,
 * doubles [channel][local tile row][strip] in device memory, one per wavefront item of k_gradient (sum of g^2 over
 * rows_per_tile rows x 124 columns) — and their geometry.  After a gradient phase that folds level 1 into the launch
 * (J2P_NORM_L1_TICKETS) every partial carries the iteration's parity in its sign bit; the magnitude is the sum.
 * Any of the output pointers may be NULL.  (tests/test_norm_gpu.py compares the doubles with tests/norm_cases.py) */
int j2p_solver_debug_partials(j2p_solver *s, double **part_g2, unsigned *ntx, unsigned *tile_rows_local, unsigned *rows_per_tile);

/* Pieces of a row-tiled run inside ONE process (what j2p_tiled below is made of; peers' device pointers must be
 * accessible from the solver's device: same GPU, or peer access enabled).
 *   stream            : the hipStream_t the solver launches on
 *   halo_rows         : the send/recv row addresses of j2p_exchange for x buffer 0 or 1 — the iterate produced by
 *                       iteration k (0-based) lives in buffer (k + 1) & 1 — independent of the solver's state
 *   norm_from_bands   : between the two phases: ||g|| from every band's level-1 sums (partials_local), read in
 *                       place; replaces the all-gather into partials_all.  nout == 0: the result is this solver's
 *                       norm; nout > 0: it is stored into every norm_out[i] (j2p_solver_norm_ptr() of the bands,
 *                       this solver's included) — ONE band reduces for all, the others call norm_external
 *   norm_external     : between the two phases: another band's norm_from_bands has stored (or will have stored, by
 *                       the time the solver's stream gets there — the caller orders the streams) this solver's norm
 *   alternate_rowsums : band solvers: from now on iteration k leaves its level-1 sums in buffers[k & 1] (returned;
 *                       buffers[0] is partials_local), so that a band may start its next gradient phase while
 *                       slower bands are still reading this iteration's sums
 *   copy_rows         : n row blocks copied on the solver's stream (the neighbours' edge rows into its halo rows) */
int j2p_solver_stream(j2p_solver *s, void **stream);
int j2p_solver_halo_rows(j2p_solver *s, int buffer, j2p_exchange *info);
int j2p_solver_alternate_rowsums(j2p_solver *s, const double *buffers[2]);
int j2p_solver_norm_from_bands(j2p_solver *s, unsigned nband, const double *const rowsums[],
                               const unsigned first_tile_row[], const unsigned tile_rows[],
                               unsigned nout, float *const norm_out[]);
int j2p_solver_norm_ptr(j2p_solver *s, float **norm);              /* device address of the solver's [channel] norms */
int j2p_solver_norm_external(j2p_solver *s);
int j2p_solver_copy_rows(j2p_solver *s, unsigned n, float *const dst[], const float *const src[], size_t floats);

/* Bands that can WRITE each other's memory (same GPU, or peer access): the two per-iteration exchanges without a
 * kernel of their own.  After link_bands a band's projection phase stores its first / last J2P_HALO_ROWS rows of the
 * new iterate ALSO into the neighbouring solvers' halo rows (no halo copy or send), and its gradient phase stores
 * its level-1 sums of ||g||^2 into EVERY band's own copy of the global [tile row][channel] array (no reduction
 * launch on a root band, no norm event); the projection phase then reduces ||g|| from its own copy inside k_project.
 * A band iteration is two launches, and all traffic between GPUs is posted writes.
 *   up_halo / down_halo : [x buffer 0 / 1][channel] — j2p_solver_halo_rows(neighbour above, buffer).recv_bottom /
 *                         (neighbour below, buffer).recv_top; all NULL at the canvas's first / last band
 *   push                : [iteration parity][band] — every band's j2p_solver_global_rowsums() arrays (this band's
 *                         own included), npush of them
 * The CALLER orders the streams: a band's gradient phase of iteration k behind its neighbours' projection of k - 1;
 * its projection of k behind EVERY band's gradient phase of k — which is also what makes the stores into the
 * neighbours' halo rows safe: they replace the halo of x_{k-1}, which the neighbours' gradient phase of k still read. */
typedef struct j2p_band_links {
        float *up_halo[2][J2P_MAX_CHANNELS];
        float *down_halo[2][J2P_MAX_CHANNELS];
        unsigned npush;
        double *push[2][32];
        /* optional (ncount 0 = none): counters in memory every GPU can update atomically (coherent pinned host memory);
         * the gradient launch adds 1 to each when the band's last tile row has been pushed, so that a band's stream can
         * wait for "every band's gradient has finished" with ONE hipStreamWaitValue64 (nband counts per iteration) */
        unsigned ncount;
        unsigned long long *count[32];
} j2p_band_links;
int j2p_solver_global_rowsums(j2p_solver *s, double *arrays[2]);   /* band solvers: [global tile row][channel], even / odd iterations */
int j2p_solver_link_bands(j2p_solver *s, const j2p_band_links *links);   /* NULL: back to halo rows of its own */

/* One plane set row-tiled over several GPUs from one process: nband solvers, band i on devices[i] (ids may
 * repeat), one host thread per band.  cuts = nband + 1 row boundaries from 0 to the canvas height, aligned to
 * lcm(16, 8 * h_samp), or NULL for near-equal bands.  run / sync / download mirror the j2p_solver calls; the
 * planes are bit-identical to a whole-canvas solver's whatever the cut.  (Reference loop: compute.c:427-453.)
 * nband == 1 is a plain whole-canvas solver behind the same calls.  How the bands exchange their row sums of g^2 and
 * their edge rows is chosen at create time (j2p_tiled_exchange() names it).  Environment J2P_TILED_EXCHANGE / J2P_TILED_WAIT
 * NAME one (then nothing else is tried and a failure is an error).  Unnamed, and with every band on a GPU of its own, the
 * first create on a device list VERIFIES the candidates there: a scratch canvas cut from the job's first rows (three
 * 16-row tile rows per band) is solved whole by one plain solver — no exchange: the truth — and as bands through each
 * candidate; a candidate whose planes differ in one bit is demoted (one line on stderr), the fastest of the rest is kept
 * for that device list for the life of the process (J2P_TILED_VERIFY=0: never; =1: also when bands share a GPU; =2: also
 * print the timings).  Bands that share a GPU get "direct" with event waits.  The exchanges:
 *   "direct" (needs every GPU to be able to write every other's memory): both exchanges ride on the two phase kernels
 *            as posted peer writes (j2p_solver_link_bands) — two launches per band and iteration; J2P_TILED_WAIT=all
 *            (default) | root | collector | counter: how a band's projection learns that every band's gradient has
 *            finished (events, or — counter — a value in host memory the kernels count up, hipStreamWaitValue64);
 *   "copy"   round 3's schedule — a copy kernel pulls the neighbours' edge rows, one band reduces ||g|| for all
 *            (experiments build only, J2P_TILED_NORM=all: every band for itself) — kept as the cross-check of "direct" and for canvases taller
 *            than 16384 rows;
 *   "rccl"   (the candidate without peer access) ncclAllGather + grouped ncclSend / ncclRecv on the band's own stream, one
 *            communicator per band from ncclCommInitAll, librccl loaded with dlopen (J2P_RCCL_LIBRARY names another
 *            copy); needs one GPU per band.
 * J2P_EDEVICE when none of them works — or verifies — on the devices given.  host_cpu_seconds: user + system time the band
 * threads have spent issuing work so far. */
typedef struct j2p_tiled j2p_tiled;
int j2p_tiled_create(j2p_tiled **out, unsigned nband, const int devices[], const unsigned cuts[], unsigned nchannel,
                     const j2p_plane planes[], float weight, const float pweight[], unsigned iterations);
void j2p_tiled_destroy(j2p_tiled *t);
int j2p_tiled_canvas(const j2p_tiled *t, unsigned *W, unsigned *H, unsigned *nband);
int j2p_tiled_band(const j2p_tiled *t, unsigned band, int *device, unsigned *row_begin, unsigned *row_end, j2p_solver **solver);
int j2p_tiled_reset(j2p_tiled *t);                                 /* back to iteration 0 from the resident inputs */
int j2p_tiled_run(j2p_tiled *t, unsigned n, j2p_log_row *rows);   /* asynchronous unless rows != NULL */
int j2p_tiled_sync(j2p_tiled *t);
int j2p_tiled_download(j2p_tiled *t, unsigned c, float *out);      /* W * H floats */
int j2p_tiled_host_cpu_seconds(const j2p_tiled *t, double *seconds);
/* the librccl the "rccl" exchange would use (dlopen, J2P_RCCL_LIBRARY): ncclGetVersion's code (e.g. 22203), J2P_EDEVICE
 * when no usable library is found — the exchange SURVEY.md §8e names (RCCL halo send/recv + norm all-gather) */
int j2p_rccl_version(int *version);
int j2p_tiled_exchange(const j2p_tiled *t, const char **name);    /* "direct" ("direct, wait root" / "…collector"), "copy", "rccl"; "none": one plain band */

/* CSV logging for band solvers (the "+3 doubles when logging" of the norm exchange): with logging on, the
 * phase calls also leave the band's tv / tv2 / prob sums in j2p_exchange.log_local; the caller adds the bands'
 * sums up (any fixed order: the values only feed the log) and turns n iterations' worth of
 * {tv, tv2, prob[J2P_MAX_CHANNELS]} into the reference's log rows (compute.c:226-272, logger.c:20-28):
 * row i reports the prob distance of the state ENTERING iteration i (0 at iteration 0). */
int j2p_solver_set_logging(j2p_solver *s, int on);
int j2p_log_rows_from_sums(unsigned nchannel, float weight, const float pweight[], unsigned n,
                           const double *sums /* n * (2 + J2P_MAX_CHANNELS) */, j2p_log_row *rows);

/* band-local arrays only: after the caller has exchanged the halo rows of the INITIAL
 * iterate, copy them into x_{k-1}'s halo rows too (fista = copy(fdata), compute.c:307-309) */
int j2p_solver_commit_initial_halo(j2p_solver *s);

/* copy channel c's band rows of the current iterate to host (W * band_rows floats);
 * this is what compute() hands back in coef->fdata (compute.c:455-461) */
int j2p_solver_download(j2p_solver *s, unsigned c, float *out);

/* diagnostics: channel c's objective gradient as the last gradient phase left it (W * band_rows
 * floats; compute.c's aux->obj_gradient before the step).  The gradient only BETWEEN the two phases of an iteration:
 * the projection phase of a channel that keeps both in one buffer (j2p_solver_shares_state) writes the prob state of the
 * next iteration over it, block by block. */
int j2p_solver_download_gradient(j2p_solver *s, unsigned c, float *out);

/* device pointer to channel c's current iterate (own rows), for on-device consumers */
int j2p_solver_plane_ptr(j2p_solver *s, unsigned c, float **dev_ptr);

int j2p_solver_sync(j2p_solver *s);

/* average device time of the two phase kernels since the last reset, measured
 * with HIP events on the solver's stream (bench.py's roofline leg) */
int j2p_solver_kernel_times(j2p_solver *s, double *gradient_ms, double *project_ms, unsigned *samples);
int j2p_solver_enable_timing(j2p_solver *s, int every);   /* 0 = off, k = sample every k-th iteration */
/* what a bracket of two event records measures with nothing in between on the solver's stream (calibrated when timing is
 * switched on): the scale of what the event brackets add to j2p_solver_kernel_times() — reported, not subtracted */
int j2p_solver_timing_overhead(j2p_solver *s, double *event_pair_ms);

/* decode_coefficients + unbox (jpeg.c:83-92, box.c:5-19) on the device:
 * out[h*w] raster floats from block-major int16 coefficients.  Host pointers. */
int j2p_decode_plane(int device, unsigned w, unsigned h, const int16_t *data,
                     const uint16_t *quant_table, float *out);

/* 8x8 transforms on the device for n blocks of 64 floats, in place (host pointers);
 * dct8x8s / idct8x8s of ooura/dct.c:98 / :34 — exposed for the parity tests */
int j2p_dct8x8_blocks(int device, float *blocks, size_t n, int inverse);

/* The colour conversion of the PNG writer on the device (png.c:37-62: YCbCr -> RGB, clamp,
 * 8/16-bit samples, crop to w x h) including the luma +128 fix-up of jpeg2png.c:156-159,
 * from the current iterates of three (solver, channel) pairs on one device — the same solver
 * three times after a joint compute(), three solvers after `-s`.  out_host receives h*w*3
 * bytes (bits == 8) or h*w*6 bytes, big-endian samples (bits == 16), ready for libpng rows. */
typedef struct j2p_plane_ref {
        j2p_solver *solver;
        unsigned channel;
} j2p_plane_ref;
int j2p_planes_to_rgb(const j2p_plane_ref planes[3], unsigned w, unsigned h, unsigned bits, uint8_t *out_host);
/* the same for image rows [row_begin, row_end) that three solvers on one device all hold — whole-canvas or band
 * solvers (the bands of a row-tiled image convert their own rows on their own GPU); out_host receives
 * (row_end - row_begin) * w * 3 (or 6) bytes */
int j2p_planes_rows_to_rgb(const j2p_plane_ref planes[3], unsigned w, unsigned row_begin, unsigned row_end, unsigned bits,
                           uint8_t *out_host);
/* Greyscale: the same writer on ONE (solver, channel) pair with Cb = Cr = 0, i.e. R = G = B of png.c:37-45 after the
 * luma +128 fix-up — one sample per pixel.  out_host receives h*w bytes (bits == 8) or h*w*2 bytes, big-endian samples
 * (bits == 16, at most 65280).  The plane is the reference's compute(1, ...) on one component: the only component of a
 * greyscale JPEG, or component 0 (Y) of a colour one, solved alone as `-s` solves it (jpeg2png.c:147-152) — not the luma
 * of a joint compute(3, ...), whose total variation couples the channels.  Same argument checks and whole / band rules
 * as j2p_planes_to_rgb / j2p_planes_rows_to_rgb. */
int j2p_planes_to_grey(const j2p_plane_ref *plane, unsigned w, unsigned h, unsigned bits, uint8_t *out_host);
int j2p_planes_rows_to_grey(const j2p_plane_ref *plane, unsigned w, unsigned row_begin, unsigned row_end, unsigned bits,
                            uint8_t *out_host);

/* Tensor output: the same conversion up to the clamp, left ON THE DEVICE as the elements of a strided tensor — for consumers
 * that run on the GPU themselves (a model that is fed deblocked images): no 8-bit truncation, no download, no host
 * synchronisation.  For image pixel (x, y) with the planes' values Y, Cb, Cr at canvas (x, y), exactly as above (png.c:37-47,
 * jpeg2png.c:156-159):
 *     yi = (float)((double)Y + 128.)
 *     v0 = clampf((float)((double)yi + 1.402 * (double)Cr))
 *     v1 = clampf((float)((double)yi - 0.34414 * (double)Cb - 0.71414 * (double)Cr))
 *     v2 = clampf((float)((double)yi + 1.772 * (double)Cb))
 * with clampf = CLAMP(x, 0., 255.) on the narrowed float; one plane: v0 = clampf(yi), Cb / Cr are not read.  Channel k's
 * element is then
 *     u8               : (uint8_t)(unsigned)v_k — the 8-bit samples of j2p_planes_to_rgb / _grey, byte for byte;
 *     f32 / f16 / bf16 : t = v_k * scale[k] rounded to f32, then t = t + bias[k] rounded to f32 (two operations, never a
 *                        fused one, and applied also for scale 1 / bias 0: -0.f becomes +0.f); f32 stores t, f16 and bf16
 *                        store t rounded to nearest, ties to even.
 * Element (k, y, x) goes to data + k * stride_c + (y - row_begin) * stride_y + x * stride_x, strides in ELEMENTS: CHW is
 * stride_x == 1, HWC is stride_c == 1 and stride_x == nplane, and anything else is served too — a slot of an N x C x H x W
 * batch, a padded canvas, a transposed view.  Bytes that are not elements of the image are never written.  (Contiguous
 * CHW / HWC destinations whose rows are aligned to 4 elements are written with 16 / 8 / 4-byte stores; any other view one
 * element at a time: as correct, only slower.)
 * nplane is 3 or 1.  Argument checks, state checks and whole / band rules of j2p_planes_to_rgb / j2p_planes_rows_to_rgb;
 * J2P_EINVAL also for an unknown dtype, a stride below 1, data NULL, not aligned to its element size, or not plain device
 * memory of the solvers' device (managed and host memory are refused), a scale or bias that is not finite, and u8 with
 * scale != 1 or bias != 0.
 * ASYNCHRONOUS: the calls enqueue on planes[0].solver's stream and return; nothing is staged, copied or waited for on that
 * stream.  The caller orders its consumers behind j2p_solver_stream() (an event, or hipStreamSynchronize). */
#define J2P_DTYPE_U8 0
#define J2P_DTYPE_F16 1
#define J2P_DTYPE_BF16 2
#define J2P_DTYPE_F32 3
typedef struct j2p_tensor {
        void *data;                      /* DEVICE memory on the solvers' device */
        int dtype;
        ptrdiff_t stride_c, stride_y, stride_x;   /* in elements, all >= 1 */
        float scale[3], bias[3];         /* float dtypes; u8 requires 1 and 0 */
} j2p_tensor;
int j2p_planes_to_tensor(const j2p_plane_ref planes[], unsigned nplane, unsigned w, unsigned h, const j2p_tensor *out);
int j2p_planes_rows_to_tensor(const j2p_plane_ref planes[], unsigned nplane, unsigned w,
                              unsigned row_begin, unsigned row_end, const j2p_tensor *out);
/* Test hook (no device needed): which of k_to_tensor's destination paths the full-width rows of a w-column image of nplane
 * (3 or 1) planes take for a destination at data_address with these strides: 0 generic (one element per store), 1 planar,
 * 2 interleaved (4 elements per store; they need the address aligned to such a store and stride_y — planar with three planes
 * also stride_c — a multiple of 4 elements).  Images narrower than 4 columns are generic. */
int j2p_debug_tensor_path(unsigned w, unsigned nplane, int dtype, ptrdiff_t stride_c, ptrdiff_t stride_y, ptrdiff_t stride_x,
                          uintptr_t data_address, int *path);

/* Resized tensor output: the same elements, of a source rectangle (the box) of the w x h image, AREA-resampled to out_w x
 * out_h — what a consumer's crop and downscale (Resize, CenterCrop, RandomResizedCrop) would compute from the full-size
 * tensor, written straight into a slot of its batch.  Every bit is defined.  v_k(x, y) is the clamped float of channel k at
 * image pixel (x, y), exactly as above.  Taps of output column X, in integers: lo = X * box_w, hi = (X + 1) * box_w; the source
 * columns i = lo / out_w ... (hi - 1) / out_w of the box, with weights a_i = min(hi, (i + 1) * out_w) - max(lo, i * out_w)
 * (1 <= a_i <= out_w, and they sum to box_w); rows likewise, with box_h, out_h and weights b_j.  An axis that is not resized
 * (out_w == box_w) has one tap of weight 1 and no division.  In f32, every operation rounded on its own (never a fused
 * multiply-add, never a reciprocal):
 *     r_j = 0.f;  r_j = r_j + (float)a_i * v_k(box_x + i, box_y + j)      for i ascending
 *     acc = 0.f;  acc = acc + (float)b_j * r_j                             for j ascending
 *     m = acc;  x resized: m = m / (float)box_w;  y resized: m = m / (float)box_h;  m = min(m, 255.f)
 * and channel k's element is made of m as above (u8 truncates; the float dtypes scale, add the bias and round).  A pure crop
 * (out == box on both axes) therefore copies v_k, except that -0.f becomes +0.f.  Element (k, Y, X) goes to
 * data + k * stride_c + Y * stride_y + X * stride_x, 0 <= X < out_w, 0 <= Y < out_h; nothing else is written, and canvas values
 * outside the box are never used.  Only downscaling: enlarging is what zooming is for.
 * Whole-canvas solvers only (a band solver: J2P_ESTATE).  The checks of j2p_planes_to_tensor, and J2P_EINVAL for r NULL, an
 * empty box, a box that leaves the image, and out_w / out_h zero or larger than the box.  ASYNCHRONOUS on planes[0].solver's
 * stream, as j2p_planes_to_tensor. */
typedef struct j2p_resize {
        unsigned box_x, box_y, box_w, box_h;   /* source rectangle, image pixels */
        unsigned out_w, out_h;                  /* 1 <= out <= box on each axis */
} j2p_resize;
int j2p_planes_to_tensor_resized(const j2p_plane_ref planes[], unsigned nplane, unsigned w, unsigned h,
                                 const j2p_resize *r, const j2p_tensor *out);

/* Filtered tensor output: the same elements of the box, resampled to out_w x out_h with taps that come from a FILTER KERNEL
 * — the formula of Pillow's resize and of torch's interpolate(antialias=True, align_corners=False) — where the area form
 * takes them from overlap lengths.  One formula shrinks (the support widens with the ratio) and enlarges (the support stays
 * at the filter's radius): out_w / out_h may be larger than the box.  Every bit is defined.
 * Filters: J2P_FILTER_TRIANGLE, radius R = 1 ("bilinear"); J2P_FILTER_CUBIC, radius R = 2, Keys' cubic with a = -0.5
 * ("bicubic").  Taps of output index X of one axis (box, out), every operation IEEE double and rounded on its own (nothing
 * fused, no reciprocal), on host and device alike:
 *     scale = (double)box / (double)out;   fs = scale > 1. ? scale : 1.;   sup = R * fs
 *     c     = ((double)X + 0.5) * scale
 *     first = max(0, (long)(c - sup + 0.5));   end = min(box, (long)(c + sup + 0.5))     (the casts truncate)
 *     taps i = first .. end - 1 (always at least one):   u_i = (((double)i - c) + 0.5) / fs;   a = |u_i|
 *     triangle: w_i = a < 1. ? 1. - a : 0.
 *     cubic:    w_i = a < 1. ? ((1.5 * a - 2.5) * a) * a + 1.  :  a < 2. ? (((a - 5.) * a + 8.) * a - 4.) * -0.5  :  0.
 *     S = 0.;  S = S + w_i for i ascending;   f_i = (float)(w_i / S)
 * The window is clipped to the box and renormalised: image pixels outside the box are never used.  An axis with out == box
 * has ONE tap, of weight 1.f, at i = X.  Then in f32, every operation rounded on its own, with the columns' weights fx and
 * the rows' weights fy:
 *     r_j = 0.f;  r_j = r_j + fx_i * v_k(box_x + i, box_y + j)            for i ascending
 *     acc = 0.f;  acc = acc + fy_j * r_j                                   for j ascending
 *     m = min(max(acc, 0.f), 255.f)
 * (no division: the weights are normalised; both clamps are needed: the cubic has negative lobes, and rounding alone takes
 * a triangle's sum beyond 255) and channel k's element is made of m as above.  out == box on both axes copies v_k, except
 * that -0.f becomes +0.f.  Element (k, Y, X) goes to data + k * stride_c + Y * stride_y + X * stride_x; nothing else is written.
 * Whole-canvas solvers only.  The checks of j2p_planes_to_tensor_resized, except that the output may be larger than the box,
 * and J2P_EINVAL for an unknown filter and for out_w / out_h above J2P_RESAMPLE_MAX_OUT; a refused call writes nothing.
 * ASYNCHRONOUS on planes[0].solver's stream: two kernels are queued (the taps of both axes into scratch memory that the
 * solver keeps, then the sampling); no host synchronisation and, once that scratch has grown to the size, no allocation. */
#define J2P_FILTER_TRIANGLE 1
#define J2P_FILTER_CUBIC 2
#define J2P_RESAMPLE_MAX_OUT 65536u
typedef struct j2p_resample {
        unsigned box_x, box_y, box_w, box_h;   /* source rectangle, image pixels */
        unsigned out_w, out_h;                  /* 1 .. J2P_RESAMPLE_MAX_OUT each; smaller or larger than the box */
        int filter;                             /* J2P_FILTER_* */
} j2p_resample;
int j2p_planes_to_tensor_resampled(const j2p_plane_ref planes[], unsigned nplane, unsigned w, unsigned h,
                                   const j2p_resample *r, const j2p_tensor *out);
/* Test hook (no device needed): the taps of output index X of an axis as above, computed by the host with the code the
 * device runs: *first, *count and weights[0 .. *count).  J2P_EINVAL for an unknown filter, box or out 0, X >= out, or more
 * taps than `capacity` (then *count is still set). */
int j2p_debug_filter_taps(int filter, unsigned box, unsigned out, unsigned X, unsigned *first, unsigned *count, float *weights,
                          unsigned capacity);

/* Multi-output filtered tensor output: n (box, size, filter, tensor) items filled from the one solved image by ONE call — the
 * crops of multi-crop training, FiveCrop / TenCrop, a pyramid of sizes.  No new arithmetic: output i receives exactly the
 * elements that j2p_planes_to_tensor_resampled(planes, nplane, w, h, &outs[i].r, &outs[i].t) writes, bit for bit, and nothing
 * else is written; the text of that function is the definition.  Each output is triangle or cubic, mixed freely; an output
 * with out == box on both axes is the plain crop the filtered form defines.  The area form is not part of this call: an unknown
 * filter code, 0 included, is J2P_EINVAL.  Boxes may overlap or be equal, sizes smaller or larger than the box, dtypes may
 * differ between outputs.  Two outputs whose ELEMENTS alias are not detected: which of them wins is undefined.
 * Every output is checked with the single call's own checks, all of them before anything is queued: a refused call writes no
 * element of any output and queues nothing.  J2P_EINVAL also for n == 0, n > J2P_MAX_OUTPUTS and outs NULL; a band solver is
 * J2P_ESTATE.
 * ASYNCHRONOUS on planes[0].solver's stream, as the single call: no host synchronisation, no copy, and no allocation once the
 * solver's scratch memory has grown to the call's size — the taps of all outputs share it, so that size is the sum of theirs.
 * Queued are one launch that forms both axes' taps of every output and one sampling launch per dtype present (at most four),
 * whose grid holds exactly the workgroups the outputs' own launches would have.  n == 1 is the single call. */
#define J2P_MAX_OUTPUTS 16
typedef struct j2p_output {
        j2p_resample r;
        j2p_tensor t;
} j2p_output;
int j2p_planes_to_tensors_resampled(const j2p_plane_ref planes[], unsigned nplane, unsigned w, unsigned h, unsigned n,
                                    const j2p_output outs[]);
/* Test hooks (no device needed): the work map of such a call for n specs of a w x h image and their tensors' dtypes, computed
 * with the code the launch uses; the specs are checked as the call checks them (J2P_EINVAL).
 * _plan: per output i its tile — tiles[3 * i ..] = lanes, slots, rows per wavefront — its own grid — grids[2 * i ..] = tile
 * columns, row groups (of 4 wavefronts) — and launch_of[i], the sampling launch that holds it; *nlaunch, and per launch its
 * dtype and its number of workgroups.  Launches are in ascending dtype code, a launch's outputs in list order.
 * _workgroups: for workgroups [first, first + count) of launch `launch`, map[3 * k ..] = output, tile column, row group —
 * what the kernel's workgroup of that index finds in its prefix table.  J2P_EINVAL beyond the launch's grid. */
int j2p_debug_outputs_plan(unsigned w, unsigned h, unsigned n, const j2p_resample specs[], const int dtypes[], unsigned tiles[],
                           unsigned grids[], unsigned launch_of[], unsigned *nlaunch, int launch_dtype[4], unsigned launch_workgroups[4]);
int j2p_debug_outputs_workgroups(unsigned w, unsigned h, unsigned n, const j2p_resample specs[], const int dtypes[], unsigned launch,
                                 unsigned first, unsigned count, unsigned map[]);

/* JPEG output: ONE (solver, channel) pair's current iterate as quantised DCT coefficients, ready for libjpeg's
 * jpeg_write_coefficients — no RGB conversion and no 8-bit samples in between.  For each 8x8 block of the canvas plane:
 * dct8x8s (ooura/dct.c:98-130, the transform j2p_dct8x8_blocks exposes), every coefficient divided by quant_table[j] as
 * the correctly rounded f32 quotient, rounded to nearest (ties to even), clamped to [-1023, 1023] (what libjpeg's Huffman
 * coder accepts).  No +128 anywhere: the planes are level-shifted already (luma is centred on 0 until the PNG writer adds
 * 128, jpeg2png.c:156-159), which is what JPEG stores.  out_host receives blocks_h * blocks_w blocks of 64 int16,
 * block-major, natural order (the layout of j2p_plane.data and of libjpeg's JBLOCK rows) — blocks_w x blocks_h from the
 * canvas's top left corner, i.e. ceil(width / 8) x ceil(height / 8) for an image cropped from it.  quant_table: 64
 * entries, natural order, all non-zero (J2P_EINVAL otherwise, as for blocks_w * 8 / blocks_h * 8 beyond the canvas).
 * Whole / band rules and argument checks as j2p_planes_to_grey / j2p_planes_rows_to_grey; the rows form takes BLOCK rows
 * [block_row_begin, block_row_end), which must lie inside the solver's band (band cuts are multiples of 16 rows: no block
 * straddles two bands), and writes (block_row_end - block_row_begin) * blocks_w blocks. */
int j2p_planes_to_coefficients(const j2p_plane_ref *plane, unsigned blocks_w, unsigned blocks_h,
                               const uint16_t quant_table[64], int16_t *out_host);
int j2p_planes_rows_to_coefficients(const j2p_plane_ref *plane, unsigned blocks_w,
                                    unsigned block_row_begin, unsigned block_row_end,
                                    const uint16_t quant_table[64], int16_t *out_host);

/* Subsampled JPEG output (4:2:2, 4:2:0, 4:4:0): the same, of a plane at 1 / sub_w x 1 / sub_h of the canvas's resolution; sub_w and
 * sub_h are 1 or 2 (J2P_EINVAL otherwise).  Output sample (X, Y), 0 <= X < 8 * blocks_w, 0 <= Y < 8 * blocks_h, is the mean the
 * projection constrains (compute.c:351-359): a float accumulator that starts at 0.f takes the sub_h * sub_w canvas values at rows
 * Y * sub_h + j, columns X * sub_w + i in raster order (j outer, i inner), one float addition each, and is divided by
 * (float)(sub_w * sub_h).  A row index beyond the canvas's last row reads the last row, a column index beyond the last column the
 * last column; every block must START inside the canvas (8 * sub_w * (blocks_w - 1) < width, 8 * sub_h * (blocks_h - 1) < height:
 * J2P_EINVAL otherwise), so only the last block row / column of a grid that overhangs the canvas replicates — e.g. the 3 chroma
 * blocks (48 columns) of a 4:2:0 file made from a 40-column canvas.  The 8x8 blocks of those samples are then transformed,
 * divided, rounded and clamped exactly as above.  With sub_w = sub_h = 1 these ARE the functions above, their stricter "inside the
 * canvas" check included.  A component of sampling (sub_w, sub_h) in an image of blocks_w x blocks_h full-resolution blocks has
 * ceil(blocks_w / sub_w) x ceil(blocks_h / sub_h) blocks (libjpeg's ceil(ceil(width / sub_w) / 8)).
 * Rows form: output block row r covers canvas rows [8 * sub_h * r, 8 * sub_h * (r + 1)); its first row must lie in the solver's
 * band, and rows beyond the band are replicated only where the band ends with the canvas (band cuts are multiples of 16 rows, so
 * no 4:2:0 block row straddles two bands). */
int j2p_planes_to_coefficients_sub(const j2p_plane_ref *plane, unsigned sub_w, unsigned sub_h, unsigned blocks_w, unsigned blocks_h,
                                   const uint16_t quant_table[64], int16_t *out_host);
int j2p_planes_rows_to_coefficients_sub(const j2p_plane_ref *plane, unsigned sub_w, unsigned sub_h, unsigned blocks_w,
                                        unsigned block_row_begin, unsigned block_row_end,
                                        const uint16_t quant_table[64], int16_t *out_host);

/* Image batches (BASELINE configs[4]; the file loop jpeg2png.c:330-337): a batch owns slots_per_device worker
 * threads per GPU, each driving one image at a time on streams of its own, so that the uploads, solves and
 * downloads of different images overlap; device memory is recycled between images (no hipMalloc / hipFree per
 * image).  A job is what decode_file() does between read_jpeg() and write_png() (jpeg2png.c:141-161). */
typedef struct j2p_batch j2p_batch;
typedef struct j2p_job {
        unsigned nchannel;                     /* 1..3 */
        j2p_plane planes[J2P_MAX_CHANNELS];    /* host arrays; must stay valid until j2p_batch_wait() returns */
        int separate;                          /* 0: one joint compute(nchannel, ...) (jpeg2png.c:144) with weight[0],
                                                  iterations[0]; 1: one compute(1, ...) per component (jpeg2png.c:147-152) */
        float weight[J2P_MAX_CHANNELS];
        float pweight[J2P_MAX_CHANNELS];
        unsigned iterations[J2P_MAX_CHANNELS];
        /* output: out_bits 8 / 16 = RGB samples (png.c:37-62 incl. the luma +128 of jpeg2png.c:156-159), cropped to
         * out_w x out_h, into out_rgb (h*w*3 or h*w*6 bytes); with nchannel == 1 the samples are greyscale
         * (j2p_planes_to_grey: h*w or h*w*2 bytes into out_rgb); nchannel == 2 has no sample output.  out_bits 0 = the
         * float canvas planes into out_planes[c] (NULL entries are skipped): W*H floats of the joint canvas, or
         * — separate — of component c's own canvas, w*w_samp x h*h_samp (compute.c:410-416 per call) */
        /* (hand over output memory that is already MAPPED — arrays reused between jobs: mapping or first-touching host memory
         * while other jobs' kernels run stalls a launch of theirs each time; 229 against 196-201 images/s at 1080p on one GPU,
         * profiles/r05_batch_prealloc.jsonl) */
        unsigned out_bits, out_w, out_h;
        uint8_t *out_rgb;
        float *out_planes[J2P_MAX_CHANNELS];
        /* optional callbacks, called on the worker thread: log rows of `n` iterations starting at `first`
         * (channel = component, or 3 for a joint solve: jpeg2png.c:143,149) and progress ticks (iterations done) */
        void (*on_rows)(void *user, unsigned channel, unsigned first, unsigned n, const j2p_log_row *rows);
        void (*on_progress)(void *user, unsigned n);
        void *user;
        /* nonzero: ONE image over SEVERAL of the batch's devices — every solve of the job is row-tiled (j2p_tiled), one
         * band per device, each band converting its own rows to RGB; for the case of fewer images than GPUs
         * (decode_file -> compute of one large image, jpeg2png.c:141-152).  Same bits either way.  The devices are
         * entries [tile_first, tile_first + tile_count) of the list given to j2p_batch_create (tile_count 0 = all of
         * them), so that a few large images can each have a share of the GPUs.  How many bands there are is the
         * library's decision: a band costs its GPU ~35 us per iteration of cross-band scheduling whatever its size
         * (profiles/r03_band_alone.jsonl), so a band gets at least 2 Mpixel per channel (tile_min_band_pixels: another
         * gate; (size_t)-1 = none: tests with small images) and at least 48 rows; an image too small for two such bands —
         * and any image when the devices cannot be tiled over (no peer access and no RCCL, or no exchange that verifies on
         * them) — is solved on ONE GPU instead */
        int tile;
        unsigned tile_first, tile_count;
        size_t tile_min_band_pixels;           /* 0 = the library's gate (2 Mpixel) */
        /* JPEG output (j2p_planes_to_coefficients): out_coef[0] != NULL selects it; out_bits must then be 0 and every one of the
         * nchannel entries of out_quant (64 non-zero steps, natural order) and out_coef (out_blocks_h * out_blocks_w * 64
         * int16) must be set.  Component c comes from the joint canvas or — separate — its own solver's; a tiled job converts
         * every band's block rows on the band's GPU.  out_planes is still honoured.  All zero: no coefficient output */
        const uint16_t *out_quant[J2P_MAX_CHANNELS];
        int16_t *out_coef[J2P_MAX_CHANNELS];
        unsigned out_blocks_w, out_blocks_h;
        /* subsampled coefficient output (j2p_planes_to_coefficients_sub): channel c at 1 / out_sub_w[c] x 1 / out_sub_h[c] of the
         * resolution (1 or 2; 0 means 1).  out_blocks_w x out_blocks_h stays the grid of a full-resolution component; channel c gets,
         * and out_coef[c] holds, ceil(out_blocks_w / out_sub_w[c]) x ceil(out_blocks_h / out_sub_h[c]) blocks */
        unsigned out_sub_w[J2P_MAX_CHANNELS], out_sub_h[J2P_MAX_CHANNELS];
        /* tensor output (j2p_planes_rows_to_tensor): out_tensor.data != NULL selects it — the image, cropped to out_w x out_h, as
         * the elements of a tensor in DEVICE memory of one of the batch's GPUs; out_bits must then be 0, out_coef[0] NULL and
         * nchannel 1 or 3.  The job runs on a worker of the tensor's device (another device: J2P_EINVAL at submit), and after
         * j2p_batch_wait the tensor is complete for any stream.  Not with `tile` (J2P_EINVAL, "not supported"): bands on other
         * GPUs would have to store into the tensor's device through peer access, which no machine at hand can test.
         * out_planes is still honoured.  Appended last: the fields above keep their offsets (j2p_debug_job_layout) */
        j2p_tensor out_tensor;
} j2p_job;
/* test hook: sizeof(j2p_job) and offsetof(j2p_job, out_tensor) as this library was compiled — what a binding's own mirror of
 * the struct is compared with */
void j2p_debug_job_layout(size_t *size, size_t *out_tensor_offset);
int j2p_batch_create(j2p_batch **out, unsigned ndev, const int devices[], unsigned slots_per_device);
void j2p_batch_destroy(j2p_batch *b);                       /* finishes queued jobs first */
int j2p_batch_submit(j2p_batch *b, const j2p_job *job, int *ticket);
/* a tensor job whose tensor receives the image resized (j2p_planes_to_tensor_resized): *r is copied; job->out_tensor.data is
 * required (J2P_EINVAL without), job->out_w x out_h stays the image's crop, which the box must lie inside, and the tensor has
 * r->out_w x r->out_h elements per channel.  Not with `tile`, as every tensor job.  r == NULL: j2p_batch_submit. */
int j2p_batch_submit_resized(j2p_batch *b, const j2p_job *job, const j2p_resize *r, int *ticket);
/* the same with a filter (j2p_planes_to_tensor_resampled): the tensor may be larger than the box.  *r is copied and travels next
 * to the job, never in it; validated here, at submit.  r == NULL: j2p_batch_submit. */
int j2p_batch_submit_resampled(j2p_batch *b, const j2p_job *job, const j2p_resample *r, int *ticket);
/* a job that fills n tensors from its one solve (j2p_planes_to_tensors_resampled): the outputs are copied and travel next to the
 * job, never in it.  job->out_w x out_h is the image's crop, which every box must lie inside; job->out_tensor.data must be NULL,
 * out_bits 0 and out_coef[0] NULL (J2P_EINVAL otherwise); out_planes is still honoured; not with `tile`, as every tensor job.
 * All tensors must be device memory of ONE GPU of the batch, on a worker of which the job runs (J2P_EINVAL at submit otherwise,
 * as for a bad spec and n > J2P_MAX_OUTPUTS); after j2p_batch_wait every tensor is complete for any stream.  n == 0 or outs
 * NULL: j2p_batch_submit. */
int j2p_batch_submit_outputs(j2p_batch *b, const j2p_job *job, unsigned n, const j2p_output outs[], int *ticket);
int j2p_batch_wait(j2p_batch *b, int ticket);               /* the job's status; its error text in j2p_last_error() */

/* test hook: n > 0: the n-th j2p_solver_run() / j2p_tiled_run() call from now on (any thread) fails with J2P_EDEVICE
 * before it queues anything — how the tests make a solve fail after its create phase (j2p_compute()'s error contract);
 * n < 0: in the |n|-th j2p_tiled_run() of a multi-band solver the LAST band fails halfway through its iterations, with
 * the other bands' work queued behind it (the teardown of a failed row-tiled run); 0 disarms. */
void j2p_debug_fail_run_after(int n);

/* test hook: compares the kernels' fast division / square root (the compiler's IEEE
 * sequences without range scaling) with `/` and sqrtf() on n pseudo-random operand pairs
 * inside the range the kernels screen for; both counters must come back 0 */
int j2p_math_selftest(int device, size_t n, unsigned seed, unsigned long long *div_mismatches,
                      unsigned long long *sqrt_mismatches);

/* test hook: ONE form of the ||g|| reduction on the caller's arrays (host memory), launched with the grid, LDS size and
 * staging a solve uses for that geometry (the solver and this hook call the same launch functions).
 *   J2P_NORM_FORM_ROWSUMS       k_rowsums: in = partials [channel][tile row][strip], nch * tile_rows * ntx doubles;
 *                               rowsums_out = [tile row][channel] level-1 sums
 *   J2P_NORM_FORM_NORM_WHOLE    k_norm_whole, both levels: in = partials as above; direct form for ntx <= 48, staged
 *                               above, in as many rounds as 156 KiB of LDS make necessary; norm_out = [channel] floats
 *   J2P_NORM_FORM_NORM_FINISH   k_norm_finish: in = row sums [tile row][channel]; norm_out (ntx is ignored from here on)
 *   J2P_NORM_FORM_NORM_BANDS    k_norm_bands: in = the same global array, read as the bands [first_tile_row[b],
 *                               + band_tile_rows[b]) in the order given (any order; they must tile the rows exactly,
 *                               at most 32) — j2p_norm_selftest: as ONE band
 *   J2P_NORM_FORM_FOLD_TREE     fold_tree, the tree k_gradient's last wavefront runs   } one launch of
 *   J2P_NORM_FORM_PROJECT_TREE  norm_tree_load + norm_tree_reduce, k_project's (NIP)   } k_norm_trees_selftest
 * tile_rows <= 4096, the two in-kernel trees <= 1024 (J2P_EINVAL beyond); nch 1..3; ntx 1..529.  The output a form does
 * not write may be NULL.  fold_tile_row has no stand-alone form: it waits for partials stamped with the running
 * iteration's parity, which only k_gradient stamps — it is tested through a solver (j2p_solver_debug_partials). */
#define J2P_NORM_FORM_ROWSUMS 0
#define J2P_NORM_FORM_NORM_WHOLE 1
#define J2P_NORM_FORM_NORM_FINISH 2
#define J2P_NORM_FORM_NORM_BANDS 3
#define J2P_NORM_FORM_FOLD_TREE 4
#define J2P_NORM_FORM_PROJECT_TREE 5
int j2p_norm_selftest(int device, int form, unsigned nch, unsigned tile_rows, unsigned ntx, const double *in_host,
                      double *rowsums_out_host, float *norm_out_host);
int j2p_norm_selftest_bands(int device, int form, unsigned nch, unsigned tile_rows, unsigned ntx, const double *in_host,
                            unsigned nband, const unsigned first_tile_row[], const unsigned band_tile_rows[],
                            double *rowsums_out_host, float *norm_out_host);

/* test hook: the two packed square-root sequences of the gradient kernel against sqrtf() on EVERY
 * float in [2^-100, 2^127) (about 1.9e9 values); both counters must come back 0 */
int j2p_sqrt_exhaustive(int device, unsigned long long *rsq_mismatches, unsigned long long *fast_mismatches);

/* test hook: exhaustive checks of the SHORT division (one residual correction, j2p_kernels.hip.h: div_exact_recip).
 *   pass 3: denominators first .. first + count - 1 of the 2^23 floats of [1, 2), reciprocal by IEEE division (what
 *           phase B uses), each against all 2^23 numerator mantissas: the quotient against `/`  — all 2^23 denominators
 *           = 2^46 quotients, the proof by enumeration the kernels rely on (report[0] must be 0);
 *   pass 1: every norm phase A can meet: its reciprocal refined from the v_rsq_f32 seed by two Newton steps against
 *           1.f / n;  pass 2: radicands first .. of the 2^24 floats of [1, 4) x all numerators with THAT reciprocal —
 *           the form phase A would use; both fail exactly where theory says (norms with an all-ones mantissa), which
 *           is why phase A keeps the long form.
 * report[0] = number of mismatches, report[1..8] = the first offenders' bit patterns. */
int j2p_division_exhaustive(int device, int pass, unsigned first, unsigned count, unsigned long long report[9]);

/* Sample input: a solver from DECODED 8-bit planes — what the GPU's hardware JPEG decoder, ffmpeg (`yuvj420p`) or libjpeg's raw-data
 * mode hand over: Y, Cb, Cr at the file's own sampling — instead of the quantised coefficients only a jpeg_read_coefficients caller
 * has.  The library recomputes the coefficients from the samples on the device.
 *
 * planes[c] gives w, h, w_samp, h_samp and quant_table as for j2p_solver_create; planes[c].data and planes[c].fdata must both be NULL
 * (J2P_EINVAL otherwise: no caller shall believe they are used too).  Whole canvas only: there is no band argument.  samples[c]
 * describes channel c's 8-bit samples: `data` points into DEVICE memory of `device` or into HOST memory (hipPointerGetAttributes
 * decides; managed memory and another GPU's memory are J2P_EINVAL, as for j2p_tensor), w x h is what is present of the coefficient
 * plane (0 < w <= plane.w, 0 < h <= plane.h), and the strides are in bytes, each at least 1 (stride_x 2: one half of an interleaved
 * NV12 chroma plane).
 *
 * The definition.  For channel c and the coefficient plane's sample (X, Y), 0 <= X < plane.w, 0 <= Y < plane.h:
 *   s(X, Y) = data[min(Y, h - 1) * stride_y + min(X, w - 1) * stride_x]   — the last column and row replicated, which is how libjpeg's
 *             encoder pads and the only thing a caller who has the visible samples alone can do;
 *   v = (float)s - 128.f (exact);
 *   every 8x8 block of v goes through dct8x8s (ooura/dct.c:98-130, the transform j2p_dct8x8_blocks exposes);
 *   each coefficient is divided by (float)quant_table[j] as the correctly rounded f32 quotient, then rintf (ties to even).
 * No clamp: |v| <= 128 and the transform's basis functions have an L1 norm of at most 8, so the result lies in [-1024, 1016] by
 * construction (the +-1023 of j2p_planes_to_coefficients is libjpeg's limit for WRITING, not a property of the data).  These int16
 * values are the solver's coefficients: from there on the solver is, bit for bit, the one j2p_solver_create makes from the same
 * values with fdata == NULL — the device decode for x_0, the narrowing to bytes where they fit (j2p_solver_coefficient_bytes), the
 * wide-footprint choice.  j2p_solver_reset works as for any solver: the coefficients are resident.
 *
 * Recovery.  A decoded sample is the inverse DCT of the dequantised coefficients rounded to 8 bits, so it is off by at most 1/2, and
 * a per-sample error of at most e moves a coefficient by at most 8 * e: the quantised coefficient the file held is recovered EXACTLY
 * when its step exceeds 8 and no sample of its block was clipped at 0 or 255.  j2p_solver_clipped_samples returns how many of the
 * w x h samples present of channel c were 0 or 255 (counted by the same kernel; J2P_ESTATE for a solver not made from samples).  Where
 * that count is not 0, or a step is 8 or less, recovery is not guaranteed (measured: still exact down to steps of 5, quality 75;
 * mismatches by one step start at quality 90) — the library refuses nothing on account of it.
 *
 * Memory and ordering.  Device samples are read in place by a kernel on the solver's stream: the caller orders their producer before
 * the call (a `stream` that is the producer's, or a wait).  Host samples are staged through a buffer the solver owns anyway, one
 * hipMemcpy2DAsync per channel (of rows (w - 1) * stride_x + 1 bytes long: J2P_EINVAL when a stride_x above 4 or so makes them larger
 * than the canvas's floats).  Either way create returns after the stream has been synchronised: the samples may be reused at once.
 * Refused before a device is touched or anything is queued (J2P_EINVAL): samples or a data NULL, w or h zero or beyond the plane, a
 * stride below 1, planes[c].data or .fdata set, and everything j2p_solver_create refuses. */
typedef struct j2p_samples {
        const uint8_t *data;               /* 8-bit samples: DEVICE memory of the solver's device, or HOST memory */
        unsigned w, h;                     /* samples present: 0 < w <= plane.w, 0 < h <= plane.h */
        ptrdiff_t stride_y, stride_x;      /* in bytes, >= 1 (stride_x 2: one half of an interleaved NV12 chroma plane) */
} j2p_samples;
int j2p_solver_create_from_samples(j2p_solver **out, int device, void *stream, unsigned nchannel,
                                   const j2p_plane planes[], const j2p_samples samples[],
                                   float weight, const float pweight[], unsigned iterations);
/* diagnostics: the quantised coefficients channel c of ANY solver holds — its own block rows, block-major [rows / 8][w / 8][64],
 * natural order, as j2p_plane.data.  Waits for the solver's stream. */
int j2p_solver_download_coefficients(j2p_solver *s, unsigned c, int16_t *out_host);
int j2p_solver_clipped_samples(const j2p_solver *s, unsigned c, unsigned long long *count);
/* a batch job whose solvers are made from samples: samples[c] belongs to job->planes[c], whose data and fdata are NULL.  The samples
 * are copied and travel next to the job, never in it (j2p_job keeps its layout).  n / outs are those of j2p_batch_submit_outputs; with
 * n == 0 or outs == NULL the job's own output fields apply, so every output form a coefficient job has is available.  Device samples
 * pin the job to a worker of their GPU, as tensor outputs do (all channels' on one GPU of the batch, and the same as the output
 * tensors': J2P_EINVAL at submit otherwise, as for everything j2p_solver_create_from_samples refuses before it touches a device);
 * they must be complete when the job is submitted — the workers' streams know nothing of the caller's — and, like host samples,
 * stay valid until j2p_batch_wait.  Not with `tile`.  samples == NULL: j2p_batch_submit_outputs / j2p_batch_submit. */
int j2p_batch_submit_samples(j2p_batch *b, const j2p_job *job, const j2p_samples samples[],
                             unsigned n, const j2p_output outs[], int *ticket);

/* The JPEG file: quantised coefficients entropy-coded ON THE DEVICE, so that a complete baseline JPEG comes down instead of 2 bytes
 * per sample of coefficients for a host library to code.  The file is, byte for byte, the one libjpeg writes from the same
 * coefficients with jpeg_set_defaults, jpeg_set_colorspace, jpeg_set_quality(Q, TRUE) and jpeg_write_coefficients: default Huffman
 * tables, one scan, no restart markers (unless asked for: "Restart intervals", below), no optimisation.  This is the definition.
 *
 * Inputs.  An image of width x height (1..65535 each) with ncomp = 1 or 3 components; chroma subsampling sub_w, sub_h, each 1 or 2
 * (one component: taken as 1 whatever the fields hold).  Component 0 has bw x bh = ceil(width / 8) x ceil(height / 8) blocks,
 * components 1 and 2 ceil(bw / sub_w) x ceil(bh / sub_h) — the grids j2p_planes_to_coefficients_sub produces.  A block is 64 int16 in
 * natural order, every value in [-1023, 1023].  quant[c]: 64 steps, natural order, each 1..255 (the file is 8-bit baseline), and
 * quant[2] must hold the values of quant[1] (the file has two table slots, as libjpeg's has); J2P_EINVAL otherwise.
 *
 * Header.  Every piece is FF, the marker's byte, the big-endian 16-bit length of what follows including the length itself, the payload:
 *   1. FF D8 (alone).
 *   2. APP0 (E0): "JFIF\0" 01 01 00 00 01 00 01 00 00.
 *   3. DQT (DB): 00, then the 64 steps of table 0 in zigzag order.  Three components: a second DQT, 01 and table 1.
 *   4. SOF0 (C0): 08, height, width (16 bits each), ncomp, then per component c: its id c + 1, its sampling byte — (sub_w << 4) | sub_h
 *      for c = 0, 0x11 otherwise — and its table: 0 for c = 0, 1 otherwise.
 *   5. DHT (C4), one per Huffman table: DC0 (class/slot byte 00), AC0 (10), and for three components DC1 (01), AC1 (11); the byte, 16
 *      counts BITS, the symbols HUFFVAL.  The tables of Annex K.3 of the JPEG standard:
 *        DC0 BITS    = {0,1,5,1,1,1,1,1,1,0,0,0,0,0,0,0}         DC1 BITS = {0,3,1,1,1,1,1,1,1,1,1,0,0,0,0,0}
 *        DC0 HUFFVAL = DC1 HUFFVAL = {0,1,2,3,4,5,6,7,8,9,10,11}
 *        AC0 BITS    = {0,2,1,3,3,2,4,3,5,5,4,4,0,0,1,125}
 *        AC0 HUFFVAL = {01,02,03,00,04,11,05,12,21,31,41,06,13,51,61,07,22,71,14,32,81,91,a1,08,23,42,b1,c1,15,52,d1,f0,24,33,62,72,
 *                       82,09,0a,16,17,18,19,1a,25,26,27,28,29,2a,34,35,36,37,38,39,3a,43,44,45,46,47,48,49,4a,53,54,55,56,57,58,59,
 *                       5a,63,64,65,66,67,68,69,6a,73,74,75,76,77,78,79,7a,83,84,85,86,87,88,89,8a,92,93,94,95,96,97,98,99,9a,a2,a3,
 *                       a4,a5,a6,a7,a8,a9,aa,b2,b3,b4,b5,b6,b7,b8,b9,ba,c2,c3,c4,c5,c6,c7,c8,c9,ca,d2,d3,d4,d5,d6,d7,d8,d9,da,e1,e2,
 *                       e3,e4,e5,e6,e7,e8,e9,ea,f1,f2,f3,f4,f5,f6,f7,f8,f9,fa}   (hexadecimal)
 *        AC1 BITS    = {0,2,1,2,4,4,3,4,7,5,4,4,0,1,2,119}
 *        AC1 HUFFVAL = {00,01,02,03,11,04,05,21,31,06,12,41,51,07,61,71,13,22,32,81,08,14,42,91,a1,b1,c1,09,23,33,52,f0,15,62,72,d1,
 *                       0a,16,24,34,e1,25,f1,17,18,19,1a,26,27,28,29,2a,35,36,37,38,39,3a,43,44,45,46,47,48,49,4a,53,54,55,56,57,58,
 *                       59,5a,63,64,65,66,67,68,69,6a,73,74,75,76,77,78,79,7a,82,83,84,85,86,87,88,89,8a,92,93,94,95,96,97,98,99,9a,
 *                       a2,a3,a4,a5,a6,a7,a8,a9,aa,b2,b3,b4,b5,b6,b7,b8,b9,ba,c2,c3,c4,c5,c6,c7,c8,c9,ca,d2,d3,d4,d5,d6,d7,d8,d9,da,
 *                       e2,e3,e4,e5,e6,e7,e8,e9,ea,f2,f3,f4,f5,f6,f7,f8,f9,fa}
 *      Codes are assigned as the standard does: in order of length, consecutive within a length, doubled from one length to the next.
 *   6. SOS (DA): ncomp, per component its id and 00 for c = 0 or 11 otherwise, then 00 3F 00.
 *
 * Scan.  One component: its blocks in raster order.  Three: MCUs in raster order, ceil(bw / sub_w) x ceil(bh / sub_h) of them, each
 * component 0's sub_h x sub_w blocks (rows outer), then one block of component 1 and one of component 2.  A block position beyond
 * component 0's grid is a DUMMY block: all AC zero, DC that of the component's previous block — it codes as DC difference 0 and EOB.
 * (The first block of a component in an MCU is never a dummy.)  Per block:
 *   1. d = DC - pred[c]; pred starts at 0 and becomes this block's DC.
 *   2. The category s is the bit length of |d|: code(DC table, s), then s bits of d (d >= 0) or of d - 1 (d < 0).
 *   3. Coefficients 1..63 in zigzag order with a zero run r: for a non-zero v, while r > 15 write code(AC, 0xF0) and take 16 off r;
 *      then code(AC, (r << 4) | s) and s bits as for the DC, and r = 0.
 *   4. After the last coefficient, if r > 0: code(AC, 0x00).
 * Component 0 uses DC0 / AC0, the others DC1 / AC1.  Bits fill bytes from the highest bit down; the last byte is completed with
 * 1-bits; every FF byte of this data, that last byte included, is followed by 00.  Then FF D9.
 *
 * Output.  *size is always set to the file's size once it is known (every argument check passed).  When `capacity` is smaller —
 * out_host may then be NULL — nothing is written and the call returns J2P_ESPACE: call again with that much room.  Nothing behind
 * the file's last byte is touched. */
#define J2P_ESPACE     -5   /* the caller's output buffer is too small; the size needed has been stored */
typedef struct j2p_jpeg {
        unsigned width, height, sub_w, sub_h;
        const uint16_t *quant[3];
} j2p_jpeg;
/* The current iterate of nplane = 1 or 3 (solver, channel) pairs as that file: plane c quantised with quant[c] at the component's
 * sampling by the kernel of j2p_planes_to_coefficients_sub, into device memory; coded there; header and data copied to out_host.
 * planes[] may be one joint solver three times or three `-s` solvers on one device.  Whole-canvas solvers only (a band solver:
 * J2P_ESTATE); the argument checks of j2p_planes_to_coefficients_sub apply to every plane with its grid, and the table rules above.
 * Device memory is the scratch of planes[0].solver: a second call of the same size allocates nothing.  Synchronises, as
 * j2p_planes_to_coefficients does (twice more on the way: the sizes of the two intermediate streams are read back, 8 bytes each, so
 * that memory follows what the image needs and not the worst case). */
int j2p_planes_to_jpeg(const j2p_plane_ref planes[], unsigned nplane, const j2p_jpeg *spec, uint8_t *out_host, size_t capacity,
                       size_t *size);
/* The same coder on the caller's coefficients (host memory; coef_host[c]: component c's grid, block-major, as above) with no solver:
 * transcoding, and what the directed tests use.  A coefficient outside [-1023, 1023] is J2P_EINVAL.  Device memory comes from the
 * library's pool. */
int j2p_entropy_encode(int device, const j2p_jpeg *spec, const int16_t *const coef_host[3], unsigned ncomp, uint8_t *out_host,
                       size_t capacity, size_t *size);
/* A batch job that delivers the file (j2p_planes_to_jpeg on the worker): *spec is copied, with its tables, and travels next to the job;
 * out / size must stay valid until j2p_batch_wait, after which *size is the file's size — also when the job failed with J2P_ESPACE.
 * job->out_bits must be 0, out_coef[0] NULL and out_tensor.data NULL; not with `tile`; spec->width and height must equal job->out_w
 * and out_h; the job has 1 or 3 channels (J2P_EINVAL at submit otherwise, as for the table rules).  samples: NULL, or as for
 * j2p_batch_submit_samples.  out_planes is still honoured. */
int j2p_batch_submit_jpeg(j2p_batch *b, const j2p_job *job, const j2p_samples samples[], const j2p_jpeg *spec, uint8_t *out,
                          size_t capacity, size_t *size, int *ticket);

/* Optimised Huffman tables: the same coefficients in fewer bytes.  With J2P_JPEG_OPTIMIZE the file is, byte for byte, the one libjpeg
 * writes from the same coefficients with optimize_coding = TRUE added to the calls named above, as IJG libjpeg 9d and later do it.
 * Everything in "The JPEG file" stands except item 5 of the header and the codes used in the scan.  This is the definition.
 *
 * Counts.  One array of 256 counts per table: DC0 and AC0 from component 0, DC1 and AC1 from components 1 and 2 together.  The scan is
 * walked exactly as it is coded, dummy blocks included.  Per block: count[s]++ for the category s of the DC difference; per non-zero AC
 * coefficient with a zero run r in front, count[0xF0] += r >> 4 and count[((r & 15) << 4) | s]++; count[0x00]++ when the block ends
 * in a zero run.  (A dummy block counts DC symbol 0 and AC symbol 0x00.)
 * Lengths, per table.  freq[0..255] = count and freq[256] = 1, a pseudo-symbol that keeps the all-ones code unused; codesize[] = 0,
 * others[] = -1.  Repeat: c1 is the index of the smallest non-zero freq, on a tie the LARGEST index (scan upwards with <=); c2 the same
 * among the rest; stop when there is no c2; freq[c1] += freq[c2], freq[c2] = 0; add 1 to codesize of c1 and of everything on its others
 * chain, append c2 to the end of that chain, add 1 to codesize of c2 and of its chain.  bits[n] is the number of symbols (256 included)
 * with codesize == n, n up to 32.  For i = 32 down to 17, while bits[i] > 0: j = i - 2, lowered while bits[j] == 0; bits[i] -= 2,
 * bits[i - 1] += 1, bits[j + 1] += 2, bits[j] -= 1.  With i the largest length <= 16 that has bits[i] > 0: bits[i] -= 1, which removes
 * the pseudo-symbol.
 * Symbols.  HUFFVAL is the symbols with a non-zero count, ordered by count descending and then by symbol value ascending; BITS[1..16]
 * deals the lengths out to them in that order.  (Older libjpegs — 6b to 9c — and libjpeg-turbo order the symbols of one length by
 * value instead: their files decode to the same coefficients, differ in bytes and are a few bytes larger.)
 * Codes.  As for every table: in order of length, consecutive within a length, doubled from one length to the next.
 * DHT.  DC0, AC0, and for three components DC1, AC1, in that order: the class/slot byte, 16 BITS, HUFFVAL at its true length.  The
 * header is never longer than with the default tables: a table holds at most 12 DC or 162 AC symbols.
 * Refusal.  A count above 1 000 000 000 is J2P_ENOTSUP before anything is written: libjpeg's own search for the rarest symbols starts
 * from that value and is undefined beyond it (a table needs more than 10^9 pixels to get there).  So is a tree with a code longer than
 * 32 bits before limiting, which libjpeg dies on (more than five million blocks whose symbol counts grow like Fibonacci numbers).
 *
 * The counts are taken on the device (k_entropy_histogram) and read back, 2 x 268 64-bit counters: a third wait on the way, next to
 * the two of j2p_planes_to_jpeg.  The tables are made on the host between two launches.  Without the flag nothing of this happens:
 * the launches, the memory and the bytes of "The JPEG file".  Unknown flag bits: J2P_EINVAL.  (The three _ex calls: shorthands, see
 * j2p_jpeg_options.) */
#define J2P_JPEG_OPTIMIZE 1u
int j2p_planes_to_jpeg_ex(const j2p_plane_ref planes[], unsigned nplane, const j2p_jpeg *spec, uint8_t *out_host, size_t capacity,
                          size_t *size, unsigned flags);
/* What the coder saw of one file (stats may be NULL): the four count arrays above — taken on the device whether or not the flag is set,
 * so that a test sees the kernel's counts themselves and not only a file they happen not to change — the bits of the scan before
 * padding and stuffing, and the FF bytes that were stuffed.  Zeroed first; the counts are there once they have been read back, also
 * when the call then fails with J2P_ESPACE. */
typedef struct j2p_encode_stats {
        unsigned long long dc0[256], ac0[256], dc1[256], ac1[256];
        unsigned long long scan_bits, stuffed_bytes;
} j2p_encode_stats;
int j2p_entropy_encode_ex(int device, const j2p_jpeg *spec, const int16_t *const coef_host[3], unsigned ncomp, uint8_t *out_host,
                          size_t capacity, size_t *size, unsigned flags, j2p_encode_stats *stats);
int j2p_batch_submit_jpeg_ex(j2p_batch *b, const j2p_job *job, const j2p_samples samples[], const j2p_jpeg *spec, uint8_t *out,
                             size_t capacity, size_t *size, unsigned flags, int *ticket);

/* The progressive JPEG file: the same coefficients as the ten scans (six for one component) of libjpeg's jpeg_simple_progression(),
 * coded on the device.  The file is, byte for byte, the one libjpeg (IJG 9d and later) writes from the same coefficients with
 * jpeg_simple_progression() added to the calls named under "Optimised Huffman tables" — libjpeg forces optimize_coding in progressive
 * mode, so every Huffman-coded scan carries tables made from that scan's own symbol counts, by the rules given there ("Lengths",
 * "Symbols", "Codes", "Refusal").  Inputs and output are those of "The JPEG file".  No other scan script is offered.  This is the
 * definition; where the wording below and libjpeg differ, libjpeg's output is the authority.
 *
 * Scans, each (components; Ss-Se; Ah, Al).  Three components:
 *    1. (0,1,2; 0-0; 0,1)    2. (0; 1-5; 0,2)    3. (2; 1-63; 0,1)    4. (1; 1-63; 0,1)    5. (0; 6-63; 0,2)
 *    6. (0; 1-63; 2,1)       7. (0,1,2; 0-0; 1,0)    8. (2; 1-63; 1,0)    9. (1; 1-63; 1,0)   10. (0; 1-63; 1,0)
 * One component:
 *    1. (0; 0-0; 0,1)    2. (0; 1-5; 0,2)    3. (0; 6-63; 0,2)    4. (0; 1-63; 2,1)    5. (0; 0-0; 1,0)    6. (0; 1-63; 1,0)
 *
 * File.  Items 1 to 3 of the header of "The JPEG file"; the frame header of item 4 with marker SOF2 (C2) in place of SOF0; then per
 * scan its DHT segments, its SOS and its data; then FF D9.
 *   DHT.  One segment per table the scan uses, made from the scan's own counts: for each component of the scan in order, its DC table
 *   if the scan is a DC first scan (Ss = 0, Ah = 0) and then its AC table if Se > 0, a table once.  Component 0 uses slots DC0 / AC0,
 *   the others DC1 / AC1.  So scan 1 of three components carries DC0 then DC1, an AC scan its one AC table (class/slot byte 10 for
 *   component 0, 11 otherwise), a DC refinement scan none.
 *   SOS (DA).  The number of components, per component its id c + 1 and the byte (Td << 4) | Ta — Td the DC slot in a DC first scan
 *   and 0 otherwise, Ta the AC slot when Se > 0 and 0 otherwise — then Ss, Se, (Ah << 4) | Al.
 *   Data.  Each scan's bits fill bytes from the highest bit down, the scan's last byte is completed with 1-bits, and every FF byte of
 *   the scan's data is followed by 00 — per scan, on its own.
 *
 * Geometry.  A DC scan of three components walks the MCUs exactly as the scan of "The JPEG file" does, dummy blocks included; of one
 * component, its blocks in raster order.  A dummy block holds the DC of the component's previous block in the scan.  An AC scan walks
 * its one component's own block grid in raster order, without dummy blocks.
 *
 * Coding, per scan kind (code(s): the scan's table for the component; >> on a DC is an arithmetic shift):
 *   DC first.  v = DC >> Al; d = v - pred[c], pred from 0, becoming v; category s = bit length of |d|; code(s), then s bits of d
 *   (d >= 0) or of d - 1.  A dummy block codes d = 0.
 *   DC refinement.  One raw bit per position: (DC >> Al) & 1 — for a dummy block its predecessor's bit, not 0.
 *   AC first.  For k = Ss..Se in zigzag order, t = |c| >> Al (the shift applies to the absolute value: +-1 at Al = 1 is zero).  A zero
 *   lengthens the run r.  A non-zero t first flushes a pending EOB run; then while r > 15: code(0xF0), r -= 16; then
 *   code((r << 4) | s) with s the bit length of t, and s bits: t, or ~t for a negative coefficient; r = 0.  A block that ends with
 *   r > 0 adds 1 to EOBRUN, which is flushed when it reaches 0x7FFF and at the end of the scan.  A flush of EOBRUN > 0 is
 *   code(n << 4) with n = floor(log2(EOBRUN)) followed by the low n bits of EOBRUN.
 *   AC refinement.  t = |c| >> Al; EOB is the position of the block's last t == 1 (0 if none); r = 0 and an empty buffer of correction
 *   bits per block.  For k = Ss..Se: a zero t lengthens r.  Otherwise: while r > 15 and k <= EOB — flush the pending EOB run,
 *   code(0xF0), r -= 16, emit and empty the buffer.  Then if t > 1, buffer the bit t & 1; if t == 1, flush the pending EOB run,
 *   code((r << 4) | 1), one sign bit (1 for a positive coefficient), emit and empty the buffer, r = 0.  After the block, if r > 0 or
 *   the buffer is not empty: EOBRUN += 1 and the buffered bits join the run's own buffer; the run is flushed when EOBRUN == 0x7FFF or
 *   when its buffer holds MORE than 937 bits (libjpeg's 1000 - 64 + 1).  A flush is the EOBn symbol and its extra bits as above, then
 *   the run's buffered bits in order.  The end of the scan flushes.
 *
 * Refusals.  Those of the optimised tables (a count above 10^9, a tree deeper than 32: J2P_ENOTSUP).  A coefficient whose shifted
 * magnitude needs more than 10 bits cannot come from values in [-1023, 1023]; a table that holds such a symbol is refused as the
 * baseline coder refuses it (J2P_EINVAL, "outside [-1023, 1023]").
 *
 * On the device the symbols of ALL scans are counted first and read back with one wait; the host makes every table (2 DC and 7 AC for
 * three components, 1 DC and 3 AC for one); every scan's bits and stuffed FF bytes come back as arrays with one wait each.  So a file
 * costs the waits of the optimised call, whatever the number of scans.  Progressive is a member of j2p_jpeg_options and no flag: the
 * _ex calls keep refusing every flag bit but J2P_JPEG_OPTIMIZE.  (The _progressive calls: shorthands, see j2p_jpeg_options.) */
#define J2P_PROGRESSIVE_SCANS 10
typedef struct j2p_progressive_scan {
        unsigned ncomp, comp[3];        /* the scan's components */
        unsigned ss, se, ah, al;
        unsigned ntables, table[2];     /* the tables it carries, in DHT order: (class << 4) | slot */
        unsigned long long counts[2][256];      /* ... and their symbol counts as taken on the device */
        unsigned long long bits;                /* of the scan's data before padding and stuffing */
        unsigned long long stuffed_bytes;       /* FF bytes that got their 00 */
        unsigned long long eob_runs;            /* EOB runs flushed (AC scans) */
} j2p_progressive_scan;
typedef struct j2p_progressive_stats {
        unsigned nscans;
        j2p_progressive_scan scan[J2P_PROGRESSIVE_SCANS];
} j2p_progressive_stats;
int j2p_planes_to_jpeg_progressive(const j2p_plane_ref planes[], unsigned nplane, const j2p_jpeg *spec, uint8_t *out_host, size_t capacity,
                                   size_t *size);
/* stats may be NULL; zeroed first; the counts are there once they have been read back, the bits and stuffed bytes once those have,
 * also when the call then fails with J2P_ESPACE. */
int j2p_entropy_encode_progressive(int device, const j2p_jpeg *spec, const int16_t *const coef_host[3], unsigned ncomp, uint8_t *out_host,
                                   size_t capacity, size_t *size, j2p_progressive_stats *stats);
int j2p_batch_submit_jpeg_progressive(j2p_batch *b, const j2p_job *job, const j2p_samples samples[], const j2p_jpeg *spec, uint8_t *out,
                                      size_t capacity, size_t *size, int *ticket);

/* Restart intervals: any of the three files above with RSTn markers in its scans, which make a file robust to damage and let a
 * parallel decoder — this library's own first of all — split every scan.  With restarts the file is, byte for byte, the one libjpeg
 * (IJG 9d) writes with the calls named under "The JPEG file", "Optimised Huffman tables" and "The progressive JPEG file" and, before
 * jpeg_write_coefficients, cinfo.restart_interval = N or cinfo.restart_in_rows = R.  This is the definition; where the wording below
 * and libjpeg differ, libjpeg's output is the authority.
 *
 * Units.  An interleaved scan — the baseline scan of three components, a progressive DC scan of three components — counts MCUs.  A
 * scan of one component — every AC scan, every scan of a one-component file — counts that component's blocks in raster order.
 * restart_interval = N (1..65535) is the interval of every scan.  restart_in_rows = R (1..65535) sets a scan's interval to
 * min(R x units per row of that scan, 65535), units per row being the MCUs per row of an interleaved scan and the component's
 * blocks per row of a one-component scan: the interval changes between the scans of a subsampled progressive file.
 * DRI.  A DRI segment (FF DD 00 04, the interval as 16 bits) stands behind the scan's DHT segments and immediately in front of its
 * SOS, and only where the interval differs from the one last written, which starts at 0 — also when the interval holds the whole scan
 * and no marker follows.  A 40x24 4:2:0 progressive file with R = 1 has DRI 3 in front of scans 1, 3, 7 and DRI 5 in front of scans
 * 2, 5 and 10; with N = 3 one DRI, in front of scan 1.
 * Intervals.  Behind every interval but the scan's last: a pending EOB run is flushed (its EOBn symbol, its extra bits, then its
 * waiting correction bits); the last byte is completed with 1-bits; every FF of the data, one made by that padding included, is
 * followed by 00; then FF D0+(k mod 8) for the k-th marker of the scan, counted from 0 per scan, not stuffed.  The DC predictors
 * restart at 0; an interval of a DC refinement scan is its bits padded to a byte.  An EOB run never spans a marker; the cuts at 32767
 * blocks and 937 correction bits apply within an interval as before.
 * Counts.  With tables made for the image the symbol counts are those of the scan as coded: DC categories follow the reset
 * predictors, and there is one EOBn per flush, the flushes at interval ends included.
 * Refusals.  J2P_EINVAL for N or R above 65535 and for both non-zero; everything the three coders refuse without restarts.
 *
 * On the device the restart plan is pure host arithmetic (j2p_debug_restart_plan shows it).  Every interval starts on a byte, so its
 * pad is (-its bits) mod 8 and is known from the unpadded bit offsets: a lane per interval adds it to the length of the interval's last
 * item, the exclusive sum runs once more, and the lane or wavefront of every interval's last item writes the 1-bits.  The staging
 * stream stays pure data; the markers go in where the FFs are stuffed.  No wait is added: a file costs the waits it cost.
 *
 * The options record: the description of a JPEG write.  flags: J2P_JPEG_* bits; progressive: 0 or 1 (flags then change nothing);
 * restart_interval, restart_in_rows: 0 for none.  The four j2p_*_opt calls below take it and are the calls every JPEG write goes
 * through; it is the one thing that travels from them to the coder (a batch copies it into the job's record next to the copied spec,
 * not into j2p_job).  A member that is 0 costs nothing: {0, 0, 0, 0} has the launches, the memory and the bytes of "The JPEG file".
 * Refusals, after a NULL argument and before anything else of the call is looked at (a batch job: after the job's own rules and
 * the spec's): NULL options, unknown flag bits, progressive above 1, the restart members as above — all J2P_EINVAL.
 * The twelve older calls are shorthands, each for the _opt call of its name with the record
 *      j2p_planes_to_jpeg, j2p_entropy_encode, j2p_batch_submit_jpeg, j2p_batch_submit_file_jpeg                       {0, 0, 0, 0}
 *      ..._ex(flags) of the four                                                                                       {flags, 0, 0, 0}
 *      ..._progressive of the four                                                                                     {0, 1, 0, 0}
 * and, for j2p_entropy_encode_ex and j2p_entropy_encode_progressive, their stats as stats / progressive_stats.  Every rule of the
 * _opt call is theirs; they keep their signatures and refuse what they refused. */
typedef struct j2p_jpeg_options {
        unsigned flags;
        unsigned progressive;
        unsigned restart_interval;
        unsigned restart_in_rows;
} j2p_jpeg_options;
/* one scan of the restart plan: its units, the units in a row, its interval (0: none), the number of intervals (1 without) and
 * whether a DRI segment precedes its SOS */
typedef struct j2p_restart_scan {
        unsigned units, units_per_row, interval, intervals, dri;
} j2p_restart_scan;
typedef struct j2p_restart_plan {
        unsigned nscans;        /* 1 for a baseline file */
        j2p_restart_scan scan[J2P_PROGRESSIVE_SCANS];
} j2p_restart_plan;
/* Test hook, needs no device: the plan of the file of width x height pixels with ncomp components and sub_w x sub_h blocks of component
 * 0 in an MCU.  J2P_EINVAL for options the coders refuse. */
int j2p_debug_restart_plan(unsigned width, unsigned height, unsigned ncomp, unsigned sub_w, unsigned sub_h, const j2p_jpeg_options *options,
                           j2p_restart_plan *plan);
/* what the coder did per scan, as taken on the device: the interval and the number of intervals, the 1-bits that completed the
 * intervals' last bytes (the scan's last included) and the RSTn markers written */
typedef struct j2p_restart_scan_stats {
        unsigned interval, intervals;
        unsigned long long padding_bits, markers;
} j2p_restart_scan_stats;
typedef struct j2p_restart_stats {
        unsigned nscans;
        j2p_restart_scan_stats scan[J2P_PROGRESSIVE_SCANS];
} j2p_restart_stats;
/* the planes of "The JPEG file" as the file of `options` */
int j2p_planes_to_jpeg_opt(const j2p_plane_ref planes[], unsigned nplane, const j2p_jpeg *spec, uint8_t *out_host, size_t capacity,
                           size_t *size, const j2p_jpeg_options *options);
/* ... and the caller's coefficients.  stats is filled by the baseline and optimised coders, progressive_stats by the progressive one
 * (its `bits` are those before any padding), restart_stats by all; each may be NULL and is zeroed first.  Asking for stats has the
 * baseline coder count the symbols (one more wait), as J2P_JPEG_OPTIMIZE does. */
int j2p_entropy_encode_opt(int device, const j2p_jpeg *spec, const int16_t *const coef_host[3], unsigned ncomp, uint8_t *out_host,
                           size_t capacity, size_t *size, const j2p_jpeg_options *options, j2p_encode_stats *stats,
                           j2p_progressive_stats *progressive_stats, j2p_restart_stats *restart_stats);
/* ... and a batch job's image, from its coefficients or samples (rules: j2p_batch_submit_jpeg) or from a file (rules:
 * j2p_batch_submit_file_jpeg). */
int j2p_batch_submit_jpeg_opt(j2p_batch *b, const j2p_job *job, const j2p_samples samples[], const j2p_jpeg *spec, uint8_t *out,
                              size_t capacity, size_t *size, const j2p_jpeg_options *options, int *ticket);
int j2p_batch_submit_file_jpeg_opt(j2p_batch *b, const j2p_job *job, const uint8_t *file, size_t size, const j2p_jpeg *spec, uint8_t *out,
                                   size_t capacity, size_t *out_size, const j2p_jpeg_options *options, int *ticket);

/* Reading a JPEG file: the entropy-coded data of a baseline file Huffman-decoded ON THE DEVICE, so that a caller without libjpeg
 * gets the file's true quantised coefficients at every quality.  For each component the result is the grid of whole blocks
 * blocks_w x blocks_h of j2p_jpeg_info, block-major, 64 int16 in natural order — value for value what libjpeg's
 * jpeg_read_coefficients delivers for the file.  This is the definition.
 *
 * Accepted.  SOF0 or SOF1 with 8-bit samples; Huffman coding; 1 or 3 components with sampling factors 1..4 and at most 10 blocks in
 * an MCU; ONE scan that holds all components in the frame's order (Ss 0, Se 63, Ah/Al 0); any number of DQT (8- or 16-bit entries,
 * slots 0..3) and DHT (slots 0..3) segments before the scan; DRI with RST0..7; fill bytes (FF FF) before markers; anything behind EOI.
 *
 * Markers.  FF D8, then segments: FF, the marker's byte, a big-endian 16-bit length that counts itself, the payload.
 *   DQT (DB)  repeated: a byte (precision << 4) | slot, then 64 entries of 1 byte (precision 0) or 2 (precision 1) in zigzag order.
 *   DHT (C4)  repeated: a byte (class << 4) | slot (class 0 DC, 1 AC), 16 counts BITS, then their sum symbols HUFFVAL.
 *   SOF (C0, C1)  08, height, width (16 bits each), ncomp, per component: id, (h << 4) | v, quantisation slot.
 *   DRI (DD)  the restart interval in MCUs, 16 bits; 0 switches restarts off.
 *   SOS (DA)  ncomp, per component: id, (DC slot << 4) | AC slot; then 00 3F 00.  The entropy-coded data follows and ends at the
 *             first FF whose next byte is none of 00, FF, D0..D7.  That marker must be EOI (D9), perhaps behind further segments.
 * Codes.  As the standard assigns them: in order of length, consecutive within a length, doubled from one length to the next.  A
 * table whose codes do not fit their lengths, or a DC table with a symbol above 15, is J2P_EFORMAT.
 * Grids.  hmax, vmax: the largest factors.  Component c has ceil(ceil(width * h_c / hmax) / 8) x ceil(ceil(height * v_c / vmax) / 8)
 * blocks.  One component: its blocks in raster order, an MCU is one block.  Three: ceil(width / (8 hmax)) x ceil(height / (8 vmax))
 * MCUs in raster order, each component 0's v_0 x h_0 blocks (rows outer), then component 1's, then component 2's.  Blocks that pad a
 * component's grid out to whole MCUs are decoded — their DC differences are links of the predictor chain — and not delivered.
 * Block.  Bits are taken from the highest bit of each byte down.  A DC symbol s (0..15), then s bits v; an AC symbol (r << 4) | s:
 * s = 0 and r = 15 skips 16 coefficients, any other s = 0 ends the block (the rest is zero), otherwise r zeros are skipped and s bits
 * v give the coefficient at the next zigzag position.  Value extension: v < 2^(s-1) stands for v - (2^s - 1).  The DC is the
 * difference plus the component's previous DC in scan order, 0 at the start of the scan and of every restart interval.
 * Restarts.  With an interval of R MCUs, every R MCUs but the last are followed by 1-bits up to the byte boundary and the marker FF Dn,
 * n counting 0..7 and round again; the DC predictors are 0 behind it.  Unstuffing: FF 00 is the data byte FF; FF FF is a fill byte.
 *
 * Refusals, with nothing delivered and nothing created.  J2P_EFORMAT: what libjpeg would warn about or die on — a truncated scan, a
 * code in no table, a run past coefficient 63, a restart marker missing or out of sequence, a table the scan names that was never
 * defined, a DC value outside int16, blocks missing or bytes left over when the data ends, a damaged segment.  J2P_ENOTSUP: valid
 * files this decoder does not read — progressive, arithmetic, lossless or hierarchical coding, 12-bit samples, 2 or 4 components,
 * several scans, a scan out of the frame's component order, DNL.  What the marker segments alone show is refused before a device is
 * touched (j2p_jpeg_parse refuses exactly that, and touches nothing): no device is selected, nothing is allocated on one and nothing
 * is queued.  The calls that take a file in either kind of memory ask the runtime what kind it is first (as sample input does), and a
 * file in device memory is copied down for the parse.  Data too short for the frame's blocks (two bits each) and restart markers (two
 * bytes each) counts as truncated: a file's claimed size alone makes the library allocate nothing. */
#define J2P_EFORMAT    -6   /* the JPEG file is damaged                                        */
#define J2P_ENOTSUP    -7   /* the JPEG file is valid, and of a kind this decoder does not read */
typedef struct j2p_jpeg_component {
        unsigned id, h_samp_factor, v_samp_factor;
        unsigned blocks_w, blocks_h;       /* the delivered grid: the coefficient plane is blocks_w * 8 x blocks_h * 8 */
        unsigned w_samp, h_samp;           /* hmax / h_samp_factor, vmax / v_samp_factor: j2p_plane's w_samp, h_samp */
        unsigned quant_slot, dc_slot, ac_slot;
        uint16_t quant[64];                /* the component's quantisation table, natural order */
} j2p_jpeg_component;
typedef struct j2p_jpeg_info {
        unsigned width, height, ncomp;
        unsigned extended;                 /* 1: SOF1 */
        j2p_jpeg_component comp[3];
        unsigned mcus_w, mcus_h, blocks_per_mcu;
        unsigned restart_interval;         /* MCUs, 0: none */
        unsigned intervals;                /* restart intervals in the scan (1 without restarts) */
        size_t scan_begin, scan_end;       /* the entropy-coded data: file[scan_begin, scan_end) */
} j2p_jpeg_info;
/* Host only: the marker segments of the file -> *info (zeroed on failure).  What a caller needs to allocate with. */
int j2p_jpeg_parse(const uint8_t *file, size_t size, j2p_jpeg_info *info);
/* The file's coefficients on the host, no solver involved: the mirror of j2p_entropy_encode.  file: HOST memory, or DEVICE memory of
 * `device` (its entropy-coded data is read in place; the file is copied down once for the host's parse; any other kind of memory is
 * J2P_EINVAL, as for j2p_samples).
 * coef_host[c]: room for comp[c].blocks_w * blocks_h * 64 values — untouched unless the call returns J2P_OK.  quant (may be NULL):
 * receives the components' tables.  info (may be NULL): as j2p_jpeg_parse.  Device memory comes from the library's pool. */
int j2p_entropy_decode(int device, const uint8_t *file, size_t size, int16_t *const coef_host[3], uint16_t quant[3][64],
                       j2p_jpeg_info *info);
/* The same with the subsequence length in bits given (0: the default, J2P_DECODE_SUBSEQUENCE_BITS; otherwise
 * J2P_DECODE_SUBSEQUENCE_MIN..MAX, any value in between, J2P_EINVAL outside) and statistics returned (stats may be NULL).  The
 * result does not depend on the length; the test hook that makes an image of a few blocks cross every boundary. */
#define J2P_DECODE_SUBSEQUENCE_BITS 1024u
#define J2P_DECODE_SUBSEQUENCE_MIN 32u     /* longer than the longest symbol the kernels read (16 + 15 bits) */
#define J2P_DECODE_SUBSEQUENCE_MAX 65536u
#define J2P_DECODE_STATS_ROUNDS 16
typedef struct j2p_decode_stats {
        unsigned subsequences;             /* in the whole scan */
        unsigned intervals;                /* restart intervals */
        unsigned rounds;                   /* rounds in which a subsequence's entry state changed, the first included */
        unsigned recomputed[J2P_DECODE_STATS_ROUNDS];   /* subsequences decoded again in round r (the first 16 rounds) */
        unsigned long long data_bytes;     /* the entropy-coded data without stuffing and markers */
        double decode_ms;                  /* host clock around the decode alone: the data's way up, every kernel, the read-backs of the
                                              rounds — not the coefficients' way down */
} j2p_decode_stats;
int j2p_entropy_decode_ex(int device, const uint8_t *file, size_t size, int16_t *const coef_host[3], uint16_t quant[3][64],
                          j2p_jpeg_info *info, unsigned subsequence_bits, j2p_decode_stats *stats);
/* A whole-canvas solver of the file's 1 or 3 components (one: the greyscale solver), its coefficients decoded on the device straight
 * into the solver's resident coefficient buffers: from there on, bit for bit, the solver j2p_solver_create makes from the same
 * coefficients with fdata == NULL.  file as for j2p_entropy_decode; pweight: one per component.  A refused file creates nothing. */
int j2p_solver_create_from_jpeg(j2p_solver **out, int device, void *stream, const uint8_t *file, size_t size, float weight,
                                const float pweight[], unsigned iterations, j2p_jpeg_info *info);
/* A batch job whose solvers are made from a file: file / size are the file's bytes — HOST memory, or DEVICE memory of a GPU of the
 * batch, which pins the job to a worker of that GPU as device samples do — and stay valid until j2p_batch_wait; they are not copied
 * (a device file is copied down once, at submit, for the parse).  The marker segments are read at submit, on the caller's thread:
 * what they show is refused there (J2P_EFORMAT, J2P_ENOTSUP) and no ticket is given; what only the data shows fails the job
 * (j2p_batch_wait returns J2P_EFORMAT) and no other.  The worker decodes the scan once on its GPU and makes every solver of the job
 * from that — the joint solve, the three of `separate`, or component 0 alone.  job->planes[c] carry no data (data and fdata NULL):
 * w and h, where set, must be the file's component's; w_samp and h_samp left zero are the file's (a zooming caller gives the file's
 * times the zoom); quant_table is ignored, the file's is used; nchannel 0 means the file's component count, otherwise it must be that
 * count, or 1 for component 0 of a three-component file; out_w and out_h left zero are the file's width and height.  n / outs are
 * those of j2p_batch_submit_outputs; with n == 0 or outs == NULL the job's own output fields apply, so every output form a
 * coefficient job has is available.  Not with `tile` (J2P_EINVAL). */
int j2p_batch_submit_file(j2p_batch *b, const j2p_job *job, const uint8_t *file, size_t size, unsigned n, const j2p_output outs[],
                          int *ticket);
/* File in and file out in one job: the solvers from `file` as above, the result as the JPEG file of j2p_batch_submit_jpeg (spec, out,
 * capacity, out_size and the job's rules as there).  Bytes go in and bytes come out; no coefficient crosses the bus. */
int j2p_batch_submit_file_jpeg(j2p_batch *b, const j2p_job *job, const uint8_t *file, size_t size, const j2p_jpeg *spec, uint8_t *out,
                               size_t capacity, size_t *out_size, int *ticket);
/* (shorthands, see j2p_jpeg_options) */
int j2p_batch_submit_file_jpeg_ex(j2p_batch *b, const j2p_job *job, const uint8_t *file, size_t size, const j2p_jpeg *spec, uint8_t *out,
                                  size_t capacity, size_t *out_size, unsigned flags, int *ticket);
int j2p_batch_submit_file_jpeg_progressive(j2p_batch *b, const j2p_job *job, const uint8_t *file, size_t size, const j2p_jpeg *spec,
                                           uint8_t *out, size_t capacity, size_t *out_size, int *ticket);

/* Reading a progressive JPEG file: every scan of an SOF2 file decoded ON THE DEVICE.  The result is, for each component, the
 * blocks_w x blocks_h grid of "Reading a JPEG file", value for value what libjpeg's jpeg_read_coefficients delivers for the file;
 * where this wording and libjpeg differ on a file libjpeg reads without a warning, libjpeg is the authority.  The calls of
 * "Reading a JPEG file" keep refusing SOF2 with J2P_ENOTSUP; the calls below are the way in.  This is the definition.
 *
 * Accepted.  SOF2, 8-bit samples, Huffman coding, 1 or 3 components with the sampling limits of the baseline reader; up to
 * J2P_DECODE_SCANS_MAX scans (more: J2P_ENOTSUP); DHT and DRI segments between scans — a scan uses the tables and the restart interval
 * in force at its SOS, so every scan carries its own snapshot of them (at most J2P_SCAN_TABLES_MAX table definitions in a file, more:
 * J2P_ENOTSUP); DQT only before the first SOS (a later one: J2P_ENOTSUP).  A single-scan SOF0 / SOF1 file is decoded by the path of
 * "Reading a JPEG file", unchanged; a multi-scan SOF0 / SOF1 file stays J2P_ENOTSUP.
 *
 * Scans (T.81 G.1.1.1.1).  SOS: ncomp, per component id and (DC slot << 4) | AC slot, then Ss, Se, (Ah << 4) | Al.
 *   Ss = 0 implies Se = 0: a DC scan of 1..ncomp components in the frame's order.  Ss > 0 implies one component and Ss <= Se <= 63.
 *   Al <= 13; Ah is 0 or Al + 1.  For each (component, coefficient) the first scan that covers it has Ah = 0 and every later one has Ah
 *   equal to the Al before it (so a coefficient has ONE first scan).  A component's AC scans come behind its DC first scan.  Anything
 *   else is a bogus progression, J2P_EFORMAT.  A script that ends before Al reaches 0 is valid: the values stay shifted, as libjpeg
 *   leaves them; a coefficient no scan covers stays 0.
 * Geometry.  A scan of several components walks the MCUs of "Reading a JPEG file" restricted to its components, the blocks that pad
 *   the grids included; its restart interval counts MCUs.  A scan of one component, DC or AC, walks that component's own
 *   blocks_w x blocks_h grid in raster order; its restart interval counts blocks.
 * Decoding.  Symbols, value extension, unstuffing and restart markers as in "Reading a JPEG file".
 *   DC first (Ah = 0).  A symbol s, s bits, extended, added to the component's predictor (0 at the start of the scan and of every
 *     restart interval); coefficient 0 becomes predictor << Al.
 *   DC refinement.  One bit per block position, padding blocks included: coefficient 0 |= bit << Al.
 *   AC first.  From k = Ss.  Symbol (r << 4) | s: s = 0, r = 15 skips 16 positions; s = 0, r < 15 is EOBn — this block from k on and
 *     the next (1 << r) + (r extra bits) - 1 blocks hold nothing in the band; otherwise k += r, s bits extended give the value v, the
 *     coefficient at zigzag k becomes v << Al (kept to 16 bits), k += 1.  The block is done when k passes Se.
 *   AC refinement.  libjpeg's decode_mcu_AC_refine.  From k = Ss.  Symbol (r << 4) | s with s 0 or 1; s = 1 is followed by a sign bit:
 *     the new coefficient is +(1 << Al) for 1, -(1 << Al) for 0.  EOBn as above.  Otherwise the walk goes on from k past r coefficients
 *     that were zero when the scan began, up to the next such one, k', where the new coefficient goes (nowhere for 15/0), and k = k' + 1.
 *     Every coefficient already non-zero that is passed — on the way to k', behind an EOBn to the band's end, in every block of an EOB
 *     run over the whole band — reads one correction bit, in zigzag order, behind the symbol's own bits: a 1 adds (1 << Al) away
 *     from zero when that bit of the coefficient is still clear.
 *   A restart marker resets the predictors and must not fall inside an EOB run.
 * Refusals.  J2P_EFORMAT: a truncated scan, a code in no table, a run past Se, an EOB run past the last block of its restart
 *   interval, s > 1 in a refinement scan, a DC that does not fit int16 with its shift, bytes left over behind a scan's or an
 *   interval's last block, a restart marker missing or out of sequence, a bogus progression, a table a scan needs that is not defined.
 *   What the marker segments alone show is refused before a device is touched, as for "Reading a JPEG file".  Per scan the data must hold
 *   a bit for every block of a DC scan, a bit for every 32767 blocks of an AC scan and two bytes for every restart marker, or the scan
 *   counts as truncated: a claimed size alone makes the library allocate nothing. */
#define J2P_DECODE_SCANS_MAX 128
#define J2P_SCAN_TABLES_MAX 392
typedef struct j2p_jpeg_scan {
        unsigned ncomp;                    /* components in the scan */
        unsigned comp[3];                  /* ... as indices into j2p_jpeg_info.comp, ascending */
        unsigned ss, se, ah, al;
        unsigned dc_slot[3], ac_slot[3];   /* as the SOS names them, per component of the scan */
        unsigned restart_interval;         /* in force at the SOS: MCUs (several components) or blocks (one); 0: none */
        unsigned intervals;                /* restart intervals in the scan */
        size_t begin, end;                 /* the scan's entropy-coded data: file[begin, end) */
} j2p_jpeg_scan;
typedef struct j2p_jpeg_scans {
        unsigned nscans;
        unsigned progressive;              /* 1: SOF2.  0: a sequential file, one scan, decoded as "Reading a JPEG file" says */
        j2p_jpeg_scan scan[J2P_DECODE_SCANS_MAX];
} j2p_jpeg_scans;
/* Host only: j2p_jpeg_parse for the files accepted above (both zeroed on failure).  info keeps its layout: scan_begin is the first scan's
 * begin, scan_end the last scan's end, restart_interval the value in force at the first scan, intervals the sum over the scans; a
 * component's dc_slot / ac_slot are those of its first DC / AC scan. */
int j2p_jpeg_parse_scans(const uint8_t *file, size_t size, j2p_jpeg_info *info, j2p_jpeg_scans *scans);
typedef struct j2p_scans_stats {
        unsigned scans;
        unsigned dc_first, ac_first, dc_refine, ac_refine;     /* scans of each kind */
        unsigned subsequences;             /* of all first scans together: they share one array and the same rounds */
        unsigned rounds;                   /* rounds in which a subsequence's entry state changed */
        unsigned host_waits;               /* times the host waited for the stream during the decode */
        unsigned long long data_bytes;     /* the scans' entropy-coded data as the file holds it */
        double decode_ms;                  /* host clock around the decode alone, as in j2p_decode_stats */
        double ac_refine_share;            /* of decode_ms: the AC refinement launches, by events around them (0 without such scans) */
} j2p_scans_stats;
/* j2p_entropy_decode_ex for the files accepted above; file, coef_host, quant, info and subsequence_bits as there.  stats may be NULL. */
int j2p_entropy_decode_scans(int device, const uint8_t *file, size_t size, int16_t *const coef_host[3], uint16_t quant[3][64],
                             j2p_jpeg_info *info, unsigned subsequence_bits, j2p_scans_stats *stats);
/* j2p_solver_create_from_jpeg for the files accepted above, argument for argument. */
int j2p_solver_create_from_jpeg_scans(j2p_solver **out, int device, void *stream, const uint8_t *file, size_t size, float weight,
                                      const float pweight[], unsigned iterations, j2p_jpeg_info *info);
/* Makes the calling thread's NEXT j2p_batch_submit_file* call on b (any of the five) accept what this section accepts (accept != 0), as
 * j2p_batch_next_orientation hands a submit its orientation: consumed by that submit whatever becomes of it; j2p_job is untouched. */
int j2p_batch_next_file_scans(j2p_batch *b, unsigned accept);

/* The PNG file: the image's samples filtered and deflated ON THE DEVICE, so that a complete PNG file comes down instead of 3 or 6 bytes
 * per pixel for a host library to deflate on one core.  Every byte of the file is defined here; tests/png_cases.py restates it.  This is
 * the definition.
 *
 * 1. Samples.  width x height pixels (1..2^24 each) of `channels` = 3 (RGB) or 1 (greyscale) samples of `bits` = 8 or 16 bits, rows from
 *    the top, a row's pixels from the left, a pixel's samples interleaved, a 16-bit sample's high byte first: rb = width * bpp bytes a
 *    row with bpp = channels * bits / 8 (3, 6, 1 or 2).  From solved planes they are exactly the bytes j2p_planes_to_rgb (three planes)
 *    or j2p_planes_to_grey (one) deliver for the same width, height and bits — the same kernel writes them, into device memory.
 * 2. Filtering.  Every row becomes a filter-type byte f and rb filtered bytes: byte x of the row, v, minus a prediction, mod 256.  With a
 *    the row's byte x - bpp, b the byte x of the row above and c that row's byte x - bpp, each 0 where there is none (x < bpp, row 0) —
 *    unfiltered bytes all, so that rows do not depend on each other's filtering:
 *      f = 0 (none) 0;  1 (sub) a;  2 (up) b;  3 (average) floor((a + b) / 2);
 *      4 (Paeth) with p = a + b - c, pa = |p - a|, pb = |p - b|, pc = |p - c|: a if pa <= pb and pa <= pc, else b if pb <= pc, else c.
 *    filter = 0..4 uses that f for every row.  filter = J2P_PNG_FILTER_ADAPTIVE chooses per row, as libpng's heuristic does: the f whose
 *    rb filtered bytes have the smallest sum of |byte taken as signed| (byte below 128: itself, otherwise 256 - byte); on a tie the
 *    lowest f.  The filtered stream is the rows one after the other, height * (rb + 1) bytes.
 * 3. Tokens.  The stream is cut into deflate blocks of block_bytes bytes (0: J2P_PNG_BLOCK_BYTES; any value J2P_PNG_SIZE_MIN..MAX; the
 *    last block holds the rest; at most J2P_PNG_BLOCKS_MAX blocks, J2P_EINVAL beyond).  Within a block, byte i is "same" when it is not
 *    the block's first and equals byte i - 1.  A maximal stretch of same bytes, L of them, is cut into pieces of 258 counted from its
 *    start (the last piece holds the rest).  A piece of 3 or more bytes is ONE match of its length at distance 1, emitted at its first
 *    position; a piece of 1 or 2 bytes is that many literals; every byte that is not same is a literal.  There are no other matches.
 *    (zlib's Z_RLE idea: a function of position that a scan evaluates, and what keeps flat areas from costing a bit per byte.)
 * 4. Coding (RFC 1951).  Each block is one dynamic-Huffman block.  Symbols: literals 0..255, EOB 256 (counted once), a match's length
 *    as the standard's symbol 257..285 with its extra bits.  Code lengths from the block's own counts, at most 15 bits:
 *      a. Huffman's algorithm with two queues over the symbols in use: the leaves by count ascending, the nodes in the order they were
 *         made; the two smallest heads are joined, a leaf before a node of the same weight.  bits[n]: the leaves at depth n.
 *      b. For i from the deepest level down to 16, while bits[i] > 0: j = i - 2, lowered while bits[j] == 0; bits[i] -= 2,
 *         bits[i - 1] += 1, bits[j + 1] += 2, bits[j] -= 1.
 *      c. The lengths are dealt out, shortest first, to the symbols by count descending, then symbol value ascending.
 *      d. Codes are canonical: in order of length, within a length in order of symbol value, consecutive (RFC 1951 3.2.2).
 *    A block always has two symbols or more (a literal and EOB); with exactly two, each has one bit.  Distances: HDIST = 0, ONE distance
 *    code, for distance 1 — of length 1 (the code `0`) where the block has a match, of length 0 where it has none; a match is its length
 *    code, the extra bits, and that one bit.  The header: BFINAL, BTYPE = 2, HLIT = (the highest symbol in use) - 256, HDIST = 0, HCLEN,
 *    then the lengths of the HLIT + 257 literal/length symbols and of the distance code as ONE sequence in the code-length code: a run
 *    of n zeros is 18s (of 138, while 11 or more are left — the last of what is left), then one 17 (3..10) or up to two 0s; a run of n
 *    equal non-zero lengths is the length once, then 16s (of 6, while 3 or more are left — the last of what is left), then the length
 *    for the one or two left.  The code-length code comes from the counts of those symbols by a. - d. with the limit 7 (level 8 in b.);
 *    HCLEN + 4 is the position of the last symbol in use in the standard's order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, at
 *    least 4.  After the header the tokens in order, then EOB.  Every block but the last is followed by an empty stored block — three
 *    zero bits, zero bits up to the byte boundary, 00 00 FF FF — so that every block starts on a byte boundary and inflates on its own
 *    (no match reaches back across a block's first byte); the last block has BFINAL set and is followed by zero bits up to the byte
 *    boundary.
 * 5. Container.  The zlib stream: 78 01, the blocks, the Adler-32 of the filtered stream, high byte first.  It is cut into IDAT chunks
 *    of idat_bytes bytes of data (0: J2P_PNG_IDAT_BYTES; J2P_PNG_SIZE_MIN..MAX; the last holds the rest).  A chunk: the data's length
 *    (32 bits, high byte first), the type, the data, the CRC-32 of type and data.  The file: 89 50 4E 47 0D 0A 1A 0A; IHDR — width,
 *    height (32 bits each), bits, colour type 2 (RGB) or 0 (greyscale), 0, 0, 0; the IDAT chunks; IEND.  No other chunk.
 *
 * How it is made.  The rows are filtered, and every block's symbols counted, on the device; the counts come down (288 words a block, a
 * wait), the host makes every block's code and header (not quadratic in the alphabet) and knows every size from then on — the file's
 * too, so J2P_ESPACE is answered before anything is coded; then the blocks are packed, the stream is laid into its chunks and their
 * CRCs are taken on the device, and the file comes down (a second wait).  Output contract as for "The JPEG file": *size is set once it
 * is known; with too little capacity — out_host may then be NULL — nothing is written and the call returns J2P_ESPACE. */
#define J2P_PNG_FILTER_ADAPTIVE (-1)
#define J2P_PNG_BLOCK_BYTES 65536u
#define J2P_PNG_IDAT_BYTES 8192u
#define J2P_PNG_SIZE_MIN 16u
#define J2P_PNG_SIZE_MAX (1u << 24)
#define J2P_PNG_SIDE_MAX (1u << 24)
#define J2P_PNG_BLOCKS_MAX (1u << 20)
typedef struct j2p_png {
        unsigned width, height, bits;
        int filter;                        /* 0..4: that filter for every row; J2P_PNG_FILTER_ADAPTIVE: chosen per row */
        unsigned block_bytes, idat_bytes;  /* 0: the defaults */
} j2p_png;
/* What the coder saw of one file (stats may be NULL): rows per filter type, deflate blocks, tokens by kind, the bytes of the zlib stream
 * and the Adler-32 of the filtered stream.  Complete once the counts have been read back, also when the call then fails with J2P_ESPACE. */
typedef struct j2p_png_stats {
        unsigned long long rows[5];
        unsigned long long blocks, literals, matches, stream_bytes;
        unsigned adler;
} j2p_png_stats;
/* The current iterate of nplane = 3 (RGB) or 1 (greyscale) (solver, channel) pairs as that file.  planes[] may be one joint solver three
 * times or three `-s` solvers on one device.  Whole-canvas solvers only (a band solver: J2P_ESTATE); the argument checks of
 * j2p_planes_to_rgb / j2p_planes_to_grey apply.  Device memory is the scratch of planes[0].solver: a second call of the same size
 * allocates nothing.  Synchronises twice, as said above. */
int j2p_planes_to_png(const j2p_plane_ref planes[], unsigned nplane, const j2p_png *spec, uint8_t *out_host, size_t capacity, size_t *size);
/* The same coder on the caller's samples (host memory, item 1's layout) with no solver: for pixels from anywhere, and what the directed
 * tests use.  Device memory comes from the library's pool. */
int j2p_png_encode(int device, const j2p_png *spec, const uint8_t *samples_host, unsigned channels, uint8_t *out_host, size_t capacity,
                   size_t *size, j2p_png_stats *stats);
/* A batch job that delivers the file (j2p_planes_to_png on the worker): *spec is copied and travels next to the job (j2p_job keeps its
 * layout); out / size must stay valid until j2p_batch_wait, after which *size is the file's size — also when the job failed with
 * J2P_ESPACE.  job->out_bits must be 0, out_coef[0] NULL and out_tensor.data NULL; not with `tile`; spec->width and height must equal
 * job->out_w and out_h; the job has 1 or 3 channels (J2P_EINVAL at submit otherwise, before any device work, and no ticket is given).
 * samples: NULL, or as for j2p_batch_submit_samples.  out_planes is still honoured. */
int j2p_batch_submit_png(j2p_batch *b, const j2p_job *job, const j2p_samples samples[], const j2p_png *spec, uint8_t *out, size_t capacity,
                         size_t *size, int *ticket);
/* File in and file out in one job: the solvers from the JPEG `file` as for j2p_batch_submit_file, the result as the PNG file above.
 * Bytes go in and bytes come out; neither coefficients nor samples cross the bus. */
int j2p_batch_submit_file_png(j2p_batch *b, const j2p_job *job, const uint8_t *file, size_t size, const j2p_png *spec, uint8_t *out,
                              size_t capacity, size_t *out_size, int *ticket);

/* Upright output: the file's EXIF Orientation applied to every output form, as a pure permutation of the solved planes.  This is the
 * definition; tests/upright_cases.py restates it.
 *
 * Orientation o is 1..8 and the source image is w x h pixels (the file's frame size, times the zoom).  The upright image U is
 * w' x h' = w x h for o in 1..4 and h x w for o in 5..8, and U[y][x] = I[sy][sx] per channel, on the full-resolution solved float
 * planes (every channel of a solver lives on the full canvas: sampling factors play no part):
 *
 *      o   sx          sy                  o   sx          sy
 *      1   x           y                   5   y           x
 *      2   w - 1 - x   y                   6   y           h - 1 - x
 *      3   w - 1 - x   h - 1 - y           7   w - 1 - y   h - 1 - x
 *      4   x           h - 1 - y           8   w - 1 - y   x
 *
 * (what PIL's ImageOps.exif_transpose does.)  Beyond the image, at x >= w' or y >= h', U replicates its last column or row:
 * U[y][x] = U[min(y, h' - 1)][min(x, w' - 1)] — what an output form sees where, unoriented, it sees the canvas's solved padding (the
 * 8x8 blocks of JPEG output, an overhanging chroma grid).  The upright canvas against which a call's extents are checked is w' and h'
 * rounded up to multiples of 16; everything beyond the image being replication, no result depends on that number.
 *
 * Every output form of an oriented solver — j2p_planes_to_rgb / _grey / _tensor / _tensor_resized / _tensor_resampled /
 * _tensors_resampled / _coefficients / _coefficients_sub / _jpeg / _png — is, bit for bit, that form applied to U: the width, height,
 * box and JPEG or PNG spec a call takes are those of the upright image.  The call queues the permutation (a copy kernel; orientations
 * 5..8 through a tile in LDS) on the stream of planes[0].solver into a block of upright planes that belongs to that solver (also the planes of the other solvers of a
 * call: one block is written and read in one stream's order only), once per call and for
 * the channels the call reads, and then runs unchanged on those planes.  All planes of one call must carry the same orientation and
 * source size (J2P_EINVAL otherwise).  With orientation 1, or none ever set, a call is what it was, launch for launch and byte for byte.
 *
 * NOT oriented: the raw float planes — j2p_job.out_planes, j2p_solver_plane_ptr, j2p_solver_download — which stay the solver's canvas.
 * The j2p_planes_rows_* forms refuse an oriented solver (J2P_ESTATE), band solvers refuse an orientation other than 1 (J2P_ESTATE from
 * the setter) and a job with `tile` refuses one (J2P_EINVAL at submit: j2p_batch_next_orientation). */
/* the Orientation tag of a JPEG file: the SHORT 0x0112 in IFD0 of the first APP1 segment whose payload begins "Exif\0\0" — byte order
 * II or MM, the magic 42 and the IFD0 offset honoured, nothing read outside the segment, segments read only up to SOS (so progressive
 * files are read like baseline ones: nothing is decoded).  *orientation is 1 — and the call J2P_OK — where there is no such segment, the
 * TIFF structure is damaged or truncated, the tag has another type or count, or its value is outside 1..8 (PIL's behaviour).  Host only,
 * no allocation; independent of j2p_jpeg_parse.  J2P_EINVAL: a NULL argument. */
int j2p_jpeg_orientation(const uint8_t *file, size_t size, unsigned *orientation);
/* orientation 1..8 (J2P_EINVAL otherwise) for a source image of width x height pixels, both at least 1 and inside the canvas
 * (J2P_EINVAL).  A band solver takes only 1 (J2P_ESTATE).  Queues nothing; holds until set again.  1 is "none". */
int j2p_solver_set_orientation(j2p_solver *s, unsigned orientation, unsigned width, unsigned height);
/* what was set: 1, 0, 0 for a solver that was never oriented (any of the three may be NULL) */
int j2p_solver_orientation(const j2p_solver *s, unsigned *orientation, unsigned *width, unsigned *height);
/* the size of the solver's block of upright planes now (0: none yet, and never any for orientation 1): taken from the pool on first
 * use, grown as the output scratch grows, given back at destroy — a second call with the same orientation leaves it unchanged */
int j2p_solver_upright_bytes(const j2p_solver *s, size_t *bytes);
/* Upright batch jobs.  The orientation travels next to the job, never in it (j2p_job keeps its layout, as for every other optional
 * part): this call sets it for the NEXT job the calling thread submits to `b`, through whichever j2p_batch_submit* entry point, and
 * that submit consumes it whether it succeeds or not.  orientation: 0 = none (the call then only clears what was set), 1..8 = that
 * EXIF orientation for a source image of orient_w x orient_h pixels (a file job: left zero, the file's frame), J2P_ORIENTATION_EXIF =
 * the tag of the job's file, read at submit on the caller's thread (file jobs only).  What is wrong with it is refused by the submit
 * (J2P_EINVAL, no ticket): a value above 8, J2P_ORIENTATION_EXIF without a file, no source size without a file, a job with `tile`.
 * The worker sets the orientation on every solver it makes for the job (joint, `separate`, component 0 alone), and every output kind
 * but out_planes follows: samples, tensors, resized and resampled ones, several outputs, coefficients, the JPEG and the PNG file.
 * job->out_w / out_h, and the spec of a PNG or JPEG job, are the UPRIGHT image's; a file job that leaves out_w / out_h zero gets the
 * upright size. */
#define J2P_ORIENTATION_EXIF 0xffffffffu
int j2p_batch_next_orientation(j2p_batch *b, unsigned orientation, unsigned orient_w, unsigned orient_h);

/* Estimated tables: quantisation tables read off decoded 8-bit samples, for sample input that has no trustworthy header — frames of
 * a hardware or video decoder, a JPEG saved again as PNG or YUV, and the recompressed JPEG, whose header carries the LAST
 * compression's small steps while the blocking is the first one's.  Two steps: a histogram made on the device and a rule applied
 * to it on the host.  This text is the definition of both.
 *
 * 1. The histogram (j2p_samples_histogram).  `samples` is one channel as for sample input: device memory of `device` or host memory,
 *    any strides >= 1.  A COMPLETE block (bx, by) has bx * 8 + 8 <= w and by * 8 + 8 <= h; a block that would need replicated
 *    samples is not looked at (its coefficients are not the file's).  A complete block with any sample equal to 0 or 255 is
 *    EXCLUDED (the decoder's clamp has moved its coefficients) and only counted in *excluded.  For every other complete block:
 *    v = (float)s - 128.f, the block through dct8x8s exactly as sample input does, and for natural-order frequency j
 *    m = |(int)rintf(coefficient j)| — the step is 1, nothing is divided — and hist[j][m] += 1; *blocks counts these blocks.
 *    m <= 1016 by the argument of sample input (a counted block's samples lie in 1..254), so hist is uint32_t [64][1024], row
 *    j at hist_host + j * 1024.  Every row's counts add up to *blocks.  Host samples are staged as sample input stages them (one
 *    2-D copy of the complete blocks' rows); the call queues everything on `stream` (NULL: one of its own), synchronises it
 *    once and returns with the samples read.  Refused before a device is touched (J2P_EINVAL): a NULL argument or data, w or h
 *    zero, a stride below 1; then managed memory and another GPU's.  A plane with no complete block gives zeros and launches nothing.
 *
 * 2. The rule (j2p_quant_estimate: host code, integers only).  For frequency j, with d(m, q) the distance of m to the nearest
 *    multiple of q:
 *      nz   = the number of values with m >= 2;
 *      qmax = the largest q in 255..4 for which at most 5 * nz / 100 (integer division) of the values have d(m, q) > 1;
 *      step = among q = qmax, qmax - 1, qmax - 2 with q >= 4 the one with the smallest sum over the values with m >= 2 of
 *             min(d(m, q), 2)^2, the larger q on a tie;
 *             where no qmax exists: none when the same search over the values with m >= 4 alone (and 5 % of their number) finds
 *             one — a large step whose zeros' noise reaches 2 and 3; otherwise s = 3 when at most nz / 4 (integer division) of
 *             the values with m >= 2 are no exact multiple of 3; otherwise s = 2 by the same test; otherwise s = 1; and s is
 *             named only when 2 * sum over m >= 2 of min(hist[j][m], hist[j][m + s]) >= nz — the counts repeat with period s,
 *             which clusters around the multiples of a larger step do not;
 *      determined[j] = a step was named and nz >= 12.
 *    (A decoded sample is off by at most 1/2, which moves a coefficient by less than 1 almost always: the values of a frequency
 *    quantised with step q lie within 1 of q's multiples.  Multiples of q are multiples of its divisors too, hence the LARGEST q.
 *    Every value lies within 1 of a multiple of 3, so the small steps are told apart by EXACT multiples: about one value in
 *    twelve is moved off its multiple, while a step that is not the file's leaves a third of them or more off.)
 *    quality = the Qf in 1..100 whose IJG table — jpeg_set_quality(Qf, TRUE) on Annex K's luminance table, or with `chroma` the
 *    chrominance one — minimises the sum over determined entries of |ijg(Qf)[j] - step[j]|; the higher Qf on a tie; 100 when
 *    nothing is determined.  table[j] = step[j] where determined, otherwise max(ijg(quality)[j], 2 * (mmax_j - 1)) clamped to
 *    1..255, mmax_j the largest m of row j with a count: the box of a coefficient taken as 0 still holds what was seen.  The
 *    fill errs towards small steps, which can only make the solver do less.
 *
 * Not covered: RGB input; a block grid that does not start at sample (0, 0) (a cropped image); chroma that was upsampled after
 * decoding (estimate from planes at the file's own sampling). */
typedef struct j2p_quant_estimate_result {
        uint16_t table[64];                /* natural order, 1..255 */
        uint8_t determined[64];            /* 1: read off the histogram; 0: filled from the fitted IJG table */
        int quality;                       /* the fitted IJG quality, 1..100 */
} j2p_quant_estimate_result;
int j2p_samples_histogram(int device, void *stream, const j2p_samples *samples, uint32_t *hist_host, unsigned long long *blocks,
                          unsigned long long *excluded);
int j2p_quant_estimate(const uint32_t hist[64][1024], int chroma, j2p_quant_estimate_result *out);
/* j2p_batch_submit_samples with estimated tables: the worker that takes the job runs j2p_samples_histogram and j2p_quant_estimate on
 * every channel's samples — channel 0 against the luminance base table, the others against the chrominance one — and makes the
 * job's solvers with those tables, as j2p_solver_create_from_samples does.  The flag travels next to the job (j2p_job keeps its
 * layout).  job->planes[c].quant_table: NULL in every plane, or set in every plane (then ignored); some set and some not is
 * J2P_EINVAL, as are `tile` and samples == NULL, with nothing queued.  estimates: NULL, or nchannel records the worker fills
 * before the job finishes; they stay the caller's and must live until j2p_batch_wait. */
int j2p_batch_submit_samples_estimated(j2p_batch *b, const j2p_job *job, const j2p_samples samples[], unsigned n, const j2p_output outs[],
                                       j2p_quant_estimate_result estimates[], int *ticket);

#ifdef __cplusplus
}
#endif
#endif
