// jpeg2png_amd — C-ABI shim over the gfx950 kernels (include/jpeg2png_amd.h).
//
// A j2p_solver is the device-resident twin of the reference's per-call working
// set (`struct aux` x nchannel, compute.c:21-34) plus the iteration scalars of
// compute()/compute_step() (compute.c:425-443, :245, :258), which are evaluated
// here on the host in float exactly as the reference does and handed to the
// kernels as arguments.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <memory>
#include <vector>

#include "jpeg2png_amd.h"
#include "j2p_internal.h"
#include "j2p_geometry.h"
#include "j2p_hip_host.h"
#include "j2p_kernels.hip.h"

using namespace j2p;

// what j2p_geometry.h restates of the kernels' constants
static_assert(kStripCols == J2P_STRIP_COLS && kTY == J2P_TILE_ROWS && kHalo == J2P_HALO_ROWS, "j2p_geometry.h and j2p_kernels.hip.h disagree");

namespace {

thread_local char g_err[512] = "";

}  // namespace

int j2p_fail(int code, const char *fmt, ...)
{
        va_list l;
        va_start(l, fmt);
        vsnprintf(g_err, sizeof(g_err), fmt, l);
        va_end(l);
        return code;
}

namespace {

struct ChanHost : j2p_row_window {           // crow0, crows: of d / pg held on this device; frow0, frows: of the decoded input (init only)
        unsigned cw = 0, ch = 0, ws = 1, hs = 1;
        float *xbuf[2] = {nullptr, nullptr}; // allocation bases, (rows + 2*halo) * W floats
        float *grad = nullptr;
        float *pg = nullptr;                 // == grad where the channel keeps both in one buffer (`shared`)
        bool shared = false;                 // j2p_shares_state: g and the prob state take turns in one buffer of rows * W floats
        int16_t *d = nullptr;
        uint8_t *d8 = nullptr;               // d + 128 in bytes (k_narrow_coefficients); read by k_project instead of d when `narrow`
        bool narrow_fits = false;            // every |d| of the channel's rows held here is <= 127
        bool narrow = false;                 // ... and the projection reads the bytes (J2P_OPT_NARROW_COEFFICIENTS, default on)
        bool wide = false;                   // ws is 3, 4, 6 or 8 and the projection takes the wide-footprint path (J2P_OPT_WIDE_FOOTPRINT)
        float *q = nullptr;
        float *decoded = nullptr;            // frows * cw floats
        float *scratch_f = nullptr;          // decode scratch of bands too short to lend their x buffers (create only)
        int16_t *scratch_d = nullptr;
        float pweight = 0.f;
};

// The norm plan: who reduces ||g|| between the two phase kernels of ONE iteration ("the norm between
// the phases": the table, the measurements).  Level 1 turns the strips' partials into per-tile-row sums (J2P_NORM_L1_*),
// level 2 runs the fixed tree over those and writes the float norm (J2P_NORM_L2_*).  Every form computes the same bits.
struct NormPlan {
        int level1 = J2P_NORM_L1_NONE, level2 = J2P_NORM_L2_NORM_WHOLE;
        // k_project's NIP template argument (0 = ||g|| is read from memory); launches between the two phase kernels
        int nip() const { return level2 == J2P_NORM_L2_PROJECT_WAVES ? 1 : (level2 == J2P_NORM_L2_PROJECT_FIRST ? 2 : 0); }
        unsigned launches() const { return (level1 == J2P_NORM_L1_ROWSUMS) + (level2 == J2P_NORM_L2_NORM_WHOLE || level2 == J2P_NORM_L2_NORM_FINISH); }
};
// The one place the choice is made: pure, a few compares.  `nip_form`: whole canvases that fold run level 2 inside k_project
// (0 no, 1 every wavefront, 2 each workgroup's first); `band_nip`: bands do (NIP 2); `split`: the phase level 2 would ride on
// comes in parts (the gradient phase of a whole canvas, the projection phase of a band) and cannot carry a reduction over
// all rows; `log`: the run wants the CSV sums, whose projection kernels have no per-wavefront tree.
NormPlan norm_plan(bool whole, bool fold, int nip_form, bool band_nip, unsigned tile_rows, bool split, bool log)
{
        const bool tree = !split && tile_rows <= J2P_NORM_TREE_ROWS;           // one in-kernel tree can take every row
        NormPlan p;
        p.level1 = fold ? J2P_NORM_L1_TICKETS : (whole ? J2P_NORM_L1_NONE : J2P_NORM_L1_ROWSUMS);
        if(!whole) { p.level2 = tree && band_nip ? J2P_NORM_L2_PROJECT_FIRST : J2P_NORM_L2_NORM_FINISH; }
        else if(!fold) { p.level2 = J2P_NORM_L2_NORM_WHOLE; }
        else if(!tree) { p.level2 = J2P_NORM_L2_NORM_FINISH; }
        else if(nip_form && !log) { p.level2 = nip_form == 2 ? J2P_NORM_L2_PROJECT_FIRST : J2P_NORM_L2_PROJECT_WAVES; }
        else { p.level2 = J2P_NORM_L2_GRADIENT; }
        return p;
}

}  // namespace

struct j2p_solver {
        int device = 0;
        hipStream_t stream = nullptr;
        bool own_stream = false;
        unsigned nch = 0;
        unsigned W = 0, H = 0;
        unsigned row0 = 0, rows = 0;
        bool whole = true;
        bool band_local = false;
        ChanHost ch[kMaxCh];
        float weight = 0.f;
        unsigned iterations = 0;
        // iteration state
        unsigned iter = 0;
        float t = 1.f;
        float factor = 0.f;      // of the iteration whose gradient phase ran last
        int cur = 0;             // xbuf[cur] is x_k
        bool grad_done = false;
        bool proj_boundary_done = false;   // between the two parts of a split projection phase
        void *arena = nullptr;   // the one device allocation everything below is carved from (pooled, see j2p_pool_take)
        size_t arena_bytes = 0;
        size_t arena_used = 0;   // ... of which carved (the pool may hand out a larger block)
        void *out_scratch = nullptr;     // the output stage's scratch (j2p_solver_scratch: the taps of a filtered tensor output); pooled, kept until destroy
        size_t out_scratch_bytes = 0;
        void *upright = nullptr;         // the upright planes of an oriented solver (j2p_solver_upright), next to the scratch: the two are live together
        size_t upright_bytes = 0;
        unsigned orientation = 1, orient_w = 0, orient_h = 0;   // j2p_solver_set_orientation: 1 = none
        // reductions
        bool fold = false;       // level 1 of the norm reduction inside k_gradient (J2P_OPT_NORM_FOLD; default: norm_defaults)
        unsigned zone_d = 0, zone_b = 0, zone_c = 0;   // shares (1/256) of a gradient launch dealt as double / half / quarter tile rows (grad_item)
        // how every XCD walks its run of each phase launch (grad_item, project_item): j2p_phase_order_of's choice unless
        // J2P_OPT_PHASE_ORDER / the environment's J2P_PHASE_ORDER forced one
        j2p_phase_order order = { J2P_ORDER_FORWARD, J2P_ORDER_FORWARD };
        int nip_form = 0;               // J2P_OPT_NORM_IN_PROJECT (with fold): level 2 inside k_project, by every wavefront (1) or the workgroup's first (2)
        NormPlan plan;                  // the running iteration's (do_phase_gradient); between iterations: nobody reads it
        int nt = 0;                     // 0..3: streams with the non-temporal hint (nt_policy; J2P_OPT_NT_GRADIENT)
        bool nt_forced = false;         // set through J2P_OPT_NT_GRADIENT: the policy no longer touches it
        bool live_registered = false;   // this solver's bytes are part of the device's live total (nt_policy)
        LiveBytes live;                 // what this solver adds to it
        bool phase_log = false;         // the gradient phase of the running iteration was issued with logging
        bool mixed_project = true;      // small canvases: all samplings in one projection launch (J2P_OPT_MIXED_PROJECT)
        bool share_state = true;        // eligible channels keep g and the prob state in one buffer (J2P_SHARE_STATE=0, experiments build: two)
        bool wide_footprint = true;     // footprints 3, 4, 6, 8 columns wide take the wide-footprint path (J2P_OPT_WIDE_FOOTPRINT)
        unsigned *d_maxabs = nullptr;                 // [channel] largest |d| (k_narrow_coefficients, create only)
        unsigned long long *d_clipped = nullptr;      // [channel] samples that were 0 or 255 (k_samples_to_coefficients, create only)
        unsigned long long clipped[kMaxCh] = {0, 0, 0};   // ... read back with d_maxabs (j2p_solver_clipped_samples)
        bool sampled = false;                         // made by j2p_solver_create_from_samples
        unsigned long long *dbg_counters = nullptr;   // J2P_DEBUG builds: [0] address violations, [1] first site, [2] first offset
        unsigned long long *trace = nullptr;          // J2P_TRACE builds: wave records (tools/wave_trace.py)
        unsigned trace_cap = 0, trace_used = 0;      // records reserved by the launches so far
        bool trace_on = false;
        unsigned *tickets = nullptr;     // device: [ntr_local] per-tile-row arrival counters + [1] finished-rows counter
        unsigned rpw = 16;
        bool interior_done = false;
        bool finish_pending = false;     // split gradient phase: j2p_solver_phase_rowsums has still to run (k_rowsums if planned, the band's log sums)
        unsigned ntx = 0, nseg = 0, ntr_local = 0, ntr_global = 0, first_tr = 0;   // strips per row, row segments
        double *part_g2 = nullptr;       // [c][ntr_local][ntx]
        double *rowsum_odd = nullptr;    // band solvers: second level-1 buffer, used by odd iterations once rowsum_alternate is on
        bool rowsum_alternate = false;
        double *rowsum_local = nullptr;  // [ntr_local][c]
        double *rowsum_all = nullptr;    // [ntr_global][c]  (== rowsum_local when whole)
        double *rowsum_all_odd = nullptr;   // band solvers: the global array of odd iterations once the bands are linked
        bool linked = false;                // j2p_solver_link_bands: neighbours' rows read in place, row sums pushed
        j2p_band_links links;
        RowsumPush *push_dev = nullptr;     // [2]: the push lists of even / odd iterations, in device memory (GradArgs::push)
        bool band_nip = true;               // band solvers: ||g|| from the global row sums inside k_project (NIP 2) instead of k_norm_finish
        float *norm = nullptr;           // [c]
        // logging
        double *part_tv = nullptr;       // [ntiles][2]
        double *part_prob = nullptr;     // [c][strips]
        unsigned strips_stride = 0;
        double *logsums = nullptr;       // [iter chunk][2 + kMaxCh]
        unsigned logsums_cap = 0;
        double carried_prob[kMaxCh] = {0., 0., 0.};
        bool carried_valid = true;
        bool log_phases = false;         // the phase calls run the logging kernels and fill log_band
        double *log_band = nullptr;      // [2 + kMaxCh]: tv, tv2 of the last gradient phase, prob per channel of the last projection
        // timing
        unsigned timing = 0;     // 0 = off, k = time every k-th iteration
        std::vector<hipEvent_t> ev;      // triples: before gradient, after gradient/before reduce.., see record()
        size_t ev_used = 0;
        double acc_grad_ms = 0., acc_proj_ms = 0.;
        unsigned acc_samples = 0;
        double ev_pair_ms = 0.;  // what two event records with NOTHING between them measure on this stream (enable_timing)
};

namespace {

// bump allocator over the arena: pass 1 (base == nullptr) only adds the sizes up
struct Carver {
        char *base = nullptr;
        size_t used = 0;
        template <typename T>
        void take(T *&p, size_t count)
        {
                used = (used + 255) & ~(size_t)255;
                p = base ? reinterpret_cast<T *>(base + used) : nullptr;
                used += count * sizeof(T);
        }
};

constexpr size_t kNtWorkingSet = (size_t)260 << 20;      // see nt_policy in j2p_solver_create
constexpr size_t kMixedProjectPixels = (size_t)1 << 20;  // canvases up to this size project all channels in one launch

// The default norm configuration, which norm_plan works from (J2P_OPT_NORM_FOLD / _NORM_IN_PROJECT override it; measured:
// DESIGN.md section 4).  Bands fold: the in-kernel reduction replaces a launch AND lets the row sums alternate between two
// buffers.  On whole canvases its serial tail costs what the k_norm_whole launch did (4096^2 140.0 us per iteration either
// way, 512^2 4:2:0 42.0 vs 40.3 us), so they fold only up to kNormInProjectPixels (2.5 Mpixel: bound by the number of
// dependent launches, every wavefront of k_project runs the tree, NIP 1) and — where one tree takes the tile rows — from
// kFoldWholePixels (32 Mpixel) on, where k_norm_whole would stage 17 K partials through one CU (both levels in k_gradient)
constexpr size_t kNormInProjectPixels = (size_t)5 << 19;
constexpr size_t kFoldWholePixels = (size_t)1 << 25;
void norm_defaults(j2p_solver *s)
{
        const size_t pixels = (size_t)s->W * s->H;
        s->nip_form = s->whole && pixels <= kNormInProjectPixels ? 1 : 0;
        s->fold = !s->whole || s->nip_form || (pixels >= kFoldWholePixels && s->ntr_global <= J2P_NORM_TREE_ROWS);
}

// nt_policy: which streams of the iteration get the non-temporal hint, so that what stays without it can live in
// the 256 MiB Infinity Cache.  Per byte and iteration x_k and x_{k-1} are touched 2-3 times, g and the prob state
// twice, d once: keep the planes, then d and the prob state if they fit beside them, g last.
// Measured on single Y planes (us per iteration; none / level 1 / level 2 / level 3):
//   4096x3584 (252 MiB) 112.3 / 114.1            4096x4096 (288 MiB) 135.8 / 127.0
//   4096x5120 (360 MiB) 175.0 / 163.7 / 159.6 / 163.4
//   16384x2048 (576 MiB) 295 / 292.7 / 250.8 / 240.2     8192x8192 (1152 MiB) - / 541.5 / 528.3 / 527.0
// The cache is the DEVICE's: the sums run over every live solver of the device (the images of a batch, the
// components of `-s`, bands sharing a GPU), re-evaluated at create and at reset.  J2P_NT_SCOPE=solver: this
// solver's own bytes only (round 2's policy; A/B).
int nt_policy(const j2p_solver *s)
{
        static const bool own_only = [] {
                const char *env = j2p_exp_env("J2P_NT_SCOPE");
                return env && strcmp(env, "solver") == 0;
        }();
        const LiveBytes l = own_only || !s->live_registered ? s->live : j2p_live_on(s->device);
        const j2p_live_bytes b = {l.working_set, l.g, l.planes, l.d};
        return j2p_nt_level(&b, kNtWorkingSet);
}

// the bytes of the coefficients the projection actually reads (one or two per coefficient, ChanHost::narrow) in the
// solver's share of the device's live total, and the policy again
void account_coefficient_bytes(j2p_solver *s)
{
        size_t d_bytes = 0;
        for(unsigned c = 0; c < s->nch; c++) {
                const ChanHost &h = s->ch[c];
                d_bytes += (size_t)(h.crows ? h.crows : 1) * h.cw * (h.narrow ? sizeof(uint8_t) : sizeof(int16_t));
        }
        if(d_bytes == s->live.d) { return; }
        if(s->live_registered) { j2p_live_add(s->device, s->live, -1); }
        s->live.working_set = s->live.working_set - s->live.d + d_bytes;
        s->live.d = d_bytes;
        if(s->live_registered) { j2p_live_add(s->device, s->live, +1); }
        if(!s->nt_forced) { s->nt = nt_policy(s); }
}

// which channels the projection sends down the wide-footprint path (project_strip: WS = ws in 3, 4, 6, 8, rows at run time)
void set_wide_footprint(j2p_solver *s)
{
        for(unsigned c = 0; c < s->nch; c++) {
                const unsigned ws = s->ch[c].ws;
                s->ch[c].wide = s->wide_footprint && (ws == 3 || ws == 4 || ws == 6 || ws == 8);
        }
}

ChanDev chan_dev(const j2p_solver *s, unsigned c)
{
        const ChanHost &h = s->ch[c];
        ChanDev k;
        const size_t halo = (size_t)kHalo * s->W;
        k.xcur = h.xbuf[s->cur] + halo;
        k.xprev = h.xbuf[s->cur ^ 1] + halo;
        k.grad = h.grad;
        k.pg = h.pg;
        k.d = h.d;
        k.d8 = h.narrow ? h.d8 : nullptr;
        k.q = h.q;
        k.cw = h.cw;
        k.ch = h.ch;
        k.ws = h.ws;
        k.hs = h.hs;
        k.crow0 = h.crow0;
        k.crows = h.crows;
        k.p_alpha = h.pweight * 2 * 255 * sqrtf(2);       // compute.c:245
        k.prob_on = h.pweight != 0.f;
#ifdef J2P_DEBUG
        {
                // what each access of the phase kernels is meant to stay inside (see DbgChan)
                const long above = s->row0 < (unsigned)kHalo ? (long)s->row0 : (long)kHalo;
                const unsigned below_rows = s->H - s->row0 - s->rows;
                const long below = below_rows < (unsigned)kHalo ? (long)below_rows : (long)kHalo;
                const float *own[2] = {k.xcur, k.xprev};
                for(int i = 0; i < 2; i++) {
                        k.dbg.x_read[i] = {reinterpret_cast<const char *>(own[i] - above * (long)s->W),
                                           reinterpret_cast<const char *>(own[i] + ((long)s->rows + below) * (long)s->W)};
                        k.dbg.x_own[i] = {reinterpret_cast<const char *>(own[i]), reinterpret_cast<const char *>(own[i] + (size_t)s->rows * s->W)};
                }
                const size_t cells = (size_t)(h.crows ? h.crows : 1) * h.cw;
                k.dbg.grad = {reinterpret_cast<const char *>(h.grad), reinterpret_cast<const char *>(h.grad + (size_t)s->rows * s->W)};
                // (a shared buffer: the prob state's range is the buffer's, the gradient's)
                k.dbg.pg = {reinterpret_cast<const char *>(h.pg), reinterpret_cast<const char *>(h.pg + (h.shared ? (size_t)s->rows * s->W : cells))};
                if(h.narrow) { k.dbg.d = {reinterpret_cast<const char *>(h.d8), reinterpret_cast<const char *>(h.d8 + cells)}; }
                else { k.dbg.d = {reinterpret_cast<const char *>(h.d), reinterpret_cast<const char *>(h.d + cells)}; }
                k.dbg.counters = s->dbg_counters;
        }
#endif
        return k;
}

Geo geo_of(const j2p_solver *s)
{
        Geo g;
        g.W = s->W;
        g.H = s->H;
        g.row0 = s->row0;
        g.rows = s->rows;
        g.ntx = s->ntx;
        g.rpw = s->rpw;
        g.seg_off = 0;
        g.seg_mul = 1;
        g.units = 0;            // (do_phase_gradient fills in the launch's own)
        g.ntr_launch = 0;
        g.zone_d = g.zone_b = g.zone_c = 0;
        g.reverse = 0;
#ifdef J2P_TRACE
        g.trace = s->trace_on ? s->trace : nullptr;
        g.trace_cap = s->trace_cap;
        g.trace_seq = s->iter;
        g.trace_base = s->trace_used;
#endif
        return g;
}

// where the gradient phase of iteration `iter` leaves its level-1 row sums [tile row][channel]: band solvers whose sums
// are read in place by other bands (j2p_solver_alternate_rowsums) alternate between two arrays
double *rowsums_of(const j2p_solver *s, unsigned iter)
{
        return (s->rowsum_alternate && (iter & 1)) ? s->rowsum_odd : s->rowsum_local;
}

NormPlan plan_of(const j2p_solver *s, bool split, bool log) { return norm_plan(s->whole, s->fold, s->nip_form, s->band_nip, s->ntr_global, split, log); }
bool rowsums_owed(const j2p_solver *s) { return s->finish_pending && s->plan.level1 == J2P_NORM_L1_ROWSUMS; }

// units of a gradient launch over `ntr` tile rows (grad_item): pairs of tile rows x 4 strips (256-thread workgroups), or —
// joint images, one wavefront per channel — x one strip
unsigned grad_units(const j2p_solver *s, unsigned ntr)
{
        const unsigned positions = s->ntx * ((ntr + 1) / 2);
        return s->nch == 1 ? (positions + 3) / 4 : positions;
}
ZoneShares zone_shares(const Geo &g) { return ZoneShares{g.zone_d, g.zone_b, g.zone_c}; }

template <int J>
void launch_gradient(const GradArgs &a, hipStream_t st, bool tgv, bool log, int nt)
{
        // J == 1: 4 strips per 256-thread workgroup; J > 1: one strip per workgroup of J wavefronts
        const dim3 grid(grad_grid(a.geo.units, zone_shares(a.geo)));
        const dim3 block = J == 1 ? dim3(256) : dim3(64 * J);
        // non-temporal g / prob state (see nt_policy): the kernels without logging
        if(nt >= 1 && !log) {
                if(nt >= 2) {
                        if(tgv) { hipLaunchKernelGGL((k_gradient<true, false, J, 2>), grid, block, 0, st, a); }
                        else { hipLaunchKernelGGL((k_gradient<false, false, J, 2>), grid, block, 0, st, a); }
                } else {
                        if(tgv) { hipLaunchKernelGGL((k_gradient<true, false, J, 1>), grid, block, 0, st, a); }
                        else { hipLaunchKernelGGL((k_gradient<false, false, J, 1>), grid, block, 0, st, a); }
                }
                return;
        }
        if(tgv) {
                if(log) { hipLaunchKernelGGL((k_gradient<true, true, J>), grid, block, 0, st, a); }
                else { hipLaunchKernelGGL((k_gradient<true, false, J>), grid, block, 0, st, a); }
        } else {
                if(log) { hipLaunchKernelGGL((k_gradient<false, true, J>), grid, block, 0, st, a); }
                else { hipLaunchKernelGGL((k_gradient<false, false, J>), grid, block, 0, st, a); }
        }
}

hipEvent_t next_event(j2p_solver *s)
{
        if(s->ev_used == s->ev.size()) {
                hipEvent_t e;
                if(hipEventCreate(&e) != hipSuccess) { return nullptr; }
                s->ev.push_back(e);
        }
        return s->ev[s->ev_used++];
}

void mark(j2p_solver *s)
{
        if(!s->timing || s->iter % s->timing) { return; }
        hipEvent_t e = next_event(s);
        if(e) { (void)hipEventRecord(e, s->stream); }
}

// fold recorded events (groups of 4: gradient begin/end, project begin/end) into the accumulators
int flush_timing(j2p_solver *s)
{
        if(s->ev_used == 0) { return J2P_OK; }
        HIP_TRY(hipStreamSynchronize(s->stream));
        for(size_t i = 0; i + 3 < s->ev_used; i += 4) {
                float g = 0.f, p = 0.f;
                HIP_TRY(hipEventElapsedTime(&g, s->ev[i], s->ev[i + 1]));
                HIP_TRY(hipEventElapsedTime(&p, s->ev[i + 2], s->ev[i + 3]));
                // (a pair of records brackets the kernel AND the records' own packets.  What an EMPTY bracket measures is
                // calibrated when timing is switched on (ev_pair_ms, 4.8 us on MI355X) and reported, but NOT taken off: with
                // a kernel in between part of it overlaps, and the corrected figures came out below rocprofv3's — 50.5 vs
                // 53.2 us — which is the wrong side to err on)
                s->acc_grad_ms += g;
                s->acc_proj_ms += p;
                s->acc_samples++;
        }
        s->ev_used = 0;
        return J2P_OK;
}

// part: 0 = all segments, 1 = interior segments only (they never read halo rows), 2 = the first and
// last segment (after the halo rows have arrived).  1 then 2 make one gradient phase; `st` is the stream
// the kernel goes to (part 2 may use a side stream so that it overlaps part 1).
// band-level sums for the CSV row (tv, tv2 after a gradient phase; prob distance after a projection)
static void launch_band_log(j2p_solver *s, int which)
{
        if(which == 0) {
                hipLaunchKernelGGL(k_log_sums, dim3(1), dim3(256), 0, s->stream, (const double *)s->part_tv, s->ntx * s->nseg,
                                   (const double *)s->part_prob, 0u, s->strips_stride, s->nch, s->log_band, 0);
        } else {
                hipLaunchKernelGGL(k_log_sums, dim3(1), dim3(256), 0, s->stream, (const double *)s->part_tv, 0u,
                                   (const double *)s->part_prob, s->strips_stride, s->strips_stride, s->nch, s->log_band, 1);
        }
}

// The launches of the stand-alone reduction kernels as functions of plain arguments: what a solve launches and what
// j2p_norm_selftest launches on a caller's arrays are the same lines (grid, LDS size, staging), so the hook cannot drift.
static unsigned tree_width(unsigned tile_rows)           // P of tree_sum_lds: the power of two >= the tile rows
{
        unsigned P = 1;
        while(P < tile_rows) { P <<= 1; }
        return P;
}
// level 1: per-tile-row sums of norm partials: blocks of up to 256 tile rows, as many as stage in LDS
static void launch_k_rowsums(hipStream_t st, const double *part, double *rowsum, unsigned ntx, unsigned tile_rows_local, unsigned nch)
{
        const unsigned total = tile_rows_local * nch;
        unsigned per_block = kStageDoubles / ntx;
        if(per_block > 256) { per_block = 256; }
        hipLaunchKernelGGL(k_rowsums, dim3((total + per_block - 1) / per_block), dim3(256), 0, st,
                           part, rowsum, ntx, tile_rows_local, nch, per_block);
}
// level 2 over the global [tile row][channel] sums
static void launch_k_norm_finish(hipStream_t st, const double *rowsum_all, unsigned tile_rows_global, unsigned nch, float *norm)
{
        hipLaunchKernelGGL(k_norm_finish, dim3(nch), dim3(256), tree_width(tile_rows_global) * sizeof(double), st,
                           rowsum_all, tile_rows_global, nch, norm);
}
// ... over the bands' own arrays (j2p_solver_norm_from_bands)
static void launch_k_norm_bands(hipStream_t st, const BandRowsums &t, unsigned tile_rows_global, unsigned nch)
{
        hipLaunchKernelGGL(k_norm_bands, dim3(nch), dim3(256), tree_width(tile_rows_global) * sizeof(double), st, t, tile_rows_global, nch);
}
// both levels in one launch.  k_norm_whole (only the A/B baseline of the folded reduction, J2P_OPT_NORM_FOLD = 0) stages
// the norm partials in up to 156 KiB of dynamic LDS: allowed once per device (idempotent) ...
static hipError_t allow_k_norm_whole_lds()
{
        return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_norm_whole), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kNormLdsBytes);
}
// ... and as many of the partials staged at once as the CU's LDS holds (P <= 4096)
static void launch_k_norm_whole(hipStream_t st, const double *part, unsigned ntx, unsigned tile_rows, unsigned nch, float *norm)
{
        const unsigned P = tree_width(tile_rows);
        unsigned stage = 0;                                  // narrow canvases: direct form (4.6 vs 5.4 us at 4096^2)
        if(ntx > 48) {
                stage = tile_rows * ntx;
                if((P + stage) * sizeof(double) > kNormLdsBytes) { stage = kNormLdsBytes / sizeof(double) - P; }
        }
        hipLaunchKernelGGL(k_norm_whole, dim3(nch), dim3(256), (P + stage) * sizeof(double), st, part, ntx, tile_rows, nch, norm, stage);
}

static void launch_rowsums(j2p_solver *s)
{
        launch_k_rowsums(s->stream, (const double *)s->part_g2, s->rowsum_local, s->ntx, s->ntr_local, s->nch);
}

// the end of a gradient phase — of a split one: on the solver's stream, which the caller has made wait for the boundary part
int do_rowsums(j2p_solver *s)
{
        if(!s->grad_done) { return j2p_fail(J2P_ESTATE, "rowsums without a finished gradient phase"); }
        if(!s->finish_pending) { return J2P_OK; }      // (a whole phase has finished itself)
        if(s->plan.level1 == J2P_NORM_L1_ROWSUMS) { launch_rowsums(s); }
        if(s->phase_log && s->log_phases) { launch_band_log(s, 0); }
        s->finish_pending = false;
        HIP_TRY(hipGetLastError());
        return J2P_OK;
}

int do_phase_gradient(j2p_solver *s, bool log, int part = 0, hipStream_t st = nullptr)
{
        if(s->grad_done) { return j2p_fail(J2P_ESTATE, "phase_gradient called twice without phase_project"); }
        if(part == 2 && !s->interior_done) { return j2p_fail(J2P_ESTATE, "gradient boundary part before the interior part"); }
        if(part != 2 && s->interior_done) { return j2p_fail(J2P_ESTATE, "gradient interior part issued twice"); }
        if(part != 0 && s->nseg < 3) { return j2p_fail(J2P_ESTATE, "band too short to split the gradient phase"); }
        if(!st) { st = s->stream; }
        if(part != 2) {
                // the iteration's norm plan, decided here once; a band learns only in do_phase_project whether ITS phase is split
                s->plan = plan_of(s, s->whole && part != 0, log);
                s->phase_log = log;
                // FISTA scalars in float, as compute.c:431-432,440
                const float tnext = (1 + sqrtf(1 + 4 * (s->t * s->t))) / 2;
                s->factor = (s->t - 1) / tnext;
                s->t = tnext;
        }
        unsigned nseg_launch = s->nseg;
        unsigned seg_off = 0, seg_mul = 1;
        if(part == 1) { nseg_launch = s->nseg - 2; seg_off = 1; }
        if(part == 2) { nseg_launch = 2; seg_mul = s->nseg - 1; }

        GradArgs a;
        for(unsigned c = 0; c < s->nch; c++) { a.ch[c] = chan_dev(s, c); }
        a.geo = geo_of(s);
        a.geo.seg_off = seg_off;
        a.geo.seg_mul = seg_mul;
        a.geo.units = grad_units(s, nseg_launch);
        a.geo.ntr_launch = nseg_launch;
        // (half / quarter items: whole phases of one channel per workgroup wavefront, see j2p_zone_shares in j2p_geometry.h)
        if(part == 0 && s->nch == 1) { a.geo.zone_d = s->zone_d; a.geo.zone_b = s->zone_b; a.geo.zone_c = s->zone_c; }
        a.geo.reverse = part == 0 ? s->order.gradient : kOrderForward;
        a.factor = s->factor;
        a.a_tv = (float)(1. / (double)sqrtf((float)s->nch));                    // compute.c:90
        const float alpha = s->weight / sqrtf((float)(4 / 2));                  // compute.c:258
        a.a_tgv = (float)((double)alpha * 1. / (double)sqrtf((float)s->nch));   // compute.c:154
        a.part_g2 = s->part_g2;
        a.part_tv = s->part_tv;
        // what of the norm reduction rides on this launch (the plan): level 1 by tickets, level 2 behind it
        a.row_ticket = s->plan.level1 == J2P_NORM_L1_TICKETS ? s->tickets : nullptr;
        a.done_ticket = s->tickets + s->ntr_local;
        a.rowsum = rowsums_of(s, s->iter);
        a.push = nullptr;
        if(s->linked) {
                if(part != 0) { return j2p_fail(J2P_ESTATE, "linked bands run whole phases (there is no exchange to hide)"); }
                a.push = s->push_dev + (s->iter & 1);
        }
        a.norm_out = s->plan.level2 == J2P_NORM_L2_GRADIENT ? s->norm : nullptr;
        a.nch_total = s->nch;
        a.fold_phase = s->iter & 1;
        a.fold_rows = s->ntr_local;
        a.ntr_global = s->ntr_global;
        const bool tgv = s->weight != 0.f;
        if(part != 2) { mark(s); }     // event timing covers the main launch only (the edge part runs on another stream)
        // one wavefront per channel; the channels of a joint image share a workgroup and exchange their norm
        // contributions through LDS (the schedules that lost to this one: DESIGN.md section 10)
        switch(s->nch) {
        case 1: launch_gradient<1>(a, st, tgv, log, s->nt); break;
        case 2: launch_gradient<2>(a, st, tgv, log, s->nt); break;
        default: launch_gradient<3>(a, st, tgv, log, s->nt); break;
        }
        if(part != 2) { mark(s); }
        HIP_TRY(hipGetLastError());
#ifdef J2P_TRACE
        if(s->trace_on) {       // one record per wavefront of the launch (J == 1: 4 strips per workgroup; joint: one strip)
                s->trace_used += grad_grid(a.geo.units, zone_shares(a.geo)) * (s->nch > 1 ? s->nch : 4u);
        }
#endif
        if(part == 1) {
                s->interior_done = true;
                return J2P_OK;
        }
        s->interior_done = false;
        s->grad_done = true;
        // k_rowsums and the band's CSV sums go behind the phase's last launch: now, or in j2p_solver_phase_rowsums()
        s->finish_pending = true;
        return part == 0 ? do_rowsums(s) : J2P_OK;
}

// the instantiations of k_project by what the launch needs: NT = non-temporal level (nt_policy), NIP = who reduces
// ||g|| (0: read from memory, 1: every wavefront, 2: the workgroup's first wavefront — bands), PTR = pointer form of the
// row loads (rows >= 64 KiB apart)
template <int NT, int NIP>
void launch_project_unit_nt(bool ptr, dim3 grid, hipStream_t st, const ProjArgs &a)
{
        if(ptr) { hipLaunchKernelGGL((k_project<false, 1, 1, NT, NIP, true>), grid, dim3(256), 0, st, a); }
        else { hipLaunchKernelGGL((k_project<false, 1, 1, NT, NIP, false>), grid, dim3(256), 0, st, a); }
}
void launch_project_unit(int nt, int nip, bool ptr, dim3 grid, hipStream_t st, const ProjArgs &a)
{
        if(nip == 2) {
                switch(nt) {
                case 0: launch_project_unit_nt<0, 2>(ptr, grid, st, a); break;
                case 1: launch_project_unit_nt<1, 2>(ptr, grid, st, a); break;
                case 2: launch_project_unit_nt<2, 2>(ptr, grid, st, a); break;
                default: launch_project_unit_nt<3, 2>(ptr, grid, st, a); break;
                }
        } else {
                switch(nt) {
                case 0: launch_project_unit_nt<0, 0>(ptr, grid, st, a); break;
                case 1: launch_project_unit_nt<1, 0>(ptr, grid, st, a); break;
                case 2: launch_project_unit_nt<2, 0>(ptr, grid, st, a); break;
                default: launch_project_unit_nt<3, 0>(ptr, grid, st, a); break;
                }
        }
}
// every other case by sampling class: logging, subsampled channels, the per-wavefront tree of small canvases
// (wide: the class's footprint takes the wide-footprint path, ChanHost::wide; any number of rows)
template <bool LOG, int NIP>
void launch_project_sampled(unsigned ws, unsigned hs, bool wide, dim3 grid, hipStream_t st, const ProjArgs &a)
{
        if(ws == 1 && hs == 1) { hipLaunchKernelGGL((k_project<LOG, 1, 1, 0, NIP>), grid, dim3(256), 0, st, a); }
        else if(ws == 2 && hs == 2) { hipLaunchKernelGGL((k_project<LOG, 2, 2, 0, NIP>), grid, dim3(256), 0, st, a); }
        else if(ws == 2 && hs == 1) { hipLaunchKernelGGL((k_project<LOG, 2, 1, 0, NIP>), grid, dim3(256), 0, st, a); }
        else if(ws == 1 && hs == 2) { hipLaunchKernelGGL((k_project<LOG, 1, 2, 0, NIP>), grid, dim3(256), 0, st, a); }
        else if(wide && ws == 4) { hipLaunchKernelGGL((k_project<LOG, 4, 0, 0, NIP>), grid, dim3(256), 0, st, a); }
        else if(wide && ws == 8) { hipLaunchKernelGGL((k_project<LOG, 8, 0, 0, NIP>), grid, dim3(256), 0, st, a); }
        else if(wide && ws == 3) { hipLaunchKernelGGL((k_project<LOG, 3, 0, 0, NIP>), grid, dim3(256), 0, st, a); }
        else if(wide && ws == 6) { hipLaunchKernelGGL((k_project<LOG, 6, 0, 0, NIP>), grid, dim3(256), 0, st, a); }
        else { hipLaunchKernelGGL((k_project<LOG, 0, 0, 0, NIP>), grid, dim3(256), 0, st, a); }
}

// whether the projection phase is ONE k_project_mixed launch (small canvases with several samplings); nip as below
bool projects_mixed(const j2p_solver *s, int nip)
{
        bool mixed = false;
        for(unsigned c = 1; c < s->nch; c++) { mixed = mixed || s->ch[c].ws != s->ch[0].ws || s->ch[c].hs != s->ch[0].hs; }
        return mixed && s->mixed_project && nip != 2 && (size_t)s->W * s->rows <= kMixedProjectPixels;
}

// part: 0 = whole phase; J2P_PROJECT_BOUNDARY (1) = norm + the band's first and last block row of every
// channel (they hold the rows the neighbours need); J2P_PROJECT_INTERIOR (2) = the rest, ends the iteration
int do_phase_project(j2p_solver *s, bool log, int part = 0)
{
        const hipStream_t st = s->stream;
        if(!s->grad_done) { return j2p_fail(J2P_ESTATE, "phase_project called before phase_gradient"); }
        if(rowsums_owed(s)) { return j2p_fail(J2P_ESTATE, "phase_project before j2p_solver_phase_rowsums"); }
        // the two phases of an iteration must agree on logging: where the norm is reduced depends on it
        if(log != s->phase_log) { return j2p_fail(J2P_ESTATE, "phase_project: logging differs from this iteration's gradient phase"); }
        if(part == 2 && !s->proj_boundary_done) { return j2p_fail(J2P_ESTATE, "interior part of phase_project before the boundary part"); }
        if(part != 2 && s->proj_boundary_done) { return j2p_fail(J2P_ESTATE, "boundary part of phase_project issued twice"); }
        // the global [tile row][channel] sums a band solver finishes ||g|| from: gathered by the caller, or — linked
        // bands — stored there by every band's gradient launch, even and odd iterations in two arrays
        const double *global_rows = s->whole ? rowsums_of(s, s->iter) : ((s->linked && (s->iter & 1)) ? s->rowsum_all_odd : s->rowsum_all);
        // (the one circumstance the gradient phase could not know: a band's projection phase in parts takes the split plan)
        if(part == 1 && !s->whole && s->plan.level2 == J2P_NORM_L2_PROJECT_FIRST) { s->plan = plan_of(s, true, log); }
        // the reduction launch in front of k_project, if the plan has one (an interior part finds ||g|| written, as if by the caller)
        switch(part == 2 ? J2P_NORM_L2_EXTERNAL : s->plan.level2) {
        case J2P_NORM_L2_NORM_FINISH:
                // level 1 came with the gradient phase (band solvers: the caller has gathered all bands' row sums)
                launch_k_norm_finish(st, global_rows, s->ntr_global, s->nch, s->norm);
                break;
        case J2P_NORM_L2_NORM_WHOLE:
                launch_k_norm_whole(st, (const double *)s->part_g2, s->ntx, s->ntr_local, s->nch, s->norm);
                break;
        default: break;        // the gradient launch or the caller has written ||g||, or k_project runs the tree itself
        }
        ProjArgs a;
        for(unsigned c = 0; c < s->nch; c++) { a.ch[c] = chan_dev(s, c); }
        a.geo = geo_of(s);
        a.factor = s->factor;
        const float radius = sqrtf((float)s->H * (float)s->W) / 2;             // compute.c:425
        a.step = radius / sqrtf((float)(1 + s->iterations));                    // compute.c:443
        a.norm = s->norm;
        a.part_prob = s->part_prob;
        a.strips_per_chan = s->strips_stride;
        a.order = s->order.project;
        const int nip = s->plan.nip();
        a.norm_rowsums = nip ? global_rows : nullptr;
        a.norm_rows = s->ntr_global;
        a.norm_nch = s->nch;
        for(unsigned c = 0; c < kMaxCh; c++) { a.halo_up[c] = a.halo_down[c] = nullptr; }
        if(s->linked) {
                // the band's edge rows of x_{k+1} also go into the neighbours' halo rows of the buffer being written
                // (only the NIP 2 instantiations store them: a linked band always takes those)
                if(nip != 2) { return j2p_fail(J2P_ESTATE, "linked bands: ||g|| must be reduced inside k_project (whole phases, at most %u tile rows, J2P_BAND_NIP not 0)", J2P_NORM_TREE_ROWS); }
                for(unsigned c = 0; c < s->nch; c++) {
                        a.halo_up[c] = s->links.up_halo[s->cur ^ 1][c];
                        a.halo_down[c] = s->links.down_halo[s->cur ^ 1][c];
                }
        }
        if(part != 1) { mark(s); }
        auto block_rows = [&](unsigned hs, unsigned z) -> unsigned {
                const unsigned brows = (s->rows + 8 * hs - 1) / (8 * hs);
                if(part == 0) { a.by_offset[z] = 0; a.by_mul[z] = 1; a.nby[z] = brows; }
                else if(part == 1) { a.by_offset[z] = 0; a.by_mul[z] = brows > 1 ? brows - 1 : 1; a.nby[z] = brows < 2 ? brows : 2; }
                else { a.by_offset[z] = 1; a.by_mul[z] = 1; a.nby[z] = brows > 2 ? brows - 2 : 0; }
                return a.nby[z];
        };
        if(projects_mixed(s, nip)) {
                // (k_project_mixed has the per-wavefront tree only; canvases this small take that form anyway)
                // small canvas, several samplings: one launch for all channels (k_project_mixed)
                unsigned max_strips = 0;
                for(unsigned c = 0; c < s->nch; c++) {
                        a.chan_of_z[c] = c;
                        const unsigned ws = s->ch[c].ws, hs = s->ch[c].hs;
                        const unsigned strips = ((s->W + 64 * ws - 1) / (64 * ws)) * block_rows(hs, c);
                        if(strips > max_strips) { max_strips = strips; }
                }
                if(max_strips) {
                        const dim3 grid((max_strips + 3) / 4, 1, s->nch);
                        if(log) { hipLaunchKernelGGL((k_project_mixed<true, false>), grid, dim3(256), 0, st, a); }
                        else if(nip == 1) { hipLaunchKernelGGL((k_project_mixed<false, true>), grid, dim3(256), 0, st, a); }
                        else { hipLaunchKernelGGL((k_project_mixed<false, false>), grid, dim3(256), 0, st, a); }
#ifdef J2P_TRACE
                        if(s->trace_on) { s->trace_used += grid.x * grid.z * 4; }
#endif
                }
        } else {
        // one launch per sampling class present (usually: luma 1x1, both chroma 2x2)
        bool done[kMaxCh] = {false, false, false};
        for(unsigned c0 = 0; c0 < s->nch; c0++) {
                if(done[c0]) { continue; }
                const unsigned ws = s->ch[c0].ws, hs = s->ch[c0].hs;
                unsigned nz = 0;
                for(unsigned c = c0; c < s->nch; c++) {
                        if(!done[c] && s->ch[c].ws == ws && s->ch[c].hs == hs) {
                                block_rows(hs, nz);
                                a.chan_of_z[nz++] = c;
                                done[c] = true;
                        }
                }
                if(a.nby[0] == 0) { continue; }
                const unsigned strips = ((s->W + 64 * ws - 1) / (64 * ws)) * a.nby[0];
                const bool wide = s->ch[c0].wide;
                dim3 grid((strips + 3) / 4, 1, nz);
                if(ws == 1 && hs == 1 && !log && nip != 1) {
                        // the 1x1 instantiations: g is read non-temporally exactly when the gradient launch wrote it that
                        // way (nt levels, nt_policy); rows >= 64 KiB apart take the pointer form of the 24 loads (see
                        // project_strip); bands reduce ||g|| themselves (NIP 2)
                        const bool far_rows = (size_t)s->W * sizeof(float) >= 65536;
                        launch_project_unit(s->nt, nip, far_rows, grid, st, a);
                }
                else if(log && nip == 2) { launch_project_sampled<true, 2>(ws, hs, wide, grid, st, a); }
                else if(log) { launch_project_sampled<true, 0>(ws, hs, wide, grid, st, a); }
                else if(nip == 2) { launch_project_sampled<false, 2>(ws, hs, wide, grid, st, a); }
                else if(nip == 1) { launch_project_sampled<false, 1>(ws, hs, wide, grid, st, a); }
                else { launch_project_sampled<false, 0>(ws, hs, wide, grid, st, a); }
#ifdef J2P_TRACE
                if(s->trace_on) {
                        s->trace_used += grid.x * grid.z * 4;
                        a.geo.trace_base = s->trace_used;       // the next sampling class's launch
                }
#endif
        }
        }
        if(part != 1) { mark(s); }
        HIP_TRY(hipGetLastError());
        if(part == 1) {
                s->proj_boundary_done = true;
                return J2P_OK;
        }
        s->proj_boundary_done = false;
        if(log && s->log_phases) { launch_band_log(s, 1); }
        s->cur ^= 1;        // SWAP(fdata, fista) of compute.c:438: the buffer just written is x_{k+1}
        s->iter++;
        s->grad_done = false;
        return J2P_OK;
}

int upload(void *dst, const void *src, size_t bytes, hipStream_t st)
{
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
        return J2P_OK;
}

int launch_init(j2p_solver *s)
{
        for(unsigned c = 0; c < s->nch; c++) {
                const ChanHost &h = s->ch[c];
                ChanDev k = chan_dev(s, c);
                k.crow0 = h.frow0;          // the decoded input has its own row window
                const int fill_halo = s->band_local ? 0 : 1;
                hipLaunchKernelGGL(k_init_state, dim3(2048), dim3(256), 0, s->stream, k, geo_of(s),
                                   (const float *)h.decoded, fill_halo);
                // (a shared buffer is zeroed whole: what a solve left in it is gradient as well as prob state)
                if(h.shared) { hipLaunchKernelGGL(k_fill_zero, dim3(1024), dim3(256), 0, s->stream, h.pg, (size_t)s->rows * s->W); }
                else if(h.crows) {
                        hipLaunchKernelGGL(k_fill_zero, dim3(1024), dim3(256), 0, s->stream, h.pg, (size_t)h.crows * h.cw);
                }
        }
        HIP_TRY(hipGetLastError());
        // the partials of a folding gradient launch carry the iteration's parity in their sign bit (fold_tile_row): what
        // the slots hold before iteration 0 must carry the other one — all bits set
        HIP_TRY(hipMemsetAsync(s->part_g2, 0xff, (size_t)s->ntx * s->ntr_local * s->nch * sizeof(double), s->stream));
        s->iter = 0;
        s->t = 1.f;
        s->cur = 0;
        s->grad_done = false;
        s->interior_done = false;
        s->finish_pending = false;
        s->plan = NormPlan();
        s->proj_boundary_done = false;
        for(unsigned c = 0; c < kMaxCh; c++) { s->carried_prob[c] = 0.; }
        s->carried_valid = true;
        return J2P_OK;
}

// ---------------------------------------------------------------------------
// The stages of j2p_solver_create, in the order it runs them.  Each returns J2P_OK or the error with its text set; the
// half-built solver is j2p_solver_create's to destroy.
// ---------------------------------------------------------------------------

// what the planes and the band say before a device is touched: the canvas, and in *band the rows the solver holds
// (samples: j2p_solver_create_from_samples — the planes carry no arrays, samples[c] stands in for them; from_file:
// j2p_solver_create_from_jpeg — none either, the file's scan is decoded into the resident coefficients)
int validate(unsigned nchannel, const j2p_plane planes[], const j2p_samples samples[], bool from_file, int band_local_arrays, j2p_canvas *cv,
             j2p_band *band, bool *is_whole)
{
        if(nchannel == 0 || nchannel > kMaxCh) { return j2p_fail(J2P_EINVAL, "nchannel must be 1..3 (compute.c:118), got %u", nchannel); }
        for(unsigned c = 0; c < nchannel; c++) {
                const j2p_plane &p = planes[c];
                if(p.w == 0 || p.h == 0 || (p.w & 7) || (p.h & 7)) {
                        return j2p_fail(J2P_EINVAL, "channel %u: coefficient plane %ux%u is not a positive multiple of 8 (box.c:6-7)", c, p.w, p.h);
                }
                if(p.w_samp == 0 || p.h_samp == 0) { return j2p_fail(J2P_EINVAL, "channel %u: zero sampling factor", c); }
                if(samples) {
                        const j2p_samples &m = samples[c];
                        if(p.data || p.fdata) { return j2p_fail(J2P_EINVAL, "channel %u: a solver made from samples takes no data / fdata (both must be NULL)", c); }
                        if(!p.quant_table) { return j2p_fail(J2P_EINVAL, "channel %u: data/quant_table is NULL", c); }
                        if(!m.data) { return j2p_fail(J2P_EINVAL, "channel %u: samples: data is NULL", c); }
                        if(m.w == 0 || m.h == 0 || m.w > p.w || m.h > p.h) {
                                return j2p_fail(J2P_EINVAL, "channel %u: samples: %ux%u samples for a coefficient plane of %ux%u", c, m.w, m.h, p.w, p.h);
                        }
                        if(m.stride_y < 1 || m.stride_x < 1) {
                                return j2p_fail(J2P_EINVAL, "channel %u: samples: strides (y, x) = (%td, %td) must be at least 1", c, m.stride_y, m.stride_x);
                        }
                }
                else if((!p.data && !from_file) || !p.quant_table) { return j2p_fail(J2P_EINVAL, "channel %u: data/quant_table is NULL", c); }
                for(int j = 0; j < 64; j++) {
                        if(p.quant_table[j] == 0) { return j2p_fail(J2P_EINVAL, "channel %u: invalid quantization table (jpeg.c:41-45)", c); }
                }
                j2p_canvas_add(cv, p.w, p.h, p.w_samp, p.h_samp);
        }
        const unsigned H = cv->H, align = cv->align;
        if(H > (unsigned)kMaxTileRows * kTY) { return j2p_fail(J2P_EINVAL, "canvas height %u exceeds %u", H, kMaxTileRows * kTY); }   // (shorter tile rows: only far below)
        const bool covers = band->row_begin == 0 && (band->row_end == 0 || band->row_end >= H);
        *is_whole = covers && !((band_local_arrays & J2P_BAND_EVEN_IF_WHOLE) && band->row_end >= H);   // (a band that names every row may stay one)
        if(covers) { *band = j2p_band{0, H}; }
        const unsigned row0 = band->row_begin, row1 = band->row_end;
        if(!*is_whole) {
                if(row0 >= row1 || row1 > H) { return j2p_fail(J2P_EINVAL, "bad band [%u,%u) for canvas height %u", row0, row1, H); }
                if(row0 % align || (row1 % align && row1 != H)) {
                        return j2p_fail(J2P_EINVAL, "band [%u,%u) must be aligned to %u rows", row0, row1, align);
                }
        }
        return J2P_OK;
}

// the solver's geometry: every channel's row windows, the strip schedule, the reductions' extents.  Pure but for the
// experiment switches read from the environment (once, here).
int place(j2p_solver *s, const j2p_plane planes[], const float pweight[], int band_local_arrays)
{
        const unsigned W = s->W, H = s->H, nchannel = s->nch;
        s->band_local = !s->whole && (band_local_arrays & J2P_BAND_LOCAL_ARRAYS) != 0;
        {
                // one projection launch per sampling class also on small canvases (J2P_OPT_MIXED_PROJECT)
                const char *env = j2p_exp_env("J2P_MIXED_PROJECT");
                if(env) { s->mixed_project = atoi(env) != 0; }
                // ... and (A/B timing): band solvers finish ||g|| with a k_norm_finish launch instead of inside k_project
                env = j2p_exp_env("J2P_BAND_NIP");
                if(env) { s->band_nip = atoi(env) != 0; }
                // ... and (A/B timing, the bits of both forms): g and the prob state in two buffers everywhere (0), or in
                // one wherever the channel is eligible, whatever the solver's size (1)
                env = j2p_exp_env("J2P_SHARE_STATE");
                if(env) { s->share_state = atoi(env) != 0; }
        }
        for(unsigned c = 0; c < nchannel; c++) {
                const j2p_plane &p = planes[c];
                ChanHost &h = s->ch[c];
                h.cw = p.w; h.ch = p.h; h.ws = p.w_samp; h.hs = p.h_samp;
                h.pweight = pweight[c];
                if(!j2p_row_window_of(h.ch, h.hs, H, s->row0, s->row0 + s->rows, s->band_local, &h)) {
                        return j2p_fail(J2P_EINVAL, "band-local arrays need every channel to cover the canvas height");
                }
                // (wide-footprint channels are 3, 4, 6 or 8 columns wide, whatever J2P_OPT_WIDE_FOOTPRINT says later)
                const bool wide = h.ws == 3 || h.ws == 4 || h.ws == 6 || h.ws == 8;
                h.shared = s->share_state && j2p_shares_state(h.cw, h.ws, h.hs, h.crow0, W, s->row0, h.pweight != 0.f, wide);
        }
        // ... and only where one buffer makes the solver's own working set fit the Infinity Cache (coefficients counted as
        // int16, as register_live_bytes does before they are known).  Past the cache it was measured both ways — 8192x4096
        // and 16384x2048, whose two x planes fill the cache exactly, lose 0.4 and 1.0 %, 8192^2 gains 0.2 % — so such
        // solvers keep the two buffers they had (profiles/r07_shared_state_ab.jsonl)
        {
                j2p_live_bytes l = {0, 0, 0, 0};
                for(unsigned c = 0; c < nchannel; c++) {
                        const ChanHost &h = s->ch[c];
                        j2p_live_bytes_add(&l, (size_t)(s->rows + 2 * kHalo) * W, (size_t)s->rows * W, (size_t)(h.crows ? h.crows : 1) * h.cw, sizeof(int16_t), h.shared);
                }
                if(j2p_nt_level(&l, kNtWorkingSet) != 0 && !j2p_exp_env("J2P_SHARE_STATE")) {
                        for(unsigned c = 0; c < nchannel; c++) { s->ch[c].shared = false; }
                }
        }
        // reductions: tile rows are counted on the canvas, the band owns a contiguous range
        j2p_strip_schedule sched = j2p_strip_schedule_of(W, H, s->rows, nchannel);
        // (timing experiments: J2P_RPW = 2 ... 64 for every solver of the process; band solvers take
        // only the divisors of the band alignment, 16 — tools/rpw_fine.py sweeps the rest on whole canvases)
        if(const char *env = j2p_exp_env("J2P_RPW")) {
                const int v = atoi(env);
                if(v >= 2 && v <= 64 && (s->whole || kTY % v == 0)) {
                        sched.rpw = (unsigned)v;
                        j2p_zone_shares(&sched, s->rows, nchannel);
                }
        }
        // (halves need two groups of four rows per tile row, quarters four: march_rows)
        const unsigned g = sched.rpw;
        if(const char *env = j2p_exp_env("J2P_ZONE_B")) { if(nchannel == 1 && g >= 8) { sched.zone_b = (unsigned)atoi(env); } }
        if(const char *env = j2p_exp_env("J2P_ZONE_C")) { if(nchannel == 1 && g >= 16) { sched.zone_c = (unsigned)atoi(env); } }
        if(const char *env = j2p_exp_env("J2P_ZONE_D")) { if(nchannel == 1 && g >= 8) { sched.zone_d = (unsigned)atoi(env); } }
        j2p_zone_clamp(&sched);
        s->rpw = sched.rpw;
        s->ntx = sched.strips;
        s->zone_d = sched.zone_d; s->zone_b = sched.zone_b; s->zone_c = sched.zone_c;
        s->nseg = (s->rows + s->rpw - 1) / s->rpw;
        s->ntr_local = s->nseg;
        s->ntr_global = (H + s->rpw - 1) / s->rpw;
        s->first_tr = s->row0 / s->rpw;
        norm_defaults(s);
        for(unsigned c = 0; c < nchannel; c++) {
                const ChanHost &h = s->ch[c];
                const unsigned strips = ((W + 64 * h.ws - 1) / (64 * h.ws)) * ((s->rows + 8 * h.hs - 1) / (8 * h.hs));
                if(strips > s->strips_stride) { s->strips_stride = strips; }
        }
        return J2P_OK;
}

// floats of one x buffer: the solver's rows with a halo above and below
size_t plane_floats_of(const j2p_solver *s) { return (size_t)(s->rows + 2 * kHalo) * s->W; }

// one arena for everything (sizes first, then the pointers)
int carve_arena(j2p_solver *s, const j2p_plane planes[])
{
        const int device = s->device;
        const unsigned W = s->W, nchannel = s->nch, max_strips = s->strips_stride;
        const size_t ntiles = (size_t)s->ntx * s->ntr_local, plane_floats = plane_floats_of(s);
        float *q_all = nullptr;
        Carver carve;
        for(int pass = 0; pass < 2; pass++) {
                if(pass == 1) {
                        HIP_TRY(j2p_pool_take(device, carve.used + 256, &s->arena, &s->arena_bytes));
                        s->arena_used = carve.used;
                        carve.base = static_cast<char *>(s->arena);
                        carve.used = 0;
                }
                for(unsigned c = 0; c < nchannel; c++) {
                        ChanHost &h = s->ch[c];
                        carve.take(h.xbuf[0], plane_floats);
                        carve.take(h.xbuf[1], plane_floats);
                        carve.take(h.grad, (size_t)s->rows * W);
                        // the prob state always has at least one (zero) row: the gradient kernel reads it unconditionally;
                        // a shared channel's is the gradient's buffer (same pitch, same first row: the same offsets)
                        if(h.shared) { h.pg = h.grad; }
                        else { carve.take(h.pg, (size_t)(h.crows ? h.crows : 1) * h.cw); }
                        carve.take(h.decoded, (size_t)h.frows * h.cw);
                        carve.take(h.d, (size_t)(h.crows ? h.crows : 1) * h.cw);
                        carve.take(h.d8, (size_t)(h.crows ? h.crows : 1) * h.cw);
                        // device-side decode of a band's input window (own rows + halo rows, rounded out to whole
                        // block rows) normally borrows the two x buffers as scratch; a band of only a few rows is
                        // smaller than that window, and gets scratch of its own
                        if(!planes[c].fdata) {
                                const size_t cells = (size_t)((h.frow0 + h.frows + 7) / 8 - h.frow0 / 8) * 8 * h.cw;
                                if(cells > plane_floats) {
                                        carve.take(h.scratch_f, cells);
                                        carve.take(h.scratch_d, cells);
                                }
                        }
                }
                carve.take(q_all, 64 * kMaxCh);
                carve.take(s->part_g2, ntiles * nchannel);
                carve.take(s->rowsum_local, (size_t)s->ntr_local * nchannel);
                if(s->whole) {
                        s->rowsum_all = s->rowsum_local;
                } else {
                        carve.take(s->rowsum_all, (size_t)s->ntr_global * nchannel);
                        carve.take(s->rowsum_all_odd, (size_t)s->ntr_global * nchannel);
                        carve.take(s->push_dev, 2);
                        carve.take(s->rowsum_odd, (size_t)s->ntr_local * nchannel);
                }
                carve.take(s->norm, kMaxCh);
                carve.take(s->tickets, (size_t)s->ntr_local + 1);
                carve.take(s->dbg_counters, 3);
                carve.take(s->d_maxabs, kMaxCh);
                carve.take(s->d_clipped, kMaxCh);
                carve.take(s->part_tv, ntiles * 2);
                carve.take(s->part_prob, (size_t)max_strips * nchannel);
        }
        for(unsigned c = 0; c < nchannel; c++) { s->ch[c].q = q_all + 64 * c; }
        return J2P_OK;
}

// J2P_OPT_PHASE_ORDER / J2P_PHASE_ORDER: value = J2P_PHASE_ORDER(gradient, project); negative: back to the policy; false: no such order
bool force_phase_order(j2p_solver *s, int value)
{
        if(value < 0) {
                s->order = j2p_phase_order_of(s->live.working_set, s->live.planes, kNtWorkingSet, s->W, s->rows, !s->whole);
                return true;
        }
        if(value > J2P_PHASE_ORDER(J2P_ORDER_REVERSE, J2P_ORDER_REVERSE)) { return false; }
        s->order.gradient = (unsigned)value & 1u;
        s->order.project = (unsigned)value >> 1;
        return true;
}

// nt_policy (see nt_policy() above): this solver's bytes join the device's live total
void register_live_bytes(j2p_solver *s)
{
        const size_t plane_floats = plane_floats_of(s);
        j2p_live_bytes l = {0, 0, 0, 0};
        for(unsigned c = 0; c < s->nch; c++) {
                const ChanHost &h = s->ch[c];
                const size_t cells = (size_t)(h.crows ? h.crows : 1) * h.cw;
                // (a shared buffer counts once and is not "g": j2p_live_bytes_add)
                j2p_live_bytes_add(&l, plane_floats, (size_t)s->rows * s->W, cells, sizeof(int16_t), h.shared);
        }
        s->live.working_set = l.working_set;
        s->live.g = l.g;
        s->live.planes = l.planes;
        s->live.d = l.d;
        j2p_live_add(s->device, s->live, +1);
        s->live_registered = true;
        s->nt = nt_policy(s);
        // which way every XCD walks its run of each phase.  Schedule only: the bits do not depend on who marches a row when.
        s->order = j2p_phase_order_of(s->live.working_set, s->live.planes, kNtWorkingSet, s->W, s->rows, !s->whole);
        if(const char *env = j2p_exp_env("J2P_GRAD_REVERSE")) { s->order.gradient = atoi(env) != 0 ? J2P_ORDER_REVERSE : J2P_ORDER_FORWARD; }
        // (read by the release library too: the benchmark can then be run in either order as it stands)
        if(const char *env = getenv("J2P_PHASE_ORDER")) { force_phase_order(s, atoi(env)); }
}

// the quantization tables go up, the counters start at zero.  qf: 64 * kMaxCh floats of the caller's that stay until the
// stream has been synchronised (decide_narrow_and_wide)
int upload_tables(j2p_solver *s, const j2p_plane planes[], float qf[])
{
        const unsigned nchannel = s->nch, max_strips = s->strips_stride;
        float *q_all = s->ch[0].q;
        for(unsigned c = 0; c < nchannel; c++) {
                for(int j = 0; j < 64; j++) { qf[64 * c + j] = (float)planes[c].quant_table[j]; }
        }
        HIP_TRY(hipMemcpyAsync(q_all, qf, sizeof(float) * 64 * nchannel, hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemsetAsync(s->tickets, 0, ((size_t)s->ntr_local + 1) * sizeof(unsigned), s->stream));
        HIP_TRY(hipMemsetAsync(s->part_prob, 0, (size_t)max_strips * nchannel * sizeof(double), s->stream));
        HIP_TRY(hipMemsetAsync(s->dbg_counters, 0, 3 * sizeof(unsigned long long), s->stream));
        HIP_TRY(hipMemsetAsync(s->d_maxabs, 0, kMaxCh * sizeof(unsigned), s->stream));
        HIP_TRY(hipMemsetAsync(s->d_clipped, 0, kMaxCh * sizeof(unsigned long long), s->stream));
        return J2P_OK;
}

// a channel's samples and where they are: device memory of the solver's device (read in place) or host memory (staged)
struct SampleSource {
        j2p_samples m;
        bool on_device;
};

// the sample source of upload_channel: channel c's coefficients are computed into h.d from 8-bit samples
// (k_samples_to_coefficients) instead of copied.  Device samples are read in place on the solver's stream; host samples
// are staged through the channel's first x buffer — not initialised yet, as the decode scratch below — with one 2-D copy
int samples_to_coefficients(j2p_solver *s, unsigned c, const SampleSource &src)
{
        ChanHost &h = s->ch[c];
        j2p_samples m = src.m;
        if(!src.on_device) {
                // rows of (w - 1) * stride_x + 1 bytes at a pitch that keeps every row 8-byte aligned
                const size_t row_bytes = (size_t)(m.w - 1) * (size_t)m.stride_x + 1, pitch = (row_bytes + 7) & ~(size_t)7;
                if(pitch * m.h > plane_floats_of(s) * sizeof(float)) {
                        return j2p_fail(J2P_EINVAL, "channel %u: samples: host samples with stride_x %td do not fit the staging buffer", c, m.stride_x);
                }
                uint8_t *stage = reinterpret_cast<uint8_t *>(h.xbuf[0]);
                // (a plain 1-D copy for rows that already lie at the staging pitch measured the same: DESIGN.md section 19)
                if((size_t)m.stride_y >= row_bytes) {
                        HIP_TRY(hipMemcpy2DAsync(stage, pitch, m.data, (size_t)m.stride_y, row_bytes, m.h, hipMemcpyHostToDevice, s->stream));
                } else {
                        // (rows that overlap in memory: no 2-D copy describes them)
                        for(unsigned y = 0; y < m.h; y++) {
                                HIP_TRY(hipMemcpyAsync(stage + y * pitch, m.data + (size_t)y * (size_t)m.stride_y, row_bytes, hipMemcpyHostToDevice, s->stream));
                        }
                }
                m.data = stage;
                m.stride_y = (ptrdiff_t)pitch;
        }
        const unsigned blocks_w = h.cw / 8, block_rows = h.ch / 8;
        const unsigned groups = ((blocks_w + 7) / 8) * block_rows;
        const int wide = m.stride_x == 1 && ((reinterpret_cast<uintptr_t>(m.data) | (uintptr_t)m.stride_y) & 7) == 0;
        hipLaunchKernelGGL(k_samples_to_coefficients, dim3((groups + 3) / 4), dim3(256), 0, s->stream, m.data, m.w, m.h, m.stride_y, m.stride_x,
                           wide, blocks_w, block_rows, (const float *)h.q, h.d, s->d_clipped + c);
        HIP_TRY(hipGetLastError());
        return J2P_OK;
}

// one channel's coefficients go up (host arrays: whole-image unless band_local; or are computed from samples, m != NULL; or
// are `resident` already, decoded from a file: j2p_decode_file) and are narrowed to bytes; its input window goes up decoded,
// or is decoded here
int upload_channel(j2p_solver *s, unsigned c, const j2p_plane &p, const SampleSource *m, bool resident)
{
        ChanHost &h = s->ch[c];
        const size_t plane_floats = plane_floats_of(s);
        const size_t host_row0 = s->band_local ? h.crow0 : 0;
        if(m) {
                // (whole canvases only: h.d holds every block row, and the decode below finds its window there)
                const int rc = samples_to_coefficients(s, c, *m);
                if(rc != J2P_OK) { return rc; }
        }
        if(h.crows) {
                // block-major: coefficient row r lives in block row r/8; rows are block aligned
                if(!m && !resident) {
                        const int16_t *src = p.data + (size_t)(h.crow0 - host_row0) * h.cw;
                        HIP_TRY(hipMemcpyAsync(h.d, src, (size_t)h.crows * h.cw * sizeof(int16_t), hipMemcpyHostToDevice, s->stream));
                }
                // ... and once more as bytes, with the largest |d| (decide_narrow_and_wide reads it back)
                const size_t cells = (size_t)h.crows * h.cw;
                const unsigned blocks = (unsigned)((cells / 8 + 255) / 256);
                hipLaunchKernelGGL(k_narrow_coefficients, dim3(blocks < 2048 ? (blocks ? blocks : 1) : 2048), dim3(256), 0, s->stream,
                                   (const int16_t *)h.d, h.d8, cells, s->d_maxabs + c);
        }
        if(p.fdata) {
                const float *src = p.fdata + (size_t)(h.frow0 - host_row0) * h.cw;
                HIP_TRY(hipMemcpyAsync(h.decoded, src, (size_t)h.frows * h.cw * sizeof(float), hipMemcpyHostToDevice, s->stream));
                return J2P_OK;
        }
        // decode on the device (jpeg.c:83-92 + box.c:5-19): whole block rows [b0, b1) of the input
        // window.  Band rows are block aligned, so when the window has no halo rows (band_local, or
        // a whole canvas) the blocks are already in h.d; otherwise the coefficients of the
        // window go up once more into the (not yet initialised) gradient plane as scratch.
        const unsigned b0 = h.frow0 / 8, b1 = (h.frow0 + h.frows + 7) / 8;
        const unsigned nb_rows = b1 - b0;
        const unsigned groups = ((h.cw / 8 + 7) / 8) * nb_rows;
        // (cannot fire: carve_arena gave the channel scratch of its own exactly when the window's floats exceed an x
        // buffer, and the int16 window is half of them)
        if(!h.scratch_f && (size_t)nb_rows * 8 * h.cw > plane_floats) {
                return j2p_fail(J2P_EINVAL, "channel %u: decode window does not fit the scratch plane", c);
        }
        const int16_t *dsrc = nullptr;
        if(h.crows && b0 * 8 >= h.crow0 && b1 * 8 <= h.crow0 + h.crows) {
                dsrc = h.d + (size_t)(b0 * 8 - h.crow0) * h.cw;
        } else {
                // scratch: the first x buffer holds (rows + 4) * W floats >= the window's int16 data
                int16_t *dtmp = h.scratch_d ? h.scratch_d : reinterpret_cast<int16_t *>(h.xbuf[0]);
                const int16_t *src = p.data + (size_t)(b0 * 8 - host_row0) * h.cw;
                HIP_TRY(hipMemcpyAsync(dtmp, src, (size_t)nb_rows * 8 * h.cw * sizeof(int16_t), hipMemcpyHostToDevice, s->stream));
                dsrc = dtmp;
        }
        if(h.frow0 == b0 * 8 && h.frows == nb_rows * 8) {
                hipLaunchKernelGGL(k_decode, dim3((groups + 3) / 4), dim3(256), 0, s->stream, dsrc,
                                   (const float *)h.q, h.decoded, h.cw, nb_rows);
        } else {
                // window not block aligned (halo rows of a band): decode into the second x buffer, copy the rows
                float *ftmp = h.scratch_f ? h.scratch_f : h.xbuf[1];
                hipLaunchKernelGGL(k_decode, dim3((groups + 3) / 4), dim3(256), 0, s->stream, dsrc,
                                   (const float *)h.q, ftmp, h.cw, nb_rows);
                HIP_TRY(hipMemcpyAsync(h.decoded, ftmp + (size_t)(h.frow0 - b0 * 8) * h.cw,
                                       (size_t)h.frows * h.cw * sizeof(float), hipMemcpyDeviceToDevice, s->stream));
        }
        HIP_TRY(hipGetLastError());
        return J2P_OK;
}

// waits for the uploads, then decides per channel what the projection reads: bytes where the values allow, and the
// wide-footprint path for the footprints it has
int decide_narrow_and_wide(j2p_solver *s)
{
        // (the largest |d| per channel comes back on the solver's own stream: a synchronous copy would wait for every
        // blocking stream of the device)
        unsigned maxabs[kMaxCh] = {0};
        HIP_TRY(hipMemcpyAsync(maxabs, s->d_maxabs, sizeof(maxabs), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(s->clipped, s->d_clipped, sizeof(s->clipped), hipMemcpyDeviceToHost, s->stream));
        // the host arrays (and j2p_solver_create's stack table) may go away as soon as this returns
        HIP_TRY(hipStreamSynchronize(s->stream));
        {
                // one byte per coefficient where the channel's values allow it: the projection then reads d8 (ChanDev::d8)
                const char *env = j2p_exp_env("J2P_NARROW_COEFFICIENTS");
                for(unsigned c = 0; c < s->nch; c++) {
                        ChanHost &h = s->ch[c];
                        h.narrow_fits = h.crows != 0 && maxabs[c] <= 127;
                        h.narrow = h.narrow_fits && !(env && atoi(env) == 0);
                }
                account_coefficient_bytes(s);
        }
        {
                // the wide-footprint projection path for the footprints it has (J2P_OPT_WIDE_FOOTPRINT)
                const char *env = j2p_exp_env("J2P_WIDE_FOOTPRINT");
                s->wide_footprint = !(env && atoi(env) == 0);
                set_wide_footprint(s);
        }
        return J2P_OK;
}

struct DestroySolver {
        void operator()(j2p_solver *s) const { j2p_solver_destroy(s); }
};

}  // namespace

extern "C" {

const char *j2p_version(void) { return "jpeg2png_amd 0.1 (gfx950)"; }
const char *j2p_last_error(void) { return g_err; }
void j2p_set_last_error(const char *msg) { snprintf(g_err, sizeof(g_err), "%s", msg ? msg : ""); }   // (for compute_host.c; not in the header)

// test hook: the n-th j2p_solver_run / j2p_tiled_run from now on fails with J2P_EDEVICE before it queues anything
// (0 = disarm) — how tests/test_capi_gpu.py makes a solve fail after create
static std::atomic<int> g_fail_run{0}, g_fail_band{0};
void j2p_debug_fail_run_after(int n)
{
        g_fail_run.store(n > 0 ? n : 0);
        g_fail_band.store(n < 0 ? -n : 0);
}

int j2p_device_count(int *count)
{
        if(!count) { return j2p_fail(J2P_EINVAL, "count is NULL"); }
        int n = 0;
        if(hipGetDeviceCount(&n) != hipSuccess) { n = 0; }
        *count = n;
        return J2P_OK;
}

void j2p_solver_destroy(j2p_solver *s)
{
        if(!s) { return; }
        DeviceGuard guard(s->device);
        if(s->stream) { (void)hipStreamSynchronize(s->stream); }
        if(s->live_registered) { j2p_live_add(s->device, s->live, -1); }
        j2p_pool_give(s->device, s->arena, s->arena_bytes);
        j2p_pool_give(s->device, s->out_scratch, s->out_scratch_bytes);
        j2p_pool_give(s->device, s->upright, s->upright_bytes);
        (void)hipFree(s->logsums);
        (void)hipFree(s->log_band);
        (void)hipFree(s->trace);
        for(hipEvent_t e : s->ev) { (void)hipEventDestroy(e); }
        if(s->own_stream && s->stream) { (void)hipStreamDestroy(s->stream); }
        delete s;
}

// a JPEG file as the source of a solver's coefficients: its parse, the scan's bytes and where they are — or, parsed == NULL, the
// grids a decode of the file has already left in device memory (a batch job decodes once for all its solvers), copied on the device
struct FileSource {
        const j2p_jpeg_parsed *parsed;
        const uint8_t *data;
        bool on_device;
        const int16_t *decoded[3];
        const j2p_jpeg_file *opened = nullptr;          // parsed == NULL too: a file opened by j2p_jpeg_open_scans, decoded by j2p_decode_opened
};

// j2p_solver_create, and — samples != NULL — j2p_solver_create_from_samples, and — file != NULL — j2p_solver_create_from_jpeg:
// the same stages, with the sample source or the file's decode in the upload stage
static int create_solver(j2p_solver **out, int device, void *stream, unsigned nchannel, const j2p_plane planes[], const j2p_samples samples[],
                         const FileSource *file, float weight, const float pweight[], unsigned iterations, j2p_band band, int band_local_arrays)
{
        if(!out) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        *out = nullptr;
        if(!planes || !pweight) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        j2p_canvas cv = J2P_CANVAS_NONE;
        bool whole = true;
        int rc = validate(nchannel, planes, samples, file != nullptr, band_local_arrays, &cv, &band, &whole);
        if(rc != J2P_OK) { return rc; }
        int ndev = 0;
        if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
                return j2p_fail(J2P_EDEVICE, "no HIP device available: the jpeg2png_amd solver has no CPU fallback");
        }
        if(device < 0 || device >= ndev) { return j2p_fail(J2P_EINVAL, "device %d out of range (0..%d)", device, ndev - 1); }
        DeviceGuard guard(device);
        if(!guard.ok) { return j2p_fail(J2P_EDEVICE, "hipSetDevice(%d) failed", device); }
        // where the samples are: this device's memory or the host's; nothing else (before anything is made or queued)
        SampleSource sources[kMaxCh];
        for(unsigned c = 0; samples && c < nchannel; c++) {
                int where = -1;
                const int kind = j2p_memory_of_pointer(samples[c].data, &where);
                if(kind == J2P_MEMORY_OTHER || (kind == J2P_MEMORY_DEVICE && where != device)) {
                        return j2p_fail(J2P_EINVAL, "channel %u: samples: data is neither host memory nor device memory of device %d (managed memory and other GPUs' are refused)", c, device);
                }
                sources[c] = SampleSource{samples[c], kind == J2P_MEMORY_DEVICE};
        }
        if(allow_k_norm_whole_lds() != hipSuccess) {
                return j2p_fail(J2P_EDEVICE, "hipFuncSetAttribute(k_norm_whole, %u bytes of LDS) failed", kNormLdsBytes);
        }
        // the half-built solver is destroyed by every return but the last
        std::unique_ptr<j2p_solver, DestroySolver> owner(new(std::nothrow) j2p_solver());
        j2p_solver *s = owner.get();
        if(!s) { return j2p_fail(J2P_ENOMEM, "host allocation failed"); }
        s->device = device;
        s->nch = nchannel;
        s->W = cv.W;
        s->H = cv.H;
        s->row0 = band.row_begin;
        s->rows = band.row_end - band.row_begin;
        s->whole = whole;
        s->weight = weight;
        s->iterations = iterations;
        s->sampled = samples != nullptr;
        if(stream) { s->stream = (hipStream_t)stream; }
        else {
                HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
                s->own_stream = true;
        }
        float qf[64 * kMaxCh];
        rc = place(s, planes, pweight, band_local_arrays);
        if(rc == J2P_OK) { rc = carve_arena(s, planes); }
        if(rc == J2P_OK) {
                register_live_bytes(s);
                rc = upload_tables(s, planes, qf);
        }
        if(rc == J2P_OK && file) {
                // (a whole canvas: every channel's resident buffer is its component's whole grid)
                int16_t *grids[3] = {nullptr, nullptr, nullptr};
                for(unsigned c = 0; c < nchannel; c++) { grids[c] = s->ch[c].d; }
                if(file->opened) {
                        rc = j2p_decode_opened(device, s->stream, *file->opened, 0, grids, nullptr, nullptr);
                } else if(file->parsed) {
                        rc = j2p_decode_file(device, s->stream, file->parsed, file->data, file->on_device, 0, grids, nullptr);
                } else {
                        for(unsigned c = 0; c < nchannel; c++) {
                                const ChanHost &h = s->ch[c];
                                HIP_TRY(hipMemcpyAsync(h.d, file->decoded[c], (size_t)h.crows * h.cw * sizeof(int16_t), hipMemcpyDeviceToDevice, s->stream));
                        }
                }
        }
        for(unsigned c = 0; rc == J2P_OK && c < nchannel; c++) {
                rc = upload_channel(s, c, planes[c], samples ? &sources[c] : nullptr, file != nullptr);
        }
        if(rc == J2P_OK) { rc = decide_narrow_and_wide(s); }
        if(rc == J2P_OK) { rc = launch_init(s); }
        if(rc != J2P_OK) { return rc; }
        *out = owner.release();
        return J2P_OK;
}

int j2p_solver_create(j2p_solver **out, int device, void *stream, unsigned nchannel, const j2p_plane planes[],
                      float weight, const float pweight[], unsigned iterations, j2p_band band, int band_local_arrays)
{
        return create_solver(out, device, stream, nchannel, planes, nullptr, nullptr, weight, pweight, iterations, band, band_local_arrays);
}

int j2p_solver_create_from_samples(j2p_solver **out, int device, void *stream, unsigned nchannel, const j2p_plane planes[],
                                   const j2p_samples samples[], float weight, const float pweight[], unsigned iterations)
{
        if(out) { *out = nullptr; }
        if(!samples) { return j2p_fail(J2P_EINVAL, "samples is NULL"); }
        const j2p_band whole = {0, 0};
        return create_solver(out, device, stream, nchannel, planes, samples, nullptr, weight, pweight, iterations, whole, 0);
}

int j2p_solver_create_from_jpeg(j2p_solver **out, int device, void *stream, const uint8_t *file, size_t size, float weight, const float pweight[],
                                unsigned iterations, j2p_jpeg_info *info)
{
        if(out) { *out = nullptr; }
        if(!out || !pweight) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        j2p_jpeg_file opened;
        if(const int rc = j2p_jpeg_open(file, size, &opened); rc != J2P_OK) { return rc; }
        if(opened.on_device && opened.device != device) {
                return j2p_fail(J2P_EINVAL, "jpeg: the file lies on device %d, the solver on %d", opened.device, device);
        }
        const j2p_jpeg_info &f = opened.parsed->info;
        j2p_plane planes[3];
        memset(planes, 0, sizeof(planes));
        for(unsigned c = 0; c < f.ncomp; c++) {
                planes[c].w = f.comp[c].blocks_w * 8;
                planes[c].h = f.comp[c].blocks_h * 8;
                planes[c].w_samp = f.comp[c].w_samp;
                planes[c].h_samp = f.comp[c].h_samp;
                planes[c].quant_table = f.comp[c].quant;
        }
        const FileSource source = {opened.parsed.get(), opened.scan, opened.on_device, {nullptr, nullptr, nullptr}};
        const j2p_band whole = {0, 0};
        const int rc = create_solver(out, device, stream, f.ncomp, planes, nullptr, &source, weight, pweight, iterations, whole, 0);
        if(rc == J2P_OK && info) { *info = f; }
        return rc;
}

int j2p_solver_create_from_jpeg_scans(j2p_solver **out, int device, void *stream, const uint8_t *file, size_t size, float weight,
                                      const float pweight[], unsigned iterations, j2p_jpeg_info *info)
{
        if(out) { *out = nullptr; }
        if(!out || !pweight) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        j2p_jpeg_file opened;
        if(const int rc = j2p_jpeg_open_scans(file, size, &opened); rc != J2P_OK) { return rc; }
        if(opened.on_device && opened.device != device) {
                return j2p_fail(J2P_EINVAL, "jpeg: the file lies on device %d, the solver on %d", opened.device, device);
        }
        const j2p_jpeg_info &f = opened.info();
        j2p_plane planes[3];
        memset(planes, 0, sizeof(planes));
        for(unsigned c = 0; c < f.ncomp; c++) {
                planes[c].w = f.comp[c].blocks_w * 8;
                planes[c].h = f.comp[c].blocks_h * 8;
                planes[c].w_samp = f.comp[c].w_samp;
                planes[c].h_samp = f.comp[c].h_samp;
                planes[c].quant_table = f.comp[c].quant;
        }
        FileSource source = {nullptr, opened.scan, opened.on_device, {nullptr, nullptr, nullptr}};
        source.opened = &opened;
        const j2p_band whole = {0, 0};
        const int rc = create_solver(out, device, stream, f.ncomp, planes, nullptr, &source, weight, pweight, iterations, whole, 0);
        if(rc == J2P_OK && info) { *info = f; }
        return rc;
}

}  // extern "C"

int j2p_solver_create_from_decoded(j2p_solver **out, int device, unsigned nchannel, const j2p_plane planes[], const int16_t *const decoded[],
                                   float weight, const float pweight[], unsigned iterations)
{
        if(out) { *out = nullptr; }
        if(!decoded) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        FileSource source = {nullptr, nullptr, true, {nullptr, nullptr, nullptr}};
        for(unsigned c = 0; c < nchannel && c < 3; c++) { source.decoded[c] = decoded[c]; }
        const j2p_band whole = {0, 0};
        return create_solver(out, device, nullptr, nchannel, planes, nullptr, &source, weight, pweight, iterations, whole, 0);
}

extern "C" {

int j2p_solver_clipped_samples(const j2p_solver *s, unsigned c, unsigned long long *count)
{
        if(!s || !count || c >= s->nch) { return j2p_fail(J2P_EINVAL, "j2p_solver_clipped_samples: bad argument"); }
        if(!s->sampled) { return j2p_fail(J2P_ESTATE, "j2p_solver_clipped_samples: the solver was not made from samples"); }
        *count = s->clipped[c];
        return J2P_OK;
}

int j2p_solver_download_coefficients(j2p_solver *s, unsigned c, int16_t *out_host)
{
        if(!s || !out_host || c >= s->nch) { return j2p_fail(J2P_EINVAL, "j2p_solver_download_coefficients: bad argument"); }
        const ChanHost &h = s->ch[c];
        if(!h.crows) { return J2P_OK; }          // (a band below the channel's last row holds none)
        DeviceGuard guard(s->device);
        HIP_TRY(hipMemcpyAsync(out_host, h.d, (size_t)h.crows * h.cw * sizeof(int16_t), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        return J2P_OK;
}

int j2p_solver_debug_option(j2p_solver *s, int option, int value)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        if(s->grad_done || s->interior_done) { return j2p_fail(J2P_ESTATE, "options change between iterations only"); }
        switch(option) {
        case J2P_OPT_NORM_FOLD:
                if((s->rowsum_alternate || s->linked) && !value) { return j2p_fail(J2P_ESTATE, "alternating / pushed row sums need the folded norm reduction"); }
                if(value && !s->fold) {
                        // (the slots must not carry the coming iteration's parity yet, see launch_init)
                        DeviceGuard guard(s->device);
                        HIP_TRY(hipMemsetAsync(s->part_g2, (s->iter & 1) ? 0x00 : 0xff, (size_t)s->ntx * s->ntr_local * s->nch * sizeof(double), s->stream));
                }
                // 0: reduction launch between the phases; 1: folded into k_gradient by tickets
                if(value != 0 && value != 1) { return j2p_fail(J2P_EINVAL, "J2P_OPT_NORM_FOLD is 0 or 1"); }
                s->fold = value == 1;
                break;
        case J2P_OPT_NORM_IN_PROJECT:
                // 0: off; 1: the per-wavefront tree; 2: the per-workgroup tree; (needs NORM_FOLD)
                s->nip_form = value == 0 ? 0 : (value == 2 ? 2 : 1);
                break;
        case J2P_OPT_NT_GRADIENT:
                s->nt_forced = value >= 0;                 // negative: back to the policy
                s->nt = value < 0 ? nt_policy(s) : (value > 3 ? 3 : value);
                break;
        case J2P_OPT_MIXED_PROJECT: s->mixed_project = value != 0; break;
        case J2P_OPT_NARROW_COEFFICIENTS:
                for(unsigned c = 0; c < s->nch; c++) { s->ch[c].narrow = value != 0 && s->ch[c].narrow_fits; }
                account_coefficient_bytes(s);
                break;
        case J2P_OPT_WIDE_FOOTPRINT:
                s->wide_footprint = value != 0;
                set_wide_footprint(s);
                break;
        case J2P_OPT_PHASE_ORDER:
                if(!force_phase_order(s, value)) { return j2p_fail(J2P_EINVAL, "J2P_OPT_PHASE_ORDER is J2P_PHASE_ORDER(gradient, project) of J2P_ORDER_* values, or negative"); }
                break;
        default: return j2p_fail(J2P_EINVAL, "unknown option %d", option);
        }
        return J2P_OK;
}

int j2p_solver_phase_order(const j2p_solver *s, unsigned *gradient, unsigned *project)
{
        if(!s || !gradient || !project) { return j2p_fail(J2P_EINVAL, "j2p_solver_phase_order: bad argument"); }
        *gradient = s->order.gradient;
        *project = s->order.project;
        return J2P_OK;
}

int j2p_solver_coefficient_bytes(const j2p_solver *s, unsigned c, unsigned *bytes)
{
        if(!s || !bytes || c >= s->nch) { return j2p_fail(J2P_EINVAL, "j2p_solver_coefficient_bytes: bad argument"); }
        *bytes = s->ch[c].narrow ? 1u : 2u;
        return J2P_OK;
}

int j2p_solver_shares_state(const j2p_solver *s, unsigned c, int *shared)
{
        if(!s || !shared || c >= s->nch) { return j2p_fail(J2P_EINVAL, "j2p_solver_shares_state: bad argument"); }
        *shared = s->ch[c].shared ? 1 : 0;
        return J2P_OK;
}

int j2p_solver_arena_bytes(const j2p_solver *s, size_t *bytes)
{
        if(!s || !bytes) { return j2p_fail(J2P_EINVAL, "j2p_solver_arena_bytes: bad argument"); }
        *bytes = s->arena_used;
        return J2P_OK;
}

int j2p_solver_output_scratch_bytes(const j2p_solver *s, size_t *bytes)
{
        if(!s || !bytes) { return j2p_fail(J2P_EINVAL, "j2p_solver_output_scratch_bytes: bad argument"); }
        *bytes = s->out_scratch_bytes;
        return J2P_OK;
}

int j2p_solver_upright_bytes(const j2p_solver *s, size_t *bytes)
{
        if(!s || !bytes) { return j2p_fail(J2P_EINVAL, "j2p_solver_upright_bytes: bad argument"); }
        *bytes = s->upright_bytes;
        return J2P_OK;
}

int j2p_solver_set_orientation(j2p_solver *s, unsigned orientation, unsigned width, unsigned height)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(orientation < 1 || orientation > 8) { return j2p_fail(J2P_EINVAL, "set_orientation: orientation %u (1..8)", orientation); }
        if(width == 0 || height == 0 || width > s->W || height > s->H) {
                return j2p_fail(J2P_EINVAL, "set_orientation: a source image of %u x %u is not inside the canvas of %u x %u", width, height, s->W, s->H);
        }
        if(!s->whole && orientation != 1) { return j2p_fail(J2P_ESTATE, "set_orientation: a band solver has no upright output"); }
        s->orientation = orientation;
        s->orient_w = width;
        s->orient_h = height;
        return J2P_OK;
}

int j2p_solver_orientation(const j2p_solver *s, unsigned *orientation, unsigned *width, unsigned *height)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(orientation) { *orientation = s->orientation; }
        if(width) { *width = s->orient_w; }
        if(height) { *height = s->orient_h; }
        return J2P_OK;
}

int j2p_solver_wide_footprint(const j2p_solver *s, unsigned c, unsigned *on)
{
        if(!s || !on || c >= s->nch) { return j2p_fail(J2P_EINVAL, "j2p_solver_wide_footprint: bad argument"); }
        // (k_project_mixed has no wide-footprint path; NIP 2 — bands of whole phases — never takes the mixed launch)
        *on = s->ch[c].wide && !projects_mixed(s, plan_of(s, false, false).nip()) ? 1u : 0u;
        return J2P_OK;
}

int j2p_solver_trace(j2p_solver *s, int on, unsigned long long *host_out, unsigned max_records, unsigned *n)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
#ifdef J2P_TRACE
        DeviceGuard guard(s->device);
        constexpr unsigned kCap = 1u << 19;                     // records (16 MiB)
        HIP_TRY(hipStreamSynchronize(s->stream));
        if(!s->trace) {
                HIP_TRY(j2p_dev_malloc((void **)&s->trace, (size_t)kCap * 32));
                HIP_TRY(hipMemset(s->trace, 0, (size_t)kCap * 32));
                s->trace_cap = kCap;
        }
        if(host_out && n) {
                unsigned long long count = s->trace_used;
                if(count > s->trace_cap - 1) { count = s->trace_cap - 1; }
                if(count > max_records) { count = max_records; }
                HIP_TRY(hipMemcpy(host_out, s->trace + 4, (size_t)count * 32, hipMemcpyDeviceToHost));
                *n = (unsigned)count;
                HIP_TRY(hipMemset(s->trace, 0, (size_t)(count + 1) * 32));     // start over
                s->trace_used = 0;
        }
        s->trace_on = on != 0;
        return J2P_OK;
#else
        (void)on; (void)host_out; (void)max_records; (void)n;
        return j2p_fail(J2P_ESTATE, "not a J2P_TRACE build");
#endif
}

int j2p_experiments_build(void)
{
#ifdef J2P_EXPERIMENTS
        return 1;
#else
        return 0;
#endif
}

static int debug_grad_items(unsigned W, unsigned rows, unsigned rows_per_tile, unsigned channel_wavefronts, unsigned zone_d, unsigned zone_b,
                            unsigned zone_c, int reverse, unsigned *items /* [max][5]: strip, first row, rows, tile row, kind */,
                            unsigned *item_workgroup /* [max] or NULL */, unsigned max_items, unsigned *n_items, unsigned *workgroups)
{
        // the map of k_gradient's launch (grad_item) evaluated on the HOST, wavefront by wavefront: no device needed
        if(!items || !n_items || !workgroups || W < 8 || rows == 0 || rows_per_tile == 0 || channel_wavefronts < 1 || channel_wavefronts > 3) {
                return j2p_fail(J2P_EINVAL, "bad argument");
        }
        Geo g;
        memset(&g, 0, sizeof(g));
        g.W = W; g.H = rows; g.row0 = 0; g.rows = rows; g.rpw = rows_per_tile;
        g.ntx = W <= 4 ? 1u : (W - 4 + 123) / 124;
        g.seg_off = 0; g.seg_mul = 1;
        g.ntr_launch = (rows + rows_per_tile - 1) / rows_per_tile;
        const unsigned positions = g.ntx * ((g.ntr_launch + 1) / 2);
        const bool joint = channel_wavefronts > 1;
        g.units = joint ? positions : (positions + 3) / 4;
        g.zone_d = zone_d; g.zone_b = zone_b; g.zone_c = zone_c;
        g.reverse = reverse ? kOrderReverse : kOrderForward;
        const unsigned nwg = grad_grid(g.units, zone_shares(g));
        *workgroups = nwg;
        unsigned n = 0;
        for(unsigned b = 0; b < nwg; b++) {
                for(int wave = 0; wave < (joint ? 1 : 4); wave++) {
                        StripItem it;
                        const bool ok = joint ? grad_item<3>(g, b, wave, it) : grad_item<1>(g, b, wave, it);
                        if(!ok || !it.active) { continue; }
                        if(n < max_items) {
                                unsigned *o = items + 5 * (size_t)n;
                                const unsigned t1 = (unsigned)(it.t0 + it.nrows) < rows ? (unsigned)(it.t0 + it.nrows) : rows;
                                o[0] = (unsigned)it.wcol; o[1] = (unsigned)it.t0; o[2] = t1 - (unsigned)it.t0; o[3] = it.tr; o[4] = (unsigned)it.kind;
                                if(item_workgroup) { item_workgroup[n] = b; }
                        }
                        n++;
                }
        }
        *n_items = n;
        return J2P_OK;
}

int j2p_debug_grad_items(unsigned W, unsigned rows, unsigned rows_per_tile, unsigned channel_wavefronts, unsigned zone_d, unsigned zone_b,
                         unsigned zone_c, int reverse, unsigned *items, unsigned max_items, unsigned *n_items, unsigned *workgroups)
{
        return debug_grad_items(W, rows, rows_per_tile, channel_wavefronts, zone_d, zone_b, zone_c, reverse, items, nullptr, max_items, n_items, workgroups);
}

int j2p_debug_grad_items_workgroups(unsigned W, unsigned rows, unsigned rows_per_tile, unsigned channel_wavefronts, unsigned zone_d, unsigned zone_b,
                                    unsigned zone_c, int reverse, unsigned *items, unsigned *item_workgroup, unsigned max_items, unsigned *n_items,
                                    unsigned *workgroups)
{
        if(!item_workgroup) { return j2p_fail(J2P_EINVAL, "bad argument"); }
        return debug_grad_items(W, rows, rows_per_tile, channel_wavefronts, zone_d, zone_b, zone_c, reverse, items, item_workgroup, max_items, n_items, workgroups);
}

int j2p_debug_project_items(unsigned strips_x, unsigned nby, unsigned by_offset, unsigned by_mul, int order, unsigned *items /* [max][4]: workgroup, wavefront, block row, strip */,
                            unsigned max_items, unsigned *n_items, unsigned *workgroups)
{
        // the map of a projection launch (project_item and project_strip's arithmetic behind it) evaluated on the HOST
        if(!items || !n_items || !workgroups || strips_x == 0 || nby == 0 || (order != (int)kOrderForward && order != (int)kOrderReverse)) {
                return j2p_fail(J2P_EINVAL, "bad argument");
        }
        const unsigned strips = strips_x * nby, nwg = (strips + 3) / 4;     // the grid of do_phase_project
        *workgroups = nwg;
        unsigned n = 0;
        for(unsigned b = 0; b < nwg; b++) {
                for(unsigned wave = 0; wave < 4; wave++) {
                        const unsigned lstrip = project_item(b, nwg, (unsigned)order) * 4 + wave;
                        if(lstrip >= strips) { continue; }
                        if(n < max_items) {
                                unsigned *o = items + 4 * (size_t)n;
                                o[0] = b; o[1] = wave; o[2] = by_offset + (lstrip / strips_x) * by_mul; o[3] = lstrip % strips_x;
                        }
                        n++;
                }
        }
        *n_items = n;
        return J2P_OK;
}

int j2p_debug_phase_order(size_t working_set, size_t planes, unsigned W, unsigned rows, int band, unsigned *gradient, unsigned *project)
{
        if(!gradient || !project) { return j2p_fail(J2P_EINVAL, "bad argument"); }
        const j2p_phase_order o = j2p_phase_order_of(working_set, planes, kNtWorkingSet, W, rows, band);
        *gradient = o.gradient;
        *project = o.project;
        return J2P_OK;
}

int j2p_debug_norm_plan(int whole, int fold, int norm_in_project, int band_nip, unsigned tile_rows, int split, int log,
                        int *level1, int *level2, unsigned *launches)
{
        if(!level1 || !level2 || !launches || norm_in_project < 0 || norm_in_project > 2 || tile_rows == 0) { return j2p_fail(J2P_EINVAL, "bad argument"); }
        const NormPlan p = norm_plan(whole != 0, fold != 0, norm_in_project, band_nip != 0, tile_rows, split != 0, log != 0);
        *level1 = p.level1;
        *level2 = p.level2;
        *launches = 2 + p.launches();
        return J2P_OK;
}

int j2p_debug_build(void)
{
#ifdef J2P_DEBUG
        return 1;
#else
        return 0;
#endif
}

int j2p_solver_debug_violations(j2p_solver *s, unsigned long long *count, unsigned *site, unsigned long long *offset)
{
        if(!s || !count) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
#ifdef J2P_DEBUG
        unsigned long long h[3] = {0, 0, 0};
        DeviceGuard guard(s->device);
        HIP_TRY(hipStreamSynchronize(s->stream));
        HIP_TRY(hipMemcpy(h, s->dbg_counters, sizeof(h), hipMemcpyDeviceToHost));
        *count = h[0];
        if(site) { *site = (unsigned)h[1]; }
        if(offset) { *offset = h[2]; }
        return J2P_OK;
#else
        (void)site;
        (void)offset;
        return j2p_fail(J2P_ESTATE, "not a J2P_DEBUG build: the address checks are compiled out");
#endif
}

int j2p_solver_canvas(const j2p_solver *s, unsigned *W, unsigned *H)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        if(W) { *W = s->W; }
        if(H) { *H = s->H; }
        return J2P_OK;
}

int j2p_solver_band(const j2p_solver *s, unsigned *row_begin, unsigned *row_end)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        if(row_begin) { *row_begin = s->row0; }
        if(row_end) { *row_end = s->row0 + s->rows; }
        return J2P_OK;
}

int j2p_solver_launches_per_iteration(const j2p_solver *s, unsigned *n)
{
        if(!s || !n) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        // (unlogged runs of whole phases; logging adds the log kernels and moves level 2 out of k_project)
        *n = 2 + plan_of(s, false, false).launches();
        return J2P_OK;
}

int j2p_solver_reset(j2p_solver *s)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        DeviceGuard guard(s->device);
        int rc = flush_timing(s);
        if(rc != J2P_OK) { return rc; }
        if(!s->nt_forced) { s->nt = nt_policy(s); }       // other solvers may have come or gone on this device
        return launch_init(s);
}

int j2p_solver_phase_gradient(j2p_solver *s)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        DeviceGuard guard(s->device);
        return do_phase_gradient(s, s->log_phases);
}

int j2p_solver_phase_gradient_part(j2p_solver *s, int part, void *stream)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        (void)stream;
#ifndef J2P_EXPERIMENTS
        // (measured slower than whole phases wherever tried, DESIGN.md section 10: the release build keeps the entry points, not the schedule)
        (void)part;
        return j2p_fail(J2P_ESTATE, "split phases exist in the experiments build only (buildlib.build_experiments)");
#endif
        if(part != J2P_GRADIENT_INTERIOR && part != J2P_GRADIENT_EDGES) { return j2p_fail(J2P_EINVAL, "part must be J2P_GRADIENT_INTERIOR or J2P_GRADIENT_EDGES"); }
        DeviceGuard guard(s->device);
        return do_phase_gradient(s, s->log_phases, part, (hipStream_t)stream);
}

int j2p_solver_phase_rowsums(j2p_solver *s)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        DeviceGuard guard(s->device);
        return do_rowsums(s);
}

int j2p_solver_phase_project(j2p_solver *s)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        DeviceGuard guard(s->device);
        return do_phase_project(s, s->log_phases);
}

int j2p_solver_phase_project_part(j2p_solver *s, int part)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
#ifndef J2P_EXPERIMENTS
        // (measured slower than whole phases wherever tried, DESIGN.md section 10: the release build keeps the entry points, not the schedule)
        (void)part;
        return j2p_fail(J2P_ESTATE, "split phases exist in the experiments build only (buildlib.build_experiments)");
#endif
        if(part != J2P_PROJECT_BOUNDARY && part != J2P_PROJECT_INTERIOR) { return j2p_fail(J2P_EINVAL, "part must be J2P_PROJECT_BOUNDARY or J2P_PROJECT_INTERIOR"); }
        DeviceGuard guard(s->device);
        return do_phase_project(s, s->log_phases, part);
}

// log rows from per-iteration sums {tv, tv2, prob distance per channel of the state LEFT by the iteration}
// (compute.c:226-272: total_alpha in float, objective in double).  carried[] is the prob distance of the
// state entering the first of the n iterations (0 at iteration 0: cos = d*q) and is updated.
static void rows_from_sums(unsigned nch, float weight, const float *pweight, unsigned n, const double *sums,
                           double *carried, bool carried_valid, j2p_log_row *rows)
{
        constexpr unsigned kRow = 2 + kMaxCh;
        float total_alpha = 0.f;
        for(unsigned c = 0; c < nch; c++) {
                if(pweight[c] != 0.f) { total_alpha += pweight[c] * 2 * 255 * sqrtf(2); }
        }
        total_alpha += nch;
        if(weight != 0.f) { total_alpha += (weight / sqrtf((float)(4 / 2))) * nch; }
        for(unsigned i = 0; i < n; i++) {
                const double *h = &sums[(size_t)i * kRow];
                double prob = 0.;
                for(unsigned c = 0; c < nch; c++) {
                        if(pweight[c] != 0.f) { prob += 0.5 * carried[c]; }   // compute_simd_step.c:61
                }
                if(!carried_valid) { prob = NAN; }
                rows[i].tv = h[0];
                rows[i].tv2 = weight != 0.f ? h[1] : 0.;
                rows[i].prob_dist = prob;
                rows[i].objective = (rows[i].tv + rows[i].tv2 + prob) / total_alpha;
                for(unsigned c = 0; c < nch; c++) { carried[c] = h[2 + c]; }
                carried_valid = true;
        }
}

}  // extern "C"

static bool countdown(std::atomic<int> &a)
{
        int v = a.load(std::memory_order_relaxed);
        while(v > 0) {
                if(a.compare_exchange_weak(v, v - 1)) { return v == 1; }
        }
        return false;
}
bool j2p_injected_failure() { return countdown(g_fail_run); }
bool j2p_injected_band_failure() { return countdown(g_fail_band); }

void j2p_rows_from_sums_carry(unsigned nch, float weight, const float *pweight, unsigned n, const double *sums,
                              double *carried, bool carried_valid, j2p_log_row *rows)
{
        rows_from_sums(nch, weight, pweight, n, sums, carried, carried_valid, rows);
}

extern "C" {

int j2p_log_rows_from_sums(unsigned nchannel, float weight, const float pweight[], unsigned n, const double *sums,
                           j2p_log_row *rows)
{
        if(!pweight || !sums || !rows) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(nchannel == 0 || nchannel > kMaxCh) { return j2p_fail(J2P_EINVAL, "nchannel must be 1..3"); }
        double carried[kMaxCh] = {0., 0., 0.};
        rows_from_sums(nchannel, weight, pweight, n, sums, carried, true, rows);
        return J2P_OK;
}

int j2p_solver_set_logging(j2p_solver *s, int on)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        DeviceGuard guard(s->device);
        // like the schedule switches: the two phases of an iteration have to agree on it (where the norm is reduced
        // depends on it)
        if(s->grad_done || s->interior_done) { return j2p_fail(J2P_ESTATE, "logging changes between iterations only"); }
        if(on && !s->log_band) {
                HIP_TRY(j2p_dev_malloc((void **)&s->log_band, (2 + kMaxCh) * sizeof(double)));
                HIP_TRY(hipMemsetAsync(s->log_band, 0, (2 + kMaxCh) * sizeof(double), s->stream));
        }
        s->log_phases = on != 0;
        return J2P_OK;
}

int j2p_solver_run(j2p_solver *s, unsigned n, j2p_log_row *rows)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        if(!s->whole) { return j2p_fail(J2P_ESTATE, "j2p_solver_run needs a whole-canvas solver; drive bands with the phase calls"); }
        if(j2p_injected_failure()) { return j2p_fail(J2P_EDEVICE, "injected failure (j2p_debug_fail_run_after)"); }
        DeviceGuard guard(s->device);
        const bool log = rows != nullptr;
        constexpr unsigned kRow = 2 + kMaxCh;
        if(log && s->logsums_cap < n) {
                (void)hipFree(s->logsums);
                s->logsums = nullptr;
                s->logsums_cap = 0;
                HIP_TRY(j2p_dev_malloc((void **)&s->logsums, (size_t)n * kRow * sizeof(double)));
                s->logsums_cap = n;
        }
        for(unsigned i = 0; i < n; i++) {
                int rc = do_phase_gradient(s, log);
                if(rc != J2P_OK) { return rc; }
                if(log) {
                        hipLaunchKernelGGL(k_log_sums, dim3(1), dim3(256), 0, s->stream, (const double *)s->part_tv,
                                           s->ntx * s->nseg, (const double *)s->part_prob, 0u, s->strips_stride, s->nch,
                                           s->logsums + (size_t)i * kRow, 0);
                }
                rc = do_phase_project(s, log);
                if(rc != J2P_OK) { return rc; }
                if(log) {
                        hipLaunchKernelGGL(k_log_sums, dim3(1), dim3(256), 0, s->stream, (const double *)s->part_tv, 0u,
                                           (const double *)s->part_prob, s->strips_stride, s->strips_stride, s->nch,
                                           s->logsums + (size_t)i * kRow, 1);
                }
                if(s->timing && s->ev_used >= 4096) {
                        rc = flush_timing(s);
                        if(rc != J2P_OK) { return rc; }
                }
        }
        HIP_TRY(hipGetLastError());
        if(log) {
                std::vector<double> host((size_t)n * kRow);
                HIP_TRY(hipMemcpyAsync(host.data(), s->logsums, host.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
                HIP_TRY(hipStreamSynchronize(s->stream));
                float pw[kMaxCh] = {0.f, 0.f, 0.f};
                for(unsigned c = 0; c < s->nch; c++) { pw[c] = s->ch[c].pweight; }
                rows_from_sums(s->nch, s->weight, pw, n, host.data(), s->carried_prob, s->carried_valid, rows);
                s->carried_valid = true;
        } else if(n) {
                s->carried_valid = false;
        }
        return J2P_OK;
}

int j2p_solver_debug_partials(j2p_solver *s, double **part_g2, unsigned *ntx, unsigned *tile_rows_local, unsigned *rows_per_tile)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        if(part_g2) { *part_g2 = s->part_g2; }
        if(ntx) { *ntx = s->ntx; }
        if(tile_rows_local) { *tile_rows_local = s->ntr_local; }
        if(rows_per_tile) { *rows_per_tile = s->rpw; }
        return J2P_OK;
}

int j2p_solver_exchange_info(j2p_solver *s, j2p_exchange *info)
{
        if(!s || !info) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        memset(info, 0, sizeof(*info));
        info->partials_local = s->rowsum_local;
        info->local_tile_rows = s->ntr_local;
        info->partials_all = s->rowsum_all;
        info->global_tile_rows = s->ntr_global;
        info->first_tile_row = s->first_tr;
        info->halo_floats = (size_t)kHalo * s->W;
        info->log_local = s->log_band;
        for(unsigned c = 0; c < s->nch; c++) {
                // between the two parts of a split projection phase the rows to exchange are those of the
                // iterate being written (the buffers swap when the interior part is issued)
                float *base = s->ch[c].xbuf[s->proj_boundary_done ? s->cur ^ 1 : s->cur];
                info->recv_top[c] = base;
                info->send_top[c] = base + (size_t)kHalo * s->W;
                info->send_bottom[c] = base + (size_t)s->rows * s->W;
                info->recv_bottom[c] = base + (size_t)(s->rows + kHalo) * s->W;
        }
        return J2P_OK;
}

int j2p_solver_stream(j2p_solver *s, void **stream)
{
        if(!s || !stream) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        *stream = (void *)s->stream;
        return J2P_OK;
}

int j2p_solver_halo_rows(j2p_solver *s, int buffer, j2p_exchange *info)
{
        if(!s || !info || (buffer != 0 && buffer != 1)) { return j2p_fail(J2P_EINVAL, "bad argument"); }
        memset(info, 0, sizeof(*info));
        info->halo_floats = (size_t)kHalo * s->W;
        for(unsigned c = 0; c < s->nch; c++) {
                float *base = s->ch[c].xbuf[buffer];
                info->recv_top[c] = base;
                info->send_top[c] = base + (size_t)kHalo * s->W;
                info->send_bottom[c] = base + (size_t)s->rows * s->W;
                info->recv_bottom[c] = base + (size_t)(s->rows + kHalo) * s->W;
        }
        return J2P_OK;
}

int j2p_solver_alternate_rowsums(j2p_solver *s, const double *buffers[2])
{
        if(!s || !buffers) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(s->whole || !s->rowsum_odd) { return j2p_fail(J2P_ESTATE, "alternating row sums are for band solvers"); }
        if(!s->fold) { return j2p_fail(J2P_ESTATE, "alternating row sums need the folded norm reduction"); }
        if(s->linked) { return j2p_fail(J2P_ESTATE, "alternating row sums: this solver's bands are linked (its sums go to the global arrays)"); }
        s->rowsum_alternate = true;
        buffers[0] = s->rowsum_local;
        buffers[1] = s->rowsum_odd;
        return J2P_OK;
}

int j2p_solver_global_rowsums(j2p_solver *s, double *arrays[2])
{
        if(!s || !arrays) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(s->whole || !s->rowsum_all_odd) { return j2p_fail(J2P_ESTATE, "global row sums: band solvers only"); }
        arrays[0] = s->rowsum_all;
        arrays[1] = s->rowsum_all_odd;
        return J2P_OK;
}

int j2p_solver_link_bands(j2p_solver *s, const j2p_band_links *links)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        if(s->grad_done || s->interior_done) { return j2p_fail(J2P_ESTATE, "bands are linked between iterations only"); }
        if(!links) {
                s->linked = false;
                return J2P_OK;
        }
        if(s->whole) { return j2p_fail(J2P_ESTATE, "link_bands: band solvers only"); }
        if(!s->fold) { return j2p_fail(J2P_ESTATE, "link_bands needs the folded norm reduction (the row sums leave from inside k_gradient)"); }
        if(s->rowsum_alternate) { return j2p_fail(J2P_ESTATE, "link_bands: this solver's row sums already alternate for norm_from_bands"); }
        if(links->npush == 0 || links->npush > (unsigned)kMaxBands) { return j2p_fail(J2P_EINVAL, "link_bands: 1..%d bands to push to", kMaxBands); }
        if(links->ncount > (unsigned)kMaxBands) { return j2p_fail(J2P_EINVAL, "link_bands: at most %d counters", kMaxBands); }
        for(unsigned b = 0; b < links->ncount; b++) {
                if(!links->count[b]) { return j2p_fail(J2P_EINVAL, "link_bands: counter %u is NULL", b); }
        }
        bool own[2] = {false, false};
        for(int par = 0; par < 2; par++) {
                for(unsigned b = 0; b < links->npush; b++) {
                        if(!links->push[par][b]) { return j2p_fail(J2P_EINVAL, "link_bands: push target %u is NULL", b); }
                        own[par] = own[par] || links->push[par][b] == (par ? s->rowsum_all_odd : s->rowsum_all);
                }
        }
        if(!own[0] || !own[1]) { return j2p_fail(J2P_EINVAL, "link_bands: the push lists must contain this solver's own arrays"); }
        for(unsigned c = 0; c < s->nch; c++) {
                // a neighbour is given for both buffers or for neither; the band at the top / bottom of the canvas has none
                const bool up = links->up_halo[0][c] != nullptr, down = links->down_halo[0][c] != nullptr;
                if(up != (links->up_halo[1][c] != nullptr) || down != (links->down_halo[1][c] != nullptr)) {
                        return j2p_fail(J2P_EINVAL, "link_bands: channel %u: a neighbour's rows are needed for both x buffers", c);
                }
                if(up != (s->row0 > 0) || down != (s->row0 + s->rows < s->H)) {
                        return j2p_fail(J2P_EINVAL, "link_bands: channel %u: neighbours do not match the band's place in the canvas", c);
                }
        }
        // the push lists live in device memory (see GradArgs::push)
        RowsumPush host[2];
        for(int par = 0; par < 2; par++) {
                memset(&host[par], 0, sizeof(host[par]));
                host[par].n = links->npush;
                host[par].first_tr = s->first_tr;
                for(unsigned b = 0; b < links->npush; b++) { host[par].dst[b] = links->push[par][b]; }
                host[par].ncount = links->ncount;
                for(unsigned b = 0; b < links->ncount; b++) { host[par].count[b] = links->count[b]; }
        }
        {
                DeviceGuard guard(s->device);
                HIP_TRY(hipMemcpyAsync(s->push_dev, host, sizeof(host), hipMemcpyHostToDevice, s->stream));
                HIP_TRY(hipStreamSynchronize(s->stream));       // `host` is on the stack
        }
        s->links = *links;
        s->linked = true;
        return J2P_OK;
}

int j2p_solver_norm_from_bands(j2p_solver *s, unsigned nband, const double *const rowsums[], const unsigned first_tile_row[],
                               const unsigned tile_rows[], unsigned nout, float *const norm_out[])
{
        if(!s || !rowsums || !first_tile_row || !tile_rows) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(nband == 0 || nband > (unsigned)kMaxBands) { return j2p_fail(J2P_EINVAL, "1..%d bands", kMaxBands); }
        if(nout > (unsigned)kMaxBands || (nout && !norm_out)) { return j2p_fail(J2P_EINVAL, "norm_from_bands: bad output list"); }
        if(!s->grad_done || rowsums_owed(s)) { return j2p_fail(J2P_ESTATE, "norm_from_bands needs a finished gradient phase"); }
        // a whole-canvas solver above kNormInProjectPixels reduces its partials in one kernel and never forms the
        // level-1 row sums this call reads
        if(s->whole && !s->fold) { return j2p_fail(J2P_ESTATE, "norm_from_bands: this solver leaves no per-tile-row sums (whole canvas, norm folding off)"); }
        DeviceGuard guard(s->device);
        BandRowsums t;
        unsigned covered = 0;
        for(unsigned b = 0; b < nband; b++) {
                if(first_tile_row[b] + tile_rows[b] > s->ntr_global) { return j2p_fail(J2P_EINVAL, "band %u: tile rows out of range", b); }
                t.rowsum[b] = rowsums[b];
                t.first[b] = first_tile_row[b];
                t.count[b] = tile_rows[b];
                covered += tile_rows[b];
        }
        if(covered != s->ntr_global) { return j2p_fail(J2P_EINVAL, "the bands cover %u of %u tile rows", covered, s->ntr_global); }
        t.nband = nband;
        // where the float norm goes: this solver's own word(s), or the list given (every band's, this one included)
        if(nout == 0) {
                t.out[0] = s->norm;
                t.nout = 1;
        } else {
                bool own = false;
                for(unsigned b = 0; b < nout; b++) {
                        if(!norm_out[b]) { return j2p_fail(J2P_EINVAL, "norm_from_bands: output %u is NULL", b); }
                        t.out[b] = norm_out[b];
                        own = own || norm_out[b] == s->norm;
                }
                if(!own) { return j2p_fail(J2P_EINVAL, "norm_from_bands: the output list must contain the solver's own norm"); }
                t.nout = nout;
        }
        launch_k_norm_bands(s->stream, t, s->ntr_global, s->nch);
        HIP_TRY(hipGetLastError());
        // (a whole canvas whose k_project runs the tree keeps doing so: the words written here are the other bands')
        if(!(s->whole && s->plan.nip())) { s->plan.level2 = J2P_NORM_L2_EXTERNAL; }
        return J2P_OK;
}

int j2p_solver_norm_ptr(j2p_solver *s, float **norm)
{
        if(!s || !norm) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        *norm = s->norm;
        return J2P_OK;
}

int j2p_solver_norm_external(j2p_solver *s)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        if(!s->grad_done || rowsums_owed(s)) { return j2p_fail(J2P_ESTATE, "norm_external needs a finished gradient phase"); }
        if(s->whole && s->plan.nip()) { return j2p_fail(J2P_ESTATE, "norm_external: this solver reduces the norm inside its projection kernel"); }
        s->plan.level2 = J2P_NORM_L2_EXTERNAL;
        return J2P_OK;
}

int j2p_solver_copy_rows(j2p_solver *s, unsigned n, float *const dst[], const float *const src[], size_t floats)
{
        if(!s || !dst || !src) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(n == 0) { return J2P_OK; }
        if(n > 2u * kMaxCh || (floats & 1) || floats > 0xfffffffeu) { return j2p_fail(J2P_EINVAL, "copy_rows: bad count / size"); }
        DeviceGuard guard(s->device);
        RowCopies t;
        for(unsigned k = 0; k < n; k++) { t.dst[k] = dst[k]; t.src[k] = src[k]; }
        t.n = n;
        t.floats = (unsigned)floats;
        unsigned blocks = (unsigned)((floats / 2 + 255) / 256);
        if(blocks > 64) { blocks = 64; }
        hipLaunchKernelGGL(k_copy_rows, dim3(blocks ? blocks : 1), dim3(256), 0, s->stream, t);
        HIP_TRY(hipGetLastError());
        return J2P_OK;
}

int j2p_solver_commit_initial_halo(j2p_solver *s)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        if(s->iter != 0 || s->grad_done) { return j2p_fail(J2P_ESTATE, "initial halo can only be committed at iteration 0"); }
        DeviceGuard guard(s->device);
        const size_t hb = (size_t)kHalo * s->W * sizeof(float);
        for(unsigned c = 0; c < s->nch; c++) {
                float *cur = s->ch[c].xbuf[s->cur], *prev = s->ch[c].xbuf[s->cur ^ 1];
                HIP_TRY(hipMemcpyAsync(prev, cur, hb, hipMemcpyDeviceToDevice, s->stream));
                const size_t off = (size_t)(s->rows + kHalo) * s->W;
                HIP_TRY(hipMemcpyAsync(prev + off, cur + off, hb, hipMemcpyDeviceToDevice, s->stream));
        }
        return J2P_OK;
}

int j2p_solver_download(j2p_solver *s, unsigned c, float *out)
{
        if(!s || !out) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(c >= s->nch) { return j2p_fail(J2P_EINVAL, "channel %u out of range", c); }
        if(s->grad_done) { return j2p_fail(J2P_ESTATE, "download between the two phases of an iteration"); }
        DeviceGuard guard(s->device);
        const float *src = s->ch[c].xbuf[s->cur] + (size_t)kHalo * s->W;
        HIP_TRY(hipMemcpyAsync(out, src, (size_t)s->rows * s->W * sizeof(float), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        return J2P_OK;
}

int j2p_solver_download_gradient(j2p_solver *s, unsigned c, float *out)
{
        if(!s || !out) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(c >= s->nch) { return j2p_fail(J2P_EINVAL, "channel %u out of range", c); }
        DeviceGuard guard(s->device);
        HIP_TRY(hipMemcpyAsync(out, s->ch[c].grad, (size_t)s->rows * s->W * sizeof(float), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        return J2P_OK;
}

int j2p_solver_plane_ptr(j2p_solver *s, unsigned c, float **dev_ptr)
{
        if(!s || !dev_ptr) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(c >= s->nch) { return j2p_fail(J2P_EINVAL, "channel %u out of range", c); }
        *dev_ptr = s->ch[c].xbuf[s->cur] + (size_t)kHalo * s->W;
        return J2P_OK;
}

int j2p_solver_sync(j2p_solver *s)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        DeviceGuard guard(s->device);
        HIP_TRY(hipStreamSynchronize(s->stream));
        return J2P_OK;
}

int j2p_solver_enable_timing(j2p_solver *s, int on)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        DeviceGuard guard(s->device);
        int rc = flush_timing(s);
        s->timing = on > 0 ? (unsigned)on : 0u;
        s->acc_grad_ms = s->acc_proj_ms = 0.;
        s->acc_samples = 0;
        if(rc == J2P_OK && s->timing && s->ev_pair_ms == 0.) {
                // calibration: 33 records back to back on the (idle) stream; the median of the 32 intervals is what a bracket
                // of two records costs by itself
                hipEvent_t e[33];
                int made = 0;
                for(; made < 33; made++) {
                        if(hipEventCreate(&e[made]) != hipSuccess) { break; }
                }
                // (no early return in here: the events are destroyed below whatever happens)
                if(made == 33 && hipStreamSynchronize(s->stream) == hipSuccess) {
                        for(int i = 0; i < 33; i++) { (void)hipEventRecord(e[i], s->stream); }
                        if(hipStreamSynchronize(s->stream) == hipSuccess) {
                                float d[32];
                                int n = 0;
                                for(int i = 0; i < 32; i++) {
                                        if(hipEventElapsedTime(&d[n], e[i], e[i + 1]) == hipSuccess) { n++; }
                                }
                                for(int i = 1; i < n; i++) {                     // insertion sort
                                        const float v = d[i];
                                        int k = i - 1;
                                        for(; k >= 0 && d[k] > v; k--) { d[k + 1] = d[k]; }
                                        d[k + 1] = v;
                                }
                                if(n) { s->ev_pair_ms = d[n / 2]; }
                        }
                }
                for(int i = 0; i < made; i++) { (void)hipEventDestroy(e[i]); }
                (void)hipGetLastError();
        }
        return rc;
}

int j2p_solver_timing_overhead(j2p_solver *s, double *event_pair_ms)
{
        if(!s || !event_pair_ms) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        *event_pair_ms = s->ev_pair_ms;
        return J2P_OK;
}

int j2p_solver_kernel_times(j2p_solver *s, double *gradient_ms, double *project_ms, unsigned *samples)
{
        if(!s) { return j2p_fail(J2P_EINVAL, "solver is NULL"); }
        DeviceGuard guard(s->device);
        int rc = flush_timing(s);
        if(rc != J2P_OK) { return rc; }
        const double n = s->acc_samples ? (double)s->acc_samples : 1.;
        if(gradient_ms) { *gradient_ms = s->acc_grad_ms / n; }
        if(project_ms) { *project_ms = s->acc_proj_ms / n; }
        if(samples) { *samples = s->acc_samples; }
        return J2P_OK;
}

int j2p_decode_plane(int device, unsigned w, unsigned h, const int16_t *data, const uint16_t *quant_table, float *out)
{
        if(!data || !quant_table || !out) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(w == 0 || h == 0 || (w & 7) || (h & 7)) { return j2p_fail(J2P_EINVAL, "plane %ux%u is not a positive multiple of 8", w, h); }
        int ndev = 0;
        if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { return j2p_fail(J2P_EDEVICE, "no HIP device available"); }
        DeviceGuard guard(device);
        if(!guard.ok) { return j2p_fail(J2P_EDEVICE, "hipSetDevice(%d) failed", device); }
        const size_t n = (size_t)w * h;
        int16_t *dd = nullptr;
        float *df = nullptr, *dq = nullptr;
        float qf[64];
        for(int j = 0; j < 64; j++) { qf[j] = (float)quant_table[j]; }
        int rc = J2P_OK;
        hipError_t e = j2p_dev_malloc((void **)&dd, n * sizeof(int16_t));
        if(e == hipSuccess) { e = j2p_dev_malloc((void **)&df, n * sizeof(float)); }
        if(e == hipSuccess) { e = j2p_dev_malloc((void **)&dq, sizeof(qf)); }
        if(e == hipSuccess) { e = hipMemcpy(dd, data, n * sizeof(int16_t), hipMemcpyHostToDevice); }
        if(e == hipSuccess) { e = hipMemcpy(dq, qf, sizeof(qf), hipMemcpyHostToDevice); }
        if(e == hipSuccess) {
                const unsigned groups = ((w / 8 + 7) / 8) * (h / 8);
                hipLaunchKernelGGL(k_decode, dim3((groups + 3) / 4), dim3(256), 0, nullptr, (const int16_t *)dd,
                                   (const float *)dq, df, w, h / 8);
                e = hipGetLastError();
        }
        if(e == hipSuccess) { e = hipMemcpy(out, df, n * sizeof(float), hipMemcpyDeviceToHost); }
        if(e != hipSuccess) { rc = j2p_fail(e == hipErrorOutOfMemory ? J2P_ENOMEM : J2P_EDEVICE, "decode_plane: %s", hipGetErrorString(e)); }
        (void)hipFree(dd);
        (void)hipFree(df);
        (void)hipFree(dq);
        return rc;
}

int j2p_dct8x8_blocks(int device, float *blocks, size_t n, int inverse)
{
        if(!blocks) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(n == 0) { return J2P_OK; }
        int ndev = 0;
        if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { return j2p_fail(J2P_EDEVICE, "no HIP device available"); }
        DeviceGuard guard(device);
        if(!guard.ok) { return j2p_fail(J2P_EDEVICE, "hipSetDevice(%d) failed", device); }
        float *db = nullptr;
        int rc = J2P_OK;
        hipError_t e = j2p_dev_malloc((void **)&db, n * 64 * sizeof(float));
        if(e == hipSuccess) { e = hipMemcpy(db, blocks, n * 64 * sizeof(float), hipMemcpyHostToDevice); }
        if(e == hipSuccess) {
                hipLaunchKernelGGL(k_dct_blocks, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, nullptr, db, n, inverse);
                e = hipGetLastError();
        }
        if(e == hipSuccess) { e = hipMemcpy(blocks, db, n * 64 * sizeof(float), hipMemcpyDeviceToHost); }
        if(e != hipSuccess) { rc = j2p_fail(e == hipErrorOutOfMemory ? J2P_ENOMEM : J2P_EDEVICE, "dct8x8_blocks: %s", hipGetErrorString(e)); }
        (void)hipFree(db);
        return rc;
}

int j2p_math_selftest(int device, size_t n, unsigned seed, unsigned long long *div_mismatches,
                      unsigned long long *sqrt_mismatches)
{
        int ndev = 0;
        if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { return j2p_fail(J2P_EDEVICE, "no HIP device available"); }
        DeviceGuard guard(device);
        if(!guard.ok) { return j2p_fail(J2P_EDEVICE, "hipSetDevice(%d) failed", device); }
        unsigned long long *dm = nullptr, hm[2] = {0, 0};
        HIP_TRY(hipMalloc(&dm, sizeof(hm)));
        hipError_t e = hipMemset(dm, 0, sizeof(hm));
        if(e == hipSuccess) {
                hipLaunchKernelGGL(k_math_selftest, dim3(4096), dim3(256), 0, nullptr, n, seed, dm);
                e = hipMemcpy(hm, dm, sizeof(hm), hipMemcpyDeviceToHost);
        }
        (void)hipFree(dm);
        if(e != hipSuccess) { return j2p_fail(J2P_EDEVICE, "math_selftest: %s", hipGetErrorString(e)); }
        if(div_mismatches) { *div_mismatches = hm[0]; }
        if(sqrt_mismatches) { *sqrt_mismatches = hm[1]; }
        return J2P_OK;
}

// one reduction form on the caller's arrays, launched exactly as a solve launches it (launch_k_* above)
int j2p_norm_selftest_bands(int device, int form, unsigned nch, unsigned tile_rows, unsigned ntx, const double *in_host,
                            unsigned nband, const unsigned first_tile_row[], const unsigned band_tile_rows[],
                            double *rowsums_out_host, float *norm_out_host)
{
        const bool from_partials = form == J2P_NORM_FORM_ROWSUMS || form == J2P_NORM_FORM_NORM_WHOLE;
        const bool in_kernel = form == J2P_NORM_FORM_FOLD_TREE || form == J2P_NORM_FORM_PROJECT_TREE;
        if(form < J2P_NORM_FORM_ROWSUMS || form > J2P_NORM_FORM_PROJECT_TREE) { return j2p_fail(J2P_EINVAL, "norm_selftest: no form %d", form); }
        if(!in_host || (form == J2P_NORM_FORM_ROWSUMS ? !rowsums_out_host : !norm_out_host)) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(nch == 0 || nch > (unsigned)kMaxCh) { return j2p_fail(J2P_EINVAL, "norm_selftest: 1..%d channels", kMaxCh); }
        if(tile_rows == 0 || tile_rows > (in_kernel ? J2P_NORM_TREE_ROWS : (unsigned)kMaxTileRows)) {
                return j2p_fail(J2P_EINVAL, "norm_selftest: form %d takes 1..%u tile rows", form, in_kernel ? J2P_NORM_TREE_ROWS : (unsigned)kMaxTileRows);
        }
        // (65536 columns, the JPEG limit, are 529 strips)
        if(from_partials && (ntx == 0 || ntx > 529)) { return j2p_fail(J2P_EINVAL, "norm_selftest: 1..529 strips per tile row"); }
        BandRowsums bands;
        if(form == J2P_NORM_FORM_NORM_BANDS) {
                if(!first_tile_row || !band_tile_rows || nband == 0 || nband > (unsigned)kMaxBands) { return j2p_fail(J2P_EINVAL, "norm_selftest: 1..%d bands", kMaxBands); }
                std::vector<bool> covered(tile_rows, false);
                for(unsigned b = 0; b < nband; b++) {
                        if(first_tile_row[b] > tile_rows || band_tile_rows[b] > tile_rows - first_tile_row[b]) { return j2p_fail(J2P_EINVAL, "band %u: tile rows out of range", b); }
                        for(unsigned r = 0; r < band_tile_rows[b]; r++) {
                                if(covered[first_tile_row[b] + r]) { return j2p_fail(J2P_EINVAL, "band %u overlaps another", b); }
                                covered[first_tile_row[b] + r] = true;
                        }
                }
                for(unsigned r = 0; r < tile_rows; r++) {
                        if(!covered[r]) { return j2p_fail(J2P_EINVAL, "the bands do not cover tile row %u", r); }
                }
        }
        int ndev = 0;
        if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { return j2p_fail(J2P_EDEVICE, "no HIP device available"); }
        DeviceGuard guard(device);
        if(!guard.ok) { return j2p_fail(J2P_EDEVICE, "hipSetDevice(%d) failed", device); }
        const size_t n_in = (size_t)nch * tile_rows * (from_partials ? ntx : 1u);
        const size_t n_rowsums = (size_t)nch * tile_rows;
        double *d_in = nullptr, *d_rowsums = nullptr;
        float *d_norm = nullptr;
        hipError_t e = hipMalloc(&d_in, n_in * sizeof(double));
        if(e == hipSuccess) { e = hipMalloc(&d_rowsums, n_rowsums * sizeof(double)); }
        if(e == hipSuccess) { e = hipMalloc(&d_norm, kMaxCh * sizeof(float)); }
        if(e == hipSuccess) { e = hipMemcpy(d_in, in_host, n_in * sizeof(double), hipMemcpyHostToDevice); }
        if(e == hipSuccess) { e = hipMemset(d_norm, 0xff, kMaxCh * sizeof(float)); }       // (NaN: a word nobody wrote shows)
        if(e == hipSuccess && form == J2P_NORM_FORM_NORM_WHOLE) { e = allow_k_norm_whole_lds(); }
        if(e == hipSuccess) {
                switch(form) {
                case J2P_NORM_FORM_ROWSUMS: launch_k_rowsums(nullptr, d_in, d_rowsums, ntx, tile_rows, nch); break;
                case J2P_NORM_FORM_NORM_WHOLE: launch_k_norm_whole(nullptr, d_in, ntx, tile_rows, nch, d_norm); break;
                case J2P_NORM_FORM_NORM_FINISH: launch_k_norm_finish(nullptr, d_in, tile_rows, nch, d_norm); break;
                case J2P_NORM_FORM_NORM_BANDS:
                        for(unsigned b = 0; b < nband; b++) {
                                bands.rowsum[b] = d_in + (size_t)first_tile_row[b] * nch;
                                bands.first[b] = first_tile_row[b];
                                bands.count[b] = band_tile_rows[b];
                        }
                        bands.nband = nband;
                        bands.out[0] = d_norm;
                        bands.nout = 1;
                        launch_k_norm_bands(nullptr, bands, tile_rows, nch);
                        break;
                default: {
                        GradArgs a{};
                        a.rowsum = d_in;
                        a.ntr_global = tile_rows;
                        a.nch_total = nch;
                        a.norm_out = d_norm;
                        hipLaunchKernelGGL(k_norm_trees_selftest, dim3(nch), dim3(64), 0, nullptr, a, form == J2P_NORM_FORM_FOLD_TREE ? 0 : 1);
                        break;
                }
                }
                e = hipGetLastError();
        }
        if(e == hipSuccess && form == J2P_NORM_FORM_ROWSUMS) { e = hipMemcpy(rowsums_out_host, d_rowsums, n_rowsums * sizeof(double), hipMemcpyDeviceToHost); }
        else if(e == hipSuccess) { e = hipMemcpy(norm_out_host, d_norm, nch * sizeof(float), hipMemcpyDeviceToHost); }
        (void)hipFree(d_in);
        (void)hipFree(d_rowsums);
        (void)hipFree(d_norm);
        if(e != hipSuccess) { return j2p_fail(e == hipErrorOutOfMemory ? J2P_ENOMEM : J2P_EDEVICE, "norm_selftest: %s", hipGetErrorString(e)); }
        return J2P_OK;
}

int j2p_norm_selftest(int device, int form, unsigned nch, unsigned tile_rows, unsigned ntx, const double *in_host,
                      double *rowsums_out_host, float *norm_out_host)
{
        const unsigned first = 0;
        return j2p_norm_selftest_bands(device, form, nch, tile_rows, ntx, in_host, 1, &first, &tile_rows, rowsums_out_host, norm_out_host);
}

int j2p_sqrt_exhaustive(int device, unsigned long long *rsq_mismatches, unsigned long long *fast_mismatches)
{
        int ndev = 0;
        if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { return j2p_fail(J2P_EDEVICE, "no HIP device available"); }
        DeviceGuard guard(device);
        if(!guard.ok) { return j2p_fail(J2P_EDEVICE, "hipSetDevice(%d) failed", device); }
        unsigned long long *dm = nullptr, hm[2] = {0, 0};
        HIP_TRY(hipMalloc(&dm, sizeof(hm)));
        hipError_t e = hipMemset(dm, 0, sizeof(hm));
        if(e == hipSuccess) {
                hipLaunchKernelGGL(k_sqrt_exhaustive, dim3(8192), dim3(256), 0, nullptr, dm);
                e = hipMemcpy(hm, dm, sizeof(hm), hipMemcpyDeviceToHost);
        }
        (void)hipFree(dm);
        if(e != hipSuccess) { return j2p_fail(J2P_EDEVICE, "sqrt_exhaustive: %s", hipGetErrorString(e)); }
        if(rsq_mismatches) { *rsq_mismatches = hm[0]; }
        if(fast_mismatches) { *fast_mismatches = hm[1]; }
        return J2P_OK;
}

// one pass (or slice of a pass) of the short division's exhaustive checks (see k_recip_exhaustive);
// report[0] = mismatches, report[1..8] = the first offenders
int j2p_division_exhaustive(int device, int pass, unsigned first, unsigned count, unsigned long long report[9])
{
        if(pass < 1 || pass > 3) { return j2p_fail(J2P_EINVAL, "pass must be 1, 2 or 3"); }
        if(!report) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        int ndev = 0;
        if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { return j2p_fail(J2P_EDEVICE, "no HIP device available"); }
        DeviceGuard guard(device);
        if(!guard.ok) { return j2p_fail(J2P_EDEVICE, "hipSetDevice(%d) failed", device); }
        unsigned long long *dm = nullptr, hm[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        HIP_TRY(j2p_dev_malloc((void **)&dm, sizeof(hm)));
        hipError_t e = hipMemset(dm, 0, sizeof(hm));
        if(e == hipSuccess) {
                if(pass == 1) { hipLaunchKernelGGL(k_recip_exhaustive, dim3(8192), dim3(256), 0, nullptr, dm); }
                else if(pass == 2) { hipLaunchKernelGGL(k_div_exhaustive<false>, dim3((count + 3) / 4), dim3(256), 0, nullptr, first, count, dm); }
                else { hipLaunchKernelGGL(k_div_exhaustive<true>, dim3((count + 3) / 4), dim3(256), 0, nullptr, first, count, dm); }
                e = hipMemcpy(hm, dm, sizeof(hm), hipMemcpyDeviceToHost);
        }
        (void)hipFree(dm);
        if(e != hipSuccess) { return j2p_fail(J2P_EDEVICE, "division_exhaustive: %s", hipGetErrorString(e)); }
        for(int i = 0; i < 9; i++) { report[i] = hm[i]; }
        return J2P_OK;
}

}  // extern "C"

// ---- what the output stage sees of a solver (j2p_internal.h) ----
j2p_solver_view j2p_solver_view_of(const j2p_solver *s)
{
        j2p_solver_view v;
        v.device = s->device;
        v.stream = s->stream;
        v.nch = s->nch;
        v.W = s->W;
        v.H = s->H;
        v.row0 = s->row0;
        v.rows = s->rows;
        v.whole = s->whole;
        v.mid_iteration = s->grad_done;
        v.orientation = s->orientation;
        v.orient_w = s->orient_w;
        v.orient_h = s->orient_h;
        return v;
}

int j2p_solver_row(const j2p_solver *s, unsigned c, unsigned y, const float **row)
{
        if(!s || !row) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(c >= s->nch) { return j2p_fail(J2P_EINVAL, "channel %u out of range", c); }
        if(y < s->row0 || y >= s->row0 + s->rows) { return j2p_fail(J2P_EINVAL, "row %u is not one of the solver's [%u,%u)", y, s->row0, s->row0 + s->rows); }
        *row = s->ch[c].xbuf[s->cur] + (size_t)(kHalo + (y - s->row0)) * s->W;
        return J2P_OK;
}

size_t j2p_solver_scratch_bytes(const j2p_solver *s) { return s ? s->out_scratch_bytes : 0; }

// one pooled block of the solver's, grown to at least `bytes`: what j2p_solver_scratch and j2p_solver_upright both do
static int grow_block(j2p_solver *s, void *&block, size_t &block_bytes, size_t bytes)
{
        if(block_bytes < bytes) {
                DeviceGuard guard(s->device);
                // what is queued on the stream may still read the block that is given back: growing waits, reusing never does
                HIP_TRY(hipStreamSynchronize(s->stream));
                j2p_pool_give(s->device, block, block_bytes);
                block = nullptr;
                block_bytes = 0;
                const size_t want = (bytes + ((size_t)256 << 10) - 1) & ~(((size_t)256 << 10) - 1);
                void *p = nullptr;
                size_t got = 0;
                HIP_TRY(j2p_pool_take(s->device, want, &p, &got));
                block = p;
                block_bytes = got;
        }
        return J2P_OK;
}

int j2p_solver_scratch(j2p_solver *s, size_t bytes, void **out)
{
        if(!s || !out) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(const int rc = grow_block(s, s->out_scratch, s->out_scratch_bytes, bytes); rc != J2P_OK) { return rc; }
        *out = s->out_scratch;
        return J2P_OK;
}

int j2p_solver_upright(j2p_solver *s, size_t bytes, float **out)
{
        if(!s || !out) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(const int rc = grow_block(s, s->upright, s->upright_bytes, bytes); rc != J2P_OK) { return rc; }
        *out = static_cast<float *>(s->upright);
        return J2P_OK;
}
