// jpeg2png_amd — the geometry every layer has to agree on, each rule once: canvas and band alignment, the least band,
// near-equal cuts, the gradient strip schedule and the per-channel row windows of a band.  Pure arithmetic on a handful
// of integers; C11 and C++, nothing from HIP, so that compute_host.c, the HIP units and a stand-alone C program
// (tests/c/geometry_main.c) all include it.  Not part of the C-ABI.
#pragma once
#include <stddef.h>
#include "jpeg2png_amd.h"          // J2P_TILE_ROWS, J2P_HALO_ROWS

// ---- canvas and band alignment: accumulated over the channels ----
// W x H is the largest plane in pixels (compute.c:410-416); band boundaries are multiples of `align`, the least common
// multiple of the 16-row tile row and every channel's block row (8 * h_samp), so that no DCT block and no gradient tile
// straddles two bands.  Sampling factors are not zero.
typedef struct {
        unsigned W, H, align;
} j2p_canvas;
#define J2P_CANVAS_NONE { 0u, 0u, (unsigned)J2P_TILE_ROWS }

static inline unsigned j2p_gcd(unsigned a, unsigned b)
{
        while(b) { const unsigned r = a % b; a = b; b = r; }
        return a;
}
static inline void j2p_canvas_add(j2p_canvas *cv, unsigned w, unsigned h, unsigned w_samp, unsigned h_samp)
{
        if(w * w_samp > cv->W) { cv->W = w * w_samp; }
        if(h * h_samp > cv->H) { cv->H = h * h_samp; }
        cv->align = cv->align / j2p_gcd(cv->align, 8 * h_samp) * (8 * h_samp);
}

// rows a band must at least have before a canvas is spread over several GPUs: three 16-row gradient segments, so that
// every band has an interior to hide the halo exchange behind, rounded up to the alignment
static inline unsigned j2p_min_band_rows(unsigned align) { return (3 * J2P_TILE_ROWS + align - 1) / align * align; }

// near-equal bands: edge[0 .. nband-1] are the first rows of nband contiguous bands of `units` alignment units, the
// first units % nband of them one unit longer.  The last edge is the caller's (the canvas height, whatever the units
// leave over).  Returns 0, with nothing written, when there are fewer units than bands.
static inline int j2p_near_equal_cuts(unsigned units, unsigned nband, unsigned align, unsigned edge[])
{
        if(nband == 0 || units < nband) { return 0; }
        unsigned start = 0;
        for(unsigned b = 0; b < nband; b++) {
                edge[b] = start * align;
                start += units / nband + (b < units % nband ? 1 : 0);
        }
        return 1;
}

// ---- the gradient strip schedule ----
#define J2P_STRIP_COLS 124u        // output columns per wavefront strip (j2p_kernels.hip.h: kStripCols)

// rows per gradient strip: 16; 8, then 4, while the strips make fewer wavefronts than half the chip's 4096 slots (the
// launch is then one generation whose length is the busiest SIMD's: shorter strips balance it, at 25 / 50 instead of 12.5 %
// redundant rows).  A limit of 4096 for the first step was measured too (profiles/r03_px_rpw_sweep.jsonl,
// r03_rpw_concurrency.json): a single 2048^2 Y plane or 1080p 4:2:0 image gains 2 %, eight concurrent 1080p 4:2:0 images —
// the batch case, where the chip is full anyway — lose 5.7 %; not taken
static const unsigned long long kHalfStripWaves = 2048;
static const unsigned long long kShortStripWaves = 2048;
// half / quarter items at the end of a gradient launch (see j2p_zone_shares): launches of fewer strips than this, and
// the shares (1/256) of every XCD's run dealt that way
static const unsigned long long kZoneMaxWaves = 3 * 4096;
static const unsigned kZoneB = 32, kZoneC = 10;
static const unsigned kBigZoneD = 200, kBigZoneB = 24, kBigZoneC = 8;

typedef struct {
        unsigned strips, rpw;                   // strips per row, rows per strip
        unsigned zone_d, zone_b, zone_c;        // shares (1/256) of a gradient launch dealt as double / half / quarter tile rows
} j2p_strip_schedule;

static inline void j2p_zone_clamp(j2p_strip_schedule *p)
{
        if(p->zone_b > 256) { p->zone_b = 256; }
        if(p->zone_b + p->zone_c > 256) { p->zone_c = 256 - p->zone_b; }
        if(p->zone_d + p->zone_b + p->zone_c > 256) { p->zone_d = 256 - p->zone_b - p->zone_c; }
}

// the zone shares of a launch over band_rows rows in strips of p->strips x p->rpw
static inline void j2p_zone_shares(j2p_strip_schedule *p, unsigned band_rows, unsigned nchannel)
{
        const unsigned g = p->rpw;
        p->zone_d = p->zone_b = p->zone_c = 0;
        // The LAST wavefronts of a gradient launch march half and quarter tile rows (grad_item): a launch ends with
        // its last wavefront, and a whole 16-row item dispatched last keeps a few SIMDs busy for a wavefront life
        // (17 us of 53 at 4096^2, profiles/r06_wave_trace.jsonl) while the rest of the chip drains.  Shares in
        // 1/256 of every XCD's run; one channel per workgroup wavefront.  Who marches a row never changes a bit
        // (march_rows), so the choice may depend on the BAND: measured (profiles/r06_zones_mid_sizes.jsonl,
        // r06_zones_by_size.jsonl; us per iteration without / with) 1080p 30.1 / 28.7, 2048^2 45.5 / 42.2,
        // 4096x2048 70.9 / 67.8, 4096x3072 94.2 / 92.0, 4096^2 120.0 / 118.7; nothing from three wavefront
        // generations on (8192x4096 235.3 / 235.9, 16384x2048 230.8 / 231.1, 8192^2 515.7 / 515.8).
        const unsigned long long launch_waves = (unsigned long long)p->strips * ((band_rows + g - 1) / g);
        if(nchannel == 1 && g >= 8 && launch_waves < kZoneMaxWaves) {
                p->zone_b = kZoneB;
                p->zone_c = g >= 16 ? kZoneC : 0;
        } else if(nchannel == 1 && g >= 16) {
                // ... and from three generations on the FIRST workgroups march two tile rows at once (34 row trips for
                // 32 rows: fewer source rows recomputed and re-read), the tail shares smaller: 16384x2048 229.8 -> 227.0
                // us per iteration, 8192^2 476.0 -> 471.1; below that doubles cost more at the end of the launch than they
                // save (2048^2 43.2 -> 46.0, 4096x2048 69.3 -> 72.4, 4096^2 +-0: profiles/r06_doubles.jsonl)
                p->zone_d = kBigZoneD;
                p->zone_b = kBigZoneB;
                p->zone_c = kBigZoneC;
        }
        j2p_zone_clamp(p);
}

// Gradient strips: 128 columns (two per lane, packed arithmetic) by rpw rows = rows per norm partial ("tile row").
// A canvas that fills the chip: 16 rows (32 / 48 / 64 measured no faster).  A smaller canvas leaves
// wavefront slots empty and is bound by how long ONE wavefront takes to walk its rows (wave timelines,
// profiles/r03_wave_trace.jsonl: ~0.9 us per row trip whatever the SIMD's load), so it gets shorter strips (8 or 4
// rows: fewer trips per wavefront; narrower strips do not pay).  Strips and rows are functions of the
// CANVAS only (never of the band), so that every band of a tiled run — and the whole-canvas solver — reduce ||g|| over
// the same partials in the same order.
static inline j2p_strip_schedule j2p_strip_schedule_of(unsigned W, unsigned H, unsigned band_rows, unsigned nchannel)
{
        j2p_strip_schedule p = { 0u, (unsigned)J2P_TILE_ROWS, 0u, 0u, 0u };
        p.strips = W <= 4 ? 1u : (W - 4 + J2P_STRIP_COLS - 1) / J2P_STRIP_COLS;
        // (limits measured, profiles/r03_px_rpw_sweep.jsonl)
        if((unsigned long long)p.strips * nchannel * ((H + p.rpw - 1) / p.rpw) < kHalfStripWaves) { p.rpw = 8; }
        if(p.rpw == 8 && (unsigned long long)p.strips * nchannel * ((H + p.rpw - 1) / p.rpw) < kShortStripWaves) { p.rpw = 4; }
        j2p_zone_shares(&p, band_rows, nchannel);
        return p;
}

// ---- the order in which every XCD walks its run of the two phase launches ----
// Both phase kernels give XCD q the q-th contiguous run of the canvas (grad_item, project_item).  J2P_ORDER_FORWARD: the
// run top-down.  J2P_ORDER_REVERSE: the XCD's own run bottom-up.  One phase forward and the other backwards (serpentine)
// lets every phase start on the rows the phase before touched last: they are still in the XCD's OWN L2 (4 MiB each), and —
// planes that do not fit it — in the Infinity Cache.  Schedule only: no bit depends on who marches a row when.
// working_set: the bytes an iteration touches; planes: x_k and x_{k-1} of them; cache: the Infinity Cache; W x rows: the
// solver's canvas rows; band: a band of a row-tiled run, not a whole canvas.
typedef struct {
        unsigned gradient, project;     // J2P_ORDER_*
} j2p_phase_order;

static inline j2p_phase_order j2p_phase_order_of(size_t working_set, size_t planes, size_t cache, unsigned W, unsigned rows, int band)
{
        j2p_phase_order o = { J2P_ORDER_FORWARD, J2P_ORDER_FORWARD };
        (void)working_set; (void)W; (void)rows;
        // Whole canvases: the GRADIENT phase bottom-up, the projection top-down.  Measured against both forward, the
        // projection reversed instead, and both reversed (profiles/phase_order_sweep.jsonl, us per iteration forward /
        // serpentine): 1080p Y 29.1 / 28.6, 2048^2 43.7 / 42.2, 4096^2 117.3 / 115.8, 8192x4096 226.4 / 223.9,
        // 16384x2048 222.7 / 220.8; no size of the sweep slower.  Reversing the projection instead gains as much or more
        // at 4096x2048 (69.6 / 67.7) and on 1080p 4:2:0 joint (73.0 / 71.2) and less at 2048^2 and 8192x4096: one rule,
        // this one.  Both reversed is both forward with the ends exchanged: no gain.
        // Past the Infinity Cache (planes > cache) the same order keeps what the cache holds of the planes (8192^2
        // 502 -> 458 us per iteration); bands get it there only, as before: within the cache they were not measured.
        if(!band || planes > cache) { o.gradient = J2P_ORDER_REVERSE; }
        return o;
}

// ---- the rows of one channel a solver of canvas rows [row0, row1) holds, in coefficient rows of the channel ----
typedef struct {
        unsigned crow0, crows;          // of d / pg: the band's own rows (block aligned because the band is)
        unsigned frow0, frows;          // of the decoded input the init kernel touches: own rows + halo, clamped like compute.c:298
} j2p_row_window;

// ch: the channel's coefficient rows, hs its vertical sampling, H the canvas height.  band_local: the host arrays hold
// the band's rows only, so the input window is the band's own; returns 0 when the channel then does not cover the canvas
// height (*out is not complete), 1 otherwise.
static inline int j2p_row_window_of(unsigned ch, unsigned hs, unsigned H, unsigned row0, unsigned row1, int band_local, j2p_row_window *out)
{
        unsigned c0 = row0 / hs, c1 = (row1 + hs - 1) / hs;
        if(c0 > ch) { c0 = ch; }
        if(c1 > ch) { c1 = ch; }
        out->crow0 = c0;
        out->crows = c1 - c0;
        if(band_local) {
                if(ch * hs < H) { return 0; }
                out->frow0 = out->crow0;
                out->frows = out->crows;
        } else {
                const unsigned y0 = row0 >= (unsigned)J2P_HALO_ROWS ? row0 - J2P_HALO_ROWS : 0;
                const unsigned y1 = row1 + J2P_HALO_ROWS < H ? row1 + J2P_HALO_ROWS : H;
                unsigned f0 = y0 / hs, f1 = (y1 - 1) / hs + 1;
                if(f0 > ch - 1) { f0 = ch - 1; }
                if(f1 > ch) { f1 = ch; }
                if(f1 <= f0) { f1 = f0 + 1; }
                out->frow0 = f0;
                out->frows = f1 - f0;
        }
        return 1;
}

// ---- one buffer for the gradient g and the prob state pg of a channel ----
// g (canvas raster: rows x W floats from canvas row row0) and pg (coefficient raster: crows x cw floats from coefficient
// row crow0) are never live at the same time for the same pixel: k_gradient reads pg(r, x) only in the lane that then
// stores g(r, x), k_project reads the g of its eight blocks and then writes their pg.  Where the two rasters put every
// sample at the same offset — a channel sampled 1x1 whose coefficient raster has the canvas's pitch and starts at the
// solver's first row — one buffer of rows x W floats serves as both.  A channel with fewer coefficient rows than the
// canvas has rows still shares: beyond its coverage no pg is written and none is used (march_rows: the row test at the
// point of use), the floats there are g's alone.  Not shared: prob term off (pweight == 0: pg must stay all zero, nobody
// writes it, and 0 * g of a non-finite g would not be 0); subsampled, narrower or wide-footprint channels.
static inline int j2p_shares_state(unsigned cw, unsigned ws, unsigned hs, unsigned crow0, unsigned W, unsigned row0, int prob_on, int wide)
{
        return ws == 1 && hs == 1 && cw == W && crow0 == row0 && prob_on && !wide;
}

// ---- what one channel keeps live per iteration, for the non-temporal policy (j2p_solver.hip: nt_policy) ----
// planes: x_k and x_{k-1} with their halo rows; g: the gradient plane where it is a buffer of its own (a shared buffer is
// counted once, in working_set, and is nobody's to hint apart: "everything but g" is then everything); d: the coefficients
// at d_bytes each.  cells = floats of the prob state = coefficients held (at least one row).
typedef struct {
        size_t working_set, g, planes, d;
} j2p_live_bytes;

static inline void j2p_live_bytes_add(j2p_live_bytes *l, size_t plane_floats, size_t grad_floats, size_t cells, size_t d_bytes, int shared)
{
        const size_t state_floats = shared ? grad_floats : grad_floats + cells;
        l->working_set += (2 * plane_floats + state_floats) * sizeof(float) + cells * d_bytes;
        l->planes += 2 * plane_floats * sizeof(float);
        l->d += cells * d_bytes;
        if(!shared) { l->g += grad_floats * sizeof(float); }
}

// how many streams get the non-temporal hint so that the rest fits `cache` bytes: 0 none, 1 g, 2 g and the prob state,
// 3 those and d.  A solver all of whose channels share has g == 0: level 1 is then level 0's test over again and never
// applies — past the cache such a solver goes straight to hinting the shared buffer in both its roles.
static inline int j2p_nt_level(const j2p_live_bytes *l, size_t cache)
{
        if(l->working_set <= cache) { return 0; }                        // everything fits
        if(l->working_set - l->g <= cache) { return 1; }                 // everything but g fits
        if(l->planes + l->d <= cache) { return 2; }                      // planes and d fit
        return 3;
}
