// jpeg2png_amd — the restart intervals of a JPEG file the library writes (include/jpeg2png_amd.h: "Restart intervals"), each rule
// once: a scan's units and units per row, its interval from restart_interval / restart_in_rows, its number of intervals and whether
// a DRI segment precedes it.  Pure arithmetic on a handful of integers; C11 and C++, nothing from HIP, so that the coder, the header
// writer, the size estimates and a stand-alone C program (tests/c/restart_main.c) all include it.  Not part of the C-ABI but for
// the two records, which j2p_debug_restart_plan hands out.
#pragma once
#include "jpeg2png_amd.h"          // j2p_restart_scan, j2p_restart_plan

#define J2P_RESTART_MAX 65535u     // what the 16 bits of a DRI segment hold

// the one component of every scan of jpeg_simple_progression(), -1 for a scan that interleaves all three (include/jpeg2png_amd.h:
// "The progressive JPEG file")
static const int kJ2pProgScanComponent[2][10] = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {-1, 0, 2, 1, 0, 0, -1, 2, 1, 0}};

// what is wrong with the two restart arguments, or NULL
static inline const char *j2p_restart_error(unsigned restart_interval, unsigned restart_in_rows)
{
        if(restart_interval > J2P_RESTART_MAX) { return "jpeg: restart_interval is above 65535"; }
        if(restart_in_rows > J2P_RESTART_MAX) { return "jpeg: restart_in_rows is above 65535"; }
        if(restart_interval && restart_in_rows) { return "jpeg: restart_interval and restart_in_rows are both set"; }
        return 0;
}

// One scan: `units` of them, `units_per_row` in a row.  *last: the interval of the last DRI written (0 before the first), updated.
static inline j2p_restart_scan j2p_restart_scan_of(unsigned units, unsigned units_per_row, unsigned restart_interval, unsigned restart_in_rows,
                                                   unsigned *last)
{
        j2p_restart_scan s;
        s.units = units;
        s.units_per_row = units_per_row;
        s.interval = restart_interval;
        if(restart_in_rows) {
                const unsigned long long nominal = (unsigned long long)restart_in_rows * units_per_row;
                s.interval = nominal < J2P_RESTART_MAX ? (unsigned)nominal : J2P_RESTART_MAX;
        }
        s.intervals = s.interval ? (units + s.interval - 1) / s.interval : 1;
        s.dri = s.interval != *last;
        *last = s.interval;
        return s;
}

// Every scan of the file of width x height pixels with ncomp (1 or 3) components, sub_w x sub_h blocks of component 0 in an MCU:
// the one scan of a baseline file, or the scans of the progressive one.  An interleaved scan counts MCUs, a scan of one
// component that component's blocks in raster order.  The arguments have passed j2p_restart_error and the spec's own checks.
static inline j2p_restart_plan j2p_restart_plan_of(unsigned width, unsigned height, unsigned ncomp, unsigned sub_w, unsigned sub_h, int progressive,
                                                   unsigned restart_interval, unsigned restart_in_rows)
{
        j2p_restart_plan p;
        unsigned bw[3], bh[3], last = 0;
        if(ncomp != 3) { sub_w = sub_h = 1; }
        bw[0] = (width + 7) / 8;
        bh[0] = (height + 7) / 8;
        bw[1] = bw[2] = (bw[0] + sub_w - 1) / sub_w;
        bh[1] = bh[2] = (bh[0] + sub_h - 1) / sub_h;
        p.nscans = progressive ? (ncomp == 3 ? 10u : 6u) : 1u;
        for(unsigned s = 0; s < J2P_PROGRESSIVE_SCANS; s++) {
                const int c = progressive ? kJ2pProgScanComponent[ncomp == 3][s] : (ncomp == 3 ? -1 : 0);
                if(s >= p.nscans) {
                        const j2p_restart_scan none = {0, 0, 0, 0, 0};
                        p.scan[s] = none;
                } else if(c < 0) {
                        p.scan[s] = j2p_restart_scan_of(bw[1] * bh[1], bw[1], restart_interval, restart_in_rows, &last);       // (the chroma grid IS the MCU grid)
                } else {
                        p.scan[s] = j2p_restart_scan_of(bw[c] * bh[c], bw[c], restart_interval, restart_in_rows, &last);
                }
        }
        return p;
}

// RSTn markers in the file: one behind every interval of a scan but its last
static inline unsigned long long j2p_restart_markers(const j2p_restart_plan *p)
{
        unsigned long long n = 0;
        for(unsigned s = 0; s < p->nscans; s++) { n += p->scan[s].intervals - 1; }
        return n;
}
