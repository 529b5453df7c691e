// jpeg2png_amd — device code that READS a progressive JPEG file: every scan's entropy-coded data decoded into the int16
// coefficient grids (include/jpeg2png_amd.h: "Reading a progressive JPEG file"; the argument: DESIGN.md section 26).  Included by
// j2p_codec.hip behind j2p_decode_kernels.hip.h, whose k_unstuff_* (once per scan, into one clean buffer), decode_peek and table
// layout it reuses, as it reuses the k_scan_* of j2p_codec_kernels.hip.h.  The passes:
//   k_scans_intervals    subsequences per (first scan, restart interval): ALL first scans share one subsequence array   -> first[]
//   k_scans_sync         one ROUND over that array: every subsequence whose entry state changed is decoded again         -> exit[], done[]
//   k_scans_write        every subsequence once more from its true state: AC values << Al into the grids, DC differences by ordinal
//   k_scans_dc           the DC differences summed per scan, component and interval: coefficient 0 = predictor << Al
//   k_scans_dc_refine    one launch per DC refinement scan, a lane per block position: coefficient 0 |= bit << Al
//   k_scans_ac_refine    one launch per AC refinement scan, in file order, a wavefront per restart interval, a lane per coefficient
// The tables are read from device memory (every scan has its own; all of them do not fit LDS).  Every loop has a trip count the
// host knows, every read of the stream is clamped (decode_peek), every store goes to a block whose ordinal was checked against the
// scan's block count.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "j2p_decode_kernels.hip.h"

namespace j2p {

constexpr unsigned kDecodeBadRefine = 64;       // s > 1 in a refinement scan
constexpr unsigned kDecodeBadEobRun = 128;      // an EOB run past the last block of its restart interval

constexpr unsigned kScanDcFirst = 0, kScanAcFirst = 1, kScanDcRefine = 2, kScanAcRefine = 3;

// one scan as the kernels see it; in device memory, indexed there
struct ScanDesc {
        unsigned kind;
        unsigned ncomp;                 // components in the scan
        unsigned comp[3];               // ... as frame indices
        unsigned bw[3], bh[3];          // ... their delivered grids
        unsigned hs[3], vs[3];          // ... their blocks in an MCU of this scan (1 x 1 in a scan of one component)
        unsigned first_blk[3];          // where a component's blocks begin in the MCU
        unsigned comp_off[3];           // where a component's DC differences begin within the scan's: units * the blocks before
        unsigned dc_tab[3], ac_tab;     // indices into the table pool
        unsigned blk_comp[12];          // [block of the MCU] its component of the scan
        unsigned per_mcu, mcus_w;       // blocks in an MCU; MCUs across (one component: 1; blocks across)
        unsigned units;                 // MCUs in the scan
        unsigned ri;                    // MCUs per restart interval (units without restarts)
        unsigned nint;                  // restart intervals
        unsigned nblocks;               // units * per_mcu
        unsigned ss, se, al;
        unsigned rst_base;              // the scan's first entry of rst[]
        unsigned sub_base;              // a first scan: its first interval among all first scans' intervals
        unsigned diff_base;             // a DC first scan: where its DC differences begin
        unsigned long long clean_base;  // where the scan's clean bytes begin in the clean buffer
        const unsigned long long *clean_bytes, *nmarkers;       // the totals of the scan's two unstuffing sums
};

struct ScansBuffers {
        const ScanDesc *scans;
        const j2p_huff_decode *pool;
        const unsigned *words;          // the clean buffer: every scan's clean stream at its clean_base, FF between and behind them
        unsigned long long nwords;
        const unsigned long long *rst;  // [a scan's rst_base + m] clean byte offset of its marker m, from its clean_base
        const unsigned short *iscan;    // [interval of the first scans] its scan
        const unsigned long long *first;// [interval of the first scans] its first subsequence
        const unsigned long long *nsub; // subsequences in all
        unsigned nfirst;                // intervals of the first scans
        unsigned S;                     // bits per subsequence
        unsigned *error;
};

struct ScansOut {
        int16_t *coef[3];               // by frame component
        unsigned *diff;                 // DC difference + 32768: by DC first scan (diff_base), component (comp_off) and scan order
};

__device__ __forceinline__ int16_t *scans_grid(const ScansOut &o, unsigned c) { return c == 0 ? o.coef[0] : c == 1 ? o.coef[1] : o.coef[2]; }

// interval k of scan d in the clean buffer, in bytes; clamped to the scan's own stream
__device__ __forceinline__ void scans_interval(const ScansBuffers &b, const ScanDesc &d, unsigned k, unsigned long long *begin, unsigned long long *end)
{
        const unsigned long long all = *d.clean_bytes;
        unsigned long long lo = k ? b.rst[d.rst_base + k - 1] : 0ull, hi = k + 1 < d.nint ? b.rst[d.rst_base + k] : all;
        if(hi > all) { hi = all; }
        if(lo > hi) { lo = hi; }
        *begin = d.clean_base + lo;
        *end = d.clean_base + hi;
}

// a symbol of table t at the head of the window w: its length (a prefix that is no code: 16 bits of the symbol 0, *bad set)
__device__ __forceinline__ unsigned scans_symbol(const j2p_huff_decode &tab, unsigned w, unsigned *sym, unsigned *bad)
{
        const unsigned e = tab.look[w >> 24];
        unsigned len = e >> 8;
        *sym = e & 0xffu;
        if(len == 0) {
                const unsigned code = w >> 16;
                for(unsigned l = 9; l <= 16; l++) {
                        const int v = (int)(code >> (16 - l));
                        if(v <= tab.maxcode[l]) {
                                len = l;
                                *sym = tab.vals[(unsigned)(v + tab.valoff[l]) & 0xffu];
                                break;
                        }
                }
                if(len == 0) {
                        len = 16;
                        *sym = 0;
                        *bad |= kDecodeBadCode;
                }
        }
        return len;
}

// the block of ordinal `ord` of scan d: its address (NULL for a block that pads the grid out to whole MCUs) and its place among
// the scan's DC differences
__device__ __forceinline__ int16_t *scans_block(const ScanDesc &d, const ScansOut &o, unsigned ord, unsigned *diff_at)
{
        const unsigned mcu = ord / d.per_mcu, blk = ord - mcu * d.per_mcu, ci = d.blk_comp[blk], j = blk - d.first_blk[ci];
        const unsigned hs = d.hs[ci], vs = d.vs[ci], bw = d.bw[ci];
        const unsigned my = mcu / d.mcus_w, mx = mcu - my * d.mcus_w, jy = j / hs, jx = j - jy * hs;
        const unsigned bx = mx * hs + jx, by = my * vs + jy;
        *diff_at = d.diff_base + d.comp_off[ci] + mcu * (hs * vs) + j;
        return bx < bw && by < d.bh[ci] ? scans_grid(o, d.comp[ci]) + ((size_t)by * bw + bx) * 64 : nullptr;
}

// ---- the first scans ----
__global__ __launch_bounds__(256) void k_scans_intervals(ScansBuffers b, unsigned *count)
{
        const unsigned gi = blockIdx.x * 256 + threadIdx.x;
        if(gi >= b.nfirst) { return; }
        const ScanDesc &d = b.scans[b.iscan[gi]];
        const unsigned k = gi - d.sub_base;
        unsigned bad = 0;
        if(k == 0 && *d.nmarkers + 1 != d.nint) { bad = kDecodeBadMarker; }
        unsigned long long begin, end;
        scans_interval(b, d, k < d.nint ? k : 0, &begin, &end);
        if(begin == end) { bad = kDecodeBadMarker; }
        count[gi] = (unsigned)(((end - begin) * 8 + b.S - 1) / b.S);
        if(bad) { atomicOr(b.error, bad); }
}

// where subsequence i lies (DecodeSpan; `interval` counts within the scan) and in which scan
__device__ __forceinline__ bool scans_span(const ScansBuffers &b, unsigned long long i, DecodeSpan *s, unsigned *scan)
{
        if(i >= *b.nsub) { return false; }
        unsigned lo = 0, hi = b.nfirst - 1;
        for(int step = 0; step < 32 && lo < hi; step++) {       // the last interval whose first subsequence is <= i
                const unsigned mid = lo + (hi - lo + 1) / 2;
                if(b.first[mid] <= i) {
                        lo = mid;
                } else {
                        hi = mid - 1;
                }
        }
        *scan = b.iscan[lo];
        const ScanDesc &d = b.scans[*scan];
        const unsigned k = lo - d.sub_base < d.nint ? lo - d.sub_base : 0;
        unsigned long long begin, end;
        scans_interval(b, d, k, &begin, &end);
        const unsigned long long local = i - b.first[lo];
        s->interval = k;
        s->begin = begin * 8;
        s->end = end * 8;
        s->start = s->begin + local * b.S;
        if(s->start > s->end) { s->start = s->end; }
        s->limit = s->start + b.S < s->end ? s->start + b.S : s->end;
        s->is_first = local == 0;
        s->is_last = s->limit == s->end;
        return true;
}

// Decodes the symbols of a first scan that begin in [st.pos, span.limit) from state st — (bit, block in MCU) in a DC scan,
// (bit, zigzag position) in an AC scan — and returns the blocks completed; an EOBn symbol completes its whole run at the symbol, so
// the state carries no run.  A total function of (state, stream), as decode_symbols is: a prefix that is no code counts as 16 bits
// of the symbol 0, a run past Se ends the block.  kFinal: as decode_symbols' — st is the true state, ord the block's ordinal in the
// scan, end_ord the interval's end; stores, stops behind the interval's last block and reports.
template <bool kFinal>
__device__ __forceinline__ unsigned scans_symbols(const ScanDesc &d, const ScansBuffers &b, const DecodeSpan &span, DecodeState &st, unsigned ord,
                                                  unsigned end_ord, const ScansOut &o, unsigned *errors)
{
        const bool dc = d.kind == kScanDcFirst;
        unsigned completed = 0, bad = 0, diff_at = 0;
        int16_t *block = nullptr;
        if(kFinal && ord < end_ord) { block = scans_block(d, o, ord, &diff_at); }
        for(unsigned n = 0; n < b.S && st.pos < span.limit; n++) {
                if(kFinal && ord >= end_ord) { break; }
                const unsigned w = decode_peek(b.words, b.nwords, st.pos);
                const j2p_huff_decode &tab = b.pool[dc ? d.dc_tab[d.blk_comp[st.blk]] : d.ac_tab];
                unsigned sym;
                const unsigned len = scans_symbol(tab, w, &sym, &bad);
                const unsigned s = sym & 15u, r = sym >> 4;
                unsigned done = 0;              // blocks this symbol completes
                if(dc) {
                        int v = 0;
                        if(s) {
                                v = (int)((w << len) >> (32u - s));
                                if(v < (1 << (s - 1))) { v -= (1 << s) - 1; }
                        }
                        st.pos += len + s;
                        if(kFinal) { o.diff[diff_at] = (unsigned)(v + 32768); }
                        st.blk = st.blk + 1 < d.per_mcu ? st.blk + 1 : 0;
                        done = 1;
                } else if(s == 0 && r < 15) {   // EOBn: this block and the run's others
                        done = 1u << r;
                        if(r) { done += (w << len) >> (32u - r); }
                        st.pos += len + r;
                        st.k = d.ss;
                } else if(s == 0) {
                        st.pos += len;
                        st.k += 16;
                        if(st.k > d.se + 1) { bad |= kDecodeBadRun; }
                        if(st.k > d.se) {
                                st.k = d.ss;
                                done = 1;
                        }
                } else {
                        int v = (int)((w << len) >> (32u - s));
                        if(v < (1 << (s - 1))) { v -= (1 << s) - 1; }
                        st.pos += len + s;
                        st.k += r;
                        if(st.k > d.se) {
                                bad |= kDecodeBadRun;
                        } else if(kFinal && block) {
                                block[kDecodeNatural[st.k]] = (int16_t)(unsigned short)((unsigned)v << d.al);
                        }
                        st.k++;
                        if(st.k > d.se) {
                                st.k = d.ss;
                                done = 1;
                        }
                }
                if(done) {
                        completed += done;
                        if(kFinal) {
                                if(done > end_ord - ord) {
                                        bad |= kDecodeBadEobRun;
                                        done = end_ord - ord;
                                }
                                ord += done;
                                if(ord < end_ord) {
                                        block = scans_block(d, o, ord, &diff_at);
                                } else if(st.pos > span.end || st.pos + 8 <= span.end) {
                                        bad |= kDecodeBadEnd;           // the last symbol crosses the interval's end, or whole bytes are left over
                                }
                        }
                }
        }
        if(kFinal) {
                if(span.is_last && ord < end_ord) { bad |= kDecodeBadEnd; }                             // blocks missing
                *errors |= bad;
        }
        return completed;
}

// the entry state of a scan's interval; and what any state is clamped to, so that a speculative decode indexes nothing outside
__device__ __forceinline__ DecodeState scans_entry(const ScanDesc &d, const DecodeSpan &span) { return DecodeState{span.begin, 0, d.kind == kScanDcFirst ? 0 : d.ss}; }

// One round (k_decode_sync's contract) over the subsequences of all first scans.
__global__ __launch_bounds__(256) void k_scans_sync(ScansBuffers b, unsigned nbound, const unsigned long long *in, unsigned long long *out,
                                                    unsigned long long *last, unsigned *done, unsigned *changed)
{
        const unsigned i = blockIdx.x * 256 + threadIdx.x;
        DecodeSpan span;
        unsigned scan = 0;
        bool again = false;
        if(i < nbound && scans_span(b, i, &span, &scan)) {
                const ScanDesc &d = b.scans[scan];
                DecodeState entry = scans_entry(d, span);
                if(!span.is_first) {
                        entry = decode_unpack(in[i - 1]);
                        if(entry.blk >= d.per_mcu) { entry.blk = 0; }
                        if(d.kind == kScanDcFirst) {
                                entry.k = 0;
                        } else if(entry.k < d.ss || entry.k > d.se) {
                                entry.k = d.ss;
                        }
                        if(entry.pos < span.start) { entry.pos = span.start; }
                }
                const unsigned long long key = decode_pack(entry);
                again = key != last[i];
                if(again) {
                        last[i] = key;
                        unsigned unused = 0;
                        done[i] = scans_symbols<false>(d, b, span, entry, 0, 0, ScansOut{}, &unused);
                        out[i] = decode_pack(entry);
                } else {
                        out[i] = in[i];
                }
        }
        const unsigned long long mask = __ballot(again);
        if(mask && ((int)threadIdx.x & 63) == __ffsll((long long)mask) - 1) { atomicAdd(changed, (unsigned)__popcll(mask)); }
}

// The final pass (k_decode_write's contract).
__global__ __launch_bounds__(256) void k_scans_write(ScansBuffers b, unsigned nbound, const unsigned long long *exit, const unsigned long long *before,
                                                     ScansOut o)
{
        const unsigned i = blockIdx.x * 256 + threadIdx.x;
        DecodeSpan span;
        unsigned scan = 0;
        if(i >= nbound || !scans_span(b, i, &span, &scan)) { return; }
        const ScanDesc &d = b.scans[scan];
        DecodeState entry = scans_entry(d, span);
        unsigned errors = 0;
        if(!span.is_first) { entry = decode_unpack(exit[i - 1]); }
        const unsigned long long per = (unsigned long long)d.ri * d.per_mcu, ord0 = span.interval * per;
        unsigned long long end = ord0 + per, ord = ord0 + (before[i] - before[b.first[d.sub_base + span.interval]]);
        if(end > d.nblocks) { end = d.nblocks; }
        if(ord >= end) { return; }                      // at or behind the interval's last block: padding
        const bool dc = d.kind == kScanDcFirst;
        if(entry.blk >= d.per_mcu || entry.pos < span.start || (dc ? (unsigned)(ord % d.per_mcu) != entry.blk || entry.k != 0 : entry.k < d.ss || entry.k > d.se)) {
                atomicOr(b.error, kDecodeBadState);     // (no true state looks like that)
                return;
        }
        (void)scans_symbols<true>(d, b, span, entry, (unsigned)ord, (unsigned)end, o, &errors);
        if(errors) { atomicOr(b.error, errors); }
}

// sums[j]: the exclusive sum of diff[].  A lane per DC difference of scan `scan` (a DC first scan): the block's predictor is the sum
// of its component's differences from the first block of its restart interval on; coefficient 0 = predictor << Al.
__global__ __launch_bounds__(256) void k_scans_dc(ScansBuffers b, unsigned scan, const unsigned *diff, const unsigned long long *sums, ScansOut o)
{
        const ScanDesc &d = b.scans[scan];
        const unsigned local0 = blockIdx.x * 256 + threadIdx.x;
        if(local0 >= d.nblocks) { return; }
        unsigned ci = 0;
        for(unsigned k = 1; k < d.ncomp; k++) {
                if(local0 >= d.comp_off[k]) { ci = k; }
        }
        const unsigned hs = d.hs[ci], vs = d.vs[ci], bw = d.bw[ci], per = hs * vs;
        const unsigned local = local0 - d.comp_off[ci], mcu = local / per, within = local - mcu * per;
        const unsigned j = d.diff_base + local0, reset = d.diff_base + d.comp_off[ci] + (mcu / d.ri) * d.ri * per;
        const long long dc = ((long long)(sums[j] + diff[j] - sums[reset]) - 32768ll * (long long)(j + 1 - reset)) * (1ll << d.al);
        if(dc < -32768 || dc > 32767) {
                atomicOr(b.error, kDecodeBadDc);
                return;
        }
        const unsigned my = mcu / d.mcus_w, mx = mcu - my * d.mcus_w, jy = within / hs, jx = within - jy * hs;
        const unsigned bx = mx * hs + jx, by = my * vs + jy;
        if(bx < bw && by < d.bh[ci]) { scans_grid(o, d.comp[ci])[((size_t)by * bw + bx) * 64] = (int16_t)dc; }
}

// ---- the refinement scans ----
// A lane per block position of DC refinement scan `scan`: its bit is the interval's first bit plus the position within the interval.
// The interval holds exactly the bytes its blocks' bits need.
__global__ __launch_bounds__(256) void k_scans_dc_refine(ScansBuffers b, unsigned scan, ScansOut o)
{
        const ScanDesc &d = b.scans[scan];
        const unsigned ord = blockIdx.x * 256 + threadIdx.x;
        if(ord >= d.nblocks) { return; }
        const unsigned per = d.ri * d.per_mcu, k = ord / per, local = ord - k * per;
        unsigned long long begin, end;
        scans_interval(b, d, k, &begin, &end);
        if(local == 0) {
                const unsigned n = d.nblocks - k * per < per ? d.nblocks - k * per : per;
                unsigned bad = 0;
                if(end - begin != (n + 7) / 8) { bad = kDecodeBadEnd; }
                if(k == 0 && *d.nmarkers + 1 != d.nint) { bad |= kDecodeBadMarker; }
                if(bad) { atomicOr(b.error, bad); }
        }
        unsigned unused;
        int16_t *const block = scans_block(d, o, ord, &unused);
        const unsigned bit = decode_peek(b.words, b.nwords, begin * 8 + local) >> 31;
        if(block && bit) { block[0] = (int16_t)(block[0] | (int16_t)(1 << d.al)); }
}

__device__ __forceinline__ unsigned long long scans_below(unsigned n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }

// One wavefront per restart interval of AC refinement scan `scan` (a scan of one component: block n of the scan is block n of the
// grid `coef`), lane k for the coefficient at zigzag position k.  Per block one ballot gives the positions of the band that were
// non-zero when the scan reached it (the history mask); the symbol walk is wave-uniform: every lane reads the same symbol, the
// positions a symbol passes follow from the mask, and every lane whose coefficient is passed finds its own correction bit at the
// symbol's end plus the number of passed positions below it.
__global__ __launch_bounds__(256) void k_scans_ac_refine(ScansBuffers b, unsigned scan, int16_t *coef)
{
        const ScanDesc &d = b.scans[scan];
        const unsigned lane = threadIdx.x & 63u;
        const unsigned k_int = blockIdx.x * 4 + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        if(k_int >= d.nint) { return; }
        const j2p_huff_decode &tab = b.pool[d.ac_tab];
        const unsigned ss = d.ss, se = d.se;
        const int p1 = 1 << d.al;
        const unsigned long long band = scans_below(se + 1) & ~scans_below(ss), mine = 1ull << lane, below_me = mine - 1;
        const unsigned nat = kDecodeNatural[lane];
        unsigned long long begin, end;
        scans_interval(b, d, k_int, &begin, &end);
        unsigned long long pos = begin * 8;
        const unsigned long long pos_end = end * 8;
        unsigned bad = 0, eobrun = 0;
        if(k_int == 0 && *d.nmarkers + 1 != d.nint) { bad |= kDecodeBadMarker; }
        const unsigned n0 = k_int * d.ri, n1 = d.nblocks - n0 < d.ri ? d.nblocks : n0 + d.ri;
        for(unsigned n = n0; n < n1; n++) {
                int16_t *const block = coef + (size_t)n * 64;
                const int was = block[nat];
                int now = was;
                const unsigned long long M = __ballot(was != 0) & band;
                unsigned k = ss;
                unsigned long long passed = 0;  // the positions a symbol passes: their correction bits begin at `pos`
                if(eobrun == 0) {
                        for(unsigned it = 0; it < 64 && k <= se; it++) {
                                const unsigned w = decode_peek(b.words, b.nwords, pos);
                                unsigned sym;
                                const unsigned len = scans_symbol(tab, w, &sym, &bad);
                                const unsigned r = sym >> 4;
                                unsigned s = sym & 15u;
                                if(s == 0 && r < 15) {
                                        eobrun = 1u << r;
                                        if(r) { eobrun += (w << len) >> (32u - r); }
                                        pos += len + r;
                                        break;
                                }
                                if(s > 1) {
                                        bad |= kDecodeBadRefine;
                                        s = 1;
                                }
                                const unsigned sign = s ? (w << len) >> 31 : 0u;
                                pos += len + s;
                                // k': the (r + 1)-th position from k on that was zero
                                unsigned long long Z = ~M & band & ~scans_below(k);
                                for(unsigned q = 0; q < r; q++) { Z &= Z - 1; }
                                unsigned kp = se + 1;
                                if(Z) {
                                        kp = (unsigned)__ffsll((long long)Z) - 1;
                                } else {
                                        bad |= kDecodeBadRun;
                                }
                                passed = M & scans_below(kp) & ~scans_below(k);
                                if(passed & mine) {
                                        const unsigned bit = decode_peek(b.words, b.nwords, pos + (unsigned)__popcll(passed & below_me)) >> 31;
                                        if(bit && (now & p1) == 0) { now += now >= 0 ? p1 : -p1; }
                                }
                                pos += (unsigned)__popcll(passed);
                                if(s && Z && lane == kp) { now = sign ? p1 : -p1; }
                                k = kp + 1;
                        }
                }
                if(eobrun > 0) {
                        // the rest of the band (all of it in the run's later blocks): correction bits only
                        passed = M & ~scans_below(k);
                        if(passed & mine) {
                                const unsigned bit = decode_peek(b.words, b.nwords, pos + (unsigned)__popcll(passed & below_me)) >> 31;
                                if(bit && (now & p1) == 0) { now += now >= 0 ? p1 : -p1; }
                        }
                        pos += (unsigned)__popcll(passed);
                        eobrun--;
                }
                if(now != was) { block[nat] = (int16_t)now; }
        }
        if(eobrun > 0) { bad |= kDecodeBadEobRun; }
        if(pos > pos_end || pos + 8 <= pos_end) { bad |= kDecodeBadEnd; }
        if(bad && lane == 0) { atomicOr(b.error, bad); }
}

}  // namespace j2p
