// jpeg2png_amd — gfx950 device code of the progressive JPEG coder: the scans of libjpeg's jpeg_simple_progression() from the
// quantised coefficients in device memory (include/jpeg2png_amd.h: "The progressive JPEG file").  Included by j2p_codec.hip
// alone, behind j2p_codec_kernels.hip.h, whose scan geometry (ScanGeom, scan_block, scan_dc_predictor), exclusive sums
// (k_scan_*) and byte stuffing (k_stuff_*) it uses as they are; it adds no line to them.  Restart intervals (the kRestart bodies
// below, k_restart_* and k_stuff_*_restart there) cut the scans into intervals of items that each end on a byte.
//
// Every scan is a row of ITEMS whose bits follow each other in the scan's stream: a DC scan's items are the positions of
// the interleaved scan (dummy blocks included), an AC scan's the blocks of its one component in raster order.  What makes
// an AC scan's items independent is the framing of the EOB run: an item's bits are
//   1. the block's own symbols (with the correction bits that libjpeg emits behind each of them),
//   2. if the block STARTS an EOB run, the run's EOBn symbol and its extra bits,
//   3. the block's tail correction bits (refinement scans: those behind its last newly non-zero coefficient),
// which is stream order: a run's symbol is written when the run is flushed, in front of the correction bits of all its
// blocks, and its first block's own symbols came before that.  So one exclusive sum over the items' lengths places
// everything, as in the baseline coder.  The passes of an AC scan, each a launch (order between workgroups comes from
// launch boundaries only; nobody waits for anybody):
//   k_prog_classify     a wavefront per block, a lane per zigzag position: two __ballots give the block's flag byte —
//                       bit 7: it emits symbols (ends the pending run), bit 6: it ends in a tail (joins a run), bits 0..5:
//                       its tail correction bits
//   k_prog_runs         a lane per block; the lane of a block that begins a SEGMENT (block 0, or a block that emits) walks
//                       the segment's flag bytes up to the next emitting block and cuts it into runs as libjpeg does:
//                       at 32767 blocks, and in a refinement scan once more than 937 correction bits wait     -> run[], zeroed before
//   k_prog_ac<COUNT>    a lane per block walks the band as libjpeg's encode_mcu_AC_first / _refine do and counts the
//                       symbols (the EOBn of run[] included) in an LDS histogram                              -> hist[]
//   k_prog_ac<LENGTH>   the same walk with the scan's table: the item's bits                                    -> len[]
//   k_prog_ac<PACK>     the same walk at the item's bit offset into the zeroed stream
// and of a DC scan k_prog_dc<COUNT / LENGTH / PACK>, a lane per position.  The three modes are ONE walk with three sinks, so
// what is counted and measured is what is written.  A lane writes whole 32-bit words of its item with plain stores and the
// first and the last, which it may share with its neighbours, with atomic ORs into zeroed memory: the bytes do not depend on
// timing.  The lane of a scan's last item completes the last byte with 1-bits.
// A lane per block reads its 64 coefficients one by one, 128 bytes apart from its neighbours': the walk is the sequential
// one by choice (DESIGN.md section 25 says what it costs and what a lane per coefficient would take).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace j2p {

constexpr unsigned kProgEobRunMax = 0x7fff;     // libjpeg flushes a run that has reached this many blocks
constexpr unsigned kProgCorrectionMax = 937;    // ... and one whose waiting correction bits EXCEED this (MAX_CORR_BITS - DCTSIZE2 + 1)
constexpr unsigned kProgHistogram = 512;        // 64-bit counters of one scan: [table of component 0 or of the AC scan][the others' DC table]

enum { kProgCount = 0, kProgLength = 1, kProgPack = 2 };

// one scan's parameters, as a kernel argument
struct ProgScan {
        unsigned ss, se, al;    // the band Ss..Se and the point transform Al
        unsigned refine;        // Ah != 0
        unsigned n;             // items
};
// the codes of the (at most two) tables of one scan: (code length << 16) | code, 0 for a symbol the table has not got
struct ProgCodes {
        unsigned code[2][256];
};

// ---- the three sinks of a walk ----
struct ProgCountSink {
        unsigned *hist;         // LDS, 256 counters of the item's table
        __device__ __forceinline__ void symbol(unsigned s) { atomicAdd(&hist[s & 255u], 1u); }
        __device__ __forceinline__ void bits(unsigned, unsigned) {}
};
struct ProgLengthSink {
        const unsigned *code;   // LDS
        unsigned n;
        __device__ __forceinline__ void symbol(unsigned s) { n += code[s & 255u] >> 16; }
        __device__ __forceinline__ void bits(unsigned, unsigned length) { n += length; }
};
// bits at a bit offset of the stream: `cur` holds the `filled` bits of the word being completed, highest first
struct ProgPackSink {
        const unsigned *code;   // LDS
        unsigned *word;
        unsigned cur, filled;
        bool first;             // nothing has gone out yet: the word may hold a neighbour's bits
        __device__ __forceinline__ ProgPackSink(const unsigned *codes, unsigned *stage, unsigned long long at)
                : code(codes), word(stage + (size_t)(at >> 5)), cur(0), filled((unsigned)(at & 31u)), first(true)
        {
        }
        __device__ __forceinline__ void bits(unsigned v, unsigned length)      // length <= 32, v below 2^length
        {
                if(length == 0) { return; }
                const unsigned long long x = ((unsigned long long)cur << 32) | ((unsigned long long)v << (64u - filled - length));
                filled += length;
                if(filled >= 32u) {
                        const unsigned w = __builtin_bswap32((unsigned)(x >> 32));      // the stream is bytes: big-endian words
                        if(first) {
                                if(w) { atomicOr(word, w); }
                                first = false;
                        } else {
                                *word = w;
                        }
                        word++;
                        cur = (unsigned)x;
                        filled -= 32u;
                } else {
                        cur = (unsigned)(x >> 32);
                }
        }
        __device__ __forceinline__ void symbol(unsigned s)
        {
                const unsigned e = code[s & 255u];
                bits(e & 0xffffu, e >> 16);
        }
        // the last, incomplete word; pad: complete the last byte with 1-bits first (the scan's last item)
        __device__ __forceinline__ void finish(bool pad)
        {
                if(pad) {
                        const unsigned short_of = (8u - (filled & 7u)) & 7u;
                        bits((1u << short_of) - 1u, short_of);
                }
                if(filled && cur) { atomicOr(word, __builtin_bswap32(cur)); }
        }
};

// up to 63 bits, the first one highest
template <class Sink>
__device__ __forceinline__ void prog_bits64(Sink &o, unsigned long long v, unsigned length)
{
        if(length > 32u) {
                o.bits((unsigned)(v >> 32), length - 32u);
                o.bits((unsigned)v, 32u);
        } else {
                o.bits((unsigned)v, length);
        }
}

// ---- the walks: libjpeg's encode_mcu_AC_first and encode_mcu_AC_refine of ONE block, without the EOB run ----
template <class Sink>
__device__ __forceinline__ void prog_ac_first(const int16_t *blk, const ProgScan &p, Sink &o)
{
        unsigned r = 0;
        for(unsigned k = p.ss; k <= p.se; k++) {
                const int v = blk[kZigzagNatural[k]];
                const unsigned a = (unsigned)(v < 0 ? -v : v) >> p.al;   // the shift applies to the absolute value
                if(a == 0) {
                        r++;
                        continue;
                }
                for(; r > 15u; r -= 16u) { o.symbol(0xf0u); }
                const unsigned s = 32u - (unsigned)__clz((int)a);
                o.symbol((r << 4) | s);
                o.bits((v < 0 ? ~a : a) & ((1u << s) - 1u), s);
                r = 0;
        }
}
// *tail, *ntail: the correction bits behind the block's last newly non-zero coefficient, which wait with the EOB run
template <class Sink>
__device__ __forceinline__ void prog_ac_refine(const int16_t *blk, const ProgScan &p, bool emits, Sink &o, unsigned long long *tail, unsigned *ntail)
{
        unsigned eob = 0;               // the last coefficient that becomes non-zero in this scan
        if(emits) {
                for(unsigned k = p.ss; k <= p.se; k++) {
                        const int v = blk[kZigzagNatural[k]];
                        if(((unsigned)(v < 0 ? -v : v) >> p.al) == 1u) { eob = k; }
                }
        }
        unsigned r = 0, nwait = 0;
        unsigned long long wait = 0;    // correction bits since the last symbol
        for(unsigned k = p.ss; k <= p.se; k++) {
                const int v = blk[kZigzagNatural[k]];
                const unsigned a = (unsigned)(v < 0 ? -v : v) >> p.al;
                if(a == 0) {
                        r++;
                        continue;
                }
                while(r > 15u && k <= eob) {
                        o.symbol(0xf0u);
                        r -= 16u;
                        prog_bits64(o, wait, nwait);
                        wait = 0;
                        nwait = 0;
                }
                if(a > 1u) {            // non-zero before this scan: its next bit
                        wait = (wait << 1) | (a & 1u);
                        nwait++;
                        continue;
                }
                o.symbol((r << 4) | 1u);
                o.bits(v < 0 ? 0u : 1u, 1u);
                prog_bits64(o, wait, nwait);
                wait = 0;
                nwait = 0;
                r = 0;
        }
        *tail = wait;
        *ntail = nwait;
}

// ---- k_prog_classify: flags[block] of one AC scan ----
constexpr unsigned kProgEmits = 0x80u, kProgTail = 0x40u, kProgTailBits = 0x3fu;

__global__ __launch_bounds__(256) void k_prog_classify(const int16_t *coef, ProgScan p, uint8_t *flags)
{
        const int lane = (int)threadIdx.x & 63;
        const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const unsigned first = (blockIdx.x * 4 + wave) * kEntropyIters;
        for(unsigned it = 0; it < kEntropyIters && first + it < p.n; it++) {
                const unsigned b = first + it;
                const int v = coef[(size_t)b * 64 + kZigzagNatural[lane]];
                const bool in_band = (unsigned)lane >= p.ss && (unsigned)lane <= p.se;
                const unsigned a = in_band ? (unsigned)(v < 0 ? -v : v) >> p.al : 0u;
                const unsigned long long nz = __ballot(a != 0), one = __ballot(a == 1u);
                unsigned f;
                if(!p.refine) {
                        f = (nz ? kProgEmits : 0u) | ((nz >> p.se) & 1ull ? 0u : kProgTail);
                } else {
                        // behind the last newly non-zero coefficient: zeros (a run) and corrections (tail bits)
                        const unsigned eob = one ? 63u - (unsigned)__clzll((long long)one) : 0u;
                        const unsigned long long behind = one ? ~((2ull << eob) - 1ull) : ~0ull;
                        f = (one ? kProgEmits : 0u) | (!one || eob < p.se ? kProgTail : 0u) | (unsigned)__popcll(nz & ~one & behind);
                }
                if(lane == 0) { flags[b] = (uint8_t)f; }
        }
}

// ---- k_prog_runs: run[block] = the length of the EOB run that STARTS at the block; *flushes += the runs ----
// run[] arrives zeroed: only the blocks that start a run are written, each by the one lane that walks its segment.  A segment is
// walked by ONE lane, sixteen flag bytes a load with the next load already under way: an image that is one segment (no block
// emits: a flat image, or a refinement scan that meets no new coefficient) is walked by one lane alone (DESIGN.md section 25:
// measured).
// kRestart (include/jpeg2png_amd.h: "Restart intervals"): the scan has restart intervals of ri blocks, and a block that begins an
// interval begins a segment too — an EOB run never spans a marker; without it ri is not read.
template <bool kRestart>
struct ProgRunWalk {
        unsigned *run;
        unsigned first, refine, ri;
        unsigned length = 0, waiting = 0, start = 0, made = 0;
        // block i with flag byte f; true: it emits (or begins an interval), the segment ended in front of it
        __device__ __forceinline__ bool step(unsigned f, unsigned i)
        {
                if(i > first && ((f & kProgEmits) || (kRestart && i % ri == 0))) { return true; }
                if(f & kProgTail) {
                        if(length == 0) { start = i; }
                        length++;
                        waiting += f & kProgTailBits;
                        if(length == kProgEobRunMax || waiting > kProgCorrectionMax) { flush(); }
                }
                return false;
        }
        // the four blocks of one word of flags, from block `at`; those that only lengthen the run — no emitter, a tail each, no
        // correction bits — at once
        __device__ __forceinline__ bool four(unsigned word, unsigned at)
        {
                // (with intervals: only where none of the four begins one — length > 0 puts `at` behind the segment's first block)
                if(word == 0x40404040u && length > 0 && length + 4 < kProgEobRunMax && (!kRestart || (at % ri != 0 && at % ri + 4 <= ri))) {
                        length += 4;
                        return false;
                }
                return step(word & 255u, at) || step((word >> 8) & 255u, at + 1) || step((word >> 16) & 255u, at + 2) || step(word >> 24, at + 3);
        }
        __device__ __forceinline__ void flush()
        {
                if(length) {
                        run[start] = length;
                        made++;
                }
                length = 0;
                waiting = 0;
        }
};

template <bool kRestart>
__device__ __forceinline__ void prog_runs(const uint8_t *flags, const ProgScan &p, unsigned *run, unsigned long long *flushes, unsigned ri)
{
        const unsigned b = blockIdx.x * 256 + threadIdx.x;
        if(b >= p.n) { return; }
        if(b != 0 && !(flags[b] & kProgEmits) && !(kRestart && b % ri == 0)) { return; }
        ProgRunWalk<kRestart> w = {run, b, p.refine, ri};
        unsigned i = b;
        bool ended = false;
        for(; i < p.n && (i & 15u) && !ended; i++) { ended = w.step(flags[i], i); }
        if(!ended && i + 16 <= p.n) {
                // (flags + i is 16-aligned: the array is, and i is)
                const uint4 *from = reinterpret_cast<const uint4 *>(flags + i);
                const uint4 head = *from;
                unsigned c0 = head.x, c1 = head.y, c2 = head.z, c3 = head.w;
                for(;;) {
                        const bool more = i + 32 <= p.n;
                        unsigned n0 = 0, n1 = 0, n2 = 0, n3 = 0;
                        if(more) {
                                const uint4 next = *++from;
                                n0 = next.x, n1 = next.y, n2 = next.z, n3 = next.w;
                        }
                        ended = w.four(c0, i) || w.four(c1, i + 4) || w.four(c2, i + 8) || w.four(c3, i + 12);
                        if(ended) { break; }
                        i += 16;
                        if(!more) { break; }
                        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
                }
        }
        for(; i < p.n && !ended; i++) { ended = w.step(flags[i], i); }
        w.flush();
        if(w.made) { atomicAdd(flushes, (unsigned long long)w.made); }
}
__global__ __launch_bounds__(256) void k_prog_runs(const uint8_t *flags, ProgScan p, unsigned *run, unsigned long long *flushes)
{
        prog_runs<false>(flags, p, run, flushes, 0);
}
__global__ __launch_bounds__(256) void k_prog_runs_restart(const uint8_t *flags, ProgScan p, unsigned ri, unsigned *run, unsigned long long *flushes)
{
        prog_runs<true>(flags, p, run, flushes, ri);
}

// the scan's table(s) into LDS
__device__ __forceinline__ void prog_tables(const ProgCodes &h, unsigned (*tab)[256])
{
        for(unsigned i = threadIdx.x; i < 512; i += 256) { tab[i >> 8][i & 255u] = h.code[i >> 8][i & 255u]; }
        __syncthreads();
}
// a workgroup's counts into the scan's 64-bit counters
__device__ __forceinline__ void prog_counts_out(const unsigned *count, unsigned long long *hist)
{
        __syncthreads();
        for(unsigned i = threadIdx.x; i < kProgHistogram; i += 256) {
                if(const unsigned n = count[i]) { atomicAdd(&hist[i], (unsigned long long)n); }
        }
}

// ---- k_prog_ac: one AC scan of component `coef`, a lane per block ----
// off: the bit offsets of ALL scans' items (one exclusive sum), off[0] this scan's first item's — the scan's stream starts
// there; stage: the scan's stream, zeroed.  hist: COUNT only; h: LENGTH and PACK; len: LENGTH; off, stage: PACK.
// kRestart: intervals of ri blocks (run[] is k_prog_runs_restart's); the lane of every interval's last block completes its byte.
template <int MODE, bool kRestart>
__device__ __forceinline__ void prog_ac(const int16_t *coef, const ProgScan &p, const uint8_t *flags, const unsigned *run, const ProgCodes &h,
                                        unsigned long long *hist, unsigned *len, const unsigned long long *off, unsigned *stage, unsigned ri)
{
        __shared__ unsigned lds[kProgHistogram];
        if constexpr(MODE == kProgCount) {
                for(unsigned i = threadIdx.x; i < kProgHistogram; i += 256) { lds[i] = 0; }
                __syncthreads();
        } else {
                prog_tables(h, reinterpret_cast<unsigned(*)[256]>(lds));
        }
        const unsigned b = blockIdx.x * 256 + threadIdx.x;
        if(b < p.n) {
                const unsigned f = flags[b], started = run[b];
                const int16_t *blk = coef + (size_t)b * 64;
                const auto item = [&](auto &o) {
                        unsigned long long tail = 0;
                        unsigned ntail = 0;
                        if(p.refine) {
                                if((f & kProgEmits) || (f & kProgTailBits)) { prog_ac_refine(blk, p, (f & kProgEmits) != 0, o, &tail, &ntail); }
                        } else if(f & kProgEmits) {
                                prog_ac_first(blk, p, o);
                        }
                        if(started) {
                                const unsigned extra = 31u - (unsigned)__clz((int)started);
                                o.symbol(extra << 4);
                                o.bits(started & ((1u << extra) - 1u), extra);
                        }
                        prog_bits64(o, tail, ntail);
                };
                if constexpr(MODE == kProgCount) {
                        ProgCountSink o = {lds};
                        item(o);
                } else if constexpr(MODE == kProgLength) {
                        ProgLengthSink o = {lds, 0};
                        item(o);
                        len[b] = o.n;
                } else {
                        ProgPackSink o(lds, stage, off[b] - off[0]);
                        item(o);
                        o.finish(b == p.n - 1 || (kRestart && (b + 1) % ri == 0));
                }
        }
        if constexpr(MODE == kProgCount) { prog_counts_out(lds, hist); }
}
template <int MODE>
__global__ __launch_bounds__(256) void k_prog_ac(const int16_t *coef, ProgScan p, const uint8_t *flags, const unsigned *run, ProgCodes h,
                                                 unsigned long long *hist, unsigned *len, const unsigned long long *off, unsigned *stage)
{
        prog_ac<MODE, false>(coef, p, flags, run, h, hist, len, off, stage, 0);
}
// (COUNT and LENGTH have no sibling: what a block counts and measures depends on run[] alone)
__global__ __launch_bounds__(256) void k_prog_ac_pack_restart(const int16_t *coef, ProgScan p, unsigned ri, const uint8_t *flags, const unsigned *run,
                                                              ProgCodes h, const unsigned long long *off, unsigned *stage)
{
        prog_ac<kProgPack, true>(coef, p, flags, run, h, nullptr, nullptr, off, stage, ri);
}

// ---- k_prog_dc: a DC scan of all components, a lane per position of the interleaved scan ----
// first scan (Ah 0): the difference of DC >> Al against the component's previous position, category and magnitude bits as in the
// baseline scan, table 0 for component 0 and table 1 for the others; refinement: the bit Al of the DC, no table.  A dummy block
// holds its predecessor's DC: difference 0, and its predecessor's bit.
// kRestart: intervals of ri positions — the predictor is scan_dc_predictor_restart's, and the lane of every interval's last position
// completes its byte.
template <int MODE, bool kRestart>
__device__ __forceinline__ void prog_dc(const ScanGeom &g, const ProgScan &p, const ProgCodes &h, unsigned long long *hist, unsigned *len,
                                        const unsigned long long *off, unsigned *stage, unsigned ri)
{
        __shared__ unsigned lds[kProgHistogram];
        if constexpr(MODE == kProgCount) {
                for(unsigned i = threadIdx.x; i < kProgHistogram; i += 256) { lds[i] = 0; }
                __syncthreads();
        } else {
                prog_tables(h, reinterpret_cast<unsigned(*)[256]>(lds));
        }
        const unsigned slot = blockIdx.x * 256 + threadIdx.x;
        if(slot < p.n) {
                unsigned c;
                size_t block;
                const bool real = scan_block(g, slot, c, block);
                const int before = kRestart ? scan_dc_predictor_restart(g, slot, ri) : scan_dc_predictor(g, slot);
                const int dc = real ? g.coef[c][block * 64] : before;
                const unsigned t = c ? 1u : 0u;
                const auto item = [&](auto &o) {
                        if(p.refine) {
                                o.bits((unsigned)(dc >> p.al) & 1u, 1u);
                                return;
                        }
                        const int d = (dc >> p.al) - (before >> p.al);   // arithmetic shifts
                        const unsigned a = (unsigned)(d < 0 ? -d : d), s = 32u - (unsigned)__clz((int)a);
                        o.symbol(s);
                        o.bits((unsigned)(d < 0 ? d - 1 : d) & ((1u << s) - 1u), s);
                };
                if constexpr(MODE == kProgCount) {
                        ProgCountSink o = {lds + 256 * t};
                        item(o);
                } else if constexpr(MODE == kProgLength) {
                        ProgLengthSink o = {lds + 256 * t, 0};
                        item(o);
                        len[slot] = o.n;
                } else {
                        ProgPackSink o(lds + 256 * t, stage, off[slot] - off[0]);
                        item(o);
                        o.finish(slot == p.n - 1 || (kRestart && (slot + 1) % ri == 0));
                }
        }
        if constexpr(MODE == kProgCount) { prog_counts_out(lds, hist); }
}
template <int MODE>
__global__ __launch_bounds__(256) void k_prog_dc(ScanGeom g, ProgScan p, ProgCodes h, unsigned long long *hist, unsigned *len,
                                                 const unsigned long long *off, unsigned *stage)
{
        prog_dc<MODE, false>(g, p, h, hist, len, off, stage, 0);
}
template <int MODE>
__global__ __launch_bounds__(256) void k_prog_dc_restart(ScanGeom g, ProgScan p, unsigned ri, ProgCodes h, unsigned long long *hist, unsigned *len,
                                                         const unsigned long long *off, unsigned *stage)
{
        prog_dc<MODE, true>(g, p, h, hist, len, off, stage, ri);
}

}  // namespace j2p
