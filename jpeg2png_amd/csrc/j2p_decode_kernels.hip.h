// jpeg2png_amd — device code that READS a JPEG file: the entropy-coded data of one baseline scan Huffman-decoded into the
// int16 coefficient grids (include/jpeg2png_amd.h: "Reading a JPEG file"; the argument: DESIGN.md section 21).  Included by
// j2p_codec.hip behind j2p_codec_kernels.hip.h, whose k_scan_* kernels it reuses.  The passes, each a launch or a few;
// order between workgroups comes from launch boundaries only, nobody waits for anybody:
//   k_unstuff_count      bytes kept and RSTn markers per 256-byte chunk of the data, k_scan_* twice     -> keepoff[], markoff[]
//   k_unstuff_copy       the clean bit stream (no 00 behind FF, no markers, no fill bytes); every marker's byte offset in it
//   k_decode_intervals   subsequences per restart interval, k_scan_*                                    -> first[]
//   k_decode_sync        one ROUND: every subsequence whose entry state changed is decoded again        -> exit[], done[]
//   k_scan_*             blocks completed per subsequence                                               -> the block ordinals
//   k_decode_write       every subsequence once more from its true state: ACs into the grids, DC differences by ordinal
//   k_scan_*, k_decode_dc  the DC differences summed per component and interval into coefficient 0
// Every loop has a trip count the host knows: a symbol takes at least one bit and starts inside its subsequence, a search
// over the intervals halves its range, a block has 64 positions.  Every read of the stream is clamped to its buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "j2p_internal.h"

namespace j2p {

constexpr int kUnstuffChunk = 256;      // bytes of the file's data per wavefront of the k_unstuff_* kernels (64 lanes x 4)

// the error flags the kernels OR into one word; any of them is J2P_EFORMAT
constexpr unsigned kDecodeBadMarker = 1;        // an RSTn out of sequence, one too many or too few, an empty interval
constexpr unsigned kDecodeBadCode = 2;          // a prefix that is no code of the table
constexpr unsigned kDecodeBadRun = 4;           // a run past coefficient 63
constexpr unsigned kDecodeBadEnd = 8;           // a symbol across the end of its interval, blocks missing, bytes left over
constexpr unsigned kDecodeBadState = 16;        // the block ordinal disagrees with the state
constexpr unsigned kDecodeBadDc = 32;           // a DC value outside int16

// what the decode kernels know of the file; lives in device memory behind the tables and is copied to LDS with them, so
// that its small arrays are indexed there and not in scratch memory
struct DecodeGeom {
        unsigned ncomp, per_mcu, mcus_w, nmcus;
        unsigned ri;                    // MCUs per restart interval (nmcus without restarts)
        unsigned nint;                  // intervals
        unsigned nblocks;               // nmcus * per_mcu
        unsigned S;                     // bits per subsequence
        unsigned bw[3], bh[3];          // the delivered grids
        unsigned hs[3], vs[3];          // blocks of a component in an MCU, across and down
        unsigned first_blk[3];          // where a component's blocks begin in the MCU
        unsigned comp_base[3];          // where a component's DC differences begin: nmcus * the blocks of the components before
        unsigned dc_tab[3], ac_tab[3];  // table slots
        unsigned blk_comp[12];          // [block of the MCU] its component
};
struct DecodeTables {
        j2p_huff_decode tab[8];         // DC slots 0..3, AC slots 0..3
        DecodeGeom g;
};
static_assert(sizeof(DecodeTables) % 4 == 0 && sizeof(DecodeTables) <= 12 * 1024, "the tables are copied to LDS word by word");

// the buffers of one decode, all device memory
struct DecodeBuffers {
        const DecodeTables *tables;
        const unsigned *words;          // the clean stream, big-endian bytes; nwords words of which the tail is FF
        unsigned long long nwords;
        const unsigned long long *clean_bytes;  // its length (the total of the kept-byte scan)
        const unsigned long long *nmarkers;     // the RSTn markers found (the total of the marker scan)
        const unsigned long long *rst;          // [nint] clean byte offset of marker m (the end of interval m)
        const unsigned long long *first;        // [nint] first subsequence of interval k (a scan's output)
        const unsigned long long *nsub;         // the total of that scan: subsequences in all
        unsigned *error;
};

__device__ __forceinline__ void decode_tables_to_lds(const DecodeTables *src, DecodeTables *lds)
{
        const unsigned *s = reinterpret_cast<const unsigned *>(src);
        unsigned *d = reinterpret_cast<unsigned *>(lds);
        for(unsigned i = threadIdx.x; i < sizeof(DecodeTables) / 4; i += blockDim.x) { d[i] = s[i]; }
        __syncthreads();
}

// ---- unstuffing: a wavefront per kUnstuffChunk bytes of the data, a lane per 4 of them ----
// Byte i is KEPT when it is data: not FF and not behind an FF (that would be the stuffed 00, or a marker's second byte), or an
// FF in front of a 00.  An FF in front of anything else is a fill byte or a marker's first byte.  It is a MARK when it is the Dn
// of an RSTn.  The byte in front of the data is the SOS segment's last (00); the one behind it is a marker's FF.
__device__ __forceinline__ void unstuff_classify(const uint8_t *raw, size_t nraw, size_t i0, unsigned bytes[4], unsigned *keep, unsigned *mark)
{
        unsigned prev = i0 > 0 && i0 - 1 < nraw ? raw[i0 - 1] : 0u;
        *keep = 0;
        *mark = 0;
        for(unsigned k = 0; k < 4; k++) {
                const size_t i = i0 + k;
                const unsigned cur = i < nraw ? raw[i] : 0xffu, next = i + 1 < nraw ? raw[i + 1] : 0xd9u;
                bytes[k] = cur;
                if(i < nraw) {
                        const bool kept = cur != 0xffu ? prev != 0xffu : next == 0u;
                        *keep |= (unsigned)kept << k;
                        *mark |= (unsigned)(prev == 0xffu && (cur & 0xf8u) == 0xd0u) << k;
                }
                prev = cur;
        }
}

__global__ __launch_bounds__(256) void k_unstuff_count(const uint8_t *raw, size_t nraw, unsigned nchunks, unsigned *keep_count, unsigned *mark_count)
{
        const int lane = (int)threadIdx.x & 63;
        const unsigned chunk = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        if(chunk >= nchunks) { return; }
        unsigned bytes[4], keep, mark;
        unstuff_classify(raw, nraw, (size_t)chunk * kUnstuffChunk + (size_t)lane * 4, bytes, &keep, &mark);
        unsigned nk = (unsigned)__popc(keep), nm = (unsigned)__popc(mark);
#pragma unroll
        for(int d = 32; d >= 1; d >>= 1) {
                nk += __shfl_xor(nk, d);
                nm += __shfl_xor(nm, d);
        }
        if(lane == 0) {
                keep_count[chunk] = nk;
                mark_count[chunk] = nm;
        }
}

// clean: the kept bytes in order; rst[m]: how many bytes were kept in front of marker m, for the nint - 1 markers the scan must
// have; marker m must be RST(m mod 8)
__global__ __launch_bounds__(256) void k_unstuff_copy(const uint8_t *raw, size_t nraw, unsigned nchunks, const unsigned long long *keepoff,
                                                      const unsigned long long *markoff, unsigned nint, uint8_t *clean, size_t clean_room,
                                                      unsigned long long *rst, unsigned *error)
{
        const int lane = (int)threadIdx.x & 63;
        const unsigned chunk = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        if(chunk >= nchunks) { return; }
        unsigned bytes[4], keep, mark;
        unstuff_classify(raw, nraw, (size_t)chunk * kUnstuffChunk + (size_t)lane * 4, bytes, &keep, &mark);
        const unsigned nk = (unsigned)__popc(keep), nm = (unsigned)__popc(mark);
        unsigned ik = nk, im = nm;
#pragma unroll
        for(int d = 1; d < 64; d <<= 1) {
                const unsigned uk = __shfl_up(ik, d), um = __shfl_up(im, d);
                if(lane >= d) {
                        ik += uk;
                        im += um;
                }
        }
        unsigned long long at = keepoff[chunk] + (ik - nk), m = markoff[chunk] + (im - nm);
        unsigned bad = 0;
#pragma unroll
        for(unsigned k = 0; k < 4; k++) {
                if(keep >> k & 1u) {
                        if(at < clean_room) { clean[at] = (uint8_t)bytes[k]; }
                        at++;
                }
                if(mark >> k & 1u) {
                        if(m + 1 < nint) {
                                rst[m] = at;
                                if((bytes[k] & 7u) != (unsigned)(m & 7u)) { bad = kDecodeBadMarker; }
                        } else {
                                bad = kDecodeBadMarker;
                        }
                        m++;
                }
        }
        if(bad) { atomicOr(error, bad); }
}

// ---- the intervals ----
// interval k of the clean stream, in bytes: between marker k - 1 and marker k; clamped, so that a damaged file's offsets lead nowhere
__device__ __forceinline__ void decode_interval(const DecodeBuffers &b, unsigned nint, unsigned k, unsigned long long *begin, unsigned long long *end)
{
        const unsigned long long all = *b.clean_bytes;
        unsigned long long lo = k ? b.rst[k - 1] : 0ull, hi = k + 1 < nint ? b.rst[k] : all;
        if(hi > all) { hi = all; }
        if(lo > hi) { lo = hi; }
        *begin = lo;
        *end = hi;
}

__global__ __launch_bounds__(256) void k_decode_intervals(DecodeBuffers b, unsigned nint, unsigned S, unsigned *count)
{
        const unsigned k = blockIdx.x * 256 + threadIdx.x;
        if(k >= nint) { return; }
        unsigned bad = 0;
        if(k == 0 && *b.nmarkers + 1 != nint) { bad = kDecodeBadMarker; }
        unsigned long long begin, end;
        decode_interval(b, nint, k, &begin, &end);
        if(begin == end) { bad = kDecodeBadMarker; }
        count[k] = (unsigned)(((end - begin) * 8 + S - 1) / S);
        if(bad) { atomicOr(b.error, bad); }
}

// ---- decoding ----
// the decoder's state at a subsequence boundary: the bit where the next symbol begins, the block's index within the MCU and
// the zigzag position (0: the DC symbol comes next), as one word
struct DecodeState {
        unsigned long long pos;
        unsigned blk, k;
};
__device__ __forceinline__ unsigned long long decode_pack(const DecodeState &s) { return (s.pos << 16) | ((unsigned long long)s.blk << 8) | s.k; }
__device__ __forceinline__ DecodeState decode_unpack(unsigned long long v)
{
        DecodeState s;
        s.pos = v >> 16;
        s.blk = (unsigned)(v >> 8) & 0xffu;
        s.k = (unsigned)v & 0xffu;
        return s;
}

// the 32 bits of the stream from bit `pos`; bits beyond the buffer are 1s
__device__ __forceinline__ unsigned decode_peek(const unsigned *words, unsigned long long nwords, unsigned long long pos)
{
        const unsigned long long w = pos >> 5;
        const unsigned b = (unsigned)pos & 31u;
        const unsigned hi = w < nwords ? __builtin_bswap32(words[w]) : 0xffffffffu;
        const unsigned lo = w + 1 < nwords ? __builtin_bswap32(words[w + 1]) : 0xffffffffu;
        return b ? (hi << b) | (lo >> (32u - b)) : hi;
}

// where subsequence i lies: its interval, the bits [start, limit) its symbols begin in, its interval's end, whether it is
// the interval's first and last.  false: there is no such subsequence.
struct DecodeSpan {
        unsigned interval;
        unsigned long long begin, start, limit, end;    // bits
        bool is_first, is_last;
};
__device__ __forceinline__ bool decode_span(const DecodeBuffers &b, const DecodeGeom &g, unsigned long long i, DecodeSpan *s)
{
        if(i >= *b.nsub) { return false; }
        unsigned lo = 0, hi = g.nint - 1;
        for(int step = 0; step < 32 && lo < hi; step++) {       // the last interval whose first subsequence is <= i
                const unsigned mid = lo + (hi - lo + 1) / 2;
                if(b.first[mid] <= i) {
                        lo = mid;
                } else {
                        hi = mid - 1;
                }
        }
        unsigned long long begin, end;
        decode_interval(b, g.nint, lo, &begin, &end);
        const unsigned long long local = i - b.first[lo];
        s->interval = lo;
        s->begin = begin * 8;
        s->end = end * 8;
        s->start = s->begin + local * g.S;
        if(s->start > s->end) { s->start = s->end; }
        s->limit = s->start + g.S < s->end ? s->start + g.S : s->end;
        s->is_first = local == 0;
        s->is_last = s->limit == s->end;
        return true;
}

// where the final pass puts what it decodes
struct DecodeOut {
        int16_t *coef[3];               // the zeroed grids
        unsigned *diff;                 // [nblocks] DC difference + 32768, by component (comp_base) and scan order
};

__constant__ const unsigned char kDecodeNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the block of scan ordinal `ord`: its component, its place among the component's DC differences, and the address of its 64
// values — NULL for a block that pads the grid out to whole MCUs
__device__ __forceinline__ int16_t *decode_block(const DecodeGeom &g, const DecodeOut &o, unsigned ord, unsigned *diff_at)
{
        const unsigned mcu = ord / g.per_mcu, blk = ord - mcu * g.per_mcu, c = g.blk_comp[blk], j = blk - g.first_blk[c];
        const unsigned my = mcu / g.mcus_w, mx = mcu - my * g.mcus_w, jy = j / g.hs[c], jx = j - jy * g.hs[c];
        const unsigned bx = mx * g.hs[c] + jx, by = my * g.vs[c] + jy;
        *diff_at = g.comp_base[c] + mcu * (g.hs[c] * g.vs[c]) + j;
        return bx < g.bw[c] && by < g.bh[c] ? o.coef[c] + ((size_t)by * g.bw[c] + bx) * 64 : nullptr;
}

// Decodes the symbols that begin in [st.pos, span.limit) from state st; returns the blocks completed.  A total function of
// (state, stream): a prefix that is no code counts as 16 bits of the symbol 00, and a run past coefficient 63 ends the block.
// kFinal (st is the TRUE state, ord the ordinal of the block it is in, end_ord the interval's end): stores what it decodes,
// stops behind the interval's last block and reports what is wrong with the stream.  Whoever completes that last block
// checks where the data ends: inside the interval, with less than a byte of padding left (the padding may reach into the
// next subsequence, whose entry state — decoded from padding by the rounds — then means nothing: a subsequence that begins
// at or behind the last block does nothing at all).  The interval's last subsequence checks that no block is missing.
template <bool kFinal>
__device__ __forceinline__ unsigned decode_symbols(const DecodeTables &t, const DecodeBuffers &b, const DecodeSpan &span, DecodeState &st, unsigned ord,
                                                   unsigned end_ord, const DecodeOut &o, unsigned *errors)
{
        const DecodeGeom &g = t.g;
        unsigned completed = 0, bad = 0, diff_at = 0;
        int16_t *block = nullptr;
        if(kFinal && ord < end_ord) { block = decode_block(g, o, ord, &diff_at); }
        for(unsigned n = 0; n < g.S && st.pos < span.limit; n++) {
                if(kFinal && ord >= end_ord) { break; }
                const unsigned w = decode_peek(b.words, b.nwords, st.pos);
                const unsigned c = g.blk_comp[st.blk];
                const j2p_huff_decode &tab = t.tab[st.k == 0 ? g.dc_tab[c] : 4 + g.ac_tab[c]];
                const unsigned e = tab.look[w >> 24];
                unsigned len = e >> 8, sym = e & 0xffu;
                if(len == 0) {
                        const unsigned code = w >> 16;
                        for(unsigned l = 9; l <= 16; l++) {
                                const int v = (int)(code >> (16 - l));
                                if(v <= tab.maxcode[l]) {
                                        len = l;
                                        sym = tab.vals[(unsigned)(v + tab.valoff[l]) & 0xffu];
                                        break;
                                }
                        }
                        if(len == 0) {
                                len = 16;
                                sym = 0;
                                bad |= kDecodeBadCode;
                        }
                }
                const unsigned s = sym & 15u, r = sym >> 4;
                int v = 0;
                if(s) {
                        v = (int)((w << len) >> (32u - s));
                        if(v < (1 << (s - 1))) { v -= (1 << s) - 1; }
                }
                st.pos += len + s;
                if(st.k == 0) {
                        if(kFinal) { o.diff[diff_at] = (unsigned)(v + 32768); }
                        st.k = 1;
                } else if(s == 0) {
                        if(r == 15) {
                                st.k += 16;
                                if(st.k > 64) { bad |= kDecodeBadRun; }
                        } else {
                                st.k = 64;
                        }
                } else {
                        st.k += r;
                        if(st.k > 63) {
                                bad |= kDecodeBadRun;
                        } else if(kFinal && block) {
                                block[kDecodeNatural[st.k]] = (int16_t)v;
                        }
                        st.k++;
                }
                if(st.k >= 64) {
                        st.k = 0;
                        st.blk = st.blk + 1 < g.per_mcu ? st.blk + 1 : 0;
                        completed++;
                        if(kFinal) {
                                ord++;
                                if(ord < end_ord) {
                                        block = decode_block(g, o, ord, &diff_at);
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

// One round.  in / out: the exit states of the previous round and of this one; last[i]: the entry state subsequence i was last
// decoded from (all ones: never).  The entry of an interval's first subsequence is known and is never anything else.
__global__ __launch_bounds__(256) void k_decode_sync(DecodeBuffers b, unsigned nbound, const unsigned long long *in, unsigned long long *out,
                                                     unsigned long long *last, unsigned *done, unsigned *changed)
{
        __shared__ DecodeTables t;
        // (what a lane needs to know whether it has anything to do comes from device memory: a workgroup none of whose
        // subsequences' entry states changed — most of them in the late rounds — leaves before it copies the tables to LDS)
        const DecodeGeom &g = b.tables->g;
        const unsigned i = blockIdx.x * 256 + threadIdx.x;
        DecodeSpan span;
        DecodeState entry = {0, 0, 0};
        unsigned long long key = 0;
        bool again = false;
        const bool live = i < nbound && decode_span(b, g, i, &span);
        if(live) {
                entry = DecodeState{span.begin, 0, 0};
                if(!span.is_first) {
                        entry = decode_unpack(in[i - 1]);
                        if(entry.blk >= g.per_mcu) { entry.blk = 0; }
                        if(entry.k > 63) { entry.k = 0; }
                        if(entry.pos < span.start) { entry.pos = span.start; }
                }
                key = decode_pack(entry);
                again = key != last[i];
                if(!again) { out[i] = in[i]; }
        }
        if(!__syncthreads_or(again)) { return; }
        decode_tables_to_lds(b.tables, &t);
        if(again) {
                last[i] = key;
                unsigned unused = 0;
                done[i] = decode_symbols<false>(t, b, span, entry, 0, 0, DecodeOut{}, &unused);
                out[i] = decode_pack(entry);
        }
        const unsigned long long mask = __ballot(again);
        if(mask && ((int)threadIdx.x & 63) == __ffsll((long long)mask) - 1) { atomicAdd(changed, (unsigned)__popcll(mask)); }
}

// The final pass.  exit: the converged exit states; before[i]: blocks completed in front of subsequence i (the exclusive sum of
// done[]), from which the block ordinal at its start follows through the known ordinal at its interval's start.
__global__ __launch_bounds__(256) void k_decode_write(DecodeBuffers b, unsigned nbound, const unsigned long long *exit, const unsigned long long *before,
                                                      DecodeOut o)
{
        __shared__ DecodeTables t;
        decode_tables_to_lds(b.tables, &t);
        const unsigned i = blockIdx.x * 256 + threadIdx.x;
        DecodeSpan span;
        if(i >= nbound || !decode_span(b, t.g, i, &span)) { return; }
        const DecodeGeom &g = t.g;
        DecodeState entry = {span.begin, 0, 0};
        unsigned errors = 0;
        if(!span.is_first) { entry = decode_unpack(exit[i - 1]); }
        const unsigned long long ord0 = (unsigned long long)span.interval * g.ri * g.per_mcu;
        unsigned long long end = ord0 + (unsigned long long)g.ri * g.per_mcu, ord = ord0 + (before[i] - before[b.first[span.interval]]);
        if(end > g.nblocks) { end = g.nblocks; }
        if(ord >= end) { return; }                      // at or behind the interval's last block: padding
        if(entry.blk >= g.per_mcu || entry.k > 63 || entry.pos < span.start || (unsigned)(ord % g.per_mcu) != entry.blk) {
                atomicOr(b.error, kDecodeBadState);     // (no true state looks like that)
                return;
        }
        (void)decode_symbols<true>(t, b, span, entry, (unsigned)ord, (unsigned)end, o, &errors);
        if(errors) { atomicOr(b.error, errors); }
}

// sums[j]: the exclusive sum of diff[] (DC differences + 32768, by component and scan order).  A block's DC is the sum of its
// component's differences from the first block of its restart interval on.
__global__ __launch_bounds__(256) void k_decode_dc(const DecodeTables *tables, const unsigned *diff, const unsigned long long *sums, DecodeOut o, unsigned *error)
{
        __shared__ DecodeTables t;
        decode_tables_to_lds(tables, &t);
        const DecodeGeom &g = t.g;
        const unsigned j = blockIdx.x * 256 + threadIdx.x;
        if(j >= g.nblocks) { return; }
        unsigned c = 0;
        for(unsigned k = 1; k < g.ncomp; k++) {
                if(j >= g.comp_base[k]) { c = k; }
        }
        const unsigned per = g.hs[c] * g.vs[c], local = j - g.comp_base[c], mcu = local / per, within = local - mcu * per;
        const unsigned reset = g.comp_base[c] + (mcu / g.ri) * g.ri * per;
        const long long dc = (long long)(sums[j] + diff[j] - sums[reset]) - 32768ll * (long long)(j + 1 - reset);
        if(dc < -32768 || dc > 32767) {
                atomicOr(error, kDecodeBadDc);
                return;
        }
        const unsigned my = mcu / g.mcus_w, mx = mcu - my * g.mcus_w, jy = within / g.hs[c], jx = within - jy * g.hs[c];
        const unsigned bx = mx * g.hs[c] + jx, by = my * g.vs[c] + jy;
        if(bx < g.bw[c] && by < g.bh[c]) { o.coef[c][((size_t)by * g.bw[c] + bx) * 64] = (int16_t)dc; }
}

}  // namespace j2p
