// jpeg2png_amd — gfx950 device code of the JPEG codec's coder: quantised coefficients in device memory into the entropy-coded
// data of a JPEG file (k_entropy_lengths, k_scan_*, k_entropy_pack, k_stuff_*; k_entropy_histogram counts the symbols for
// tables made for the image; the k_*_restart siblings and k_restart_* at the end are for files with restart intervals).
// Included by j2p_codec.hip alone, in front of
// j2p_decode_kernels.hip.h, which reuses the k_scan_* kernels for the way back.  It shares nothing with the output stage's
// kernels (j2p_output_kernels.hip.h): k_quantise_blocks, which leaves the coefficients, lives there.  Compiled with the
// same flags as every device unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace j2p {

// ---------------------------------------------------------------------------
// JPEG output, the last step: the quantised coefficients k_quantise_blocks left in device memory as the entropy-coded
// data of ONE baseline scan (include/jpeg2png_amd.h: "The JPEG file"), so that only the file's bytes come down.  Kernels
// of their own at the end of the code object; k_quantise_blocks above is untouched.  The passes, each a launch (order
// between workgroups comes from launch boundaries only; nobody waits for anybody):
//   k_entropy_lengths   bits of every scan position (a block of a component, or a dummy block)      -> len[]
//   k_scan_*            exclusive sum of len[] into 64-bit bit offsets (three launches)              -> off[]
//   k_entropy_pack      every block's codes at its offset into the zeroed staging stream
//   k_stuff_count       FF bytes per 256-byte chunk of the stream, k_scan_* again                   -> ffoff[]
//   k_stuff_copy        the stream with a 00 behind every FF
// A scan position belongs to one wavefront: lane j holds the coefficient at zigzag position j (lane 0 the DC
// difference), one __ballot gives the mask of the non-zero ACs, and the zero run in front of a lane's coefficient is the
// distance to the next lower set bit — so the ZRL codes, the run / size symbol and the EOB (lane 63, when its own
// coefficient is 0) are each lane's own business, and a block's bits are the lanes' bits in lane order.  The 128 bytes
// of a block are one coalesced load.  The bytes do not depend on timing: a block's bits are ORed into an LDS buffer of
// the wavefront's, whose words go to the stream as plain stores where the block owns the whole word and as atomic ORs
// into zeroed memory where it shares the word with its neighbours (its first and last).
// ---------------------------------------------------------------------------
constexpr int kEntropyIters = 16;       // scan positions per wavefront of a launch, one after the other
constexpr int kEntropyWords = 56;       // 32-bit words a block's bits can touch: 20 (DC) + 63 * 26 (AC) bits, plus the 31 in front
constexpr int kScanTile = 1024;         // elements per workgroup of the k_scan_* kernels (256 threads x 4)
constexpr int kStuffChunk = 256;        // bytes of the stream per wavefront of the k_stuff_* kernels (64 lanes x 4)

struct HuffCodes {
        unsigned dc[2][12], ac[2][256];  // [table][symbol]: (code length << 16) | code; 0 for a symbol the table has not got
};
struct ScanGeom {
        const int16_t *coef[3];          // [component] block-major [bh][bw][64], natural order
        unsigned bw[3], bh[3];           // [component] its block grid
        unsigned ncomp;                  // 1: blocks in raster order; 3: MCUs in raster order
        unsigned sub_w, sub_h, mcus_w;   // blocks of component 0 per MCU; MCUs per row
        unsigned per_mcu;                // scan positions per MCU: sub_w * sub_h + 2 (three components)
        unsigned nslots;                 // scan positions in all
};
static_assert(sizeof(HuffCodes) + sizeof(ScanGeom) + 2 * 8 <= 4096, "kernel arguments: 4 KB");

__constant__ const unsigned char kZigzagNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the component and block of scan position `slot`; false: the position lies beyond the component's grid (a dummy block)
__device__ __forceinline__ bool scan_block(const ScanGeom &g, unsigned slot, unsigned &c, size_t &block)
{
        if(g.ncomp == 1) {
                c = 0;
                block = slot;
                return true;
        }
        const unsigned mcu = slot / g.per_mcu, k = slot - mcu * g.per_mcu, my = mcu / g.mcus_w, mx = mcu - my * g.mcus_w, hv = g.per_mcu - 2;
        unsigned bx = mx, by = my;
        c = 0;
        if(k < hv) {
                const unsigned ky = k / g.sub_w;
                by = my * g.sub_h + ky;
                bx = mx * g.sub_w + (k - ky * g.sub_w);
        } else {
                c = 1 + k - hv;
        }
        block = (size_t)by * g.bw[c] + bx;
        return bx < g.bw[c] && by < g.bh[c];
}

// the DC the difference of scan position `slot` (a real block) is taken against: that of the component's last real block
// before it in scan order (a dummy block repeats its predecessor's DC), 0 for the first
__device__ __forceinline__ int scan_dc_predictor(const ScanGeom &g, unsigned slot)
{
        if(g.ncomp == 1) { return slot ? g.coef[0][(size_t)(slot - 1) * 64] : 0; }
        unsigned mcu = slot / g.per_mcu, k = slot - mcu * g.per_mcu;
        const unsigned hv = g.per_mcu - 2;
        if(k >= hv) { return mcu ? g.coef[1 + k - hv][(size_t)(mcu - 1) * 64] : 0; }    // (a chroma grid IS the MCU grid)
        for(;;) {
                // (ends: the first block of component 0 in an MCU is never a dummy)
                if(k == 0) {
                        if(mcu == 0) { return 0; }
                        mcu--;
                        k = hv - 1;
                } else {
                        k--;
                }
                unsigned c;
                size_t block;
                if(scan_block(g, mcu * g.per_mcu + k, c, block)) { return g.coef[0][block * 64]; }
        }
}

// what lane `lane` holds of scan position `slot`: the coefficient at zigzag position `lane`, lane 0 the DC difference; a
// dummy block is all zero.  *table: 0 for component 0, 1 for the others.
__device__ __forceinline__ int scan_value(const ScanGeom &g, unsigned slot, int lane, unsigned *table)
{
        unsigned c;
        size_t block;
        const bool real = scan_block(g, slot, c, block);
        *table = c ? 1 : 0;
        if(!real) { return 0; }
        const int v = g.coef[c][block * 64 + kZigzagNatural[lane]];
        return lane == 0 ? v - scan_dc_predictor(g, slot) : v;
}

// a lane's bits of its block, first bit highest: at most 3 ZRL codes of 11 bits, a code of 16 and 10 magnitude bits
struct LaneCode {
        unsigned long long bits;
        unsigned n;
};
// dc, ac: the block's tables; v: scan_value; nz: the lanes 1..63 whose v is not 0
__device__ __forceinline__ LaneCode entropy_lane(const unsigned *dc, const unsigned *ac, int lane, int v, unsigned long long nz)
{
        const unsigned a = (unsigned)(v < 0 ? -v : v);
        const unsigned s = 32u - (unsigned)__clz((int)a);               // the category: bit length of |v|, 0 for 0
        const unsigned mag = (unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1u);
        LaneCode r = {0, 0};
        if(lane == 0) {
                const unsigned e = dc[s];
                r.bits = ((unsigned long long)(e & 0xffffu) << s) | mag;
                r.n = (e >> 16) + s;
        } else if(v != 0) {
                const unsigned long long before = (nz | 1ull) & ((1ull << lane) - 1ull);        // (bit 0: the DC's place)
                const unsigned run = (unsigned)lane - 1u - (63u - (unsigned)__clzll((long long)before));
                const unsigned e = ac[((run & 15u) << 4) | s], z = ac[0xf0];
                for(unsigned k = 0; k < (run >> 4); k++) {
                        r.bits = (r.bits << (z >> 16)) | (z & 0xffffu);
                        r.n += z >> 16;
                }
                r.bits = (((r.bits << (e >> 16)) | (e & 0xffffu)) << s) | mag;
                r.n += (e >> 16) + s;
        } else if(lane == 63) {
                r.bits = ac[0] & 0xffffu;                               // EOB: the block ends in a run of zeros
                r.n = ac[0] >> 16;
        }
        return r;
}

// the tables into LDS: [table][12 DC + 256 AC]
__device__ __forceinline__ void entropy_tables(const HuffCodes &h, unsigned (*tab)[268])
{
        for(unsigned i = threadIdx.x; i < 2 * 268; i += 256) {
                const unsigned t = i / 268, k = i - t * 268;
                tab[t][k] = k < 12 ? h.dc[t][k] : h.ac[t][k - 12];
        }
        __syncthreads();
}

__global__ __launch_bounds__(256) void k_entropy_lengths(ScanGeom g, HuffCodes h, unsigned *len)
{
        __shared__ unsigned tab[2][268];
        entropy_tables(h, tab);
        const int lane = (int)threadIdx.x & 63;
        const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const unsigned first = (blockIdx.x * 4 + wave) * kEntropyIters;
        for(unsigned it = 0; it < kEntropyIters && first + it < g.nslots; it++) {
                unsigned t;
                const int v = scan_value(g, first + it, lane, &t);
                unsigned n = entropy_lane(tab[t], tab[t] + 12, lane, v, __ballot(lane > 0 && v != 0)).n;
#pragma unroll
                for(int d = 32; d >= 1; d >>= 1) { n += __shfl_xor(n, d); }
                if(lane == 0) { len[first + it] = n; }
        }
}

// ---- the symbol counts the optimised Huffman tables are made from (include/jpeg2png_amd.h: "Optimised Huffman tables") ----
// k_entropy_lengths' walk without the tables: lane 0 counts its block's DC category, a non-zero lane its (run & 15, size)
// symbol and its run >> 4 ZRLs, lane 63 the EOB of a block that ends in zeros.  Counts go to an LDS histogram of the
// workgroup, [table][12 DC + 256 AC] like the tables' (a workgroup sees at most 64 positions of 64 symbols: 32 bits hold
// them), one ds_add per lane, and behind the barrier every non-zero entry is added to hist[2][268], 64-bit counters in
// device memory that the host zeroed.  Integers: the result does not depend on who comes first.
// At high quality most lanes of a block hold a (0, s) symbol — a handful of addresses for 63 lanes, which an LDS atomic
// takes one after the other.  It does not show: the walk costs what it costs k_entropy_lengths, and the forms that merge
// equal lanes first (a ballot per bit of the entry number, the lowest lane adds the popcount) or sum the ZRLs over the
// wavefront before counting them were measured slower (profiles/patches/histogram_merged_lanes.patch).
constexpr unsigned kHistogramEntries = 2 * 268;

__global__ __launch_bounds__(256) void k_entropy_histogram(ScanGeom g, unsigned long long *hist)
{
        __shared__ unsigned count[kHistogramEntries];
        for(unsigned i = threadIdx.x; i < kHistogramEntries; i += 256) { count[i] = 0; }
        __syncthreads();
        const int lane = (int)threadIdx.x & 63;
        const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const unsigned first = (blockIdx.x * 4 + wave) * kEntropyIters;
        for(unsigned it = 0; it < kEntropyIters && first + it < g.nslots; it++) {
                unsigned t;
                const int v = scan_value(g, first + it, lane, &t);
                const unsigned long long nz = __ballot(lane > 0 && v != 0);
                const unsigned a = (unsigned)(v < 0 ? -v : v);
                const unsigned s = 32u - (unsigned)__clz((int)a);
                unsigned *mine = count + t * 268u;      // (every index below stays under 268 whatever the coefficients hold)
                if(lane == 0) {
                        atomicAdd(&mine[s < 12u ? s : 11u], 1u);
                } else if(v != 0) {
                        const unsigned long long before = (nz | 1ull) & ((1ull << lane) - 1ull);
                        const unsigned run = (unsigned)lane - 1u - (63u - (unsigned)__clzll((long long)before));
                        atomicAdd(&mine[12u + ((((run & 15u) << 4) | s) & 255u)], 1u);
                        if(run >> 4) { atomicAdd(&mine[12u + 0xf0u], run >> 4); }
                } else if(lane == 63) {
                        atomicAdd(&mine[12u], 1u);
                }
        }
        __syncthreads();
        for(unsigned i = threadIdx.x; i < kHistogramEntries; i += 256) {
                if(const unsigned n = count[i]) { atomicAdd(&hist[i], (unsigned long long)n); }
        }
}

// off[]: the bit offset of every scan position (k_scan_apply); stage: the stream, zeroed, ceil(bits / 32) + 1 words.  The
// last position's wavefront also sets the 1-bits that pad the last byte.
__global__ __launch_bounds__(256) void k_entropy_pack(ScanGeom g, HuffCodes h, const unsigned long long *off, unsigned *stage)
{
        __shared__ unsigned tab[2][268];
        __shared__ unsigned words[4][kEntropyWords];
        if(threadIdx.x < 4 * kEntropyWords) { (&words[0][0])[threadIdx.x] = 0; }
        entropy_tables(h, tab);
        const int lane = (int)threadIdx.x & 63;
        const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const unsigned first = (blockIdx.x * 4 + wave) * kEntropyIters;
        for(unsigned it = 0; it < kEntropyIters; it++) {                // (the same trips for every wavefront: barriers inside)
                const unsigned slot = first + it;
                const bool live = slot < g.nslots;
                unsigned long long base = 0;
                unsigned total = 0;
                if(live) {
                        unsigned t;
                        const int v = scan_value(g, slot, lane, &t);
                        const LaneCode code = entropy_lane(tab[t], tab[t] + 12, lane, v, __ballot(lane > 0 && v != 0));
                        unsigned incl = code.n;
#pragma unroll
                        for(int d = 1; d < 64; d <<= 1) {
                                const unsigned up = __shfl_up(incl, d);
                                if(lane >= d) { incl += up; }
                        }
                        total = __shfl(incl, 63);
                        base = off[slot];
                        if(code.n) {
                                // the lane's bits at bit p of the wavefront's buffer (bit 0: the highest bit of word 0): three words
                                const unsigned p = (unsigned)(base & 31u) + incl - code.n, w = p >> 5, b = p & 31u;
                                const unsigned long long val = code.bits << (64u - code.n);
                                const unsigned part[3] = {(unsigned)(val >> (32u + b)), (unsigned)(val >> b), (unsigned)(val << (32u - b))};
#pragma unroll
                                for(unsigned k = 0; k < 3; k++) {
                                        if(part[k] && w + k < kEntropyWords) { atomicOr(&words[wave][w + k], part[k]); }
                                }
                        }
                }
                __syncthreads();
                if(live) {
                        const unsigned nwords = ((unsigned)(base & 31u) + total + 31u) >> 5;    // (at most 53)
                        if((unsigned)lane < nwords) {
                                const unsigned x = __builtin_bswap32(words[wave][lane]);         // the stream is bytes: big-endian words
                                words[wave][lane] = 0;
                                unsigned *dst = stage + (size_t)(base >> 5) + lane;
                                if(lane == 0 || (unsigned)lane == nwords - 1) {
                                        if(x) { atomicOr(dst, x); }                              // shared with the neighbours
                                } else {
                                        *dst = x;
                                }
                        }
                        if(slot == g.nslots - 1 && lane == 0) {
                                const unsigned long long end = base + total;
                                const unsigned pad = (8u - (unsigned)(end & 7u)) & 7u;
                                if(pad) { atomicOr(stage + (size_t)(end >> 5), __builtin_bswap32(((1u << pad) - 1u) << (32u - (unsigned)(end & 31u) - pad))); }
                        }
                }
                __syncthreads();
        }
}

// ---- exclusive sums of n 32-bit counts into 64-bit offsets: k_scan_sums (a total per tile of kScanTile), k_scan_tiles
// (ONE workgroup: the totals into offsets, sums[ntiles] the grand total), k_scan_apply (every element's offset) ----
// the sum of the 256 threads' values before this thread's; *all: of all of them.  lds: 4 words, free again on return.
__device__ __forceinline__ unsigned long long scan_workgroup(unsigned long long mine, unsigned long long *lds, unsigned long long *all)
{
        const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
        unsigned long long incl = mine;
#pragma unroll
        for(int d = 1; d < 64; d <<= 1) {
                const unsigned long long up = __shfl_up(incl, d);
                if(lane >= d) { incl += up; }
        }
        if(lane == 63) { lds[wave] = incl; }
        __syncthreads();
        unsigned long long before = 0, sum = 0;
        for(int w = 0; w < 4; w++) {
                if(w < wave) { before += lds[w]; }
                sum += lds[w];
        }
        __syncthreads();
        *all = sum;
        return before + incl - mine;
}

__global__ __launch_bounds__(256) void k_scan_sums(const unsigned *in, unsigned n, unsigned long long *sums)
{
        __shared__ unsigned long long lds[4];
        const unsigned i0 = blockIdx.x * kScanTile + threadIdx.x * 4;
        unsigned long long mine = 0, all;
        for(unsigned k = 0; k < 4; k++) { mine += i0 + k < n ? in[i0 + k] : 0u; }
        (void)scan_workgroup(mine, lds, &all);
        if(threadIdx.x == 0) { sums[blockIdx.x] = all; }
}

__global__ __launch_bounds__(256) void k_scan_tiles(unsigned long long *sums, unsigned ntiles)
{
        __shared__ unsigned long long lds[4];
        unsigned long long carry = 0;
        for(unsigned i0 = 0; i0 < ntiles; i0 += 256) {
                const unsigned i = i0 + threadIdx.x;
                const unsigned long long mine = i < ntiles ? sums[i] : 0ull;
                unsigned long long all;
                const unsigned long long before = scan_workgroup(mine, lds, &all);
                if(i < ntiles) { sums[i] = carry + before; }
                carry += all;
        }
        if(threadIdx.x == 0) { sums[ntiles] = carry; }
}

__global__ __launch_bounds__(256) void k_scan_apply(const unsigned *in, unsigned n, const unsigned long long *sums, unsigned long long *out)
{
        __shared__ unsigned long long lds[4];
        const unsigned i0 = blockIdx.x * kScanTile + threadIdx.x * 4;
        unsigned v[4];
        unsigned long long mine = 0, all;
        for(unsigned k = 0; k < 4; k++) {
                v[k] = i0 + k < n ? in[i0 + k] : 0u;
                mine += v[k];
        }
        unsigned long long at = sums[blockIdx.x] + scan_workgroup(mine, lds, &all);
        for(unsigned k = 0; k < 4; k++) {
                if(i0 + k < n) { out[i0 + k] = at; }
                at += v[k];
        }
}

// ---- byte stuffing: a wavefront per kStuffChunk bytes of the stream, a lane per 4 of them ----
// the lane's word of chunk `chunk` (bytes beyond nbytes are zero) and how many of its bytes are FF
__device__ __forceinline__ unsigned stuff_word(const unsigned *stage, size_t nbytes, size_t chunk, int lane, unsigned *ff)
{
        const size_t i = chunk * (kStuffChunk / 4) + (size_t)lane;
        const unsigned x = i * 4 < nbytes ? stage[i] : 0u;
        *ff = ((x & 0xffu) == 0xffu) + ((x & 0xff00u) == 0xff00u) + ((x & 0xff0000u) == 0xff0000u) + ((x & 0xff000000u) == 0xff000000u);
        return x;
}

__global__ __launch_bounds__(256) void k_stuff_count(const unsigned *stage, size_t nbytes, unsigned nchunks, unsigned *count)
{
        const int lane = (int)threadIdx.x & 63;
        const unsigned chunk = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        if(chunk >= nchunks) { return; }
        unsigned ff;
        (void)stuff_word(stage, nbytes, chunk, lane, &ff);
#pragma unroll
        for(int d = 32; d >= 1; d >>= 1) { ff += __shfl_xor(ff, d); }
        if(lane == 0) { count[chunk] = ff; }
}

// ffoff[chunk]: FF bytes in front of the chunk (k_scan_apply of the counts); out: nbytes + their total bytes
__global__ __launch_bounds__(256) void k_stuff_copy(const unsigned *stage, size_t nbytes, unsigned nchunks, const unsigned long long *ffoff,
                                                    uint8_t *out)
{
        const int lane = (int)threadIdx.x & 63;
        const unsigned chunk = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        if(chunk >= nchunks) { return; }
        unsigned ff;
        const unsigned x = stuff_word(stage, nbytes, chunk, lane, &ff);
        unsigned incl = ff;
#pragma unroll
        for(int d = 1; d < 64; d <<= 1) {
                const unsigned up = __shfl_up(incl, d);
                if(lane >= d) { incl += up; }
        }
        const size_t at = (size_t)chunk * kStuffChunk + (size_t)lane * 4;
        uint8_t *dst = out + at + ffoff[chunk] + (incl - ff);
        for(unsigned k = 0; k < 4 && at + k < nbytes; k++) {
                const uint8_t byte = (uint8_t)(x >> (8 * k));
                *dst++ = byte;
                if(byte == 0xff) { *dst++ = 0; }
        }
}

// ---- restart intervals (include/jpeg2png_amd.h: "Restart intervals"): a scan's items — its positions, or an AC scan's blocks —
// in intervals of ri items, nint of them, the last possibly shorter ----
// Every interval is completed to a byte with 1-bits, so every interval STARTS on a byte and its pad is (-its bits) mod 8, which the
// unpadded offsets give without anybody waiting for anybody:
//   k_restart_pad       a lane per interval adds the pad to the length of the interval's last item; the exclusive sum is queued again
//   k_restart_ends      a lane per interval but the last: the byte of the padded stream behind which its RSTn marker stands   -> ends[]
// The staging stream stays pure data.  The markers go in where the FFs are stuffed: ends[] is sorted (an interval has at least one
// bit, so at least a byte), k_stuff_count_restart adds 2 per end inside its chunk, k_stuff_copy_restart shifts every byte by the
// FFs and twice the ends in front of it, and the lane that holds the byte in front of an end writes FF, D0 + (ordinal & 7) behind it.

// scan_dc_predictor in a scan with restart intervals of `ri` positions (whole MCUs; include/jpeg2png_amd.h: "Restart intervals"):
// 0 for the first real block of a component in its interval — the walk never goes behind the interval's first MCU — and within
// the interval as above, a dummy block repeating its predecessor
__device__ __forceinline__ int scan_dc_predictor_restart(const ScanGeom &g, unsigned slot, unsigned ri)
{
        const unsigned begin = slot / ri * ri;
        if(g.ncomp == 1) { return slot > begin ? g.coef[0][(size_t)(slot - 1) * 64] : 0; }
        unsigned mcu = slot / g.per_mcu, k = slot - mcu * g.per_mcu;
        const unsigned hv = g.per_mcu - 2, mcu0 = begin / g.per_mcu;
        if(k >= hv) { return mcu > mcu0 ? g.coef[1 + k - hv][(size_t)(mcu - 1) * 64] : 0; }
        for(;;) {
                if(k == 0) {
                        if(mcu == mcu0) { return 0; }
                        mcu--;
                        k = hv - 1;
                } else {
                        k--;
                }
                unsigned c;
                size_t block;
                if(scan_block(g, mcu * g.per_mcu + k, c, block)) { return g.coef[0][block * 64]; }
        }
}

// scan_value with that predictor
__device__ __forceinline__ int scan_value_restart(const ScanGeom &g, unsigned slot, int lane, unsigned *table, unsigned ri)
{
        unsigned c;
        size_t block;
        const bool real = scan_block(g, slot, c, block);
        *table = c ? 1 : 0;
        if(!real) { return 0; }
        const int v = g.coef[c][block * 64 + kZigzagNatural[lane]];
        return lane == 0 ? v - scan_dc_predictor_restart(g, slot, ri) : v;
}

// The three walking kernels for a scan with restart intervals of ri positions: k_entropy_lengths, k_entropy_histogram and
// k_entropy_pack line for line, but that the DC differences are taken against scan_dc_predictor_restart and that the wavefront of
// EVERY interval's last position sets the 1-bits that complete its byte — every interval starts on a byte (k_restart_pad), so the
// pad is known from the position's own end.  Copies and no template: the kernels above stay, text and machine code, what they were.
__global__ __launch_bounds__(256) void k_entropy_lengths_restart(ScanGeom g, HuffCodes h, unsigned ri, unsigned *len)
{
        __shared__ unsigned tab[2][268];
        entropy_tables(h, tab);
        const int lane = (int)threadIdx.x & 63;
        const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const unsigned first = (blockIdx.x * 4 + wave) * kEntropyIters;
        for(unsigned it = 0; it < kEntropyIters && first + it < g.nslots; it++) {
                unsigned t;
                const int v = scan_value_restart(g, first + it, lane, &t, ri);
                unsigned n = entropy_lane(tab[t], tab[t] + 12, lane, v, __ballot(lane > 0 && v != 0)).n;
#pragma unroll
                for(int d = 32; d >= 1; d >>= 1) { n += __shfl_xor(n, d); }
                if(lane == 0) { len[first + it] = n; }
        }
}


__global__ __launch_bounds__(256) void k_entropy_histogram_restart(ScanGeom g, unsigned ri, unsigned long long *hist)
{
        __shared__ unsigned count[kHistogramEntries];
        for(unsigned i = threadIdx.x; i < kHistogramEntries; i += 256) { count[i] = 0; }
        __syncthreads();
        const int lane = (int)threadIdx.x & 63;
        const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const unsigned first = (blockIdx.x * 4 + wave) * kEntropyIters;
        for(unsigned it = 0; it < kEntropyIters && first + it < g.nslots; it++) {
                unsigned t;
                const int v = scan_value_restart(g, first + it, lane, &t, ri);
                const unsigned long long nz = __ballot(lane > 0 && v != 0);
                const unsigned a = (unsigned)(v < 0 ? -v : v);
                const unsigned s = 32u - (unsigned)__clz((int)a);
                unsigned *mine = count + t * 268u;      // (every index below stays under 268 whatever the coefficients hold)
                if(lane == 0) {
                        atomicAdd(&mine[s < 12u ? s : 11u], 1u);
                } else if(v != 0) {
                        const unsigned long long before = (nz | 1ull) & ((1ull << lane) - 1ull);
                        const unsigned run = (unsigned)lane - 1u - (63u - (unsigned)__clzll((long long)before));
                        atomicAdd(&mine[12u + ((((run & 15u) << 4) | s) & 255u)], 1u);
                        if(run >> 4) { atomicAdd(&mine[12u + 0xf0u], run >> 4); }
                } else if(lane == 63) {
                        atomicAdd(&mine[12u], 1u);
                }
        }
        __syncthreads();
        for(unsigned i = threadIdx.x; i < kHistogramEntries; i += 256) {
                if(const unsigned n = count[i]) { atomicAdd(&hist[i], (unsigned long long)n); }
        }
}


__global__ __launch_bounds__(256) void k_entropy_pack_restart(ScanGeom g, HuffCodes h, unsigned ri, const unsigned long long *off, unsigned *stage)
{
        __shared__ unsigned tab[2][268];
        __shared__ unsigned words[4][kEntropyWords];
        if(threadIdx.x < 4 * kEntropyWords) { (&words[0][0])[threadIdx.x] = 0; }
        entropy_tables(h, tab);
        const int lane = (int)threadIdx.x & 63;
        const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const unsigned first = (blockIdx.x * 4 + wave) * kEntropyIters;
        for(unsigned it = 0; it < kEntropyIters; it++) {                // (the same trips for every wavefront: barriers inside)
                const unsigned slot = first + it;
                const bool live = slot < g.nslots;
                unsigned long long base = 0;
                unsigned total = 0;
                if(live) {
                        unsigned t;
                        const int v = scan_value_restart(g, slot, lane, &t, ri);
                        const LaneCode code = entropy_lane(tab[t], tab[t] + 12, lane, v, __ballot(lane > 0 && v != 0));
                        unsigned incl = code.n;
#pragma unroll
                        for(int d = 1; d < 64; d <<= 1) {
                                const unsigned up = __shfl_up(incl, d);
                                if(lane >= d) { incl += up; }
                        }
                        total = __shfl(incl, 63);
                        base = off[slot];
                        if(code.n) {
                                // the lane's bits at bit p of the wavefront's buffer (bit 0: the highest bit of word 0): three words
                                const unsigned p = (unsigned)(base & 31u) + incl - code.n, w = p >> 5, b = p & 31u;
                                const unsigned long long val = code.bits << (64u - code.n);
                                const unsigned part[3] = {(unsigned)(val >> (32u + b)), (unsigned)(val >> b), (unsigned)(val << (32u - b))};
#pragma unroll
                                for(unsigned k = 0; k < 3; k++) {
                                        if(part[k] && w + k < kEntropyWords) { atomicOr(&words[wave][w + k], part[k]); }
                                }
                        }
                }
                __syncthreads();
                if(live) {
                        const unsigned nwords = ((unsigned)(base & 31u) + total + 31u) >> 5;    // (at most 53)
                        if((unsigned)lane < nwords) {
                                const unsigned x = __builtin_bswap32(words[wave][lane]);         // the stream is bytes: big-endian words
                                words[wave][lane] = 0;
                                unsigned *dst = stage + (size_t)(base >> 5) + lane;
                                if(lane == 0 || (unsigned)lane == nwords - 1) {
                                        if(x) { atomicOr(dst, x); }                              // shared with the neighbours
                                } else {
                                        *dst = x;
                                }
                        }
                        if((slot == g.nslots - 1 || (slot + 1) % ri == 0) && lane == 0) {
                                const unsigned long long end = base + total;
                                const unsigned pad = (8u - (unsigned)(end & 7u)) & 7u;
                                if(pad) { atomicOr(stage + (size_t)(end >> 5), __builtin_bswap32(((1u << pad) - 1u) << (32u - (unsigned)(end & 31u) - pad))); }
                        }
                }
                __syncthreads();
        }
}

// len, off: the scan's items and their unpadded offsets; *total: the offset behind the last.  *padding += the pads.
__global__ __launch_bounds__(256) void k_restart_pad(unsigned *len, const unsigned long long *off, const unsigned long long *total, unsigned n,
                                                     unsigned ri, unsigned nint, unsigned long long *padding)
{
        const unsigned i = blockIdx.x * 256 + threadIdx.x;
        if(i >= nint) { return; }
        const unsigned long long begin = (unsigned long long)i * ri, end = begin + ri < n ? begin + ri : n;
        const unsigned long long bits = (end < n ? off[end] : *total) - off[begin];
        const unsigned pad = (unsigned)(0ull - bits) & 7u;
        if(pad) {
                len[end - 1] += pad;
                atomicAdd(padding, (unsigned long long)pad);
        }
}

// off: the items' padded offsets, off[0] at the scan's first byte; ends[i]: bytes of the scan's stream in front of marker i
__global__ __launch_bounds__(256) void k_restart_ends(const unsigned long long *off, unsigned ri, unsigned nends, unsigned long long *ends)
{
        const unsigned i = blockIdx.x * 256 + threadIdx.x;
        if(i < nends) { ends[i] = (off[((size_t)i + 1) * ri] - off[0]) >> 3; }
}

// the ends at or below byte `at`: the ordinal of the first marker that stands behind byte `at` or later
__device__ __forceinline__ unsigned restart_ends_before(const unsigned long long *ends, unsigned nends, unsigned long long at)
{
        unsigned lo = 0, hi = nends;
        while(lo < hi) {
                const unsigned mid = lo + (hi - lo) / 2;
                if(ends[mid] <= at) {
                        lo = mid + 1;
                } else {
                        hi = mid;
                }
        }
        return lo;
}

// k_stuff_count with 2 more for every marker behind a byte of the chunk
__global__ __launch_bounds__(256) void k_stuff_count_restart(const unsigned *stage, size_t nbytes, unsigned nchunks, const unsigned long long *ends,
                                                             unsigned nends, unsigned *count)
{
        const int lane = (int)threadIdx.x & 63;
        const unsigned chunk = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        if(chunk >= nchunks) { return; }
        unsigned ff;
        (void)stuff_word(stage, nbytes, chunk, lane, &ff);
#pragma unroll
        for(int d = 32; d >= 1; d >>= 1) { ff += __shfl_xor(ff, d); }
        if(lane == 0) {
                const unsigned long long at = (unsigned long long)chunk * kStuffChunk;
                count[chunk] = ff + 2u * (restart_ends_before(ends, nends, at + kStuffChunk) - restart_ends_before(ends, nends, at));
        }
}

// k_stuff_copy with the markers: ffoff[chunk] counts the FFs and twice the markers in front of the chunk
__global__ __launch_bounds__(256) void k_stuff_copy_restart(const unsigned *stage, size_t nbytes, unsigned nchunks, const unsigned long long *ffoff,
                                                            const unsigned long long *ends, unsigned nends, uint8_t *out)
{
        const int lane = (int)threadIdx.x & 63;
        const unsigned chunk = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        if(chunk >= nchunks) { return; }
        unsigned ff;
        const unsigned x = stuff_word(stage, nbytes, chunk, lane, &ff);
        const size_t at = (size_t)chunk * kStuffChunk + (size_t)lane * 4;
        unsigned marker = restart_ends_before(ends, nends, at);
        const unsigned extra = ff + 2u * (restart_ends_before(ends, nends, at + 4) - marker);
        unsigned incl = extra;
#pragma unroll
        for(int d = 1; d < 64; d <<= 1) {
                const unsigned up = __shfl_up(incl, d);
                if(lane >= d) { incl += up; }
        }
        uint8_t *dst = out + at + ffoff[chunk] + (incl - extra);
        for(unsigned k = 0; k < 4 && at + k < nbytes; k++) {
                const uint8_t byte = (uint8_t)(x >> (8 * k));
                *dst++ = byte;
                if(byte == 0xff) { *dst++ = 0; }
                if(marker < nends && ends[marker] == at + k + 1) {
                        *dst++ = 0xff;
                        *dst++ = (uint8_t)(0xd0u + (marker & 7u));
                        marker++;
                }
        }
}

}  // namespace j2p
