// jpeg2png_amd — gfx950 device code of the PNG coder: 8- or 16-bit samples in device memory into the IDAT chunks of a PNG file
// (include/jpeg2png_amd.h: "The PNG file"), so that only the file's bytes come down.  Included by j2p_codec.hip alone, behind the JPEG
// coder's and decoder's kernels, whose scan_workgroup it reuses: kernels of their own at the end of the code object; nothing above is
// touched.  The passes, each a launch (order between workgroups comes from launch boundaries only; nobody waits for anybody):
//   k_png_filter   a wavefront per row: the five filters' costs, then the winner's bytes behind its type byte        -> stream[]
//   k_png_count    a workgroup per deflate block: its tokens' symbols counted in LDS, its two Adler-32 sums          -> counts[]
//   (host)         j2p_deflate.h: every block's code, header and size from its counts                                -> blocks[]
//   k_png_pack     a workgroup per deflate block: header, tokens and EOB ORed into the zeroed zlib stream            -> stage[]
//   k_png_chunks   the zlib stream laid out as the data of IDAT chunks
//   k_png_crc      a lane per chunk: its length, its type and its CRC-32
// The bytes do not depend on timing: counts are integers added in LDS and stored by the block's one owner, and the stream's words
// are plain stores where a tile owns the whole word and atomic ORs into zeroed memory where it shares the word (a tile's first and
// last, the header's bytes, what follows the last token).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "j2p_deflate.h"

namespace j2p {

constexpr int kPngTile = 1024;          // positions of a block per trip of its workgroup: 256 threads x 4
constexpr int kPngAhead = 257;          // bytes behind a position that decide its token: a match is at most 258 long
constexpr int kPngTileBytes = 1 + kPngTile + kPngAhead;         // the byte in front of the tile, the tile, what lies ahead
// words a tile's bits can touch: at most 15 bits a position, and 6 more (5 extra bits and the distance's) for a match at the tile's
// last position, whose silent followers are the next tile's
constexpr int kPngWords = (31 + kPngTile * 15 + 6 + 31) / 32 + 2;
constexpr unsigned kPngNone = 0xffffffffu;

// what the host makes of a block's counts (j2p_deflate.h), as k_png_pack reads it
struct PngBlock {
        unsigned long long offset;      // of the block's first byte in the zlib stream
        unsigned header_bits, final;
        unsigned code[J2P_DEFLATE_SYMBOLS];     // (length << 16) | the code, first bit lowest
        uint8_t header[J2P_DEFLATE_HEADER_MAX];
};
static_assert(sizeof(PngBlock) % 8 == 0, "an array of them keeps offset aligned");

// ---- filtering ----
__device__ __forceinline__ unsigned png_paeth(int a, int b, int c)
{
        const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
        return (unsigned)(pa <= pb && pa <= pc ? a : (pb <= pc ? b : c));
}
// byte x of row y under filter f; in: the samples, rb bytes a row
__device__ __forceinline__ void png_neighbours(const uint8_t *in, size_t rb, unsigned y, size_t x, unsigned bpp, unsigned &v, unsigned &a, unsigned &b,
                                               unsigned &c)
{
        const uint8_t *row = in + (size_t)y * rb;
        v = row[x];
        a = x >= bpp ? row[x - bpp] : 0u;
        b = y ? (row - rb)[x] : 0u;
        c = y && x >= bpp ? (row - rb)[x - bpp] : 0u;
}
__device__ __forceinline__ unsigned png_filtered(unsigned f, unsigned v, unsigned a, unsigned b, unsigned c)
{
        const unsigned pred = f == 0 ? 0u : (f == 1 ? a : (f == 2 ? b : (f == 3 ? (a + b) >> 1 : png_paeth((int)a, (int)b, (int)c))));
        return (v - pred) & 255u;
}
__device__ __forceinline__ unsigned png_cost(unsigned byte) { return byte < 128u ? byte : 256u - byte; }

// fixed: 0..4, or 5 for the adaptive choice.  stream: height rows of 1 + rb bytes.  chosen[5]: rows per filter type, zeroed.
__global__ __launch_bounds__(256) void k_png_filter(const uint8_t *in, size_t rb, unsigned height, unsigned bpp, unsigned fixed, uint8_t *stream,
                                                    unsigned *chosen)
{
        const unsigned lane = threadIdx.x & 63u;
        const unsigned y = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        if(y >= height) { return; }                                            // (no barrier in this kernel)
        unsigned f = fixed;
        if(fixed > 4) {
                unsigned cost[5] = {0, 0, 0, 0, 0};
                for(size_t x = lane; x < rb; x += 64) {
                        unsigned v, a, b, c;
                        png_neighbours(in, rb, y, x, bpp, v, a, b, c);
#pragma unroll
                        for(unsigned k = 0; k < 5; k++) { cost[k] += png_cost(png_filtered(k, v, a, b, c)); }
                }
                // (a row of 2^24 bytes of cost 128 each is 2^31)
#pragma unroll
                for(unsigned k = 0; k < 5; k++) {
#pragma unroll
                        for(int d = 32; d >= 1; d >>= 1) { cost[k] += __shfl_xor(cost[k], d); }
                }
                f = 0;
#pragma unroll
                for(unsigned k = 1; k < 5; k++) {
                        if(cost[k] < cost[f]) { f = k; }                        // (strictly: the lowest number wins a tie)
                }
        }
        uint8_t *out = stream + (size_t)y * (rb + 1);
        if(lane == 0) {
                out[0] = (uint8_t)f;
                atomicAdd(&chosen[f], 1u);
        }
        for(size_t x = lane; x < rb; x += 64) {
                unsigned v, a, b, c;
                png_neighbours(in, rb, y, x, bpp, v, a, b, c);
                out[1 + x] = (uint8_t)png_filtered(f, v, a, b, c);
        }
}

// ---- tokens ----
// the length symbol of a match of n = 3..258 bytes, its extra bits and their value (RFC 1951 3.2.5)
__host__ __device__ constexpr unsigned png_length_symbol(unsigned n, unsigned *extra_bits, unsigned *extra)
{
        const unsigned l = n - 3;
        if(n == 258 || l < 8) {
                *extra_bits = 0;
                *extra = 0;
                return n == 258 ? 285u : 257u + l;
        }
        const unsigned e = 29u - (unsigned)__builtin_clz(l);                    // floor(log2(l)) - 2
        *extra_bits = e;
        *extra = l & ((1u << e) - 1u);
        return 257u + 4u * e + 4u + ((l >> e) & 3u);
}
constexpr bool png_length_symbols_agree()
{
        for(unsigned n = 3; n <= 258; n++) {
                unsigned bits = 0, extra = 0, k = 28;
                while(j2p_deflate_length_base[k] > n) { k--; }
                if(png_length_symbol(n, &bits, &extra) != 257 + k || bits != j2p_deflate_length_extra[k] || extra != n - j2p_deflate_length_base[k]) { return false; }
        }
        return true;
}
static_assert(png_length_symbols_agree(), "the kernels' length symbols are the host's table");

// the largest of the 256 threads' values before this thread's (-1: none); *all: of all of them.  lds: 4 words, free again on return.
__device__ __forceinline__ int png_scan_max(int mine, int *lds, int *all)
{
        const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
        int incl = mine;
#pragma unroll
        for(int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d);
                if(lane >= d) { incl = max(incl, up); }
        }
        int before = __shfl_up(incl, 1);
        if(lane == 0) { before = -1; }
        if(lane == 63) { lds[wave] = incl; }
        __syncthreads();
        int top = -1;
        for(int w = 0; w < 4; w++) {
                if(w < wave) { before = max(before, lds[w]); }
                top = max(top, lds[w]);
        }
        __syncthreads();
        *all = top;
        return before;
}

// The tile of a block that begins at position t0 (a multiple of kPngTile) into LDS: bytes[1 + i] = the block's byte t0 + i, as far
// as the block (n bytes from src) goes and at most kPngAhead beyond the tile; bytes[0] the byte in front of the tile.
__device__ __forceinline__ void png_tile_load(const uint8_t *src, unsigned n, unsigned t0, uint8_t *bytes)
{
        const unsigned have = min((unsigned)kPngTileBytes, 1u + n - t0);
        for(unsigned i = threadIdx.x; i < have; i += 256) { bytes[i] = t0 + i ? src[t0 + i - 1] : (uint8_t)0; }
        __syncthreads();
}

// The tokens of this thread's four positions t0 + 4 * threadIdx.x + k of a block of n bytes (include/jpeg2png_amd.h, "The PNG
// file", item 3): sym[k] a literal, a length symbol with its extra bits, or kPngNone.  Byte i is "same" when i > 0 and it equals byte
// i - 1; j is its distance from the first same byte of its stretch — position minus the last byte that is not same, minus 1, found
// by a running maximum over the workgroup and, in *carry, over the tiles before — and j % 258 its place in its piece: place 0
// begins a match when two more same bytes follow in the piece (its length: a walk through LDS, at most 257 steps, which a piece's
// other positions do not take), place 1 is silent when one more follows, a place from 2 on is always silent.
// All 256 threads call it (barriers inside); scan: 4 words.
__device__ __forceinline__ void png_tile_tokens(const uint8_t *bytes, unsigned n, unsigned t0, int *carry, int *scan, unsigned sym[4], unsigned extra_bits[4],
                                                unsigned extra[4])
{
        const unsigned p0 = t0 + threadIdx.x * 4;
        bool same[4];
        int last = -1;
#pragma unroll
        for(unsigned k = 0; k < 4; k++) {
                const unsigned p = p0 + k;
                same[k] = p > 0 && p < n && bytes[1 + p - t0] == bytes[p - t0];
                if(!same[k] && p < n) { last = (int)p; }
        }
        int all;
        int start = max(*carry, png_scan_max(last, scan, &all));
        *carry = max(*carry, all);
#pragma unroll
        for(unsigned k = 0; k < 4; k++) {
                const unsigned p = p0 + k;
                sym[k] = kPngNone;
                extra_bits[k] = extra[k] = 0;
                if(p >= n) { continue; }
                const uint8_t *at = bytes + 1 + p - t0;
                if(!same[k]) {
                        start = (int)p;
                        sym[k] = at[0];
                        continue;
                }
                const unsigned j = (p - (unsigned)start - 1u) % 258u;
                if(j >= 2) { continue; }
                const bool next = p + 1 < n && at[1] == at[0];
                if(j == 1) {
                        if(!next) { sym[k] = at[0]; }
                        continue;
                }
                if(!(next && p + 2 < n && at[2] == at[0])) {
                        sym[k] = at[0];
                        continue;
                }
                const unsigned most = min(258u, n - p);
                unsigned len = 3;
                while(len < most && at[len] == at[0]) { len++; }
                sym[k] = png_length_symbol(len, &extra_bits[k], &extra[k]);
        }
}

// counts: per block J2P_DEFLATE_COUNTS words — the 286 symbols' counts (EOB once), then the block's bytes d_i summed and summed with
// the weights n - i, both mod 65521 (j2p_deflate_adler_add).  A block has at most 2^24 bytes: 32 bits hold every count, 64 every sum.
__global__ __launch_bounds__(256) void k_png_count(const uint8_t *stream, size_t total, unsigned block_bytes, unsigned *counts)
{
        __shared__ unsigned hist[J2P_DEFLATE_SYMBOLS];
        __shared__ uint8_t bytes[kPngTileBytes + 3];
        __shared__ int scan[4];
        __shared__ unsigned long long sums[2][4];
        const size_t begin = (size_t)blockIdx.x * block_bytes;
        const unsigned n = (unsigned)min((size_t)block_bytes, total - begin);
        const uint8_t *src = stream + begin;
        for(unsigned i = threadIdx.x; i < J2P_DEFLATE_SYMBOLS; i += 256) { hist[i] = i == 256 ? 1u : 0u; }
        int carry = -1;
        unsigned long long s1 = 0, s2 = 0;
        for(unsigned t0 = 0; t0 < n; t0 += kPngTile) {
                png_tile_load(src, n, t0, bytes);
                unsigned sym[4], extra_bits[4], extra[4];
                png_tile_tokens(bytes, n, t0, &carry, scan, sym, extra_bits, extra);
#pragma unroll
                for(unsigned k = 0; k < 4; k++) {
                        const unsigned p = t0 + threadIdx.x * 4 + k;
                        if(sym[k] != kPngNone) { atomicAdd(&hist[sym[k]], 1u); }
                        if(p < n) {
                                const unsigned d = bytes[1 + p - t0];
                                s1 += d;
                                s2 += (unsigned long long)(n - p) * d;
                        }
                }
                __syncthreads();                                                // (the next trip overwrites bytes)
        }
#pragma unroll
        for(int d = 32; d >= 1; d >>= 1) {
                s1 += __shfl_xor(s1, d);
                s2 += __shfl_xor(s2, d);
        }
        if((threadIdx.x & 63u) == 0) {
                sums[0][threadIdx.x >> 6] = s1;
                sums[1][threadIdx.x >> 6] = s2;
        }
        __syncthreads();
        unsigned *out = counts + (size_t)blockIdx.x * J2P_DEFLATE_COUNTS;
        for(unsigned i = threadIdx.x; i < J2P_DEFLATE_SYMBOLS; i += 256) { out[i] = hist[i]; }
        if(threadIdx.x < 2) {
                const unsigned long long *s = sums[threadIdx.x];
                out[J2P_DEFLATE_SYMBOLS + threadIdx.x] = (unsigned)((s[0] % J2P_DEFLATE_ADLER + s[1] % J2P_DEFLATE_ADLER + s[2] % J2P_DEFLATE_ADLER + s[3] % J2P_DEFLATE_ADLER) % J2P_DEFLATE_ADLER);
        }
}

// `nbits` bits of `v`, lowest first, at bit `at` of the stream (bit 0: the lowest bit of word 0), ORed in: two words
__device__ __forceinline__ void png_or_bits(unsigned *words, unsigned long long at, unsigned long long v)
{
        const unsigned long long x = v << (at & 31u);
        if((unsigned)x) { atomicOr(words + (size_t)(at >> 5), (unsigned)x); }
        if((unsigned)(x >> 32)) { atomicOr(words + (size_t)(at >> 5) + 1, (unsigned)(x >> 32)); }
}

// stage: the zlib stream as little-endian words, zeroed, ceil(bytes / 4) + 1 of them; adler: of the filtered stream, which the last
// block's workgroup puts behind it; the first block's puts the two bytes 78 01 in front.
__global__ __launch_bounds__(256) void k_png_pack(const uint8_t *stream, size_t total, unsigned block_bytes, const PngBlock *blocks, unsigned adler,
                                                  unsigned *stage)
{
        __shared__ unsigned tab[J2P_DEFLATE_SYMBOLS];
        __shared__ unsigned words[kPngWords];
        __shared__ uint8_t bytes[kPngTileBytes + 3];
        __shared__ int scan[4];
        __shared__ unsigned long long lds[4];
        const PngBlock &blk = blocks[blockIdx.x];
        const size_t begin = (size_t)blockIdx.x * block_bytes;
        const unsigned n = (unsigned)min((size_t)block_bytes, total - begin);
        const uint8_t *src = stream + begin;
        for(unsigned i = threadIdx.x; i < J2P_DEFLATE_SYMBOLS; i += 256) { tab[i] = blk.code[i]; }
        for(unsigned i = threadIdx.x; i < kPngWords; i += 256) { words[i] = 0; }
        const unsigned long long first = blk.offset * 8;
        const unsigned header_bytes = (blk.header_bits + 7) / 8;
        for(unsigned i = threadIdx.x; i < header_bytes; i += 256) {
                if(const unsigned b = blk.header[i]) { png_or_bits(stage, first + 8ull * i, b); }
        }
        if(blockIdx.x == 0 && threadIdx.x == 0) { atomicOr(stage, 0x0178u); }
        unsigned long long base = first + blk.header_bits;
        int carry = -1;
        for(unsigned t0 = 0; t0 < n; t0 += kPngTile) {
                png_tile_load(src, n, t0, bytes);               // (its barrier also orders the zeroing of words before the ORs)
                unsigned sym[4], extra_bits[4], extra[4], nbits[4];
                unsigned long long code[4];
                png_tile_tokens(bytes, n, t0, &carry, scan, sym, extra_bits, extra);
                unsigned mine = 0;
#pragma unroll
                for(unsigned k = 0; k < 4; k++) {
                        nbits[k] = 0;
                        code[k] = 0;
                        if(sym[k] == kPngNone) { continue; }
                        const unsigned e = tab[sym[k]], len = e >> 16;
                        // a match: its length code, the extra bits, and the one distance code there is (distance 1): a 0 bit
                        code[k] = (e & 0xffffu) | ((unsigned long long)extra[k] << len);
                        nbits[k] = len + extra_bits[k] + (sym[k] > 256u ? 1u : 0u);
                        mine += nbits[k];
                }
                unsigned long long all;
                unsigned at = (unsigned)(base & 31u) + (unsigned)scan_workgroup(mine, lds, &all);
#pragma unroll
                for(unsigned k = 0; k < 4; k++) {
                        if(nbits[k]) { png_or_bits(words, at, code[k]); }
                        at += nbits[k];
                }
                __syncthreads();
                const unsigned nwords = ((unsigned)(base & 31u) + (unsigned)all + 31u) >> 5;     // (at most kPngWords - 2)
                for(unsigned w = threadIdx.x; w < nwords; w += 256) {
                        const unsigned x = words[w];
                        words[w] = 0;
                        unsigned *dst = stage + (size_t)(base >> 5) + w;
                        if(w == 0 || w == nwords - 1) {
                                if(x) { atomicOr(dst, x); }                     // shared with the header, the next tile or a neighbour
                        } else {
                                *dst = x;
                        }
                }
                base += all;
                __syncthreads();
        }
        if(threadIdx.x == 0) {
                const unsigned eob = tab[256];
                png_or_bits(stage, base, eob & 0xffffu);
                base += eob >> 16;
                if(!blk.final) {
                        // the empty stored block: three zero bits, zeros up to the byte, 00 00 FF FF
                        const unsigned long long byte = (base + 3 + 7) / 8;
                        png_or_bits(stage, (byte + 2) * 8, 0xffffu);
                } else {
                        const unsigned long long byte = (base + 7) / 8;
                        png_or_bits(stage, byte * 8, __builtin_bswap32(adler));
                }
        }
}

// ---- the container ----
// out: the IDAT chunks one behind the other, each 4 bytes of length, "IDAT", idat_bytes of the zlib stream (the last: the rest) and
// 4 bytes of CRC.  k_png_chunks copies the stream's bytes to their places, a thread 4 of them; k_png_crc (behind it) does the rest,
// a lane per chunk, byte by byte through a 256-entry table in LDS.
__global__ __launch_bounds__(256) void k_png_chunks(const uint8_t *z, size_t zlen, unsigned idat_bytes, uint8_t *out)
{
        const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
        for(size_t i = i0; i < i0 + 4 && i < zlen; i++) {
                const size_t chunk = i / idat_bytes;
                out[chunk * 12 + 8 + i] = z[i];
        }
}

__global__ __launch_bounds__(64) void k_png_crc(uint8_t *out, size_t zlen, unsigned idat_bytes, unsigned nchunks)
{
        __shared__ unsigned table[256];
        for(unsigned i = threadIdx.x; i < 256; i += 64) {
                unsigned c = i;
                for(int k = 0; k < 8; k++) { c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u))); }
                table[i] = c;
        }
        __syncthreads();
        const unsigned chunk = blockIdx.x * 64 + threadIdx.x;
        if(chunk >= nchunks) { return; }
        const size_t begin = (size_t)chunk * idat_bytes;
        const unsigned n = (unsigned)min((size_t)idat_bytes, zlen - begin);
        uint8_t *p = out + (size_t)chunk * ((size_t)idat_bytes + 12);
        const unsigned type = 0x49444154u;                                      // "IDAT"
        unsigned c = 0xffffffffu;
#pragma unroll
        for(int k = 3; k >= 0; k--) {
                p[3 - k] = (uint8_t)(n >> (8 * k));
                p[7 - k] = (uint8_t)(type >> (8 * k));
                c = table[(c ^ (type >> (8 * k))) & 255u] ^ (c >> 8);
        }
        for(unsigned i = 0; i < n; i++) { c = table[(c ^ p[8 + i]) & 255u] ^ (c >> 8); }
        c = ~c;
        p[8 + n] = (uint8_t)(c >> 24);
        p[9 + n] = (uint8_t)(c >> 16);
        p[10 + n] = (uint8_t)(c >> 8);
        p[11 + n] = (uint8_t)c;
}

}  // namespace j2p
