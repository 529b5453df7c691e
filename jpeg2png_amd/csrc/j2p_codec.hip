// jpeg2png_amd — the JPEG codec: quantised coefficients to the entropy-coded file a j2p_jpeg_options record describes
// (j2p_encode_options, j2p_entropy_encode_opt and its shorthands, over the file-local j2p_encode_scan and j2p_encode_progressive) and a
// baseline file's entropy-coded data back to coefficients (j2p_jpeg_open, j2p_decode_file, j2p_decoded_grids,
// j2p_entropy_decode; every scan of a progressive file: j2p_jpeg_open_scans, j2p_decode_scans_file, j2p_decode_opened,
// j2p_entropy_decode_scans; include/jpeg2png_amd.h, j2p_internal.h) — and, at the end, the PNG coder: samples to the filtered and
// deflated file (j2p_png_write, j2p_png_encode).
//
// A translation unit of its own, with its own device code (j2p_codec_kernels.hip.h, j2p_progressive_kernels.hip.h, j2p_decode_kernels.hip.h, j2p_scan_decode_kernels.hip.h): neither way
// uses a kernel of the output stage or of the solver, and an edit here recompiles neither.  It knows no solver: the output
// stage's j2p_planes_to_jpeg hands the coder its coefficients and a solver's scratch through j2p_encode_options.
//
// The three file coders each work in one device block whose size they learn on the way: j2p_coder_block.h asks `memory` for it and
// queues a coder's stages again when it moved, PooledCall is the stand-alone entry points' `memory`, stuffed_streams both JPEG coders' end.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <chrono>
#include <new>
#include <type_traits>
#include <vector>

#include "jpeg2png_amd.h"
#include "j2p_internal.h"
#include "j2p_coder_block.h"
#include "j2p_hip_host.h"
#include "j2p_huffman.h"
#include "j2p_restart.h"
#include "j2p_codec_kernels.hip.h"
#include "j2p_progressive_kernels.hip.h"
#include "j2p_decode_kernels.hip.h"
#include "j2p_scan_decode_kernels.hip.h"
#include "j2p_png_kernels.hip.h"

using namespace j2p;

// ---- the JPEG file: k_entropy_lengths, k_scan_*, k_entropy_pack, k_stuff_count, k_stuff_copy; k_entropy_histogram ----
namespace {

// Annex K.3 of the JPEG standard, as include/jpeg2png_amd.h states them: [0] the tables of component 0, [1] of the others
const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
const uint8_t kAcVals[2][162] = {
        {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
         0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
         0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
         0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
         0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
         0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
         0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
         0xfa},
        {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
         0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
         0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
         0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
         0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
         0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
         0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
         0xfa}};
// natural index of zigzag position k (the kernels' kZigzagNatural)
const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the codes of one table, by symbol: in order of length, consecutive within a length, doubled from one length to the next
void huffman_codes(const uint8_t bits[16], const uint8_t *vals, unsigned *by_symbol)
{
        unsigned code = 0, k = 0;
        for(unsigned length = 1; length <= 16; length++) {
                for(unsigned i = 0; i < bits[length - 1]; i++) { by_symbol[vals[k++]] = (length << 16) | code++; }
                code <<= 1;
        }
}
// the four tables of a file, as its DHT segments hold them: DC0, AC0, DC1, AC1
struct FileTables {
        j2p_huff_table t[4];
};
HuffCodes huffman_codes_of(const FileTables &f)
{
        HuffCodes h;
        memset(&h, 0, sizeof(h));
        for(int t = 0; t < 2; t++) {
                // (a DC table made for an image holds no symbol above 11: k_entropy_histogram counts none)
                unsigned dc[256] = {0};
                huffman_codes(f.t[2 * t].bits, f.t[2 * t].vals, dc);
                memcpy(h.dc[t], dc, sizeof(h.dc[t]));
                huffman_codes(f.t[2 * t + 1].bits, f.t[2 * t + 1].vals, h.ac[t]);
        }
        return h;
}
// Annex K.3
const FileTables &default_tables()
{
        static const FileTables tables = [] {
                FileTables f;
                memset(&f, 0, sizeof(f));
                for(int t = 0; t < 2; t++) {
                        memcpy(f.t[2 * t].bits, kDcBits[t], 16);
                        memcpy(f.t[2 * t].vals, kDcVals, 12);
                        f.t[2 * t].nvals = 12;
                        memcpy(f.t[2 * t + 1].bits, kAcBits[t], 16);
                        memcpy(f.t[2 * t + 1].vals, kAcVals[t], 162);
                        f.t[2 * t + 1].nvals = 162;
                }
                return f;
        }();
        return tables;
}
const HuffCodes &huffman_tables()
{
        static const HuffCodes tables = huffman_codes_of(default_tables());
        return tables;
}

// everything in front of the entropy-coded data; at most 623 bytes and the 6 of a DRI segment (a table has at most 12 DC or 162 AC symbols, which
// j2p_encode_scan checks of the ones it makes).  Returns their number.
constexpr size_t kJpegHeaderMax = 640;
// a marker segment's first four bytes at p, which moves behind them: the marker and the length of `payload` bytes and itself
void segment(uint8_t *&p, uint8_t marker, size_t payload)
{
        *p++ = 0xff;
        *p++ = marker;
        *p++ = (uint8_t)((payload + 2) >> 8);
        *p++ = (uint8_t)(payload + 2);
}
// one table's DHT segment at p, which moves behind it; id: (class << 4) | slot
void dht_segment(uint8_t *&p, unsigned id, const j2p_huff_table &t)
{
        segment(p, 0xc4, 1 + 16 + t.nvals);
        *p++ = (uint8_t)id;
        memcpy(p, t.bits, 16);
        memcpy(p + 16, t.vals, t.nvals);
        p += 16 + t.nvals;
}
// SOI, APP0, the DQTs and the frame header with marker `sof` (C0: baseline, C2: progressive); at most 200 bytes.  Returns their number.
size_t jpeg_frame(const j2p_jpeg &spec, unsigned ncomp, uint8_t sof, uint8_t *out)
{
        uint8_t *p = out;
        *p++ = 0xff;
        *p++ = 0xd8;
        static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
        segment(p, 0xe0, sizeof(jfif));
        memcpy(p, jfif, sizeof(jfif));
        p += sizeof(jfif);
        for(unsigned t = 0; t < (ncomp == 3 ? 2u : 1u); t++) {
                segment(p, 0xdb, 65);
                *p++ = (uint8_t)t;
                for(int k = 0; k < 64; k++) { *p++ = (uint8_t)spec.quant[t][kZigzag[k]]; }
        }
        segment(p, sof, 6 + 3 * ncomp);
        *p++ = 8;
        *p++ = (uint8_t)(spec.height >> 8);
        *p++ = (uint8_t)spec.height;
        *p++ = (uint8_t)(spec.width >> 8);
        *p++ = (uint8_t)spec.width;
        *p++ = (uint8_t)ncomp;
        for(unsigned c = 0; c < ncomp; c++) {
                *p++ = (uint8_t)(c + 1);
                *p++ = c == 0 && ncomp == 3 ? (uint8_t)((spec.sub_w << 4) | spec.sub_h) : 0x11;
                *p++ = c ? 1 : 0;
        }
        return (size_t)(p - out);
}
// a DRI segment at p, which moves behind it
void dri_segment(uint8_t *&p, unsigned interval)
{
        segment(p, 0xdd, 2);
        *p++ = (uint8_t)(interval >> 8);
        *p++ = (uint8_t)interval;
}
// dri: the scan's restart interval, 0 for a file without one (no DRI segment)
size_t jpeg_header(const j2p_jpeg &spec, unsigned ncomp, const FileTables &tables, unsigned dri, uint8_t *out)
{
        uint8_t *p = out + jpeg_frame(spec, ncomp, 0xc0, out);
        for(unsigned k = 0; k < (ncomp == 3 ? 4u : 2u); k++) { dht_segment(p, ((k & 1u) << 4) | (k >> 1), tables.t[k]); }
        if(dri) { dri_segment(p, dri); }
        segment(p, 0xda, 1 + 2 * ncomp + 3);
        *p++ = (uint8_t)ncomp;
        for(unsigned c = 0; c < ncomp; c++) {
                *p++ = (uint8_t)(c + 1);
                *p++ = c ? 0x11 : 0x00;
        }
        *p++ = 0;
        *p++ = 0x3f;
        *p++ = 0;
        return (size_t)(p - out);
}

// the scan's geometry for a spec that j2p_jpeg_error accepted, but for the coefficients' addresses
ScanGeom scan_geometry(const j2p_jpeg &spec, unsigned ncomp)
{
        const j2p_scan_grids grids = j2p_scan_grids_of(spec, ncomp);
        ScanGeom g;
        memset(&g, 0, sizeof(g));
        g.ncomp = ncomp;
        g.sub_w = grids.sub_w;
        g.sub_h = grids.sub_h;
        for(unsigned c = 0; c < ncomp; c++) {
                g.bw[c] = grids.bw[c];
                g.bh[c] = grids.bh[c];
        }
        g.mcus_w = (g.bw[0] + g.sub_w - 1) / g.sub_w;
        const unsigned mcus_h = (g.bh[0] + g.sub_h - 1) / g.sub_h;
        g.per_mcu = ncomp == 3 ? g.sub_w * g.sub_h + 2 : 1;
        g.nslots = ncomp == 3 ? g.mcus_w * mcus_h * g.per_mcu : g.bw[0] * g.bh[0];       // (at most 6 * 8192^2 / 4)
        return g;
}

using ull = unsigned long long;     // the kernels' 64-bit counts and offsets

// an exclusive sum of n counts on the stream: in -> out, sums: ceil(n / kScanTile) + 1 words, the last the total
void queue_scan(hipStream_t stream, const unsigned *in, unsigned n, unsigned long long *sums, unsigned long long *out)
{
        const unsigned ntiles = (n + kScanTile - 1) / kScanTile;
        hipLaunchKernelGGL(k_scan_sums, dim3(ntiles), dim3(256), 0, stream, in, n, sums);
        hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(256), 0, stream, sums, ntiles);
        hipLaunchKernelGGL(k_scan_apply, dim3(ntiles), dim3(256), 0, stream, in, n, static_cast<const unsigned long long *>(sums), out);
}

}  // namespace

j2p_scan_grids j2p_scan_grids_of(const j2p_jpeg &spec, unsigned ncomp)
{
        j2p_scan_grids g;
        memset(&g, 0, sizeof(g));
        g.sub_w = ncomp == 3 ? spec.sub_w : 1;
        g.sub_h = ncomp == 3 ? spec.sub_h : 1;
        g.bw[0] = (spec.width + 7) / 8;
        g.bh[0] = (spec.height + 7) / 8;
        for(unsigned c = 1; c < ncomp; c++) {
                g.bw[c] = (g.bw[0] + g.sub_w - 1) / g.sub_w;
                g.bh[c] = (g.bh[0] + g.sub_h - 1) / g.sub_h;
        }
        return g;
}

// j2p_huff_build (j2p_huffman.h), its refusals as a coder answers them
static int build_table(const uint64_t count[256], j2p_huff_table *table)
{
        const int rc = j2p_huff_build(count, table);
        if(rc == J2P_HUFF_COUNT) { return j2p_fail(J2P_ENOTSUP, "jpeg: a symbol is coded more than %llu times: no optimised table for it", J2P_HUFF_COUNT_MAX); }
        if(rc != J2P_HUFF_OK) { return j2p_fail(J2P_ENOTSUP, "jpeg: an optimised code would be longer than %d bits before limiting", J2P_HUFF_TREE_MAX); }
        return J2P_OK;
}

// The tables made for this image from the device's counts (hist: [table][12 DC + 256 AC], as k_entropy_histogram leaves them),
// and the counts as the caller sees them
static int tables_from_counts(const unsigned long long *hist, unsigned ncomp, FileTables &tables, j2p_encode_stats *stats)
{
        memset(&tables, 0, sizeof(tables));
        for(unsigned k = 0; k < 4; k++) {
                uint64_t count[256] = {0};
                const unsigned long long *from = hist + (k >> 1) * 268 + (k & 1u ? 12 : 0);
                for(unsigned s = 0; s < (k & 1u ? 256u : 12u); s++) { count[s] = from[s]; }
                if(stats) {
                        unsigned long long *to = k == 0 ? stats->dc0 : (k == 1 ? stats->ac0 : (k == 2 ? stats->dc1 : stats->ac1));
                        for(unsigned s = 0; s < 256; s++) { to[s] = count[s]; }
                }
                if(k >= 2 && ncomp != 3) { continue; }
                if(const int rc = build_table(count, &tables.t[k]); rc != J2P_OK) { return rc; }
                if(tables.t[k].nvals > (k & 1u ? 162u : 12u)) { return j2p_fail(J2P_EINVAL, "jpeg: a coefficient is outside [-1023, 1023]"); }
        }
        return J2P_OK;
}

namespace {

// what n streams of a JPEG file are once their FF bytes are counted
struct Stuffed {
        size_t nbytes[J2P_PROGRESSIVE_SCANS];   // stream s before stuffing
        ull ffs[J2P_PROGRESSIVE_SCANS + 1];     // the FF bytes, and twice the RSTn markers, of the streams before s; [n]: of all
        unsigned markers[J2P_PROGRESSIVE_SCANS] = {0};  // the RSTn markers of stream s (restart intervals)
        size_t bytes(unsigned s) const { return nbytes[s] + (size_t)(ffs[s + 1] - ffs[s]); }    // stream s in the file, markers included
        ull stuffed(unsigned s) const { return ffs[s + 1] - ffs[s] - 2ull * markers[s]; }       // FF bytes of stream s that got their 00
};

// where the RSTn markers of the streams stand (restart intervals): ends_at[s] is the place in the block of stream s's nends[s] sorted
// byte positions (k_restart_ends), which pack(s, stage) queues with the stream
struct RestartEnds {
        unsigned nends[J2P_PROGRESSIVE_SCANS];
        size_t ends_at[J2P_PROGRESSIVE_SCANS];
};

// The end both JPEG coders share: n streams (a baseline file's one scan, a progressive file's scans) of bits[s] bits, through the
// block's parts behind `part` — [stage: ceil(bits / 32) + 1 words per stream][count: chunks u32][ffoff: chunks u64][sums][out: the
// stuffed bytes, one stream behind the other] — to the host.  The block's last stage and its last two requests are here, and the
// block is not asked again afterwards: pack(s, stage) queues what leaves stream s in its zeroed words, then the FF bytes of every
// stream's chunks are counted and ONE exclusive sum places them all.  The sums at the streams' first chunks and the total come
// down (a wait); place(done, to) writes the file's size and, where the buffer has room for it (or else its error ends the call), the
// headers, and says where stream s goes on the host (to[s]); every stream is stuffed and comes down (a wait), and EOI follows the last.
// A baseline file cannot meet the refusal: its scan has at most 6 * 8192^2 / 4 slots of less than 1700 bits, 84 million chunks.
// restart (may be NULL: the launches are then what they were before restart intervals existed): a stream with markers is counted and
// copied by the _restart siblings of the two kernels, and the markers are bytes of the stream from the first guess on.
template<class Pack, class Place>
int stuffed_streams(hipStream_t stream, j2p_coder_block &block, j2p_carve &part, unsigned n, const ull *bits, const Pack &pack, const Place &place,
                    const RestartEnds *restart = nullptr)
{
        Stuffed done;
        size_t marker_bytes = 0;
        for(unsigned s = 0; restart && s < n; s++) {
                done.markers[s] = restart->nends[s];
                marker_bytes += 2 * (size_t)restart->nends[s];
        }
        const auto ends = [&](unsigned s) { return static_cast<const ull *>(block.at<ull>(restart->ends_at[s])); };
        size_t word[J2P_PROGRESSIVE_SCANS + 1] = {0}, chunk[J2P_PROGRESSIVE_SCANS + 1] = {0}, byte[J2P_PROGRESSIVE_SCANS + 1] = {0};
        for(unsigned s = 0; s < n; s++) {
                done.nbytes[s] = (size_t)((bits[s] + 7) / 8);
                word[s + 1] = word[s] + (size_t)((bits[s] + 31) / 32) + 1;
                chunk[s + 1] = chunk[s] + (done.nbytes[s] + kStuffChunk - 1) / kStuffChunk;
                byte[s + 1] = byte[s] + done.nbytes[s];
        }
        if(chunk[n] > 0x7fffffffull) { return j2p_fail(J2P_EINVAL, "jpeg: %zu bytes of scan data are too many", byte[n]); }
        const unsigned nchunks = (unsigned)chunk[n], chunk_tiles = (nchunks + kScanTile - 1) / kScanTile;
        const size_t stage_at = part(word[n] * 4), count_at = part((size_t)nchunks * 4), ffoff_at = part((size_t)nchunks * 8);
        const size_t ffsums_at = part(((size_t)chunk_tiles + 1) * 8), out_at = part.total;
        const auto chunks = [&](unsigned s) { return (unsigned)(chunk[s + 1] - chunk[s]); };
        // from the bit offsets to every stream and where its FF bytes are
        const auto streams = [&] {
                (void)hipMemsetAsync(block.at(stage_at), 0, word[n] * 4, stream);
                for(unsigned s = 0; s < n; s++) {
                        unsigned *const stage = block.at<unsigned>(stage_at) + word[s];
                        pack(s, stage);
                        if(done.markers[s]) {
                                hipLaunchKernelGGL(k_stuff_count_restart, dim3((chunks(s) + 3) / 4), dim3(256), 0, stream, static_cast<const unsigned *>(stage),
                                                   done.nbytes[s], chunks(s), ends(s), done.markers[s], block.at<unsigned>(count_at) + chunk[s]);
                                continue;
                        }
                        hipLaunchKernelGGL(k_stuff_count, dim3((chunks(s) + 3) / 4), dim3(256), 0, stream, static_cast<const unsigned *>(stage), done.nbytes[s],
                                           chunks(s), block.at<unsigned>(count_at) + chunk[s]);
                }
                queue_scan(stream, block.at<unsigned>(count_at), nchunks, block.at<ull>(ffsums_at), block.at<ull>(ffoff_at));
        };
        if(const int rc = block.grow(out_at + byte[n] + byte[n] / 16 + 256 + marker_bytes); rc != J2P_OK) { return rc; }
        block.stage(streams);
        done.ffs[0] = 0;
        for(unsigned s = 1; s < n; s++) { HIP_TRY(hipMemcpyAsync(&done.ffs[s], block.at<ull>(ffoff_at) + chunk[s], 8, hipMemcpyDeviceToHost, stream)); }
        HIP_TRY(hipMemcpyAsync(&done.ffs[n], block.at<ull>(ffsums_at) + chunk_tiles, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        uint8_t *to[J2P_PROGRESSIVE_SCANS];
        if(const int rc = place(done, to); rc != J2P_OK) { return rc; }
        if(const int rc = block.grow(out_at + byte[n] + (size_t)done.ffs[n]); rc != J2P_OK) { return rc; }
        for(unsigned s = 0; s < n; s++) {
                if(done.markers[s]) {
                        hipLaunchKernelGGL(k_stuff_copy_restart, dim3((chunks(s) + 3) / 4), dim3(256), 0, stream,
                                           static_cast<const unsigned *>(block.at<unsigned>(stage_at) + word[s]), done.nbytes[s], chunks(s),
                                           static_cast<const ull *>(block.at<ull>(ffoff_at) + chunk[s]), ends(s), done.markers[s],
                                           block.at<uint8_t>(out_at) + byte[s]);
                        HIP_TRY(hipMemcpyAsync(to[s], block.at(out_at) + byte[s] + (size_t)done.ffs[s], done.bytes(s), hipMemcpyDeviceToHost, stream));
                        continue;
                }
                hipLaunchKernelGGL(k_stuff_copy, dim3((chunks(s) + 3) / 4), dim3(256), 0, stream, static_cast<const unsigned *>(block.at<unsigned>(stage_at) + word[s]),
                                   done.nbytes[s], chunks(s), static_cast<const ull *>(block.at<ull>(ffoff_at) + chunk[s]), block.at<uint8_t>(out_at) + byte[s]);
                HIP_TRY(hipMemcpyAsync(to[s], block.at(out_at) + byte[s] + (size_t)done.ffs[s], done.bytes(s), hipMemcpyDeviceToHost, stream));
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        memcpy(to[n - 1] + done.bytes(n - 1), "\xff\xd9", 2);
        return J2P_OK;
}

}  // namespace

// The coder (j2p_internal.h: what memory and fill are).  The block's layout, each part aligned to 256 bytes:
//   [coefficients per component][len: nslots u32][off: nslots u64][sums: tiles + 1 u64]              known from the spec
//   [hist: 2 x 268 u64 — only when the symbols are counted]
//   [ends: intervals - 1 u64][padding: u64 — only with restart intervals that put a marker into the scan]
//   [stage: the stream, ceil(bits / 32) + 1 words][count: chunks u32][ffoff: chunks u64][sums]      known once the bits are
//   [out: the stuffed bytes]                                                                        known once the FFs are
// so the two totals are read back (8 bytes each, a wait each) and the block is asked for three times, the first two times
// with a guess for what is not known yet (j2p_coder_block.h).  Its stages are the coefficients, the lengths and — in
// stuffed_streams — the stream: a block that moved has them queued again.  A second image of the same size or smaller finds the
// block large enough at once.
// J2P_JPEG_OPTIMIZE (or stats) puts k_entropy_histogram and a third read-back and wait, of the 2 x 268 counters, between the
// coefficients and the lengths: the tables are made on the host (j2p_huffman.h) and this call's own HuffCodes go to the two
// coding kernels.  The counting is no stage: the counts live on the host from then on.  Without either, the launches, the layout
// and the bytes are what they were before the option existed.
// Restart intervals (include/jpeg2png_amd.h: "Restart intervals"; j2p_codec_kernels.hip.h says how) put the _restart siblings in the
// places of the three walking kernels, k_restart_pad and a second exclusive sum into the lengths stage and k_restart_ends into the
// stream's; the pads' sum comes down with the bits, so no wait is added.
static int j2p_encode_scan(hipStream_t stream, const j2p_jpeg &spec, unsigned ncomp, const std::function<int(size_t, void **, bool *)> &memory,
                           const std::function<void(hipStream_t, int16_t *const[3])> &fill, uint8_t *out_host, size_t capacity, size_t *size,
                           unsigned flags, j2p_encode_stats *stats, const j2p_restart_scan *restart, j2p_restart_scan_stats *restart_stats)
{
        ScanGeom g = scan_geometry(spec, ncomp);
        // restart intervals: ri positions each; the _restart kernels only where a marker stands (an interval that holds the whole scan
        // changes the header alone)
        const unsigned dri = restart ? restart->interval : 0, nint = restart ? restart->intervals : 1, ri = nint > 1 ? dri * g.per_mcu : 0;
        const bool optimise = (flags & J2P_JPEG_OPTIMIZE) != 0, counting = optimise || stats;
        HuffCodes own_codes;
        FileTables own_tables;
        const HuffCodes *codes = &huffman_tables();
        const FileTables *tables = &default_tables();
        const unsigned nslots = g.nslots, slot_tiles = (nslots + kScanTile - 1) / kScanTile;
        j2p_carve part;
        size_t coef_at[3];
        for(unsigned c = 0; c < ncomp; c++) { coef_at[c] = part(j2p_grid_bytes(g.bw[c], g.bh[c])); }
        const size_t coef_bytes = part.total;
        const size_t len_at = part((size_t)nslots * 4), off_at = part((size_t)nslots * 8), sums_at = part(((size_t)slot_tiles + 1) * 8);
        const size_t hist_at = counting ? part(kHistogramEntries * 8) : 0;
        const size_t ends_at = ri ? part((size_t)(nint - 1) * 8) : 0, padding_at = ri ? part(8) : 0;
        const size_t fixed = part.total;
        j2p_coder_block block(memory);
        const unsigned per_workgroup = 4 * kEntropyIters, coding_grid = (nslots + per_workgroup - 1) / per_workgroup;
        // the coefficients into the block
        const auto coefficients = [&] {
                int16_t *coef[3] = {nullptr, nullptr, nullptr};
                for(unsigned c = 0; c < ncomp; c++) { g.coef[c] = coef[c] = block.at<int16_t>(coef_at[c]); }
                fill(stream, coef);
        };
        // from the coefficients to the bit offsets
        const auto lengths = [&] {
                if(ri) {
                        // every interval's pad from the unpadded offsets into its last position's length; the offsets once more
                        hipLaunchKernelGGL(k_entropy_lengths_restart, dim3(coding_grid), dim3(256), 0, stream, g, *codes, ri, block.at<unsigned>(len_at));
                        queue_scan(stream, block.at<unsigned>(len_at), nslots, block.at<ull>(sums_at), block.at<ull>(off_at));
                        (void)hipMemsetAsync(block.at(padding_at), 0, 8, stream);
                        hipLaunchKernelGGL(k_restart_pad, dim3((nint + 255) / 256), dim3(256), 0, stream, block.at<unsigned>(len_at),
                                           static_cast<const ull *>(block.at<ull>(off_at)), static_cast<const ull *>(block.at<ull>(sums_at) + slot_tiles), nslots, ri,
                                           nint, block.at<ull>(padding_at));
                        queue_scan(stream, block.at<unsigned>(len_at), nslots, block.at<ull>(sums_at), block.at<ull>(off_at));
                        return;
                }
                hipLaunchKernelGGL(k_entropy_lengths, dim3(coding_grid), dim3(256), 0, stream, g, *codes, block.at<unsigned>(len_at));
                queue_scan(stream, block.at<unsigned>(len_at), nslots, block.at<ull>(sums_at), block.at<ull>(off_at));
        };
        if(const int rc = block.grow(fixed + coef_bytes / 4); rc != J2P_OK) { return rc; }     // (a file is rarely an eighth of its coefficients)
        block.stage(coefficients);
        if(stats) { memset(stats, 0, sizeof(*stats)); }
        if(counting) {
                unsigned long long hist[kHistogramEntries];
                HIP_TRY(hipMemsetAsync(block.at(hist_at), 0, sizeof(hist), stream));
                if(ri) {
                        hipLaunchKernelGGL(k_entropy_histogram_restart, dim3(coding_grid), dim3(256), 0, stream, g, ri, block.at<ull>(hist_at));
                } else {
                        hipLaunchKernelGGL(k_entropy_histogram, dim3(coding_grid), dim3(256), 0, stream, g, block.at<ull>(hist_at));
                }
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(hist, block.at(hist_at), sizeof(hist), hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipStreamSynchronize(stream));
                FileTables made;
                if(const int rc = tables_from_counts(hist, ncomp, made, stats); optimise && rc != J2P_OK) { return rc; }
                if(optimise) {
                        own_tables = made;
                        own_codes = huffman_codes_of(own_tables);
                        tables = &own_tables;
                        codes = &own_codes;
                }
        }
        block.stage(lengths);
        ull bits = 0, padding = 0;        // (with intervals `bits` holds every interval's pad, the last one's too)
        HIP_TRY(hipMemcpyAsync(&bits, block.at<ull>(sums_at) + slot_tiles, 8, hipMemcpyDeviceToHost, stream));
        if(ri) { HIP_TRY(hipMemcpyAsync(&padding, block.at(padding_at), 8, hipMemcpyDeviceToHost, stream)); }
        HIP_TRY(hipStreamSynchronize(stream));
        if(restart_stats) { *restart_stats = {dri, nint, ri ? padding : (0ull - bits) & 7ull, 0}; }
        RestartEnds ends;
        ends.nends[0] = nint - 1;
        ends.ends_at[0] = ends_at;
        return stuffed_streams(
                stream, block, part, 1, &bits,
                [&](unsigned, unsigned *stage) {
                        if(ri) {
                                hipLaunchKernelGGL(k_entropy_pack_restart, dim3(coding_grid), dim3(256), 0, stream, g, *codes, ri,
                                                   static_cast<const ull *>(block.at<ull>(off_at)), stage);
                                hipLaunchKernelGGL(k_restart_ends, dim3((nint - 1 + 255) / 256), dim3(256), 0, stream,
                                                   static_cast<const ull *>(block.at<ull>(off_at)), ri, nint - 1, block.at<ull>(ends_at));
                                return;
                        }
                        hipLaunchKernelGGL(k_entropy_pack, dim3(coding_grid), dim3(256), 0, stream, g, *codes,
                                           static_cast<const ull *>(block.at<ull>(off_at)), stage);
                },
                [&](const Stuffed &done, uint8_t **to) {
                        if(stats) { stats->scan_bits = bits - padding, stats->stuffed_bytes = done.stuffed(0); }
                        if(restart_stats) { restart_stats->markers = done.markers[0]; }
                        uint8_t header[kJpegHeaderMax];
                        const size_t header_bytes = jpeg_header(spec, ncomp, *tables, dri, header);
                        *size = header_bytes + done.bytes(0) + 2;
                        if(capacity < *size || !out_host) {
                                return j2p_fail(J2P_ESPACE, "jpeg: the file has %zu bytes, the buffer %zu", *size, out_host ? capacity : 0);
                        }
                        memcpy(out_host, header, header_bytes);
                        to[0] = out_host + header_bytes;
                        return (int)J2P_OK;
                },
                ri ? &ends : nullptr);
}

// ---- the progressive file: k_prog_* (j2p_progressive_kernels.hip.h), k_scan_*, k_stuff_* ----
namespace {

// jpeg_simple_progression(): (components; Ss-Se; Ah, Al)
struct ProgScript {
        unsigned ncomp, comp[3], ss, se, ah, al;
};
const ProgScript kProgColour[10] = {{3, {0, 1, 2}, 0, 0, 0, 1}, {1, {0}, 1, 5, 0, 2},  {1, {2}, 1, 63, 0, 1},       {1, {1}, 1, 63, 0, 1}, {1, {0}, 6, 63, 0, 2},
                                    {1, {0}, 1, 63, 2, 1},      {3, {0, 1, 2}, 0, 0, 1, 0}, {1, {2}, 1, 63, 1, 0}, {1, {1}, 1, 63, 1, 0}, {1, {0}, 1, 63, 1, 0}};
const ProgScript kProgGrey[6] = {{1, {0}, 0, 0, 0, 1}, {1, {0}, 1, 5, 0, 2}, {1, {0}, 6, 63, 0, 2}, {1, {0}, 1, 63, 2, 1}, {1, {0}, 0, 0, 1, 0}, {1, {0}, 1, 63, 1, 0}};

// the tables a scan carries, in DHT order, as (class << 4) | slot: a DC first scan its components' DC tables, an AC scan its AC table
unsigned prog_scan_tables(const ProgScript &s, unsigned table[2])
{
        if(s.ss == 0 && s.ah == 0) {
                table[0] = 0x00;
                table[1] = 0x01;
                return s.ncomp == 3 ? 2 : 1;
        }
        if(s.ss == 0) { return 0; }
        table[0] = 0x10 | (s.comp[0] ? 1u : 0u);
        return 1;
}

// a scan's DHT segments, DRI and SOS; at most 2 * 277 + 6 + 14 bytes.  Returns their number.
constexpr size_t kProgScanHeaderMax = 576;
// restart: the scan's entry of the restart plan (NULL: none): its DRI segment, where the plan has one, stands in front of the SOS
size_t prog_scan_header(const ProgScript &s, unsigned ntables, const unsigned table[2], const j2p_huff_table made[2], const j2p_restart_scan *restart,
                        uint8_t *out)
{
        uint8_t *p = out;
        for(unsigned k = 0; k < ntables; k++) { dht_segment(p, table[k], made[k]); }
        if(restart && restart->dri) { dri_segment(p, restart->interval); }
        segment(p, 0xda, 1 + 2 * s.ncomp + 3);
        *p++ = (uint8_t)s.ncomp;
        for(unsigned i = 0; i < s.ncomp; i++) {
                const unsigned slot = s.comp[i] ? 1u : 0u;
                *p++ = (uint8_t)(s.comp[i] + 1);
                *p++ = (uint8_t)(((s.ss == 0 && s.ah == 0 ? slot : 0u) << 4) | (s.se ? slot : 0u));
        }
        *p++ = (uint8_t)s.ss;
        *p++ = (uint8_t)s.se;
        *p++ = (uint8_t)((s.ah << 4) | s.al);
        return (size_t)(p - out);
}

}  // namespace

// The progressive coder (j2p_internal.h: what memory and fill are).  A scan's ITEMS are its positions (DC) or its component's blocks
// (AC); all scans' items stand in one row, scan after scan.  The block's layout, each part aligned to 256 bytes:
//   [coefficients per component][len: items u32][off: items u64][sums][per AC scan — flags: blocks u8][per AC scan — run: blocks u32]
//   [hist: scans x 512 u64][flushes: scans u64]                                                      known from the spec
//   [per scan with restart markers — ends: intervals - 1 u64][padding: scans u64 — only with such a scan]
//   [stage: every scan's stream, ceil(bits / 32) + 1 words each][count: chunks u32][ffoff: chunks u64][sums]   once the bits are
//   [out: every scan's stuffed bytes, one behind the other]                                          once the FFs are
// ONE exclusive sum places the items of all scans (a scan's stream starts at its first item's offset) and ONE the FF counts of all
// scans' chunks, so three reads come back as arrays — all counts, all scans' bits, all scans' FFs — with a wait each, as in the
// optimised call, and the file's bytes with a fourth.  The block is asked for three times as j2p_encode_scan's is, with the same
// three stages (j2p_coder_block.h): the coefficients — with them the flags and the EOB runs — every scan's lengths, and in
// stuffed_streams every scan's stream.  The walk that counts is no stage: the counts and tables live on the host by then.
static int j2p_encode_progressive(hipStream_t stream, const j2p_jpeg &spec, unsigned ncomp, const std::function<int(size_t, void **, bool *)> &memory,
                                  const std::function<void(hipStream_t, int16_t *const[3])> &fill, uint8_t *out_host, size_t capacity, size_t *size,
                                  j2p_progressive_stats *stats, const j2p_restart_plan *restart, j2p_restart_stats *restart_stats)
{
        ScanGeom g = scan_geometry(spec, ncomp);
        const ProgScript *const script = ncomp == 3 ? kProgColour : kProgGrey;
        const unsigned nscans = ncomp == 3 ? 10 : 6;
        ProgScan scan[J2P_PROGRESSIVE_SCANS];
        size_t first[J2P_PROGRESSIVE_SCANS + 1] = {0};
        // restart intervals: ri[s] items each in scan s, nint[s] of them; ri 0 where no marker stands (no intervals, or one that holds
        // the whole scan), and such a scan's launches are the ones it had before restart intervals existed
        unsigned ri[J2P_PROGRESSIVE_SCANS] = {0}, nint[J2P_PROGRESSIVE_SCANS];
        bool restarts = false;
        for(unsigned s = 0; s < nscans; s++) {
                const ProgScript &k = script[s];
                const unsigned c = k.comp[0];
                scan[s] = {k.ss, k.se, k.al, k.ah ? 1u : 0u, k.ss == 0 ? g.nslots : g.bw[c] * g.bh[c]};
                first[s + 1] = first[s] + scan[s].n;
                nint[s] = restart ? restart->scan[s].intervals : 1;
                if(nint[s] > 1) { ri[s] = restart->scan[s].interval * (k.ss == 0 ? g.per_mcu : 1u); }
                restarts = restarts || ri[s];
        }
        const size_t nitems = first[nscans];
        if(nitems > 0xffffffffull) { return j2p_fail(J2P_EINVAL, "jpeg: %zu scan positions are too many", nitems); }
        const unsigned item_tiles = (unsigned)((nitems + kScanTile - 1) / kScanTile);
        j2p_carve part;
        size_t coef_at[3], flags_at[J2P_PROGRESSIVE_SCANS] = {0}, run_at[J2P_PROGRESSIVE_SCANS] = {0};
        for(unsigned c = 0; c < ncomp; c++) { coef_at[c] = part(j2p_grid_bytes(g.bw[c], g.bh[c])); }
        const size_t coef_bytes = part.total;
        const size_t len_at = part(nitems * 4), off_at = part(nitems * 8), sums_at = part(((size_t)item_tiles + 1) * 8);
        for(unsigned s = 0; s < nscans; s++) {
                if(scan[s].ss) { flags_at[s] = part((size_t)scan[s].n); }
        }
        const size_t runs_at = part.total;
        for(unsigned s = 0; s < nscans; s++) {
                if(scan[s].ss) { run_at[s] = part((size_t)scan[s].n * 4); }
        }
        const size_t runs_bytes = part.total - runs_at;
        const size_t hist_bytes = (size_t)nscans * (kProgHistogram + 1) * 8;
        const size_t hist_at = part(hist_bytes);                         // (the flush counters behind the counts)
        size_t ends_at[J2P_PROGRESSIVE_SCANS] = {0};
        for(unsigned s = 0; s < nscans; s++) {
                if(ri[s]) { ends_at[s] = part((size_t)(nint[s] - 1) * 8); }
        }
        const size_t padding_at = restarts ? part((size_t)nscans * 8) : 0, fixed = part.total;
        j2p_coder_block block(memory);
        const auto grid = [](unsigned n) { return dim3((n + 255) / 256); };
        static const ProgCodes no_codes = {};
        std::vector<ProgCodes> codes(nscans, no_codes);
        const int16_t *coef[3] = {nullptr, nullptr, nullptr};
        // the coefficients into the block, and what of every AC scan needs no table: the blocks' flags and the EOB runs
        const auto coefficients = [&] {
                int16_t *into[3] = {nullptr, nullptr, nullptr};
                for(unsigned c = 0; c < ncomp; c++) { coef[c] = g.coef[c] = into[c] = block.at<int16_t>(coef_at[c]); }
                fill(stream, into);
                (void)hipMemsetAsync(block.at(hist_at), 0, hist_bytes, stream);
                (void)hipMemsetAsync(block.at(runs_at), 0, runs_bytes, stream);
                for(unsigned s = 0; s < nscans; s++) {
                        if(scan[s].ss == 0) { continue; }
                        const unsigned per_workgroup = 4 * kEntropyIters;
                        hipLaunchKernelGGL(k_prog_classify, dim3((scan[s].n + per_workgroup - 1) / per_workgroup), dim3(256), 0, stream,
                                           coef[script[s].comp[0]], scan[s], block.at<uint8_t>(flags_at[s]));
                        if(ri[s]) {
                                hipLaunchKernelGGL(k_prog_runs_restart, grid(scan[s].n), dim3(256), 0, stream,
                                                   static_cast<const uint8_t *>(block.at<uint8_t>(flags_at[s])), scan[s], ri[s], block.at<unsigned>(run_at[s]),
                                                   block.at<ull>(hist_at) + (size_t)nscans * kProgHistogram + s);
                                continue;
                        }
                        hipLaunchKernelGGL(k_prog_runs, grid(scan[s].n), dim3(256), 0, stream, static_cast<const uint8_t *>(block.at<uint8_t>(flags_at[s])),
                                           scan[s], block.at<unsigned>(run_at[s]), block.at<ull>(hist_at) + (size_t)nscans * kProgHistogram + s);
                }
        };
        // one scan's walk in one of its three modes
        const auto walk = [&](auto mode, unsigned s, unsigned *stage) {
                constexpr int kMode = decltype(mode)::value;
                ull *const hist = block.at<ull>(hist_at) + (size_t)s * kProgHistogram;
                unsigned *const len = block.at<unsigned>(len_at) + first[s];
                const ull *const off = block.at<ull>(off_at) + first[s];
                if(scan[s].ss == 0) {
                        if(kMode == kProgCount && scan[s].refine) { return; }
                        if(ri[s]) {
                                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_prog_dc_restart<kMode>), grid(scan[s].n), dim3(256), 0, stream, g, scan[s], ri[s], codes[s], hist,
                                                   len, off, stage);
                                return;
                        }
                        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_prog_dc<kMode>), grid(scan[s].n), dim3(256), 0, stream, g, scan[s], codes[s], hist, len, off, stage);
                } else if(kMode == kProgPack && ri[s]) {
                        hipLaunchKernelGGL(k_prog_ac_pack_restart, grid(scan[s].n), dim3(256), 0, stream, coef[script[s].comp[0]], scan[s], ri[s],
                                           static_cast<const uint8_t *>(block.at<uint8_t>(flags_at[s])), static_cast<const unsigned *>(block.at<unsigned>(run_at[s])),
                                           codes[s], off, stage);
                } else {
                        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_prog_ac<kMode>), grid(scan[s].n), dim3(256), 0, stream, coef[script[s].comp[0]], scan[s],
                                           static_cast<const uint8_t *>(block.at<uint8_t>(flags_at[s])), static_cast<const unsigned *>(block.at<unsigned>(run_at[s])),
                                           codes[s], hist, len, off, stage);
                }
        };
        const auto lengths = [&] {
                for(unsigned s = 0; s < nscans; s++) { walk(std::integral_constant<int, kProgLength>(), s, nullptr); }
                queue_scan(stream, block.at<unsigned>(len_at), (unsigned)nitems, block.at<ull>(sums_at), block.at<ull>(off_at));
                if(!restarts) { return; }
                // every interval's pad from the unpadded offsets into its last item's length; the offsets once more
                (void)hipMemsetAsync(block.at(padding_at), 0, (size_t)nscans * 8, stream);
                for(unsigned s = 0; s < nscans; s++) {
                        if(!ri[s]) { continue; }
                        const ull *const behind = s + 1 < nscans ? block.at<ull>(off_at) + first[s + 1] : block.at<ull>(sums_at) + item_tiles;
                        hipLaunchKernelGGL(k_restart_pad, grid(nint[s]), dim3(256), 0, stream, block.at<unsigned>(len_at) + first[s],
                                           static_cast<const ull *>(block.at<ull>(off_at) + first[s]), behind, scan[s].n, ri[s], nint[s],
                                           block.at<ull>(padding_at) + s);
                }
                queue_scan(stream, block.at<unsigned>(len_at), (unsigned)nitems, block.at<ull>(sums_at), block.at<ull>(off_at));
        };
        if(const int rc = block.grow(fixed + coef_bytes / 4); rc != J2P_OK) { return rc; }
        block.stage(coefficients);
        for(unsigned s = 0; s < nscans; s++) { walk(std::integral_constant<int, kProgCount>(), s, nullptr); }
        HIP_TRY(hipGetLastError());
        // wait 1: every scan's counts
        std::vector<unsigned long long> hist;
        try {
                hist.resize(hist_bytes / 8);
        } catch(const std::bad_alloc &) { return j2p_fail(J2P_ENOMEM, "out of memory"); }
        HIP_TRY(hipMemcpyAsync(hist.data(), block.at(hist_at), hist_bytes, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if(stats) {
                memset(stats, 0, sizeof(*stats));
                stats->nscans = nscans;
        }
        j2p_huff_table made[J2P_PROGRESSIVE_SCANS][2];
        unsigned ntables[J2P_PROGRESSIVE_SCANS], table[J2P_PROGRESSIVE_SCANS][2] = {};   // (zero behind a scan's ntables: stats copy both)
        memset(made, 0, sizeof(made));
        int refused = J2P_OK;
        for(unsigned s = 0; s < nscans; s++) {
                ntables[s] = prog_scan_tables(script[s], table[s]);
                if(stats) {
                        j2p_progressive_scan &o = stats->scan[s];
                        o.ncomp = script[s].ncomp;
                        memcpy(o.comp, script[s].comp, sizeof(o.comp));
                        o.ss = script[s].ss, o.se = script[s].se, o.ah = script[s].ah, o.al = script[s].al;
                        o.ntables = ntables[s];
                        memcpy(o.table, table[s], sizeof(o.table));
                        o.eob_runs = hist[(size_t)nscans * kProgHistogram + s];
                }
                for(unsigned k = 0; k < ntables[s]; k++) {
                        uint64_t count[256];
                        for(unsigned i = 0; i < 256; i++) { count[i] = hist[(size_t)s * kProgHistogram + k * 256 + i]; }
                        if(stats) { memcpy(stats->scan[s].counts[k], count, sizeof(count)); }
                        if(refused != J2P_OK) { continue; }
                        refused = build_table(count, &made[s][k]);
                        // a DC category above 11, an AC size above 10: the shifted magnitude needs more bits than the file's precision has
                        for(unsigned i = 0; i < made[s][k].nvals && refused == J2P_OK; i++) {
                                const unsigned v = made[s][k].vals[i];
                                if(table[s][k] & 0x10 ? (v & 15u) > 10u : v > 11u) { refused = j2p_fail(J2P_EINVAL, "jpeg: a coefficient is outside [-1023, 1023]"); }
                        }
                        huffman_codes(made[s][k].bits, made[s][k].vals, codes[s].code[k]);
                }
        }
        if(refused != J2P_OK) { return refused; }
        // wait 2: every scan's bits
        block.stage(lengths);
        ull begins[J2P_PROGRESSIVE_SCANS + 1] = {0}, bits[J2P_PROGRESSIVE_SCANS];
        for(unsigned s = 1; s < nscans; s++) { HIP_TRY(hipMemcpyAsync(&begins[s], block.at<ull>(off_at) + first[s], 8, hipMemcpyDeviceToHost, stream)); }
        HIP_TRY(hipMemcpyAsync(&begins[nscans], block.at<ull>(sums_at) + item_tiles, 8, hipMemcpyDeviceToHost, stream));
        ull padding[J2P_PROGRESSIVE_SCANS] = {0};       // (a scan with intervals: its bits hold every interval's pad, the last one's too)
        if(restarts) { HIP_TRY(hipMemcpyAsync(padding, block.at(padding_at), (size_t)nscans * 8, hipMemcpyDeviceToHost, stream)); }
        HIP_TRY(hipStreamSynchronize(stream));
        RestartEnds ends;
        if(restart_stats) {
                memset(restart_stats, 0, sizeof(*restart_stats));
                restart_stats->nscans = nscans;
        }
        for(unsigned s = 0; s < nscans; s++) {
                bits[s] = begins[s + 1] - begins[s];
                if(stats) { stats->scan[s].bits = bits[s] - padding[s]; }
                ends.nends[s] = ri[s] ? nint[s] - 1 : 0;
                ends.ends_at[s] = ends_at[s];
                if(restart_stats) {
                        restart_stats->scan[s] = {restart ? restart->scan[s].interval : 0, nint[s], ri[s] ? padding[s] : (0ull - bits[s]) & 7ull, ends.nends[s]};
                }
        }
        // waits 3 and 4: every scan's FF bytes; the scans' bytes to their places in the file, the headers between them
        return stuffed_streams(
                stream, block, part, nscans, bits,
                [&](unsigned s, unsigned *stage) {
                        walk(std::integral_constant<int, kProgPack>(), s, stage);
                        if(ri[s]) {
                                hipLaunchKernelGGL(k_restart_ends, grid(nint[s] - 1), dim3(256), 0, stream, static_cast<const ull *>(block.at<ull>(off_at) + first[s]),
                                                   ri[s], nint[s] - 1, block.at<ull>(ends_at[s]));
                        }
                },
                [&](const Stuffed &done, uint8_t **to) {
                        uint8_t frame[256];
                        std::vector<uint8_t> heads;
                        size_t head_at[J2P_PROGRESSIVE_SCANS + 1] = {0};
                        const size_t frame_bytes = jpeg_frame(spec, ncomp, 0xc2, frame);
                        try {
                                heads.resize((size_t)nscans * kProgScanHeaderMax);
                        } catch(const std::bad_alloc &) { return j2p_fail(J2P_ENOMEM, "out of memory"); }
                        for(unsigned s = 0; s < nscans; s++) {
                                if(stats) { stats->scan[s].stuffed_bytes = done.stuffed(s); }
                                head_at[s + 1] = head_at[s] + prog_scan_header(script[s], ntables[s], table[s], made[s], restart ? &restart->scan[s] : nullptr,
                                                                                 heads.data() + head_at[s]);
                        }
                        *size = frame_bytes + head_at[nscans] + 2;
                        for(unsigned s = 0; s < nscans; s++) { *size += done.bytes(s); }
                        if(capacity < *size || !out_host) {
                                return j2p_fail(J2P_ESPACE, "jpeg: the file has %zu bytes, the buffer %zu", *size, out_host ? capacity : 0);
                        }
                        memcpy(out_host, frame, frame_bytes);
                        uint8_t *p = out_host + frame_bytes;
                        for(unsigned s = 0; s < nscans; s++) {
                                memcpy(p, heads.data() + head_at[s], head_at[s + 1] - head_at[s]);
                                to[s] = p + head_at[s + 1] - head_at[s];
                                p = to[s] + done.bytes(s);
                        }
                        return (int)J2P_OK;
                },
                restarts ? &ends : nullptr);
}

const char *j2p_jpeg_options_error(const j2p_jpeg_options *options)
{
        if(!options) { return "jpeg: NULL options"; }
        if(options->flags & ~J2P_JPEG_OPTIMIZE) { return "jpeg: unknown flag bits"; }
        if(options->progressive > 1) { return "jpeg: progressive is 0 or 1"; }
        return j2p_restart_error(options->restart_interval, options->restart_in_rows);
}

int j2p_encode_options(hipStream_t stream, const j2p_jpeg &spec, unsigned ncomp, const j2p_jpeg_options &options,
                       const std::function<int(size_t, void **, bool *)> &memory, const std::function<void(hipStream_t, int16_t *const[3])> &fill,
                       uint8_t *out_host, size_t capacity, size_t *size, j2p_encode_stats *stats, j2p_progressive_stats *progressive_stats,
                       j2p_restart_stats *restart_stats)
{
        const bool restarts = options.restart_interval || options.restart_in_rows;
        const j2p_restart_plan plan = j2p_restart_plan_of(spec.width, spec.height, ncomp, spec.sub_w, spec.sub_h, options.progressive != 0,
                                                          options.restart_interval, options.restart_in_rows);
        if(restart_stats) { memset(restart_stats, 0, sizeof(*restart_stats)); }
        if(options.progressive) {
                return j2p_encode_progressive(stream, spec, ncomp, memory, fill, out_host, capacity, size, progressive_stats, restarts ? &plan : nullptr,
                                              restart_stats);
        }
        j2p_restart_scan_stats one = {0, 0, 0, 0};
        const int rc = j2p_encode_scan(stream, spec, ncomp, memory, fill, out_host, capacity, size, options.flags, stats, restarts ? &plan.scan[0] : nullptr,
                                       restart_stats ? &one : nullptr);
        if(restart_stats && one.intervals) {
                restart_stats->nscans = 1;
                restart_stats->scan[0] = one;
        }
        return rc;
}

// the device of a j2p_entropy_* call
static int check_device(int device)
{
        int have = 0;
        if(hipGetDeviceCount(&have) != hipSuccess || have <= 0) { return j2p_fail(J2P_EDEVICE, "no HIP device available"); }
        if(device < 0 || device >= have) { return j2p_fail(J2P_EINVAL, "device %d out of range (0..%d)", device, have - 1); }
        return J2P_OK;
}

// What a stand-alone call (j2p_entropy_encode*, j2p_png_encode) gives its coder: a stream of its own and, as `memory` (std::ref), one
// pooled block that grows as the solvers' scratch does — a request beyond it waits for the stream (what is queued may still read
// the old block), gives the block back and takes a larger one.  The calling thread's device is `device`.
struct PooledCall {
        const int device;
        hipStream_t stream = nullptr;
        void *block = nullptr;
        size_t block_bytes = 0;
        explicit PooledCall(int device) : device(device) {}
        PooledCall(const PooledCall &) = delete;
        PooledCall &operator=(const PooledCall &) = delete;
        int open()
        {
                HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
                return J2P_OK;
        }
        int operator()(size_t bytes, void **p, bool *moved)
        {
                *moved = block_bytes < bytes;
                if(*moved) {
                        HIP_TRY(hipStreamSynchronize(stream));
                        j2p_pool_give(device, block, block_bytes);
                        block = nullptr;
                        block_bytes = 0;
                        HIP_TRY(j2p_pool_take(device, bytes, &block, &block_bytes));
                }
                *p = block;
                return J2P_OK;
        }
        ~PooledCall()
        {
                if(!stream) { return; }
                (void)hipStreamSynchronize(stream);
                j2p_pool_give(device, block, block_bytes);
                (void)hipStreamDestroy(stream);
        }
};

extern "C" {

// The file `options` describe from the caller's coefficients in host memory: the argument checks, in the order the header gives
// them, and a PooledCall for j2p_encode_options.  A NULL stats pointer stays NULL on the way down, so only a caller who asks has the symbols counted.
int j2p_entropy_encode_opt(int device, const j2p_jpeg *spec, const int16_t *const coef_host[3], unsigned ncomp, uint8_t *out_host, size_t capacity,
                           size_t *size, const j2p_jpeg_options *options, j2p_encode_stats *stats, j2p_progressive_stats *progressive_stats,
                           j2p_restart_stats *restart_stats)
{
        if(!coef_host || !size) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(const char *why = j2p_jpeg_options_error(options)) { return j2p_fail(J2P_EINVAL, "%s", why); }
        if(const char *why = j2p_jpeg_error(spec, ncomp)) { return j2p_fail(J2P_EINVAL, "%s", why); }
        const j2p_scan_grids g = j2p_scan_grids_of(*spec, ncomp);
        size_t values[3] = {0, 0, 0};
        for(unsigned c = 0; c < ncomp; c++) {
                if(!coef_host[c]) { return j2p_fail(J2P_EINVAL, "jpeg: component %u has no coefficients", c); }
                values[c] = (size_t)g.bw[c] * g.bh[c] * 64;
                for(size_t i = 0; i < values[c]; i++) {
                        if(coef_host[c][i] < -1023 || coef_host[c][i] > 1023) {
                                return j2p_fail(J2P_EINVAL, "jpeg: component %u: coefficient %d (block %zu, index %zu) is outside [-1023, 1023]", c,
                                                coef_host[c][i], i / 64, i % 64);
                        }
                }
        }
        if(const int rc = check_device(device); rc != J2P_OK) { return rc; }
        DeviceGuard guard(device);
        PooledCall call(device);
        if(const int rc = call.open(); rc != J2P_OK) { return rc; }
        return j2p_encode_options(
                call.stream, *spec, ncomp, *options, std::ref(call),
                [&](hipStream_t st, int16_t *const coef[3]) {
                        for(unsigned c = 0; c < ncomp; c++) {
                                (void)hipMemcpyAsync(coef[c], coef_host[c], values[c] * sizeof(int16_t), hipMemcpyHostToDevice, st);
                        }
                },
                out_host, capacity, size, stats, progressive_stats, restart_stats);
}

// the shorthands: each is j2p_entropy_encode_opt with its record
int j2p_entropy_encode_ex(int device, const j2p_jpeg *spec, const int16_t *const coef_host[3], unsigned ncomp, uint8_t *out_host, size_t capacity,
                          size_t *size, unsigned flags, j2p_encode_stats *stats)
{
        const j2p_jpeg_options options = {flags, 0, 0, 0};
        return j2p_entropy_encode_opt(device, spec, coef_host, ncomp, out_host, capacity, size, &options, stats, nullptr, nullptr);
}

int j2p_entropy_encode_progressive(int device, const j2p_jpeg *spec, const int16_t *const coef_host[3], unsigned ncomp, uint8_t *out_host, size_t capacity,
                                   size_t *size, j2p_progressive_stats *stats)
{
        const j2p_jpeg_options options = {0, 1, 0, 0};
        return j2p_entropy_encode_opt(device, spec, coef_host, ncomp, out_host, capacity, size, &options, nullptr, stats, nullptr);
}

int j2p_entropy_encode(int device, const j2p_jpeg *spec, const int16_t *const coef_host[3], unsigned ncomp, uint8_t *out_host, size_t capacity,
                       size_t *size)
{
        const j2p_jpeg_options options = {0, 0, 0, 0};
        return j2p_entropy_encode_opt(device, spec, coef_host, ncomp, out_host, capacity, size, &options, nullptr, nullptr, nullptr);
}

int j2p_debug_restart_plan(unsigned width, unsigned height, unsigned ncomp, unsigned sub_w, unsigned sub_h, const j2p_jpeg_options *options,
                           j2p_restart_plan *plan)
{
        if(!plan) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(const char *why = j2p_jpeg_options_error(options)) { return j2p_fail(J2P_EINVAL, "%s", why); }
        if((ncomp != 1 && ncomp != 3) || width < 1 || height < 1 || width > 65535 || height > 65535 || sub_w < 1 || sub_w > 2 || sub_h < 1 || sub_h > 2) {
                return j2p_fail(J2P_EINVAL, "jpeg: no such file: %ux%u, %u components, %ux%u blocks of the first in an MCU", width, height, ncomp, sub_w, sub_h);
        }
        *plan = j2p_restart_plan_of(width, height, ncomp, sub_w, sub_h, options->progressive != 0, options->restart_interval, options->restart_in_rows);
        return J2P_OK;
}

}  // extern "C"

// ---- reading a JPEG file: k_unstuff_*, k_decode_* (j2p_decode_kernels.hip.h), the scans above ----
namespace {

DecodeTables decode_tables(const j2p_jpeg_parsed &p, unsigned S)
{
        DecodeTables t;
        memset(&t, 0, sizeof(t));
        for(int s = 0; s < 4; s++) {
                t.tab[s] = p.dc[s];
                t.tab[4 + s] = p.ac[s];
        }
        const j2p_jpeg_info &f = p.info;
        DecodeGeom &g = t.g;
        g.ncomp = f.ncomp;
        g.per_mcu = f.blocks_per_mcu;
        g.mcus_w = f.mcus_w;
        g.nmcus = f.mcus_w * f.mcus_h;
        g.ri = f.restart_interval ? f.restart_interval : g.nmcus;
        g.nint = f.intervals;
        g.nblocks = g.nmcus * g.per_mcu;
        g.S = S;
        unsigned blk = 0;
        for(unsigned c = 0; c < f.ncomp; c++) {
                g.bw[c] = f.comp[c].blocks_w;
                g.bh[c] = f.comp[c].blocks_h;
                g.hs[c] = f.ncomp == 1 ? 1 : f.comp[c].h_samp_factor;
                g.vs[c] = f.ncomp == 1 ? 1 : f.comp[c].v_samp_factor;
                g.first_blk[c] = blk;
                g.comp_base[c] = g.nmcus * blk;
                g.dc_tab[c] = f.comp[c].dc_slot;
                g.ac_tab[c] = f.comp[c].ac_slot;
                for(unsigned k = 0; k < g.hs[c] * g.vs[c]; k++) { g.blk_comp[blk++] = c; }
        }
        return t;
}

const char *decode_error_text(unsigned flags)
{
        if(flags & kDecodeBadMarker) { return "a restart marker is missing or out of sequence"; }
        if(flags & kDecodeBadCode) { return "a code that is in no Huffman table"; }
        if(flags & kDecodeBadRun) { return "a run past coefficient 63"; }
        if(flags & kDecodeBadEnd) { return "the scan is truncated, or data is left over behind its last block"; }
        if(flags & kDecodeBadDc) { return "a DC value outside int16"; }
        if(flags & kDecodeBadRefine) { return "a refinement scan's symbol of more than one bit"; }
        if(flags & kDecodeBadEobRun) { return "an EOB run past the last block of its restart interval"; }
        return "the block count disagrees with the decoder's state";
}

// rounds queued before the change counters are first read back, and between two reads after that
constexpr unsigned kDecodeFirstGroup = 3, kDecodeGroup = 4;

}  // namespace

// The decoder: p's scan from `data` (the entropy-coded bytes p.info.scan_begin.., HOST memory, or DEVICE memory of `device` read in
// place) into the device grids coef[c] (blocks_w * blocks_h * 64 int16 each), on `stream`, which has been waited for on return.  One
// pooled block holds every intermediate and goes back before returning.  stats may be NULL.
int j2p_decode_file(int device, hipStream_t stream, const j2p_jpeg_parsed *parsed, const uint8_t *data, bool data_on_device, unsigned S,
                    int16_t *const coef[3], j2p_decode_stats *stats)
{
        const j2p_jpeg_parsed &p = *parsed;
        const j2p_jpeg_info &f = p.info;
        if(S == 0) { S = J2P_DECODE_SUBSEQUENCE_BITS; }
        if(S < J2P_DECODE_SUBSEQUENCE_MIN || S > J2P_DECODE_SUBSEQUENCE_MAX) {
                return j2p_fail(J2P_EINVAL, "decode: %u bits in a subsequence (%u..%u)", S, J2P_DECODE_SUBSEQUENCE_MIN, J2P_DECODE_SUBSEQUENCE_MAX);
        }
        const size_t nraw = f.scan_end - f.scan_begin;
        if(nraw == 0) { return j2p_fail(J2P_EFORMAT, "jpeg: the scan holds no data"); }
        const unsigned long long bound = ((unsigned long long)nraw * 8 + S - 1) / S + f.intervals;
        const unsigned long long blocks = (unsigned long long)f.mcus_w * f.mcus_h * f.blocks_per_mcu;
        if(bound > 0x7fffffffull || blocks > 0xffffffffull || nraw / kUnstuffChunk > 0x7fffffffull) {
                return j2p_fail(J2P_EINVAL, "decode: %zu bytes of data are too many for subsequences of %u bits", nraw, S);
        }
        const DecodeTables tables = decode_tables(p, S);
        const unsigned nint = f.intervals, nbound = (unsigned)bound, nblocks = tables.g.nblocks;
        const unsigned nchunks = (unsigned)((nraw + kUnstuffChunk - 1) / kUnstuffChunk);
        const auto tiles = [](unsigned n) { return (n + kScanTile - 1) / kScanTile; };
        const size_t clean_room = (nraw + 16 + 3) / 4 * 4;
        j2p_carve take;
        const size_t raw_at = take(data_on_device ? 0 : nraw), clean_at = take(clean_room);
        const size_t keepc_at = take((size_t)nchunks * 4), markc_at = take((size_t)nchunks * 4), keepo_at = take((size_t)nchunks * 8);
        const size_t marko_at = take((size_t)nchunks * 8), keeps_at = take(((size_t)tiles(nchunks) + 1) * 8), marks_at = take(((size_t)tiles(nchunks) + 1) * 8);
        const size_t rst_at = take((size_t)nint * 8), icount_at = take((size_t)nint * 4), first_at = take((size_t)nint * 8);
        const size_t isums_at = take(((size_t)tiles(nint) + 1) * 8);
        const size_t exit_at[2] = {take((size_t)nbound * 8), take((size_t)nbound * 8)};
        const size_t last_at = take((size_t)nbound * 8), done_at = take((size_t)nbound * 4), before_at = take((size_t)nbound * 8);
        const size_t dsums_at = take(((size_t)tiles(nbound) + 1) * 8);
        const size_t diff_at = take((size_t)nblocks * 4), dc_at = take((size_t)nblocks * 8), dcsums_at = take(((size_t)tiles(nblocks) + 1) * 8);
        const size_t tables_at = take(sizeof(DecodeTables)), flags_at = take(256);     // flags: [0] the error word, [1..] the rounds' change counters
        void *block = nullptr;
        size_t block_bytes = 0;
        HIP_TRY(j2p_pool_take(device, take.total, &block, &block_bytes));
        char *const base = static_cast<char *>(block);
        const auto u32 = [&](size_t at) { return reinterpret_cast<unsigned *>(base + at); };
        const auto u64 = [&](size_t at) { return reinterpret_cast<unsigned long long *>(base + at); };
        unsigned *const flags = u32(flags_at);
        // everything below leaves through `finish`, which gives the block back once the stream is idle
        const auto finish = [&](int rc) {
                (void)hipStreamSynchronize(stream);
                j2p_pool_give(device, block, block_bytes);
                return rc;
        };
        const auto failed = [&](hipError_t e, const char *what) { return finish(j2p_fail(J2P_EDEVICE, "decode: %s: %s", what, hipGetErrorString(e))); };

        const auto t_begin = std::chrono::steady_clock::now();
        const uint8_t *raw = data;
        hipError_t e = hipSuccess;
        if(!data_on_device) {
                e = hipMemcpyAsync(base + raw_at, data, nraw, hipMemcpyHostToDevice, stream);
                raw = reinterpret_cast<const uint8_t *>(base + raw_at);
        }
        if(e == hipSuccess) { e = hipMemcpyAsync(base + tables_at, &tables, sizeof(tables), hipMemcpyHostToDevice, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + clean_at, 0xff, clean_room, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + rst_at, 0, (size_t)nint * 8, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + exit_at[0], 0, (size_t)nbound * 8, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + last_at, 0xff, (size_t)nbound * 8, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + done_at, 0, (size_t)nbound * 4, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + diff_at, 0, (size_t)nblocks * 4, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(flags, 0, 256, stream); }
        if(e != hipSuccess) { return failed(e, "staging"); }
        // the clean stream and the restart markers' places
        hipLaunchKernelGGL(k_unstuff_count, dim3((nchunks + 3) / 4), dim3(256), 0, stream, raw, nraw, nchunks, u32(keepc_at), u32(markc_at));
        queue_scan(stream, u32(keepc_at), nchunks, u64(keeps_at), u64(keepo_at));
        queue_scan(stream, u32(markc_at), nchunks, u64(marks_at), u64(marko_at));
        hipLaunchKernelGGL(k_unstuff_copy, dim3((nchunks + 3) / 4), dim3(256), 0, stream, raw, nraw, nchunks, static_cast<const unsigned long long *>(u64(keepo_at)),
                           static_cast<const unsigned long long *>(u64(marko_at)), nint, reinterpret_cast<uint8_t *>(base + clean_at), clean_room, u64(rst_at),
                           flags);
        // the subsequences of every interval
        DecodeBuffers b;
        b.tables = reinterpret_cast<const DecodeTables *>(base + tables_at);
        b.words = u32(clean_at);
        b.nwords = clean_room / 4;
        b.clean_bytes = u64(keeps_at) + tiles(nchunks);
        b.nmarkers = u64(marks_at) + tiles(nchunks);
        b.rst = u64(rst_at);
        b.first = u64(first_at);
        b.nsub = u64(isums_at) + tiles(nint);
        b.error = flags;
        hipLaunchKernelGGL(k_decode_intervals, dim3((nint + 255) / 256), dim3(256), 0, stream, b, nint, S, u32(icount_at));
        queue_scan(stream, u32(icount_at), nint, u64(isums_at), u64(first_at));
        // rounds until no entry state changes: at most one per subsequence of the longest interval, and one that finds nothing to do
        j2p_decode_stats st;
        memset(&st, 0, sizeof(st));
        st.intervals = nint;
        unsigned rounds = 0;
        bool settled = false;
        while(!settled) {
                if(rounds > nbound) { return finish(j2p_fail(J2P_EFORMAT, "jpeg: the decoder's states did not settle in %u rounds", rounds)); }
                const unsigned group = rounds == 0 ? kDecodeFirstGroup : kDecodeGroup;
                if(rounds) { (void)hipMemsetAsync(flags + 1, 0, group * 4, stream); }
                for(unsigned q = 0; q < group; q++, rounds++) {
                        hipLaunchKernelGGL(k_decode_sync, dim3((nbound + 255) / 256), dim3(256), 0, stream, b, nbound,
                                           static_cast<const unsigned long long *>(u64(exit_at[rounds & 1])), u64(exit_at[(rounds + 1) & 1]), u64(last_at),
                                           u32(done_at), flags + 1 + q);
                }
                unsigned seen[1 + kDecodeGroup] = {0};
                unsigned long long totals[2] = {0, 0};
                e = hipMemcpyAsync(seen, flags, (1 + group) * 4, hipMemcpyDeviceToHost, stream);
                if(e == hipSuccess) { e = hipMemcpyAsync(&totals[0], b.nsub, 8, hipMemcpyDeviceToHost, stream); }
                if(e == hipSuccess) { e = hipMemcpyAsync(&totals[1], b.clean_bytes, 8, hipMemcpyDeviceToHost, stream); }
                if(e == hipSuccess) { e = hipStreamSynchronize(stream); }
                if(e != hipSuccess) { return failed(e, "rounds"); }
                if(seen[0]) { return finish(j2p_fail(J2P_EFORMAT, "jpeg: %s", decode_error_text(seen[0]))); }
                st.subsequences = (unsigned)totals[0];
                st.data_bytes = totals[1];
                for(unsigned q = 0; q < group && !settled; q++) {
                        if(seen[1 + q] == 0) {
                                settled = true;
                        } else {
                                if(st.rounds < J2P_DECODE_STATS_ROUNDS) { st.recomputed[st.rounds] = seen[1 + q]; }
                                st.rounds++;
                        }
                }
        }
        const unsigned long long *const exits = u64(exit_at[rounds & 1]);       // what the last round queued wrote
        // the block ordinals, the ACs and the DC differences, the DCs
        queue_scan(stream, u32(done_at), nbound, u64(dsums_at), u64(before_at));
        DecodeOut o;
        memset(&o, 0, sizeof(o));
        for(unsigned c = 0; c < f.ncomp; c++) {
                o.coef[c] = coef[c];
                (void)hipMemsetAsync(coef[c], 0, j2p_grid_bytes(f.comp[c].blocks_w, f.comp[c].blocks_h), stream);
        }
        o.diff = u32(diff_at);
        hipLaunchKernelGGL(k_decode_write, dim3((nbound + 255) / 256), dim3(256), 0, stream, b, nbound, exits, static_cast<const unsigned long long *>(u64(before_at)), o);
        queue_scan(stream, u32(diff_at), nblocks, u64(dcsums_at), u64(dc_at));
        hipLaunchKernelGGL(k_decode_dc, dim3((nblocks + 255) / 256), dim3(256), 0, stream, b.tables, static_cast<const unsigned *>(u32(diff_at)),
                           static_cast<const unsigned long long *>(u64(dc_at)), o, flags);
        unsigned bad = 0;
        e = hipGetLastError();
        if(e == hipSuccess) { e = hipMemcpyAsync(&bad, flags, 4, hipMemcpyDeviceToHost, stream); }
        if(e == hipSuccess) { e = hipStreamSynchronize(stream); }
        if(e != hipSuccess) { return failed(e, "the final pass"); }
        if(bad) { return finish(j2p_fail(J2P_EFORMAT, "jpeg: %s", decode_error_text(bad))); }
        st.decode_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        if(stats) { *stats = st; }
        return finish(J2P_OK);
}

// ---- reading a progressive JPEG file: k_unstuff_* per scan, k_scans_* (j2p_scan_decode_kernels.hip.h) ----
// Every scan is unstuffed by launches of its own into one clean buffer (no host wait: a scan's clean bytes are at most its raw ones,
// so the host knows where each begins).  All first scans share one subsequence array and the rounds of j2p_decode_file, so the host
// waits as often as for one baseline scan, whatever the number of scans; the refinement scans are queued behind the final pass in
// file order, and the one wait that ends the decode covers them.
int j2p_decode_scans_file(int device, hipStream_t stream, const j2p_scans_parsed *parsed, const uint8_t *data, bool data_on_device, unsigned S,
                          int16_t *const coef[3], j2p_scans_stats *stats)
{
        const j2p_scans_parsed &p = *parsed;
        const j2p_jpeg_info &f = p.base.info;
        const unsigned nscans = p.scans.nscans;
        if(S == 0) { S = J2P_DECODE_SUBSEQUENCE_BITS; }
        if(S < J2P_DECODE_SUBSEQUENCE_MIN || S > J2P_DECODE_SUBSEQUENCE_MAX) {
                return j2p_fail(J2P_EINVAL, "decode: %u bits in a subsequence (%u..%u)", S, J2P_DECODE_SUBSEQUENCE_MIN, J2P_DECODE_SUBSEQUENCE_MAX);
        }
        if(!p.scans.progressive || nscans == 0 || nscans > J2P_DECODE_SCANS_MAX) { return j2p_fail(J2P_EINVAL, "decode: not a progressive file's scans"); }
        const size_t nraw = f.scan_end - f.scan_begin;
        const auto tiles = [](unsigned n) { return (n + kScanTile - 1) / kScanTile; };
        // the scans as the kernels see them, and how much of everything there is
        std::vector<ScanDesc> descs(nscans);
        std::vector<unsigned short> iscan;
        struct Unstuff {
                size_t raw_at, nraw, clean_room;
                unsigned nchunks;
                size_t keepc, markc, keepo, marko, keeps, marks;
        };
        std::vector<Unstuff> un(nscans);
        j2p_scans_stats st;
        memset(&st, 0, sizeof(st));
        st.scans = nscans;
        unsigned long long clean_room = 0, nint_all = 0, bound = 0, ndiff = 0, data_bytes = 0;
        for(unsigned s = 0; s < nscans; s++) {
                const j2p_jpeg_scan &q = p.scans.scan[s];
                ScanDesc &d = descs[s];
                memset(&d, 0, sizeof(d));
                d.kind = q.ss == 0 ? (q.ah ? kScanDcRefine : kScanDcFirst) : (q.ah ? kScanAcRefine : kScanAcFirst);
                (d.kind == kScanDcFirst ? st.dc_first : d.kind == kScanAcFirst ? st.ac_first : d.kind == kScanDcRefine ? st.dc_refine : st.ac_refine)++;
                d.ncomp = q.ncomp;
                unsigned blk = 0;
                unsigned long long units = q.ncomp > 1 ? (unsigned long long)f.mcus_w * f.mcus_h : 0;
                for(unsigned c = 0; c < q.ncomp; c++) {
                        const j2p_jpeg_component &k = f.comp[q.comp[c]];
                        d.comp[c] = q.comp[c];
                        d.bw[c] = k.blocks_w;
                        d.bh[c] = k.blocks_h;
                        d.hs[c] = q.ncomp == 1 ? 1 : k.h_samp_factor;
                        d.vs[c] = q.ncomp == 1 ? 1 : k.v_samp_factor;
                        d.first_blk[c] = blk;
                        d.dc_tab[c] = d.kind == kScanDcFirst ? p.dc_table[s][c] : 0;
                        if(q.ncomp == 1) { units = (unsigned long long)k.blocks_w * k.blocks_h; }
                        for(unsigned i = 0; i < d.hs[c] * d.vs[c] && blk < 12; i++) { d.blk_comp[blk++] = c; }
                }
                d.per_mcu = blk;
                if(units * blk > 0xffffffffull || units == 0) { return j2p_fail(J2P_EINVAL, "decode: a scan of %llu blocks is too large", units * blk); }
                for(unsigned c = 0; c < q.ncomp; c++) { d.comp_off[c] = (unsigned)units * d.first_blk[c]; }
                d.ac_tab = q.ss ? p.ac_table[s] : 0;
                d.mcus_w = q.ncomp == 1 ? d.bw[0] : f.mcus_w;
                d.units = (unsigned)units;
                d.ri = q.restart_interval && q.restart_interval < d.units ? q.restart_interval : d.units;
                d.nint = q.intervals;
                d.nblocks = d.units * d.per_mcu;
                d.ss = q.ss;
                d.se = q.se;
                d.al = q.al;
                if(d.nint != (d.units + d.ri - 1) / d.ri || q.end <= q.begin || q.begin < f.scan_begin || q.end > f.scan_end) {
                        return j2p_fail(J2P_EINVAL, "decode: scan %u is inconsistent", s);
                }
                d.rst_base = (unsigned)nint_all;
                d.clean_base = clean_room;
                Unstuff &u = un[s];
                u.raw_at = q.begin - f.scan_begin;
                u.nraw = q.end - q.begin;
                u.clean_room = (u.nraw + 16 + 3) / 4 * 4;
                if(u.nraw / kUnstuffChunk > 0x7fffffffull) { return j2p_fail(J2P_EINVAL, "decode: %zu bytes of data are too many", u.nraw); }
                u.nchunks = (unsigned)((u.nraw + kUnstuffChunk - 1) / kUnstuffChunk);
                clean_room += u.clean_room;
                data_bytes += u.nraw;
                nint_all += d.nint;
                if(d.kind == kScanDcFirst || d.kind == kScanAcFirst) {
                        d.sub_base = (unsigned)iscan.size();
                        try {
                                iscan.insert(iscan.end(), d.nint, (unsigned short)s);
                        } catch(const std::bad_alloc &) { return j2p_fail(J2P_ENOMEM, "out of memory"); }
                        bound += ((unsigned long long)u.nraw * 8 + S - 1) / S + d.nint;
                }
                if(d.kind == kScanDcFirst) {
                        d.diff_base = (unsigned)ndiff;
                        ndiff += d.nblocks;
                }
        }
        if(bound > 0x7fffffffull || nint_all > 0x7fffffffull || ndiff > 0xffffffffull || iscan.empty()) {
                return j2p_fail(J2P_EINVAL, "decode: %zu bytes of data are too many for subsequences of %u bits", nraw, S);
        }
        const unsigned nfirst = (unsigned)iscan.size(), nbound = (unsigned)bound, nint = (unsigned)nint_all, nblocks = (unsigned)ndiff;
        j2p_carve take;
        const size_t raw_at = take(data_on_device ? 0 : nraw), clean_at = take(clean_room);
        for(Unstuff &u : un) {
                u.keepc = take((size_t)u.nchunks * 4);
                u.markc = take((size_t)u.nchunks * 4);
                u.keepo = take((size_t)u.nchunks * 8);
                u.marko = take((size_t)u.nchunks * 8);
                u.keeps = take(((size_t)tiles(u.nchunks) + 1) * 8);
                u.marks = take(((size_t)tiles(u.nchunks) + 1) * 8);
        }
        const size_t rst_at = take((size_t)nint * 8), icount_at = take((size_t)nfirst * 4), first_at = take((size_t)nfirst * 8);
        const size_t isums_at = take(((size_t)tiles(nfirst) + 1) * 8), iscan_at = take((size_t)nfirst * 2);
        const size_t exit_at[2] = {take((size_t)nbound * 8), take((size_t)nbound * 8)};
        const size_t last_at = take((size_t)nbound * 8), done_at = take((size_t)nbound * 4), before_at = take((size_t)nbound * 8);
        const size_t dsums_at = take(((size_t)tiles(nbound) + 1) * 8);
        const size_t diff_at = take((size_t)nblocks * 4), dc_at = take((size_t)nblocks * 8), dcsums_at = take(((size_t)tiles(nblocks) + 1) * 8);
        const size_t descs_at = take(sizeof(ScanDesc) * nscans), pool_at = take(sizeof(j2p_huff_decode) * (p.ntables ? p.ntables : 1)), flags_at = take(256);
        void *block = nullptr;
        size_t block_bytes = 0;
        HIP_TRY(j2p_pool_take(device, take.total, &block, &block_bytes));
        char *const base = static_cast<char *>(block);
        const auto u32 = [&](size_t at) { return reinterpret_cast<unsigned *>(base + at); };
        const auto u64 = [&](size_t at) { return reinterpret_cast<unsigned long long *>(base + at); };
        unsigned *const flags = u32(flags_at);
        hipEvent_t ev[2] = {nullptr, nullptr};
        const auto finish = [&](int rc) {
                (void)hipStreamSynchronize(stream);
                for(hipEvent_t e : ev) {
                        if(e) { (void)hipEventDestroy(e); }
                }
                j2p_pool_give(device, block, block_bytes);
                return rc;
        };
        const auto failed = [&](hipError_t e, const char *what) { return finish(j2p_fail(J2P_EDEVICE, "decode: %s: %s", what, hipGetErrorString(e))); };
        for(unsigned s = 0; s < nscans; s++) {
                descs[s].clean_bytes = u64(un[s].keeps) + tiles(un[s].nchunks);
                descs[s].nmarkers = u64(un[s].marks) + tiles(un[s].nchunks);
        }

        const auto t_begin = std::chrono::steady_clock::now();
        const uint8_t *raw = data;
        hipError_t e = hipSuccess;
        if(!data_on_device) {
                e = hipMemcpyAsync(base + raw_at, data, nraw, hipMemcpyHostToDevice, stream);
                raw = reinterpret_cast<const uint8_t *>(base + raw_at);
        }
        if(e == hipSuccess) { e = hipMemcpyAsync(base + descs_at, descs.data(), sizeof(ScanDesc) * nscans, hipMemcpyHostToDevice, stream); }
        if(e == hipSuccess && p.ntables) { e = hipMemcpyAsync(base + pool_at, p.pool, sizeof(j2p_huff_decode) * p.ntables, hipMemcpyHostToDevice, stream); }
        if(e == hipSuccess) { e = hipMemcpyAsync(base + iscan_at, iscan.data(), (size_t)nfirst * 2, hipMemcpyHostToDevice, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + clean_at, 0xff, clean_room, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + rst_at, 0, (size_t)nint * 8, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + exit_at[0], 0, (size_t)nbound * 8, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + last_at, 0xff, (size_t)nbound * 8, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + done_at, 0, (size_t)nbound * 4, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + diff_at, 0, (size_t)nblocks * 4, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(flags, 0, 256, stream); }
        for(unsigned c = 0; c < f.ncomp && e == hipSuccess; c++) { e = hipMemsetAsync(coef[c], 0, j2p_grid_bytes(f.comp[c].blocks_w, f.comp[c].blocks_h), stream); }
        if(e != hipSuccess) { return failed(e, "staging"); }
        // every scan's clean stream and its restart markers' places
        for(unsigned s = 0; s < nscans; s++) {
                const Unstuff &u = un[s];
                const uint8_t *const from = raw + u.raw_at;
                hipLaunchKernelGGL(k_unstuff_count, dim3((u.nchunks + 3) / 4), dim3(256), 0, stream, from, u.nraw, u.nchunks, u32(u.keepc), u32(u.markc));
                queue_scan(stream, u32(u.keepc), u.nchunks, u64(u.keeps), u64(u.keepo));
                queue_scan(stream, u32(u.markc), u.nchunks, u64(u.marks), u64(u.marko));
                hipLaunchKernelGGL(k_unstuff_copy, dim3((u.nchunks + 3) / 4), dim3(256), 0, stream, from, u.nraw, u.nchunks,
                                   static_cast<const unsigned long long *>(u64(u.keepo)), static_cast<const unsigned long long *>(u64(u.marko)), descs[s].nint,
                                   reinterpret_cast<uint8_t *>(base + clean_at + descs[s].clean_base), u.clean_room, u64(rst_at) + descs[s].rst_base, flags);
        }
        ScansBuffers b;
        b.scans = reinterpret_cast<const ScanDesc *>(base + descs_at);
        b.pool = reinterpret_cast<const j2p_huff_decode *>(base + pool_at);
        b.words = u32(clean_at);
        b.nwords = clean_room / 4;
        b.rst = u64(rst_at);
        b.iscan = reinterpret_cast<const unsigned short *>(base + iscan_at);
        b.first = u64(first_at);
        b.nsub = u64(isums_at) + tiles(nfirst);
        b.nfirst = nfirst;
        b.S = S;
        b.error = flags;
        hipLaunchKernelGGL(k_scans_intervals, dim3((nfirst + 255) / 256), dim3(256), 0, stream, b, u32(icount_at));
        queue_scan(stream, u32(icount_at), nfirst, u64(isums_at), u64(first_at));
        // the rounds of the first scans, all together
        unsigned rounds = 0;
        bool settled = false;
        while(!settled) {
                if(rounds > nbound) { return finish(j2p_fail(J2P_EFORMAT, "jpeg: the decoder's states did not settle in %u rounds", rounds)); }
                const unsigned group = rounds == 0 ? kDecodeFirstGroup : kDecodeGroup;
                if(rounds) { (void)hipMemsetAsync(flags + 1, 0, group * 4, stream); }
                for(unsigned q = 0; q < group; q++, rounds++) {
                        hipLaunchKernelGGL(k_scans_sync, dim3((nbound + 255) / 256), dim3(256), 0, stream, b, nbound,
                                           static_cast<const unsigned long long *>(u64(exit_at[rounds & 1])), u64(exit_at[(rounds + 1) & 1]), u64(last_at),
                                           u32(done_at), flags + 1 + q);
                }
                unsigned seen[1 + kDecodeGroup] = {0};
                unsigned long long total = 0;
                e = hipMemcpyAsync(seen, flags, (1 + group) * 4, hipMemcpyDeviceToHost, stream);
                if(e == hipSuccess) { e = hipMemcpyAsync(&total, b.nsub, 8, hipMemcpyDeviceToHost, stream); }
                if(e == hipSuccess) { e = hipStreamSynchronize(stream); }
                st.host_waits++;
                if(e != hipSuccess) { return failed(e, "rounds"); }
                if(seen[0]) { return finish(j2p_fail(J2P_EFORMAT, "jpeg: %s", decode_error_text(seen[0]))); }
                st.subsequences = (unsigned)total;
                for(unsigned q = 0; q < group && !settled; q++) {
                        if(seen[1 + q] == 0) {
                                settled = true;
                        } else {
                                st.rounds++;
                        }
                }
        }
        const unsigned long long *const exits = u64(exit_at[rounds & 1]);
        queue_scan(stream, u32(done_at), nbound, u64(dsums_at), u64(before_at));
        ScansOut o;
        memset(&o, 0, sizeof(o));
        for(unsigned c = 0; c < f.ncomp; c++) { o.coef[c] = coef[c]; }
        o.diff = u32(diff_at);
        hipLaunchKernelGGL(k_scans_write, dim3((nbound + 255) / 256), dim3(256), 0, stream, b, nbound, exits, static_cast<const unsigned long long *>(u64(before_at)), o);
        queue_scan(stream, u32(diff_at), nblocks, u64(dcsums_at), u64(dc_at));
        for(unsigned s = 0; s < nscans; s++) {
                if(descs[s].kind == kScanDcFirst) {
                        hipLaunchKernelGGL(k_scans_dc, dim3((descs[s].nblocks + 255) / 256), dim3(256), 0, stream, b, s, static_cast<const unsigned *>(u32(diff_at)),
                                           static_cast<const unsigned long long *>(u64(dc_at)), o);
                }
        }
        // the refinement scans: a coefficient's come behind its first scan and in file order; DC and AC ones touch different coefficients
        for(unsigned s = 0; s < nscans; s++) {
                if(descs[s].kind == kScanDcRefine) { hipLaunchKernelGGL(k_scans_dc_refine, dim3((descs[s].nblocks + 255) / 256), dim3(256), 0, stream, b, s, o); }
        }
        if(st.ac_refine) {
                e = hipEventCreate(&ev[0]);
                if(e == hipSuccess) { e = hipEventCreate(&ev[1]); }
                if(e == hipSuccess) { e = hipEventRecord(ev[0], stream); }
                if(e != hipSuccess) { return failed(e, "events"); }
                for(unsigned s = 0; s < nscans; s++) {
                        if(descs[s].kind == kScanAcRefine) {
                                hipLaunchKernelGGL(k_scans_ac_refine, dim3((descs[s].nint + 3) / 4), dim3(256), 0, stream, b, s, coef[descs[s].comp[0]]);
                        }
                }
                e = hipEventRecord(ev[1], stream);
                if(e != hipSuccess) { return failed(e, "events"); }
        }
        unsigned bad = 0;
        e = hipGetLastError();
        if(e == hipSuccess) { e = hipMemcpyAsync(&bad, flags, 4, hipMemcpyDeviceToHost, stream); }
        if(e == hipSuccess) { e = hipStreamSynchronize(stream); }
        st.host_waits++;
        if(e != hipSuccess) { return failed(e, "the final pass"); }
        if(bad) { return finish(j2p_fail(J2P_EFORMAT, "jpeg: %s", decode_error_text(bad))); }
        st.data_bytes = data_bytes;
        st.decode_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        if(st.ac_refine) {
                float ms = 0.f;
                if(hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess && st.decode_ms > 0.) { st.ac_refine_share = (double)ms / st.decode_ms; }
        }
        if(stats) { *stats = st; }
        return finish(J2P_OK);
}

int j2p_jpeg_open(const uint8_t *file, size_t size, j2p_jpeg_file *opened)
{
        *opened = j2p_jpeg_file();
        if(!file || size == 0) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        int where = -1;
        const int kind = j2p_memory_of_pointer(file, &where);
        if(kind == J2P_MEMORY_OTHER) { return j2p_fail(J2P_EINVAL, "jpeg: the file lies in managed or unknown memory (plain device memory, or host memory)"); }
        // the parser reads host memory: a file in device memory comes down for it, and the copy goes when this returns
        std::unique_ptr<uint8_t[]> copy;
        if(kind == J2P_MEMORY_DEVICE) {
                copy.reset(new(std::nothrow) uint8_t[size]);
                if(!copy) { return j2p_fail(J2P_ENOMEM, "out of memory"); }
                if(const hipError_t e = hipMemcpy(copy.get(), file, size, hipMemcpyDeviceToHost); e != hipSuccess) {
                        return j2p_fail(J2P_EDEVICE, "jpeg: reading the file: %s", hipGetErrorString(e));
                }
        }
        std::unique_ptr<j2p_jpeg_parsed> parsed(new(std::nothrow) j2p_jpeg_parsed);
        if(!parsed) { return j2p_fail(J2P_ENOMEM, "out of memory"); }
        if(const int rc = j2p_jpeg_parse_full(copy ? copy.get() : file, size, parsed.get()); rc != J2P_OK) { return rc; }
        opened->scan = file + parsed->info.scan_begin;
        opened->parsed = std::move(parsed);
        opened->on_device = kind == J2P_MEMORY_DEVICE;
        opened->device = opened->on_device ? where : -1;
        return J2P_OK;
}

int j2p_jpeg_open_scans(const uint8_t *file, size_t size, j2p_jpeg_file *opened)
{
        *opened = j2p_jpeg_file();
        if(!file || size == 0) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        int where = -1;
        const int kind = j2p_memory_of_pointer(file, &where);
        if(kind == J2P_MEMORY_OTHER) { return j2p_fail(J2P_EINVAL, "jpeg: the file lies in managed or unknown memory (plain device memory, or host memory)"); }
        std::unique_ptr<uint8_t[]> copy;
        if(kind == J2P_MEMORY_DEVICE) {
                copy.reset(new(std::nothrow) uint8_t[size]);
                if(!copy) { return j2p_fail(J2P_ENOMEM, "out of memory"); }
                if(const hipError_t e = hipMemcpy(copy.get(), file, size, hipMemcpyDeviceToHost); e != hipSuccess) {
                        return j2p_fail(J2P_EDEVICE, "jpeg: reading the file: %s", hipGetErrorString(e));
                }
        }
        std::unique_ptr<j2p_scans_parsed> scans(new(std::nothrow) j2p_scans_parsed);
        if(!scans) { return j2p_fail(J2P_ENOMEM, "out of memory"); }
        if(const int rc = j2p_jpeg_parse_scans_full(copy ? copy.get() : file, size, scans.get()); rc != J2P_OK) { return rc; }
        opened->scan = file + scans->base.info.scan_begin;
        opened->scans = std::move(scans);
        opened->on_device = kind == J2P_MEMORY_DEVICE;
        opened->device = opened->on_device ? where : -1;
        return J2P_OK;
}

// an opened file's decode into coef[] on `stream`: every scan of a progressive file, or the one scan of a sequential file
int j2p_decode_opened(int device, hipStream_t stream, const j2p_jpeg_file &file, unsigned S, int16_t *const coef[3], j2p_decode_stats *stats,
                      j2p_scans_stats *scans_stats)
{
        if(!file.scans) { return j2p_decode_file(device, stream, file.parsed.get(), file.scan, file.on_device, S, coef, stats); }
        if(file.scans->scans.progressive) { return j2p_decode_scans_file(device, stream, file.scans.get(), file.scan, file.on_device, S, coef, scans_stats); }
        j2p_decode_stats one;
        const int rc = j2p_decode_file(device, stream, &file.scans->base, file.scan, file.on_device, S, coef, &one);
        if(rc == J2P_OK && scans_stats) {
                memset(scans_stats, 0, sizeof(*scans_stats));
                scans_stats->scans = 1;
                scans_stats->subsequences = one.subsequences;
                scans_stats->rounds = one.rounds;
                scans_stats->data_bytes = one.data_bytes;
                scans_stats->decode_ms = one.decode_ms;
        }
        return rc;
}

j2p_decoded_grids::j2p_decoded_grids(int device, const j2p_jpeg_file &file, unsigned S, j2p_decode_stats *stats, j2p_scans_stats *scans_stats)
    : device_(device)
{
        rc = decode(file, S, stats, scans_stats);
}

int j2p_decoded_grids::decode(const j2p_jpeg_file &file, unsigned S, j2p_decode_stats *stats, j2p_scans_stats *scans_stats)
{
        const j2p_jpeg_info &f = file.info();
        j2p_carve part;
        for(unsigned c = 0; c < f.ncomp; c++) { at[c] = part(j2p_grid_bytes(f.comp[c].blocks_w, f.comp[c].blocks_h)); }
        bytes = part.total;
        HIP_TRY(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
        HIP_TRY(j2p_pool_take(device_, bytes, &block, &block_bytes_));
        for(unsigned c = 0; c < f.ncomp; c++) { coef[c] = reinterpret_cast<int16_t *>(static_cast<char *>(block) + at[c]); }
        return j2p_decode_opened(device_, stream_, file, S, coef, stats, scans_stats);
}

j2p_decoded_grids::~j2p_decoded_grids()
{
        if(stream_) {
                (void)hipStreamSynchronize(stream_);
                (void)hipStreamDestroy(stream_);
        }
        if(block) { j2p_pool_give(device_, block, block_bytes_); }
}

extern "C" {

int j2p_entropy_decode_ex(int device, const uint8_t *file, size_t size, int16_t *const coef_host[3], uint16_t quant[3][64], j2p_jpeg_info *info,
                          unsigned subsequence_bits, j2p_decode_stats *stats)
{
        if(!coef_host) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(subsequence_bits && (subsequence_bits < J2P_DECODE_SUBSEQUENCE_MIN || subsequence_bits > J2P_DECODE_SUBSEQUENCE_MAX)) {
                return j2p_fail(J2P_EINVAL, "decode: %u bits in a subsequence (%u..%u)", subsequence_bits, J2P_DECODE_SUBSEQUENCE_MIN, J2P_DECODE_SUBSEQUENCE_MAX);
        }
        j2p_jpeg_file opened;
        if(const int rc = j2p_jpeg_open(file, size, &opened); rc != J2P_OK) { return rc; }
        const j2p_jpeg_info &f = opened.parsed->info;
        for(unsigned c = 0; c < f.ncomp; c++) {
                if(!coef_host[c]) { return j2p_fail(J2P_EINVAL, "decode: component %u has no room for its coefficients", c); }
        }
        if(const int rc = check_device(device); rc != J2P_OK) { return rc; }
        if(opened.on_device && opened.device != device) {
                return j2p_fail(J2P_EINVAL, "jpeg: the file lies on device %d, the decode runs on %d", opened.device, device);
        }
        DeviceGuard guard(device);
        const j2p_decoded_grids grids(device, opened, subsequence_bits, stats);
        if(grids.rc != J2P_OK) { return grids.rc; }
        // one staging copy down, so that nothing reaches the caller's arrays unless all of it does
        const std::unique_ptr<char[]> staged(new(std::nothrow) char[grids.bytes]);
        if(!staged) { return j2p_fail(J2P_ENOMEM, "out of memory"); }
        if(const hipError_t e = hipMemcpy(staged.get(), grids.block, grids.bytes, hipMemcpyDeviceToHost); e != hipSuccess) {
                return j2p_fail(J2P_EDEVICE, "decode: %s", hipGetErrorString(e));
        }
        for(unsigned c = 0; c < f.ncomp; c++) {
                memcpy(coef_host[c], staged.get() + grids.at[c], j2p_grid_bytes(f.comp[c].blocks_w, f.comp[c].blocks_h));
                if(quant) { memcpy(quant[c], f.comp[c].quant, sizeof(f.comp[c].quant)); }
        }
        if(info) { *info = f; }
        return J2P_OK;
}

int j2p_entropy_decode_scans(int device, const uint8_t *file, size_t size, int16_t *const coef_host[3], uint16_t quant[3][64], j2p_jpeg_info *info,
                             unsigned subsequence_bits, j2p_scans_stats *stats)
{
        if(!coef_host) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(subsequence_bits && (subsequence_bits < J2P_DECODE_SUBSEQUENCE_MIN || subsequence_bits > J2P_DECODE_SUBSEQUENCE_MAX)) {
                return j2p_fail(J2P_EINVAL, "decode: %u bits in a subsequence (%u..%u)", subsequence_bits, J2P_DECODE_SUBSEQUENCE_MIN, J2P_DECODE_SUBSEQUENCE_MAX);
        }
        j2p_jpeg_file opened;
        if(const int rc = j2p_jpeg_open_scans(file, size, &opened); rc != J2P_OK) { return rc; }
        const j2p_jpeg_info &f = opened.info();
        for(unsigned c = 0; c < f.ncomp; c++) {
                if(!coef_host[c]) { return j2p_fail(J2P_EINVAL, "decode: component %u has no room for its coefficients", c); }
        }
        if(const int rc = check_device(device); rc != J2P_OK) { return rc; }
        if(opened.on_device && opened.device != device) {
                return j2p_fail(J2P_EINVAL, "jpeg: the file lies on device %d, the decode runs on %d", opened.device, device);
        }
        DeviceGuard guard(device);
        const j2p_decoded_grids grids(device, opened, subsequence_bits, nullptr, stats);
        if(grids.rc != J2P_OK) { return grids.rc; }
        const std::unique_ptr<char[]> staged(new(std::nothrow) char[grids.bytes]);
        if(!staged) { return j2p_fail(J2P_ENOMEM, "out of memory"); }
        if(const hipError_t e = hipMemcpy(staged.get(), grids.block, grids.bytes, hipMemcpyDeviceToHost); e != hipSuccess) {
                return j2p_fail(J2P_EDEVICE, "decode: %s", hipGetErrorString(e));
        }
        for(unsigned c = 0; c < f.ncomp; c++) {
                memcpy(coef_host[c], staged.get() + grids.at[c], j2p_grid_bytes(f.comp[c].blocks_w, f.comp[c].blocks_h));
                if(quant) { memcpy(quant[c], f.comp[c].quant, sizeof(f.comp[c].quant)); }
        }
        if(info) { *info = f; }
        return J2P_OK;
}

int j2p_entropy_decode(int device, const uint8_t *file, size_t size, int16_t *const coef_host[3], uint16_t quant[3][64], j2p_jpeg_info *info)
{
        return j2p_entropy_decode_ex(device, file, size, coef_host, quant, info, 0, nullptr);
}

}  // extern "C"

// ---- the PNG file: k_png_filter, k_png_count, the tables on the host (j2p_deflate.h), k_png_pack, k_png_chunks, k_png_crc ----
namespace {

// a chunk without data or with the 13 bytes of IHDR: length, type, data, CRC-32 of type and data
size_t png_chunk(const char type[4], const uint8_t *data, unsigned n, uint8_t *out)
{
        out[0] = out[1] = out[2] = 0;
        out[3] = (uint8_t)n;
        memcpy(out + 4, type, 4);
        if(n) { memcpy(out + 8, data, n); }
        const uint32_t crc = j2p_crc32(out + 4, 4 + n);
        for(int k = 0; k < 4; k++) { out[8 + n + k] = (uint8_t)(crc >> (24 - 8 * k)); }
        return 12 + (size_t)n;
}
constexpr size_t kPngHead = 8 + 25, kPngTail = 12;       // the signature and IHDR; IEND

}  // namespace

// The coder (j2p_internal.h: what memory and fill are).  The block's layout, each part aligned to 256 bytes:
//   [samples][stream: the filtered rows][chosen: 5 u32][counts: blocks x 288 u32][blocks: PngBlock each]    known from the spec
//   [stage: the zlib stream, ceil(bytes / 4) + 1 words][out: the IDAT chunks]                                known once the counts are
// The counts come down once (a wait), the tables are made on the host (j2p_deflate.h), and every size follows from them: the
// file's own is known — and J2P_ESPACE answered — before anything is packed.  The block is asked for twice, the first time with
// a guess for the second part (j2p_coder_block.h); its one stage makes the samples and the filtered rows, again when the block
// moved (the counts live on the host by then, and the blocks' records go up after the second request).  A second image of the
// same size or smaller finds the block large enough at once.
int j2p_png_write(hipStream_t stream, const j2p_png &spec, unsigned channels, const std::function<int(size_t, void **, bool *)> &memory,
                  const std::function<void(hipStream_t, uint8_t *)> &fill, uint8_t *out_host, size_t capacity, size_t *size, j2p_png_stats *stats)
{
        const unsigned bpp = channels * spec.bits / 8;
        const size_t rb = (size_t)spec.width * bpp, total = (size_t)spec.height * (rb + 1);
        const unsigned block_bytes = spec.block_bytes ? spec.block_bytes : J2P_PNG_BLOCK_BYTES;
        const unsigned idat_bytes = spec.idat_bytes ? spec.idat_bytes : J2P_PNG_IDAT_BYTES;
        const size_t nblocks = (total + block_bytes - 1) / block_bytes;
        if(nblocks > J2P_PNG_BLOCKS_MAX) {
                return j2p_fail(J2P_EINVAL, "png: %zu deflate blocks of %u bytes (at most %u: raise block_bytes)", nblocks, block_bytes, J2P_PNG_BLOCKS_MAX);
        }
        j2p_carve part;
        const size_t samples_at = part((size_t)spec.height * rb), stream_at = part(total), chosen_at = part(5 * 4);
        const size_t counts_at = part(nblocks * J2P_DEFLATE_COUNTS * 4), blocks_at = part(nblocks * sizeof(PngBlock));
        const size_t fixed = part.total;
        j2p_coder_block block(memory);
        // from the samples to the filtered rows
        const auto filter = [&] {
                fill(stream, block.at<uint8_t>(samples_at));
                (void)hipMemsetAsync(block.at(chosen_at), 0, 5 * 4, stream);
                hipLaunchKernelGGL(k_png_filter, dim3((spec.height + 3) / 4), dim3(256), 0, stream, static_cast<const uint8_t *>(block.at<uint8_t>(samples_at)), rb, spec.height,
                                   bpp, spec.filter < 0 ? 5u : (unsigned)spec.filter, block.at<uint8_t>(stream_at), block.at<unsigned>(chosen_at));
        };
        if(const int rc = block.grow(fixed + total / 2 + total / 4 + 4096); rc != J2P_OK) { return rc; }      // (a photograph's file: half to two thirds of its samples)
        block.stage(filter);
        hipLaunchKernelGGL(k_png_count, dim3((unsigned)nblocks), dim3(256), 0, stream, static_cast<const uint8_t *>(block.at<uint8_t>(stream_at)), total, block_bytes,
                           block.at<unsigned>(counts_at));
        HIP_TRY(hipGetLastError());
        std::vector<unsigned> counts;
        std::vector<PngBlock> blocks;
        try {
                counts.resize(nblocks * J2P_DEFLATE_COUNTS);
                blocks.resize(nblocks);
        } catch(const std::bad_alloc &) { return j2p_fail(J2P_ENOMEM, "out of memory"); }
        unsigned chosen[5] = {0, 0, 0, 0, 0};
        HIP_TRY(hipMemcpyAsync(counts.data(), block.at(counts_at), counts.size() * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(chosen, block.at(chosen_at), sizeof(chosen), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        // the tables, the blocks' places and the checksum
        j2p_png_stats st;
        memset(&st, 0, sizeof(st));
        for(int f = 0; f < 5; f++) { st.rows[f] = chosen[f]; }
        st.blocks = nblocks;
        uint32_t a = 1, b = 0;
        unsigned long long zlen = 2;
        {
                j2p_deflate_block made;
                for(size_t k = 0; k < nblocks; k++) {
                        const unsigned *c = counts.data() + k * J2P_DEFLATE_COUNTS;
                        const bool final = k + 1 == nblocks;
                        j2p_deflate_block_make(c, final, &made);
                        PngBlock &d = blocks[k];
                        d.offset = zlen;
                        d.header_bits = made.header_bits;
                        d.final = final;
                        memcpy(d.code, made.code, sizeof(d.code));
                        memcpy(d.header, made.header, sizeof(d.header));
                        zlen += made.bytes;
                        st.literals += made.literals;
                        st.matches += made.matches;
                        const size_t n = final ? total - k * (size_t)block_bytes : block_bytes;
                        j2p_deflate_adler_add(&a, &b, n, c[J2P_DEFLATE_SYMBOLS], c[J2P_DEFLATE_SYMBOLS + 1]);
                }
        }
        zlen += 4;
        st.adler = (b << 16) | a;
        st.stream_bytes = zlen;
        if(stats) { *stats = st; }
        const unsigned long long nchunks = (zlen + idat_bytes - 1) / idat_bytes;
        const size_t data_bytes = (size_t)(zlen + 12 * nchunks);
        *size = kPngHead + data_bytes + kPngTail;
        if(capacity < *size || !out_host) { return j2p_fail(J2P_ESPACE, "png: the file has %zu bytes, the buffer %zu", *size, out_host ? capacity : 0); }
        if(nchunks > 0x7fffffffull) { return j2p_fail(J2P_EINVAL, "png: %llu IDAT chunks of %u bytes are too many", nchunks, idat_bytes); }
        const size_t stage_words = (size_t)((zlen + 3) / 4) + 1;
        const size_t stage_at = part(stage_words * 4), out_at = part(data_bytes);
        if(const int rc = block.grow(part.total); rc != J2P_OK) { return rc; }
        HIP_TRY(hipMemcpyAsync(block.at(blocks_at), blocks.data(), nblocks * sizeof(PngBlock), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(block.at(stage_at), 0, stage_words * 4, stream));
        hipLaunchKernelGGL(k_png_pack, dim3((unsigned)nblocks), dim3(256), 0, stream, static_cast<const uint8_t *>(block.at<uint8_t>(stream_at)), total, block_bytes,
                           reinterpret_cast<const PngBlock *>(block.at(blocks_at)), st.adler, block.at<unsigned>(stage_at));
        hipLaunchKernelGGL(k_png_chunks, dim3((unsigned)((zlen + 1023) / 1024)), dim3(256), 0, stream, static_cast<const uint8_t *>(block.at<uint8_t>(stage_at)), (size_t)zlen,
                           idat_bytes, block.at<uint8_t>(out_at));
        hipLaunchKernelGGL(k_png_crc, dim3((unsigned)((nchunks + 63) / 64)), dim3(64), 0, stream, block.at<uint8_t>(out_at), (size_t)zlen, idat_bytes, (unsigned)nchunks);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out_host + kPngHead, block.at(out_at), data_bytes, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        static const uint8_t signature[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
        memcpy(out_host, signature, 8);
        uint8_t ihdr[13];
        for(int k = 0; k < 4; k++) {
                ihdr[k] = (uint8_t)(spec.width >> (24 - 8 * k));
                ihdr[4 + k] = (uint8_t)(spec.height >> (24 - 8 * k));
        }
        ihdr[8] = (uint8_t)spec.bits;
        ihdr[9] = channels == 3 ? 2 : 0;
        ihdr[10] = ihdr[11] = ihdr[12] = 0;
        (void)png_chunk("IHDR", ihdr, 13, out_host + 8);
        (void)png_chunk("IEND", nullptr, 0, out_host + kPngHead + data_bytes);
        return J2P_OK;
}

extern "C" {

int j2p_png_encode(int device, const j2p_png *spec, const uint8_t *samples_host, unsigned channels, uint8_t *out_host, size_t capacity, size_t *size,
                   j2p_png_stats *stats)
{
        if(!samples_host || !size) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(const char *why = j2p_png_error(spec, channels)) { return j2p_fail(J2P_EINVAL, "%s", why); }
        if(const int rc = check_device(device); rc != J2P_OK) { return rc; }
        DeviceGuard guard(device);
        PooledCall call(device);
        if(const int rc = call.open(); rc != J2P_OK) { return rc; }
        const size_t sample_bytes = (size_t)spec->width * spec->height * channels * (spec->bits / 8);
        return j2p_png_write(
                call.stream, *spec, channels, std::ref(call),
                [&](hipStream_t st, uint8_t *samples) { (void)hipMemcpyAsync(samples, samples_host, sample_bytes, hipMemcpyHostToDevice, st); }, out_host, capacity,
                size, stats);
}

}  // extern "C"
